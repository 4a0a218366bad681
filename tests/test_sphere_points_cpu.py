"""S-PSNR-NN / S-PSNR-I / CPP-PSNR (sphere_points.py, pseudo_codec --test --sphere) without a GPU: the point sets, the
records, the torch twins on their exact cases, the summation bound, and the command line on the oracle backend."""
import math
import re

import numpy as np
import pytest
import torch

import sphere_points_cases as K
from pseudocylindrical_convolution_amd import sphere_points as SP
from pseudocylindrical_convolution_amd._native import PconvError


@pytest.mark.parametrize("level", range(5))
def test_icosphere_points(level):
    v = SP.icosphere_vertices(level)
    count = 10 * 4 ** level + 2
    assert v.shape == (count, 3) and v.dtype == np.float64
    assert np.abs(np.sqrt((v * v).sum(axis=1)) - 1).max() <= 4e-16
    assert any((v == (0, 0, 1)).all(axis=1)) and any((v == (0, 0, -1)).all(axis=1))
    assert np.unique(v, axis=0).shape[0] == count
    # no two points closer than a third of the edge length of this level
    edge = 2 * math.sin(math.atan(2) / 2) / 2 ** level
    d2 = 2 - 2 * (v @ v.T) + 8 * np.eye(count)                 # |a - b|^2 of unit vectors
    assert d2.min() > (edge / 3) ** 2
    pts = SP.icosphere(level)
    assert pts.shape == (count, 2) and np.abs(pts[:, 0]).max() <= np.pi and np.abs(pts[:, 1]).max() <= np.pi / 2
    assert pts[0].tolist() == [0.0, np.pi / 2] and (pts == (0.0, -np.pi / 2)).all(axis=1).sum() == 1
    back = np.stack([np.cos(pts[:, 1]) * np.cos(pts[:, 0]), np.cos(pts[:, 1]) * np.sin(pts[:, 0]), np.sin(pts[:, 1])], axis=1)
    assert np.abs(back - v).max() <= 1e-15
    assert len(SP.PointSet(pts)) == count


def test_icosphere_default_is_the_size_of_the_standard_file():
    assert SP.LEVEL == 8 and 10 * 4 ** SP.LEVEL + 2 == 655362
    with pytest.raises(PconvError):
        SP.icosphere(-1)


@pytest.mark.parametrize("h,w", [(8, 16), (50, 100), (48, 130)])
def test_cpp_grid_keeps_the_valid_pixels(h, w):
    pts = SP.cpp_grid(h, w)
    kept = []
    for j in range(h):
        p = 3 * math.asin((0.5 - (j + 0.5) / h) * math.pi / math.pi)
        for i in range(w):
            t = ((i + 0.5) / w - 0.5) * (2 * math.pi) / (2 * math.cos(2 * p / 3) - 1)
            if abs(t) <= math.pi:
                kept.append((t, p))
    assert pts.shape == (len(kept), 2)
    # row-major, the same pixels.  A kept pixel has 2 cos(2p/3) - 1 >= |X| / pi >= 1 / w, so an ulp of difference between
    # two cosine routines is amplified by at most 2 w in t, |t| <= pi
    assert np.abs(pts - np.array(kept)).max() <= 4 * w * 2.0 ** -52 * math.pi
    share = len(kept) / float(h * w)
    assert 0.6 < share < 0.72
    rows = np.unique(pts[:, 1])
    assert rows.size == h                                      # every row keeps pixels


def test_load_points_round_trip(tmp_path):
    g = np.random.default_rng(3)
    lat, lon = g.uniform(-90, 90, 40), g.uniform(-180, 180, 40)
    lat[:2], lon[:2] = (90.0, -90.0), (180.0, -180.0)
    want = np.stack([np.radians(lon), np.radians(lat)], axis=1)
    for order, cols in (("latlon", (lat, lon)), ("lonlat", (lon, lat))):
        for count in (False, True):
            path = tmp_path / ("%s_%d.txt" % (order, count))
            with open(path, "w") as f:
                if count:
                    f.write("%d\n" % lat.size)
                for a, b in zip(*cols):
                    f.write("%r %r\n" % (float(a), float(b)))
            got = SP.load_points(str(path), order)
            assert got.dtype == np.float64 and np.array_equal(got, want)
            SP.PointSet(got)
    path = tmp_path / "wrapped.txt"
    path.write_text("2\n10 350\n-10 190.5\n")
    assert np.array_equal(SP.load_points(str(path)), np.stack([np.radians([-10.0, -169.5]), np.radians([10.0, -10.0])], axis=1))
    path.write_text("3\n10 350\n-10 190.5\n")
    with pytest.raises(PconvError):
        SP.load_points(str(path))
    path.write_text("91 0\n")
    with pytest.raises(PconvError):
        SP.load_points(str(path))
    with pytest.raises(PconvError):
        SP.load_points(str(path), "xy")


def test_point_sets_are_checked():
    for bad in (np.zeros((0, 2)), np.zeros((3, 3)), np.array([[3.2, 0.0]]), np.array([[0.0, 1.6]]), np.array([[np.nan, 0.0]])):
        with pytest.raises(PconvError):
            SP.PointSet(bad)
    ps = K.pointset("ico2")
    with pytest.raises(ValueError):
        ps.points[0, 0] = 1.0
    assert ps.records(8, 16) is ps.records(8, 16)              # cached
    for size in ((1, 16), (8, 1 << 21), (1 << 15, 1 << 15)):
        with pytest.raises(PconvError):
            ps.records(*size)


def _centres(h, w):
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([(((i + 0.5) / w - 0.5) * (2 * np.pi)).ravel(), ((0.5 - (j + 0.5) / h) * np.pi).ravel()], axis=1), j, i


@pytest.mark.parametrize("h,w", K.SIZES)
def test_records_of_pixel_centres(h, w):
    pts, j, i = _centres(h, w)
    rec = SP.records_numpy(pts, h, w)
    assert rec.dtype == np.int32 and rec.shape == (h * w, 2)
    assert np.array_equal(rec[:, 0], 256 * i.ravel()) and np.array_equal(rec[:, 1], 256 * j.ravel())


def test_records_of_the_handmade_set():
    h, w = K.HAND_SIZE
    rec = SP.records_numpy(K.handmade(), h, w)
    assert rec[0].tolist() == [w * 128 - 128, -128] and rec[1].tolist() == [w * 128 - 128, h * 256 - 128]      # the poles
    assert rec[2, 0] == w * 256 - 128 and rec[3, 0] == w * 256 - 128                              # t = pi and t = -pi
    assert set((rec[8:, 0] % 256).tolist()) == {0, 128, 255} and set((rec[8:, 1] % 256).tolist()) == {0, 128, 255}
    assert torch.equal(SP.records(K.pointset("hand"), h, w), torch.from_numpy(rec))
    for size in K.SIZES:
        r = SP.records_numpy(K.handmade(), *size)
        assert r[:, 0].min() >= 0 and r[:, 0].max() < size[1] * 256


@pytest.mark.parametrize("h,w", K.SIZES)
@pytest.mark.parametrize("interp", K.INTERPS)
def test_sampling_the_own_pixel_centres_returns_the_picture(h, w, interp):
    x = K.picture(2, 3, h, w, 1)
    ps = SP.PointSet(_centres(h, w)[0])
    out = SP.sample_torch(x, ps.records(h, w), interp)
    assert out.dtype == torch.float32 and torch.equal(out, x.reshape(2, 3, h * w))
    assert torch.equal(SP.sample(x, ps, interp), out)          # CPU tensors run the twin
    u8 = (x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(SP.sample(u8, ps, interp), (u8.permute(0, 3, 1, 2).float() / 255.).reshape(2, 3, h * w))


@pytest.mark.parametrize("interp", K.INTERPS)
def test_nearest_and_lanczos_at_the_poles_and_the_seam(interp):
    """the hand-made set on (6, 4): every sample is a finite value; in nearest mode it is the pixel the rule names"""
    h, w = 6, 4
    x = K.picture(1, 1, h, w, 2)
    rec = SP.records(K.pointset("hand"), h, w)
    out = SP.sample_torch(x, rec, interp)
    assert out.shape == (1, 1, len(K.pointset("hand"))) and torch.isfinite(out).all()
    if interp == "nearest":
        for k, (qu, qv) in enumerate(rec.tolist()):
            c, r = ((qu + 128) // 256) % w, (qv + 128) // 256
            if r < 0 or r >= h:
                r, c = (-1 - r if r < 0 else 2 * h - 1 - r), (c + w // 2) % w
            assert out[0, 0, k] == x[0, 0, min(max(r, 0), h - 1), c]


@pytest.mark.parametrize("name", K.POINTSETS)
@pytest.mark.parametrize("interp", K.INTERPS)
def test_mse_exact_cases(name, interp):
    ps = K.pointset(name)
    for (h, w), (n, c) in zip(K.SIZES, K.BATCHES):
        x = K.picture(n, c, h, w, 3)
        zero = SP.mse_torch(x, x, ps, interp)
        assert zero.dtype == torch.float64 and zero.shape == (n, c) and zero.device.type == "cpu"
        assert torch.equal(zero, torch.zeros(n, c, dtype=torch.float64))
        assert torch.equal(SP.mse(x, x.clone(), ps, interp), zero)
    if interp == "nearest":
        g = torch.Generator().manual_seed(4)
        x = torch.randint(0, 129, (2, 3, 50, 100), generator=g).float() / 256.
        assert torch.equal(SP.mse_torch(x, x + 0.25, ps, interp), torch.full((2, 3), 0.0625, dtype=torch.float64))
        for (a, b) in K.PAIRS:       # constant pictures of different sizes
            assert torch.equal(SP.mse_torch(torch.full((1, 3) + a, 0.3), torch.full((1, 3) + b, 0.3), ps, interp),
                               torch.zeros(1, 3, dtype=torch.float64))


@pytest.mark.parametrize("name", K.POINTSETS)
@pytest.mark.parametrize("interp", K.INTERPS)
def test_mse_sum_against_fsum(name, interp):
    """all terms are non-negative, so any order of the float64 sum is within (P - 1) 2^-53 relative of the exact sum;
    twice that is asserted, on same-size and cross-size pairs"""
    ps = K.pointset(name)
    count = len(ps)
    for a, b in K.PAIRS + [(s, s) for s in K.SIZES[:2]]:
        x, y = K.picture(1, 2, a[0], a[1], 5), K.picture(1, 2, b[0], b[1], 6)
        got = SP.mse_torch(x, y, ps, interp)
        d = SP.sample_torch(x, ps.records(*a), interp) - SP.sample_torch(y, ps.records(*b), interp)
        e = (d * d).double()
        for c in range(2):
            exact = math.fsum(e[0, c].tolist()) / count
            assert exact > 0 and abs(got[0, c].item() - exact) <= K.sum_bound(count) * exact


def test_figures_and_refusals():
    x, y = K.picture(2, 3, 24, 48, 7), K.picture(2, 3, 50, 100, 8)
    ps4 = SP.icosphere_set(4)
    assert SP.icosphere_set(4) is ps4 and len(ps4) == 2562
    for fig, want in ((SP.s_psnr_nn(x, y, level=4), SP.mse_torch(x, y, ps4, "nearest")),
                      (SP.s_psnr_i(x, y, level=4), SP.mse_torch(x, y, ps4, "lanczos")),
                      (SP.cpp_psnr(x, y), SP.mse_torch(x, y, SP.cpp_set(24, 48), "lanczos")),
                      (SP.cpp_psnr(x, y, size=(50, 100)), SP.mse_torch(x, y, SP.cpp_set(50, 100), "lanczos"))):
        assert fig.dtype == torch.float64 and fig.shape == (2,)
        assert torch.equal(fig, 10 * torch.log10(1. / want.mean(dim=1)))
    assert SP.s_psnr_nn(x, x, level=2).tolist() == [math.inf, math.inf]
    with pytest.raises(PconvError):
        SP.mse(x, y[:1], ps4)
    with pytest.raises(PconvError):
        SP.mse(x, y[:, :2], ps4)
    with pytest.raises(PconvError):
        SP.mse(x, y, ps4, "bilinear")
    with pytest.raises(PconvError):
        SP.sample(x.double(), ps4)
    with pytest.raises(PconvError):
        SP.sample_torch(x, ps4.records(24, 48).long())


def test_gpu_tensor_without_the_ops_is_refused(oracle_backend, monkeypatch):
    """a GPU tensor on a backend without the kernels raises (no quiet torch path); no device is needed to see it"""
    class OnGpu(object):
        is_cuda = True
        dtype = torch.float32
        shape = (1, 1, 8, 16)
        device = torch.device("cuda:0")

        def dim(self):
            return 4

    ps = K.pointset("ico2")
    monkeypatch.setitem(ps._records, (8, 16, "cuda:0"), torch.zeros(len(ps), 2, dtype=torch.int32))
    for call in (lambda: SP.sample(OnGpu(), ps), lambda: SP.mse(OnGpu(), OnGpu(), ps)):
        with pytest.raises(PconvError, match="active backend has no sphere_points"):
            call()
    monkeypatch.delitem(ps._records, (8, 16, "cuda:0"))
    with pytest.raises(PconvError, match="active backend has no sphere_points_records"):
        ps.records(8, 16, "cuda:0")


def test_cli_sphere_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    """--enc --code-size --container of a 256 x 512 PNG; --test --sphere adds its two lines per image and for the
    average and leaves every other line alone; the refusals"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cpu")
    h, w = 256, 512
    _write_png("src.png", h, w, 4)
    common = ["--ssim", "--model-idx", "3"]
    PC.main(["--enc", "--code-size", "384x192", "--container", "--img-list", "src.png", "--code-list", "src.pcv"] + common)
    capsys.readouterr()
    test = ["--test", "--code-list", "src.pcv", "--img-list", "src.png"]
    PC.main(test)
    plain = capsys.readouterr().out.splitlines()
    PC.main(test + ["--sphere"])
    lines = capsys.readouterr().out.splitlines()
    assert not any("S-PSNR" in l for l in plain)
    assert [l for l in lines if "S-PSNR" not in l] == plain
    fig = r"S-PSNR-NN:([0-9.]+)dB, S-PSNR-I:([0-9.]+)dB, CPP-PSNR:([0-9.]+)dB"
    extra = [l for l in lines if "S-PSNR" in l]
    assert [bool(re.fullmatch(" ?" + fig + r"( \(coded size\))?", l)) for l in extra] == [True] * 4
    assert [l.startswith(" ") for l in extra] == [True, True, False, False]
    assert [l.endswith("(coded size)") for l in extra] == [False, True, False, True]
    assert extra[0].strip() == extra[2] and extra[1].strip() == extra[3] and extra[0] + " (coded size)" != extra[1]
    # the figures are sphere_points' own of the tensors the command line holds
    t2 = PC.PseudoDecoder(56, 0)
    PC.load_models(t2, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    rec, geometry = t2.decode_coded("src.pcv", None, None, raw=False)
    src = PC.img2tensor(PC.read_image("src.png"), "cpu")
    small = geometry.from_coded(rec, to_source=False)
    assert tuple(small.shape[2:]) == (192, 384)
    for line, y in ((extra[0], geometry.from_coded(rec)), (extra[1], small)):
        want = (SP.s_psnr_nn(src, y)[0].item(), SP.s_psnr_i(src, y)[0].item(), SP.cpp_psnr(src, y)[0].item())
        assert re.search(fig, line).groups() == tuple("%.2f" % v for v in want) and all(0 < v < 100 for v in want)    # (a seeded random model: a few dB)
    rows = PC.decoding_and_test(["src.pcv"], ["src.png"], 3, False, 0, sphere=True)
    assert len(rows) == 1 and len(rows[0]) == 9 and all(np.isfinite(v) for v in rows[0])
    capsys.readouterr()
    for argv in (["--dec", "--code-list", "src.pcv", "--out-list", "y.png", "--sphere"],
                 ["--enc", "--img-list", "src.png", "--code-list", "x.bin", "--sphere"] + common,
                 ["--test", "--code-list", "src.pcv", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "yuv420p", "--sphere"]):
        with pytest.raises(SystemExit):
            PC.main(argv)
        assert "--sphere" in capsys.readouterr().err, argv
