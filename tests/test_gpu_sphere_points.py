"""S-PSNR-NN / S-PSNR-I / CPP-PSNR on the GPU (csrc/sphere_points.hip): the records equal the host's, the sampler equals
its torch twin bit for bit, the fused MSE lies within the summation bound of the twin and does not depend on the batch,
the host refuses bad arguments before any launch, and the command line prints both lines."""
import math
import re

import pytest
import torch

import sphere_points_cases as K
from pseudocylindrical_convolution_amd import sphere_points as SP
from pseudocylindrical_convolution_amd._native import PconvError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_SIZES = K.SIZES + [(24, 48)]      # (24, 48): the small side of a cross-size pair


@pytest.mark.parametrize("name", K.POINTSETS)
def test_records_equal_the_host(hip_backend, name):
    ps = K.pointset(name)
    for h, w in ALL_SIZES:
        rec = SP.records(ps, h, w, DEV)
        assert rec.is_cuda and rec.dtype == torch.int32 and tuple(rec.shape) == (len(ps), 2)
        assert torch.equal(rec.cpu(), torch.from_numpy(SP.records_numpy(ps, h, w)))
        assert SP.records(ps, h, w, DEV) is rec


@pytest.mark.parametrize("h,w", K.SIZES)
@pytest.mark.parametrize("interp", K.INTERPS)
def test_sample_equals_the_twin_bit_for_bit(hip_backend, h, w, interp):
    for name in K.POINTSETS:
        ps = K.pointset(name)
        for n, c in ((1, 1), (3, 3)):
            x = K.picture(n, c, h, w, 11)
            rec = SP.records(ps, h, w, DEV)
            got = SP.sample(x.to(DEV), ps, interp)
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, c, len(ps))
            assert torch.equal(got.cpu(), SP.sample_torch(x, rec.cpu(), interp)), (name, n, c)
    # the op on records of its own, and into out=
    rec = SP.records(K.pointset("hand"), h, w, DEV)
    x = K.picture(2, 3, h, w, 12).to(DEV)
    out = torch.full((2, 3, rec.shape[0]), -1.0, device=DEV)
    assert hip_backend.sphere_points_sample_f32(x, rec, interp, out) is out
    assert torch.equal(out, SP.sample_torch(x, rec, interp))


def _pairs():
    return K.PAIRS + [(s, s) for s in K.SIZES]


@pytest.mark.parametrize("name", K.POINTSETS)
@pytest.mark.parametrize("interp", K.INTERPS)
def test_mse_within_the_summation_bound_of_the_twin(hip_backend, name, interp):
    ps = K.pointset(name)
    bound = K.sum_bound(len(ps))
    for a, b in _pairs():
        for n, c in ((1, 1), (3, 3)):
            x, y = K.picture(n, c, a[0], a[1], 13), K.picture(n, c, b[0], b[1], 14)
            got = SP.mse(x.to(DEV), y.to(DEV), ps, interp)
            want = SP.mse_torch(x, y, ps, interp)
            assert got.dtype == torch.float64 and got.device.type == "cpu" and tuple(got.shape) == (n, c)
            rel = ((got - want).abs() / want).max().item()
            print("mse %s %s %s/%s n%d C%d: relative difference %.3g, bound %.3g" % (name, interp, a, b, n, c, rel, bound))
            assert (want > 0).all() and rel <= bound, (a, b, n, c)
            zero = SP.mse(x.to(DEV), x.to(DEV), ps, interp)
            assert torch.equal(zero, torch.zeros(n, c, dtype=torch.float64))
            xd = x.to(DEV)
            assert torch.equal(SP.mse(xd, xd, ps, interp), zero)       # x == y, the same tensor, is allowed


@pytest.mark.parametrize("interp", K.INTERPS)
def test_a_frame_gives_the_same_bits_anywhere(hip_backend, interp):
    for name in ("ico4", "cpp50x100", "ico2"):
        ps = K.pointset(name)
        for a, b in K.PAIRS + [((48, 130), (48, 130))]:
            x, y = K.picture(3, 3, a[0], a[1], 15).to(DEV), K.picture(3, 3, b[0], b[1], 16).to(DEV)
            whole = SP.mse(x, y, ps, interp)
            assert torch.equal(SP.mse(x, y, ps, interp), whole)                      # a second call
            for f in range(3):
                assert torch.equal(SP.mse(x[f:f + 1], y[f:f + 1], ps, interp)[0], whole[f])          # alone
            order = [2, 0, 1]
            assert torch.equal(SP.mse(x[order].contiguous(), y[order].contiguous(), ps, interp), whole[order])
            # a channel alone: the planes do not depend on each other either
            assert torch.equal(SP.mse(x[:, 1:2].contiguous(), y[:, 1:2].contiguous(), ps, interp)[:, 0], whole[:, 1])


def test_uint8_frames_and_exact_cases(hip_backend):
    ps = K.pointset("ico4")
    g = torch.Generator().manual_seed(17)
    x = torch.randint(0, 129, (2, 3, 50, 100), generator=g).float() / 256.
    assert torch.equal(SP.mse(x.to(DEV), (x + 0.25).to(DEV), ps, "nearest"), torch.full((2, 3), 0.0625, dtype=torch.float64))
    a, b = torch.full((1, 3, 50, 100), 0.3, device=DEV), torch.full((1, 3, 24, 48), 0.3, device=DEV)
    assert torch.equal(SP.mse(a, b, ps, "nearest"), torch.zeros(1, 3, dtype=torch.float64))
    u, v = (torch.randint(0, 256, (2, 24, 48, 3), generator=g, dtype=torch.uint8) for _ in range(2))
    for interp in K.INTERPS:
        got, want = SP.mse(u.to(DEV), v.to(DEV), ps, interp), SP.mse_torch(u, v, ps, interp)
        assert ((got - want).abs() / want).max().item() <= K.sum_bound(len(ps))


def test_refusals_come_from_the_host(hip_backend):
    """every refusal of include/pconv_hip.h is raised before any launch: the pointers below are never dereferenced"""
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    d = 1 << 20          # an aligned dummy address
    big = 1 << 28

    def refused(rc, *words):
        err = lib.pconv_last_error()
        assert rc == -1 and all(w in err for w in words), (rc, err, words)

    # records(points, records, P, h, w, stream)
    R = lib.pconv_sphere_points_records
    refused(R(None, d, 10, 8, 16, None), b"sphere_points_records", b"null")
    refused(R(d, None, 10, 8, 16, None), b"null")
    refused(R(d + 4, 4 * d, 10, 8, 16, None), b"aligned")
    refused(R(d, 4 * d + 4, 10, 8, 16, None), b"aligned")
    refused(R(d, 4 * d, 0, 8, 16, None), b"2^28 - 1")
    refused(R(d, 4 * d, big, 8, 16, None), b"2^28 - 1")
    refused(R(d, 4 * d, 10, 1, 16, None), b"outside 2 .. 2^20")
    refused(R(d, 4 * d, 10, 8, (1 << 20) + 1, None), b"outside 2 .. 2^20")
    refused(R(d, 4 * d, 10, 1 << 15, 1 << 14, None), b"2^31 bytes")
    # sample(in, out, records, phases, n, c, h, w, P, mode, stream)
    S = lib.pconv_sphere_points_sample_f32
    ok = [d, 64 * d, 2 * d, 3 * d, 1, 3, 8, 16, 10, 0, None]

    def with_(args, **kw):
        names = ["a0", "a1", "a2", "a3", "n", "c", "h", "w", "P", "mode"]
        args = list(args)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args

    for kw, words in (({"a0": None}, (b"sphere_points_sample_f32", b"null")), ({"a1": None}, (b"null",)), ({"a2": None}, (b"null",)),
                      ({"a3": None}, (b"null",)), ({"a0": d + 2}, (b"aligned",)), ({"a1": 64 * d + 1}, (b"aligned",)),
                      ({"a2": 2 * d + 4}, (b"aligned",)), ({"a3": 3 * d + 2}, (b"aligned",)), ({"n": 0}, (b"planes",)),
                      ({"c": 0}, (b"planes",)), ({"n": 256, "c": 256}, (b"planes",)), ({"h": 1}, (b"outside 2 .. 2^20",)),
                      ({"w": 1 << 21}, (b"outside 2 .. 2^20",)), ({"h": 1 << 15, "w": 1 << 14}, (b"2^31 bytes",)),
                      ({"P": 0}, (b"2^28 - 1",)), ({"P": big}, (b"2^28 - 1",)), ({"mode": 2}, (b"unknown mode",)),
                      ({"mode": -1}, (b"unknown mode",)), ({"a1": d}, (b"distinct",))):
        refused(S(*with_(ok, **kw)), *words)
    # workspace_bytes(n, c, P)
    W = lib.pconv_sphere_points_mse_workspace_bytes
    assert W(2, 3, 2562) == 2 * 3 * 3 * 8 and W(1, 1, 1024) == 8 and W(1, 1, 1025) == 16
    for args in ((0, 1, 10), (1, 0, 10), (256, 256, 10), (1, 1, 0), (1, 1, big)):
        assert W(*args) < 0 and b"sphere_points_mse_workspace_bytes" in lib.pconv_last_error()
    # mse(x, h1, w1, rec_x, y, h2, w2, rec_y, phases, n, c, P, mode, workspace, out, stream)
    M = lib.pconv_sphere_points_mse_f32
    ok = [d, 8, 16, 2 * d, 3 * d, 6, 4, 4 * d, 5 * d, 1, 3, 10, 0, 6 * d, 7 * d, None]
    names = ["x", "h1", "w1", "rx", "y", "h2", "w2", "ry", "ph", "n", "c", "P", "mode", "ws", "out"]
    for kw, words in ([({k: None}, (b"sphere_points_mse_f32", b"null")) for k in ("x", "rx", "y", "ry", "ph", "ws", "out")]
                      + [({k: ok[names.index(k)] + off}, (b"aligned",)) for k, off in
                         (("x", 2), ("y", 1), ("ph", 2), ("rx", 4), ("ry", 4), ("ws", 4), ("out", 4))]
                      + [({"h1": 1}, (b"outside 2 .. 2^20",)), ({"w2": 1 << 21}, (b"outside 2 .. 2^20",)),
                         ({"h2": 1 << 15, "w2": 1 << 14}, (b"2^31 bytes",)), ({"n": 0}, (b"planes",)), ({"c": 65536}, (b"planes",)),
                         ({"P": 0}, (b"2^28 - 1",)), ({"P": big}, (b"2^28 - 1",)), ({"mode": 7}, (b"unknown mode",)),
                         ({"out": d}, (b"alias",)), ({"out": 3 * d + 8}, (b"alias",)), ({"ws": d + 64}, (b"alias",)),
                         ({"ws": 7 * d}, (b"alias",))]):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        refused(M(*args), *words)
    # ... and through the Python surface, before anything reaches the library
    x = torch.zeros(1, 1, 8, 16, device=DEV)
    rec = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    for call in (lambda: hip_backend.sphere_points_sample_f32(x, rec, "cubic"), lambda: hip_backend.sphere_points_sample_f32(x, rec.long()),
                 lambda: hip_backend.sphere_points_sample_f32(x.cpu(), rec), lambda: hip_backend.sphere_points_sample_f32(x, rec.cpu()),
                 lambda: hip_backend.sphere_points_mse(x, rec, x, rec[:3].contiguous()),
                 lambda: hip_backend.sphere_points_mse(x, rec, torch.zeros(2, 1, 8, 16, device=DEV), rec),
                 lambda: hip_backend.sphere_points_records(torch.zeros(4, 2, device=DEV), 8, 16),
                 lambda: hip_backend.sphere_points_records(torch.zeros(4, 2, dtype=torch.float64, device=DEV), 1, 16)):
        with pytest.raises(PconvError):
            call()


def test_any_record_content_stays_inside_the_picture(hip_backend):
    """records are data: whatever they hold is reduced to a position inside the frame, as in the twin"""
    h, w = 6, 4
    x = K.picture(1, 2, h, w, 18)
    big = 2 ** 31 - 1
    rec = torch.tensor([[big, big], [-big - 1, -big - 1], [big, -big - 1], [-1, -1], [w * 256, h * 256], [-129, h * 256 + 127],
                        [123456789, -987654321]], dtype=torch.int32)
    for interp in K.INTERPS:
        got = hip_backend.sphere_points_sample_f32(x.to(DEV), rec.to(DEV), interp)
        assert torch.equal(got.cpu(), SP.sample_torch(x, rec, interp))


def test_the_figures_equal_those_composed_from_sample(hip_backend):
    """the bound of the sums in dB: d(10 log10 m) = (10 / ln 10) dm / m, plus the roundings of the two logarithms"""
    x, y = K.picture(2, 3, 50, 100, 19).to(DEV), K.picture(2, 3, 24, 48, 20).to(DEV)

    def composed(ps, interp):
        d = SP.sample(x, ps, interp) - SP.sample(y, ps, interp)
        return SP.psnr_of(((d * d).double().sum(dim=2) / len(ps)).cpu())

    for got, ps, interp in ((SP.s_psnr_nn(x, y, level=4), SP.icosphere_set(4), "nearest"),
                            (SP.s_psnr_i(x, y, level=4), SP.icosphere_set(4), "lanczos"),
                            (SP.s_psnr_nn(x, y), SP.icosphere_set(8), "nearest"),
                            (SP.s_psnr_i(x, y), SP.icosphere_set(8), "lanczos"),
                            (SP.cpp_psnr(x, y), SP.cpp_set(50, 100), "lanczos"),
                            (SP.cpp_psnr(x, y, size=(24, 48)), SP.cpp_set(24, 48), "lanczos")):
        want = composed(ps, interp)
        tol = 10 / math.log(10) * K.sum_bound(len(ps)) + 2 * want.abs().max().item() * 2.0 ** -52
        print("%s P%d: %s vs %s, tolerance %.3g dB" % (interp, len(ps), got.tolist(), want.tolist(), tol))
        assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and torch.isfinite(got).all()
        assert (got - want).abs().max().item() <= tol
    assert len(SP.icosphere_set(8)) == 655362


def test_cli_sphere_on_the_gpu(hip_backend, tmp_path, monkeypatch, capsys):
    """--rd --sphere --code-size on a 256 x 512 image: both lines, finite, and the coded-size line differs"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, DEV)
    _write_png("img.png", 256, 512, 0)
    common = ["--ssim", "--model-idx", "3", "--img-list", "img.png"]
    PC.main(["--rd", "--code-size", "384x192"] + common)
    plain = capsys.readouterr().out.splitlines()
    PC.main(["--rd", "--sphere", "--code-size", "384x192"] + common)
    lines = capsys.readouterr().out.splitlines()
    assert [l for l in lines if "S-PSNR" not in l] == plain and not any("S-PSNR" in l for l in plain)
    fig = r"S-PSNR-NN:([0-9.]+)dB, S-PSNR-I:([0-9.]+)dB, CPP-PSNR:([0-9.]+)dB"
    extra = [l for l in lines if "S-PSNR" in l]
    assert len(extra) == 4 and [l.endswith(" (coded size)") for l in extra] == [False, True, False, True]
    values = [[float(v) for v in re.fullmatch(" ?" + fig + r"( \(coded size\))?", l).groups()[:3]] for l in extra]
    assert all(math.isfinite(v) and v > 0 for row in values for v in row)
    rows = PC.rate_distortion(["img.png"], 3, False, 0, code_size=(192, 384), sphere=True)
    assert len(rows[0]) == 9 and all(math.isfinite(v) for v in rows[0])
    assert tuple(rows[0][3:6]) != tuple(rows[0][6:9])           # the coded-size figures are another measurement
    assert ["%.2f" % v for v in rows[0][3:6]] == ["%.2f" % v for v in values[0]]
    assert ["%.2f" % v for v in rows[0][6:9]] == ["%.2f" % v for v in values[1]]
    # a size that is not resized has no second line
    capsys.readouterr()
    PC.main(["--rd", "--sphere", "--height", "256", "--width", "512"] + common)
    assert len([l for l in capsys.readouterr().out.splitlines() if "S-PSNR" in l]) == 2
