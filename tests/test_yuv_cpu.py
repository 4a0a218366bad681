"""YUV 4:2:0 frames (pseudocylindrical_convolution_amd/yuv.py, include/pconv_hip.h "YUV 4:2:0 frames") without a GPU:
the definition's own properties, the vectorised torch twin against a per-pixel loop, the layouts, raw files and the
command line on the oracle backend."""
import itertools
import os

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import erp_size, yuv
from pseudocylindrical_convolution_amd._native import PconvError

COMBOS = list(itertools.product(["yuv420p", "yuv420p10le"], ["bt709", "bt601"], ["limited", "full"]))   # depth x matrix x range


def random_frames(n, h, w, fmt, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1 << yuv.depth(fmt), (n, yuv.frame_elems(h, w)), generator=g, dtype=torch.int32).to(yuv.dtype(fmt))


def frames_of(Y, U, V, fmt):
    """frame buffers of the format from integer planes (n, h, w), (n, h/2, w/2) x 2"""
    n, h, w = Y.shape
    buf = torch.empty((n, yuv.frame_elems(h, w)), dtype=torch.int32)
    for dst, src in zip(yuv.plane_views_of(buf, h, w, fmt), (Y, U, V)):
        dst.copy_(src)
    return buf.to(yuv.dtype(fmt))


def test_formats_and_constants():
    assert yuv.frame_bytes(4, 6, "yuv420p") == 36 and yuv.frame_bytes(4, 6, "nv12") == 36
    assert yuv.frame_bytes(4, 6, "yuv420p10le") == 72 and yuv.dtype("yuv420p10le") == torch.uint16
    k = yuv.coefficients("bt709", "limited", "yuv420p10le")
    assert (k["yo"], k["ys"], k["co"], k["cs"], k["qmax"]) == (64.0, 876.0, 512.0, 896.0, 1023.0)
    k = yuv.coefficients("bt601", "full", "yuv420p")
    assert (k["yo"], k["ys"], k["co"], k["cs"], k["qmax"]) == (0.0, 255.0, 128.0, 255.0, 255.0)
    Kg = 1.0 - 0.299 - 0.114
    assert k["Kg"] == float(np.float32(Kg)) and k["b"] == float(np.float32(0.114 * (2 * (1 - 0.114)) / Kg))
    assert k["a"] == float(np.float32(1.402)) and k["dd"] == float(np.float32(1.772))
    for bad in ((3, 4), (4, 5), (0, 4)):
        with pytest.raises(PconvError):
            yuv.frame_elems(*bad)
    with pytest.raises(PconvError):
        yuv.coefficients("bt2020")
    with pytest.raises(PconvError):
        yuv.depth("yuv444p")


def test_chroma_upsampling_is_exact_in_float32():
    for d in (8, 10):
        c = torch.randint(0, 1 << d, (2, 9, 7), generator=torch.Generator().manual_seed(d))
        c[0, 0, :2], c[0, -1, -2:] = 0, (1 << d) - 1
        assert torch.equal(yuv.chroma_up(c, torch.float32).double(), yuv.chroma_up(c, torch.float64))


@pytest.mark.parametrize("fmt,matrix,rng", COMBOS)
def test_gray_and_constant_chroma_round_trip_exactly(fmt, matrix, rng):
    d, h, w = yuv.depth(fmt), 8, 12
    s = 1 << (d - 8)
    lo, hi = (16 * s, 235 * s) if rng == "limited" else (0, (1 << d) - 1)
    mid = 1 << (d - 1)
    g = torch.Generator().manual_seed(3)
    Y = torch.randint(lo, hi + 1, (3, h, w), generator=g)
    Y[0, 0, :2] = torch.tensor([lo, hi])
    gray = frames_of(Y, torch.full((3, h // 2, w // 2), mid), torch.full((3, h // 2, w // 2), mid), fmt)
    assert torch.equal(yuv.from_rgb(yuv.to_rgb(gray, h, w, fmt, matrix, rng), h, w, fmt, matrix, rng), gray)
    Y = torch.randint(100 * s, 150 * s, (3, h, w), generator=g)
    tinted = frames_of(Y, torch.full((3, h // 2, w // 2), mid + 10 * s), torch.full((3, h // 2, w // 2), mid - 7 * s), fmt)
    rgb = yuv.to_rgb(tinted, h, w, fmt, matrix, rng)
    assert 0 < float(rgb.min()) and float(rgb.max()) < 1     # in gamut: nothing was clamped
    assert torch.equal(yuv.from_rgb(rgb, h, w, fmt, matrix, rng), tinted)


@pytest.mark.parametrize("fmt,matrix,rng", COMBOS)
def test_float32_statement_against_float64(fmt, matrix, rng):
    h, w = 64, 128
    buf = random_frames(2, h, w, fmt)
    a32 = yuv.to_rgb_torch(buf, h, w, fmt, matrix, rng)
    a64 = yuv.to_rgb_torch(buf, h, w, fmt, matrix, rng, dt=torch.float64)
    err = float((a32.double() - a64).abs().max())
    print("ingest float32 - float64: %.3g" % err)
    assert a32.dtype == torch.float32 and err <= 1e-6
    # a (2, 3, 64, 128) frame at its coded size: the rows outside the crop are not read
    x = torch.zeros(2, 3, *erp_size.coded_size(h, w)[:2])
    top = erp_size.coded_size(h, w)[2]
    x[:, :, top:top + h] = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(0))
    e32 = yuv.from_rgb_torch(x, h, w, fmt, matrix, rng).to(torch.int32)
    e64 = yuv.from_rgb_torch(x, h, w, fmt, matrix, rng, dt=torch.float64).to(torch.int32)
    diff = (e32 - e64).abs()
    print("egress codes that differ: max %d, share %.3g" % (int(diff.max()), float((diff > 0).double().mean())))
    assert int(diff.max()) <= 1 and float((diff > 0).double().mean()) <= 1e-3


def loop_to_rgb(buf, h, w, fmt, matrix, rng):
    """the ingest of the definition pixel by pixel in numpy float32 scalars, at the coded size"""
    f = np.float32
    k = {name: f(v) for name, v in yuv.coefficients(matrix, rng, fmt).items()}
    Y, U, V = (yuv._codes(p, fmt).numpy() for p in yuv.plane_views(buf, h, w, fmt))
    H, W, top = erp_size.coded_size(h, w)
    m = (W - w + 1) // 2
    out = np.zeros((buf.shape[0], 3, H, W), np.float32)

    def chroma(C, y, x):
        j, i = y // 2, x // 2
        if y % 2 == 0:
            col = lambda i: f(0.25) * f(C[max(j - 1, 0), i]) + f(0.75) * f(C[j, i])
        else:
            col = lambda i: f(0.75) * f(C[j, i]) + f(0.25) * f(C[min(j + 1, h // 2 - 1), i])
        return col(i) if x % 2 == 0 else f(0.5) * (col(i) + col((i + 1) % (w // 2)))

    for n in range(buf.shape[0]):
        for yc in range(H):
            y, flip = yc - top, False
            if y < 0:
                y, flip = -1 - y, True
            elif y >= h:
                y, flip = 2 * h - 1 - y, True
            y = min(max(y, 0), h - 1)
            for xc in range(W):
                x = xc if xc < w else (w - 1 if xc - w < m else 0)
                if flip:
                    x = (x + w // 2) % w
                yy = (f(Y[n, y, x]) - k["yo"]) / k["ys"]
                cb = (chroma(U[n], y, x) - k["co"]) / k["cs"]
                cr = (chroma(V[n], y, x) - k["co"]) / k["cs"]
                rgb = (yy + k["a"] * cr, (yy - k["b"] * cb) - k["c"] * cr, yy + k["dd"] * cb)
                out[n, :, yc, xc] = [min(max(v, f(0)), f(1)) for v in rgb]
    return torch.from_numpy(out)


def loop_from_rgb(x, h, w, fmt, matrix, rng):
    """the egress of the definition sample by sample in numpy float32 scalars: integer planes Y, U, V"""
    f = np.float32
    k = {name: f(v) for name, v in yuv.coefficients(matrix, rng, fmt).items()}
    top = erp_size.coded_size(h, w)[2]
    p = np.clip(x.numpy()[:, :, top:top + h, :w], f(0), f(1))
    n = p.shape[0]
    Y, U, V = np.zeros((n, h, w), np.int64), np.zeros((n, h // 2, w // 2), np.int64), np.zeros((n, h // 2, w // 2), np.int64)
    quant = lambda v, scale, offset: int(min(max(np.floor((v * scale + offset) + f(0.5)), f(0)), k["qmax"]))
    for b in range(n):
        y = np.zeros((h, w), np.float32)
        cb, cr = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        for r in range(h):
            for c in range(w):
                R, G, B = p[b, :, r, c]
                y[r, c] = (k["Kr"] * R + k["Kg"] * G) + k["Kb"] * B
                cb[r, c], cr[r, c] = (B - y[r, c]) / k["dd"], (R - y[r, c]) / k["a"]
                Y[b, r, c] = quant(y[r, c], k["ys"], k["yo"])
        for j in range(h // 2):
            for plane, src in ((U, cb), (V, cr)):
                v = [f(0.5) * (src[2 * j, c] + src[2 * j + 1, c]) for c in range(w)]
                for i in range(w // 2):
                    plane[b, j, i] = quant((f(0.25) * v[(2 * i - 1) % w] + f(0.5) * v[2 * i]) + f(0.25) * v[2 * i + 1],
                                           k["cs"], k["co"])
    return Y, U, V


@pytest.mark.parametrize("fmt,matrix,rng", [("yuv420p", "bt709", "limited"), ("yuv420p10le", "bt601", "full"),
                                            ("nv12", "bt601", "limited")])
def test_vectorised_twin_is_the_loop(fmt, matrix, rng):
    h, w = 4, 6   # w/2 odd: the column parity flips across the poles; the coded frame is 256 x 16
    buf = random_frames(2, h, w, fmt, seed=5)
    assert torch.equal(yuv.to_rgb(buf, h, w, fmt, matrix, rng), loop_to_rgb(buf, h, w, fmt, matrix, rng))
    x = torch.rand(2, 3, *erp_size.coded_size(h, w)[:2], generator=torch.Generator().manual_seed(6)) * 1.2 - 0.1
    want = frames_of(*(torch.from_numpy(p) for p in loop_from_rgb(x, h, w, fmt, matrix, rng)), fmt)
    assert torch.equal(yuv.from_rgb(x, h, w, fmt, matrix, rng), want)


def test_unpadded_conversion_pads_to_the_coded_one():
    buf = random_frames(1, 6, 10, "yuv420p", seed=8)
    plain = yuv.to_rgb_torch(buf, 6, 10, "yuv420p", pad=False)
    assert tuple(plain.shape) == (1, 3, 6, 10)
    assert torch.equal(erp_size.pad_torch(plain), yuv.to_rgb(buf, 6, 10, "yuv420p"))
    codable = random_frames(1, 256, 32, "yuv420p", seed=9)
    assert torch.equal(yuv.to_rgb_torch(codable, 256, 32, "yuv420p", pad=False), yuv.to_rgb(codable, 256, 32, "yuv420p"))


def test_nv12_and_yuv420p_hold_the_same_planes():
    h, w = 6, 10
    planar = random_frames(2, h, w, "yuv420p", seed=11)
    Y, U, V = yuv.plane_views(planar, h, w, "yuv420p")
    semi = frames_of(Y, U, V, "nv12")
    assert not torch.equal(semi, planar)
    assert all(torch.equal(a, b) for a, b in zip(yuv.plane_views(semi, h, w, "nv12"), (Y, U, V)))
    assert torch.equal(yuv.to_rgb(semi, h, w, "nv12"), yuv.to_rgb(planar, h, w, "yuv420p"))
    x = torch.rand(2, 3, *erp_size.coded_size(h, w)[:2], generator=torch.Generator().manual_seed(12))
    a, b = yuv.from_rgb(x, h, w, "nv12"), yuv.from_rgb(x, h, w, "yuv420p")
    assert all(torch.equal(p, q) for p, q in zip(yuv.plane_views(a, h, w, "nv12"), yuv.plane_views(b, h, w, "yuv420p")))
    for p, q in zip(yuv.planes(a, h, w, "nv12"), yuv.planes(b, h, w, "yuv420p")):
        assert p.dtype == torch.float32 and p.dim() == 4 and p.shape[1] == 1 and torch.equal(p, q)


def test_ten_bit_samples_are_taken_modulo_1024():
    h, w = 4, 6
    buf = random_frames(1, h, w, "yuv420p10le", seed=13)
    high = (buf.to(torch.int32) + 1024 * 5).to(torch.uint16)
    assert torch.equal(yuv.to_rgb(high, h, w, "yuv420p10le"), yuv.to_rgb(buf, h, w, "yuv420p10le"))


def test_ws_psnr_yuv_on_the_cpu():
    from pseudocylindrical_convolution_amd import sphere_metrics
    h, w, fmt = 8, 12, "yuv420p10le"
    a, b = random_frames(2, h, w, fmt, seed=14), random_frames(2, h, w, fmt, seed=15)
    got = yuv.ws_psnr_yuv(a, b, h, w, fmt)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3)
    for c, (p, q) in enumerate(zip(yuv.planes(a, h, w, fmt), yuv.planes(b, h, w, fmt))):
        assert torch.equal(got[:, c], sphere_metrics.ws_psnr(p, q))
    assert torch.isinf(yuv.ws_psnr_yuv(a, a, h, w, fmt)).all()


@pytest.mark.parametrize("fmt", sorted(yuv.FORMATS))
def test_raw_files_round_trip(tmp_path, fmt):
    h, w = 4, 6
    path = str(tmp_path / "clip.yuv")
    buf = random_frames(5, h, w, fmt, seed=16)
    assert yuv.write_frames(path, buf[:2], h, w, fmt) == 2
    assert yuv.write_frames(path, buf[2:], h, w, fmt, append=True) == 3
    assert os.path.getsize(path) == 5 * yuv.frame_bytes(h, w, fmt) and yuv.count_frames(path, h, w, fmt) == 5
    assert torch.equal(yuv.read_frames(path, h, w, fmt), buf)
    assert torch.equal(yuv.read_frames(path, h, w, fmt, start=1, count=3), buf[1:4])
    if fmt == "yuv420p10le":   # little-endian on disk
        with open(path, "rb") as f:
            first = f.read(2)
        assert first[0] + 256 * first[1] == int(buf[0, 0])
    with pytest.raises(PconvError, match="holds 5"):
        yuv.read_frames(path, h, w, fmt, start=3, count=3)
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(PconvError, match="whole number"):
        yuv.read_frames(path, h, w, fmt)


@pytest.mark.parametrize("flags,message", [
    (["--enc", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "nv12", "--img-list", "a.png", "--code-list", "a.bin"],
     "two sources"),
    (["--enc", "--yuv", "a.yuv", "--pix-fmt", "nv12", "--code-list", "a.bin"], "--size"),
    (["--enc", "--yuv", "a.yuv", "--size", "512x256", "--code-list", "a.bin"], "--pix-fmt"),
    (["--enc", "--yuv", "a.yuv", "--size", "511x256", "--pix-fmt", "nv12", "--code-list", "a.bin"], "even"),
    (["--enc", "--yuv", "a.yuv", "--size", "512", "--pix-fmt", "nv12", "--code-list", "a.bin"], "WIDTHxHEIGHT"),
    (["--enc", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "yuv444p", "--code-list", "a.bin"], "invalid choice"),
    (["--enc", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "nv12", "--frames", "2", "--code-list", "a.bin"],
     "one code file per frame"),
    (["--dec", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "nv12", "--code-list", "a.bin"], "--yuv-out"),
    (["--enc", "--yuv-out", "a.yuv", "--pix-fmt", "nv12", "--code-list", "a.bin"], "needs --dec"),
    (["--dec", "--yuv-out", "a.yuv", "--pix-fmt", "nv12", "--code-list", "a.bin", "--out-list", "a.png"], "two destinations"),
    (["--rd", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "nv12"], "--rd takes images"),
    (["--enc", "--img-list", "a.png", "--code-list", "a.bin", "--pix-fmt", "nv12"], "needs --yuv"),
    (["--enc", "--img-list", "a.png", "--code-list", "a.bin", "--yuv-range", "full"], "needs --yuv"),
])
def test_cli_refuses_contradictory_flags(capsys, flags, message):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    with pytest.raises(SystemExit) as stop:
        PC.main(flags)
    assert stop.value.code == 2 and message in capsys.readouterr().err


def test_cli_yuv_end_to_end_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    """--enc --yuv -> --dec --yuv-out at 256x512 on the oracle backend (tests/test_cli.py's set-up): the file has the
    right length and its frames are from_rgb of the decoded tensor; --test --ws prints the per-plane figures"""
    from test_cli import _models
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cpu")
    h, w, fmt = 256, 512, "yuv420p"
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    rgb = torch.stack([0.5 + 0.3 * torch.sin(9 * xx + k) * torch.cos(4 * yy) for k in range(3)])[None]
    clip = torch.cat([random_frames(1, h, w, fmt, seed=20), yuv.from_rgb(rgb, h, w, fmt), yuv.from_rgb(1 - rgb, h, w, fmt)])
    yuv.write_frames("in.yuv", clip, h, w, fmt)
    common = ["--ssim", "--model-idx", "3"]
    src = ["--yuv", "in.yuv", "--size", "%dx%d" % (w, h), "--pix-fmt", fmt, "--start", "1"]
    PC.main(["--enc", "--code-list", "f1.bin", "f2.bin"] + src + common)
    PC.main(["--dec", "--code-list", "f1.bin", "f2.bin", "--yuv-out", "out.yuv", "--pix-fmt", fmt, "--size", "%dx%d" % (w, h)] + common)
    assert os.path.getsize("out.yuv") == 2 * yuv.frame_bytes(h, w, fmt)
    got = yuv.read_frames("out.yuv", h, w, fmt)
    dec = PC.PseudoDecoder(56, 0)
    PC.load_models(dec, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    for k, name in enumerate(["f1.bin", "f2.bin"]):
        rec = dec(name, h, w)     # the codec's planes are B, G, R
        assert torch.equal(got[k:k + 1], yuv.from_rgb(rec.flip(1).contiguous(), h, w, fmt))
    # a container carries the size: no --size on the way back, and another pixel format out than in
    PC.main(["--enc", "--container", "--frames", "1", "--code-list", "g.pcv"] + src + common)
    PC.main(["--dec", "--code-list", "g.pcv", "--yuv-out", "out10.yuv", "--pix-fmt", "yuv420p10le"])
    assert os.path.getsize("out10.yuv") == yuv.frame_bytes(h, w, "yuv420p10le")
    capsys.readouterr()
    PC.main(["--test", "--ws", "--code-list", "f1.bin", "f2.bin"] + src + common)
    out = capsys.readouterr().out
    assert out.count("WS-PSNR-Y:") == 3 and out.count("WS-PSNR-V:") == 3 and out.count("WS-SSIM:") == 3
    assert "Average Performance" in out
