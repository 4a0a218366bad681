"""The sphere-aware Lanczos-3 resize (erp_resample.py, container version 3, --code-size) without a GPU: the C tap table
against an independent float64 evaluation of the formulas, the torch twin against a per-pixel numpy loop that states
the rule on its own, exact properties of the twin, the container format, and the command line end to end on the
oracle backend at 300x600 -> 256x512."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import container as C
from pseudocylindrical_convolution_amd import erp_resample as R
from pseudocylindrical_convolution_amd import erp_size

PAIRS = [(96, 48), (64, 96), (70, 44), (128, 16), (5760, 4096), (50, 50), (7, 7)]


def python_taps(n_in, n_out):
    """include/pconv_hip.h's tap table from the formulas alone: (first list, float64 weights (n_out, T) zero-padded)"""
    D = 2 * max(n_in, n_out)
    first, rows = [], []
    for i in range(n_out):
        ks = [k for k in range(-3 * D, n_in + 3 * D)
              if abs(2 * n_out * k - (2 * i + 1) * n_in + n_out) < 3 * D] if n_in + n_out < 400 else None
        if ks is None:   # the same set from the real-valued bounds (large axes: the brute-force range is too slow)
            c = Fraction((2 * i + 1) * n_in - n_out, 2 * n_out)
            r = Fraction(3 * D, 2 * n_out)
            lo, hi = math.floor(c - r) + 1, math.ceil(c + r) - 1
            ks = list(range(lo, hi + 1))
        raw = []
        for k in ks:
            N = 2 * n_out * k - (2 * i + 1) * n_in + n_out
            assert abs(N) < 3 * D
            if N == 0:
                raw.append(1.0)
            elif N % D == 0:
                raw.append(0.0)
            else:
                x = math.pi * abs(N) / D
                raw.append(3.0 * math.sin(x) * math.sin(x / 3.0) / (x * x))
        total = 0.0
        for v in raw:
            total += v
        first.append(ks[0])
        rows.append([v / total for v in raw])
    T = max(len(r) for r in rows)
    return first, np.array([r + [0.0] * (T - len(r)) for r in rows], dtype=np.float64)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_c_table_is_the_formula(n_in, n_out):
    first, w = R.taps(n_in, n_out)
    want_first, want_w = python_taps(n_in, n_out)
    assert first.dtype == torch.int32 and w.dtype == torch.float32
    assert first.tolist() == want_first
    assert tuple(w.shape) == want_w.shape                                   # T
    assert np.abs(w.numpy().astype(np.float64) - want_w).max() <= 2.0 ** -23
    T = w.shape[1]
    assert (w.double().sum(1) - 1.0).abs().max().item() <= T * 2.0 ** -24
    # periodicity, bit for bit
    g = math.gcd(n_in, n_out)
    p, step = n_out // g, n_in // g
    if p < n_out:
        assert torch.equal(first[p:], first[:-p] + step)
        assert torch.equal(w[p:], w[:-p])
    if n_in == n_out:
        assert torch.equal((w != 0).sum(1), torch.ones(n_out, dtype=torch.long))
        assert torch.equal(w.max(1).values, torch.ones(n_out))
        centre = (w == 1).float().argmax(1).int()
        assert torch.equal(first + centre, torch.arange(n_out, dtype=torch.int32))


def test_tap_counts_and_refusals():
    from pseudocylindrical_convolution_amd._native import PconvError
    assert R.taps(64, 96)[1].shape[1] == 6 and R.taps(96, 48)[1].shape[1] == 12
    assert R.taps(5760, 4096)[1].shape[1] == 9 and R.taps(128, 16)[1].shape[1] == 48
    for bad in ((90, 10), (1, 8), (8, 1), ((1 << 20) + 1, 1 << 20)):
        with pytest.raises(PconvError):
            R.taps(*bad)
    with pytest.raises(PconvError):
        R.resize(torch.zeros(1, 1, 4, 90), 4, 10)
    with pytest.raises(PconvError):
        R.resize(torch.zeros(1, 1, 4, 8).double(), 4, 4)


def numpy_resize(img, h2, w2, clamp):
    """the rule stated as a loop over output pixels, float32 operation by operation: (c, h, w) -> (c, h2, w2)"""
    c, h, w = img.shape
    fx, wx = (t.numpy() for t in R.taps(w, w2))
    fy, wy = (t.numpy() for t in R.taps(h, h2))
    mid = np.empty((c, h, w2), dtype=np.float32)
    for y in range(h):
        for i in range(w2):
            acc = None
            for t in range(wx.shape[1]):
                k = (int(fx[i]) + t) % w                       # Python's modulo is the mathematical one: the seam
                term = np.float32(wx[i, t]) * img[:, y, k]
                acc = term if acc is None else (acc + term).astype(np.float32)
            mid[:, y, i] = acc
    out = np.empty((c, h2, w2), dtype=np.float32)
    for j in range(h2):
        for i in range(w2):
            acc = None
            for t in range(wy.shape[1]):
                r, col = int(fy[j]) + t, i
                if r < 0:
                    r, col = -1 - r, (i + w2 // 2) % w2          # across the north pole: half a turn of longitude
                elif r >= h:
                    r, col = 2 * h - 1 - r, (i + w2 // 2) % w2   # across the south pole
                r = min(max(r, 0), h - 1)
                term = np.float32(wy[j, t]) * mid[:, r, col]
                acc = term if acc is None else (acc + term).astype(np.float32)
            out[:, j, i] = acc
    if clamp:
        out = np.minimum(np.maximum(out, np.float32(0)), np.float32(1))
    return out


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("h,w,h2,w2", [(12, 16, 6, 8), (12, 16, 7, 10), (5, 8, 9, 14), (6, 10, 4, 7)])
def test_twin_is_the_numpy_rule(h, w, h2, w2, clamp):
    g = torch.Generator().manual_seed(h * 100 + w2)
    x = torch.randint(0, 256, (2, 3, h, w), generator=g).float() / 255.
    if clamp:
        x = (x > 0.5).float()                                                # hard edges: the overshoot is there to clamp
    got = R.resize(x, h2, w2, clamp=clamp)
    want = np.stack([numpy_resize(f, h2, w2, clamp) for f in x.numpy()])
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, h2, w2)
    assert np.array_equal(got.numpy(), want)
    if (h, w, h2, w2) == (5, 8, 9, 14):
        fy = R.taps(h, h2)[0]
        assert bool(((fy < 0) | (fy + R.taps(h, h2)[1].shape[1] > h)).all())  # pole-touching taps on every output row


def test_equal_sizes_return_the_input():
    x = torch.rand(2, 3, 11, 18, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.resize(x, 11, 18), x)
    out = torch.empty_like(x)
    assert R.resize(x, 11, 18, out=out) is out and torch.equal(out, x)


@pytest.mark.parametrize("w,w2,m", [(48, 16, 5), (48, 24, 1), (16, 48, 3), (20, 40, 7)])
def test_the_seam_is_a_roll_bit_for_bit(w, w2, m):
    """at an integer ratio f a roll of the input by f*m columns is a roll of the output by m; at an integer up-ratio g
    a roll by m is a roll by g*m"""
    x = torch.rand(1, 2, 10, w, generator=torch.Generator().manual_seed(w))
    for h2 in (10, 7):
        y = R.resize(x, h2, w2)
        if w >= w2:
            f = w // w2
            assert torch.equal(R.resize(torch.roll(x, f * m, 3), h2, w2), torch.roll(y, m, 3))
        else:
            g = w2 // w
            assert torch.equal(R.resize(torch.roll(x, m, 3), h2, w2), torch.roll(y, g * m, 3))


@pytest.mark.parametrize("h,w,h2,w2", [(12, 16, 7, 10), (5, 8, 9, 14), (64, 128, 8, 16), (40, 70, 33, 45)])
def test_a_constant_frame_stays_constant(h, w, h2, w2):
    """each output is a chain of T products and T - 1 additions of weights that sum to 1 within T * 2^-24: the error
    of one pass is below 2 * T * 2^-24 * |c|, of both below 2 * (Tx + Ty) * 2^-24 * |c|"""
    c = 0.7
    tx, ty = R.taps(w, w2)[1].shape[1], R.taps(h, h2)[1].shape[1]
    y = R.resize(torch.full((1, 1, h, w), c), h2, w2)
    err = (y.double() - float(np.float32(c))).abs().max().item()
    assert err <= 2 * (tx + ty) * 2.0 ** -24 * c, err


def test_the_clamp_bounds_a_step_edge():
    x = torch.zeros(1, 1, 16, 64)
    x[..., 16:48] = 1.0
    free = R.resize(x, 16, 96)
    assert free.min().item() < -0.02 and free.max().item() > 1.02            # Lanczos overshoots
    held = R.resize(x, 16, 96, clamp=True)
    assert held.min().item() == 0.0 and held.max().item() == 1.0
    assert torch.equal(held, free.clamp(0, 1))


def test_container_v3_round_trip_and_errors():
    args = dict(height=2048, width=4096, model_idx=3, ssim=True, valid_dim=56)
    blob = C.pack_any(b"\x01\x02\x03", source=(4096, 8192), **args)
    assert len(blob) == C.HEADER_BYTES_SOURCE + 3 == 31 and blob[:4] == b"PCVC" and blob[4] == 3
    head, payload = C.unpack(blob)
    assert payload == b"\x01\x02\x03"
    assert head == {"height": 2048, "width": 4096, "model_idx": 3, "ssim": True, "valid_dim": 56,
                    "source_height": 4096, "source_width": 8192}
    # a coded size the codec does not take as it is, under a source
    odd = C.unpack(C.pack_any(b"", height=250, width=500, model_idx=0, ssim=False, valid_dim=192, source=(300, 600)))[0]
    assert (odd["height"], odd["width"], odd["source_height"], odd["source_width"]) == (250, 500, 300, 600)
    # no source, or the coded size itself: versions 1 and 2, byte for byte as before
    assert C.pack_any(b"xyz", **args) == C.pack(b"xyz", **args) == C.pack_any(b"xyz", source=(2048, 4096), **args)
    assert C.pack_any(b"xyz", **args)[4] == 1 and len(C.pack_any(b"xyz", **args)) == 19
    v2 = dict(args, height=2880, width=5760)
    assert C.pack_any(b"xyz", **v2) == C.pack_any(b"xyz", source=None, **v2) == C.pack_any(b"xyz", source=(2880, 5760), **v2)
    assert C.pack_any(b"xyz", **v2)[4] == 2 and len(C.pack_any(b"xyz", **v2)) == 23
    assert C.pack_any(b"xyz", **v2)[:20] == b"PCVC\x02\x01\x03\x0e" + (2880).to_bytes(4, "little") + \
        (5760).to_bytes(4, "little") + (3).to_bytes(4, "little")
    assert set(C.unpack(C.pack_any(b"xyz", **v2))[0]) == set(C.unpack(C.pack(b"xyz", **args))[0]) == \
        {"height", "width", "model_idx", "ssim", "valid_dim"}
    # truncated, over-long, unknown version, wrong magic, sizes out of range (the cases of the version-2 test)
    for bad in (blob[:10], blob[:18], blob[:26], blob[:-1], blob + b"\x00", blob[:4] + b"\x04" + blob[5:],
                b"XXXX" + blob[4:], blob[:8] + b"\x01\x00\x00\x00" + blob[12:],
                blob[:16] + b"\x01\x00\x00\x00" + blob[20:], blob[:20] + b"\x00\x00\x20\x00" + blob[24:]):
        with pytest.raises(C.ContainerError):
            C.unpack(bad)
    with pytest.raises(C.ContainerError):
        C.pack_any(b"", source=(1, 64), **args)
    with pytest.raises(C.ContainerError):
        C.pack_any(b"", height=1, width=64, model_idx=0, ssim=True, valid_dim=56, source=(64, 64))


def test_sniff_and_header_bytes_v3(tmp_path):
    boxed = str(tmp_path / "a.pcv")
    C.write_any(boxed, b"\x05" * 40, height=256, width=512, model_idx=3, ssim=True, valid_dim=56, source=(300, 600))
    assert C.sniff(boxed) == {"height": 256, "width": 512, "model_idx": 3, "ssim": True, "valid_dim": 56,
                              "source_height": 300, "source_width": 600}
    assert C.header_bytes(boxed) == 28
    assert C.read(boxed)[1] == b"\x05" * 40
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    assert PC.bitrate(boxed, 300, 600) == 40 * 8 / 600. / 300.


def drive_code_size(tmp_path, monkeypatch, capsys, device):
    """--enc --code-size 512x256 --container of a 300 x 600 PNG, then --dec and --test --ws of the file"""
    from PIL import Image
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from pseudocylindrical_convolution_amd.PCONV_operator import backend
    from test_cli import _models
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, device)
    h, w, h2, w2 = 300, 600, 256, 512
    g = np.random.default_rng(5)
    yy, xx = np.linspace(0, 1, h)[:, None, None], np.linspace(0, 1, w)[None, :, None]
    img = (0.5 + 0.3 * np.sin(6.28318 * 2 * xx + g.random(3)) * np.cos(3.14159 * yy) + 0.05 * g.random((h, w, 3)))
    Image.fromarray((img.clip(0, 1) * 255).astype(np.uint8)).save("src.png")
    common = ["--ssim", "--model-idx", "3"]
    PC.main(["--enc", "--code-size", "%dx%d" % (w2, h2), "--container", "--img-list", "src.png", "--code-list", "src.pcv"]
            + common)
    out = capsys.readouterr().out
    head, payload = C.read("src.pcv")
    assert head == {"height": h2, "width": w2, "model_idx": 3, "ssim": True, "valid_dim": 56,
                    "source_height": h, "source_width": w}
    assert C.header_bytes("src.pcv") == 28
    assert re.findall(r"bitrate: ([0-9.]+)bpp", out) == ["%.3f" % (len(payload) * 8 / float(h * w))]
    # the payload is today's path on the twin-resized picture
    dev = backend.device_of(0)
    small = R.resize_torch(PC.img2tensor(PC.read_image("src.png"), "cpu"), h2, w2, clamp=True)
    t1 = PC.PseudoEncoder(56, device_id=0).to(dev)
    PC.load_models(t1, "demo/ssim/4_56_encoder.pt", "demo/ssim/4_56_ent.pt", dev)
    t1(small.to(dev), "direct.pcv", {"model_idx": 3, "ssim": True})
    dhead, dpayload = C.read("direct.pcv")
    assert (dhead["height"], dhead["width"]) == (h2, w2) and "source_height" not in dhead and dpayload == payload
    # --dec: a picture of the source size, the resize of the direct file's decode
    PC.main(["--dec", "--code-list", "src.pcv", "direct.pcv", "--out-list", "dec.png", "dec_direct.png"])
    dec, dec_direct = PC.read_image("dec.png"), PC.read_image("dec_direct.png")
    assert dec.shape == (h, w, 3) and dec_direct.shape == (h2, w2, 3)
    capsys.readouterr()
    # --test --ws at the source size, bpp over h * w
    PC.main(["--test", "--ws", "--code-list", "src.pcv", "--img-list", "src.png"])
    out = capsys.readouterr().out
    rate, psnr, ssim = re.findall(r"Bitrate:([0-9.]+)bpp, PSNR:([0-9.]+)dB, SSIM:([0-9.]+)", out)[0]
    assert rate == "%.3f" % (len(payload) * 8 / float(h * w))
    wsp, wss = re.findall(r"WS-PSNR:([0-9.]+)dB, WS-SSIM:([0-9.]+)", out)[0]
    assert all(np.isfinite(float(v)) for v in (psnr, ssim, wsp, wss))
    rows = PC.decoding_and_test(["src.pcv"], ["src.png"], 3, False, 0, ws=True)
    assert abs(rows[0][0] - len(payload) * 8 / float(h * w)) < 1e-12 and all(np.isfinite(v) for v in rows[0])
    # the refusals: no --container, with --native-size, with --yuv
    enc = ["--enc", "--code-size", "512x256", "--img-list", "src.png", "--code-list", "x.bin"] + common
    for extra in ([], ["--container", "--native-size"],
                  ["--container", "--yuv", "a.yuv", "--size", "600x300", "--pix-fmt", "yuv420p"]):
        with pytest.raises(SystemExit):
            PC.main(enc + extra)
    assert "--code-size" in capsys.readouterr().err


def test_cli_code_size_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    drive_code_size(tmp_path, monkeypatch, capsys, "cpu")
