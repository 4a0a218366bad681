"""WS-PSNR / WS-SSIM (sphere_metrics.py, pseudo_codec --test --ws) without a GPU: the row weights against the
formula, the float64 torch path against a literal numpy loop over pixels and windows, the uniform weighting against
pytorch_ssim and plain PSNR, and the command line end to end on the oracle backend at 256x512."""
import math
import re

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import sphere_metrics as S
from pseudocylindrical_convolution_amd._native import PconvError

SHAPES = [(1, 3, 7, 13), (2, 3, 16, 32), (1, 1, 33, 64), (1, 3, 5, 20), (2, 2, 24, 9), (1, 3, 1, 1)]


def pair(shape, seed, noise=0.06):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    return x, (x + noise * torch.randn(shape, generator=g)).clamp(0, 1)


def numpy_metrics(x, y, weighting):
    """the definitions as a float64 loop: every pixel's 11 x 11 window of the zero-padded frame, every row weight"""
    n, c, h, w = x.shape
    k = np.arange(11) - 5
    g = np.exp(-k ** 2 / (2 * 1.5 ** 2))
    g /= g.sum()
    win = np.outer(g, g)
    wr = [math.cos(((j + 0.5) / h - 0.5) * math.pi) if weighting == "ws" else 1.0 for j in range(h)]
    out = np.zeros((n, 2))
    for f in range(n):
        se = ss = 0.0
        for ch in range(c):
            a = np.pad(x[f, ch].astype(np.float64), 5)
            b = np.pad(y[f, ch].astype(np.float64), 5)
            for j in range(h):
                for i in range(w):
                    pa, pb = a[j:j + 11, i:i + 11], b[j:j + 11, i:i + 11]
                    mu1, mu2 = (win * pa).sum(), (win * pb).sum()
                    s1 = (win * pa * pa).sum() - mu1 * mu1
                    s2 = (win * pb * pb).sum() - mu2 * mu2
                    s12 = (win * pa * pb).sum() - mu1 * mu2
                    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
                    d = a[j + 5, i + 5] - b[j + 5, i + 5]
                    se += wr[j] * d * d
                    ss += wr[j] * m
        norm = c * w * sum(wr)
        out[f] = se / norm, ss / norm
    return out


def test_weights_are_the_formula():
    for h in (1, 2, 3, 7, 64, 255, 2048):
        w = S.weights(h)
        want = torch.tensor([math.cos(((j + 0.5) / h - 0.5) * math.pi) for j in range(h)], dtype=torch.float64)
        assert w.dtype == torch.float64 and w.shape == (h,)
        assert torch.allclose(w, want, rtol=0, atol=1e-15)
        assert torch.equal(w, w.flip(0))                           # symmetric about the equator, bit for bit
        assert bool((w > 0).all()) and w.max() <= 1.0
        assert torch.equal(S.weights(h, "uniform"), torch.ones(h, dtype=torch.float64))
    with pytest.raises(ValueError):
        S.weights(8, "cpp")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("weighting", ["ws", "uniform"])
def test_torch_path_is_the_numpy_loop(shape, weighting):
    x, y = pair(shape, sum(shape))
    got = S.metrics(x, y, weighting)
    want = numpy_metrics(x.numpy(), y.numpy(), weighting)
    assert got.dtype == torch.float64 and got.shape == (shape[0], 2)
    assert np.allclose(got[:, 0].numpy(), want[:, 0], rtol=1e-6, atol=0)   # fp32 difference and square
    assert np.allclose(got[:, 1].numpy(), want[:, 1], rtol=0, atol=1e-12)
    assert torch.equal(S.ws_psnr(x, y, weighting), S.psnr(got[:, 0])) and torch.equal(S.ws_ssim(x, y, weighting), got[:, 1])


def test_uniform_is_pytorch_ssim_and_plain_psnr():
    from pseudocylindrical_convolution_amd.PCONV_operator import pytorch_ssim
    x, y = pair((3, 3, 48, 96), 11)
    ssim, psnr = S.ws_ssim(x, y, "uniform"), S.ws_psnr(x, y, "uniform")
    for i in range(3):
        assert abs(ssim[i].item() - pytorch_ssim.ssim(x[i:i + 1], y[i:i + 1]).item()) <= 1e-6
        mse = ((x[i].double() - y[i].double()) ** 2).mean().item()
        assert abs(psnr[i].item() - 10 * math.log10(1. / mse)) <= 1e-6
    # the sphere weighting is another figure on the same frames
    assert not torch.allclose(S.ws_psnr(x, y), psnr, rtol=0, atol=1e-6)


def test_uint8_form_is_the_float_form():
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 256, (2, 20, 33, 3), generator=g, dtype=torch.uint8)
    v = torch.randint(0, 256, (2, 20, 33, 3), generator=g, dtype=torch.uint8)
    f = lambda t: (t.permute(0, 3, 1, 2).float() / 255.).contiguous()     # img2tensor's arithmetic
    assert torch.equal(S.metrics(u, v), S.metrics(f(u), f(v)))


def test_identical_frames_give_inf_and_one():
    x, _ = pair((2, 3, 16, 40), 5)
    m = S.metrics(x, x.clone())
    assert torch.equal(m[:, 0], torch.zeros(2, dtype=torch.float64))
    assert torch.equal(S.ws_psnr(x, x), torch.full((2,), math.inf, dtype=torch.float64))
    assert torch.allclose(S.ws_ssim(x, x), torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-12)
    assert S.psnr(0.0) == math.inf and S.psnr(0.01) == pytest.approx(20.0)


def test_polar_error_costs_less_than_equatorial_error():
    h, w = 64, 128
    x = torch.full((1, 3, h, w), 0.5)
    polar, equator = x.clone(), x.clone()
    polar[..., 0:4, 10:30] += 0.2
    equator[..., h // 2 - 2:h // 2 + 2, 10:30] += 0.2
    assert S.ws_psnr(x, polar).item() > S.ws_psnr(x, equator).item() + 10
    assert S.ws_ssim(x, polar).item() > S.ws_ssim(x, equator).item()
    # the same error counts the same on the plain grid
    assert S.ws_psnr(x, polar, "uniform").item() == pytest.approx(S.ws_psnr(x, equator, "uniform").item(), abs=1e-9)


def test_bad_inputs_are_refused():
    x, y = pair((1, 3, 8, 8), 1)
    with pytest.raises(PconvError):
        S.metrics(x, y[:, :, :7])                                  # shape mismatch
    with pytest.raises(PconvError):
        S.metrics(x, y.double())                                   # dtype
    with pytest.raises(PconvError):
        S.metrics(x[0], y[0])                                      # not a batch
    with pytest.raises(PconvError):
        S.metrics(torch.zeros((1, 8, 8, 4), dtype=torch.uint8), torch.zeros((1, 8, 8, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        S.metrics(x, y, "s-psnr")


def drive_ws(tmp_path, monkeypatch, capsys, device, sizes, native=False):
    """--enc --container of a PNG per size (--native-size: coded at the padded size, scored at its own), --dec to
    PNG, then --test with and without --ws.  Returns the --ws rows and, per file, (source, decoded) uint8 images."""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, device)
    common = ["--ssim", "--model-idx", "3"]
    srcs, codes, decs = [], [], []
    for k, (H, W) in enumerate(sizes):
        src, code, dec = "ws%d.png" % k, "ws%d.pcv" % k, "ws%d_dec.png" % k
        _write_png(src, H, W, 30 + k)
        size = ["--native-size"] if native else ["--height", str(H), "--width", str(W)]
        PC.main(["--enc", "--container", "--img-list", src, "--code-list", code] + common + size)
        PC.main(["--dec", "--code-list", code, "--out-list", dec])
        srcs.append(src), codes.append(code), decs.append(dec)
    capsys.readouterr()
    rows = PC.decoding_and_test(codes, srcs, 3, False, 0, ws=True)
    out = capsys.readouterr().out
    assert len(re.findall(r"WS-PSNR:[0-9.]+dB, WS-SSIM:[0-9.]+", out)) == len(sizes) + 1
    assert out.index("Average Performance") < out.rindex("WS-PSNR:")
    assert all(len(r) == 5 for r in rows)
    plain = PC.decoding_and_test(codes, srcs, 3, False, 0)
    out_plain = capsys.readouterr().out
    assert "WS-" not in out_plain and all(len(r) == 3 for r in plain)
    assert np.allclose(np.array(rows)[:, :3], np.array(plain), rtol=1e-6, atol=0)   # the viewport figures as before
    # the command line: --ws prints the lines, --ws outside --test is refused
    PC.main(["--test", "--ws", "--code-list"] + codes + ["--img-list"] + srcs)
    assert len(re.findall(r"WS-PSNR:", capsys.readouterr().out)) == len(sizes) + 1
    PC.main(["--test", "--code-list"] + codes + ["--img-list"] + srcs)
    assert "WS-" not in capsys.readouterr().out
    with pytest.raises(AssertionError):
        PC.main(["--dec", "--ws", "--code-list", codes[0], "--out-list", "x.png"])
    return rows, [(PC.read_image(s), PC.read_image(d)) for s, d in zip(srcs, decs)]


def test_cli_ws_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    rows, images = drive_ws(tmp_path, monkeypatch, capsys, "cpu", [(256, 512)])
    for row, (src, dec) in zip(rows, images):
        m = S.metrics(torch.from_numpy(src)[None], torch.from_numpy(dec)[None])
        assert row[3:] == (S.psnr(m[0, 0].item()), m[0, 1].item())
        assert np.isfinite(row[3]) and 0 < row[4] < 1
