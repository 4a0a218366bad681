"""WS-MS-SSIM (sphere_metrics.ms_*, pseudo_codec --test --ws --ms-ssim, train.py --loss ws-ms) without a GPU: the
float64 torch statement against a literal numpy loop over scales, pixels and windows, the pooling order, the clamp
and its zero gradient, torch's gradcheck, the explicit gradient chain against torch autograd, refused inputs, and the
command line and two training steps on the oracle backend."""
import math
import os
import re

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import sphere_metrics as S
from pseudocylindrical_convolution_amd._native import PconvError

WEIGHTINGS = ["ws", "uniform"]


def pair64(shape, seed):
    """float64-valued x = rand, y = x + 0.1·randn, not clamped"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    return x, x + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)


def gout_of(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((n, 2), generator=g, dtype=torch.float64)
    return v + torch.sign(v) * 0.25


def numpy_scales(x, y, weighting):
    """the definition as a float64 loop: five scales of 2x2 means, every pixel's 11 x 11 window of the zero-padded
    scale, the row weights of a frame with that scale's rows"""
    n, c = x.shape[:2]
    k = np.arange(11) - 5
    g = np.exp(-k ** 2 / (2 * 1.5 ** 2))
    g /= g.sum()
    win = np.outer(g, g)
    out = np.zeros((n, 5))
    for s in range(5):
        h, w = x.shape[2:]
        wr = [math.cos(((j + 0.5) / h - 0.5) * math.pi) if weighting == "ws" else 1.0 for j in range(h)]
        for f in range(n):
            acc = 0.0
            for ch in range(c):
                a, b = np.pad(x[f, ch], 5), np.pad(y[f, ch], 5)
                for j in range(h):
                    for i in range(w):
                        pa, pb = a[j:j + 11, i:i + 11], b[j:j + 11, i:i + 11]
                        mu1, mu2 = (win * pa).sum(), (win * pb).sum()
                        s1 = (win * pa * pa).sum() - mu1 * mu1
                        s2 = (win * pb * pb).sum() - mu2 * mu2
                        s12 = (win * pa * pb).sum() - mu1 * mu2
                        m = (2 * s12 + 9e-4) / (s1 + s2 + 9e-4)
                        if s == 4:
                            m *= (2 * mu1 * mu2 + 1e-4) / (mu1 * mu1 + mu2 * mu2 + 1e-4)
                        acc += wr[j] * m
            out[f, s] = acc / (c * w * sum(wr))
        if s < 4:
            h2, w2 = h // 2, w // 2
            nx, ny = np.zeros((n, c, h2, w2)), np.zeros((n, c, h2, w2))
            for j in range(h2):
                for i in range(w2):
                    for src, dst in ((x, nx), (y, ny)):
                        dst[:, :, j, i] = ((src[:, :, 2 * j, 2 * i] + src[:, :, 2 * j, 2 * i + 1])
                                           + (src[:, :, 2 * j + 1, 2 * i] + src[:, :, 2 * j + 1, 2 * i + 1])) * 0.25
            x, y = nx, ny
    return out


def test_last_scale_is_ws_ssim_of_the_pooled_frames():
    """v_4 of the float64 statement has the bits of the single-scale statement's WS-SSIM on pool⁴ of the frames"""
    for shape in [(1, 1, 16, 16), (2, 3, 17, 19), (1, 2, 33, 65), (1, 1, 130, 258), (1, 1, 528, 1040)]:
        x, y = pair64(shape, sum(shape))
        a, b = x, y
        for _ in range(S.SCALES - 1):
            a, b = S.pool(a), S.pool(b)
        for weighting in WEIGHTINGS:
            v4 = S.ms_scales_torch(x, y, weighting, torch.float64)[:, 4]
            assert torch.equal(v4, S.loss_terms(a, b, weighting)[:, 1]), (shape, weighting)


@pytest.mark.parametrize("shape", [(1, 1, 16, 16), (2, 3, 17, 19)])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_scales_are_the_numpy_loop(shape, weighting):
    x, y = pair64(shape, sum(shape))
    got = S.ms_scales_torch(x, y, weighting)
    want = numpy_scales(x.numpy(), y.numpy(), weighting)
    assert got.dtype == torch.float64 and got.shape == (shape[0], 5)
    assert np.abs(got.numpy() - want).max() <= 1e-12
    ms = np.prod(np.maximum(want, 0) ** np.array(S.BETAS), axis=1)
    assert np.abs(S.ms_loss_terms(x, y, weighting)[:, 1].numpy() - ms).max() <= 1e-12
    assert np.abs(S.ms_product(got).numpy() - ms).max() <= 1e-12


def test_betas_and_pool_are_the_written_order():
    assert S.BETAS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    t = torch.rand((2, 3, 7, 9), generator=torch.Generator().manual_seed(1))
    p = S.pool(t)
    assert p.shape == (2, 3, 3, 4) and p.dtype == torch.float32        # the odd last row and column are dropped
    for j in range(3):
        for i in range(4):
            want = ((t[:, :, 2 * j, 2 * i] + t[:, :, 2 * j, 2 * i + 1])
                    + (t[:, :, 2 * j + 1, 2 * i] + t[:, :, 2 * j + 1, 2 * i + 1])) * 0.25
            assert torch.equal(p[:, :, j, i], want)
    assert S.pool(t.double()).dtype == torch.float64


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_identical_frames_give_one(weighting):
    x, _ = pair64((2, 3, 17, 40), 5)
    for t in (x.float(),):
        m = S.ms_metrics(t, t.clone(), weighting)
        assert m.dtype == torch.float64 and m.shape == (2, 2)
        assert torch.equal(m[:, 0], torch.zeros(2, dtype=torch.float64))
        assert (m[:, 1] - 1).abs().max().item() <= 1e-12
        assert (S.ms_scales_torch(t, t, weighting) - 1).abs().max().item() <= 1e-12


def test_clamped_frame_gives_zero_and_a_zero_gradient():
    x, _ = pair64((2, 2, 17, 19), 9)
    y = (1 - x).requires_grad_()
    assert bool((S.ms_scales_torch(x, y.detach()) <= 0).any(dim=1).all())     # the clamp is active on both frames
    terms = S.ms_loss_terms(x, y)
    assert torch.equal(terms[:, 1].detach(), torch.zeros(2, dtype=torch.float64))
    terms[:, 1].sum().backward()
    assert torch.isfinite(y.grad).all() and torch.equal(y.grad, torch.zeros_like(y.grad))
    y.grad = None
    S.ms_loss_terms(x, y).sum().backward()                                    # the MSE part alone is left
    assert torch.isfinite(y.grad).all() and y.grad.abs().max().item() > 0
    gout = torch.tensor([[0.0, 1.0]] * 2, dtype=torch.float64)
    assert torch.equal(S.ms_backward_torch(x, y.detach(), gout), torch.zeros_like(x))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_gradcheck_of_ms_loss_terms(weighting):
    x, y = pair64((1, 2, 17, 19), 3)
    x.requires_grad_()
    y.requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: S.ms_loss_terms(a, b, weighting), (x, y))


@pytest.mark.parametrize("shape", [(2, 3, 17, 19), (1, 1, 64, 128), (3, 1, 37, 70)])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_explicit_chain_is_torch_autograd(shape, weighting):
    x, y = pair64(shape, sum(shape) + 7)
    x.requires_grad_()
    y.requires_grad_()
    gout = gout_of(shape[0], sum(shape))
    terms = S.ms_loss_terms(x, y, weighting)
    assert terms.dtype == torch.float64 and terms.shape == (shape[0], 2) and terms.requires_grad
    (terms * gout).sum().backward()
    gy = S.ms_backward_torch(x, y, gout, weighting, dt=torch.float64)
    gx = S.ms_backward_torch(y, x, gout, weighting, dt=torch.float64)      # the swapped call
    assert gy.dtype == torch.float64 and gy.shape == shape
    scale = max(x.grad.abs().max().item(), y.grad.abs().max().item())
    dy, dx = (gy - y.grad).abs().max().item(), (gx - x.grad).abs().max().item()
    print("explicit chain vs autograd %s %s: %.3g %.3g of the largest gradient" % (shape, weighting, dy / scale, dx / scale))
    assert dy <= 1e-12 * scale and dx <= 1e-12 * scale


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_loss_values_are_ms_metrics(weighting):
    for shape in [(1, 1, 16, 16), (2, 3, 17, 19), (1, 2, 33, 65)]:
        x, y = (t.float() for t in pair64(shape, sum(shape) + 3))
        want = S.ms_metrics(x, y, weighting)
        got = S.ms_loss_terms(x, y.clone().requires_grad_(), weighting)
        assert got.requires_grad and got.device.type == "cpu" and not want.requires_grad
        assert torch.equal(got.detach(), want)
        assert torch.equal(want[:, 0], S.metrics(x, y, weighting)[:, 0])            # the WS-MSE of `metrics`
        assert torch.equal(S.ws_ms_ssim(x, y, weighting), want[:, 1])
        assert torch.equal(want[:, 1], S.ms_product(S.ms_scales_torch(x, y, weighting)))


def test_uint8_form_is_the_float_form():
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 256, (2, 20, 33, 3), generator=g, dtype=torch.uint8)
    v = (u.int() + torch.randint(-20, 20, u.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    f = lambda t: (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    assert torch.equal(S.ms_metrics(u, v), S.ms_metrics(f(u), f(v)))


def test_refusals():
    x, y = (t.float() for t in pair64((1, 3, 16, 32), 5))
    u = torch.zeros((1, 16, 32, 3), dtype=torch.uint8)
    for fn in (S.ms_metrics, S.ms_loss_terms, S.ms_scales_torch):
        for a, b in ((x[:, :, :15], y[:, :, :15]), (x[..., :15], y[..., :15])):      # h or w of 15
            with pytest.raises(PconvError, match="h and w must be at least 16"):
                fn(a, b)
        with pytest.raises(PconvError):
            fn(x, y[:, :, :, :31])                              # unequal shapes
        with pytest.raises(PconvError):
            fn(x, y.double())                                   # unequal types
        with pytest.raises(PconvError):
            fn(x[0], y[0])                                      # not a batch
        with pytest.raises(ValueError):
            fn(x, y, "s-psnr")                                  # unknown weighting
    with pytest.raises(PconvError):
        S.ms_metrics(u[:, :15], u[:, :15])
    with pytest.raises(PconvError):
        S.ms_loss_terms(u, u)                                   # uint8 batches carry no gradient
    with pytest.raises(ValueError):
        S.ms_backward_torch(x, y, torch.ones(1, 2), "s-psnr")
    with pytest.raises(PconvError):
        S.ms_backward_torch(x, y, torch.ones(2, 2))             # gout of another batch
    with pytest.raises(PconvError, match="at least 16"):
        S.ms_backward_torch(x[..., :15], y[..., :15], torch.ones(1, 2))


def test_cli_ms_ssim_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    """the existing --ws drive is unchanged without --ms-ssim (drive_ws asserts its lines and rows); with it, one
    more line per image and for the average and one more column, the float64 path's value on the written PNGs"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_sphere_metrics_cpu import drive_ws
    rows, images = drive_ws(tmp_path, monkeypatch, capsys, "cpu", [(256, 512)])
    capsys.readouterr()
    PC.main(["--test", "--ws", "--code-list", "ws0.pcv", "--img-list", "ws0.png"])
    plain = capsys.readouterr().out
    assert "WS-MS-SSIM" not in plain
    ms_rows = PC.decoding_and_test(["ws0.pcv"], ["ws0.png"], 3, False, 0, ws=True, ms_ssim=True)
    capsys.readouterr()
    PC.main(["--test", "--ws", "--ms-ssim", "--code-list", "ws0.pcv", "--img-list", "ws0.png"])
    out = capsys.readouterr().out
    found = re.findall(r"^( ?)WS-MS-SSIM:([0-9.]+)$", out, flags=re.M)
    assert [f[0] for f in found] == [" ", ""]                   # per image (indented), then the average block
    assert out.index("Average Performance") < out.rindex("WS-MS-SSIM:")
    assert [l for l in out.splitlines() if "WS-MS-SSIM" not in l] == plain.splitlines()   # every other line as before
    (src, dec), row = images[0], ms_rows[0]
    assert len(ms_rows) == 1 and len(row) == 6 and row[:5] == rows[0]
    want = S.ws_ms_ssim(torch.from_numpy(src)[None], torch.from_numpy(dec)[None])[0].item()
    assert abs(row[5] - want) <= 1e-5 and 0 < row[5] < 1
    assert all(abs(float(f[1]) - want) <= 1e-5 + 5e-5 for f in found)      # as printed: four decimals
    with pytest.raises(AssertionError, match="--ms-ssim needs --ws"):
        PC.main(["--test", "--ms-ssim", "--code-list", "ws0.pcv", "--img-list", "ws0.png"])


def test_train_with_the_ws_ms_loss_on_the_cpu(oracle_backend, tmp_path, monkeypatch):
    """--loss ws-ms --device cpu for two steps: finishes, logs finite mse / ms-ssim / rate, constructs no
    MultiProject (and no SSIM module), and calls ms_loss_terms"""
    import torch.distributed as dist
    from pseudocylindrical_convolution_amd import train

    def refuse(*a, **k):
        raise AssertionError("--loss ws-ms must not construct the viewport loss")

    calls = []
    real = S.ms_loss_terms
    monkeypatch.setattr(train, "MultiProject", refuse)
    monkeypatch.setattr(train, "SSIM", refuse)
    monkeypatch.setitem(train.SPHERE_LOSSES, "ws-ms", lambda a, b: calls.append(a.shape) or real(a, b))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(37000 + os.getpid() % 2000), RANK="0", WORLD_SIZE="1")
    args = train.build_parser().parse_args(
        ["--device", "cpu", "--loss", "ws-ms", "--synthetic", "2", "--height", "256", "--width", "512", "--batch-size", "1",
         "--test-batch-size", "1", "--acc-batch", "1", "--epochs", "1", "--max-steps", "2", "--valid-dim", "8",
         "--channels", "16", "--code-dim", "16", "--workers", "0", "--no-opt", "--mean", "0", "--beta", "0.1",
         "--alpha", "0.05", "--base-dir", str(tmp_path)])
    try:
        hist = train.Job(0, 1, args)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(hist) == 1 and len(calls) >= 3                          # two training steps and the test set
    (loss, mse, ssim, rate), ls = hist[0]
    assert all(np.isfinite(v) for v in (loss, mse, ssim, rate)) and mse > 0 and 0 <= ssim <= 1 and rate > 0
    assert len(ls) == 1 and np.isfinite(ls[0]) and ls[0] > 0           # gamma·mse + beta·(1 - ms-ssim) + alpha·rate
    log = open(os.path.join(str(tmp_path), "save_models", "ent_normal_16_8_16_logs_0.txt")).read()
    assert log.count("Train Epoch: 1") == 2 and "Test set:" in log and "nan" not in log.lower()
    assert "WS-MSE / WS-MS-SSIM" in log
    assert train.build_parser().parse_args([]).loss == "viewport"      # the default stays
