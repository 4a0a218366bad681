"""GPU: WS-MSE / WS-SSIM as a training loss (csrc/sphere_metrics.hip: ms_backward_kernel, one scale).  The HIP kernel
against the float64 statement of the gradient (sphere_metrics.backward_torch) within a bound taken from the float32
statement's own error, the pure MSE part bit for bit, batching and repeat determinism, the autograd entry
(sphere_metrics.loss_terms), refused arguments, and a few training steps on the loss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the smallest shapes at which tiling (32 x 64), halo (10) and window (11) handling can go wrong
SHAPES = [
    (1, 1, 1, 1),      # single pixel
    (2, 3, 5, 3),      # frame smaller than the window
    (1, 2, 13, 17),    # odd sides below one tile
    (1, 1, 64, 128),   # whole 32 x 64 tiles
    (1, 3, 33, 65),    # one row and one column past a tile edge
    (3, 1, 37, 70),    # several frames with a remainder
    (1, 3, 75, 150),   # several tiles on both axes with remainders
]
HALF_FLAT = "half-flat"   # (1, 1, 64, 128) whose upper half is the constant 0.5 in both pictures: B2 ~ C2
CASES = SHAPES + [HALF_FLAT]
WEIGHTINGS = ["ws", "uniform"]
GOUTS = ["random", "mse", "ssim"]


def inputs(case):
    """x = rand, y = x + 0.1·randn, neither clamped (float32, CPU)"""
    shape = (1, 1, 64, 128) if case == HALF_FLAT else case
    g = torch.Generator().manual_seed(sum(shape) + (100 if case == HALF_FLAT else 0))
    x = torch.rand(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    if case == HALF_FLAT:
        x[:, :, :32] = 0.5
        y[:, :, :32] = 0.5
    return x, y


def gout_of(n, kind):
    if kind == "mse":
        return torch.tensor([[1.0, 0.0]] * n, dtype=torch.float64)
    if kind == "ssim":
        return torch.tensor([[0.0, 1.0]] * n, dtype=torch.float64)
    v = torch.randn((n, 2), generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    return v + torch.sign(v) * 0.25


_twins = {}


def twins(case, weighting, kind):
    """(x, y, gout, float64 twin, e32, G) of a case, computed once on the CPU and shared"""
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    key = (case, weighting, kind)
    if key not in _twins:
        x, y = inputs(case)
        gout = gout_of(x.shape[0], kind)
        g64 = S.backward_torch(x, y, gout, weighting, dt=torch.float64)
        g32 = S.backward_torch(x, y, gout, weighting, dt=torch.float32)
        _twins[key] = (x, y, gout, g64, (g32.double() - g64).abs().max().item(), g64.abs().max().item())
    return _twins[key]


def run_kernel(x, y, gout, weighting):
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV.ws_metrics_backward(x.to(DEV), y.to(DEV), gout.to(DEV), weighting)


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_kernel_is_the_float64_twin(hip_backend, case, weighting):
    """within 8·e32 + 1e-6·G of backward_torch(dt=float64), e32 the float32 statement's own error against it and G
    the largest gradient: the kernel sums each 11-tap filter with fmaf where torch adds rounded products, and rounds
    ks and km once.  An error of structure (halo, tap, weight, tile edge) shows at 1e-2·G"""
    for kind in GOUTS:
        x, y, gout, g64, e32, G = twins(case, weighting, kind)
        got = run_kernel(x, y, gout, weighting)
        assert got.dtype == torch.float32 and got.shape == x.shape and got.device.type == "cuda"
        got = got.cpu()
        assert torch.isfinite(got).all()
        err = (got.double() - g64).abs().max().item()
        print("ws backward %s %s %s: G %.3g e32/G %.3g err/G %.3g err/e32 %.3g"
              % (case, weighting, kind, G, e32 / G, err / G, err / e32 if e32 > 0 else 0.0))
        assert err <= 8 * e32 + 1e-6 * G, (case, weighting, kind, err, e32, G)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_pure_mse_part_is_exact(hip_backend, weighting):
    """gout = (1, 0): float32(2·w_j / N)·(y - x) in float32 torch on the device, bit for bit"""
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    for shape in SHAPES:
        x, y = inputs(shape)
        n, c, h, w = shape
        got = run_kernel(x, y, gout_of(n, "mse"), weighting)
        wr = S.weights(h, weighting)
        km = (2.0 * wr / (c * w * float(wr.sum()))).float().view(1, 1, h, 1).to(DEV)
        want = km * (y.to(DEV) - x.to(DEV))
        assert torch.equal(got, want), (shape, (got - want).abs().max().item())


def test_same_bits_again_and_alone(hip_backend):
    x, y = inputs((3, 1, 37, 70))
    gout = gout_of(3, "random")
    batch = run_kernel(x, y, gout, "ws")
    assert torch.equal(batch, run_kernel(x, y, gout, "ws"))
    for k in range(3):
        alone = run_kernel(x[k:k + 1].contiguous(), y[k:k + 1].contiguous(), gout[k:k + 1].contiguous(), "ws")
        assert torch.equal(alone, batch[k:k + 1])


def test_autograd_entry(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, sphere_metrics as S
    from pseudocylindrical_convolution_amd._native import PconvError
    x, y = (t.to(DEV) for t in inputs((3, 1, 37, 70)))
    y.requires_grad_()
    terms = S.loss_terms(x, y)
    assert terms.dtype == torch.float64 and terms.shape == (3, 2) and terms.device == y.device and terms.requires_grad
    assert torch.equal(terms.detach().cpu(), S.metrics(x, y.detach()))
    terms.sum().backward()
    assert x.grad is None and y.grad is not None and y.grad.shape == y.shape and torch.isfinite(y.grad).all()
    ones = torch.ones((3, 2), dtype=torch.float64, device=DEV)
    assert torch.equal(y.grad, PCONV.ws_metrics_backward(x, y.detach(), ones, "ws"))
    # both inputs: the gradient of x is the swapped call
    xb, yb = x.clone().requires_grad_(), y.detach().clone().requires_grad_()
    gout = gout_of(3, "random").to(DEV)
    (S.loss_terms(xb, yb, "uniform") * gout).sum().backward()
    assert torch.equal(xb.grad, PCONV.ws_metrics_backward(yb.detach(), xb.detach(), gout, "uniform"))
    assert torch.equal(yb.grad, PCONV.ws_metrics_backward(xb.detach(), yb.detach(), gout, "uniform"))
    # a non-contiguous upstream gradient
    yc = y.detach().clone().requires_grad_()
    up = torch.stack([gout[:, 1], gout[:, 0]]).t()            # (3, 2) with strides (1, 3)
    assert not up.is_contiguous()
    S.loss_terms(x, yc).backward(up)
    assert torch.equal(yc.grad, PCONV.ws_metrics_backward(x, yc.detach(), up.contiguous(), "ws"))
    # uint8 frames carry no gradient
    u = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(PconvError):
        S.loss_terms(u, u)
    with pytest.raises(PconvError):
        PCONV.ws_metrics_backward(u, u, ones[:1].contiguous())
    with pytest.raises(PconvError):
        PCONV.ws_metrics_backward(x, y.detach(), ones.float())            # gout must be float64
    with pytest.raises(PconvError):
        PCONV.ws_metrics_backward(x, y.detach(), ones.cpu())              # ... on the inputs' device
    with pytest.raises(PconvError):
        PCONV.ws_metrics_backward(x, y.detach(), ones, "s-psnr")


def test_refusals_of_the_native_entry(hip_backend):
    """each returns -1 with a message, before any launch (the pointers are never dereferenced)"""
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    dummy = 4096
    bad = [
        (None, dummy, dummy, 1, 1, 8, 8, 0, dummy, b"null pointer"),
        (dummy, None, dummy, 1, 1, 8, 8, 0, dummy, b"null pointer"),
        (dummy, dummy, None, 1, 1, 8, 8, 0, dummy, b"null pointer"),
        (dummy, dummy, dummy, 1, 1, 8, 8, 0, None, b"null pointer"),
        (dummy, dummy, dummy, 1, 1, 8, 8, 2, dummy, b"unknown weighting"),
        (dummy, dummy, dummy, 0, 1, 8, 8, 0, dummy, b"frame count"),
        (dummy, dummy, dummy, 1, 4097, 8, 8, 0, dummy, b"channel count"),
        (dummy, dummy, dummy, 1, 1, 0, 8, 0, dummy, b"frame size"),
        (dummy, dummy, dummy, 1, 1, 16384, 32768, 0, dummy, b"2^31 bytes"),
    ]
    for case in bad:
        rc = lib.pconv_ws_metrics_backward_f32(*case[:9], None)
        assert rc == -1 and b"ws_metrics_backward" in lib.pconv_last_error() and case[9] in lib.pconv_last_error(), case


def test_training_steps_on_the_ws_loss(hip_backend):
    """CMPNetV2MF at the benchmark's width on 256 x 512: mean WS-MSE + 0.1·(1 - mean WS-SSIM) + 0.05·rate; every
    parameter gets a finite gradient through the backward kernel and five Adam steps lower the loss"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, sphere_metrics as S
    torch.manual_seed(0)
    net = Z.CMPNetV2MF(56, 192, 192, 16, 8, True, False, 0).to(DEV)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    x = torch.rand(2, 3, 256, 512, generator=torch.Generator().manual_seed(3)).to(DEV)
    losses = []
    for it in range(5):
        y, ent, mask = net(x)
        terms = S.loss_terms(x, y)
        loss = terms[:, 0].mean() + 0.1 * (1 - terms[:, 1].mean()) + 0.05 * torch.sum(ent) / torch.sum(mask).item()
        opt.zero_grad()
        loss.backward()
        if it == 0:
            missing = [n for n, p in net.named_parameters() if p.grad is None]
            assert not missing, missing
            assert all(torch.isfinite(p.grad).all().item() for p in net.parameters())
            assert net.encoder.net[0].conv1.weight.grad.abs().max().item() > 0
        opt.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
