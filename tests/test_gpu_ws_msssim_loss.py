"""GPU: WS-MSE / WS-MS-SSIM as a training loss (csrc/sphere_metrics.hip: ms_backward_kernel, one launch per scale).  The
kernels against the float64 statement of the gradient chain (sphere_metrics.ms_backward_torch) within a bound taken
from the float32 statement's own error, the pure MSE part bit for bit against the single-scale backward, batching
and repeat determinism, the autograd entry (sphere_metrics.ms_loss_terms), the clamped frame, refused arguments, and
a few training steps on the loss."""
import numpy as np
import pytest
import torch

from test_gpu_ws_msssim import CASES, DEV, SHAPES, WEIGHTINGS, inputs

pytestmark = pytest.mark.gpu
GOUTS = ["random", "mse", "ms"]


def gout_of(n, kind):
    if kind == "mse":
        return torch.tensor([[1.0, 0.0]] * n, dtype=torch.float64)
    if kind == "ms":
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
        g64 = S.ms_backward_torch(x, y, gout, weighting, dt=torch.float64)
        g32 = S.ms_backward_torch(x, y, gout, weighting, dt=torch.float32)
        _twins[key] = (x, y, gout, g64, (g32.double() - g64).abs().max().item(), g64.abs().max().item())
    return _twins[key]


def run_kernels(x, y, gout, weighting):
    """the forward (whose pyramid and values the backward reads), then the backward"""
    from pseudocylindrical_convolution_amd import PCONV
    x, y = x.to(DEV), y.to(DEV)
    values, workspace = PCONV.ws_msssim_device(x, y, weighting)
    return PCONV.ws_msssim_backward(x, y, workspace, values, gout.to(DEV), weighting)


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_kernels_are_the_float64_twin(hip_backend, case, weighting):
    """within 8·e32 + 1e-6·G of ms_backward_torch(dt=float64), e32 the float32 statement's own error against it and G
    the largest gradient (the rule and its margin are those of the single-scale loss test).  e32 / G is 1e-6..1.4e-5
    here, so an error of structure (halo, tap, dropped row, upsample index, wrong β) shows at 1e-2·G"""
    for kind in GOUTS:
        x, y, gout, g64, e32, G = twins(case, weighting, kind)
        got = run_kernels(x, y, gout, weighting)
        assert got.dtype == torch.float32 and got.shape == x.shape and got.device.type == "cuda"
        got = got.cpu()
        assert torch.isfinite(got).all()
        err = (got.double() - g64).abs().max().item()
        print("ws-ms backward %s %s %s: G %.3g e32/G %.3g err/G %.3g err/e32 %.3g"
              % (case, weighting, kind, G, e32 / G, err / G, err / e32 if e32 > 0 else 0.0))
        assert err <= 8 * e32 + 1e-6 * G, (case, weighting, kind, err, e32, G)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_pure_mse_part_is_the_single_scale_backward(hip_backend, weighting):
    """gout = (1, 0): the bits of ws_metrics_backward, float32(2·w_j / N)·(y - x)"""
    from pseudocylindrical_convolution_amd import PCONV
    for shape in SHAPES:
        x, y = inputs(shape)
        gout = gout_of(shape[0], "mse")
        got = run_kernels(x, y, gout, weighting)
        want = PCONV.ws_metrics_backward(x.to(DEV), y.to(DEV), gout.to(DEV), weighting)
        assert torch.equal(got, want), (shape, (got - want).abs().max().item())


def test_same_bits_again_alone_and_in_a_batch(hip_backend):
    x, y = inputs((3, 1, 37, 70))
    gout = gout_of(3, "random")
    batch = run_kernels(x, y, gout, "ws")
    assert torch.equal(batch, run_kernels(x, y, gout, "ws"))
    for k in range(3):
        alone = run_kernels(x[k:k + 1].contiguous(), y[k:k + 1].contiguous(), gout[k:k + 1].contiguous(), "ws")
        assert torch.equal(alone, batch[k:k + 1])


def test_autograd_entry(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, sphere_metrics as S
    from pseudocylindrical_convolution_amd._native import PconvError
    x, y = (t.to(DEV) for t in inputs((3, 1, 37, 70)))
    y.requires_grad_()
    terms = S.ms_loss_terms(x, y)
    assert terms.dtype == torch.float64 and terms.shape == (3, 2) and terms.device == y.device and terms.requires_grad
    assert torch.equal(terms.detach().cpu(), S.ms_metrics(x, y.detach()))
    terms.sum().backward()
    assert x.grad is None and y.grad is not None and y.grad.shape == y.shape and torch.isfinite(y.grad).all()
    ones = torch.ones((3, 2), dtype=torch.float64, device=DEV)
    assert torch.equal(y.grad, run_kernels(x, y.detach(), ones, "ws"))
    # both inputs: the gradient of x is the swapped call on the same workspace, and the bits of a forward of (y, x)
    xb, yb = x.clone().requires_grad_(), y.detach().clone().requires_grad_()
    gout = gout_of(3, "random").to(DEV)
    (S.ms_loss_terms(xb, yb, "uniform") * gout).sum().backward()
    values, workspace = PCONV.ws_msssim_device(xb.detach(), yb.detach(), "uniform")
    assert torch.equal(xb.grad, PCONV.ws_msssim_backward(yb.detach(), xb.detach(), workspace, values, gout, "uniform",
                                                         swapped=True))
    assert torch.equal(xb.grad, run_kernels(yb.detach(), xb.detach(), gout, "uniform"))
    assert torch.equal(yb.grad, run_kernels(xb.detach(), yb.detach(), gout, "uniform"))
    # a non-contiguous upstream gradient
    yc = y.detach().clone().requires_grad_()
    up = torch.stack([gout[:, 1], gout[:, 0]]).t()            # (3, 2) with strides (1, 3)
    assert not up.is_contiguous()
    S.ms_loss_terms(x, yc).backward(up)
    assert torch.equal(yc.grad, run_kernels(x, yc.detach(), up.contiguous(), "ws"))
    # refusals
    u = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(PconvError):
        S.ms_loss_terms(u, u)                                              # uint8 frames carry no gradient
    with pytest.raises(PconvError, match="at least 16"):
        S.ms_loss_terms(x[:, :, :15].contiguous(), y.detach()[:, :, :15].contiguous())
    yd = y.detach()
    values, workspace = PCONV.ws_msssim_device(x, yd)
    with pytest.raises(PconvError):
        PCONV.ws_msssim_backward(x, yd, workspace, values, ones.float())                # gout must be float64
    with pytest.raises(PconvError):
        PCONV.ws_msssim_backward(x, yd, workspace, values, ones.cpu())                  # ... on the inputs' device
    with pytest.raises(PconvError):
        PCONV.ws_msssim_backward(x, yd, workspace, values, ones, "s-psnr")
    with pytest.raises(PconvError):
        PCONV.ws_msssim_backward(x, yd, workspace[:-8], values, ones)                   # another frame's workspace
    with pytest.raises(PconvError):
        PCONV.ws_msssim_backward(x, yd, workspace, values[:, :2].contiguous(), ones)    # not the forward's values
    uw = PCONV.ws_msssim_device(u, u)
    with pytest.raises(PconvError):
        PCONV.ws_msssim_backward(u, u, uw[1], uw[0], ones[:1].contiguous())             # uint8


def test_clamped_frame_has_a_zero_ms_gradient(hip_backend):
    """y = 1 - x: WS-MS-SSIM is 0 and its gradient all zeros and finite; the MSE part is untouched"""
    from pseudocylindrical_convolution_amd import PCONV, sphere_metrics as S
    x, _ = (t.to(DEV) for t in inputs((2, 3, 17, 19)))
    y = (1 - x).contiguous().requires_grad_()
    terms = S.ms_loss_terms(x, y)
    assert torch.equal(terms[:, 1].detach().cpu(), torch.zeros(2, dtype=torch.float64))
    terms[:, 1].sum().backward()
    assert torch.isfinite(y.grad).all() and torch.equal(y.grad, torch.zeros_like(y.grad))
    both = run_kernels(x, y.detach(), gout_of(2, "random"), "ws")
    mse_only = gout_of(2, "random")
    mse_only[:, 1] = 0
    assert torch.isfinite(both).all()
    assert torch.equal(both, PCONV.ws_metrics_backward(x, y.detach(), mse_only.to(DEV), "ws"))


def test_refusals_of_the_native_entry(hip_backend):
    """each returns -1 with a message, before any launch (the pointers are never dereferenced)"""
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    d = 4096
    ok = [d, d, d, d, d, 1, 1, 16, 16, 0, 0, d, d]
    bad = [({k: None}, b"null pointer") for k in (0, 1, 2, 3, 4, 11, 12)] + [
        ({2: d + 4}, b"misaligned"),
        ({9: 2}, b"unknown weighting"),
        ({10: 2}, b"swapped"),
        ({5: 0}, b"frame count"),
        ({6: 4097}, b"channel count"),
        ({7: 0}, b"frame size"),
        ({7: 15}, b"h and w must be at least 16"),
        ({8: 15}, b"h and w must be at least 16"),
        ({7: 16384, 8: 32768}, b"2^31 bytes"),
    ]
    for change, message in bad:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        rc = lib.pconv_ws_msssim_backward_f32(*args, None)
        assert rc == -1 and b"ws_msssim_backward" in lib.pconv_last_error() and message in lib.pconv_last_error(), change


def test_training_steps_on_the_ws_ms_loss(hip_backend):
    """CMPNetV2MF at the benchmark's width on 256 x 512: mean WS-MSE + 0.1·(1 - mean WS-MS-SSIM) + 0.05·rate; every
    parameter gets a finite gradient through the backward kernels and five Adam steps lower the loss"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, sphere_metrics as S
    torch.manual_seed(0)
    net = Z.CMPNetV2MF(56, 192, 192, 16, 8, True, False, 0).to(DEV)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    x = torch.rand(2, 3, 256, 512, generator=torch.Generator().manual_seed(3)).to(DEV)
    losses = []
    for it in range(5):
        y, ent, mask = net(x)
        terms = S.ms_loss_terms(x, y)
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
