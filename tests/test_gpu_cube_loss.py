"""GPU: training on cube pictures (csrc/cube.hip: cube_pad_backward_f32_kernel; csrc/sphere_metrics.hip: ms_backward_kernel
with the per-pixel factor of pconv_weighted_ssim_backward_f32).  The face continuation's backward against its torch twin
bit for bit; the weighted SSIM's backward against the float64 statement within the bound of tests/test_gpu_sphere_loss.py;
batching and repeat determinism; the autograd entries against the direct kernel calls; stale memory; a few training steps."""
import argparse

import numpy as np
import pytest
import torch

import cube_loss_cases as L
import stale_memory as SM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- 1. pad_backward: kernel == twin, bit for bit ----

@pytest.mark.parametrize("case", L.pad_cases(L.GPU_FACES), ids=L.pad_id)
def test_pad_backward_is_its_twin(hip_backend, case):
    from pseudocylindrical_convolution_amd import cube
    kind, a, depth = case
    A = a + 2 * depth
    table, lists = cube.pad_table_on(kind, a, None, depth), cube.pad_reverse_lists(kind, a, depth)
    for n, c in L.PLANES:
        g = L.gradient(n, c, 6 * A, A, seed=7 * a + depth + c)
        want = cube.pad_backward_torch(g, table, lists, a, depth)
        got = cube.pad_backward(g.to(DEV), kind, a, depth)
        assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (n, c, 6 * a, a)
        assert torch.equal(got.cpu(), want), (case, n, c, (got.cpu() - want).abs().max().item())
        assert torch.equal(got, cube.pad_backward(g.to(DEV), kind, a, depth))                      # again
        for k in range(n):                                                                          # a frame alone
            assert torch.equal(cube.pad_backward(g[k:k + 1].contiguous().to(DEV), kind, a, depth), got[k:k + 1])


def test_pad_with_grad_gives_the_same_bits_on_both_devices(hip_backend):
    from pseudocylindrical_convolution_amd import cube
    for kind, a, depth in (("cmp", 7, 3), ("eac", 12, 5)):
        A = a + 2 * depth
        y = L.frames(2, 3, 6 * a, a, seed=a)
        g = L.gradient(2, 3, 6 * A, A, seed=a + 1)
        grads = []
        for dev in ("cpu", DEV):
            leaf = y.to(dev).requires_grad_(True)
            out = cube.pad(leaf, kind, depth, grad=True)
            assert out.requires_grad and torch.equal(out.detach(), cube.pad(leaf.detach(), kind, depth))
            grads.append(torch.autograd.grad(out, leaf, g.to(dev))[0].cpu())
        assert torch.equal(grads[0], grads[1])


# ---- 2. ssim_backward: the rule of tests/test_gpu_sphere_loss.py ----

def _ssim_kernel(x, y, plane, gout):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    return WM.ssim_backward(x.to(DEV), y.to(DEV), plane, gout.to(DEV))


@pytest.mark.parametrize("case", L.SSIM_CASES, ids=L.ssim_id)
def test_ssim_backward_is_the_float64_twin(hip_backend, case):
    """within 8 e32 + 1e-6 G of ssim_backward_torch(dt=float64), e32 the float32 statement's own error against it and G the
    largest gradient: the kernel sums each 11-tap filter with fmaf where torch adds rounded products.  An error of
    structure (halo, tap, weight, tile edge) shows at 1e-2 G"""
    x, y, plane, gout, g64, e32, G = L.ssim_twins(case)
    got = _ssim_kernel(x, y, plane, gout)
    assert got.dtype == torch.float32 and got.shape == x.shape and got.device.type == "cuda"
    got = got.cpu()
    assert torch.isfinite(got).all()
    err = (got.double() - g64).abs().max().item()
    print("weighted ssim backward %s: G %.3g e32/G %.3g err/G %.3g err/e32 %.3g"
          % (L.ssim_id(case), G, e32 / G, err / G, err / e32 if e32 > 0 else 0.0))
    assert err <= 8 * e32 + 1e-6 * G, (case, err, e32, G)
    if case[1] == "zero-block" and case[0][2] >= 37:
        r0, r1, c0, c1 = L.zero_block(*case[0][2:])
        assert (got[:, :, r0 + 5:r1 - 5, c0 + 5:c1 - 5] == 0).all() and (got[:, :, r0:r0 + 5, c0:c1] != 0).any()


def test_ssim_backward_same_bits_again_and_alone(hip_backend):
    case = ((3, 1, 37, 70), "zero-block")
    x, y, plane, gout, _, _, _ = L.ssim_twins(case)
    batch = _ssim_kernel(x, y, plane, gout)
    assert torch.equal(batch, _ssim_kernel(x, y, plane, gout))
    for k in range(3):
        alone = _ssim_kernel(x[k:k + 1].contiguous(), y[k:k + 1].contiguous(), plane, gout[k:k + 1].contiguous())
        assert torch.equal(alone, batch[k:k + 1])
    # a plane's result depends on its own gout alone: channels apart
    x, y, plane, gout, _, _, _ = L.ssim_twins(((1, 3, 33, 65), "random"))
    batch = _ssim_kernel(x, y, plane, gout)
    for c in range(3):
        alone = _ssim_kernel(x[:, c:c + 1].contiguous(), y[:, c:c + 1].contiguous(), plane, gout[:, c:c + 1].contiguous())
        assert torch.equal(alone, batch[:, c:c + 1])


# ---- 3. the autograd entries against the direct kernel calls ----

def test_ssim_loss_terms(hip_backend):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    from pseudocylindrical_convolution_amd._native import PconvError
    x, y, plane, _, _, _, _ = L.ssim_twins(((1, 3, 33, 65), "zero-block"))
    x, y = x.to(DEV), y.to(DEV).requires_grad_(True)
    terms = WM.ssim_loss_terms(x, y, plane)
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (1,) and terms.device == y.device and terms.requires_grad
    assert torch.equal(terms.detach(), WM.channel_mean(WM.ssim_device(x, y.detach(), plane)))
    up = torch.tensor([0.75], dtype=torch.float64, device=DEV)
    terms.backward(up)
    share = (up / torch.full((), 3.0, dtype=torch.float64, device=DEV))[:, None].expand(1, 3).contiguous()
    assert x.grad is None and torch.equal(y.grad, WM.ssim_backward(x, y.detach(), plane, share))
    xb, yb = x.clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    WM.ssim_loss_terms(xb, yb, plane).backward(up)
    assert torch.equal(yb.grad, y.grad) and torch.equal(xb.grad, WM.ssim_backward(yb.detach(), xb.detach(), plane, share))
    u8 = torch.zeros((1, 33, 65, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(PconvError, match="uint8"):
        WM.ssim_loss_terms(u8, u8, plane)
    for fn in (WM.ssim, WM.ssim_device):
        with pytest.raises(PconvError, match="requires grad"):
            fn(x, y, plane)
    with pytest.raises(PconvError, match="gout"):
        WM.ssim_backward(x, y.detach(), plane, share.float())


@pytest.mark.parametrize("kind", L.KINDS)
def test_cube_ws_ssim_loss_terms(hip_backend, kind):
    from pseudocylindrical_convolution_amd import cube, weighted_metrics as WM
    from pseudocylindrical_convolution_amd._native import PconvError
    a, n, c = 12, 2, 2
    sp = cube.spec(kind, "3x2")
    x = L.frames(n, c, 2 * a, 3 * a, seed=41).to(DEV)
    y = (x + 0.1 * L.gradient(n, c, 2 * a, 3 * a, seed=42).to(DEV)).requires_grad_(True)
    terms = cube.ws_ssim_loss_terms(x, y, sp)
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (n,) and terms.device == y.device
    assert torch.equal(terms.detach().cpu(), cube.ws_ssim(x, y.detach(), sp))
    up = torch.tensor([1.0, -0.5], dtype=torch.float64, device=DEV)
    terms.backward(up)
    stacks = [cube.pad(cube.unpack(t.detach(), "3x2").contiguous(), kind, cube.SSIM_PAD) for t in (x, y)]
    share = (up / torch.full((), float(c), dtype=torch.float64, device=DEV))[:, None].expand(n, c).contiguous()
    g_stack = WM.ssim_backward(stacks[0], stacks[1], cube.ssim_plane(kind, a), share)
    assert torch.equal(y.grad, cube.pack(cube.pad_backward(g_stack, kind, a, cube.SSIM_PAD), "3x2"))
    A = a + 2 * cube.SSIM_PAD
    ring = g_stack.reshape(n, c, 6, A, A).clone()
    ring[:, :, :, 5:5 + a, 5:5 + a] = 0
    assert ring.abs().max().item() > 1e-3 * g_stack.abs().max().item()      # the rings weigh zero and carry a gradient
    with pytest.raises(PconvError, match="requires grad"):
        cube.ws_ssim(x, y, sp)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("ss", [1, 2])
def test_cube_to_erp_with_grad(hip_backend, kind, ss):
    from pseudocylindrical_convolution_amd import PCONV, cube, viewport
    from pseudocylindrical_convolution_amd._native import PconvError
    a, h, w = 8, 16, 32
    A = a + 2 * cube.PAD
    sp = cube.spec(kind, "3x2")
    y = L.frames(2, 3, 2 * a, 3 * a, seed=51).to(DEV).requires_grad_(True)
    out = cube.to_erp(y, (h, w), sp, ss=ss, grad=True)
    assert out.requires_grad and tuple(out.shape) == (2, 3, h, w)
    assert torch.equal(out.detach(), cube.to_erp(y.detach(), (h, w), sp, ss=ss))
    g = L.gradient(2, 3, h, w, seed=52).to(DEV)
    (got,) = torch.autograd.grad(out, y, g)
    map = cube.to_erp_map(kind, a, h, w, ss, DEV)
    g_stack = PCONV.remap_backward_f32(g, map, viewport.reverse_lists(map, 6 * A, A), 6 * A, A, h, w, ss)
    assert torch.equal(got, cube.pack(cube.pad_backward(g_stack, kind, a, cube.PAD), "3x2"))
    # the CPU twins walk the same lists in the same order
    leaf = y.detach().cpu().requires_grad_(True)
    cpu_map = cube.to_erp_map(kind, a, h, w, ss)
    if torch.equal(cpu_map, map.cpu()):
        (twin,) = torch.autograd.grad(cube.to_erp(leaf, (h, w), sp, ss=ss, grad=True), leaf, g.cpu())
        assert torch.equal(got.cpu(), twin)
    with pytest.raises(PconvError, match="no backward"):
        cube.to_erp(y, (h, w), sp, ss=ss)


# ---- 4. stale memory ----

def test_both_backward_kernels_ignore_what_fresh_memory_held(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import cube
    a, depth = 12, 5
    A = a + 2 * depth
    g = L.gradient(2, 5, 6 * A, A, seed=61).to(DEV)
    x, y, plane, gout, _, _, _ = L.ssim_twins(((1, 3, 75, 150), "zero-block"))
    runs = []
    for regime, enter in SM.regimes(monkeypatch):
        with enter() as made:
            runs.append((cube.pad_backward(g, "eac", a, depth), _ssim_kernel(x, y, plane, gout)))
            assert regime == "plain" or made.count("empty") >= 2          # both results were allocated under the fill
    for pad_grad, ssim_grad in runs[1:]:
        assert SM.same_bits(pad_grad, runs[0][0]) and SM.same_bits(ssim_grad, runs[0][1])
    # the out= form of the binding: gin pre-filled by hand
    from pseudocylindrical_convolution_amd import _metric_ops
    table, lists = cube.pad_table_on("eac", a, DEV, depth), cube.pad_reverse_lists("eac", a, depth, DEV)
    for kind in SM.KINDS:
        out = SM.fill_(torch.empty((2, 5, 6 * a, a), dtype=torch.float32, device=DEV), kind)
        assert _metric_ops.cube_pad_backward(g, table, lists, a, depth, out) is out and SM.same_bits(out, runs[0][0])


# ---- 5. training ----

def test_adam_steps_on_the_cube_ws_terms_lower_the_loss(hip_backend):
    """a free (1, 3, 32, 64) picture under the two terms of train.py --loss cube-ws: every pixel gets a finite gradient
    through from_erp's, the continuation's and the weighted metrics' backward kernels, and five Adam steps lower the loss"""
    from pseudocylindrical_convolution_amd import train
    args = argparse.Namespace(cube_kind="eac", cube_face=None)
    data = L.frames(1, 3, 32, 64, seed=71).to(DEV)
    y = torch.nn.Parameter(L.frames(1, 3, 32, 64, seed=72).to(DEV))
    opt = torch.optim.Adam([y], lr=0.02)
    losses = []
    for it in range(5):
        mse, ssim = (t.mean() for t in train.cube_ws_terms(args, data, y))
        loss = mse + 0.1 * (1 - ssim)
        opt.zero_grad()
        loss.backward()
        if it == 0:
            assert torch.isfinite(y.grad).all() and (y.grad != 0).float().mean().item() > 0.5
        opt.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
