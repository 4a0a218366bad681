"""GPU: the ordered backward of the viewport renderer and of the sphere rotation (csrc/remap_backward.hip,
pconv_remap_backward_f32) bit for bit against its torch twin run on the CPU on the same map and lists (itself held to a
sequential float32 loop in tests/test_viewport_backward_cpu.py), the strided gradient, Renderer.render, erp_rotate.rotate
and viewport.loss_terms under autograd, and two reproducible optimiser steps of --loss vp.

Which edge of the kernel as built each case reaches.  A workgroup takes 256 consecutive source pixels, a lane one pixel
and up to four planes of one frame per walk of its list (grid.y = n * ceil(C / 4)); a workgroup without a list leaves
before it stages the phase table.
  4x4 -> 3x5 ss2          one workgroup, 16 live lanes, every tap column coinciding with another
  2x64 -> 4x6 ss1         the pole rule and the clamp in every footprint
  32x64 -> 9x15 ss1       8 workgroups, some with no list at all
  50x99 -> 37x70 ss2      4950 pixels: a ragged last workgroup; lists of a few thousand entries at the pole
  6x2100 -> 5x300 ss1     long rows
  32x64 -> 37x70 ss3      float32(1 / 9)
  50x99 -> 9x15 ss4       sixteen records per pixel
  50x99 -> 5x300 ss2
Batches (2, 3), (1, 1), (3, 2): a ragged plane group, one plane, two frames' worth of groups."""
import pytest
import torch

import viewport_backward_cases as B
from viewport_backward_cases import CASES, case_id

pytestmark = pytest.mark.gpu

_cache = {}


def _lists(case):
    from pseudocylindrical_convolution_amd import viewport
    if ("lists", case) not in _cache:
        _cache[("lists", case)] = viewport.reverse_lists(B.source_map(case), case[0], case[1])
    return _cache[("lists", case)]


def _first(n, c, h, w):
    return torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(5 + h + w))


def _twin(case, n, c, accumulate):
    """the CPU twin's result on the numpy map, computed once per (case, n, c, accumulate)"""
    from pseudocylindrical_convolution_amd import viewport
    key = (case, n, c, accumulate)
    if key not in _cache:
        h, w, vh, vw, ss, _ = case
        _cache[key] = viewport.render_backward_torch(B.gradient(n, c, vh, vw), B.source_map(case), _lists(case), h, w, vh, vw,
                                                     ss, accumulate_into=_first(n, c, h, w) if accumulate else None)
    return _cache[key]


@pytest.mark.parametrize("n,c", B.BATCHES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_is_the_twin(hip_backend, case, n, c):
    from pseudocylindrical_convolution_amd import PCONV
    h, w, vh, vw, ss, _ = case
    g, q = B.gradient(n, c, vh, vw).cuda(), B.source_map(case).cuda()
    lists = tuple(t.cuda() for t in _lists(case))
    got = PCONV.remap_backward_f32(g, q, lists, h, w, vh, vw, ss)
    assert got.shape == (n, c, h, w) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), _twin(case, n, c, False))
    first = _first(n, c, h, w)
    assert bool((first != 0).all())
    gin = first.cuda()
    assert PCONV.remap_backward_f32(g, q, lists, h, w, vh, vw, ss, gin, accumulate=True).data_ptr() == gin.data_ptr()
    assert torch.equal(gin.cpu(), _twin(case, n, c, True))
    untouched = (lists[0][1:] == lists[0][:-1]).view(h, w).cpu()
    assert torch.equal(gin.cpu()[:, :, untouched], first[:, :, untouched])
    # a gin that held something else is overwritten in full without accumulate: +0 where no sample reads
    gin.fill_(float("nan"))
    PCONV.remap_backward_f32(g, q, lists, h, w, vh, vw, ss, gin)
    assert torch.equal(gin.cpu(), _twin(case, n, c, False))


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[6]], ids=case_id)
def test_a_gradient_is_read_in_place_from_its_slot(hip_backend, case):
    from pseudocylindrical_convolution_amd import PCONV
    h, w, vh, vw, ss, _ = case
    n, c, views = 2, 3, 3
    q, lists = B.source_map(case).cuda(), tuple(t.cuda() for t in _lists(case))
    stack = torch.randn(n, views, c, vh, vw, generator=torch.Generator().manual_seed(11)).cuda()
    for k in range(views):
        want = PCONV.remap_backward_f32(stack[:, k].contiguous(), q, lists, h, w, vh, vw, ss)
        assert torch.equal(PCONV.remap_backward_f32(stack, q, lists, h, w, vh, vw, ss, slot=k), want)
    assert not torch.equal(PCONV.remap_backward_f32(stack, q, lists, h, w, vh, vw, ss, slot=0), want)


def _renderer3():
    from pseudocylindrical_convolution_amd import viewport
    r = viewport.Renderer(32, 64, [viewport.view(*a) for a in B.VIEWS3], (9, 15), device="cuda")
    assert r.ss == (1, 2, 4)
    return r


def _chained_twin(r, g):
    """the twin, view after view, on host copies of the renderer's own maps and lists"""
    from pseudocylindrical_convolution_amd import viewport
    want = None
    for k in range(len(r.views)):
        want = viewport.render_backward_torch(g[:, k].contiguous().cpu(), r.maps[k].cpu(), tuple(t.cpu() for t in r.lists(k)),
                                              r.h, r.w, r.vh, r.vw, r.plans[k][2], accumulate_into=want)
    return want


def test_renderer_under_autograd_is_the_chained_twin_twice(hip_backend):
    r = _renderer3()
    x = torch.rand(2, 3, 32, 64, generator=torch.Generator().manual_seed(3)).cuda().requires_grad_()
    g = torch.randn(2, 3, 3, 9, 15, generator=torch.Generator().manual_seed(4)).cuda()
    grads = []
    for _ in range(2):
        x.grad = None
        out = r.render(x)
        assert out.grad_fn is not None and torch.equal(out.detach(), r.render(x.detach()))
        out.backward(g)
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert torch.equal(grads[0].cpu(), _chained_twin(r, g))


def test_rotate_under_autograd_is_the_twin(hip_backend):
    from pseudocylindrical_convolution_amd import erp_rotate, viewport
    rot = erp_rotate.units(123.25, -33.5, -170)
    x = torch.rand(2, 3, 50, 99, generator=torch.Generator().manual_seed(6)).cuda().requires_grad_()
    out = erp_rotate.rotate(x, rot, clamp=True)
    assert out.grad_fn is not None and torch.equal(out.detach(), erp_rotate.rotate(x.detach(), rot, clamp=True))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).cuda()
    out.backward(g)
    raw = erp_rotate.rotate(x.detach(), rot)
    masked = torch.where((raw >= 0) & (raw <= 1), g, torch.zeros_like(g)).cpu()
    q = erp_rotate.source_map(50, 99, rot, device="cuda").cpu()
    assert torch.equal(x.grad.cpu(), viewport.render_backward_torch(masked, q, viewport.reverse_lists(q, 50, 99), 50, 99, 50, 99, 1))


def test_loss_terms_are_the_metrics_and_compose_with_the_render_backward(hip_backend):
    from pseudocylindrical_convolution_amd import sphere_metrics, viewport
    r = _renderer3()
    gen = torch.Generator().manual_seed(10)
    x = torch.rand(2, 3, 32, 64, generator=gen)
    y = (x + 0.1 * torch.randn(x.shape, generator=gen)).cuda().requires_grad_()
    x = x.cuda()
    terms = viewport.loss_terms(r, x, y)
    assert terms.dtype == torch.float64 and terms.shape == (2, 2) and terms.is_cuda and terms.requires_grad
    assert torch.equal(terms.detach().cpu(), viewport.metrics(r, x, y.detach()))
    gout = torch.tensor([[0.75, -1.5], [1.25, 0.5]], dtype=torch.float64, device="cuda")
    (terms * gout).sum().backward()
    # the same chain by hand: the gradient sphere_metrics.loss_terms gives on the detached views, through the twin
    vx, vy = r.render(x), r.render(y.detach()).requires_grad_()
    total = None
    for k in range(3):
        m = sphere_metrics.loss_terms(vx[:, k].contiguous(), vy[:, k].contiguous(), "uniform")
        total = m if total is None else total + m
    ((total / 3) * gout).sum().backward()
    assert torch.equal(y.grad.cpu(), _chained_twin(r, vy.grad))


def _model_steps(monkeypatch):
    """two Adam steps of CMPNetV2M (16 channels, one frame of 256 x 512) under --deterministic --conv native-all --optim
    native --loss vp, the library's convolution made to raise"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, optim, train

    def refuse(*a, **k):
        raise AssertionError("--conv native-all --loss vp reached torch.nn.functional.conv2d")

    monkeypatch.setattr(torch.nn.functional, "conv2d", refuse)
    args = train.build_parser().parse_args(["--conv", "native-all", "--loss", "vp", "--base", "--optim", "native",
                                            "--deterministic"])
    torch.manual_seed(0)
    net = Z.CMPNetV2M(8, 16, 16, 16, opt=False, init=False, device_id=0).to("cuda:0")
    net.train()
    params = [p for name, p in net.named_parameters() if name != "quant.count"]
    opt = optim.Adam(params, lr=1e-3)
    x = torch.rand(1, 3, 256, 512, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    with train.native_conv_mode("native-all"), train.deterministic_mode():
        for _ in range(2):
            mse, ssim, _ = train.forward_losses(args, net, x, None, None, train.make_sim_func(args, "cuda:0"))
            opt.zero_grad()
            (mse + 0.1 * (1 - ssim)).backward()
            opt.step(clip=0.1)
    assert opt.last_grad_norm.item() > 0
    return [p.detach().clone() for p in params]


def test_two_steps_on_the_vp_loss_give_the_same_bits_twice(hip_backend, monkeypatch):
    a, b = _model_steps(monkeypatch), _model_steps(monkeypatch)
    assert len(a) > 10 and all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    assert all(bool(torch.isfinite(p).all()) for p in a)
