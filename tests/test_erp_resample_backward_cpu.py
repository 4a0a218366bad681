"""The ordered backward of the sphere-aware resize without a GPU (include/pconv_hip.h, pconv_erp_resample_backward_f32):
the host lists against a numpy construction, the torch twin against the definition as a plain float32 loop and against
torch's autograd of resize_torch within a derived bound, the adjoint identity, erp_resample.resize under autograd, the
renderer's opt-in prefilter gradient, and train.py --code-size on the oracle backend."""
import numpy as np
import pytest
import torch

import erp_resample_backward_cases as B
from erp_resample_backward_cases import CASES, case_id

U23 = 2.0 ** -23


def _axes():
    seen = []
    for case in CASES:
        for axis in ((case[2], case[4]), (case[3], case[5])):
            if axis not in seen:
                seen.append(axis)
    return seen


@pytest.mark.parametrize("pole", [0, 1])
@pytest.mark.parametrize("axis", _axes(), ids=lambda a: "%d-to-%d" % a)
def test_host_lists_are_a_stable_sort_of_the_forward_walk(axis, pole):
    from pseudocylindrical_convolution_amd import erp_resample
    n_in, n_out = axis
    T = erp_resample.taps(n_in, n_out)[1].shape[1]
    start, entry, crossed = erp_resample.reverse_taps(n_in, n_out, pole)
    assert start.dtype == torch.int32 and entry.dtype == torch.int32 and crossed.dtype == torch.uint8
    assert start.numel() == n_in + 1 and entry.numel() == n_out * T == crossed.numel()
    want = B.numpy_lists(n_in, n_out, pole)
    for got, w in zip((start, entry, crossed), want):
        assert np.array_equal(got.numpy(), w)
    assert start[0].item() == 0 and start[-1].item() == n_out * T       # the list lengths sum to n_out T
    assert np.array_equal(np.sort(entry.numpy()), np.arange(n_out * T))
    if not pole:
        assert not bool(crossed.any())
    assert erp_resample.reverse_taps(n_in, n_out, pole)[1] is entry     # cached


def test_host_lists_refuse_bad_arguments_before_writing():
    from pseudocylindrical_convolution_amd._native import PconvError, call, hip_lib
    start, entry = np.full(10, -7, dtype=np.int32), np.full(5 * 11, -7, dtype=np.int32)
    crossed = np.full(5 * 11, 9, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data
    assert call("pconv_host_lanczos_reverse_size", 9, 5) == 5 * 11
    assert hip_lib().pconv_host_lanczos_reverse_size(17, 2) < 0
    assert hip_lib().pconv_host_lanczos_reverse_size(1, 5) < 0
    for pole, hole in ((0, 3), (0, 4), (1, 3), (1, 4), (1, 5)):
        args = [9, 5, pole, ptr(start), ptr(entry), ptr(crossed)]
        args[hole] = None
        with pytest.raises(PconvError, match="null pointer"):
            call("pconv_host_lanczos_reverse", *args)
    for n_in, n_out, reason in ((1, 5, "outside 2"), (9, 1, "outside 2"), ((1 << 20) + 1, 1 << 20, "outside 2"),
                                (17, 2, "shrinks by more than 8:1")):
        with pytest.raises(PconvError, match=reason):
            call("pconv_host_lanczos_reverse", n_in, n_out, 1, ptr(start), ptr(entry), ptr(crossed))
    assert (start == -7).all() and (entry == -7).all() and (crossed == 9).all()
    assert call("pconv_host_lanczos_reverse", 9, 5, 0, ptr(start), ptr(entry), None) == 5 * 11     # pole = 0 needs no flags
    assert (crossed == 9).all() and start[0] == 0 and start[9] == 5 * 11


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_twin_is_the_plain_float32_loop_bit_for_bit(case):
    from pseudocylindrical_convolution_amd import erp_resample
    g = B.gradient(case)
    got = erp_resample.resize_backward_torch(g, case[2], case[3])
    assert got.shape == case[:4] and got.dtype == torch.float32
    assert torch.equal(got, B.walk(g, case[2], case[3]))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_twin_is_within_the_chains_bound_of_torchs_autograd(case):
    """Both are float32 evaluations of the same sum of products, in two orders.  A chain of N terms ends within N u
    sum|term| of the exact sum (u = 2^-24, first order), the rounding of gmid included when N counts the terms of both
    passes; two such evaluations differ by at most twice that: N 2^-23 sum|term| per element, with N and sum|term|
    taken over both passes in float64"""
    from pseudocylindrical_convolution_amd import erp_resample
    n, c, h, w, h2, w2 = case
    g = B.gradient(case)
    x = B.frames(case).requires_grad_()
    erp_resample.resize_torch(x, h2, w2).backward(g)
    got = erp_resample.resize_backward_torch(g, h, w)
    bound = B.term_counts(h, w, h2, w2) * U23 * B.walk(g, h, w, np.float64, absolute=True)
    err = (got.double() - x.grad.double()).abs()
    print("%s: max |twin - autograd| = %.3e, the bound there %.3e, max err / bound %.3f"
          % (case_id(case), err.max().item(), bound.flatten()[err.argmax()].item(), (err / bound).max().item()))
    assert bool((bound > 0).all()) and bool((err <= bound).all())
    exact = B.walk(g, h, w, np.float64)
    assert bool(((got.double() - exact).abs() <= bound).all())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_adjoint_identity_in_float64(case):
    """<resize(x), g> = <x, backward(g)>, the inner products taken in float64 of the float32 results.  The forward's
    chains have T_x + T_y terms, the backward's at most max(n_h) + max(n_v): with N the larger of the two, each side is
    within N u <|x|, |A|^T |g|> of the exact bilinear form, the two within N 2^-23 of it of each other"""
    from pseudocylindrical_convolution_amd import erp_resample
    n, c, h, w, h2, w2 = case
    g, x = B.gradient(case), B.frames(case, lo=-0.5, hi=1.5)
    left = (erp_resample.resize_torch(x, h2, w2).double() * g.double()).sum().item()
    right = (x.double() * erp_resample.resize_backward_torch(g, h, w).double()).sum().item()
    taps = erp_resample.taps(w, w2)[1].shape[1] + erp_resample.taps(h, h2)[1].shape[1]
    terms = max(taps, B.term_counts(h, w, h2, w2).max().item())
    bound = terms * U23 * (x.double().abs() * B.walk(g, h, w, np.float64, absolute=True)).sum().item()
    print("%s: <Ax, g> - <x, A^T g> = %.3e, bound %.3e" % (case_id(case), left - right, bound))
    assert abs(left - right) <= bound and abs(left) > 1e2 * bound


def test_identity_returns_the_gradient_bit_for_bit():
    from pseudocylindrical_convolution_amd import erp_resample
    n, c, h, w, h2, w2 = B.IDENTITY
    row = erp_resample.taps(w, w2)[1]
    assert bool((row.sum(1) == 1).all()) and bool(((row == 0) | (row == 1)).all())
    g = B.gradient(B.IDENTITY)
    assert torch.equal(erp_resample.resize_backward_torch(g, h, w).view(torch.int32), g.view(torch.int32))


def _clamp_case():
    n, c, h, w, h2, w2 = B.CLAMPED
    return B.frames(B.CLAMPED, seed=3, lo=-0.5, hi=1.5), B.gradient(B.CLAMPED, seed=3), h, w, h2, w2


def test_clamp_masks_as_torch_clamp_does():
    from pseudocylindrical_convolution_amd import erp_resample
    x, g, h, w, h2, w2 = _clamp_case()
    raw = erp_resample.resize_torch(x, h2, w2)
    inside = (raw >= 0) & (raw <= 1)
    assert bool(inside.any()) and not bool(inside.all())     # some but not all outputs are clamped
    x.requires_grad_()
    out = erp_resample.resize(x, h2, w2, clamp=True)
    assert torch.equal(out.detach(), raw.clamp(0, 1))
    out.backward(g)
    masked = torch.where(inside, g, torch.zeros(()))
    assert bool((masked[~inside] == 0).all()) and torch.equal(masked[inside], g[inside])
    assert torch.equal(x.grad, erp_resample.resize_backward_torch(masked, h, w))
    assert not torch.equal(x.grad, erp_resample.resize_backward_torch(g, h, w))
    y = x.detach().clone().requires_grad_()
    erp_resample.resize_torch(y, h2, w2, clamp=True).backward(g)          # torch.clamp's own gradient
    bound = B.term_counts(h, w, h2, w2) * U23 * B.walk(masked, h, w, np.float64, absolute=True) + 1e-300
    assert bool(((x.grad.double() - y.grad.double()).abs() <= bound).all())


@pytest.mark.parametrize("case", B.SMALL, ids=case_id)
def test_resize_under_autograd_on_cpu_tensors(case):
    from pseudocylindrical_convolution_amd import erp_resample
    from pseudocylindrical_convolution_amd._native import PconvError
    n, c, h, w, h2, w2 = case
    g, x = B.gradient(case), B.frames(case)
    plain = erp_resample.resize(x, h2, w2)
    assert plain.grad_fn is None and torch.equal(plain, erp_resample.resize_torch(x, h2, w2))
    out = torch.empty(n, c, h2, w2)
    assert erp_resample.resize(x, h2, w2, out=out) is out and torch.equal(out, plain)
    x.requires_grad_()
    with torch.no_grad():
        assert erp_resample.resize(x, h2, w2).grad_fn is None
    res = erp_resample.resize(x, h2, w2)
    assert res.grad_fn is not None and torch.equal(res.detach(), plain)
    res.backward(g)
    assert torch.equal(x.grad, erp_resample.resize_backward_torch(g, h, w))
    with pytest.raises(PconvError, match="out= cannot be combined with a gradient"):
        erp_resample.resize(x, h2, w2, out=out)


def _prefiltered():
    from pseudocylindrical_convolution_amd import viewport
    v = viewport.view(0, 0, 0, 120, 90)
    assert viewport.plan(64, 128, v, 4, 6)[:2] != (64, 128)
    return v


def test_renderer_refuses_the_prefilter_gradient_by_default():
    from pseudocylindrical_convolution_amd import viewport
    from pseudocylindrical_convolution_amd._native import PconvError
    with pytest.raises(PconvError, match="carries no gradient"):
        viewport.Renderer(64, 128, [_prefiltered()], (4, 6)).render(torch.rand(1, 1, 64, 128).requires_grad_())


def test_renderer_prefilter_gradient_is_the_chain_rule_by_hand():
    from pseudocylindrical_convolution_amd import erp_resample, viewport
    wide, narrow = _prefiltered(), viewport.view(30, 20, 10, 20, 15)
    r = viewport.Renderer(64, 128, [narrow, wide, narrow], (4, 6), prefilter_grad=True)
    (h2, w2, ss) = r.plans[1]
    assert r.plans[0][:2] == (64, 128) and (h2, w2) != (64, 128) and r.plans[2] == r.plans[0]
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(2, 3, 64, 128, generator=gen).requires_grad_()
    g = torch.randn(2, 3, 3, 4, 6, generator=gen)
    out = r.render(x)
    assert out.grad_fn is not None and torch.equal(out.detach(), r.render(x.detach()))     # the views in their order
    out.backward(g)
    assert bool(torch.isfinite(x.grad).all()) and bool((x.grad != 0).any())
    full = None
    for k in (0, 2):
        full = viewport.render_backward_torch(g[:, k].contiguous(), r.maps[k], r.lists(k), 64, 128, 4, 6, r.plans[k][2],
                                              accumulate_into=full)
    small = viewport.render_backward_torch(g[:, 1].contiguous(), r.maps[1], r.lists(1), h2, w2, 4, 6, ss)
    reduced = erp_resample.resize_backward_torch(small, 64, 128)
    assert bool((reduced != 0).any())
    assert torch.equal(x.grad, full + reduced)             # two terms: the float32 sum is commutative
    # one prefiltered view alone, clamped: loss_terms works for any plan
    alone = viewport.Renderer(64, 128, [wide], (4, 6), prefilter_grad=True)
    y = torch.rand(1, 3, 64, 128, generator=gen).requires_grad_()
    terms = viewport.loss_terms(alone, x.detach()[:1], y)
    assert torch.equal(terms.detach(), viewport.metrics(alone, x.detach()[:1], y.detach()))
    terms.sum().backward()
    assert bool(torch.isfinite(y.grad).all()) and bool((y.grad != 0).any())


def test_code_size_parses_and_refuses():
    from pseudocylindrical_convolution_amd import train
    from pseudocylindrical_convolution_amd.optim import TrainState
    parse = train.build_parser().parse_args
    args = parse(["--height", "512", "--width", "1024", "--code-size", "512x256"])
    assert args.code_size == (256, 512)
    assert parse([]).code_size is None
    for bad in (["--code-size", "512"], ["--code-size", "500x256"], ["--code-size", "512x250"],
                ["--height", "4096", "--width", "8192", "--code-size", "512x512"],       # 16:1 in width
                ["--height", "4096", "--width", "2048", "--code-size", "512x256"]):      # 16:1 in height
        with pytest.raises(SystemExit):
            parse(bad)
    # the fingerprint carries the argument only when given: a state file from before it still resumes
    assert "code_size" not in TrainState.fingerprint(parse([]), 1)
    assert TrainState.fingerprint(parse(["--code-size", "512x256"]), 1)["code_size"] == (256, 512)
    assert TrainState.fingerprint(parse(["--code-size", "512x256"]), 1) != TrainState.fingerprint(parse(["--code-size", "1024x256"]), 1)


def test_a_step_with_code_size_on_the_cpu(oracle_backend):
    """one forward_losses step of the base model: the model sees 256 x 512, the losses the 320 x 768 frames"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, train
    args = train.build_parser().parse_args(["--device", "cpu", "--loss", "ws", "--base", "--height", "320", "--width", "768",
                                            "--code-size", "512x256"])
    torch.manual_seed(0)
    net = Z.CMPNetV2M(8, 16, 16, 16, opt=False, init=False, device_id=0)
    net.train()
    seen = []
    hook = net.register_forward_pre_hook(lambda m, inp: seen.append(tuple(inp[0].shape)))
    x = torch.rand(1, 3, 320, 768, generator=torch.Generator().manual_seed(3))
    mse, ssim, rate = train.forward_losses(args, net, x, None, None, None)
    hook.remove()
    assert seen == [(1, 3, 256, 512)] and rate is None
    assert bool(torch.isfinite(mse)) and bool(torch.isfinite(ssim)) and mse.item() > 0
    (mse + 0.1 * (1 - ssim)).backward()
    transforms = [(name, p) for name, p in net.named_parameters() if name.startswith(("encoder", "decoder"))]
    assert len(transforms) > 10
    for name, p in transforms:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(bool((p.grad != 0).any()) for _, p in transforms)
