"""GPU: the native masked 5x5 convolution (pconv_conv5*, PCONV.conv5x5 / conv5x5_backward, PCONV.native_masked_conv)
held BIT FOR BIT -- the sign of zero included -- to its CPU twins (tests/masked_conv_cases.py), then its Python surface
(need flags, the autograd bridge of MaskConv2, packs that follow an optimiser step), the viewport SSIM term of
`train.py --conv native-all` against pytorch_ssim, and whole training steps of the full model that never reach
torch.nn.functional.conv2d."""
import contextlib

import pytest
import torch

import masked_conv_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Owner(object):
    pass


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


def on_gpu(case):
    return tuple(t.to(DEV) for t in M.inputs(case))


@pytest.mark.parametrize("case", M.CASES, ids=M.IDS)
def test_forward_and_gradients_are_the_twin_bit_for_bit_twice(hip_backend, case):
    ty, tin, tw, tb = M.twin(case)
    x, weight, bias, gout = on_gpu(case)
    owner = Owner()
    for call in range(2):   # the same bits on a second call (the second on the cached packs)
        y = P().conv5x5(owner, x, weight, bias)
        gin, gw, gb = P().conv5x5_backward(x, weight, gout, (case.need_x, True, True), owner=owner)
        M.same_bits(y, ty, "case %s y, call %d" % (case.name, call))
        assert (gin is None) == (not case.need_x)
        if case.need_x:
            M.same_bits(gin, tin, "case %s gin, call %d" % (case.name, call))
        M.same_bits(gw, tw, "case %s gw, call %d" % (case.name, call))
        M.same_bits(gb, tb, "case %s gb, call %d" % (case.name, call))
    M.same_bits(P().conv5x5(Owner(), x, weight, None), pconv_chain(x, weight, None), "case %s y without a bias" % case.name)


def pconv_chain(x, weight, bias):
    from oracle import pconv_cpu
    return pconv_cpu.conv2d_chain(x.detach().cpu(), weight.detach().cpu(), None if bias is None else bias.detach().cpu(), 1)


def test_one_tile_alone_is_its_slice_of_the_batchs(hip_backend):
    case = M.BY_NAME["a"]
    x, weight, bias, gout = on_gpu(case)
    both_y = P().conv5x5(Owner(), x, weight, bias)
    both_gin = P().conv5x5_backward(x, weight, gout, (True, False, False))[0]
    alone_y = P().conv5x5(Owner(), x[1:2].contiguous(), weight, bias)
    alone_gin = P().conv5x5_backward(x[1:2].contiguous(), weight, gout[1:2].contiguous(), (True, False, False))[0]
    M.same_bits(alone_y, both_y[1:2], "forward of tile 1 alone")
    M.same_bits(alone_gin, both_gin[1:2], "data gradient of tile 1 alone")


def test_a_gradient_that_is_not_asked_for_is_neither_computed_nor_returned(hip_backend, monkeypatch):
    PC = P()
    case = M.BY_NAME["b"]
    _, tin, tw, tb = M.twin(case)
    x, weight, bias, gout = on_gpu(case)
    launched = []
    real = PC.call
    monkeypatch.setattr(PC, "call", lambda fn, *a: (launched.append(fn), real(fn, *a))[1])
    expect = {
        (True, False, False): {"pconv_conv5_pack_weight_transposed", "pconv_conv5_dgrad"},
        (False, True, False): {"pconv_conv5_wgrad"},
        (False, False, True): {"pconv_conv5_wgrad"},
        (False, True, True): {"pconv_conv5_wgrad"},
    }
    for need, entries in expect.items():
        del launched[:]
        out = PC.conv5x5_backward(x, weight.clone(), gout, need)   # (a fresh weight: no cached pack)
        assert set(launched) == entries, (need, launched)
        for got, ref, asked, name in zip(out, (tin, tw, tb), need, ("gin", "gw", "gb")):
            assert (got is not None) == asked, (need, name)
            if asked:
                M.same_bits(got, ref, "%s with need %s" % (name, need))
    # a bias-only call brings the fp64 planes alone, not the partials' workspace
    made = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (made.append((a, k)), real_empty(*a, **k))[1])
    PC.conv5x5_backward(x, weight, gout, (False, False, True))
    monkeypatch.setattr(torch, "empty", real_empty)
    sizes = [a[0] for a, k in made if k.get("dtype") == torch.uint8]
    assert sizes == [case.tn * case.cout * 8], sizes
    del launched[:]
    assert PC.conv5x5_backward(x, weight, gout, (False, False, False)) == (None, None, None)
    assert launched == []


def test_tensors_that_are_not_dense_float32_on_the_gpu_or_not_5x5_are_refused(hip_backend):
    from pseudocylindrical_convolution_amd._native import PconvError
    case = M.BY_NAME["b"]
    x, weight, bias, gout = on_gpu(case)
    bad = [(x.cpu(), weight, gout), (x, weight.cpu(), gout), (x, weight.double(), gout), (x.double(), weight, gout),
           (x, weight, gout.transpose(2, 3).contiguous().transpose(2, 3)), (x, weight[:, :, 1:4, 1:4].contiguous(), gout),
           (x, weight, gout[:, :, :, 1:].contiguous()), (x[:, 1:].contiguous(), weight, gout)]
    for need in ((True, False, False), (False, True, True)):
        for xs, ws, gs in bad:
            with pytest.raises(PconvError):
                P().conv5x5_backward(xs, ws, gs, need)
    for xs, ws, bs in ((x.cpu(), weight, bias), (x, weight[:, :, 1:4, 1:4].contiguous(), bias), (x, weight, bias[1:]),
                       (x[:, :, :4].contiguous(), weight, bias), (x.transpose(2, 3).contiguous().transpose(2, 3), weight, bias)):
        with pytest.raises(PconvError):
            P().conv5x5(Owner(), xs, ws, bs)


def _mask_conv(seed=0):
    from pseudocylindrical_convolution_amd.PCONV_operator import MaskConv2
    torch.manual_seed(seed)
    conv = MaskConv2(14, 3, 3, 5, hidden=True).to(DEV)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(42, generator=torch.Generator().manual_seed(seed + 1)))
    return conv


def test_autograd_through_maskconv2_is_the_native_backward_and_close_to_float64(hip_backend):
    case = M.BY_NAME["a"]
    x, _, _, gout = on_gpu(case)
    conv = _mask_conv()
    xr = x.clone().requires_grad_(True)
    with P().native_masked_conv(True):
        y = conv(xr)
        assert type(y.grad_fn).__name__ == "MaskConvCallBackward"
        native = torch.autograd.grad(y, (xr, conv.weight, conv.bias), gout)
    wm = conv.weight.detach().clone()            # masked by the forward
    M.same_bits(wm, M.masked(wm.cpu(), case), "the weight after a forward is the masked weight")
    M.same_bits(y, pconv_chain(x, wm, conv.bias), "y through the module")
    direct = P().conv5x5_backward(x, wm, gout)
    y = conv(xr)
    assert "Convolution" in type(y.grad_fn).__name__      # the switch is off again: the library's
    ref = M.f64_grads(x.cpu(), wm.cpu(), gout.cpu(), 1)
    for what, n, d, r, bound in zip(("gin", "gw", "gb"), native, direct, ref, M.bounds(case, x.cpu(), wm.cpu(), gout.cpu())):
        M.same_bits(n, d, "%s through autograd" % what)
        err = (n.double().cpu() - r).abs()
        print("%s: max |native - f64| %.3e, largest share of the bound %.3g"
              % (what, err.max().item(), (err / bound.clamp_min(1e-300)).max().item()))
        assert bool((err <= bound).all()), what
    gone = M.masked(torch.ones_like(wm.cpu()), case) == 0
    assert bool((native[1].cpu()[gone] != 0).any())       # the dense weight gradient, masked taps included


def test_the_first_layers_input_asks_for_no_data_gradient(hip_backend, monkeypatch):
    PC = P()
    case = M.BY_NAME["g"]
    x, _, _, gout = on_gpu(case)
    conv = _mask_conv()
    asked = []
    real = PC.conv5x5_backward
    monkeypatch.setattr(PC, "conv5x5_backward", lambda x, w, g, need=(True, True, True), owner=None:
                        (asked.append(tuple(bool(n) for n in need)), real(x, w, g, need, owner=owner))[1])
    with PC.native_masked_conv(True):
        (conv(x) * gout).sum().backward()                 # x are the symbols: no gradient
    assert asked == [(False, True, True)]
    direct = real(x, conv.weight.detach(), gout, (False, True, True))
    M.same_bits(conv.weight.grad, direct[1], "gw")
    M.same_bits(conv.bias.grad, direct[2], "gb")


def test_packs_follow_an_optimiser_step_and_are_made_after_the_mask(hip_backend, monkeypatch):
    """the mask goes through weight.data and leaves weight._version alone; an Adam step moves the masked taps away
    from zero (the weight gradient is dense) and bumps the version: the second forward masks first, packs then"""
    PC = P()
    case = M.BY_NAME["a"]
    x, _, _, gout = on_gpu(case)
    conv = _mask_conv()
    gone = (M.masked(torch.ones(case.cout, case.cin, 5, 5), case) == 0).to(DEV)
    opt = torch.optim.Adam(conv.parameters(), lr=1e-2)
    seen = []
    real = PC.call

    def spy(fn, *a):
        if fn.startswith("pconv_conv5_pack_weight"):
            seen.append((fn, int((conv.weight.detach()[gone] != 0).sum())))
        return real(fn, *a)

    monkeypatch.setattr(PC, "call", spy)
    with PC.native_masked_conv(True):
        xr = x.clone().requires_grad_(True)
        y1 = conv(xr)
        M.same_bits(y1, pconv_chain(x, conv.weight, conv.bias), "first forward")
        (y1 * gout).sum().backward()
        conv(xr)                                           # the weights stand: both packs are cached
        assert [fn for fn, _ in seen] == ["pconv_conv5_pack_weight", "pconv_conv5_pack_weight_transposed"]
        opt.step()
        assert int((conv.weight.detach()[gone] != 0).sum()) > 0      # the step has left the mask
        y2 = conv(xr)
        gin2 = torch.autograd.grad(y2, xr, gout)[0]
    assert [fn for fn, _ in seen] == ["pconv_conv5_pack_weight", "pconv_conv5_pack_weight_transposed"] * 2
    assert all(nonzero == 0 for _, nonzero in seen), seen             # masked before every pack
    wm = M.masked(conv.weight.detach().cpu(), case)
    M.same_bits(conv.weight.detach(), wm, "the weight after the second forward")
    M.same_bits(y2, pconv_chain(x, wm, conv.bias), "second forward: the chain on the newly masked weight")
    import conv_backward_cases as B
    M.same_bits(gin2, B.twin_dgrad(wm, gout.cpu(), case.h, case.w, 1), "data gradient after the step")
    assert not bool((M.bits(y2) == M.bits(y1)).all())


def test_viewport_ssim_term_is_pytorch_ssims_within_the_vendor_paths_own_error(hip_backend):
    """`--conv native-all` computes the SSIM term of the viewport loss as loss_terms(px, py, "uniform")[:, 1].mean()
    in the place of SSIM(11, 3)(px, py).  Yardstick: SSIM(11, 3) in float64 on the CPU; the error may be at most
    8 * e32 + 1e-6, e32 the error of the float32 SSIM(11, 3) on the GPU against the same value (the margin pattern of
    tests/test_gpu_sphere_loss.py); the same for the gradient with respect to py."""
    from pseudocylindrical_convolution_amd import sphere_metrics
    from pseudocylindrical_convolution_amd.PCONV_operator import SSIM
    g = torch.Generator().manual_seed(11)
    px, py = torch.rand(2, 3, 171, 256, generator=g), torch.rand(2, 3, 171, 256, generator=g)

    def value_and_grad(fn, a, b):
        b = b.clone().requires_grad_(True)
        v = fn(a, b)
        return v.detach().double().cpu(), torch.autograd.grad(v, b)[0].detach().double().cpu()

    ref, gref = value_and_grad(SSIM(11, 3), px.double(), py.double())
    ven, gven = value_and_grad(SSIM(11, 3).to(DEV), px.to(DEV), py.to(DEV))
    own, gown = value_and_grad(lambda a, b: sphere_metrics.loss_terms(a, b, weighting="uniform")[:, 1].mean(), px.to(DEV), py.to(DEV))
    e32, err = (ven - ref).abs().item(), (own - ref).abs().item()
    print("SSIM term: float64 %.12f, vendor float32 error %.3e, loss_terms(uniform) error %.3e" % (ref.item(), e32, err))
    assert err <= 8 * e32 + 1e-6
    ge32, gerr, scale = (gven - gref).abs().max().item(), (gown - gref).abs().max().item(), gref.abs().max().item()
    print("its gradient: max |float64| %.3e, vendor float32 max error %.3e, loss_terms(uniform) max error %.3e" % (scale, ge32, gerr))
    assert gerr <= 8 * ge32 + 1e-6
    # the absolute 1e-6 is written for a value of order 1; the gradient of a mean over 393 216 elements is far below
    # it, so the same allowance is also applied relative to the gradient's own size
    assert gerr <= 8 * ge32 + 1e-6 * scale


# ---- whole training steps ------------------------------------------------------------------------------------------

def _steps(native_all, guard, monkeypatch):
    """two Adam steps (one on the vendor path) of CMPNetV2MF from the seed under train.deterministic_mode() on the
    DEFAULT loss, --loss viewport, as train.forward_losses computes it: (loss of the first step, the parameters after
    the last)"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, train
    from pseudocylindrical_convolution_amd.PCONV_operator import MultiProject, SSIM
    args = train.build_parser().parse_args(["--conv", "native-all"] if native_all else [])
    torch.manual_seed(0)
    net = Z.CMPNetV2MF(56, 192, 192, 16, 8, True, False, 0).to(DEV)
    net.train()
    pr1, pr2 = MultiProject(64, 96, 0.5, False, 0).to(DEV), MultiProject(64, 96, 0.5, False, 0).to(DEV)
    sim_func = train.make_sim_func(args, DEV)
    assert (sim_func is None) == native_all
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    x = torch.rand(2, 3, 256, 512, generator=torch.Generator().manual_seed(3)).to(DEV)
    losses = []
    with contextlib.ExitStack() as stack:
        stack.enter_context(train.deterministic_mode())
        stack.enter_context(P().native_conv_grad(native_all))
        stack.enter_context(P().native_masked_conv(native_all))
        if native_all:
            assert P().backward_is_ordered() and P().conv_grad_is_native() and P().masked_conv_is_native()
        if guard is not None:
            stack.enter_context(monkeypatch.context()).setattr(torch.nn.functional, "conv2d", guard)
        for it in range(2 if native_all else 1):
            mse, ssim, rate = train.forward_losses(args, net, x, pr1, pr2, sim_func)
            loss = mse + 0.1 * (1 - ssim) + 0.05 * rate
            opt.zero_grad()
            loss.backward()
            if it == 0 and native_all:
                assert all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in net.parameters())
            opt.step()
            losses.append(loss.item())
    return losses[0], [p.detach().clone() for p in net.parameters()]


def test_whole_model_trains_on_the_default_loss_without_any_library_convolution_to_the_same_bits_twice(hip_backend, monkeypatch):
    """CMPNetV2MF, 2 frames of 256 x 512, the viewport loss: with all three switches on and the SSIM term of
    `--conv native-all`, torch.nn.functional.conv2d -- patched to raise UNCONDITIONALLY -- is never reached; repeated
    from the seed the loss and every parameter are bit-identical; the first step's loss is within 1e-4 relative of the
    vendor path's (switches off, SSIM(11, 3)): the forward's tolerance against the library, DESIGN 2."""
    def guard(*args, **kwargs):
        raise AssertionError("torch.nn.functional.conv2d was called under --conv native-all")

    la, pa = _steps(True, guard, monkeypatch)
    lb, pb = _steps(True, guard, monkeypatch)
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(M.bits(a), M.bits(b))
    assert not (P().masked_conv_is_native() or P().conv_grad_is_native() or P().backward_is_ordered())
    lv = _steps(False, None, monkeypatch)[0]
    print("first step's loss: native-all %.9g, vendor %.9g, relative difference %.3g" % (la, lv, abs(la - lv) / abs(lv)))
    assert abs(la - lv) <= 1e-4 * abs(lv)
