"""GPU: the native convolution backward (csrc/conv_backward.hip, PCONV.tile_conv2d_backward, PCONV.native_conv_grad)
held BIT FOR BIT -- the sign of zero included -- to its CPU twin (tests/conv_backward_cases.py), then its Python
surface (need flags, the transposed pack's cache, the autograd bridge of TileConv2d) and whole training steps that
never reach the vendor library's convolution."""
import pytest
import torch

import conv_backward_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c.name for c in C.CASES]


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


def same_bits(got, ref, what):
    got, ref = C.bits(got), C.bits(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got != ref
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d entries differ, first at %s: got 0x%08x, expected 0x%08x"
                             % (what, int(bad.sum()), bad.numel(), first, got[first].item() & 0xffffffff,
                                ref[first].item() & 0xffffffff))


def run(case, need=None, **kw):
    x, weight, gout = (t.to(DEV) for t in C.inputs(case))
    need = (case.need_x, True, True) if need is None else need
    return P().tile_conv2d_backward(x, weight, gout, case.s, need, **kw)


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_gradients_are_the_twin_bit_for_bit_twice(hip_backend, case):
    tin, tw, tb = C.twin(case)
    for call in range(2):   # the same bits on a second call
        gin, gw, gb = run(case)
        assert (gin is None) == (not case.need_x)
        if case.need_x:
            same_bits(gin, tin, "case %s gin, call %d" % (case.name, call))
        same_bits(gw, tw, "case %s gw, call %d" % (case.name, call))
        same_bits(gb, tb, "case %s gb, call %d" % (case.name, call))
    if case.name == "b":
        assert int((C.bits(gin[:, :, 9]) != 0).sum()) == 0   # the untouched bottom row: +0, not merely zero


def test_data_gradient_of_one_tile_alone_is_its_slice_of_the_batchs(hip_backend):
    case = C.BY_NAME["a"]
    x, weight, gout = (t.to(DEV) for t in C.inputs(case))
    both = P().tile_conv2d_backward(x, weight, gout, case.s, (True, False, False))[0]
    alone = P().tile_conv2d_backward(x[1:2].contiguous(), weight, gout[1:2].contiguous(), case.s, (True, False, False))[0]
    same_bits(alone, both[1:2], "tile 1 alone")


def test_a_gradient_that_is_not_asked_for_is_neither_computed_nor_returned(hip_backend, monkeypatch):
    PC = P()
    case = C.BY_NAME["b"]
    tin, tw, tb = C.twin(case)
    launched = []
    real = PC.call
    monkeypatch.setattr(PC, "call", lambda fn, *a: (launched.append(fn), real(fn, *a))[1])
    expect = {
        (True, False, False): {"pconv_conv_pack_weight_transposed", "pconv_conv2d_dgrad"},
        (False, True, False): {"pconv_conv2d_wgrad"},
        (False, False, True): {"pconv_conv2d_wgrad"},
        (False, True, True): {"pconv_conv2d_wgrad"},
    }
    for need, entries in expect.items():
        del launched[:]
        out = run(case, need)
        assert set(launched) == entries, (need, launched)
        for got, ref, asked, name in zip(out, (tin, tw, tb), need, ("gin", "gw", "gb")):
            assert (got is not None) == asked, (need, name)
            if asked:
                same_bits(got, ref, "%s with need %s" % (name, need))
    # a bias-only call brings the fp64 planes alone, not the partials' workspace
    made = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (made.append((a, k)), real_empty(*a, **k))[1])
    run(case, (False, False, True))
    monkeypatch.setattr(torch, "empty", real_empty)
    sizes = [a[0] for a, k in made if k.get("dtype") == torch.uint8]
    assert sizes == [case.tn * case.cout * 8], sizes
    assert run(case, (False, False, False)) == (None, None, None)


def test_tensors_that_are_not_dense_float32_on_the_gpu_are_refused(hip_backend):
    from pseudocylindrical_convolution_amd._native import PconvError
    case = C.BY_NAME["c"]
    x, weight, gout = (t.to(DEV) for t in C.inputs(case))
    bad = [(x.cpu(), weight, gout), (x, weight.cpu(), gout), (x, weight.double(), gout), (x.double(), weight, gout),
           (x, weight, gout.transpose(2, 3).contiguous().transpose(2, 3)), (x, weight[:, :, 0, 0], gout),
           # a 5x5 layer whose shapes fit: conv5x5_backward's, not this entry's
           (x.new_zeros(2, 5, 8, 12), x.new_zeros(3, 5, 5, 5), x.new_zeros(2, 3, 4, 8))]
    for need in ((True, False, False), (False, True, True)):
        for xs, ws, gs in bad:
            with pytest.raises(PconvError):
                P().tile_conv2d_backward(xs, ws, gs, case.s, need)


def test_data_gradient_follows_an_in_place_change_of_the_weights(hip_backend):
    case = C.BY_NAME["a"]
    x, weight, gout = (t.to(DEV) for t in C.inputs(case))

    class Owner(object):
        pass

    owner = Owner()
    first = P().tile_conv2d_backward(x, weight, gout, case.s, (True, False, False), owner=owner)[0]
    key, packed = owner._pconv_packed_t
    again = P().tile_conv2d_backward(x, weight, gout, case.s, (True, False, False), owner=owner)[0]
    assert owner._pconv_packed_t[1] is packed            # cached while the weights stand
    same_bits(again, first, "second call on the cached pack")
    weight.mul_(2.0)                                     # what an optimiser step does: in place
    second = P().tile_conv2d_backward(x, weight, gout, case.s, (True, False, False), owner=owner)[0]
    assert owner._pconv_packed_t[0] != key
    same_bits(second, first * 2.0, "data gradient after weight *= 2")   # (scaling by two is exact)
    same_bits(first, C.twin(case)[0], "data gradient before")


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_autograd_through_tileconv2d_is_the_native_backward_and_close_to_the_vendors(hip_backend, name):
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z
    case = C.BY_NAME[name]
    x, weight, gout = (t.to(DEV) for t in C.inputs(case))
    conv = Z.TileConv2d(case.cin, case.cout, case.k, case.s).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(weight)
    xr = x.clone().requires_grad_(True)
    with P().native_conv_grad(True):
        y = conv(xr)
        assert type(y.grad_fn).__name__ == "TileConvCallBackward"
        native = torch.autograd.grad(y, (xr, conv.weight, conv.bias), gout)
    direct = P().tile_conv2d_backward(x, conv.weight.detach(), gout, case.s)
    y = conv(xr)
    assert "Convolution" in type(y.grad_fn).__name__      # the switch is off again: the library's
    vendor = torch.autograd.grad(y, (xr, conv.weight, conv.bias), gout)
    bx, bw, _ = C.bounds(case, *C.inputs(case))
    # (the library sums the bias gradient in float32: a chain of tn*ho*wo adds in some order)
    bb = gout.shape[0] * gout.shape[2] * gout.shape[3] * C.U * gout.abs().double().sum((0, 2, 3)).cpu()
    for what, n, d, v, bound in zip(("gin", "gw", "gb"), native, direct, vendor, (bx, bw, bb)):
        same_bits(n, d, "%s through autograd" % what)
        err = (n.double() - v.double()).abs().cpu()
        print("case %s %s: max |native - vendor| %.3e, largest share of the bound %.3g"
              % (name, what, err.max().item(), (err / bound.clamp_min(1e-300)).max().item()))
        assert bool((err <= bound).all()), what


def test_the_first_layer_asks_for_no_data_gradient(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z
    PC = P()
    case = C.BY_NAME["e"]
    x, weight, gout = (t.to(DEV) for t in C.inputs(case))
    conv = Z.TileConv2d(case.cin, case.cout, case.k, case.s).to(DEV)
    asked = []
    real = PC.tile_conv2d_backward
    monkeypatch.setattr(PC, "tile_conv2d_backward", lambda x, w, g, s, need=(True, True, True), owner=None:
                        (asked.append(tuple(bool(n) for n in need)), real(x, w, g, s, need, owner=owner))[1])
    with PC.native_conv_grad(True):
        (conv(x) * gout).sum().backward()                 # x is an image: it needs no gradient
    assert asked == [(False, True, True)]
    direct = real(x, conv.weight.detach(), gout, case.s, (False, True, True))
    same_bits(conv.weight.grad, direct[1], "gw")
    same_bits(conv.bias.grad, direct[2], "gb")


# ---- whole training steps ------------------------------------------------------------------------------------------

def _steps(net_class, frames, native, guard, monkeypatch):
    """two Adam steps of a small model from the seed under train.deterministic_mode(), on the loss of
    `train.py --loss ws` as train.forward_losses computes it (the loss the no-library-convolution claim is made for:
    the default --loss viewport has the library's 11 x 11 blur in its SSIM term): (loss of the first step, the
    parameters after the second, the model)"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, train
    import contextlib
    args = train.build_parser().parse_args(["--loss", "ws"])
    torch.manual_seed(0)
    net = getattr(Z, net_class)(56, 192, 192, 16, 8, True, False, 0).to(DEV)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    x = torch.rand(frames, 3, 256, 512, generator=torch.Generator().manual_seed(3)).to(DEV)
    losses = []
    with contextlib.ExitStack() as stack:
        stack.enter_context(train.deterministic_mode())
        stack.enter_context(P().native_conv_grad(native))
        if guard is not None:
            stack.enter_context(monkeypatch.context()).setattr(torch.nn.functional, "conv2d", guard)
        for it in range(2 if native else 1):
            mse, ssim, rate = train.forward_losses(args, net, x, None, None, None)
            loss = mse + 0.1 * (1 - ssim) + (0.0 if rate is None else 0.05 * rate)
            opt.zero_grad()
            loss.backward()
            if it == 0 and native:
                assert all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in net.parameters())
            opt.step()
            losses.append(loss.item())
    return losses[0], [p.detach().clone() for p in net.parameters()], net


def test_base_stage_model_trains_without_the_library_convolution_to_the_same_bits_twice(hip_backend, monkeypatch):
    """CMPNetV2M (the --base stage: transforms and quantiser) on the loss of --loss ws: with the switch on NO
    convolution reaches torch.nn.functional.conv2d -- every TileConv2d and the GDN's contraction run on this project's
    kernels, and the sphere-weighted loss has no convolution of torch's.  (Under the default --loss viewport the SSIM
    term's blur is a library convolution: tests/test_conv_backward_cpu.py pins that, and the claim is not made there.)"""
    def guard(*args, **kwargs):
        raise AssertionError("torch.nn.functional.conv2d was called under native_conv_grad")

    la, pa, _ = _steps("CMPNetV2M", 1, True, guard, monkeypatch)
    lb, pb, _ = _steps("CMPNetV2M", 1, True, guard, monkeypatch)
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(C.bits(a), C.bits(b))
    lv = _steps("CMPNetV2M", 1, False, None, monkeypatch)[0]
    print("first step's loss: native %.9g, vendor %.9g, relative difference %.3g" % (la, lv, abs(la - lv) / abs(lv)))
    assert abs(la - lv) <= 1e-4 * abs(lv)


def test_whole_model_trains_on_the_native_convolutions_to_the_same_bits_twice(hip_backend, monkeypatch):
    """CMPNetV2MF at the size tests/test_gpu_sphere_loss.py uses, two Adam steps under train.deterministic_mode()
    with native_conv_grad(True): repeated from the seed every parameter ends bit-identical, and the first step's
    loss is within 1e-4 relative of the vendor path's (the forward's tolerance against the library).
    torch.nn.functional.conv2d is patched to raise for every convolution the native kernels take (k in {1, 3}: all
    TileConv2d layers and the GDN); the entropy model's masked 5 x 5 convolutions are outside that scope and are the
    only calls let through -- counted, so that nothing else hides behind them."""
    real = torch.nn.functional.conv2d
    passed = []

    def guard(x, weight, *args, **kwargs):
        if weight.shape[2] != 5:
            raise AssertionError("torch.nn.functional.conv2d was called for a %s kernel under native_conv_grad"
                                 % (tuple(weight.shape),))
        passed.append(tuple(weight.shape))
        return real(x, weight, *args, **kwargs)

    from pseudocylindrical_convolution_amd.PCONV_operator import MaskConv2
    la, pa, net = _steps("CMPNetV2MF", 2, True, guard, monkeypatch)
    n_masked = len(passed)
    masked_layers = sum(isinstance(m, MaskConv2) for m in net.modules())
    del net
    lb, pb, _ = _steps("CMPNetV2MF", 2, True, guard, monkeypatch)
    assert n_masked == 2 * masked_layers and len(passed) == 2 * n_masked, (n_masked, masked_layers, len(passed))
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(C.bits(a), C.bits(b))
    lv = _steps("CMPNetV2MF", 2, False, None, monkeypatch)[0]
    print("first step's loss: native %.9g, vendor %.9g, relative difference %.3g" % (la, lv, abs(la - lv) / abs(lv)))
    assert abs(la - lv) <= 1e-4 * abs(lv)
