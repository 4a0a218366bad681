"""The native convolution backward without a GPU: its CPU twin (tests/conv_backward_cases.py) against float64 autograd
within the chain's own bound, the PCONV.native_conv_grad switch, `train.py --conv`, and TileConv2d's unchanged vendor
branch while the switch is off."""
import pytest
import torch

import conv_backward_cases as C


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_twin_is_within_the_chains_bound_of_float64_autograd(case):
    x, weight, gout = C.inputs(case)
    gin, gw, gb = C.twin(case)
    rin, rw, rb = C.f64_grads(x, weight, gout, case.s)
    bin_, bw, bb = C.bounds(case, x, weight, gout)
    ho, wo = C.out_size(case)
    assert gw.shape == weight.shape and gb.shape == (case.cout,)
    for name, got, ref, bound in (("gin", gin, rin, bin_), ("gw", gw, rw, bw), ("gb", gb, rb, bb)):
        if got is None:
            continue
        err = (got.double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print("case %s %s: max |twin - f64| %.3e, largest share of the bound %.3g" % (case.name, name, err.max().item(), worst))
        assert bool((err <= bound).all()), "%s of case %s leaves the bound: share %.3g" % (name, case.name, worst)
    if gin is not None and (case.h - case.k) % case.s:
        # rows no output pixel reaches get a chain of zero products from +0
        untouched = C.bits(gin[:, :, case.h - (case.h - case.k) % case.s:])
        assert int((untouched != 0).sum()) == 0
    if case.edges:
        flat = torch.cat([t.reshape(-1) for t in (gin, gw) if t is not None])
        neg0 = ((flat == 0) & (C.bits(flat) < 0)).sum().item()
        sub = ((flat != 0) & (flat.abs() < 2.0 ** -126)).sum().item()
        print("case %s: %d results are -0, %d subnormal" % (case.name, neg0, sub))
        assert neg0 > 0 and sub > 0, "the edge recipe no longer reaches -0 / subnormal results"


def test_prepared_gradient_has_the_input_size_after_the_convolution():
    for case in C.CASES:
        ho, wo = C.out_size(case)
        p = C.prepared_gradient(torch.ones(1, 1, ho, wo), case.h, case.w, case.k, case.s)
        assert p.shape[2] - case.k + 1 == case.h and p.shape[3] - case.k + 1 == case.w
        assert p.sum().item() == ho * wo


def test_switch_defaults_off_restores_and_nests():
    from pseudocylindrical_convolution_amd import PCONV
    assert PCONV.conv_grad_is_native() is False
    assert not PCONV.native_conv_grad()          # a query leaves it
    assert PCONV.conv_grad_is_native() is False
    with PCONV.native_conv_grad(True) as previous:
        assert not previous and PCONV.conv_grad_is_native()
        with PCONV.native_conv_grad(False):
            assert not PCONV.conv_grad_is_native()
            with PCONV.native_conv_grad(True):
                assert PCONV.conv_grad_is_native()
            assert not PCONV.conv_grad_is_native()
        assert PCONV.conv_grad_is_native()
    assert PCONV.conv_grad_is_native() is False
    with pytest.raises(ZeroDivisionError):
        with PCONV.native_conv_grad(True):
            1 / 0
    assert PCONV.conv_grad_is_native() is False
    previous = PCONV.native_conv_grad(True)      # the plain setter returns what was there
    assert not previous and PCONV.conv_grad_is_native()
    PCONV.native_conv_grad(previous)
    assert PCONV.conv_grad_is_native() is False
    # ... and it is not the ordered-backward switch
    with PCONV.native_conv_grad(True):
        assert not PCONV.backward_is_ordered()


def test_train_conv_flag_parses_and_native_is_refused_on_the_cpu_backend(oracle_backend, tmp_path):
    from pseudocylindrical_convolution_amd import PCONV, train
    parser = train.build_parser()
    assert parser.parse_args([]).conv == "vendor"
    assert parser.parse_args(["--conv", "native"]).conv == "native"
    with pytest.raises(SystemExit):
        parser.parse_args(["--conv", "cudnn"])
    with pytest.raises(RuntimeError, match="--conv native needs the HIP backend"):
        train.native_conv_mode()
    args = parser.parse_args(["--conv", "native", "--device", "cpu", "--base", "--synthetic", "2", "--base-dir", str(tmp_path)])
    with pytest.raises(RuntimeError, match="--conv native needs"):
        train.Job(0, 1, args)
    assert PCONV.conv_grad_is_native() is False
    assert not (tmp_path / "save_models").exists()   # refused before anything is set up


def test_tileconv2d_with_the_switch_off_calls_the_library_convolution_as_before(oracle_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import PCONV, model_zoo_v2 as Z
    from pseudocylindrical_convolution_amd.PCONV_operator import ops
    calls = []
    real = torch.nn.functional.conv2d

    def spy(*args, **kwargs):
        calls.append((args, kwargs))
        return real(*args, **kwargs)

    def never(*args, **kwargs):
        raise AssertionError("the native autograd bridge was taken with the switch off")

    monkeypatch.setattr(torch.nn.functional, "conv2d", spy)
    monkeypatch.setattr(ops.TileConvCall, "apply", never)
    assert not PCONV.conv_grad_is_native()
    torch.manual_seed(0)
    conv, prelu = Z.TileConv2d(4, 6, 3, 2), torch.nn.PReLU(6)
    x = torch.randn(2, 4, 9, 11, requires_grad=True)
    y = conv.fuse(x, prelu)
    assert len(calls) == 1
    args, kwargs = calls[0]
    assert not kwargs and len(args) == 4
    assert args[0] is x and args[1] is conv.weight and args[2] is conv.bias and args[3] == conv.stride
    expected = torch.nn.functional.prelu(real(x, conv.weight, conv.bias, conv.stride), prelu.weight)
    assert torch.equal(y, expected)
    y.sum().backward()
    assert x.grad is not None and conv.weight.grad is not None and conv.bias.grad is not None
    # a backend without the kernels ignores the switch: the oracle has no tile_conv2d_backward
    with PCONV.native_conv_grad(True):
        conv(x)
    assert len(calls) == 2


def test_bad_arguments_are_refused_before_any_launch():
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    d = 4096   # never dereferenced: the checks come first
    assert lib.pconv_conv2d_wgrad(d, d, d, d, None, 1, 4, 8, 8, 4, 3, 1, None) < 0 and b"null" in lib.pconv_last_error()
    assert lib.pconv_conv2d_wgrad(d, d, d, d, d, 1, 4, 8, 8, 4, 5, 1, None) < 0 and b"k=5" in lib.pconv_last_error()
    assert lib.pconv_conv2d_wgrad(d, d, d, d, d, 1, 4, 8, 8, 4, 3, 3, None) < 0 and b"stride=3" in lib.pconv_last_error()
    assert lib.pconv_conv2d_wgrad(d, d, d, d, d, 1, 1 << 20, 8, 8, 1 << 20, 3, 1, None) < 0 and b"int32" in lib.pconv_last_error()
    assert lib.pconv_conv2d_dgrad(d, d, None, d, 1, 4, 8, 8, 4, 3, 1, None) < 0 and b"null" in lib.pconv_last_error()
    assert lib.pconv_conv2d_dgrad(d, d, d, None, 1, 4, 8, 8, 4, 3, 2, None) < 0 and b"workspace" in lib.pconv_last_error()
    assert lib.pconv_conv2d_dgrad(d, d, d, d, 1, 4, 8, 8, 4, 2, 1, None) < 0 and b"k=2" in lib.pconv_last_error()
    assert lib.pconv_conv_grad_prepare(d, d + 4, 1, 4, 8, 8, 3, 1, None) < 0 and b"aligned" in lib.pconv_last_error()
    assert lib.pconv_conv2d_wgrad_workspace_bytes(0, 4, 4, 3) < 0
    assert lib.pconv_conv2d_wgrad_workspace_bytes(32, 192, 192, 3) == 32 * 192 * 192 * 9 * 4 + 32 * 192 * 8
    assert lib.pconv_conv2d_dgrad_workspace_bytes(2, 4, 8, 9, 1, 1) == 0
    assert lib.pconv_conv2d_dgrad_workspace_bytes(2, 4, 8, 9, 3, 2) == 2 * 4 * 10 * 11 * 4


def test_cpu_tensors_are_refused_by_the_python_entry():
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd._native import PconvError
    x, weight, gout = C.inputs(C.BY_NAME["c"])
    for need in ((True, False, False), (False, True, False), (False, False, True)):
        with pytest.raises(PconvError, match="GPU tensor"):
            PCONV.tile_conv2d_backward(x, weight, gout, 1, need)


def test_the_viewport_loss_keeps_a_library_convolution(monkeypatch):
    """what `--conv native` does NOT cover, pinned so that the documents cannot drift from the code: the SSIM term of
    the default --loss viewport blurs with torch.nn.functional.conv2d (an 11 x 11 depthwise kernel, five calls), while
    train.forward_losses under --loss ws calls none beyond the model's own"""
    from pseudocylindrical_convolution_amd import train
    from pseudocylindrical_convolution_amd.PCONV_operator import SSIM
    calls = []
    real = torch.nn.functional.conv2d
    monkeypatch.setattr(torch.nn.functional, "conv2d", lambda x, w, *a, **k: (calls.append((tuple(w.shape), k)), real(x, w, *a, **k))[1])
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 3, 32, 48, generator=g), torch.rand(1, 3, 32, 48, generator=g)
    SSIM(11, 3)(a, b)
    assert len(calls) == 5 and all(shape == (3, 1, 11, 11) and k.get("groups") == 3 for shape, k in calls), calls
    del calls[:]
    args = train.build_parser().parse_args(["--loss", "ws"])
    train.forward_losses(args, lambda data: b, a, None, None, None)
    assert calls == []
