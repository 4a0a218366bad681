"""The native masked 5x5 convolution without a GPU: its CPU twins (tests/masked_conv_cases.py) against float64 autograd
within the chain's own bound, the PCONV.native_masked_conv switch, `train.py --conv native-all`, the argument checks of
the pconv_conv5* entry points, and _MaskConv's unchanged library branch."""
import pytest
import torch

import masked_conv_cases as M


@pytest.mark.parametrize("case", [c for c in M.CASES if c.name != "e"], ids=[c for c in M.IDS if c != "e"])
def test_twin_is_within_the_chains_bound_of_float64_autograd(case):
    x, weight, bias, gout = M.inputs(case)
    y, gin, gw, gb = M.twin(case)
    assert y.shape == gout.shape and gw.shape == weight.shape and gb.shape == (case.cout,)
    yref = torch.nn.functional.conv2d(x.double(), weight.double(), bias.double())
    rin, rw, rb = M.f64_grads(x, weight, gout, 1)
    bin_, bw, bb = M.bounds(case, x, weight, gout)
    for name, got, ref, bound in (("y", y, yref, M.forward_bound(case, x, weight, bias)), ("gin", gin, rin, bin_),
                                  ("gw", gw, rw, bw), ("gb", gb, rb, bb)):
        if got is None:
            assert name == "gin" and not case.need_x
            continue
        err = (got.double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print("case %s %s: max |twin - f64| %.3e, largest share of the bound %.3g" % (case.name, name, err.max().item(), worst))
        assert bool((err <= bound).all()), "%s of case %s leaves the bound: share %.3g" % (name, case.name, worst)
    if case.edges:
        flat = torch.cat([t.reshape(-1) for t in (y, gin, gw) if t is not None])
        neg0 = ((flat == 0) & (M.bits(flat) < 0)).sum().item()
        sub = ((flat != 0) & (flat.abs() < 2.0 ** -126)).sum().item()
        print("case %s: %d results are -0, %d subnormal" % (case.name, neg0, sub))
        assert neg0 > 0 and sub > 0, "the edge recipe no longer reaches -0 / subnormal results"


def test_the_mask_keeps_about_half_of_the_taps_and_the_weight_gradient_is_dense():
    first, hidden = M.kept_fraction(M.BY_NAME["b"]), M.kept_fraction(M.BY_NAME["a"])
    print("kept taps: first layer %.3f, hidden layer %.3f" % (first, hidden))
    assert 0.4 < first < 0.5 < hidden < 0.6
    # the gradient of a masked tap is not zero: the twin (and the kernel) return the dense gradient
    case = M.BY_NAME["a"]
    gone = M.masked(torch.ones(case.cout, case.cin, 5, 5), case) == 0
    assert bool((M.twin(case)[2][gone] != 0).any())
    assert bool((M.inputs(case)[1][gone] == 0).all())


def test_switch_defaults_off_restores_nests_and_is_independent_of_the_other_two():
    from pseudocylindrical_convolution_amd import PCONV
    assert PCONV.masked_conv_is_native() is False
    assert not PCONV.native_masked_conv()          # a query leaves it
    assert PCONV.masked_conv_is_native() is False
    with PCONV.native_masked_conv(True) as previous:
        assert not previous and PCONV.masked_conv_is_native()
        with PCONV.native_masked_conv(False):
            assert not PCONV.masked_conv_is_native()
            with PCONV.native_masked_conv(True):
                assert PCONV.masked_conv_is_native()
            assert not PCONV.masked_conv_is_native()
        assert PCONV.masked_conv_is_native()
    assert PCONV.masked_conv_is_native() is False
    with pytest.raises(ZeroDivisionError):
        with PCONV.native_masked_conv(True):
            1 / 0
    assert PCONV.masked_conv_is_native() is False
    previous = PCONV.native_masked_conv(True)      # the plain setter returns what was there
    assert not previous and PCONV.masked_conv_is_native()
    PCONV.native_masked_conv(previous)
    assert PCONV.masked_conv_is_native() is False
    # neither switch changes another, in both directions
    with PCONV.native_masked_conv(True):
        assert not PCONV.conv_grad_is_native() and not PCONV.backward_is_ordered()
        with PCONV.native_conv_grad(True), PCONV.ordered_backward(True):
            assert PCONV.masked_conv_is_native()
        assert PCONV.masked_conv_is_native() and not PCONV.conv_grad_is_native() and not PCONV.backward_is_ordered()
    with PCONV.native_conv_grad(True), PCONV.ordered_backward(True):
        assert not PCONV.masked_conv_is_native()
        with PCONV.native_masked_conv(True):
            assert PCONV.conv_grad_is_native() and PCONV.backward_is_ordered()
        assert PCONV.conv_grad_is_native() and PCONV.backward_is_ordered() and not PCONV.masked_conv_is_native()
    assert not (PCONV.masked_conv_is_native() or PCONV.conv_grad_is_native() or PCONV.backward_is_ordered())


def test_train_conv_native_all_parses_and_is_refused_on_the_cpu_backend(oracle_backend, tmp_path):
    from pseudocylindrical_convolution_amd import PCONV, train
    parser = train.build_parser()
    assert parser.parse_args([]).conv == "vendor"
    assert parser.parse_args(["--conv", "native"]).conv == "native"
    assert parser.parse_args(["--conv", "native-all"]).conv == "native-all"
    with pytest.raises(RuntimeError, match="--conv native-all needs the HIP backend"):
        with train.native_all_conv_mode():
            pass
    assert PCONV.conv_grad_is_native() is False and PCONV.masked_conv_is_native() is False
    # --device cpu; then --device cuda on a backend without the kernels (the oracle): both before anything is set up
    for device in ("cpu", "cuda"):
        args = parser.parse_args(["--conv", "native-all", "--device", device, "--synthetic", "2", "--base-dir", str(tmp_path)])
        with pytest.raises(RuntimeError, match="--conv native-all needs"):
            train.Job(0, 1, args)
        assert PCONV.conv_grad_is_native() is False and PCONV.masked_conv_is_native() is False
        assert not (tmp_path / "save_models").exists()
    # no SSIM module is constructed under native-all, and forward_losses takes the kernel's SSIM without one
    assert train.make_sim_func(parser.parse_args(["--conv", "native-all"]), "cpu") is None
    assert train.make_sim_func(parser.parse_args(["--loss", "ws"]), "cpu") is None
    assert type(train.make_sim_func(parser.parse_args(["--conv", "native"]), "cpu")).__name__ == "SSIM"


def test_forward_losses_without_an_ssim_module_takes_loss_terms_uniform(monkeypatch):
    """--conv native-all under --loss viewport: the SSIM term is sphere_metrics.loss_terms(uniform) over the views;
    on CPU tensors that is its float64 torch statement, which is pytorch_ssim's map: checked against SSIM(11, 3)"""
    from pseudocylindrical_convolution_amd import train
    from pseudocylindrical_convolution_amd.PCONV_operator import SSIM
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2, 3, 32, 48, generator=g), torch.rand(2, 3, 32, 48, generator=g)
    args = train.build_parser().parse_args(["--conv", "native-all"])
    ident = lambda t: t
    mse, ssim, rate = train.forward_losses(args, lambda data: b, a, ident, ident, None)
    assert rate is None and abs(mse.item() - ((a - b) ** 2).mean().item()) < 1e-7
    ref = SSIM(11, 3)(a.double(), b.double()).item()
    # (pytorch_ssim rounds its window to float32 before it is cast: 2^-24 relative per tap, on a value of order 1)
    assert abs(ssim.item() - ref) < 1e-6, (ssim.item(), ref)
    # with a module the branch is the module's, as before
    calls = []
    assert train.forward_losses(args, lambda data: b, a, ident, ident, lambda x, y: calls.append(1) or torch.tensor(0.5))[1] == 0.5
    assert calls == [1]


def test_bad_arguments_are_refused_before_any_launch():
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    d = 4096   # never dereferenced: the checks come first

    def refused(rc, word):
        return rc < 0 and word in lib.pconv_last_error()

    # forward: null pointers, h or w below 5, shapes beyond int32, a misaligned pack
    assert refused(lib.pconv_conv5(None, d, d, d, 1, 4, 8, 8, 4, None), b"null")
    assert refused(lib.pconv_conv5(d, None, d, d, 1, 4, 8, 8, 4, None), b"null")
    assert refused(lib.pconv_conv5(d, d, d, None, 1, 4, 8, 8, 4, None), b"null")
    assert refused(lib.pconv_conv5(d, d, d, d, 1, 4, 4, 8, 4, None), b">= 5")
    assert refused(lib.pconv_conv5(d, d, d, d, 1, 4, 8, 4, 4, None), b">= 5")
    assert refused(lib.pconv_conv5(d, d, d, d, 0, 4, 8, 8, 4, None), b"bad shape")
    assert refused(lib.pconv_conv5(d, d, d, d, 1, 1 << 20, 8, 8, 1 << 20, None), b"int32")
    assert refused(lib.pconv_conv5(d, d, d, d, 1, 4, 1 << 16, 1 << 16, 4, None), b"int32")
    assert refused(lib.pconv_conv5(d, d + 4, d, d, 1, 4, 8, 8, 4, None), b"aligned")
    # packs
    assert refused(lib.pconv_conv5_pack_weight(None, d, 4, 4, None), b"null")
    assert refused(lib.pconv_conv5_pack_weight(d, d, 1 << 20, 1 << 20, None), b"int32")
    assert refused(lib.pconv_conv5_pack_weight_transposed(d, None, 4, 4, None), b"null")
    assert refused(lib.pconv_conv5_pack_weight_transposed(d, d, 0, 4, None), b"bad shape")
    assert lib.pconv_conv5_packed_size(1 << 20, 1 << 20, None, None) < 0
    # cout padded to 32 / 96 / 192, cin to 2, times the 25 taps
    assert lib.pconv_conv5_packed_size(42, 14, None, None) == 96 * 14 * 25
    assert lib.pconv_conv5_packed_size(14, 43, None, None) == 32 * 44 * 25
    assert lib.pconv_conv5_packed_size(144, 144, None, None) == 192 * 144 * 25
    # data gradient: null pointers, a missing / misaligned workspace, small and oversized shapes
    assert refused(lib.pconv_conv5_dgrad(d, d, None, d, 1, 4, 8, 8, 4, None), b"null pointer")
    assert refused(lib.pconv_conv5_dgrad(d, d, d, None, 1, 4, 8, 8, 4, None), b"null workspace")
    assert refused(lib.pconv_conv5_dgrad(d, d, d, d + 4, 1, 4, 8, 8, 4, None), b"aligned")
    assert refused(lib.pconv_conv5_dgrad(d, d, d, d, 1, 4, 4, 8, 4, None), b">= 5")
    assert refused(lib.pconv_conv5_dgrad(d, d, d, d, 1, 1 << 20, 8, 8, 1 << 20, None), b"int32")
    # weight / bias gradient
    assert refused(lib.pconv_conv5_wgrad(d, None, d, d, d, 1, 4, 8, 8, 4, None), b"null pointer")
    assert refused(lib.pconv_conv5_wgrad(None, d, d, d, d, 1, 4, 8, 8, 4, None), b"null pointer")   # gw without the input
    assert refused(lib.pconv_conv5_wgrad(d, d, None, None, d, 1, 4, 8, 8, 4, None), b"null pointer")
    assert refused(lib.pconv_conv5_wgrad(d, d, d, d, None, 1, 4, 8, 8, 4, None), b"null workspace")
    assert refused(lib.pconv_conv5_wgrad(d, d, d, d, d + 8, 1, 4, 8, 8, 4, None), b"aligned")
    assert refused(lib.pconv_conv5_wgrad(d, d, d, d, d, 1, 4, 8, 4, 4, None), b">= 5")
    assert refused(lib.pconv_conv5_wgrad(d, d, d, d, d, 1, 1 << 20, 8, 8, 1 << 20, None), b"int32")
    # the workspace sizes are the documented formulas
    assert lib.pconv_conv5_wgrad_workspace_bytes(0, 4, 4) < 0
    assert lib.pconv_conv5_wgrad_workspace_bytes(32, 144, 144) == 32 * 144 * 144 * 25 * 4 + 32 * 144 * 8
    assert lib.pconv_conv5_wgrad_workspace_bytes(1, 1, 3) == 304 + 24            # 300 bytes of partials rounded up to 16
    assert lib.pconv_conv5_dgrad_workspace_bytes(2, 4, 8, 9) == 2 * 4 * 12 * 13 * 4
    assert lib.pconv_conv5_dgrad_workspace_bytes(2, 4, 4, 9) < 0
    # ... and the k in {1, 3} entry points keep refusing k = 5
    assert refused(lib.pconv_conv2d(d, d, d, d, 1, 4, 8, 8, 4, 5, 1, 0, None, None, 0, None, None, 0, 0, None, None), b"k=5")
    assert refused(lib.pconv_conv_pack_weight(d, d, 4, 4, 5, None), b"bad argument")
    assert refused(lib.pconv_conv_pack_weight_transposed(d, d, 4, 4, 5, None), b"bad argument")
    assert refused(lib.pconv_conv2d_dgrad(d, d, d, d, 1, 4, 8, 8, 4, 5, 1, None), b"k=5")


def test_cpu_tensors_are_refused_by_the_python_entries():
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd._native import PconvError
    x, weight, bias, gout = M.inputs(M.BY_NAME["b"])
    with pytest.raises(PconvError, match="GPU tensor"):
        PCONV.conv5x5(object(), x, weight, bias)
    for need in ((True, False, False), (False, True, False), (False, False, True)):
        with pytest.raises(PconvError, match="GPU tensor"):
            PCONV.conv5x5_backward(x, weight, gout, need)
    with pytest.raises(PconvError):
        PCONV.tile_conv2d(object(), x, weight, bias, 1)        # the k in {1, 3} surface does not take it either
    with pytest.raises(PconvError):
        PCONV.tile_conv2d_backward(x, weight, gout, 1)


def _spies(monkeypatch):
    from pseudocylindrical_convolution_amd.PCONV_operator import ops
    calls = []
    real = torch.nn.functional.conv2d

    def spy(*args, **kwargs):
        calls.append((args, kwargs))
        return real(*args, **kwargs)

    def never(*args, **kwargs):
        raise AssertionError("the native autograd bridge of the masked convolution was taken")

    monkeypatch.setattr(torch.nn.functional, "conv2d", spy)
    monkeypatch.setattr(ops.MaskConvCall, "apply", never)
    return calls, real


def test_maskconv2_on_a_backend_without_the_kernels_ignores_the_switch(oracle_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd.PCONV_operator import MaskConv2
    calls, real = _spies(monkeypatch)
    case = M.BY_NAME["b"]
    torch.manual_seed(0)
    conv = MaskConv2(case.G, 1, 3, 5, hidden=False)
    x = M.inputs(case)[0].clone().requires_grad_(True)
    with PCONV.native_masked_conv(True):
        y = conv(x)
    assert len(calls) == 1
    args, kwargs = calls[0]
    assert not kwargs and len(args) == 3 and args[0] is x and args[1] is conv.weight and args[2] is conv.bias
    gone = M.masked(torch.ones_like(conv.weight), case) == 0
    assert bool(gone.any()) and bool((conv.weight.detach()[gone] == 0).all())        # ... with the masked weight
    assert torch.equal(y, real(x, M.masked(conv.weight, case), conv.bias))
    y.sum().backward()
    assert x.grad is not None and conv.weight.grad is not None and conv.bias.grad is not None


def test_maskconv_with_the_switch_off_calls_the_library_convolution_as_before(oracle_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd.PCONV_operator import MaskConv2, MaskConv3
    calls, real = _spies(monkeypatch)
    assert not PCONV.masked_conv_is_native()
    torch.manual_seed(0)
    x = torch.randn(1, 14, 7, 9)
    for conv in (MaskConv2(14, 1, 3, 5, hidden=False), MaskConv3(14, 1, 3, 5, hidden=False), MaskConv3(14, 1, 3, 3)):
        del calls[:]
        y = conv(x)
        assert len(calls) == 1 and calls[0][0][1] is conv.weight
        assert torch.equal(y, real(x, conv.weight, conv.bias))
