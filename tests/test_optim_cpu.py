"""optim.Adam on CPU tensors: the numpy twin of csrc/optim.hip (the definition of include/pconv_hip.h restated)
against float64 Adam, its state interchange with torch.optim.Adam, what it refuses, and the edges of the norm."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_cases as C


def _optim():
    from pseudocylindrical_convolution_amd import optim
    return optim


@pytest.mark.parametrize("clip", [0.0, C.CLIP_BINDS])
def test_twenty_steps_are_as_close_to_float64_adam_as_torch_in_float32(clip):
    """max|p_twin - p_64| <= 2 * max|p_torch32 - p_64| + 2^-23 * max|p|: both sides measured here.  The factor 2
    covers a different rounding order among about five roundings per step.  Measured (twin, torch32; max|p| 3.98):
    clip 0: 1.01e-06, 1.01e-06; clip 0.1: 9.59e-07, 9.59e-07."""
    case, steps = C.BY_NAME["sizes"], 20
    p64 = C.torch_steps(case, steps, True, clip, torch.float64)[0]
    p32 = C.torch_steps(case, steps, True, clip, torch.float32)[0]
    twin = C.native_steps(case, steps, True, clip)[0]
    err = lambda ps: max((p.detach().double() - q.detach()).abs().max().item() for p, q in zip(ps, p64))
    top = max(q.detach().abs().max().item() for q in p64)
    print("clip %g: max|p_twin - p_64| = %.3g, max|p_torch32 - p_64| = %.3g, max|p| = %.3g" % (clip, err(twin), err(p32), top))
    assert err(twin) <= 2 * err(p32) + 2.0 ** -23 * top


@pytest.mark.parametrize("name", ["sizes", "many", "skipped"])
@pytest.mark.parametrize("with_acc", [False, True])
def test_the_norm_is_the_float64_norm_within_float64_rounding(name, with_acc):
    """the step gradient is acc + grad rounded to fp32; its squares are exact in fp64, so the two-stage sum differs
    from any other fp64 sum of n terms by at most n * 2^-53 relative (far less in fact); the clip coefficient is
    clip_grad_norm_'s, rounded once to fp32"""
    case = C.BY_NAME[name]
    figures = C.native_steps(case, 1, with_acc, C.CLIP_BINDS)[3]
    total, norm, coef = figures[0]
    assert norm.dtype == torch.float64 and norm.dim() == 0 and coef.dtype == torch.float32
    gs = [g if not with_acc else a + g for g, a in zip(C.gradients(case, 0), C.accumulators(case, 0)) if g is not None]
    n = sum(g.numel() for g in gs)
    ref = math.fsum(float(x) ** 2 for g in gs for x in g.reshape(-1).tolist())
    assert abs(total.item() - ref) <= n * 2.0 ** -53 * ref
    assert abs(norm.item() - math.sqrt(ref)) <= n * 2.0 ** -53 * math.sqrt(ref)
    assert coef.item() == np.float32(min(1.0, np.float64(np.float32(C.CLIP_BINDS)) / (norm.item() + 1e-6)))
    assert C.native_steps(case, 1, with_acc, 0.0)[3][0][2].item() == 1.0      # no clip: coef 1, the norm all the same
    assert C.native_steps(case, 1, with_acc, 0.0)[3][0][1].item() == norm.item()


def test_state_dicts_interchange_with_torch_adam_both_ways():
    optim, case = _optim(), C.BY_NAME["groups"]
    # torch -> native: one native step from the loaded state is the twin applied to that state
    tp, topt, _ = C.torch_steps(case, 3, False, 0.0, torch.float32)
    params, nopt = C.build(case, lambda groups: optim.Adam(groups))
    with torch.no_grad():
        for p, q in zip(params, tp):
            p.copy_(q)
    nopt.load_state_dict(copy.deepcopy(topt.state_dict()))
    st = C.states(nopt, params)
    assert all(float(s["step"]) == 3 and torch.equal(s["exp_avg"], topt.state[q]["exp_avg"]) for s, q in zip(st, tp))
    C.set_gradients(case, 3, params)
    items = []
    for gi, group in enumerate(nopt.param_groups):
        for p in group["params"]:
            s = nopt.state[p]
            items.append(dict(p=p.detach().clone().view(-1).numpy(), grad=p.grad.clone().view(-1).numpy(), acc=None,
                              m=s["exp_avg"].clone().view(-1).numpy(), v=s["exp_avg_sq"].clone().view(-1).numpy(),
                              scalars=optim._scalars(case.lrs[gi], 0.9, 0.999, 1e-8, 4.0)))
    optim._twin(items, 0.0)
    nopt.step()
    for p, it in zip(params, items):
        assert torch.equal(C.bits(p), C.bits(torch.from_numpy(it["p"]).view(p.shape)))
        assert torch.equal(C.bits(nopt.state[p]["exp_avg_sq"]), C.bits(torch.from_numpy(it["v"]).view(p.shape)))
        assert float(nopt.state[p]["step"]) == 4
    # native -> torch: the state loads and torch's step runs on it, close to the native one (not bit-equal: another
    # order of roundings)
    nparams, nopt2, _, _ = C.native_steps(case, 3, False, 0.0)
    tparams, topt2 = C.build(case, lambda groups: torch.optim.Adam(groups))
    with torch.no_grad():
        for p, q in zip(tparams, nparams):
            p.copy_(q)
    topt2.load_state_dict(copy.deepcopy(nopt2.state_dict()))
    assert [g["lr"] for g in topt2.param_groups] == case.lrs
    C.set_gradients(case, 3, tparams)
    C.set_gradients(case, 3, nparams)
    topt2.step()
    nopt2.step()
    for p, q in zip(tparams, nparams):
        assert float(topt2.state[p]["step"]) == 4
        assert (p - q).abs().max().item() <= 1e-6 * max(1.0, q.abs().max().item())


def test_refusals_name_the_offender_and_leave_the_state_untouched():
    optim, case = _optim(), C.BY_NAME["sizes"]
    for name, value in (("weight_decay", 0.1), ("amsgrad", True), ("maximize", True)):
        with pytest.raises(ValueError, match=name):
            optim.Adam([torch.zeros(3, requires_grad=True)], **{name: value})
    params, opt, _, _ = C.native_steps(case, 1, False, 0.0)
    before = copy.deepcopy(opt.state_dict())
    snapshot = [p.detach().clone() for p in params]

    def untouched():
        now = opt.state_dict()
        assert all(torch.equal(p, q) for p, q in zip(params, snapshot))
        for k, s in before["state"].items():
            assert all(torch.equal(s[n], now["state"][k][n]) for n in ("step", "exp_avg", "exp_avg_sq"))

    p32, p64 = torch.zeros(5, requires_grad=True), torch.zeros(3, dtype=torch.float64, requires_grad=True)
    mixed = optim.Adam([p32, p64])
    p32.grad, p64.grad = torch.ones(5), torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"parameter 1 .*float64"):
        mixed.step()
    assert len(mixed.state) == 0 and not p32.detach().any()       # the float32 one in front of it did not step either
    C.set_gradients(case, 1, params)
    params[8].grad = params[8].grad.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    with pytest.raises(ValueError, match=r"gradient 8 .*not dense"):
        opt.step()
    untouched()
    C.set_gradients(case, 1, params)
    accs = [a for a in C.accumulators(case, 1)]
    accs[3] = accs[3].half()
    with pytest.raises(ValueError, match=r"accumulator 3 .*float16"):
        opt.step(acc=accs, clip=0.1)
    untouched()
    with pytest.raises(ValueError, match="accumulators for"):
        opt.step(acc=accs[:-1])
    untouched()
    for name, value in (("weight_decay", 0.01), ("amsgrad", True), ("maximize", True)):
        opt.param_groups[0][name] = value
        with pytest.raises(ValueError, match=name):
            opt.step()
        opt.param_groups[0][name] = before["param_groups"][0][name]
        untouched()
    opt.step()   # and with nothing wrong it steps
    assert not torch.equal(params[0], snapshot[0])


def test_a_parameter_without_gradient_is_skipped_and_keeps_its_step_count():
    case = C.BY_NAME["skipped"]
    params, opt, accs, _ = C.native_steps(case, 3, True, C.CLIP_BINDS)
    start = [p for group in C.parameters(case) for p in group]
    assert params[case.skipped] not in opt.state or len(opt.state[params[case.skipped]]) == 0
    assert torch.equal(params[case.skipped].detach(), start[case.skipped])
    assert torch.equal(accs[case.skipped], C.accumulators(case, 2)[case.skipped])   # its accumulator is left alone
    assert all(float(opt.state[p]["step"]) == 3 for i, p in enumerate(params) if i != case.skipped)
    assert all(not a.any() for i, a in enumerate(accs) if i != case.skipped)
    # it joins later with a count of its own: its first step has the bias corrections of t = 1
    C.set_gradients(C.BY_NAME["sizes"], 3, params)
    opt.step()
    assert float(opt.state[params[case.skipped]]["step"]) == 1 and float(opt.state[params[0]]["step"]) == 4
    g = C.gradients(C.BY_NAME["sizes"], 3)[case.skipped]
    moved = (params[case.skipped].detach() - start[case.skipped]).abs()
    assert torch.allclose(moved[g.abs() > 1e-3], torch.tensor(1e-3), rtol=1e-3)     # Adam's first step: lr * sign


def test_a_step_counts_as_an_in_place_write_of_what_it_wrote():
    """the step writes through raw pointers; caches keyed on a parameter's version (the convolutions' packed weights)
    must see it as torch's in-place step"""
    optim = _optim()
    case = C.BY_NAME["skipped"]
    params, opt = C.build(case, lambda groups: optim.Adam(groups))
    C.set_gradients(case, 0, params)
    accs = C.accumulators(case, 0)
    before = [(p._version, a._version) for p, a in zip(params, accs)]
    opt.step(acc=accs, clip=0.1)
    for i, (p, a) in enumerate(zip(params, accs)):
        assert (p._version > before[i][0]) == (i != case.skipped) and (a._version > before[i][1]) == (i != case.skipped)


def test_inf_and_nan_gradients_do_what_the_definition_says():
    """an infinite norm gives coef 0, a NaN norm a NaN coef (the minimum does not drop it); without a clip coef is 1"""
    for clip in (C.CLIP_BINDS, C.CLIP_LOOSE):
        params, _, _, fig = C.native_steps(C.BY_NAME["inf"], 1, False, clip)
        total, norm, coef = fig[0]
        assert math.isinf(total.item()) and math.isinf(norm.item()) and coef.item() == 0.0
        flat = params[0].detach().view(-1)
        assert flat[5].isnan() and flat.isnan().sum() == 1          # inf * 0 is NaN there; g * 0 = 0 everywhere else
        assert torch.equal(params[1].detach(), C.parameters(C.BY_NAME["inf"])[0][1])   # m' = 0: p - step * (0 / eps)
        params, _, _, fig = C.native_steps(C.BY_NAME["nan"], 1, False, clip)
        assert all(math.isnan(x.item()) for x in fig[0])
        assert all(p.detach().isnan().all() for p in params)
    params, _, _, fig = C.native_steps(C.BY_NAME["inf"], 1, False, 0.0)
    assert math.isinf(fig[0][1].item()) and fig[0][2].item() == 1.0
    assert params[0].detach().view(-1).isnan().sum() == 1 and not params[1].detach().isnan().any()


def test_the_twin_keeps_subnormals_and_signed_zeros():
    """the edge list against the same operations done one element at a time in numpy scalars"""
    optim, case = _optim(), C.BY_NAME["small"]
    params, opt, accs, fig = C.native_steps(case, 1, True, 0.0)
    f = np.float32
    step_size, bc2, eps, omb1, b2, omb2 = optim._scalars(1e-3, 0.9, 0.999, 1e-8, 1.0)
    p0, (m0, v0) = C.parameters(case)[0][1], [x[1] for x in C.moments(case)]
    g0, a0 = C.gradients(case, 0)[1], C.accumulators(case, 0)[1]
    with np.errstate(all="ignore"):
        for i in range(7):
            g = f(a0[i].item()) + f(g0[i].item())
            g = g * f(1.0)
            m = f(m0[i].item()) + omb1 * (g - f(m0[i].item()))
            v = (b2 * f(v0[i].item())) + omb2 * (g * g)
            p = f(p0[i].item()) - step_size * (m / (np.sqrt(v) / bc2 + eps))
            assert C.bits(params[1])[i].item() == np.asarray(p, dtype=np.float32).view(np.int32).item()
            assert C.bits(opt.state[params[1]]["exp_avg"])[i].item() == np.asarray(m, dtype=np.float32).view(np.int32).item()
    assert any(0 < abs(x) < 2.0 ** -126 for x in opt.state[params[0]]["exp_avg"].view(-1).tolist())   # subnormals live


def test_entry_points_return_einval_before_anything_is_launched():
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    counts = (ctypes.c_longlong * 2)(4097, 7)
    dummy = 4096   # never dereferenced: the checks come first
    assert lib.pconv_host_optim_segments(ctypes.addressof(counts), 2, None) == 3
    table = (ctypes.c_int32 * 6)()
    assert lib.pconv_host_optim_segments(ctypes.addressof(counts), 2, ctypes.addressof(table)) == 3
    assert list(table) == [0, 0, 0, 1, 1, 0]
    assert lib.pconv_optim_workspace_bytes(2, 3) == 32 + 3 * 8
    c = ctypes.addressof(counts)
    for args in ((None, dummy, c, 2, 3, dummy), (dummy, None, c, 2, 3, dummy), (dummy, dummy, None, 2, 3, dummy),
                 (dummy, dummy, c, 2, 3, None), (dummy, dummy, c, 2, 2, dummy), (dummy, dummy, c, 2, 4, dummy),
                 (dummy, dummy, c, 0, 3, dummy), (dummy, dummy, c, 2, -1, dummy)):
        assert lib.pconv_optim_sqnorm(*args[:5], 0.1, args[5], None) == -1 and b"optim_sqnorm" in lib.pconv_last_error()
        assert lib.pconv_optim_adam(*args, None) == -1 and b"optim_adam" in lib.pconv_last_error()
    bad = (ctypes.c_longlong * 2)(4097, -7)
    assert lib.pconv_optim_adam(dummy, dummy, ctypes.addressof(bad), 2, 2, dummy, None) == -1
    assert lib.pconv_host_optim_segments(ctypes.addressof(bad), 2, None) == -1
