"""GPU: the optimiser step of csrc/optim.hip (optim.Adam on GPU tensors, PCONV.optim_step) held BIT FOR BIT to its
CPU twin on the cases of tests/optim_cases.py, its independence of the list, the C ABI's refusals, and a model trained
with it."""
import contextlib
import ctypes

import pytest
import torch

import optim_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c.name for c in C.CASES]


def same_bits(got, ref, what):
    assert C.same_bits(got, ref), "%s: %d of %d entries differ" % (
        what, int((C.bits(got) != C.bits(ref)).sum()), ref.numel())


@pytest.mark.parametrize("clip", [C.CLIP_BINDS, C.CLIP_LOOSE], ids=["clip-binds", "clip-loose"])
@pytest.mark.parametrize("with_acc", [False, True], ids=["grad", "acc+grad"])
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_three_steps_are_the_twin_bit_for_bit_twice(hip_backend, case, with_acc, clip):
    """parameters, both moments, the zeroed accumulators, total, norm and coef after each of three consecutive steps
    (the later ones from non-zero state)"""
    tp, topt, tacc, tfig = C.native_steps(case, 3, with_acc, clip, "cpu")
    for call in range(2):
        gp, gopt, gacc, gfig = C.native_steps(case, 3, with_acc, clip, DEV)
        for step, (g, t) in enumerate(zip(gfig, tfig)):
            for name, a, b in zip(("total", "norm", "coef"), g, t):
                same_bits(a, b, "%s of step %d (call %d)" % (name, step, call))
        if case.edge is None:
            assert (gfig[0][2].item() < 1.0) == (clip == C.CLIP_BINDS)
        for i, (p, q) in enumerate(zip(gp, tp)):
            assert p.is_cuda
            same_bits(p, q, "parameter %d (call %d)" % (i, call))
            if i == case.skipped:
                assert len(gopt.state.get(p, {})) == 0
                continue
            same_bits(gopt.state[p]["exp_avg"], topt.state[q]["exp_avg"], "exp_avg %d" % i)
            same_bits(gopt.state[p]["exp_avg_sq"], topt.state[q]["exp_avg_sq"], "exp_avg_sq %d" % i)
            assert float(gopt.state[p]["step"]) == 3
            if with_acc:
                same_bits(gacc[i], tacc[i], "accumulator %d" % i)
                assert not gacc[i].any()


def test_unaligned_tensors_take_the_same_values(hip_backend):
    """views that start 4 bytes into an allocation (the 4-byte path) get the bits of the aligned tensors"""
    from pseudocylindrical_convolution_amd import optim
    case = C.BY_NAME["sizes"]
    ref, _, _, rfig = C.native_steps(case, 1, True, C.CLIP_BINDS, DEV)
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    params = [off(p.to(DEV)).requires_grad_() for group in C.parameters(case) for p in group]
    assert all(p.data_ptr() % 16 == 4 for p in params)
    opt = optim.Adam(params)
    for p, g in zip(params, C.gradients(case, 0)):
        p.grad = off(g.to(DEV)) if p.numel() % 2 else g.to(DEV)      # aligned and unaligned pointers in one record too
    opt.step(acc=[off(a.to(DEV)) for a in C.accumulators(case, 0)], clip=C.CLIP_BINDS)
    same_bits(opt.last_total.cpu(), rfig[0][0], "total")
    for i, (p, q) in enumerate(zip(params, ref)):
        same_bits(p, q, "parameter %d" % i)


def test_with_no_clip_a_tensor_alone_gets_the_bits_it_gets_in_a_list(hip_backend):
    from pseudocylindrical_convolution_amd import optim
    case = C.BY_NAME["sizes"]
    together = C.native_steps(case, 1, True, 0.0, DEV)[0]
    for i in (0, 3, 7, 8):
        p = [p for group in C.parameters(case) for p in group][i].to(DEV).requires_grad_()
        p.grad = C.gradients(case, 0)[i].to(DEV)
        optim.Adam([p]).step(acc=[C.accumulators(case, 0)[i].to(DEV)], clip=0.0)
        same_bits(p, together[i], "parameter %d alone" % i)


def test_the_c_abi_refuses_before_a_byte_is_written(hip_backend):
    """a table that does not match nsegment (one segment FEWER than the counts give: were it launched all the same,
    it would stay inside every buffer), a negative count, null pointers: PCONV_EINVAL, and parameter, moments,
    accumulator and workspace keep every byte"""
    from pseudocylindrical_convolution_amd import _native
    import numpy as np
    lib = _native.hip_lib()
    n = 4097 + 7
    bufs = {k: torch.full((n,), 3.25, device=DEV) for k in ("p", "grad", "acc", "m", "v")}
    counts = np.array([4097, 7], dtype=np.int64)
    seg = P().optim_segments(counts, torch.device(DEV))
    assert seg.nsegment == 3 and seg.table.cpu().tolist() == [[0, 0], [0, 1], [1, 0]]
    scal = np.array([[1e-3, 1.0, 1e-8, 0.1, 0.999, 0.001]] * 2, dtype=np.float32).view(np.int64)
    ptrs = np.array([[bufs[k].data_ptr() + 4 * o for k in ("p", "grad", "acc", "m", "v")] + [c]
                     for o, c in ((0, 4097), (4097, 7))], dtype=np.int64)
    rec = torch.from_numpy(np.concatenate([ptrs, scal], axis=1)).to(DEV)
    ws = torch.full((4 + 3,), -7.0, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    bad_counts = np.array([4097, -7], dtype=np.int64)
    c, b = counts.ctypes.data, bad_counts.ctypes.data
    for args in ((rec.data_ptr(), seg.table.data_ptr(), c, 2, 2, ws.data_ptr()),
                 (rec.data_ptr(), seg.table.data_ptr(), b, 2, 3, ws.data_ptr()),
                 (None, seg.table.data_ptr(), c, 2, 3, ws.data_ptr()),
                 (rec.data_ptr(), None, c, 2, 3, ws.data_ptr()),
                 (rec.data_ptr(), seg.table.data_ptr(), None, 2, 3, ws.data_ptr()),
                 (rec.data_ptr(), seg.table.data_ptr(), c, 2, 3, None),
                 (rec.data_ptr(), seg.table.data_ptr(), c, -2, 3, ws.data_ptr())):
        assert lib.pconv_optim_sqnorm(*args[:5], ctypes.c_float(0.1), args[5], stream) == -1
        assert lib.pconv_optim_adam(*args, stream) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 3.25).all()) for t in bufs.values()) and bool((ws == -7.0).all())
    # ... and the same tables, given rightly, step
    assert lib.pconv_optim_sqnorm(rec.data_ptr(), seg.table.data_ptr(), c, 2, 3, ctypes.c_float(0.0), ws.data_ptr(), stream) == 0
    assert lib.pconv_optim_adam(rec.data_ptr(), seg.table.data_ptr(), c, 2, 3, ws.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert ws[0].item() == n * (3.25 + 3.25) ** 2 and not bufs["acc"].any() and bool((bufs["p"] != 3.25).all())


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


def _model_steps():
    """two optimiser steps of CMPNetV2M (16 channels, one frame of 256 x 512) on --loss ws under
    train.deterministic_mode() and --conv native, with optim.Adam fed through an AccGrad window of 2 and a clip"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, optim, train
    args = train.build_parser().parse_args(["--conv", "native", "--loss", "ws", "--base"])
    torch.manual_seed(0)
    net = Z.CMPNetV2M(8, 16, 16, 16, opt=False, init=False, device_id=0).to(DEV)
    net.train()
    params = [p for name, p in net.named_parameters() if name != "quant.count"]   # (the histogram has its own SGD)
    opt = optim.Adam(params, lr=1e-3)
    acc = Z.AccGrad(params)
    x = torch.rand(1, 3, 256, 512, generator=torch.Generator().manual_seed(3)).to(DEV)
    norms = []
    with contextlib.ExitStack() as stack:
        stack.enter_context(train.deterministic_mode())
        stack.enter_context(P().native_conv_grad(True))
        for it in range(4):
            mse, ssim, _ = train.forward_losses(args, net, x, None, None, None)
            opt.zero_grad()
            (mse + 0.1 * (1 - ssim)).backward()
            if it % 2 == 1:
                opt.step(acc=acc.acc_grad, clip=0.1)
                norms.append(opt.last_grad_norm)
            else:
                acc.acc(params)
        # the convolutions' packed weights follow the step (they are cached on the parameter's version, which a write
        # through a raw pointer does not bump by itself): a model made anew from these weights computes the same
        net.eval()
        fresh = Z.CMPNetV2M(8, 16, 16, 16, opt=False, init=False, device_id=0).to(DEV).eval()
        fresh.load_state_dict(net.state_dict())
        with torch.no_grad():
            assert torch.equal(net(x), fresh(x)), "the forward after a native step runs on stale packed weights"
    return params, opt, [n.item() for n in norms]


def test_a_model_trains_on_the_native_step_to_the_same_bits_twice_and_its_state_loads_into_torch_adam(hip_backend):
    params_a, opt_a, norms_a = _model_steps()
    params_b, opt_b, norms_b = _model_steps()
    assert norms_a == norms_b and all(n > 0 and n == n for n in norms_a)
    moved = 0
    for i, (a, b) in enumerate(zip(params_a, params_b)):
        same_bits(a, b, "parameter %d" % i)
        if a.grad is not None:
            same_bits(opt_a.state[a]["exp_avg_sq"], opt_b.state[b]["exp_avg_sq"], "exp_avg_sq %d" % i)
            assert float(opt_a.state[a]["step"]) == 2
            moved += 1
    assert moved > 10
    theirs = torch.optim.Adam(params_a, lr=1e-3)
    theirs.load_state_dict(opt_a.state_dict())
    before = [p.detach().clone() for p in params_a]
    theirs.step()                                            # torch's step runs on the loaded state
    assert all(float(s["step"]) == 3 for s in theirs.state.values())
    assert any(not torch.equal(p, q) for p, q in zip(params_a, before))
