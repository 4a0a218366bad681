"""GPU: the HIP ops against the oracle on EVERY case of tests/ref_ops_cases.py -- the 99 small cases (of which
tests/test_gpu_reference_golden.py meets the stored third) and the 80 mid-size ones (MID_CASES: the weight sets other
than W16 at 264, 520 and 131 columns).  The oracle is held to the reference's own kernels on all of them, live, by
tests/test_reference_ops_cpu.py; how each result is held to the oracle is said in one place,
ref_ops_cases.check_against_oracle (its teeth: tests/test_ref_cases_vs_oracle_cpu.py).

Then the same cases under PCONV.ordered_backward(True) for the families with a backward, and the product-only paths
that replace these ops in the models, on the same geometries: the ring-only pad (PseudoPadOp.forward_ring) and the
quantiser's and dequantiser's 16-byte forms (the codec's call: eval mode under no_grad)."""
import pytest
import torch

import ref_ops_cases as C
from oracle import pconv_cpu as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
EVERY = list(C.ALL_CASES) + list(C.MID_CASES)
WITH_BACKWARD = [n for n in EVERY if C.case_of(n)["op"] in C.BACKWARD_FAMILIES]
PAD_CASES = [n for n in EVERY if C.case_of(n)["op"] == "pad" and C.case_of(n)["pad"] > 0]
QUANT_EVAL_CASES = [n for n in EVERY if C.case_of(n)["op"] == "quant" and not C.case_of(n)["train"]]
_oracle = {}


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)      # the product's published polynomials, whatever an earlier module left
    yield


def oracle(name):
    """(case, inputs, the oracle's results): computed once per case, shared, left unchanged (run() clones)"""
    if name not in _oracle:
        assert O.CONV_ORDER == 1
        case = C.case_of(name)
        ins = C.inputs(case)
        _oracle[name] = (case, ins, C.run(O, case, ins))
    return _oracle[name]


@pytest.mark.parametrize("name", EVERY)
def test_hip_ops_hold_the_oracles_results(hip_backend, name):
    case, ins, want = oracle(name)
    got = C.run(hip_backend, case, ins, DEV, tables=False)
    bad = C.check_against_oracle(case, got, want)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", WITH_BACKWARD)
def test_hip_ops_hold_the_oracles_results_with_the_ordered_backward(hip_backend, name):
    case, ins, want = oracle(name)
    with hip_backend.ordered_backward(True):
        got = C.run(hip_backend, case, ins, DEV, tables=False)
    assert hip_backend.backward_is_ordered() is False
    bad = C.check_against_oracle(case, got, want, ordered=True)
    assert not bad, "\n".join(bad)


def _params(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    return list(mark.args[1])


def test_no_case_drops_out():
    every = set(C.ALL_CASES) | set(C.MID_CASES)
    assert len(C.ALL_CASES) == 99 and len(C.MID_CASES) == 80 and len(every) == 179
    names = _params(test_hip_ops_hold_the_oracles_results)
    assert len(names) == len(set(names)) and set(names) == every
    ordered = _params(test_hip_ops_hold_the_oracles_results_with_the_ordered_backward)
    assert set(ordered) == {n for n in every if C.case_of(n)["op"] in ("slice", "uslice", "projects", "quant")}
    assert set(_params(test_ring_only_pad_equals_the_copying_pad)) == \
        {n for n in every if C.case_of(n)["op"] == "pad" and C.case_of(n)["pad"] > 0}
    assert set(_params(test_quantiser_sixteen_byte_forms)) == \
        {n for n in every if C.case_of(n)["op"] == "quant" and not C.case_of(n)["train"]}
    for n in every:       # no mark on any case: nothing skips, nothing is expected to fail
        assert isinstance(n, str)


@pytest.mark.parametrize("name", PAD_CASES)
def test_ring_only_pad_equals_the_copying_pad(hip_backend, name):
    """PseudoPadOp.forward_ring on a view inside a NaN-filled buffer of store 2 (what the models run after a
    convolution that wrote into a ring buffer) against the copying pad of the same values, bit for bit -- and so
    against the oracle; where pad < store a wider pad has used the buffer before.  The dead
    columns are zeroed first in every case, as the recipe of tests/test_gpu_ops.py does and the network's producers
    do: interior columns past the wrap are the producer's by the ring kernel's contract (csrc/tilepad.hip)."""
    P = hip_backend
    case, ins, want = oracle(name)
    p, store = case["pad"], 2
    ctx = P.PseudoContextOp(C.NPART, 20, C.WEIGHTS[case["weight"]], 0, False)
    ctx.start_context(case["w"])
    xg = P.PseudoFillOp(0, C.NPART, 0, 0, ctx.addr(), 0, 0, False).forward(ins["x"].clone().to(DEV))[0]
    full = P.PseudoPadOp(p, C.NPART, ctx.addr(), 0, False).forward(xg)[0].clone()
    tn, c, h, w = xg.shape
    buf = torch.full((tn, c, h + 2 * store, w + 2 * store), NAN, device=DEV)
    view = buf[:, :, store:-store, store:-store]
    view.copy_(xg)
    view._pconv_ring = (buf, store)
    if p < store:      # a wider pad used the buffer before: its wrap columns must not survive
        P.PseudoPadOp(store, C.NPART, ctx.addr(), 0, False).forward_ring(view)
    ring = P.PseudoPadOp(p, C.NPART, ctx.addr(), 0, False).forward_ring(view)
    assert ring.data_ptr() != full.data_ptr() and tuple(ring.shape) == tuple(full.shape)
    assert ring.data_ptr() == buf[:, :, store - p:, store - p:].data_ptr()      # in place: no copy was taken
    assert torch.equal(ring, full), "%d elements differ" % int((ring != full).sum())
    # (the copying pad reads no dead column and writes zeros past the wrap: the oracle's result of a `dirty` case too)
    assert torch.equal(ring.cpu(), want["y"])


def _unaligned(t):
    """the same values at an address that is no multiple of 16: the host must take the scalar form"""
    flat = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("name", QUANT_EVAL_CASES)
def test_quantiser_sixteen_byte_forms(hip_backend, name):
    """PseudoQuantOp.forward / PseudoDQuantOp.forward as the codec calls them, eval mode under no_grad
    (quant8x4_kernel / dquant8x4_kernel where the host takes them: rows of a multiple of 4 columns; at 131 columns
    it has to take the scalar kernels): values, indices and dequantised values bit-equal to the scalar form's and to
    the oracle's, dead columns zero -- with tile widths that end inside a quad"""
    P = hip_backend
    case, ins, want = oracle(name)
    ctx = P.PseudoContextOp(C.NPART, 20, C.WEIGHTS[case["weight"]], 0, False)
    ctx.start_context(case["w"])
    x, weight, count = (ins[k].clone().to(DEV) for k in ("x", "weight", "count"))
    op = P.PseudoQuantOp(case["c"], case["bins"], C.NPART, 0.9, 1, case["ntop"], 0.1, ctx.addr(), 0, False)
    dq = P.PseudoDQuantOp(C.NPART, case["c"], case["bins"], ctx.addr(), 0, False)
    # the scalar forms: gradients enabled (the histogram's reader may exist) / an input that is not 16-byte aligned
    val_s = op.forward(x, weight, count, False)[0].clone()
    idx_s = op._top[1].clone()
    assert float(op.count_data_.sum()) < 0.0
    dq_s = dq.forward(_unaligned(idx_s), weight)[0].clone()
    with torch.no_grad():
        val_q = op.forward(x, weight, count, False)[0].clone()
        idx_q = op._top[1].clone()
        assert float(op.count_data_.abs().sum()) == 0.0       # no histogram: the call the 16-byte form is for
        dq_q = dq.forward(idx_q.contiguous(), weight)[0].clone()
    for key, quad, scalar in (("val", val_q, val_s), ("idx", idx_q, idx_s), ("dq", dq_q, dq_s)):
        assert torch.equal(quad, scalar), "%s: %d elements differ from the scalar form" % (key, int((quad != scalar).sum()))
        if key in want:      # (ntop 1: the oracle hands out the values alone)
            assert torch.equal(quad.cpu(), want[key]), "%s: %d elements differ from the oracle" % (key, int((quad.cpu() != want[key]).sum()))
        dead = C.dead_columns(case, key, quad)
        assert not bool((quad.cpu()[dead] != 0).any()), key
    assert torch.equal(val_q.cpu(), want["val"])
    assert torch.equal(weight.cpu(), ins["weight"]) and torch.equal(count.cpu(), ins["count"])     # eval: left alone
