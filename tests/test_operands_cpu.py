"""CPU: the operand table of tests/operand_cases.py is complete, its deformations are what they claim, and its harness
has teeth -- run on fake wrappers that check nothing, check too late or write outside a view, it says so.  The sweep
itself needs the GPU: tests/test_gpu_operands.py."""
import collections
import types

import pytest
import torch

import operand_cases as OC


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


# ---- completeness ------------------------------------------------------------------------------------------------------

def test_every_public_entry_and_every_tensor_operand_is_in_the_table():
    bad = OC.incomplete(P())
    assert not bad, "\n".join(bad)
    assert len({OC.row_id(r) for r in OC.ROWS}) == len(OC.ROWS)
    assert OC.NOT_SWEPT == {}      # every public entry that turns a tensor into an address has a row


def test_the_gaps_this_sweep_was_written_for_are_rows():
    entries = {r.entry: r for r in OC.ROWS if not r.route}
    routes = {r.route for r in OC.ROWS if r.entry == "tile_conv2d"}
    assert routes == {"direct", "1x1", "wino", "wino_flat", "wino42", "direct-ring2"}
    for entry, operands in [("tile_gdn", {"gamma", "beta", "col_limit"}), ("PseudoQuantOp.forward", {"weight"}),
                            ("PseudoDQuantOp.forward", {"weight"}), ("PseudoQuantOp.backward", {"grads[0]", "grads[1]", "out"}),
                            ("EntropyConv2Op.forward", {"weight", "bias"}), ("EntropyConv2Op.forward_act_batch", {"act"}),
                            ("EntropyAddOp.forward", {"y"}), ("EntropyGmmOp.forward", {"delta", "mean", "label"}),
                            ("EntropyGmmTableOp.forward", {"delta", "mean", "tnum"})]:
        assert operands <= {o.name for o in entries[entry].operands}, entry
    for r in OC.ROWS:
        if r.entry == "tile_conv2d":
            assert {"weight", "bias", "slope", "col_limit"} <= {o.name for o in r.operands}


def test_a_missing_row_a_missing_operand_and_a_row_for_nothing_are_noticed():
    PC = P()
    without = [r for r in OC.ROWS if r.entry != "EntropyAddOp.forward"]
    assert any("EntropyAddOp.forward: a public entry point with no row" in b for b in OC.incomplete(PC, rows=without))
    at = [i for i, r in enumerate(OC.ROWS) if r.entry == "EntropyGmmOp.forward"][0]
    fewer = list(OC.ROWS)
    fewer[at] = fewer[at]._replace(operands=tuple(o for o in fewer[at].operands if o.name != "label"))
    assert any("label holds a tensor and is no named operand" in b for b in OC.incomplete(PC, rows=fewer))
    ghost = list(OC.ROWS) + [OC.ROWS[0]._replace(entry="NoSuchOp.forward")]
    assert any("NoSuchOp.forward: listed, but" in b for b in OC.incomplete(PC, rows=ghost))
    assert any("no_such_function" in b for b in OC.incomplete(PC, not_swept=dict(OC.NOT_SWEPT, no_such_function="?")))
    unreasoned = list(OC.ROWS)
    o = unreasoned[at].operands[1]
    unreasoned[at] = unreasoned[at]._replace(operands=(unreasoned[at].operands[0], o._replace(short=None)) + unreasoned[at].operands[2:])
    assert any("short has neither a form nor a reason" in b for b in OC.incomplete(PC, rows=unreasoned))


def test_nothing_drops_out():
    run, na = OC.cases()
    assert len(run) == 847 and len(na) == 93 and len(OC.ROWS) == 77 and len({r.entry for r in OC.ROWS}) == 71
    assert all(not hasattr(c, "marks") for c in run)
    assert [sum(1 for c in run if c[2] == d) for d in OC.DEFORMATIONS] == [185, 185, 185, 185, 107]
    assert collections.Counter(c[3] for c in na) == {OC.DEFINES_SHAPE: 80, OC.NOT_A_TENSOR: 11, OC.ONE_ELEMENT: 2}
    # the in-place ops and the ring outputs are held to "nothing outside the view"
    inplace = {r.entry for r in OC.ROWS if r.inplace}
    assert {"PseudoFillOp.forward", "EntropyAddOp.forward", "MaskConstrainOp.forward", "leaky_clip_"} <= inplace
    assert {"direct-ring2"} <= {r.route for r in OC.ROWS if r.entry == "tile_conv2d"}
    assert {"ring2"} <= {r.route for r in OC.ROWS if r.entry == "tile_gdn"}
    assert {"optim_step", "PseudoPadOp.forward_ring", "packed_conv_weight"} <= {r.entry for r in OC.ROWS}


def test_what_does_not_apply_names_one_of_the_three_reasons():
    run, na = OC.cases()
    assert len(run) > 300 and na
    ids = [OC.case_id(c) for c in run]
    assert len(set(ids)) == len(ids)
    for r, o, d, reason in na:
        assert reason in OC.REASONS, (OC.row_id(r), o.name, d)
        if reason == OC.DEFINES_SHAPE:
            assert d == "short"
        if reason == OC.ONE_ELEMENT:
            assert d == "strided" and OC.get(r.make(P(), "cpu").args, o.name).numel() == 1


# ---- the deformations ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,dtype", [((5,), torch.float32), ((3, 1), torch.float32), ((4, 6), torch.int32),
                                         ((2, 3, 4, 5), torch.float32), ((2, 4, 6, 3), torch.uint8)], ids=str)
def test_the_deformations_are_what_they_claim(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    t = (torch.arange(n) % 200).to(dtype).view(shape)
    forms = OC.strided_forms(t)
    assert forms[0][0] == "wide" and ([f[0] for f in forms] == ["wide", "transposed"]) == (len(shape) >= 2 and min(shape[-2:]) > 1)
    for form, view, buf in forms:
        assert not view.is_contiguous() and tuple(view.shape) == shape and view.dtype == dtype and torch.equal(view, t)
        assert OC.dense_read_covered(view)
    wide, buf = forms[0][1:]
    assert wide.stride(-1) == 2 and buf.shape[-1] == 2 * shape[-1] and bool((buf[..., 1::2] == OC._sentinel(dtype)).all())
    view, buf = OC.offset_form(t)
    assert view.is_contiguous() and torch.equal(view, t) and view.storage_offset() == 1 and buf.numel() == n + 1
    assert view.data_ptr() % view.element_size() == 0 and OC.dense_read_covered(view)
    if view.element_size() == 4:
        assert view.data_ptr() % 8 == 4 and view.data_ptr() % 16 in (4, 12)
    assert buf[0] == OC._sentinel(dtype)
    other = OC.other_dtype(t)
    assert other.dtype != dtype and tuple(other.shape) == shape and other.element_size() != t.element_size()
    assert OC.other_device(t, "meta").device != t.device and tuple(OC.other_device(t, "meta").shape) == shape
    short = OC.shorter(t)
    assert tuple(short.shape) == (shape[0] - 1,) + shape[1:] and short.is_contiguous() and short.dtype == dtype
    assert short.untyped_storage().nbytes() < n * t.element_size()      # read as `shape`, it would be read past its end
    count = torch.tensor([7], dtype=torch.int32)
    assert int(OC.one_more(count)[0]) == 8 and int(count[0]) == 7


def test_bits_tell_minus_zero_and_nan_payloads_apart():
    a = torch.tensor([0.0, float("nan")])
    b = torch.tensor([-0.0, float("nan")])
    assert not torch.equal(OC.bits(a), OC.bits(b)) and OC.bits(a).dtype == torch.int32
    payload = OC.bits(a).clone()
    payload[1] += 1
    assert bool(torch.isnan(payload.view(torch.float32)[1])) and not torch.equal(payload, OC.bits(a))


# ---- the harness on fake wrappers --------------------------------------------------------------------------------------------

class FakeError(RuntimeError):
    pass


def fake_module():
    m = types.SimpleNamespace(PconvError=FakeError, launched=[])
    m.call = lambda fn, *args: m.launched.append(fn)
    m._backward_call = m.call
    m._native = types.SimpleNamespace(call=m.call)

    def checked(x, bias, what):
        for name, t, shape in (("x", x, tuple(x.shape)), ("bias", bias, (x.shape[0],))):
            if t.dtype != torch.float32 or t.device != x.device or tuple(t.shape) != shape or not t.is_contiguous():
                raise FakeError("%s: %s must be contiguous float32 %s on x's device" % (what, name, shape))

    def good(x, bias):
        checked(x, bias, "good")
        m.call("kernel", x.data_ptr(), bias.data_ptr())
        return x + bias[:, None]

    def checks_nothing(x, bias):
        m.call("kernel", x.data_ptr(), bias.data_ptr())
        return x + bias[:, None].to(x.dtype)

    def checks_late(x, bias):
        m._native.call("pack_weight", x.data_ptr())      # a weight packed, a workspace filled ... before the last check
        checked(x, bias, "checks_late")
        m.call("kernel", x.data_ptr(), bias.data_ptr())
        return x + bias[:, None]

    def good_(x, bias):
        checked(x, bias, "good_")
        m.call("kernel", x.data_ptr(), bias.data_ptr())
        x += bias[:, None]

    def writes_outside_(x, bias):
        checked(x, bias, "writes_outside_")
        m.call("kernel", x.data_ptr(), bias.data_ptr())
        x += bias[:, None]
        if x.storage_offset():      # one element in front of the view
            torch.as_strided(x, (1,), (1,), x.storage_offset() - 1).zero_()

    def other_kernel(x, bias):
        checked(x, bias, "other_kernel")
        m.call("kernel" if x.data_ptr() % 8 == 0 else "scalar_kernel", x.data_ptr(), bias.data_ptr())
        return x + bias[:, None]

    m.good, m.checks_nothing, m.checks_late, m.good_, m.writes_outside_ = good, checks_nothing, checks_late, good_, writes_outside_
    m.other_kernel = other_kernel
    return m


def fake_row(name, inplace):
    def make(PC, dev):
        g = torch.Generator().manual_seed(1)
        args = OC.A(dev, x=torch.randn(4, 6, generator=g), bias=torch.randn(4, generator=g))

        def run(a):
            res = getattr(PC, name)(a["x"], a["bias"])
            return OC.R(y=a["x"] if inplace else res)
        return OC.Case(args, run, None)
    return OC.Row(name, "", name, make, (OC.X(), OC.opd("bias")), ("x",) if inplace else (), {})


def _verdicts(name, inplace=False):
    m, out = fake_module(), collections.OrderedDict()
    run, _ = OC.cases([fake_row(name, inplace)])
    for c in run:
        with pytest.MonkeyPatch.context() as patch:
            try:
                OC.check(m, c[0], c[1], c[2], "cpu", "meta", patch)
                out[OC.case_id(c)] = "ok"
            except OC.Reached as e:
                out[OC.case_id(c)] = "reached: %s" % e
            except AssertionError as e:
                out[OC.case_id(c)] = "failed: %s" % e
    return out


def test_a_wrapper_that_checks_every_operand_first_passes():
    for name, inplace in (("good", False), ("good_", True)):
        verdicts = _verdicts(name, inplace)
        assert len(verdicts) == 9 and set(verdicts.values()) == {"ok"}, verdicts


def test_a_wrapper_that_checks_nothing_is_reported():
    verdicts = _verdicts("checks_nothing")
    for d in ("dtype", "device", "short"):
        v = verdicts["checks_nothing-bias-" + d]
        assert v.startswith("reached: reached the library with a refused operand: checks_nothing, bias, " + d), v
    assert verdicts["checks_nothing-x-dtype"].startswith("reached: ") and verdicts["checks_nothing-x-device"].startswith("reached: ")
    assert "ran, the table says refused" in verdicts["checks_nothing-x-strided"]
    assert "ran, the table says refused" in verdicts["checks_nothing-bias-strided"]
    assert verdicts["checks_nothing-x-offset"] == "ok" == verdicts["checks_nothing-bias-offset"]


def test_a_wrapper_that_checks_after_its_first_call_is_reported():
    verdicts = _verdicts("checks_late")
    for case, v in verdicts.items():
        if case.split("-")[-1] in ("dtype", "device", "short"):
            assert v.startswith("reached: ") and "(pack_weight)" in v, (case, v)
        else:
            assert v == "ok", (case, v)


def test_a_wrapper_that_writes_outside_a_view_is_reported():
    verdicts = _verdicts("writes_outside_", True)
    assert "wrote outside the view (1 gap elements changed)" in verdicts["writes_outside_-x-offset"]
    assert all(v == "ok" for case, v in verdicts.items() if case != "writes_outside_-x-offset"), verdicts


def test_a_wrapper_that_takes_another_entry_point_for_an_honoured_operand_is_reported():
    verdicts = _verdicts("other_kernel")
    assert "the library calls ['scalar_kernel'], with a dense operand ['kernel']" in verdicts["other_kernel-x-offset"]
    assert all(v == "ok" for case, v in verdicts.items() if case != "other_kernel-x-offset"), verdicts


def test_a_refusal_that_does_not_name_the_operand_is_reported():
    m = fake_module()
    r = fake_row("good", False)

    def vague(x, bias):
        if bias.dtype != torch.float32:
            raise FakeError("good: only float32 is supported")
        return m.good(x, bias)
    m.good_named = m.good
    m.good = vague
    with pytest.MonkeyPatch.context() as patch, pytest.raises(AssertionError, match="does not name the operand bias"):
        OC.check(m, r, r.operands[1], "dtype", "cpu", "meta", patch)
