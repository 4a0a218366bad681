"""GPU: no result depends on what freshly allocated memory held (tests/stale_memory.py: the fills, the workspace table,
the UNWRITTEN regions; its teeth: tests/test_stale_memory_cpu.py).

Every item runs under fill A (NaN / 0) and fill B (0.747 / 1) of every torch.empty, empty_like and new_empty:
  (i)  the result passes the rule its family already has against its oracle or twin -- no tolerance here is a new
       number: each is the family's (ref_ops_cases.oracle_rule through check_against_oracle, same_bits, torch.equal, or
       the family's own test run as it stands under the fill);
  (ii) wherever the path is deterministic, the results under A, under B and unpatched are the same bits.
The float-atomic backward sums of the reference-pinned ops are held to (i) only.

FAMILIES lists what runs; test_no_case_and_no_family_drops_out holds the list and the 179 reference-pinned cases
complete."""
import contextlib
import importlib

import numpy as np
import pytest
import torch

import conv_backward_cases as CB
import masked_conv_cases as MC
import option_cases as OC
import ref_ops_cases as C
import stale_memory as SM
from oracle import pconv_cpu as O
from test_gpu_conv_backward import same_bits as conv_same_bits
from test_gpu_ref_cases_vs_oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EVERY = list(C.ALL_CASES) + list(C.MID_CASES)
WITH_BACKWARD = [n for n in EVERY if C.case_of(n)["op"] in C.BACKWARD_FAMILIES]
STEPPED = ("wave", "econv")
FILLS = list(SM.KINDS)


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)
    yield


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


def assert_same_bits(got, ref, what):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, tuple(got.shape))
    a, b = SM.bits(got), SM.bits(ref)
    if not torch.equal(a, b):
        bad = a != b
        raise AssertionError("%s: %d of %d elements differ in their bits, first at %s"
                             % (what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist())))


def under_each_regime(monkeypatch, compute):
    """{regime: compute()} for unpatched, fill A and fill B, and (ii): the same bits in all three.  compute returns
    an ordered dict name -> tensor (or None)"""
    runs = {}
    for regime, enter in SM.regimes(monkeypatch):
        with enter():
            runs[regime] = compute()
    plain = runs["plain"]
    for kind in FILLS:
        assert list(runs[kind]) == list(plain)
        for key, ref in plain.items():
            if ref is None:
                assert runs[kind][key] is None, (kind, key)
            else:
                assert_same_bits(runs[kind][key], ref, "%s under fill %s" % (key, kind))
    return runs


# ---- the reference-pinned ops --------------------------------------------------------------------------------------

def _key(args):
    return repr([a if isinstance(a, (int, float, bool, str)) else list(a) for a in args])


class Reusing(object):
    """a backend whose ops are built once: the first C.run records every op it constructs, a run after replay() gets
    the same objects back in the same order (C.run itself stays as it is)"""

    def __init__(self, backend):
        self._backend, self.ops, self._at, self._replay = backend, [], 0, False

    def replay(self):
        self._at, self._replay = 0, True

    def __getattr__(self, name):
        real = getattr(self._backend, name)
        if not (isinstance(real, type) and name.endswith("Op")):
            return real

        def make(*args):
            if not self._replay:
                self.ops.append((name, _key(args), real(*args)))
                return self.ops[-1][2]
            kept = self.ops[self._at]
            self._at += 1
            assert kept[:2] == (name, _key(args)), (kept[:2], name)
            return kept[2]
        return make


def restart_and_refill(backend, kind):
    """before the second use: a stepped op is restarted (its pass begins again at step 0, where it zeroes what it
    carries), the quantiser's training-iteration counter likewise begins again, and every tensor an op owns is filled"""
    n = 0
    for name, _, op in backend.ops:
        if hasattr(op, "restart"):
            op.restart()
        if hasattr(op, "iter_"):
            op.iter_ = 0
        if name.endswith("ContextOp") or kind is None or not hasattr(op, "_top"):
            continue      # the geometry caches: tables computed once per shape, inputs of the ops and not their results
        n += SM.refill(op, kind)
    return n


# families whose ops carry more than their result from pass to pass by design (DExtract2Op keeps its last count over a
# restart, as the reference's does): their second use is held to the ORACLE's second use of the same ops
CARRIES_STATE = ("wave",)
_oracle_again = {}


def oracle_second_use(name):
    """the oracle's results when its ops, built once, run the case a second time after restart(); computed once"""
    if name not in _oracle_again:
        case, ins, want = oracle(name)
        if case["op"] in CARRIES_STATE:
            backend = Reusing(O)
            C.run(backend, case, ins)
            restart_and_refill(backend, None)
            backend.replay()
            want = C.run(backend, case, ins)
        _oracle_again[name] = want
    return _oracle_again[name]


FORWARD_RESULTS = ("y", "loss")      # forward results that are held to a bound, not to equality (entropy pad, GMM loss)


def _deterministic(case, key, ordered):
    """every forward, everything under ordered_backward(True), every result held bit for bit; what is left are the
    float-atomic backward sums of the default backward"""
    return C.oracle_rule(case, key, ordered) == C.EQUAL or ordered or key in FORWARD_RESULTS


def _hold(case, got, want, ordered, what):
    bad = C.check_against_oracle(case, got, want, ordered=ordered)
    assert not bad, what + "\n" + "\n".join(bad)


def _ref_case(hip_backend, monkeypatch, name, kind, ordered):
    case, ins, want = oracle(name)
    mode = hip_backend.ordered_backward(True) if ordered else contextlib.nullcontext()
    with mode, SM.filled(monkeypatch, kind) as made:
        backend = Reusing(hip_backend)
        first = C.run(backend, case, ins, DEV, tables=False)
        _hold(case, first, want, ordered, "first use under fill %s" % kind)
        # (the in-place families, fill and mask, allocate nothing and own nothing)
        assert made or case["op"] in ("fill", "mask"), "no allocation went through the fill"
        # the second use of the same ops, every buffer they own filled
        assert restart_and_refill(backend, kind) > 0 or case["op"] in ("fill", "mask")
        backend.replay()
        second = C.run(backend, case, ins, DEV, tables=False)
        assert backend._at == len(backend.ops)
        again = oracle_second_use(name)
        _hold(case, second, again, ordered, "second use after refill(%s)" % kind)
    for key in first:
        if not torch.equal(again[key], want[key]):
            continue      # carried from pass to pass by design: held to the oracle's second use above
        # (ii) the deterministic results: bit for bit the same on the refilled buffers.  The float-atomic sums: (i) only.
        p = case["pad"] if (case["op"] == "slice" and key == "y") else 0      # UNWRITTEN: slice_pad_ring
        cut = (lambda t: t[:, :, p:-p, p:-p]) if p else (lambda t: t)
        if _deterministic(case, key, ordered):
            assert_same_bits(cut(second[key]), cut(first[key]), "%s/%s: second use" % (name, key))
    return first


def _ref_case_under_both_fills(hip_backend, monkeypatch, name, ordered):
    """the case under fill A and under fill B, each held to the oracle twice, then (ii): the deterministic results of
    the two fills bit for bit the same"""
    case = C.case_of(name)
    got = {kind: _ref_case(hip_backend, monkeypatch, name, kind, ordered) for kind in FILLS}
    for key in got["A"]:
        if _deterministic(case, key, ordered):
            p = case["pad"] if (case["op"] == "slice" and key == "y") else 0      # UNWRITTEN: slice_pad_ring
            cut = (lambda t: t[:, :, p:-p, p:-p]) if p else (lambda t: t)
            assert_same_bits(cut(got["A"][key]), cut(got["B"][key]), "%s/%s: fill A against fill B" % (name, key))


@pytest.mark.parametrize("name", EVERY)
def test_ref_ops_hold_the_oracle_whatever_fresh_memory_held(hip_backend, monkeypatch, name):
    _ref_case_under_both_fills(hip_backend, monkeypatch, name, False)


@pytest.mark.parametrize("name", WITH_BACKWARD)
def test_ref_ops_with_the_ordered_backward_whatever_fresh_memory_held(hip_backend, monkeypatch, name):
    _ref_case_under_both_fills(hip_backend, monkeypatch, name, True)
    assert hip_backend.backward_is_ordered() is False


# ---- the tile convolutions -----------------------------------------------------------------------------------------

# (id, mode of PCONV_CONV3X3, (tn, cin, h, w, cout), k, stride, the launches conv_plan gives).  The shapes are those of
# tests/option_cases.py, tests/test_gpu_wino.py and tests/test_gpu_wino42.py with FOUR tiles each (five in one row: the
# pattern wraps), so that every kernel meets a whole tile, a limit a little over half, a ragged one and a wholly dead tile
TILE_CONVS = [
    ("direct-3x3-s1", "direct", (4, 24, 8, 70, 64), 3, 1, ["direct"]),
    ("direct-3x3-s2", "direct", (4, 24, 15, 131, 64), 3, 2, ["direct"]),
    ("direct-1x1", "direct", (4, 20, 5, 70, 96), 1, 1, ["direct"]),
    ("small-12", "direct", (4, 24, 6, 70, 12), 3, 1, ["direct"]),
    ("small-3", "direct", (4, 24, 6, 70, 3), 3, 1, ["direct"]),
    ("wino", "wino", (4, 96, 6, 66, 96), 3, 1, ["wino"]),
    ("wino-flat", "wino", (5, 96, 4, 70, 96), 3, 1, ["wino_flat"]),
    ("wino42", "wino42", (4, 24, 10, 40, 64), 3, 1, ["wino42"]),
    ("wino42-row-split", "wino42", (4, 96, 14, 66, 64), 3, 1, ["wino42", "wino"]),
]


def _tile_conv_inputs(shape, k, stride, seed=71):
    tn, cin, h, w, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tn, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / np.sqrt(cin * k * k))
    b, sl = torch.randn(cout, generator=g), torch.rand(cout, generator=g)
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    res = torch.randn(tn, cout, ho, wo, generator=g)
    limit = torch.tensor(([wo, wo // 2 + 1, wo - 3, 0] * tn)[:tn], dtype=torch.int32)
    # every limit of the pattern is met: a whole tile, two that bind and a wholly dead tile
    assert tn >= 4 and sorted(set(limit.tolist())) == sorted({0, wo // 2 + 1, wo - 3, wo}) and 0 < wo // 2 + 1 < wo - 3 < wo
    return x, wt, b, sl, res, limit


@pytest.mark.parametrize("row", TILE_CONVS, ids=[r[0] for r in TILE_CONVS])
def test_tile_convolutions_write_all_they_own(hip_backend, monkeypatch, row):
    """plain; PReLU + residual + trim + column limits [wo, wo // 2 + 1, wo - 3, 0]; the same into ring buffers of 0 and
    2; the depth-to-width store: the same bits under either fill and unpatched, exact zeros from each tile's limit on,
    and the direct kernels' plain result the oracle's fmaf chain"""
    ident, mode, shape, k, stride, launches = row
    PC = P()
    monkeypatch.setenv("PCONV_CONV3X3", mode)
    tn, cin, h, w, cout = shape
    assert [l[0] for l in PC.conv_plan(cin, h, w, cout, k, stride)[0]] == launches
    x, wt, b, sl, res, limit = _tile_conv_inputs(shape, k, stride)
    assert bool((limit == 0).any()) and bool(((limit > 0) & (limit < res.shape[3])).any())
    xg, wg, bg, sg, rg, lg = (t.to(DEV) for t in (x, wt, b, sl, res, limit))
    d2w = cout % 4 == 0 and k == 3 and stride == 1

    def compute():
        owner = type("Owner", (), {})()      # (made here: the weights are packed anew, into filled memory, per regime)
        out = {"plain": PC.tile_conv2d(owner, xg, wg, bg, stride)}
        for ring in (0, 2):
            out["epilogue-ring%d" % ring] = PC.tile_conv2d(owner, xg, wg, bg, stride, sg, lg, tn, residual=rg, trim=True, ring=ring)
        out["limits-only"] = PC.tile_conv2d(owner, xg, wg, bg, stride, sg, lg, tn)
        if d2w:
            out["d2w"] = PC.tile_conv2d(owner, xg, wg, bg, stride, sg, None, 0, d2w=True)
        return out

    runs = under_each_regime(monkeypatch, compute)
    for regime, out in runs.items():
        for ring in (0, 2):
            y = out["epilogue-ring%d" % ring]
            assert bool(torch.isfinite(y).all()), (regime, ring)
            checked = 0
            for t in range(tn):
                beyond = y[t, :, :, int(limit[t]):]
                checked += beyond.numel()
                assert not bool((beyond != 0).any()), "%s: tile %d is not zero from its limit on" % (regime, t)
                if int(limit[t]) > 0:      # ... and live in front of it
                    assert bool((y[t, :, :, :int(limit[t])] != 0).any()), (regime, t)
            assert checked >= y[0].numel()      # (the dead tile alone is that many)
        if launches == ["direct"]:      # pconv_conv2d's sentence: 64-column tiles at or beyond the limit are zeros
            dead = [-(-int(v) // 64) * 64 for v in limit]      # (the Winograd builds' column tiles differ: trim alone
            for t in range(tn):                                 # promises zeros from the limit itself)
                assert not bool((out["limits-only"][t, :, :, dead[t]:] != 0).any()), (regime, t)
        if out["epilogue-ring2"]._pconv_ring[1] == 2:
            assert_same_bits(out["epilogue-ring2"].contiguous(), out["epilogue-ring0"], "%s: ring 2 against ring 0" % regime)
    if launches == ["direct"]:
        assert torch.equal(runs["A"]["plain"].cpu(), O.conv2d_chain(x, wt, b, stride, None))


@pytest.mark.parametrize("mode,cin,cout,k,h,launch", [("direct", 24, 64, 3, 2, "direct"), ("wino", 96, 96, 3, 2, "wino_flat"),
                                                      ("wino", 96, 96, 3, 4, "wino"), ("direct", 20, 96, 1, 2, "direct")])
def test_ring_buffer_is_whole_after_forward_ring(hip_backend, monkeypatch, mode, cin, cout, k, h, launch):
    """a convolution writes the interior of a ring-2 buffer (trim: zeros from each tile's width on), PseudoPadOp's
    forward_ring fills the ring: before it the ring may hold the fill (UNWRITTEN: ring_output_before_forward_ring),
    after it no element of the padded buffer does, and the buffer is the same bits under either fill and unpatched"""
    PC = P()
    monkeypatch.setenv("PCONV_CONV3X3", mode)
    assert "ring_output_before_forward_ring" in SM.UNWRITTEN
    w, store = 72, 2
    assert [l[0] for l in PC.conv_plan(cin, h + k - 1, w + k - 1, cout, k, 1)[0]] == [launch]
    geometry = dict(op="pad", weight="W16", w=w, h=h, pad=store)
    widths = C.widths(geometry)
    x, wt, b, sl, res, _ = _tile_conv_inputs((C.NPART, cin, h + k - 1, w + k - 1, cout), k, 1, seed=73)
    xg, wg, bg, sg, rg = (t.to(DEV) for t in (x, wt, b, sl, res))
    assert min(widths) < w // 2 and max(widths) == w      # polar tiles of a few columns: most of their row is dead
    lg = torch.tensor(widths, dtype=torch.int32, device=DEV)
    ctx = PC.PseudoContextOp(C.NPART, 20, C.WEIGHTS["W16"], 0, False)
    ctx.start_context(w)

    def compute():
        owner = type("Owner", (), {})()
        view = PC.tile_conv2d(owner, xg, wg, bg, 1, sg, lg, C.NPART, residual=rg, trim=True, ring=store)
        buf, ring = view._pconv_ring
        assert ring == store and tuple(buf.shape) == (C.NPART, cout, h + 2 * store, w + 2 * store)
        before.append(buf.clone())
        padded = PC.PseudoPadOp(store, C.NPART, ctx.addr(), 0, False).forward_ring(view)
        assert padded.data_ptr() == buf.data_ptr()
        return {"buffer": buf, "interior": view.contiguous()}

    before = []
    runs = under_each_regime(monkeypatch, compute)
    for kind, untouched in zip(FILLS, before[1:]):
        # the control: before forward_ring the ring does hold the fill (the region UNWRITTEN names; it also shows that the
        # fill reaches the device and that holds_pattern sees it there), the interior does not
        mask = torch.ones(untouched.shape[2:], dtype=torch.bool, device=DEV)
        mask[store:-store, store:-store] = False
        assert bool(SM.holds_pattern(untouched[:, :, mask], kind).all()), "fill %s: the fresh ring is not the fill" % kind
        assert not bool(SM.holds_pattern(untouched[:, :, ~mask], kind).any()), "fill %s is left in the interior" % kind
        assert not bool(SM.holds_pattern(runs[kind]["buffer"], kind).any()), "fill %s is left in the padded buffer" % kind
    # against the copying pad of the interior (the rule of test_ring_only_pad_equals_the_copying_pad: torch.equal)
    full = PC.PseudoPadOp(store, C.NPART, ctx.addr(), 0, False).forward(runs["plain"]["interior"])[0]
    assert torch.equal(runs["A"]["buffer"], full)


# ---- the fused GDN -------------------------------------------------------------------------------------------------

# one case per dispatch branch of pconv_gdn (the table in the header of tests/test_gpu_gdn.py): (shape index, setting)
# with and without a residual
GDN_BRANCHES = [(0, "resident"), (1, "resident"), (0, "default"), (6, "resident"), (0, "pipe"), (0, "batch"), (1, "default"),
                (3, "default"), (4, "default"), (5, "default")]


@pytest.mark.parametrize("si,setting", GDN_BRANCHES, ids=lambda v: str(v))
def test_gdn_branches_write_all_they_own(hip_backend, monkeypatch, si, setting):
    import test_gpu_gdn as G
    monkeypatch.setenv("PCONV_CONV3X3", "direct")
    c = G.case(si, "1")
    G.select(monkeypatch, setting)

    def compute():
        out, owner = {}, type("Owner", (), {})()      # (gamma is packed anew, into filled memory, per regime)
        for inverse, has_res, ring in ((False, False, 0), (False, True, 0), (True, True, 2), (False, False, 2)):
            res = c.gres if has_res else None
            out[(inverse, has_res, ring, None)] = P().tile_gdn(owner, c.gx, c.ggamma, c.gbeta, inverse, None, 0, res, ring)
            for li in range(len(c.glimits)):
                out[(inverse, has_res, ring, li)] = P().tile_gdn(owner, c.gx, c.ggamma, c.gbeta, inverse, c.glimits[li], 16, res, ring)
        return out

    # the limit sets of tests/test_gpu_gdn.py, the rotated ones included: with fewer than 16 tiles the head of the
    # unrotated pattern is all `w`.  Between them the sets hold a limit that binds and, where the pattern reaches this
    # width (w > 1), a dead tile
    tn, w = G.SHAPES[si][0], G.SHAPES[si][3]
    met = {int(v) for l in c.limits for v in l[:tn].tolist()}
    assert len(c.glimits) == len(G.ROLLS[tn]) and any(0 < v < w for v in met) and 0 in met, (met, w)

    runs = under_each_regime(monkeypatch, compute)
    for kind in FILLS:
        for (inverse, has_res, ring, li), y in runs[kind].items():
            G.same(y, c.ref(inverse, has_res, li), "%s %s fill %s inverse=%d residual=%d ring=%d limits=%s"
                   % (G._id(si), setting, kind, inverse, has_res, ring, li))
            if li is not None:
                for t in range(tn):
                    assert not bool((y[t, :, :, int(c.limits[li][t % 16]):] != 0).any()), (kind, li, t)


# ---- the convolution backward and the 5x5 masked convolutions ---------------------------------------------------------

NEEDS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)]


@pytest.mark.parametrize("name", ["a", "b", "c", "f", "i"])
def test_convolution_backward_writes_all_it_owns(hip_backend, monkeypatch, name):
    """every `need` combination (they change which part of the workspace exists: the prepared gradient, the partials,
    the fp64 planes alone), the workspace the wrapper allocates filled like every other allocation"""
    case = CB.BY_NAME[name]
    tin, tw, tb = CB.twin(case)
    x, weight, gout = (t.to(DEV) for t in CB.inputs(case))

    def compute():
        out = {}
        for need in NEEDS:
            for what, t in zip(("gin", "gw", "gb"), P().tile_conv2d_backward(x, weight.clone(), gout, case.s, need)):
                out["%s with need %s" % (what, need)] = t
        return out

    runs = under_each_regime(monkeypatch, compute)
    for kind in FILLS:
        for what, got in runs[kind].items():
            if got is not None:
                conv_same_bits(got, {"gin": tin, "gw ": tw, "gb ": tb}[what[:3].ljust(3)], "case %s %s, fill %s" % (name, what, kind))


def _into_a_callers_workspaces(family, case, x, weight, gout, twins, kind, same, what):
    """the native entries of `family` as a caller of the C interface drives them: workspaces of exactly the queried sizes
    and the gradient tensors all hold the fill when the call is made (no allocation of the wrapper's is involved)"""
    from pseudocylindrical_convolution_amd import _native
    PC = P()
    tin, tw, tb = twins
    lib, stream = _native.hip_lib(), PC._stream(x.device)
    tn, cin, h, w, cout, k, s = case.tn, case.cin, case.h, case.w, case.cout, case.k, case.s
    ks, kst = ((k,), (k, s)) if family.sized else ((), ())

    def filled(shape, dtype=torch.float32, workspace=None):
        return SM.fill_(torch.zeros(shape, dtype=dtype, device=DEV), kind, workspace)

    if case.need_x:
        packed = PC._pack_transposed(weight, family, stream)
        nbytes = getattr(lib, family.dgrad_workspace)(tn, cout, h, w, *kst)
        assert nbytes >= 0
        ws = filled((int(nbytes),), torch.uint8, "float") if nbytes else None
        gin = filled((tn, cin, h, w))
        PC.call(family.dgrad, PC._ptr(gout), PC._ptr(packed), PC._ptr(gin), PC._ptr(ws), tn, cin, h, w, cout, *kst + (stream,))
        same(gin, tin, "%s gin, caller's workspace, fill %s" % (what, kind))
    for need_w in (True, False):      # with the weight gradient, and the bias gradient alone on the fp64 planes alone
        nbytes = getattr(lib, family.wgrad_workspace)(tn, cin, cout, *ks) if need_w else tn * cout * 8
        assert nbytes > 0
        ws = filled((int(nbytes),), torch.uint8, "float")
        gw, gb = (filled((cout, cin, k, k)) if need_w else None), filled((cout,))
        PC.call(family.wgrad, PC._ptr(x) if need_w else None, PC._ptr(gout), PC._ptr(gw), PC._ptr(gb), PC._ptr(ws),
                tn, cin, h, w, cout, *kst + (stream,))
        if need_w:
            same(gw, tw, "%s gw, caller's workspace, fill %s" % (what, kind))
        same(gb, tb, "%s gb, caller's workspace, fill %s, weight gradient %s" % (what, kind, need_w))


@pytest.mark.parametrize("kind", FILLS)
@pytest.mark.parametrize("name", ["a", "b", "c", "f", "i"])
def test_convolution_backward_into_a_callers_filled_workspace(hip_backend, name, kind):
    case = CB.BY_NAME[name]
    x, weight, gout = (t.to(DEV) for t in CB.inputs(case))
    _into_a_callers_workspaces(P()._TILE_CONV, case, x, weight, gout, CB.twin(case), kind, conv_same_bits, "case " + name)


@pytest.mark.parametrize("kind", FILLS)
@pytest.mark.parametrize("case", MC.CASES[:2], ids=MC.IDS[:2])
def test_masked_convolution_backward_into_a_callers_filled_workspace(hip_backend, case, kind):
    assert (case.k, case.s) == (5, 1)
    x, weight, bias, gout = (t.to(DEV) for t in MC.inputs(case))
    _into_a_callers_workspaces(P()._CONV5, case, x, weight, gout, MC.twin(case)[1:], kind, MC.same_bits, "5x5 case " + case.name)


@pytest.mark.parametrize("case", MC.CASES[:2], ids=MC.IDS[:2])
def test_masked_convolutions_write_all_they_own(hip_backend, monkeypatch, case):
    ty, tin, tw, tb = MC.twin(case)
    x, weight, bias, gout = (t.to(DEV) for t in MC.inputs(case))

    def compute():
        out = {"y": P().conv5x5(type("Owner", (), {})(), x, weight, bias)}
        for need in NEEDS:
            if need[0] and not case.need_x:
                continue
            for what, t in zip(("gin", "gw", "gb"), P().conv5x5_backward(x, weight.clone(), gout, need)):
                out["%s with need %s" % (what, need)] = t
        return out

    runs = under_each_regime(monkeypatch, compute)
    for kind in FILLS:
        for what, got in runs[kind].items():
            if got is not None:
                ref = ty if what == "y" else {"gin": tin, "gw ": tw, "gb ": tb}[what[:3].ljust(3)]
                MC.same_bits(got, ref, "case %s %s, fill %s" % (case.name, what, kind))


# ---- the sphere metrics --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighting", ["ws", "uniform"])
@pytest.mark.parametrize("shape", [(1, 1, 16, 16), (2, 3, 17, 19), (1, 2, 33, 65)], ids=str)
def test_sphere_metrics_write_all_they_own(hip_backend, monkeypatch, shape, weighting):
    """ws_metrics f32 / u8 and backward, ws_msssim forward, its pyramid and backward with the `coarse` workspace: the
    smallest frames the entries accept, an odd side at every scale, a row and a column past a tile edge"""
    from test_gpu_ws_msssim import inputs
    PC = P()
    x, y = (t.to(DEV) for t in inputs(shape))
    n, c, h, w = shape
    g = torch.Generator().manual_seed(h + w)
    gout = torch.rand(n, 2, generator=g, dtype=torch.float64).to(DEV)
    u = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(DEV)
    v = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(DEV)

    def compute():
        out = {"ws_metrics": PC.ws_metrics_device(x, y, weighting), "ws_metrics_u8": PC.ws_metrics_device(u, v, weighting),
               "ws_metrics_backward": PC.ws_metrics_backward(x, y, gout, weighting)}
        values, workspace = PC.ws_msssim_device(x, y, weighting)
        out["ws_msssim"] = values
        for s, (lx, ly) in enumerate(PC.ws_msssim_levels(workspace, n, c, h, w), 1):
            out["x_%d" % s], out["y_%d" % s] = lx.clone(), ly.clone()
        out["ws_msssim_backward"] = PC.ws_msssim_backward(x, y, workspace, values, gout, weighting)
        out["ws_msssim_u8"] = PC.ws_msssim_device(u, v, weighting)[0]
        return out

    runs = under_each_regime(monkeypatch, compute)
    for kind in FILLS:
        out = runs[kind]
        for key, t in out.items():
            assert bool(torch.isfinite(t).all()), (kind, key)
        # the families' exact rules: WS-MSE of the multi-scale entry is ws_metrics' bits, the pyramid is the pool
        assert torch.equal(out["ws_msssim"][:, 5], out["ws_metrics"][:, 0])
        from pseudocylindrical_convolution_amd import sphere_metrics as S
        px, py = x, y
        for s in range(1, 5):
            px, py = S.pool(px), S.pool(py)
            assert torch.equal(out["x_%d" % s], px) and torch.equal(out["y_%d" % s], py), (kind, s)


# ---- every other family: its own test, as it stands, under either fill -----------------------------------------------

def _family(module, test, **picks):
    return (module, test, picks)


# (module, test, arguments): the smallest cases of each family's table; the test's own assertions are the rule (i).
# Index-producing kernels (the maps, the records, the reverse lists behind the ordered backward) have tests of their own
# in front of their consumers'.  Some of these tests reach a kernel through a cache of the package (a PointSet keeps its
# records): test_frame_side_kernels_give_the_same_bits_under_either_fill calls those entries directly, per regime.
FAMILIES = [
    _family("test_gpu_sphere_points", "test_records_equal_the_host", name="ico2"),
    _family("test_gpu_sphere_points", "test_records_equal_the_host", name="hand"),
    _family("test_gpu_sphere_points", "test_sample_equals_the_twin_bit_for_bit", h=8, w=16, interp="lanczos"),
    _family("test_gpu_sphere_points", "test_sample_equals_the_twin_bit_for_bit", h=8, w=16, interp="nearest"),
    _family("test_gpu_sphere_points", "test_mse_within_the_summation_bound_of_the_twin", name="ico2", interp="lanczos"),
    _family("test_gpu_sphere_points", "test_mse_within_the_summation_bound_of_the_twin", name="hand", interp="nearest"),
    _family("test_gpu_viewport", "test_map_kernel_is_the_float64_map", case=0),
    _family("test_gpu_viewport", "test_renderer_is_the_twin", case=0, n=1, c=1),
    _family("test_gpu_viewport", "test_renderer_is_the_twin", case=1, n=2, c=3),
    _family("test_gpu_viewport_backward", "test_kernel_is_the_twin", case=0, n=1, c=1),
    _family("test_gpu_viewport_backward", "test_kernel_is_the_twin", case=1, n=2, c=3),
    _family("test_gpu_erp_rotate", "test_map_kernel_is_the_float64_map", case=0),
    _family("test_gpu_erp_rotate", "test_sampler_is_the_twin", case=("SAMPLER_CASES", 0), clamp=False),
    _family("test_gpu_erp_rotate", "test_sampler_is_the_twin", case=("SAMPLER_CASES", 4), clamp=True),
    _family("test_gpu_erp_resample", "test_kernels_are_the_twin", case=0, clamp=False),
    _family("test_gpu_erp_resample", "test_kernels_are_the_twin", case=-2, clamp=True),
    _family("test_gpu_erp_resample_backward", "test_kernels_are_the_twin", case=0),
    _family("test_gpu_erp_resample_backward", "test_kernels_are_the_twin", case=1),
    _family("test_gpu_erp_resample_backward", "test_kernels_are_the_twin", case=3),
    _family("test_gpu_erp_size", "test_u8_to_f32_erp_kernel_is_the_rule", n=1, h=37, w=50),
    _family("test_gpu_erp_size", "test_erp_pad_f32_kernel_is_the_rule", n=1, h=37, w=50),
    _family("test_gpu_erp_size", "test_f32_to_u8_crop_kernel_is_tensor2img_of_the_crop", n=1, h=37, w=50),
    _family("test_gpu_yuv", "test_ingest_kernel_is_the_definition", case=0, fmt="yuv420p", n=1),
    _family("test_gpu_yuv", "test_ingest_kernel_is_the_definition", case=0, fmt="nv12", n=1),
    _family("test_gpu_yuv", "test_ingest_kernel_is_the_definition", case=0, fmt="yuv420p10le", n=1),
    _family("test_gpu_yuv", "test_egress_kernel_is_the_definition", case=0, fmt="yuv420p", n=1),
    _family("test_gpu_yuv", "test_egress_kernel_is_the_definition", case=0, fmt="nv12", n=1),
    _family("test_gpu_yuv", "test_egress_kernel_is_the_definition", case=0, fmt="yuv420p10le", n=1),
    _family("test_gpu_sphere_metrics", "test_kernel_is_the_float64_path", shape=0, weighting="ws"),
    _family("test_gpu_sphere_metrics", "test_uint8_form_is_bitwise_the_float_form", n=2, h=37, w=51),
    _family("test_gpu_sphere_loss", "test_kernel_is_the_float64_twin", case=0, weighting="ws"),
    _family("test_gpu_sphere_loss", "test_kernel_is_the_float64_twin", case=1, weighting="uniform"),
    _family("test_gpu_ws_msssim", "test_values_are_the_float64_twin", case=1, weighting="ws"),
    _family("test_gpu_ws_msssim", "test_uint8_form_is_bitwise_the_float_form", n=2, h=37, w=51),
    _family("test_gpu_ws_msssim_loss", "test_kernels_are_the_float64_twin", case=0, weighting="ws"),
    _family("test_gpu_ws_msssim_loss", "test_kernels_are_the_float64_twin", case=1, weighting="uniform"),
    _family("test_gpu_optim", "test_three_steps_are_the_twin_bit_for_bit_twice", case=0, with_acc=False, clip="binds"),
    _family("test_gpu_optim", "test_three_steps_are_the_twin_bit_for_bit_twice", case=1, with_acc=True, clip="loose"),
    _family("test_gpu_conv_backward", "test_a_gradient_that_is_not_asked_for_is_neither_computed_nor_returned"),
    _family("test_gpu_masked_conv", "test_a_gradient_that_is_not_asked_for_is_neither_computed_nor_returned"),
]
REQUIRED_MODULES = {"test_gpu_sphere_points", "test_gpu_viewport", "test_gpu_viewport_backward", "test_gpu_erp_rotate",
                    "test_gpu_erp_resample", "test_gpu_erp_resample_backward", "test_gpu_erp_size", "test_gpu_yuv",
                    "test_gpu_sphere_metrics", "test_gpu_sphere_loss", "test_gpu_ws_msssim", "test_gpu_ws_msssim_loss",
                    "test_gpu_optim", "test_gpu_conv_backward", "test_gpu_masked_conv"}


def _arguments(module, picks):
    """the picks as the test's arguments: `case` / `shape` by index into the module's table, the clip by name"""
    m = importlib.import_module(module)
    args = dict(picks)
    if isinstance(args.get("case"), tuple):
        args["case"] = getattr(m, args["case"][0])[args["case"][1]]
    elif isinstance(args.get("case"), int):
        args["case"] = (m.C.CASES if module == "test_gpu_optim" else m.CASES)[args["case"]]
    if isinstance(args.get("shape"), int):
        args["shape"] = m.SHAPES[args["shape"]]
    if module == "test_gpu_yuv":
        h, w, matrix, rng = args.pop("case")
        args.update(h=h, w=w, matrix=matrix, rng=rng)
    if "clip" in args:
        args["clip"] = {"binds": m.C.CLIP_BINDS, "loose": m.C.CLIP_LOOSE}[args["clip"]]
    return m, args


def _family_id(row):
    return "%s-%s-%s" % (row[0].replace("test_gpu_", ""), row[1].replace("test_", "")[:28],
                         "-".join(str(v) for v in row[2].values()))


@pytest.mark.parametrize("kind", FILLS)
@pytest.mark.parametrize("row", FAMILIES, ids=_family_id)
def test_family_holds_its_own_rule_whatever_fresh_memory_held(hip_backend, monkeypatch, row, kind):
    module, test, picks = row
    m, args = _arguments(module, picks)
    fn = getattr(m, test)
    names = fn.__code__.co_varnames[:fn.__code__.co_argcount]
    if "monkeypatch" in names:
        args["monkeypatch"] = monkeypatch
    with SM.filled(monkeypatch, kind) as made:
        fn(hip_backend, **args)
    assert made, "%s::%s allocated nothing through the fill" % (module, test)


def test_frame_side_kernels_give_the_same_bits_under_either_fill(hip_backend, monkeypatch):
    """(ii) for the frame-side kernels, on the smallest cases: the maps and records (indices: held on their own first),
    then their consumers -- the point sampler and its mse, the renderer and its ordered backward, the rotation's sampler;
    the resize and its backward; u8 <-> f32, the ERP pad and crop, the YUV ingest and egress"""
    import test_gpu_yuv as Y
    import viewport_backward_cases as VB
    import erp_resample_backward_cases as RB
    import sphere_points_cases as K
    from viewport_cases import CASES as VIEWS
    from pseudocylindrical_convolution_amd import sphere_points as SP
    PC = P()

    from pseudocylindrical_convolution_amd import erp_rotate, viewport
    points = torch.tensor(K.pointset("ico2").points).to(DEV)      # (the PointSet caches its records: the entry itself)
    view_case = VIEWS[1]                                          # odd width, every footprint at a pole, ragged tile
    h, w, vh, vw, ss, angles = view_case
    rot = erp_rotate.units(30, 20, 10)

    def indices():
        return {"viewport_map": PC.viewport_map(h, w, vh * ss, vw * ss, viewport.view(*angles)),
                "rotation_map": PC.erp_rotation_map(50, 100, rot, False),
                "records": PC.sphere_points_records(points, 8, 16)}

    maps = under_each_regime(monkeypatch, indices)
    for kind in FILLS:      # each index producer against its CPU twin, before any consumer runs on its output
        rec, q = maps[kind]["records"], maps[kind]["viewport_map"]
        assert torch.equal(rec.cpu(), torch.from_numpy(SP.records_numpy(K.pointset("ico2"), 8, 16)))
        assert torch.equal(q.cpu(), torch.from_numpy(viewport.source_map_numpy(h, w, vh * ss, vw * ss, viewport.view(*angles))))
        assert torch.equal(maps[kind]["rotation_map"].cpu(), torch.from_numpy(erp_rotate.source_map_numpy(50, 100, rot, False)))
    rec, q = maps["A"]["records"], maps["A"]["viewport_map"]
    frames_v = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(9)).to(DEV)
    x = K.picture(2, 3, 8, 16).to(DEV)
    y = K.picture(2, 3, 8, 16, seed=1).to(DEV)
    case = RB.SMALL[0]
    frames, grad = RB.frames(case).to(DEV), RB.gradient(case).to(DEV)
    u = torch.randint(0, 256, (1, 8, 16, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    odd = torch.randint(0, 256, (1, 37, 50, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    rot_map = maps["A"]["rotation_map"]
    turned = torch.rand(2, 3, 50, 100, generator=torch.Generator().manual_seed(6)).to(DEV)
    lists = tuple(t.to(DEV) for t in viewport.reverse_lists(q, h, w))      # (host code: the transpose of the map)
    view_grad = VB.gradient(2, 3, vh, vw).to(DEV)
    yuv_in = {fmt: Y.source(1, 4, 6, fmt).to(DEV) for fmt in Y.FORMATS}
    yuv_out = Y.reconstruction(1, 4, 6).to(DEV)

    def consumers():
        out = {}
        for interp in K.INTERPS:
            out["sample-" + interp] = PC.sphere_points_sample_f32(x, rec, interp)
            out["mse-" + interp] = PC.sphere_points_mse_device(x, rec, y, rec, interp)
        for clamp in (False, True):
            out["render-%d" % clamp] = PC.viewport_render_f32(frames_v, q, vh, vw, ss, clamp)
            out["rotate-%d" % clamp] = PC.erp_remap_f32(turned, rot_map, clamp)
        out["render-backward"] = PC.remap_backward_f32(view_grad, q, lists, h, w, vh, vw, ss)
        padded = PC.frames_u8_to_f32_erp(odd)
        out["erp-pad"], out["erp-crop"] = padded, PC.frames_f32_to_u8_crop(padded, 37, 50)
        for fmt in Y.FORMATS:
            out["yuv-in-" + fmt] = PC.frames_yuv420_to_f32(yuv_in[fmt], 4, 6, fmt)
            out["yuv-out-" + fmt] = PC.frames_f32_to_yuv420(yuv_out, 4, 6, fmt)
        out["resize"] = PC.erp_resample_f32(frames, case[4], case[5])
        out["resize-clamped"] = PC.erp_resample_f32(frames, case[4], case[5], clamp=True)
        out["resize-backward"] = PC.erp_resample_backward_f32(grad, case[2], case[3])
        f = PC.frames_u8_to_f32(u)
        out["u8-to-f32"], out["f32-to-u8"] = f, PC.frames_f32_to_u8(f)
        return out

    runs = under_each_regime(monkeypatch, consumers)
    assert torch.equal(runs["A"]["f32-to-u8"], u) and torch.equal(runs["A"]["erp-crop"], odd)


def test_optimiser_step_gives_the_same_bits_under_either_fill(hip_backend, monkeypatch):
    """optim.sqnorm's partials and the native Adam step (the workspace of PCONV.optim_step)"""
    import optim_cases as OP
    case = OP.CASES[0]

    def compute():
        got = OP.native_steps(case, 2, False, OP.CLIP_BINDS, DEV)
        flat = got if isinstance(got, (list, tuple)) else [got]
        out, k = {}, 0
        stack = list(flat)
        while stack:
            t = stack.pop(0)
            if isinstance(t, torch.Tensor):
                out["t%d" % k] = t.detach().clone()
                k += 1
            elif isinstance(t, (list, tuple)):
                stack = list(t) + stack
            elif isinstance(t, dict):
                stack = list(t.values()) + stack
        assert out
        return out

    under_each_regime(monkeypatch, compute)


# ---- the entropy engine --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", ["packed", "int32"])
@pytest.mark.parametrize("n", [1, 3])
def test_engine_results_do_not_depend_on_fresh_memory(hip_backend, monkeypatch, n, rows):
    """PCONV_ENGINE_ALLOC_FILL=0xFF / 0x3F (every device and pinned-host buffer of a group overwritten right after it is
    allocated; ctx / act[] then zeroed by clear() as always): the default engine's bytes, its streams decoded to the
    coded symbols, rate() equal to the default's as bits -- for one frame and for three (two lock-step groups), and again
    on a second call with other symbols, the stale-but-finite regime clear() documents"""
    import test_gpu_option_paths as T
    T._clean(monkeypatch)
    monkeypatch.delenv("PCONV_ENGINE_ALLOC_FILL", raising=False)
    ent = T._net(56)
    h, w = OC.EE_SHAPE
    batches = [T._batch(ent, n, h, w, seed) for seed in (51, 53)]
    plain = T._engine(ent, h, w, n)
    assert plain.option("PCONV_ENGINE_ALLOC_FILL") == -1
    want = []
    for sym in batches:
        streams = plain.encode(sym)
        bits, pos = plain.rate(sym, rate_map=True)
        want.append((streams, bits.clone(), pos.clone()))
        assert torch.equal(plain.decode(streams), sym)
    assert want[0][0] != want[1][0]
    assert OC.ALLOC_FILL == ("0xFF", "0x3F") and [int(v, 0) for v in OC.ALLOC_FILL] == [SM.FLOAT_BYTE[k] for k in FILLS]
    for value, kind in zip(OC.ALLOC_FILL, FILLS):
        monkeypatch.setenv("PCONV_ENGINE_ALLOC_FILL", value)
        monkeypatch.setenv("PCONV_ENGINE_ROWS", rows)      # int32: labels_d / labels_h exist, and are filled, only there
        with SM.filled(monkeypatch, kind):
            filled_enc, filled_dec = T._engine(ent, h, w, n), T._engine(ent, h, w, n)
            monkeypatch.delenv("PCONV_ENGINE_ALLOC_FILL")
            monkeypatch.delenv("PCONV_ENGINE_ROWS")
            assert filled_enc.option("PCONV_ENGINE_ROWS") == (rows == "int32")
            assert filled_enc.option("PCONV_ENGINE_ALLOC_FILL") == int(value, 0) == filled_dec.option("PCONV_ENGINE_ALLOC_FILL")
            for call, (sym, (streams, bits, pos)) in enumerate(zip(batches, want)):
                what = "fill %s, call %d" % (value, call)
                got_bits, got_pos = filled_enc.rate(sym, rate_map=True)      # first: nothing of this call exists yet
                assert_same_bits(got_bits, bits, what + ": rate")
                assert_same_bits(got_pos, pos, what + ": rate map")
                assert_same_bits(filled_enc.rate(sym), bits, what + ": rate alone")
                assert filled_enc.encode(sym) == streams, what
                assert torch.equal(filled_dec.decode(streams), sym), what      # a decoder that never encoded
                assert torch.equal(filled_enc.decode(streams), sym), what


# ---- the whole model -----------------------------------------------------------------------------------------------

def test_codec_round_trip_does_not_depend_on_fresh_memory(hip_backend, monkeypatch):
    """encode -> decode of one 256 x 512 frame through pseudo_codec / engine.py: the same stream bytes and the same
    reconstruction bits under either fill and unpatched (codec, engines and every buffer made under the regime)"""
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    from test_gpu_engine import _codec, _frames
    x = _frames(1, 256, 512)
    streams = {}

    def compute():
        enc, dec = _codec()
        eng = CodecEngine(56, 0, enc, dec)
        got = eng.encode(x)
        streams[len(streams)] = got
        return {"reconstruction": eng.decode(got, 256, 512), "symbols": eng.symbols(x)}

    runs = under_each_regime(monkeypatch, compute)
    assert len(streams) == 3 and streams[0] == streams[1] == streams[2] and len(streams[0][0]) > 0
    assert bool(torch.isfinite(runs["plain"]["reconstruction"]).all())


def test_training_steps_do_not_depend_on_fresh_memory(hip_backend, monkeypatch):
    """the two-step recipe of tests/test_gpu_erp_resample_backward.py (--deterministic --conv native-all --optim native
    --loss ws, CMPNetV2M at 16 channels): every parameter the same bits under either fill and unpatched, all finite"""
    from test_gpu_erp_resample_backward import _model_steps
    runs = under_each_regime(monkeypatch, lambda: {"p%03d" % k: p for k, p in enumerate(_model_steps(monkeypatch))})
    assert len(runs["plain"]) > 10
    for regime, params in runs.items():
        assert all(bool(torch.isfinite(p).all()) for p in params.values()), regime


# ---- nothing drops out ---------------------------------------------------------------------------------------------

def _params(test, name):
    for mark in test.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == name:
            return list(mark.args[1])
    raise KeyError(name)


def test_no_case_and_no_family_drops_out():
    every = set(C.ALL_CASES) | set(C.MID_CASES)
    assert len(C.ALL_CASES) == 99 and len(C.MID_CASES) == 80 and len(every) == 179
    for test, cases in ((test_ref_ops_hold_the_oracle_whatever_fresh_memory_held, every),
                        (test_ref_ops_with_the_ordered_backward_whatever_fresh_memory_held,
                         {n for n in every if C.case_of(n)["op"] in ("slice", "uslice", "projects", "quant")})):
        names = _params(test, "name")
        assert len(names) == len(set(names)) and set(names) == cases and all(isinstance(n, str) for n in names)
    assert FILLS == ["A", "B"]      # (both inside each of these tests: _ref_case_under_both_fills)
    assert {C.case_of(n)["op"] for n in every if C.case_of(n)["op"] in STEPPED} == set(STEPPED)
    assert _params(test_family_holds_its_own_rule_whatever_fresh_memory_held, "kind") == ["A", "B"]
    rows = _params(test_family_holds_its_own_rule_whatever_fresh_memory_held, "row")
    assert rows == FAMILIES and {r[0] for r in rows} == REQUIRED_MODULES
    assert all(not hasattr(r, "marks") for r in rows)                      # no mark on any row: nothing skips
    kernels = {k for row in _params(test_tile_convolutions_write_all_they_own, "row") for k in row[5]}
    assert kernels == {"direct", "wino", "wino_flat", "wino42"}
    assert len({(si, s) for si, s in GDN_BRANCHES}) == len(GDN_BRANCHES) == 10
    assert _params(test_convolution_backward_writes_all_it_owns, "name") == ["a", "b", "c", "f", "i"]
    assert _params(test_engine_results_do_not_depend_on_fresh_memory, "n") == [1, 3]
    assert _params(test_engine_results_do_not_depend_on_fresh_memory, "rows") == ["packed", "int32"]
    assert _params(test_convolution_backward_into_a_callers_filled_workspace, "name") == ["a", "b", "c", "f", "i"]
    assert _params(test_convolution_backward_into_a_callers_filled_workspace, "kind") == FILLS
    assert _params(test_masked_convolution_backward_into_a_callers_filled_workspace, "case") == MC.CASES[:2]
    assert _params(test_masked_convolution_backward_into_a_callers_filled_workspace, "kind") == FILLS
    assert all(row[2][0] >= 4 for row in _params(test_tile_convolutions_write_all_they_own, "row"))      # a dead tile each
    import sys
    me = sys.modules[__name__]
    for name in ("test_ring_buffer_is_whole_after_forward_ring", "test_gdn_branches_write_all_they_own",
                 "test_masked_convolutions_write_all_they_own", "test_sphere_metrics_write_all_they_own",
                 "test_frame_side_kernels_give_the_same_bits_under_either_fill",
                 "test_optimiser_step_gives_the_same_bits_under_either_fill",
                 "test_codec_round_trip_does_not_depend_on_fresh_memory", "test_training_steps_do_not_depend_on_fresh_memory"):
        test = getattr(me, name)
        assert callable(test) and not any(m.name in ("skip", "skipif", "xfail") for m in getattr(test, "pytestmark", []))
