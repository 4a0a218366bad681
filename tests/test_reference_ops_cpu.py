"""The oracle (oracle/pconv_cpu.py over oracle/pconv_oracle.c) against the REFERENCE's own kernels, on the CPU.

Live tests: the reference's extension/*.cu compiled in place for the CPU (oracle/ref_ops.py; one thread walks
each kernel's grid-stride loop) run every case of tests/ref_ops_cases.py in two fresh child processes whose
allocator fills new memory differently -- what differs between the two was never written by the reference and is
masked; a mask may not touch a tile's valid interior.  They skip only where neither the reference tree nor a
built module exists.  Fixture tests: the same comparison against tests/golden/ref_ops_*.npz, anywhere.

Held bit for bit (torch.equal under the mask): all index work, every float op without transcendentals (both
sides are serial fp32 with contraction off), and -- with libm on both sides, set_detmath(False) -- the erf / exp
ops too.  With the product's published polynomials, set_detmath(True) (divergence 1), the
CDF tables stay within one count and the float results within bounds derived from the polynomials' published
accuracy (include/pconv_detmath.h: |erff - erf| < 1.2e-7 absolute, expf within 2 ulp); the derivations are at
the checks.

EntropyConv2Op, the masked 5x5 wavefront convolution, is blocks of 128 cooperating threads: its file alone runs on
the cooperative launcher of oracle/ref_shim/ (fibers, a real barrier, a real 32-lane shuffle), which is checked on
kernels of our own first.  The oracle in the reference's summation order (CONV_ORDER = 0) is held to it bit for
bit, every result of every econv case; the default order 1 (the product's, DESIGN.md section 2, divergence 2) under
the bound derived in ref_ops_cases.econv_bound.  Its four stored cases live in tests/golden/ref_ops_econv.npz.
"""
import os

import numpy as np
import pytest
import torch

import ref_ops_cases as C
from oracle import pconv_cpu as O
from oracle import ref_ops as ref_build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23          # spacing of float32 at 1.0
ERF_ABS = 1.2e-7          # include/pconv_detmath.h
EXP_ULPS = 2
DETMATH_OPS = ("gmm", "gmm_table", "gmm_table_batch", "quant")


@pytest.fixture(autouse=True)
def _libm_by_default():
    O.set_detmath(False)
    yield
    O.set_detmath(True)


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """the reference's results of every case and the masks of the elements it never writes"""
    if ref_build.ref_ops() is None:
        pytest.skip("neither the reference tree nor a built oracle/_ref module is here")
    return C.reference_results(tmp_path_factory.mktemp("ref_ops"))


@pytest.fixture(scope="module")
def stored():
    return C.load_fixtures(GOLDEN)


def assert_bit_equal(case, got, ref, masks):
    report = C.compare(case, got, ref, masks)
    assert not report, "%s: (result, worst |diff|, scale, elements) %s" % (case["name"], report)


def assert_within_one_ulp(case, got, ref, masks):
    """another libm than the one the fixtures were made with: equal values, or one unit in the last place"""
    for name in ref:
        a, b = got[name].double(), ref[name].double()
        if name in masks:
            keep = ~torch.as_tensor(masks[name])
            a, b = a[keep], b[keep]
        spacing = torch.from_numpy(np.spacing(np.maximum(a.abs().numpy(), b.abs().numpy()).astype(np.float32))).double()
        worst = ((a - b).abs() / spacing).max().item() if a.numel() else 0.0
        assert worst <= 1.0, "%s/%s: %.1f ulp" % (case["name"], name, worst)


# -- live: oracle against the reference's kernels -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_equals_reference(live, name):
    results, masks = live
    case = C.CASES[name]
    got = C.run(O, case, C.inputs(case))
    assert_bit_equal(case, got, results[name], masks[name])


def test_only_the_ring_of_a_padded_slice_is_unwritten(live):
    """what the two allocator fills showed: the reference leaves exactly the pad ring of SphereSliceOp's result
    unwritten, whole, and writes every other element of every result (dead columns included: zeros)"""
    results, masks = live
    for name, m in masks.items():
        case = C.ALL_CASES[name]
        if case["op"] == "slice" and case["pad"] > 0:
            assert list(m) == ["y"]
            ring = np.ones(m["y"].shape, bool)
            p = case["pad"]
            ring[:, :, p:-p, p:-p] = False
            assert np.array_equal(m["y"], ring)
            assert not (m["y"] & C.interior(case, "y", m["y"].shape)).any()
        else:
            assert not m, (name, list(m))


def test_tile_widths_of_the_host_geometry(live):
    """sphere_cal_npart_hw_v3 through the context ops: the widths both backends hand out are the plain formulas'
    (fixed widths above a weight total of 3 * npart, the cosine rule below), which the interior condition uses"""
    results, _ = live
    seen = set()
    for name, case in C.CASES.items():
        if case["op"] == "pad":
            assert results[name]["fill_param"].tolist() == C.widths(case), name
            seen.add(case["weight"])
    assert seen >= {"W16", "WCOS", "WFULL"}


def test_slice_parameters_reach_both_wrap_branches():
    """the cases hold source columns with pw == 0 and pw >= width - 2 (the modulo branch of the slice kernels) and
    columns strictly inside (the plain branch)"""
    for w, wt in ((72, C.W16), (40, C.WFULL)):
        for width in C.widths(dict(op="uslice", weight="W16" if wt is C.W16 else "WFULL", w=w, h=2)):
            pw = np.floor((np.arange(w) + 0.5) / w * width - 0.5 + 1e-9)
            pw = np.where(pw < 0, pw + width, pw).astype(int)
            assert (pw == 0).any() and (pw >= width - 2).any()
            assert ((pw > 0) & (pw < width - 2)).any() or width <= 3


def test_results_do_not_depend_on_allocation_history(live):
    """a second and third op object of one class built in one process (the reference reads members before it
    sets them; the binding constructs every object in zero-filled storage) give the child processes' results"""
    results, masks = live
    R = ref_build.ref_ops()
    for name in ("slice_h2_w72_p0", "uslice_h2_w72_p0", "slice_h1_w40_p2_n2", "slice_h2_w72_p0", "pad_h2_w72_p1_filled",
                 "quant_ntop2", "slice_h2_w72_p0_cosb"):
        case = C.CASES[name]
        junk = [torch.full((257, 33), float(k)) for k in range(3)]     # stir the allocator between objects
        del junk
        assert_bit_equal(case, C.run(R, case, C.inputs(case)), results[name], masks[name])


# -- the published polynomials against the reference's libm calls (documented divergence 1) --------------------
def check_detmath(case, got, ref):
    """the oracle with set_detmath(True) against the reference; returns {result: worst measured difference}"""
    op, worst = case["op"], {}
    if op in ("gmm_table", "gmm_table_batch"):
        diff = (got["table"] - ref["table"]).abs()
        worst["table_counts"] = diff.max().item()
        assert diff.max().item() <= 1.0                       # the bound of test_detmath_close_to_libm: one count
        ng = case["ng"]
        if op == "gmm_table":
            wa, wb = got["weight_after"], ref["weight_after"]
            assert torch.equal(got["delta_after"], ref["delta_after"])
        else:
            n = got["data_after"].shape[1]
            wa, wb = got["data_after"][0], ref["data_after"][0]
            assert torch.equal(got["data_after"][1:], ref["data_after"][1:])     # deltas (+ beta), means: no exp
        # softmax e_i / sum(e): each e_i within 2 ulp, the sum of ng of them within 2 ulp plus (ng - 1) roundings on
        # either side, the quotient's rounding on either side: (2 + 2 + (ng - 1) + 1) ulp, relative
        bound = (EXP_ULPS + EXP_ULPS + (ng - 1) + 1) * ULP
        rel = ((wa - wb).abs() / wb.abs().clamp_min(1e-30)).max().item()
        worst["softmax_relative"] = rel
        assert rel <= bound
    elif op == "gmm":
        bound = C.gmm_loss_bound(ref["loss"], ERF_ABS)          # derived there from the polynomial's accuracy
        diff = (got["loss"].double() - ref["loss"].double()).abs()
        worst["loss_abs"] = diff.max().item()
        worst["loss_over_bound"] = (diff / bound).max().item()
        assert (diff <= bound).all()
        # (the gradients divide differences of exponentials by p + 1e-7; they are held bit for bit under libm above)
    elif op == "quant":
        # the level table is exp(weight) within 2 ulp per level; a value is the input minus a chain of at most
        # `bins` subtractions of levels: at most bins * 2 ulp from the levels and one rounding per subtraction on
        # either side, all at the scale of the largest value
        scale = max(1.0, ref["val"].abs().max().item())
        bound = (case["bins"] * EXP_ULPS + 2 * case["bins"]) * 2.0 ** -24 * scale
        if "idx" in ref:
            assert torch.equal(got["idx"], ref["idx"])         # a flip needs an input within the bound of a boundary
        for k in ("val", "dq"):
            if k in ref:
                worst[k] = (got[k] - ref[k]).abs().max().item()
                assert worst[k] <= bound
        assert torch.equal(got["histogram"], ref["histogram"])
    return worst


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c["op"] in DETMATH_OPS and not c.get("train")])
def test_detmath_oracle_close_to_reference(live, name):
    results, _ = live
    case = C.CASES[name]
    O.set_detmath(True)
    got = C.run(O, case, C.inputs(case))
    print(name, check_detmath(case, got, results[name]))


# -- the masked convolution: the reference's 128-thread blocks on the cooperative launcher ------------------------
def test_cooperative_launcher_on_kernels_of_our_own():
    """oracle/ref_shim/coop_launch.cpp, before the reference's kernels are trusted to it (coop_selfcheck.cu)"""
    R = ref_build.ref_ops()
    if R is None:
        pytest.skip("neither the reference tree nor a built oracle/_ref module is here")
    # a neighbour exchange through shared memory: wrong wherever a reader runs before its writer (a barrier that
    # does nothing under serial execution); two blocks, three launches in a row, then a smaller and a larger block
    for n, blocks, launches in ((128, 2, 3), (64, 3, 1), (256, 1, 2)):
        got = np.array(R.coop_neighbour(n, blocks, launches), np.float32).reshape(launches, blocks, n)
        t = (np.arange(n) + 1) % n
        for l in range(launches):
            for b in range(blocks):
                assert np.array_equal(got[l, b], (100000 * l + 1000 * b + 3 * t + 1).astype(np.float32)), (n, l, b)
    # the 128 -> 1 tree of the reference's shape against the same order in plain loops, bit for bit; values of mixed
    # magnitude, so that another order of the additions gives other bits; four blocks, launched twice
    rng = np.random.default_rng(3)
    data = (rng.standard_normal(4 * 128) * 10.0 ** rng.integers(-3, 4, 4 * 128)).astype(np.float32)
    want, serial = [], []
    for blk in data.reshape(4, 128):
        s = blk.copy()
        for half in (64, 32, 16, 8, 4, 2, 1):
            s[:half] = s[:half] + s[half:2 * half]
        want.append(s[0])
        serial.append(np.add.accumulate(blk, dtype=np.float32)[-1])
    assert want != serial                                      # (the order does matter for these values)
    for _ in range(2):
        got = np.array(R.coop_tree(data.tolist()), np.float32)
        assert got.tobytes() == np.array(want, np.float32).tobytes()
    # shuffle-down at 16 .. 1 by the first warp alone, the other threads of the block gone: a lane whose source
    # lies in the warp takes the source's value of the stage before, every other lane keeps its own
    for n in (128, 32, 48):
        vals = rng.standard_normal(2 * n).astype(np.float32)
        got = np.array(R.coop_shuffle(vals.tolist(), n), np.float32).reshape(2, 5, n)
        for b in range(2):
            v = vals[b * n:(b + 1) * n].copy()
            for stage, off in enumerate((16, 8, 4, 2, 1)):
                nxt = v.copy()
                nxt[:32 - off] = v[off:32]
                v = nxt
                assert np.array_equal(got[b, stage], v), (n, b, off)


ECONV_RESULTS = ("step0", "third", "last", "past_the_end_unchanged", "restart_columns")


def with_conv_order(order, case, ins):
    assert O.CONV_ORDER == 1
    O.CONV_ORDER = order
    try:
        return C.run(O, case, ins)
    finally:
        O.CONV_ORDER = 1


def check_econv_reference(case, ref, masks):
    """what the reference's own results must look like for the other checks to mean something: nothing unwritten
    (step 0 zeroes the whole result), every written element non-zero -- so that "exactly zero" reads "not written"
    -- and after step 0, after a third of the steps and at the end exactly the valid positions whose diagonal has
    been reached written"""
    assert not masks, list(masks)
    assert list(ref) == list(ECONV_RESULTS)
    nsteps, third = C.econv_steps(case)
    shape = tuple(ref["last"].shape)
    valid, diagonal = C.interior(case, "last", shape), C.econv_diagonal(case, shape)
    assert 2 < third < diagonal[valid].max() < nsteps
    for key, reached in (("step0", 0), ("third", third), ("last", nsteps)):
        assert np.array_equal(ref[key].numpy() != 0, valid & (diagonal <= reached)), key
    assert int(ref["past_the_end_unchanged"]) == 1
    po = case["pad_out"]
    assert np.array_equal(ref["restart_columns"].numpy() != 0, (valid & (diagonal <= 2))[:, :, :, :po + 4])
    assert torch.equal(ref["restart_columns"], torch.where(torch.from_numpy(diagonal <= 2), ref["last"],
                                                           torch.zeros(()))[:, :, :, :po + 4])
    if "act" in case["entry"]:             # both branches of the activation
        assert (ref["last"] < 0).any() and (ref["last"] > 0).any()


@pytest.mark.parametrize("name", list(C.ECONV_CASES))
def test_econv_reference_writes_the_reached_diagonals(live, name):
    results, masks = live
    check_econv_reference(C.ECONV_CASES[name], results[name], masks[name])


@pytest.mark.parametrize("name", list(C.ECONV_CASES))
def test_econv_oracle_order0_equals_reference(live, name):
    """the oracle in the reference's summation order against the reference's kernels: every result, bit for bit"""
    results, masks = live
    case = C.ECONV_CASES[name]
    assert_bit_equal(case, with_conv_order(0, case, C.inputs(case)), results[name], masks[name])


@pytest.mark.parametrize("name", list(C.ECONV_CASES))
def test_econv_oracle_order1_within_bound(live, name):
    """the oracle's default order, the product's, against the reference (divergence 2)"""
    results, _ = live
    case = C.ECONV_CASES[name]
    ins = C.inputs(case)
    print(name, "worst difference / bound: %.3f" % C.econv_within_bound(case, ins, C.run(O, case, ins), results[name]))


# -- the mid-size cases: the same pin at widths past one and two trips of a 256-thread row loop, and at an odd width --
# The four mid masked convolutions (14 groups, 42 -> 42 channels, 308 steps of 128-fiber blocks on the cooperative
# launcher) are NOT run on the reference here: they take 14 s of CPU each and twice that for the two fills -- measured,
# with a pair of child processes per case side by side, this module took 43 s against 13 s without the mid cases,
# more than the factor of two it is allowed to grow by.  The masked convolution keeps its live pin on the ten small
# cases above (the production shape among them); the mid ones meet the oracle's order 1 on the GPU.
MID_PLAIN = [n for n, c in C.MID_CASES.items() if c["op"] != "econv"]


@pytest.fixture(scope="module")
def live_mid(tmp_path_factory):
    """the reference's results of the mid cases (two child processes of their own), and the unwritten-element masks"""
    if ref_build.ref_ops() is None:
        pytest.skip("neither the reference tree nor a built oracle/_ref module is here")
    return C.reference_results(tmp_path_factory.mktemp("ref_ops_mid"), MID_PLAIN)


@pytest.mark.parametrize("name", MID_PLAIN)
def test_oracle_equals_reference_on_the_mid_cases(live_mid, name):
    results, masks = live_mid
    case = C.MID_CASES[name]
    got = C.run(O, case, C.inputs(case))
    assert_bit_equal(case, got, results[name], masks[name])
    if case["op"] == "slice":          # as on the small cases: exactly the pad ring is unwritten
        ring = np.ones(masks[name]["y"].shape, bool)
        ring[:, :, case["pad"]:-case["pad"], case["pad"]:-case["pad"]] = False
        assert list(masks[name]) == ["y"] and np.array_equal(masks[name]["y"], ring)
    else:
        assert not masks[name], list(masks[name])
    if case["op"] == "pad":
        assert results[name]["fill_param"].tolist() == C.widths(case)


# -- fixtures: the same pin where the reference is absent ---------------------------------------------------------
@pytest.fixture(scope="module")
def stored_econv():
    return C.load_econv_fixtures(GOLDEN)


def test_econv_fixture_file_is_small_and_whole(stored_econv):
    assert C.ECONV_FIXTURE_FILE not in C.FIXTURE_FILES
    size = os.path.getsize(os.path.join(GOLDEN, C.ECONV_FIXTURE_FILE))
    assert size <= os.path.getsize(os.path.join(GOLDEN, "reference_graph.npz"))
    assert list(stored_econv) == list(C.ECONV_FIXTURE_CASES)
    cases = [C.ECONV_CASES[n] for n in C.ECONV_FIXTURE_CASES]
    for name, case in zip(C.ECONV_FIXTURE_CASES, cases):
        assert stored_econv[name][0] == case                   # the stored arguments are the case's
        for k, v in C.inputs(case).items():
            assert torch.equal(stored_econv[name][1][k], v), (name, k)
    assert {c["entry"] for c in cases} == {"forward", "forward_act", "forward_batch", "forward_act_batch"}
    assert {c["constrain"] for c in cases} == {5, 6} and {c["pad_out"] for c in cases} == {0, 2}
    assert any(c["weight"] == "WNOPT" for c in cases)
    assert {(c["n"], c["nset"]) for c in cases if "batch" in c["entry"]} == {(2, 2), (2, 1)}
    assert any(c["entry"] == "forward_act_batch" and c["nset"] == 2 for c in cases)      # slopes per weight set


@pytest.mark.parametrize("name", C.ECONV_FIXTURE_CASES)
def test_econv_fixture_reference_writes_the_reached_diagonals(stored_econv, name):
    case, ins, res, masks = stored_econv[name]
    check_econv_reference(case, res, masks)


@pytest.mark.parametrize("name", C.ECONV_FIXTURE_CASES)
def test_econv_fixture_oracle_order0_equals_reference(stored_econv, name):
    case, ins, res, masks = stored_econv[name]
    assert_bit_equal(case, with_conv_order(0, case, ins), res, masks)


@pytest.mark.parametrize("name", C.ECONV_FIXTURE_CASES)
def test_econv_fixture_oracle_order1_within_bound(stored_econv, name):
    case, ins, res, _ = stored_econv[name]
    print(name, "worst difference / bound: %.3f" % C.econv_within_bound(case, ins, C.run(O, case, ins), res))


def test_fixture_files_are_small_and_whole(stored):
    largest = os.path.getsize(os.path.join(GOLDEN, "reference_graph.npz"))
    total = 0
    for fname in C.FIXTURE_FILES:
        size = os.path.getsize(os.path.join(GOLDEN, fname))
        assert size <= largest, fname
        total += size
    assert total <= 1100000
    assert list(stored) == [n for f, ops in C.FIXTURE_FILES.items() for n in C.FIXTURE_CASES if C.CASES[n]["op"] in ops]
    families = {case["op"] for case, _, _, _ in stored.values()}
    assert families == {op for ops in C.FIXTURE_FILES.values() for op in ops}


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_fixture_masks_stay_outside_the_interior(stored, name):
    case, ins, res, masks = stored[name]
    assert case == C.CASES[name]                               # the stored arguments are the case's
    for k, m in masks.items():
        assert m.any() and not (m & C.interior(case, k, m.shape)).any()
        assert (res[k][torch.as_tensor(m)] == 0).all()         # masked elements are stored as zeros
    assert bool(masks) == (case["op"] == "slice" and case["pad"] > 0)


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_fixture_oracle_equals_reference(stored, name):
    case, ins, res, masks = stored[name]
    got = C.run(O, case, ins)
    if case["op"] in C.TRANSCENDENTAL and C.compare(case, got, res, masks):
        assert_within_one_ulp(case, got, res, masks)           # this host's libm is not the fixtures'
    else:
        assert_bit_equal(case, got, res, masks)


@pytest.mark.parametrize("name", [n for n in C.FIXTURE_CASES if C.CASES[n]["op"] in DETMATH_OPS and not C.CASES[n].get("train")])
def test_fixture_detmath_oracle_close_to_reference(stored, name):
    case, ins, res, _ = stored[name]
    O.set_detmath(True)
    check_detmath(case, C.run(O, case, ins), res)
