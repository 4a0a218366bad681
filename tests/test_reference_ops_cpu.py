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
the checks.  EntropyConv2Op needs 128 cooperating threads and stays on the dense masked-convolution invariant
of tests/test_oracle_properties.py.
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
        case = C.CASES[name]
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


# -- fixtures: the same pin where the reference is absent ---------------------------------------------------------
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
