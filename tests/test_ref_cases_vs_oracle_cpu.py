"""CPU: the rule that holds the HIP ops to the oracle on every case of tests/ref_ops_cases.py
(ref_ops_cases.check_against_oracle, used on the GPU by tests/test_gpu_ref_cases_vs_oracle.py) has teeth, and the
mid-size cases reach what they were added for.

Teeth: the oracle's own results pass; a copy of them with one planted fault does not --
  (a) the last valid column of the narrowest tile of a bit-exact tile stack moved by one unit in the last place,
  (b) a non-zero in the first dead column of slice `y` / the quantiser's `g_in`,
  (c) first and last valid column of a wrapping (full-width) tile swapped in a `gx` held to 1e-5,
  (d) one element of the masked convolution on the last reached diagonal moved by one unit in the last place,
  (e) under ordered=True, one element of a backward result moved by one unit in the last place (which the default
      bound, 1e-5 / 1e-4 of scale, lets through).
Which faults a case can carry follows from its family and widths alone, and is asserted."""
import numpy as np
import pytest
import torch

import ref_ops_cases as C
from oracle import pconv_cpu as O

EVERY = list(C.ALL_CASES) + list(C.MID_CASES)
_results = {}


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)      # what the GPU module compares against
    yield


def oracle_results(name):
    if name not in _results:
        assert O.CONV_ORDER == 1
        case = C.case_of(name)
        _results[name] = C.run(O, case, C.inputs(case))
    return _results[name]


def copy(res):
    return type(res)((k, v.clone()) for k, v in res.items())


def ulp_up(t, index):
    assert t.dtype == torch.float32
    t[index] = torch.nextafter(t[index], torch.tensor(float("inf")))


def last_valid(case, key, shape, tile):
    """(tile, 0, first valid row, last valid column) of a tile stack"""
    keep = C.interior(case, key, shape)[tile, 0]
    rows, cols = np.nonzero(keep.any(1))[0], np.nonzero(keep.any(0))[0]
    return (tile, 0, int(rows[0]), int(cols[-1])), int(cols[0])


def planted_faults(case, want):
    """[(kind, result, ordered, faulty copy of `want`)]"""
    op, out = case["op"], []
    stacks = C.TILE_STACKS.get(op, {})
    wd = C.widths(case) if "weight" in case else None
    for key in stacks:
        if key not in want:
            continue
        narrow = min((t for t in range(C.NPART) if wd[t] > 0), key=lambda t: wd[t])
        for ordered in (False, True):
            if C.oracle_rule(case, key, ordered) == C.EQUAL and not (ordered and C.oracle_rule(case, key) == C.EQUAL):
                bad = copy(want)
                ulp_up(bad[key], last_valid(case, key, tuple(want[key].shape), narrow)[0])
                out.append(("a", key, ordered, bad))
    dead_key = {"slice": "y", "quant": "g_in"}.get(op)
    if dead_key and min(wd) < case["w"]:
        tile = min(range(C.NPART), key=lambda t: wd[t])
        index, _ = last_valid(case, dead_key, tuple(want[dead_key].shape), tile)
        bad = copy(want)
        assert bad[dead_key][index[:3] + (index[3] + 1,)] == 0
        bad[dead_key][index[:3] + (index[3] + 1,)] = 1e-30
        out.append(("b", dead_key, False, bad))
    if op in ("slice", "uslice", "pad", "epad"):
        assert C.oracle_rule(case, "gx") == ("scale", 1e-5)
        tile = C.NPART // 2                                   # an equator tile: as wide as the frame, it wraps
        assert wd[tile] == max(wd) and (wd[tile] == case["w"] or case["weight"] == "WEDGE")
        bad = copy(want)
        g = bad["gx"]
        if op == "slice":                                     # the ERP image: the tile's rows, its whole width
            rows = slice(tile * case["h"], (tile + 1) * case["h"])
            reached = g[:, :, rows].abs().sum((0, 1, 2)).nonzero().flatten()     # (WEDGE: tiles of 3 columns reach few)
            first, last = int(reached[0]), int(reached[-1])
            assert (first, last) == (0, case["w"] - 1) or case["weight"] == "WEDGE"
            a, b = g[:, :, rows, first].clone(), g[:, :, rows, last].clone()
            g[:, :, rows, first], g[:, :, rows, last] = b, a
        else:
            (_, _, _, last), first = last_valid(case, "gx", tuple(g.shape), tile)
            a, b = g[tile, :, :, first].clone(), g[tile, :, :, last].clone()
            g[tile, :, :, first], g[tile, :, :, last] = b, a
        assert not torch.equal(g, want["gx"])
        out.append(("c", "gx", False, bad))
    if op == "econv":
        shape = tuple(want["last"].shape)
        diagonal = np.where(C.interior(case, "last", shape), C.econv_diagonal(case, shape), -1)
        index = tuple(int(i) for i in np.argwhere(diagonal == diagonal.max())[-1])
        assert want["last"][index] != 0
        bad = copy(want)
        ulp_up(bad["last"], index)
        out.append(("d", "last", False, bad))
    for key in ("gx", "count", "g_in", "g_weight"):
        if op in C.BACKWARD_FAMILIES and key in want and C.oracle_rule(case, key, True) == C.EQUAL != C.oracle_rule(case, key):
            bad = copy(want)
            index = tuple(int(i) for i in np.unravel_index(int(want[key].abs().argmax()), tuple(want[key].shape)))
            ulp_up(bad[key], index)
            out.append(("e", key, True, bad))
    return out


def expected_kinds(case):
    """from the family and the widths alone"""
    op = case["op"]
    kinds = set()
    if op in ("slice", "pad", "fill", "quant", "wave", "econv", "uslice"):
        kinds.add("a")               # (uslice: its tile stack `gx` is bit-exact under ordered=True)
    if op in ("slice", "quant") and min(C.widths(case)) < case["w"]:
        kinds.add("b")
    if op in ("slice", "uslice", "pad", "epad"):
        kinds.add("c")
    if op == "econv":
        kinds.add("d")
    if op in ("slice", "uslice", "projects"):
        kinds.add("e")
    return kinds


@pytest.mark.parametrize("name", EVERY)
def test_the_oracle_passes_and_every_planted_fault_is_reported(name):
    case, want = C.case_of(name), oracle_results(name)
    for ordered in (False, True):
        assert C.check_against_oracle(case, copy(want), want, ordered=ordered) == []
    faults = planted_faults(case, want)
    assert {kind for kind, _, _, _ in faults} == expected_kinds(case)
    for kind, key, ordered, bad in faults:
        report = C.check_against_oracle(case, bad, want, ordered=ordered)
        assert len(report) >= 1 and all("/" + key + ":" in line for line in report), (kind, key, ordered, report)
        if kind == "e":              # ... which the default bound lets through: the flag is what catches it
            assert C.check_against_oracle(case, bad, want, ordered=False) == []


def test_a_missing_or_misshapen_result_is_reported():
    case, want = C.case_of("quant_ntop2"), oracle_results("quant_ntop2")
    short = copy(want)
    del short["dq"]
    assert C.check_against_oracle(case, short, want)
    bad = copy(want)
    bad["val"] = bad["val"][:, :, :, :-1]
    assert C.check_against_oracle(case, bad, want)
    nan = copy(want)
    nan["g_weight"][0, 0] = float("nan")
    assert C.check_against_oracle(case, nan, want)


TRAIN_QUANT = [n for n in EVERY if C.case_of(n)["op"] == "quant" and C.case_of(n)["train"]]


@pytest.mark.parametrize("name", TRAIN_QUANT)
def test_the_merge_bound_of_a_training_mode_quantiser(name):
    """the one derived bound (ref_ops_cases.quant_merge_bound): zero wherever the merge leaves a weight alone, a
    few float32 spacings of the weights where it does not, met by the product's own formulation of the step on another
    libm (torch's CPU exp / log), and with teeth of its own"""
    import types
    from pseudocylindrical_convolution_amd import PCONV
    case, want = C.case_of(name), oracle_results(name)
    ins = C.inputs(case)
    bound = C.quant_merge_bound(case, ins)
    moved = want["weight_after"] != ins["weight"]
    assert bool(moved.any()) and bool((bound[moved] > 0).all()) and bool((bound[~moved] == 0).all())
    # a handful of float32 spacings of the weights themselves (|w| in 2 .. 8: 2.4e-7 .. 4.8e-7), no more
    assert 0 < bound.max().item() <= 6 * float(np.spacing(np.float32(want["weight_after"].abs().max().item())))
    # the product's update_weight is plain torch: on the CPU it is the same step on a second libm
    w, cnt = ins["weight"].clone(), ins["count"].clone()
    stub = types.SimpleNamespace(iter_=1, mod_=1, bin_num_=case["bins"], weight_decay_=0.9)
    PCONV.PseudoQuantOp.update_weight(stub, w, cnt)
    assert bool(((w.double() - want["weight_after"].double()).abs() <= bound).all())
    assert torch.equal(cnt, want["count_after"])
    # teeth: twice the bound on a merged weight, one unit in the last place on an untouched one
    index = tuple(int(i) for i in np.unravel_index(int(bound.argmax()), tuple(bound.shape)))
    bad = copy(want)
    bad["weight_after"][index] += 2 * bound[index].float() + float(np.spacing(np.float32(abs(float(want["weight_after"][index])))))
    report = C.check_against_oracle(case, bad, want)
    assert any("/weight_after:" in line for line in report)
    still = tuple(int(i) for i in (~moved).nonzero()[0])
    bad = copy(want)
    ulp_up(bad["weight_after"], still)
    assert any("/weight_after:" in line for line in C.check_against_oracle(case, bad, want))


def test_the_table_results_of_the_oracle_are_not_asked_of_the_product():
    case, want = C.case_of("pad_h2_w72_p1_filled"), oracle_results("pad_h2_w72_p1_filled")
    assert any(k.startswith("table_") for k in want)
    got = type(want)((k, v.clone()) for k, v in want.items() if not k.startswith("table_"))
    assert C.check_against_oracle(case, got, want) == []


# -- the mid cases reach what they are for (from widths(case) alone) -------------------------------------------
def test_mid_cases_are_the_asked_for_grid():
    assert len(C.MID_CASES) == 80 and not set(C.MID_CASES) & set(C.ALL_CASES)
    for wt in ("WNOPT", "WFULL", "WCOS", "WCOSB"):
        for w in (264, 520, 131):
            ops = sorted(c["op"] for c in C.MID_CASES.values() if c["weight"] == wt and c["w"] == w)
            want = ["epad", "fill", "pad", "quant", "slice", "uslice"] + (["econv", "wave"] if w == 264 else [])
            assert ops == sorted(want), (wt, w, ops)
    for name in C.FIXTURE_CASES + C.ECONV_FIXTURE_CASES:
        assert name in C.ALL_CASES


@pytest.mark.parametrize("name", list(C.MID_CASES))
def test_mid_case_reaches_what_it_is_for(name):
    case = C.MID_CASES[name]
    wd, w = C.widths(case), case["w"]
    assert len(wd) == C.NPART and max(wd) == w and min(wd) > 0
    if case["weight"] == "WFULL":
        assert wd == [w] * C.NPART                 # every tile wraps
    else:
        # tiles whose valid width ends inside a 4-column quad: at least half of them in every case
        assert sum(1 for v in wd if v % 4) >= 8, wd
        assert min(wd) < w // 2
    if w == 520:                                   # a row loop of 256 threads takes a second / third trip, ragged
        assert any(v > 256 and v % 256 for v in wd)
        assert any(v > 512 and v % 256 for v in wd)
    if w == 264:
        assert any(v > 256 and v % 256 for v in wd)
    if w == 131:                                   # odd rows: no tile row but the first is 16-byte aligned
        assert w % 2 == 1 and (w + 2 * case.get("pad", 0)) % 2 == 1
