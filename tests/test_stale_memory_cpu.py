"""CPU: the fill harness of tests/stale_memory.py has teeth, and the references the GPU module compares against do not
themselves depend on fresh memory.

  - the patterns are what the module's table says, read back as integers;
  - the patch reaches torch.empty, torch.empty_like and Tensor.new_empty, leaves torch.zeros alone and is gone after
    the block;
  - every comparator tests/test_gpu_stale_memory.py uses reports ONE output element that holds pattern A, and one that
    holds pattern B;
  - a B-valued element in a dead column of slice `y` is reported;
  - the oracle and the CPU twins give the same bits under fill A, fill B and unpatched."""
import numpy as np
import pytest
import torch

import conv_backward_cases as CB
import erp_resample_backward_cases as RB
import ref_ops_cases as C
import stale_memory as SM
from oracle import pconv_cpu as O
from test_gpu_conv_backward import same_bits as conv_same_bits


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)
    yield


# ---- the patterns ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,f32,f64,i32,u8", [("A", -1, -1, 0, 0), ("B", 0x3F3F3F3F, 0x3F3F3F3F3F3F3F3F, 0x01010101, 1)])
def test_bit_patterns(monkeypatch, kind, f32, f64, i32, u8):
    with SM.filled(monkeypatch, kind) as made:
        a = torch.empty((3, 5), dtype=torch.float32)
        b = torch.empty(7, dtype=torch.float64)
        c = torch.empty((2, 2), dtype=torch.int32)
        d = torch.empty((4, 4, 3), dtype=torch.uint8)
        like, new = torch.empty_like(a), a.new_empty((2, 3))
        wide = torch.empty_like(b)
    assert made == ["empty"] * 4 + ["empty_like", "new_empty", "empty_like"]
    for t in (a, like, new):
        assert bool((t.view(torch.int32) == f32).all()) and t.numel() > 0
    for t in (b, wide):
        assert bool((t.view(torch.int64) == f64).all())
    assert bool((c == i32).all()) and bool((d == u8).all())
    if kind == "A":
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    else:
        assert bool((a == np.float32(SM.B_FLOAT32)).all()) and abs(SM.B_FLOAT32 - 0.7470588) < 1e-7
        assert bool(torch.isfinite(b).all()) and 1e-4 < float(b[0]) < 1.0      # 0x3F3F...: 4.8e-4 as float64, finite
    for t in (a, b, c, d):
        assert bool(SM.holds_pattern(t, kind).all())
    assert SM.FLOAT_BYTE == {"A": 0xFF, "B": 0x3F} and SM.INT_BYTE == {"A": 0x00, "B": 0x01}
    # a float workspace takes the float pattern, whatever its element type
    assert SM.byte_for(torch.uint8, kind, "float") == SM.FLOAT_BYTE[kind] != SM.byte_for(torch.uint8, kind, "index")
    assert SM.byte_for(torch.uint8, kind) == SM.INT_BYTE[kind] == SM.byte_for(torch.int64, kind)


def test_scope_of_the_patch(monkeypatch):
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty, torch.zeros)
    for kind in SM.KINDS:
        with SM.filled(monkeypatch, kind):
            assert torch.zeros is real[3]
            assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.Tensor.new_empty is not real[2]
            z = torch.zeros((4, 4))
            assert bool((z.view(torch.int32) == 0).all())
            assert torch.empty(0).numel() == 0                                  # nothing to fill: no error
            p = torch.empty((2, 2), requires_grad=True)                         # a leaf that wants a gradient
            assert p.requires_grad and bool(SM.holds_pattern(p, kind).all())
            q = torch.empty((2, 3, 4, 5)).to(memory_format=torch.channels_last)
            assert bool(SM.holds_pattern(torch.empty_like(q), kind).all())      # dense, not contiguous
        assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, torch.zeros) == real
    with pytest.raises(RuntimeError, match="boom"):
        with SM.filled(monkeypatch, "A"):
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, torch.zeros) == real


def test_every_workspace_and_every_unwritten_region_cites_its_sentence():
    """the words each entry quotes stand in include/pconv_hip.h (or, for tile_conv2d's, in its docstring)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    squeeze = lambda s: re.sub(r"[\s*]+", " ", s)
    header = squeeze(open(os.path.join(root, "include", "pconv_hip.h")).read())
    pconv = squeeze(open(os.path.join(root, "pseudocylindrical_convolution_amd", "PCONV.py")).read())
    for name, (what, words) in SM.WORKSPACES.items():
        assert what in ("float", "index")
        for part in re.split(r" / |; ", words):
            assert squeeze(part) in header, (name, part)
        where, qualified = name.split(":")
        assert where == "PCONV.py" and re.search(r"def %s\(" % qualified.split(".")[-1], pconv), name
        if "." in qualified:      # Class.method / outer.inner: the owner exists too
            assert re.search(r"(class|def) %s\b" % qualified.split(".")[0], pconv), name
    assert set(SM.UNWRITTEN) == {"slice_pad_ring", "ring_output_before_forward_ring", "engine_stream_beyond_length"}
    for name, words in SM.UNWRITTEN.items():
        for part in words.split(" -- "):
            entry, sentence = part.split(": ", 1)
            where = pconv if entry.startswith("PCONV.") else header
            assert entry.replace("PCONV.", "") in where and squeeze(sentence) in where, (name, part)


def test_an_allocation_site_is_its_file_and_qualified_name(monkeypatch):
    """two functions named `backward` / `workspace` are two sites: only the ones WORKSPACES names are classified"""
    import sys

    class PseudoQuantOp(object):
        def backward(self):
            return SM.allocation_site(sys._getframe(0))

    class Other(PseudoQuantOp):
        pass

    class Unrelated(object):
        def backward(self):
            return SM.allocation_site(sys._getframe(0))

    def _conv_backward():
        def workspace():
            return SM.allocation_site(sys._getframe(0))
        return workspace()

    def workspace():
        return SM.allocation_site(sys._getframe(0))

    me = "test_stale_memory_cpu.py:"
    assert PseudoQuantOp().backward() == Other().backward() == me + "PseudoQuantOp.backward"
    assert Unrelated().backward() == me + "Unrelated.backward"
    assert _conv_backward() == me + "_conv_backward.workspace"
    assert workspace() == me + "test_an_allocation_site_is_its_file_and_qualified_name.workspace"
    for site in ("PCONV.py:PseudoQuantOp.backward", "PCONV.py:_conv_backward.workspace"):
        assert site in SM.WORKSPACES
    assert not any(key.split(":")[1] in ("backward", "workspace") for key in SM.WORKSPACES)


def test_refill_overwrites_what_an_op_owns_and_refuses_a_stepped_op_in_mid_pass():
    class Op(object):
        pass

    op = Op()
    op._top = {0: torch.zeros(3, 4), 1: torch.zeros(5, dtype=torch.int32), "partials": torch.zeros(16, dtype=torch.uint8),
               "tab": None}
    for kind in SM.KINDS:
        assert SM.refill(op, kind) == 3
        assert bool(SM.holds_pattern(op._top[0], kind).all()) and bool(SM.holds_pattern(op._top[1], kind).all())
        assert bool((op._top["partials"] == SM.FLOAT_BYTE[kind]).all())
    op.pidx_ = 3
    with pytest.raises(AssertionError):
        SM.refill(op, "A")
    op.pidx_ = 0
    assert SM.refill(op, "A") == 3


# ---- the comparators ------------------------------------------------------------------------------------------------

_results = {}


def oracle_results(name):
    if name not in _results:
        case = C.case_of(name)
        _results[name] = C.run(O, case, C.inputs(case))
    return _results[name]


def copy(res):
    return type(res)((k, v.clone()) for k, v in res.items())


def plant(t, index, kind):
    t[index] = SM.pattern(t.dtype, kind)


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("name,key,rule", [("slice_h2_w72_p0", "y", C.EQUAL), ("slice_h2_w72_p0", "gx", ("scale", 1e-5)),
                                           ("gmm_loss", "loss", ("abs", 1e-5)), ("econv_act_c6_p0_g2_i3_h2_w40", "last", C.EQUAL),
                                           ("quant_ntop2", "idx", C.EQUAL)])
def test_check_against_oracle_reports_one_filled_element(name, key, rule, kind):
    case, want = C.case_of(name), oracle_results(name)
    assert C.oracle_rule(case, key) == rule
    assert C.check_against_oracle(case, copy(want), want) == []
    bad = copy(want)
    t = bad[key]
    # a live element whose right value is not the pattern's: the largest one
    index = tuple(int(i) for i in np.unravel_index(int(want[key].double().abs().argmax()), tuple(t.shape)))
    assert not bool(SM.holds_pattern(t[index].reshape(1), kind).all())
    plant(t, index, kind)
    report = C.check_against_oracle(case, bad, want)
    assert len(report) == 1 and "/" + key + ":" in report[0], report


@pytest.mark.parametrize("kind", SM.KINDS)
def test_a_filled_element_in_a_dead_column_is_reported(kind):
    """slice `y`: the first column past the narrowest tile's width holds the pattern -- B (0.747, finite) as well as A"""
    name = "slice_h2_w72_p0"
    case, want = C.case_of(name), oracle_results(name)
    wd = C.widths(case)
    tile = min(range(C.NPART), key=lambda t: wd[t])
    assert wd[tile] < case["w"]
    bad = copy(want)
    assert bad["y"][tile, 0, 0, wd[tile]] == 0
    plant(bad["y"], (tile, 0, 0, wd[tile]), kind)
    report = C.check_against_oracle(case, bad, want)
    assert report and all("/y:" in line for line in report), report
    assert any("dead columns" in line for line in report) or kind == "A"       # (NaN != 0 too: asserted next)
    dead = C.dead_columns(case, "y", bad["y"])
    assert bool((bad["y"][dead] != 0).any())


@pytest.mark.parametrize("kind", SM.KINDS)
def test_same_bits_and_int32_views_report_one_filled_element(kind):
    ref = torch.rand(3, 4, 5, generator=torch.Generator().manual_seed(5)) + 1.0
    conv_same_bits(ref.clone(), ref, "untouched")
    assert torch.equal(ref.clone().view(torch.int32), ref.view(torch.int32)) and SM.same_bits(ref.clone(), ref)
    bad = ref.clone()
    plant(bad, (1, 2, 3), kind)
    with pytest.raises(AssertionError, match="1 of 60 entries differ"):
        conv_same_bits(bad, ref, "planted")
    assert not torch.equal(bad.view(torch.int32), ref.view(torch.int32))
    assert not SM.same_bits(bad, ref)
    # ... where a comparison of VALUES would let fill A through on both sides
    both = bad.clone()
    assert kind == "B" or not bool((both == bad).all())
    assert SM.same_bits(both, bad)
    wide = ref.double()
    bad = wide.clone()
    plant(bad, (0, 0, 0), kind)
    assert not SM.same_bits(bad, wide) and not torch.equal(bad.view(torch.int64), wide.view(torch.int64))
    ints = torch.arange(24, dtype=torch.int32).view(4, 6) + 7
    bad = ints.clone()
    plant(bad, (2, 2), kind)
    assert not torch.equal(bad, ints)


# ---- the references under the harness -------------------------------------------------------------------------------

TWIN_CASES = ["slice_h1_w40_p2_n2", "uslice_h2_w72_p1_cos", "pad_h2_w72_p1_filled", "epad_h1_w40_p2_n2_v1", "fill_p2_trim_v1",
              "quant_ntop2_train", "dtow_s2", "context_reshape", "mask_constrain_5", "wave_h1_w24_g2_nopt",
              "econv_plain_c5_p2_g4_i1_h1_w24_nopt", "gmm_loss", "gmm_table", "gmm_table_batch", "projects_bilinear"]


def test_twin_cases_name_every_family():
    assert {C.case_of(n)["op"] for n in TWIN_CASES} == {c["op"] for c in C.ALL_CASES.values()}


@pytest.mark.parametrize("name", TWIN_CASES)
def test_the_oracle_gives_the_same_bits_under_either_fill(monkeypatch, name):
    """the slice's pad ring is the one region the oracle itself leaves to the allocator (UNWRITTEN: slice_pad_ring)"""
    case = C.case_of(name)
    ins = C.inputs(case)
    runs = []
    for regime, enter in SM.regimes(monkeypatch):
        with enter():
            runs.append(C.run(O, case, ins))
    plain = runs[0]
    for regime, got in zip(("A", "B"), runs[1:]):
        assert list(got) == list(plain)
        for key in plain:
            a, b = got[key], plain[key]
            if case["op"] == "slice" and key == "y" and case["pad"] > 0:
                p = case["pad"]
                a, b = a[:, :, p:-p, p:-p], b[:, :, p:-p, p:-p]
            assert SM.same_bits(a, b), (name, key, regime)
        assert C.check_against_oracle(case, got, plain) == []


def test_the_resize_backward_twin_gives_the_same_bits_under_either_fill(monkeypatch):
    from pseudocylindrical_convolution_amd import erp_resample
    for case in RB.SMALL:
        g = RB.gradient(case)
        runs = []
        for regime, enter in SM.regimes(monkeypatch):
            with enter():
                runs.append(erp_resample.resize_backward_torch(g, case[2], case[3]))
        assert bool(torch.isfinite(runs[0]).all())
        assert SM.same_bits(runs[1], runs[0]) and SM.same_bits(runs[2], runs[0]), RB.case_id(case)


@pytest.mark.parametrize("name", ["b", "c"])
def test_the_convolution_backward_twin_gives_the_same_bits_under_either_fill(monkeypatch, name):
    case = CB.BY_NAME[name]
    x, weight, gout = CB.inputs(case)
    runs = []
    for regime, enter in SM.regimes(monkeypatch):
        with enter():
            runs.append((CB.twin_dgrad(weight, gout, case.h, case.w, case.s), CB.twin_wgrad(x, gout, case.k, case.s),
                         CB.twin_bgrad(gout)))
    for got in runs[1:]:
        for a, b, what in zip(got, runs[0], ("gin", "gw", "gb")):
            conv_same_bits(a, b, "%s of case %s" % (what, name))
    for a, b in zip(runs[0], CB.twin(case)):
        conv_same_bits(a, b, "the cached twin")
