"""PCONV.conv_plan: which kernel takes which output rows of a tile convolution.  The plan is arithmetic on the
layer's shape plus the library's own pconv_wino_supported / pconv_wino42_supported (host functions: no kernel is
launched, this runs without a GPU).  tests/test_gpu_wino.py and tests/test_gpu_wino42.py check on the GPU that
tile_conv2d launches what the plan says."""
import pytest


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


@pytest.fixture
def default_mode(monkeypatch):
    monkeypatch.delenv("PCONV_CONV3X3", raising=False)
    monkeypatch.setattr(P(), "WINO_ROW_SPLIT", True)
    monkeypatch.setattr(P(), "WINO_FLAT_REMAINDER", True)
    assert P().conv3x3_mode() == "wino42"


def plan(cin, h, w, cout, **kw):
    return P().conv_plan(cin, h, w, cout, 3, 1, **kw)


def probe_names(launches):
    """the kernel names tile_conv2d's probe reports for a plan (direct: conv_kernel_name's template name)"""
    return [P().CONV_KERNELS[kind].probe_name or "conv_mfma_kernel" for kind, _, _ in launches]


def test_default_mode_table(default_mode):
    """F(4x2) for 64-multiple couts whose output rows fill the 8-row blocks to 8/9 at least, F(2x2) for the rest of
    what Winograd takes (cin % 24 != 0: F(4x2) does not take it at all), the direct kernel below four output rows"""
    for (cfg, want) in (((32, 10, 66, 64), "wino_conv3x3_kernel"), ((96, 5, 66, 128), "conv_mfma_kernel"),
                        ((96, 10, 66, 96), "wino_conv3x3_kernel"), ((96, 10, 66, 128), "wino42_conv3x3_kernel"),
                        ((192, 10, 66, 192), "wino42_conv3x3_kernel"), ((192, 66, 66, 192), "wino42_conv3x3_kernel"),
                        ((192, 16, 66, 192), "wino_conv3x3_kernel"), ((192, 8, 66, 192), "wino_conv3x3_kernel")):
        launches, fallback = plan(*cfg)
        assert probe_names(launches) == [want], cfg
        assert launches[0][1:] == (0, cfg[1] - 2), cfg
        assert fallback == (want == "conv_mfma_kernel"), cfg


SPLIT_SHAPES = ((192, 68, 66, 192), (192, 36, 66, 192), (192, 20, 66, 192), (192, 12, 66, 192), (96, 14, 66, 64))


def test_row_split(default_mode):
    """a remainder of up to four rows behind whole 8-row blocks: the blocks on F(4x2), the remainder on F(2x2)"""
    for cfg in SPLIT_SHAPES:
        ho = cfg[1] - 2
        launches, fallback = plan(*cfg)
        assert probe_names(launches) == ["wino42_conv3x3_kernel", "wino_conv3x3_kernel"], cfg
        assert launches[0] == ("wino42", 0, ho // 8 * 8), cfg
        assert launches[1][1:] == (ho // 8 * 8, ho % 8), cfg
        assert not fallback


def test_row_split_off(default_mode, monkeypatch):
    monkeypatch.setattr(P(), "WINO_ROW_SPLIT", False)
    assert plan(192, 68, 66, 192) == ([("wino42", 0, 66)], False)    # a ninth 8-row block for two rows: 72 * 8 <= 9 * 66
    assert plan(192, 36, 66, 192) == ([("wino", 0, 34)], False)      # 40 * 8 > 9 * 34


def test_wino42_forced(default_mode, monkeypatch):
    """ "wino42!" takes every layer the kernel supports and never splits"""
    monkeypatch.setenv("PCONV_CONV3X3", "wino42!")
    assert plan(96, 10, 66, 96) == ([("wino42", 0, 8)], False)
    assert plan(192, 36, 66, 192) == ([("wino42", 0, 34)], False)
    assert plan(32, 10, 66, 64) == ([("wino", 0, 8)], False)         # cin % 24: F(4x2) does not take it


def test_mode_direct_and_wino(default_mode, monkeypatch):
    monkeypatch.setenv("PCONV_CONV3X3", "direct")
    for cfg in SPLIT_SHAPES + ((192, 10, 66, 192), (24, 6, 66, 40)):
        assert plan(*cfg) == ([("direct", 0, cfg[1] - 2)], False), cfg      # not wanted: no fallback either
    monkeypatch.setenv("PCONV_CONV3X3", "wino")
    for cfg in SPLIT_SHAPES + ((192, 10, 66, 192), (96, 10, 66, 128)):
        assert plan(*cfg) == ([("wino", 0, cfg[1] - 2)], False), cfg
    assert plan(24, 6, 66, 40) == ([("direct", 0, 4)], True)         # (test_wino_fallbacks_are_counted)
    assert plan(96, 6, 66, 96) == ([("wino", 0, 4)], False)


def test_fused_and_unaligned_layers_go_direct(default_mode):
    for cfg in SPLIT_SHAPES + ((192, 10, 66, 192), (96, 10, 66, 96)):
        direct = [("direct", 0, cfg[1] - 2)]
        assert plan(*cfg, fused=True) == (direct, False), cfg        # sigmoid / gate: Winograd was never wanted
        assert plan(*cfg, aligned=False) == (direct, True), cfg      # wanted, not taken: counted
        assert plan(*cfg, fused=True, aligned=False) == (direct, False), cfg


def test_two_row_launches_take_the_flat_entry(default_mode, monkeypatch):
    assert plan(192, 68, 66, 192)[0] == [("wino42", 0, 64), ("wino_flat", 64, 2)]
    assert plan(192, 4, 262, 192)[0] == [("wino_flat", 0, 2)]
    # a four-row remainder, or a four-row layer, never does
    assert plan(192, 14, 66, 192)[0] == [("wino42", 0, 8), ("wino", 8, 4)]
    assert plan(192, 6, 66, 192)[0] == [("wino", 0, 4)]
    monkeypatch.setenv("PCONV_CONV3X3", "wino")
    assert plan(192, 4, 262, 192)[0] == [("wino_flat", 0, 2)]
    monkeypatch.setattr(P(), "WINO_FLAT_REMAINDER", False)
    assert plan(192, 4, 262, 192)[0] == [("wino", 0, 2)]
    monkeypatch.delenv("PCONV_CONV3X3")
    assert plan(192, 68, 66, 192)[0] == [("wino42", 0, 64), ("wino", 64, 2)]
    # the flat build is the same kernel on the same weights
    flat, wino = P().CONV_KERNELS["wino_flat"], P().CONV_KERNELS["wino"]
    assert flat.entry != wino.entry and flat[1:] == wino[1:]


def test_other_kernel_sizes_and_strides_are_one_direct_launch(default_mode, monkeypatch):
    for mode in ("wino42", "wino42!", "wino", "direct"):
        monkeypatch.setenv("PCONV_CONV3X3", mode)
        for (k, stride, h, ho) in ((1, 1, 66, 66), (3, 2, 67, 33), (1, 2, 66, 33), (3, 2, 68, 33)):
            for kw in ({}, {"d2w": True}, {"aligned": False}):
                assert P().conv_plan(192, h, 66, 192, k, stride, **kw) == ([("direct", 0, ho)], False), (mode, k, stride)


def test_depth_to_width_layers(default_mode):
    assert plan(192, 10, 70, 768, d2w=True) == ([("wino42", 0, 8)], False)
    assert plan(192, 12, 70, 768, d2w=True) == ([("wino42", 0, 8), ("wino_flat", 8, 2)], False)


@pytest.mark.parametrize("mode", ["wino42", "wino42!", "wino"])
@pytest.mark.parametrize("split,flat", [(True, True), (False, True), (True, False)])
def test_plans_tile_the_output_rows_with_supported_launches(mode, split, flat, monkeypatch):
    """every plan covers [0, ho) exactly once and in order, the direct kernel only ever alone, and each Winograd launch
    satisfies its own kernel's predicate at its sub-shape (what the C entry point checks again)"""
    monkeypatch.setenv("PCONV_CONV3X3", mode)
    monkeypatch.setattr(P(), "WINO_ROW_SPLIT", split)
    monkeypatch.setattr(P(), "WINO_FLAT_REMAINDER", flat)
    lib = P()._native.hip_lib()
    for ho in range(2, 71):
        for cout in (32, 64, 96, 128, 192, 768):
            for cin in (24, 48, 96, 192):
                for d2w in (False, True):
                    launches, fallback = plan(cin, ho + 2, 66, cout, d2w=d2w)
                    at = 0
                    for kind, r0, rows in launches:
                        assert r0 == at and rows > 0, (cin, ho, cout, launches)
                        at += rows
                        supported = P().CONV_KERNELS[kind].supported
                        if supported is None:
                            assert len(launches) == 1 and fallback
                        else:
                            assert getattr(lib, supported)(cin, rows + 2, 66, cout, int(d2w)) == 1, (cin, ho, cout, launches)
                            assert (kind == "wino_flat") == (rows == 2 and flat) or kind == "wino42"
                    assert at == ho, (cin, ho, cout, launches)
                    assert fallback == (launches[0][0] == "direct")
