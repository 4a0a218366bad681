"""Shared by tests/test_options.py (CPU) and tests/test_gpu_option_paths.py (GPU): which GPU test launches the code
each tuning option of csrc/options.h selects, the option sets and shapes those tests run, and the launchers'
arithmetic restated in Python so that a test can say which launch shape a set produces.  No GPU, no import of the
package: plain data and integer arithmetic.

OPTIONS has one row per X-macro row of options.h; tests/test_options.py::test_every_option_has_a_gpu_test holds the
two lists together, so an option added to options.h without a GPU test that names it fails on the CPU."""
import collections

Row = collections.namedtuple("Row", "values file test")   # non-default values run (as set in the environment)

NEW = "test_gpu_option_paths.py"

# ---- a. the decoder step kernel (ee_conv / ee_step_kernel, csrc/entropy_engine.hip) --------------------------------

# h = 4, w = 128 (tests/test_gpu_engine.py's knob shape): 64 symbol rows, the longest wavefront plane has 60 positions
# and planes of EVERY length 1 .. 60 occur, so every parity of a share, empty parts (first >= cnt) and a half-filled
# last pair are reached without a larger frame
EE_SHAPE = (4, 128)
EE_LONGEST = 60
EE_FRAMES = (1, 3)    # one frame: automatic ppw 2; three frames = groups of 2 and 1 frames: automatic ppw 8 and 2
EE_NAMES = ("PCONV_EE_BLOCK", "PCONV_EE_PPW", "PCONV_EE_JOINT", "PCONV_EE_CONTIG", "PCONV_EE_XCD")


def _ee(**kw):
    return {"PCONV_EE_" + k: str(v) for k, v in kw.items()}


EE_SETS = [
    _ee(BLOCK=512),
    _ee(BLOCK=1024),
    _ee(BLOCK=1024, PPW=1),            # split 4, PJ = 1
    _ee(BLOCK=512, PPW=1),             # split 8, share 8 with a last share of 4
    _ee(PPW=1),
    _ee(PPW=3),
    _ee(PPW=5),
    _ee(PPW=16),
    _ee(JOINT=1),
    _ee(CONTIG=0),
    _ee(CONTIG=0, JOINT=1),
    _ee(CONTIG=2),
    _ee(CONTIG=2, JOINT=1),
    _ee(XCD=1),
    _ee(XCD=1, CONTIG=2),              # the pair DESIGN.md measured
    _ee(XCD=1, BLOCK=512, PPW=3),
]
# the wide nets (valid_dim 112 / 192): hidden layers ITER = 33 / 57 (always PJ = 1), input layers ITER = 11 / 19 (PJ = 2)
WIDE_SETS = [_ee(BLOCK=512), _ee(BLOCK=1024), _ee(XCD=1, CONTIG=2), _ee(JOINT=1)]
# (frames, symbol rows per tile, width) of tests/test_gpu_wide_models.py's SHAPES: the 60-position planes of the 14-group
# shape, and three frames (groups of 2 and 1) on 5 rows x 40 columns (odd rows, a width that is no multiple of 16)
WIDE_SHAPES = [(1, 4, 128), (3, 5, 40)]
WIDE_ITERS = {112: (11, 33), 192: (19, 57)}   # (input layer, hidden layers): ceil(cin * 25 / 64)
ITERS_56 = (6, 17)


def set_id(env):
    return "-".join("%s=%s" % (k.replace("PCONV_EE_", ""), v) for k, v in sorted(env.items())) or "default"


def group_frames(nimg, groups):
    """frames per lock-step group (csrc/engine.cpp init)"""
    return [nimg // groups + (1 if k < nimg % groups else 0) for k in range(groups)]


EeLaunch = collections.namedtuple("EeLaunch", "block ppw split pj contig xcd")


def ee_launch(env, group_nimg, longest, iters):
    """what ee_conv makes of an option set for a group of `group_nimg` frames: threads per workgroup, positions per
    wave, workgroups per (set, plane, image), and the PJ of the kernel per ITER of `iters`"""
    block = int(env.get("PCONV_EE_BLOCK", 256))
    block = block if block in (512, 1024) else 256
    ppw = int(env.get("PCONV_EE_PPW", 0))
    ppw = ppw if ppw > 0 else (2 if group_nimg <= 1 else 8)
    joint = int(env.get("PCONV_EE_JOINT", 2))
    waves = block // 64
    split = max(1, -(-longest // (waves * ppw)))
    pj = tuple(2 if (joint == 2 and it <= 20 and ppw >= 2) else 1 for it in iters)
    return EeLaunch(block, ppw, split, pj, int(env.get("PCONV_EE_CONTIG", 1)), int(env.get("PCONV_EE_XCD", 0)))


def shares(cnt, split):
    """positions of each of the `split` contiguous shares of a plane of cnt positions (0: an empty part)"""
    share = -(-cnt // split)
    return [max(0, min(cnt, (p + 1) * share) - p * share) for p in range(split)]


def step_planes(nstart, ngroup):
    """planes in the window of every wavefront step (csrc/engine.cpp window()); nstart = len(plane_start) = rows + w"""
    out = []
    for s in range(nstart - 1 + ngroup - 1):
        st, end = max(0, s - ngroup + 1), (s + 1 if s < nstart - 2 else nstart - 1)
        out.append(max(0, end - st))
    return out


# ---- b. PCONV_CONV_XCD on the direct 3x3 kernel (conv_mfma_kernel, csrc/conv.hip) ----------------------------------

# couts 33 .. 96 take conv_mfma_kernel<3, 1, 1, 8, 3, S, 4>: 96 couts x (4 rows x 64 columns) per workgroup, so
# cblocks = 1, a stripe = xcd_group = tiles_r workgroups, stripes = tn * tiles_c, and the kernel permutes the first
# full = floor(stripes / 8) * 8 stripes.  (name, tn, cin, h, w, cout, stride, stripes, what it reaches)
ConvCase = collections.namedtuple("ConvCase", "name tn cin h w cout stride stripes")
CONV_XCD_CASES = [
    ConvCase("s1-6-stripes", 3, 24, 8, 70, 64, 1, 6),         # fewer than 8: full = 0, the identity; 2 row tiles
    ConvCase("s1-8-by-tiles", 8, 24, 8, 66, 96, 1, 8),        # 8 tiles x 1 column tile: all permuted, no remainder
    ConvCase("s1-8-by-columns", 1, 32, 9, 504, 64, 1, 8),     # 1 tile x 8 column tiles (the last ragged: 502 columns)
    ConvCase("s1-11-by-tiles", 11, 24, 12, 40, 96, 1, 11),    # 8 permuted + 3 in place; 3 row tiles, the last ragged
    ConvCase("s1-11-by-columns", 1, 48, 10, 652, 64, 1, 11),  # 11 column tiles of one tile
    ConvCase("s2-4-stripes", 2, 24, 15, 131, 64, 2, 4),       # stride 2: 7 x 65 outputs, the identity
    ConvCase("s2-8-mixed", 4, 32, 17, 131, 96, 2, 8),         # 4 tiles x 2 column tiles
    ConvCase("s2-11-by-tiles", 11, 24, 13, 41, 64, 2, 11),
    ConvCase("s2-11-by-columns", 1, 24, 15, 1301, 96, 2, 11),
]
CONV_TILE_ROWS, CONV_TILE_COLS, CONV_TILE_COUTS = 4, 64, 96


def conv_xcd_launch(case):
    """(stripes, xcd_group, grid, full) of launch_conv for a case of CONV_XCD_CASES"""
    ho, wo = (case.h - 3) // case.stride + 1, (case.w - 3) // case.stride + 1
    tiles_r, tiles_c = -(-ho // CONV_TILE_ROWS), -(-wo // CONV_TILE_COLS)
    cblocks = -(-case.cout // CONV_TILE_COUTS)
    group = cblocks * tiles_r
    grid = case.tn * tiles_r * tiles_c * cblocks
    return grid // group, group, grid, grid // (8 * group) * 8 * group


# ---- c. PCONV_RESAMPLE_ROWS (rows_per_block of pconv_sphere_slice / _uslice, csrc/resample.hip) --------------------

RESAMPLE_ROWS = ("1", "2", "4")
# ERP shape (n, c, height, width) with 16 latitude tiles -> rows_per_block per setting
RESAMPLE_CASES = [
    ((1, 3, 64, 128), {"1": 1, "2": 2, "4": 4}),     # 4 rows per tile: 4 is taken
    ((1, 3, 96, 128), {"1": 1, "2": 2, "4": 2}),     # 6 rows per tile: 4 does not divide them, falls to 2
    ((1, 3, 48, 128), {"1": 1, "2": 1, "4": 1}),     # 3 rows per tile: everything falls to 1
    ((1, 3, 64, 8192), {"1": 1, "2": 2, "4": 2}),    # 4 rows x 8192 x 4 B = 128 KiB of LDS: 4 falls to 2
]


def rows_per_block(tile_rows, width, cap):
    rb = cap if 1 <= cap <= 4 else 4
    while rb > 1 and (tile_rows % rb != 0 or rb * width * 4 > 64 * 1024):
        rb >>= 1
    return rb


# ---- the table -----------------------------------------------------------------------------------------------------

def _values(name, *sets):
    return tuple(sorted({env[name] for group in sets for env in group if name in env}, key=lambda v: (len(v), v)))


_KNOBS = ("test_gpu_engine.py", "test_engine_knobs_that_must_not_change_a_stream")
_VARIANTS = ("test_gpu_entropy_mfma.py", "test_measured_variants_of_the_matrix_core_kernel_agree")
_RESIDENT = ("test_gpu_ops.py", "test_resident_1x1_equals_tiled_kernel")
_STEP = (NEW, "test_step_kernel_launch_shapes")
REST_SETS = [{"PCONV_EE_BULK0": "valu"}, {"PCONV_ENGINE_WORKERS": "1"}, {"PCONV_ENGINE_WORKERS": "2"},
             {"PCONV_ENGINE_BLOCKING_SYNC": "1"}, {"PCONV_ENGINE_SPIN_US": "0"}, {"PCONV_ENGINE_SPIN_US": "50"},
             {"PCONV_ENGINE_TIMING": "1"}]
_REST = (NEW, "test_host_side_engine_options_keep_the_streams")
STAGGER = ("1", "3")
ALLOC_FILL = ("0xFF", "0x3F")     # the two float patterns of tests/stale_memory.py over every buffer an engine allocates

OPTIONS = {
    "PCONV_EE_BLOCK": Row(_values("PCONV_EE_BLOCK", EE_SETS, WIDE_SETS), *_STEP),
    "PCONV_EE_PPW": Row(_values("PCONV_EE_PPW", EE_SETS), *_STEP),
    "PCONV_EE_JOINT": Row(_values("PCONV_EE_JOINT", EE_SETS, WIDE_SETS), *_STEP),
    "PCONV_EE_CONTIG": Row(_values("PCONV_EE_CONTIG", EE_SETS, WIDE_SETS), *_STEP),
    "PCONV_EE_XCD": Row(_values("PCONV_EE_XCD", EE_SETS, WIDE_SETS), *_STEP),
    "PCONV_EE_FUSE_PPW": Row(("2",), *_KNOBS),
    "PCONV_EE_MFMA_WSRC": Row(("ring",), *_VARIANTS),
    "PCONV_EE_MFMA_WAVES": Row(("8",), *_VARIANTS),
    "PCONV_EE_MFMA_NT": Row(("2",), *_VARIANTS),
    "PCONV_ENGINE_GROUPS": Row(("1",), "test_gpu_codec_vs_oracle.py", "test_engine_lockstep_pair_equals_oracle"),
    "PCONV_ENGINE_WORKERS": Row(_values("PCONV_ENGINE_WORKERS", REST_SETS), *_REST),
    "PCONV_ENGINE_CHAIN": Row(("queued", "host"), "test_gpu_engine.py", "test_queued_chain_equals_host_driven_chain"),
    "PCONV_ENGINE_BLOCKING_SYNC": Row(_values("PCONV_ENGINE_BLOCKING_SYNC", REST_SETS), *_REST),
    "PCONV_ENGINE_SPIN_US": Row(_values("PCONV_ENGINE_SPIN_US", REST_SETS), *_REST),
    "PCONV_ENGINE_ROWS": Row(("int32",), *_KNOBS),
    "PCONV_ENGINE_STEPWISE_ENCODER": Row(("1",), *_KNOBS),
    "PCONV_ENGINE_CLEAR_EVERY_CALL": Row(("1",), NEW, "test_clear_every_call_keeps_the_streams"),
    "PCONV_ENGINE_ALLOC_FILL": Row(ALLOC_FILL, "test_gpu_stale_memory.py", "test_engine_results_do_not_depend_on_fresh_memory"),
    "PCONV_ENGINE_ENCODE_RANGES": Row(("1", "7"), *_KNOBS),
    "PCONV_ENGINE_ENCODE_INTERLEAVE": Row(("0",), *_KNOBS),
    "PCONV_ENGINE_RATE_STREAMS": Row(("groups",), NEW, "test_rate_on_group_streams_gives_the_same_bits"),
    "PCONV_ENGINE_TIMING": Row(_values("PCONV_ENGINE_TIMING", REST_SETS), *_REST),
    "PCONV_EE_BULK": Row(("valu",), "test_gpu_wide_models.py", "test_wide_streams_equal_vector_kernel"),
    "PCONV_EE_BULK0": Row(_values("PCONV_EE_BULK0", REST_SETS), *_REST),
    "PCONV_EE_MFMA_FORM": Row(("16x4",), *_KNOBS),
    "PCONV_EE_FUSE_TABLES": Row(("1",), *_KNOBS),
    "PCONV_CONV1X1": Row(("tiled", "resident"), *_RESIDENT),
    "PCONV_CONV1X1_STAGGER": Row(STAGGER, NEW, "test_staggered_resident_1x1_equals_unstaggered"),
    "PCONV_CONV1X1_WAYOUT": Row(("batch", "pipe"), *_RESIDENT),
    "PCONV_CONV_SMALL": Row(("0",), "test_gpu_ops.py", "test_small_cout_3x3_kernel"),
    "PCONV_CONV_XCD": Row(("1",), NEW, "test_xcd_order_of_the_direct_3x3_kernel"),
    "PCONV_RESAMPLE_ROWS": Row(tuple(v for v in RESAMPLE_ROWS if v != "2"), NEW, "test_resample_rows_per_block"),
}

# the values that had no launch anywhere before tests/test_gpu_option_paths.py; they stay in the rows above
MUST_RUN = {
    "PCONV_EE_BLOCK": ("512", "1024"), "PCONV_EE_PPW": ("1", "3", "5", "16"), "PCONV_EE_JOINT": ("1",),
    "PCONV_EE_CONTIG": ("0", "2"), "PCONV_EE_XCD": ("1",), "PCONV_CONV_XCD": ("1",), "PCONV_RESAMPLE_ROWS": ("1", "4"),
    "PCONV_CONV1X1_STAGGER": ("1", "3"), "PCONV_ENGINE_CLEAR_EVERY_CALL": ("1",), "PCONV_ENGINE_RATE_STREAMS": ("groups",),
}
