"""GPU: every kernel path a tuning option of csrc/options.h selects, against the bits of the default path.

DESIGN.md ("What runs by default") and INTEGRATION.md promise "the same bits" for every PCONV_ variable; this file
launches the values that no other test launches (tests/option_cases.py holds the table, the option sets and the shapes;
tests/test_options.py::test_every_option_has_a_gpu_test keeps the table complete).  Everything here is exact:
torch.equal or equal bytes, no tolerance anywhere.

  a. the decoder step kernel's launch shapes (PCONV_EE_BLOCK / _PPW / _JOINT / _CONTIG / _XCD): an engine created under
     a set decodes the default engine's streams into the coded symbols, and with the stepwise encoder (network_step +
     ee_conv with the engine's launch options, step by step) writes the default engine's bytes;
  b. PCONV_CONV_XCD=1: the stripe permutation of conv_mfma_kernel, forward and through the native data gradient;
  c. PCONV_RESAMPLE_ROWS: rows a workgroup of slice / uslice stages;
  d. PCONV_CONV1X1_STAGGER, PCONV_ENGINE_CLEAR_EVERY_CALL, PCONV_ENGINE_RATE_STREAMS and the host-side engine options.

Resources of ee_step_kernel<CIN, ITER, BLOCK, PJ> as built for gfx950 (kernel descriptors / metadata notes of the code
object; static LDS bytes, VGPRs, scratch bytes per lane).  BLOCK = 512 and 1024 ran for the first time with this file:

    CIN ITER PJ |  LDS   | VGPRs at BLOCK 256 / 512 / 1024 | scratch
     14    6  1 |   6144 |  43 /  43 /  43                 | 0
     14    6  2 |   7680 |  48 /  48 /  48                 | 0
     28   11  1 |  11264 |  59 /  59 /  59                 | 0
     28   11  2 |  14080 |  58 /  58 /  58                 | 0
     42   17  1 |  17408 |  56 /  56 /  76                 | 0
     42   17  2 |  21760 |  70 /  70 /  70                 | 0
     48   19  1 |  19456 |  60 /  60 /  82                 | 0
     48   19  2 |  24320 |  74 /  74 /  74                 | 0
     84   33  1 |  33792 | 124 / 124 / 124                 | 0
    144   57  1 |  58368 | 196 / 136 / 128                 | 0 / 0 / 44 (10 VGPRs spilled at BLOCK 1024)

Every one can be launched: the largest static LDS is 58368 B (57 x 64 float4), below the 64 KiB a kernel gets without
asking; a 1024-thread workgroup is 16 waves = 4 per SIMD, which 512 VGPRs per SIMD allow up to 128 VGPRs per wave
(__launch_bounds__(1024, 4): the compiler keeps to 128 and spills 10 registers of the 144-channel layer to 44 B of
scratch); a 512-thread workgroup is 2 waves per SIMD, 256 VGPRs allowed, 136 used.  No agprs, no dynamic stack."""
import ctypes

import numpy as np
import pytest
import torch

import option_cases as OC
from oracle import pconv_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W16 = [15., 31., 54., 63., 63., 64., 64., 64., 64., 64., 64., 63., 63., 54., 31., 15.]


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)
    yield


def _clean(monkeypatch):
    """no tuning variable set: what the reference engines and calls run under"""
    for name in list(OC.OPTIONS) + ["PCONV_ENGINE_CU_MASK"]:
        monkeypatch.delenv(name, raising=False)


def _engine(ent, h, w, n):
    from pseudocylindrical_convolution_amd.engine import EntropyEngine
    return EntropyEngine(ent, h, w, n, DEV)


_NETS, _REFS = {}, {}


def _net(vd):
    """the entropy net of tests/test_gpu_engine.py (56) / tests/test_gpu_wide_models.py (112, 192), made once"""
    if vd not in _NETS:
        if vd == 56:
            from test_gpu_engine import _codec
            _NETS[vd] = _codec()[0].ent
        else:
            from test_gpu_wide_models import _ent
            _NETS[vd] = _ent(vd)
    return _NETS[vd]


def _reference(vd, n, h, w, seed, monkeypatch):
    """(net, symbols, streams of an engine created with no variable set), made once per shape and left unchanged"""
    key = (vd, n, h, w, seed)
    if key not in _REFS:
        _clean(monkeypatch)
        ent = _net(vd)
        sym = torch.randint(0, 8, (ent.npart * n, ent.ngroup, h, w), generator=torch.Generator().manual_seed(seed)).float().cuda()
        sym = ent.fill(sym).contiguous()
        eng = _engine(ent, h, w, n)
        streams = eng.encode(sym)
        assert len(set(streams)) == n and torch.equal(eng.decode(streams), sym)
        _REFS[key] = (ent, sym, streams)
    return _REFS[key]


def _wavefront(h, w, npart=16):
    """plane_start of the wavefront schedule (pconv_host_wavefront): host code, no GPU"""
    from pseudocylindrical_convolution_amd import _native
    from pseudocylindrical_convolution_amd.PCONV_operator.base import set_weight
    weight = np.asarray(set_weight(npart, True), dtype=np.float32)
    widths, order = np.zeros(npart, np.int32), np.zeros(npart * h * w, np.int32)
    start = np.zeros(npart * h + w, np.int32)
    _native.call("pconv_host_tile_widths", weight.ctypes.data, npart, npart * h, w, widths.ctypes.data)
    _native.call("pconv_host_wavefront", widths.ctypes.data, npart, h, w, order.ctypes.data, start.ctypes.data)
    return start


def _groups(n):
    """lock-step groups an engine of n frames is created with (pconv_ee_host_plan, the environment as it is)"""
    from pseudocylindrical_convolution_amd import _native
    plan = [ctypes.c_int(-1) for _ in range(4)]
    assert _native.hip_lib().pconv_ee_host_plan(n, *[ctypes.addressof(v) for v in plan]) == 0
    return OC.group_frames(n, plan[0].value)


def _runs_the_default_bits(env, vd, n, h, w, seed, monkeypatch):
    ent, sym, ref = _reference(vd, n, h, w, seed, monkeypatch)
    _clean(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dec = _engine(ent, h, w, n)
    for k, v in env.items():
        assert dec.option(k) == int(v), (env, k)
    assert dec.option("PCONV_ENGINE_STEPWISE_ENCODER") == 0
    assert torch.equal(dec.decode(ref), sym), "%s: the default engine's streams decode to other symbols" % (env,)
    monkeypatch.setenv("PCONV_ENGINE_STEPWISE_ENCODER", "1")
    enc = _engine(ent, h, w, n)
    for k, v in env.items():
        assert enc.option(k) == int(v), (env, k)
    assert enc.option("PCONV_ENGINE_STEPWISE_ENCODER") == 1
    got = enc.encode(sym)
    assert got == ref, "%s: stepwise encoder writes other bytes (%s vs %s)" % (env, [len(s) for s in got], [len(s) for s in ref])


# ---- a. the decoder step kernel's launch shapes --------------------------------------------------------------------

def launch_table(groups_of=_groups):
    """[(set id, frames, frames of the group, EeLaunch)] of every option set at EE_SHAPE"""
    rows = []
    for env in OC.EE_SETS:
        for n in OC.EE_FRAMES:
            for gn in sorted(set(groups_of(n))):
                rows.append((OC.set_id(env), n, gn, OC.ee_launch(env, gn, OC.EE_LONGEST, OC.ITERS_56)))
    return rows


def test_step_kernel_sets_cover_the_launcher(monkeypatch):
    """from ee_conv's split formula: the sets of test_step_kernel_launch_shapes reach split = 1, a split with an uneven
    last share, empty parts, PJ = 1 through ppw < 2 and through PCONV_EE_JOINT=1, and under PCONV_EE_XCD a workgroup count
    that is no multiple of 8 (the padded 1-D grid's `v >= nb` exit)"""
    _clean(monkeypatch)
    h, w = OC.EE_SHAPE
    start = _wavefront(h, w)
    counts = np.diff(start)
    assert counts.max() == OC.EE_LONGEST == 60 and set(range(1, 61)) <= set(counts.tolist())
    planes = OC.step_planes(len(start), 14)
    assert len(planes) == 16 * h + w + 14 - 2 and max(planes) == 14 and min(planes) == 1
    seen = set()
    for name, n, gn, launch in launch_table():
        print("%-26s frames %d group of %d: block %4d ppw %2d split %d PJ %s" % (name, n, gn, launch.block, launch.ppw,
                                                                                launch.split, launch.pj))
        env = dict(kv.split("=") for kv in name.split("-")) if name != "default" else {}
        if launch.split == 1:
            seen.add("split 1")
        if launch.split > 1 and launch.contig:
            last = [OC.shares(int(c), launch.split) for c in counts]
            if any(0 < s[-1] < s[0] for s in last):
                seen.add("uneven last share")
            if any(s[-1] == 0 for s in last):
                seen.add("empty part")
        if launch.split > 1 and not launch.contig and any(int(c) <= (launch.split - 1) * launch.block // 64 for c in counts):
            seen.add("empty interleaved part")
        if launch.pj == (1, 1) and launch.ppw < 2:
            seen.add("PJ 1 by ppw")
        if launch.pj == (1, 1) and launch.ppw >= 2:
            assert env.get("JOINT") == "1"
            seen.add("PJ 1 by joint")
        if launch.pj == (2, 2):
            seen.add("PJ 2 contig %d" % launch.contig)
        if launch.xcd and any((launch.split * p * 3 * gn) % 8 for p in planes):
            seen.add("XCD grid padded")
    assert seen >= {"split 1", "uneven last share", "empty part", "empty interleaved part", "PJ 1 by ppw", "PJ 1 by joint",
                    "PJ 2 contig 0", "PJ 2 contig 1", "PJ 2 contig 2", "XCD grid padded"}, seen
    # the two shapes the table of option sets promises
    assert OC.ee_launch(OC.EE_SETS[2], 1, 60, OC.ITERS_56)[:4] == (1024, 1, 4, (1, 1))
    assert OC.ee_launch(OC.EE_SETS[3], 1, 60, OC.ITERS_56)[:4] == (512, 1, 8, (1, 1)) and OC.shares(60, 8) == [8] * 7 + [4]
    # the automatic ppw: 2 for a group of one frame, 8 for more
    assert OC.ee_launch({}, 1, 60, OC.ITERS_56)[1:3] == (2, 8) and OC.ee_launch({}, 2, 60, OC.ITERS_56)[1:3] == (8, 2)
    # the wide nets: hidden layers always PJ = 1, input layers PJ = 2 unless PCONV_EE_JOINT=1
    for vd, iters in OC.WIDE_ITERS.items():
        assert iters == tuple(-(-c * 25 // 64) for c in (vd // 4, 3 * vd // 4))
        for env in OC.WIDE_SETS:
            assert OC.ee_launch(env, 1, 60, iters).pj == ((1, 1) if "PCONV_EE_JOINT" in env else (2, 1))


@pytest.mark.parametrize("n", OC.EE_FRAMES)
@pytest.mark.parametrize("env", OC.EE_SETS, ids=OC.set_id)
def test_step_kernel_launch_shapes(env, n, hip_backend, monkeypatch):
    """PCONV_EE_BLOCK, PCONV_EE_PPW, PCONV_EE_JOINT, PCONV_EE_CONTIG, PCONV_EE_XCD: every launch shape of ee_step_kernel
    reads and writes the default's bits.  4 x 128 symbols per tile: the longest wavefront plane has 60 positions and
    planes of every length 1 .. 60 occur (asserted here as in test_engine_knobs_that_must_not_change_a_stream); one frame
    and three (groups of two and one: the automatic ppw is 8 and 2).  The symbols are that test's draw."""
    assert set(env) <= set(OC.EE_NAMES) == {"PCONV_EE_BLOCK", "PCONV_EE_PPW", "PCONV_EE_JOINT", "PCONV_EE_CONTIG", "PCONV_EE_XCD"}
    h, w = OC.EE_SHAPE
    assert np.diff(_wavefront(h, w)).max() == 60
    _runs_the_default_bits(env, 56, n, h, w, 29, monkeypatch)


@pytest.mark.parametrize("vd", [112, 192])
@pytest.mark.parametrize("env", OC.WIDE_SETS, ids=OC.set_id)
def test_step_kernel_launch_shapes_of_the_wide_nets(env, vd, hip_backend, monkeypatch):
    """the 28 / 48-group nets under PCONV_EE_BLOCK, PCONV_EE_JOINT and PCONV_EE_XCD + PCONV_EE_CONTIG: hidden layers of
    ITER = 33 / 57 (always one position per loop body), input layers of ITER = 11 / 19 (two, one under JOINT=1)"""
    for k, (n, h, w) in enumerate(OC.WIDE_SHAPES):
        _runs_the_default_bits(env, vd, n, h, w, 100 + k, monkeypatch)


# ---- b. PCONV_CONV_XCD ---------------------------------------------------------------------------------------------

class _Probe(object):
    def __init__(self):
        self.records = []


def _poison(shape, ring=0, dtype=torch.float32):
    """NaN where the next torch.empty of this shape lands (the caching allocator hands the freed block out again): a
    workgroup that skips its tile must not find the right values of an earlier call there.  The tests below also keep
    every result alive, so that no block holding right values is ever free.
    (tests/test_gpu_stale_memory.py holds the same calls -- tile_conv2d with its epilogues and rings, the data gradient,
    rate() -- with the stronger mechanism: torch.empty itself returns filled memory, whatever block the allocator picks.)"""
    shape = tuple(shape[:-2]) + (shape[-2] + 2 * ring, shape[-1] + 2 * ring)
    del_me = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    del del_me


def _conv_inputs(case, seed=71):
    g = torch.Generator().manual_seed(seed)
    k = 3
    x = torch.randn(case.tn, case.cin, case.h, case.w, generator=g)
    wt = torch.randn(case.cout, case.cin, k, k, generator=g) * (1.0 / np.sqrt(case.cin * k * k))
    b, sl = torch.randn(case.cout, generator=g), torch.rand(case.cout, generator=g)
    ho, wo = (case.h - k) // case.stride + 1, (case.w - k) // case.stride + 1
    res = torch.randn(case.tn, case.cout, ho, wo, generator=g)
    # valid widths per tile: whole, a little over half (dead column tiles where there are several), ragged, none
    limit = torch.tensor(([wo, wo // 2 + 1, wo - 3, 0] * case.tn)[:case.tn], dtype=torch.int32)
    if case.tn == 1:
        limit[0] = wo // 2 + 1
    return x, wt, b, sl, res, limit


@pytest.mark.parametrize("case", OC.CONV_XCD_CASES, ids=[c.name for c in OC.CONV_XCD_CASES])
def test_xcd_order_of_the_direct_3x3_kernel(case, hip_backend, monkeypatch):
    """PCONV_CONV_XCD=1 permutes the workgroups of conv_mfma_kernel in whole stripes (xcd_group = cblocks * tiles_r
    workgroups of one column tile): the first full = floor(stripes / 8) * 8 stripes are dealt XCD-major, the remainder
    keeps its place.  Fewer than 8 stripes (the identity), exactly 8, and 11 (8 permuted, 3 in place), the count reached
    by the tile count and by the column tiles, stride 1 and 2 -- the outputs are those of the unpermuted launch and of the
    oracle's fmaf chain: plain, with bias + PReLU over a column limit that leaves some stripes dead, and with residual +
    trim into a ring buffer."""
    from pseudocylindrical_convolution_amd import _native
    PC = P()
    monkeypatch.setenv("PCONV_CONV3X3", "direct")
    monkeypatch.delenv("PCONV_CONV_XCD", raising=False)
    stripes, group, grid, full = OC.conv_xcd_launch(case)
    assert stripes == case.stripes and full == stripes // 8 * 8 * group and grid == stripes * group
    x, wt, b, sl, res, limit = _conv_inputs(case)
    wo = res.shape[3]
    dead = [-(-int(v) // 64) * 64 for v in limit]               # first column of a tile's dead column tiles
    if stripes > case.tn:
        assert any(d < wo for d in dead), "no dead stripe in this case"
    xg, wg, bg, sg, rg, lg = (t.to(DEV) for t in (x, wt, b, sl, res, limit))
    owner = type("Owner", (), {})()

    def variants():
        out = []
        for args, kw in (((None,), {}), ((sg, lg, case.tn), {}), ((sg, lg, case.tn), dict(residual=rg, trim=True, ring=2))):
            _poison(res.shape, kw.get("ring", 0))
            out.append(PC.tile_conv2d(owner, xg, wg, bg, case.stride, *args, **kw))
        return out

    # the permuted launches first, into poisoned memory: no output of this case exists anywhere yet
    probe = _Probe()
    monkeypatch.setattr(PC, "conv_probe", probe)
    monkeypatch.setenv("PCONV_CONV_XCD", "1")
    assert _native.option("PCONV_CONV_XCD") == 1
    permuted = variants()
    monkeypatch.setattr(PC, "conv_probe", None)
    monkeypatch.delenv("PCONV_CONV_XCD")
    assert _native.option("PCONV_CONV_XCD") == 0
    plain = variants()
    # the launches: the 96-cout x (4 rows x 64 columns) tile this case's stripe count is derived from
    assert [r[0] for r in probe.records] == ["conv_mfma_kernel<3, 1, 1, 8, 3, %d, 4, false>" % case.stride] * 3
    mt, nt, wm, wn = 3, 1, 1, 8
    assert (32 * mt * wm, wn * nt // 2) == (OC.CONV_TILE_COUTS, OC.CONV_TILE_ROWS) and case.cout <= OC.CONV_TILE_COUTS
    assert case.tn * -(-wo // OC.CONV_TILE_COLS) == case.stripes
    for i, (a, r) in enumerate(zip(plain, permuted)):
        assert torch.equal(a, r), "variant %d: %d outputs differ from the unpermuted launch" % (i, int((a != r).sum()))
    chain, chain_act = O.conv2d_chain(x, wt, b, case.stride, None), O.conv2d_chain(x, wt, b, case.stride, sl)
    limited, trimmed = chain_act.clone(), res + chain_act
    for t in range(case.tn):
        limited[t, :, :, dead[t]:] = 0
        trimmed[t, :, :, int(limit[t]):] = 0
    for i, ref in enumerate((chain, limited, trimmed)):
        assert torch.equal(permuted[i].cpu(), ref), "variant %d differs from the fmaf chain" % i


def test_xcd_order_in_the_native_data_gradient(hip_backend, monkeypatch):
    """the data gradient of PCONV.tile_conv2d_backward is the forward kernel on the prepared gradient: under
    PCONV_CONV_XCD=1 its 5 tiles x 2 column tiles = 10 stripes (8 permuted, 2 in place; 2 row tiles each) give the bits
    of the CPU twin (tests/conv_backward_cases.py) and of the call without the variable"""
    import conv_backward_cases as C
    case = C.Case("x", 3, 1, 40, 24, 7, 70, 5, True, False)     # the transposed layer: 24 -> 40 channels, 7 x 70 outputs
    assert OC.conv_xcd_launch(OC.ConvCase("dgrad", case.tn, case.cout, case.h + 2, case.w + 2, case.cin, 1, 10))[0] == 10
    x, weight, gout = C.inputs(case)
    xg, wg, gg = x.to(DEV), weight.to(DEV), gout.to(DEV)

    def run():
        _poison(x.shape)
        return P().tile_conv2d_backward(xg, wg, gg, case.s, (True, False, False))[0]

    monkeypatch.setenv("PCONV_CONV_XCD", "1")
    permuted = run()
    monkeypatch.delenv("PCONV_CONV_XCD")
    plain = run()
    twin = C.twin_dgrad(weight, gout, case.h, case.w, case.s)
    assert torch.equal(C.bits(permuted), C.bits(plain))
    assert torch.equal(C.bits(permuted), C.bits(twin))


# ---- c. PCONV_RESAMPLE_ROWS ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["slice", "uslice"])
@pytest.mark.parametrize("shape,rows", OC.RESAMPLE_CASES, ids=["x".join(map(str, s)) for s, _ in OC.RESAMPLE_CASES])
def test_resample_rows_per_block(shape, rows, op, hip_backend, monkeypatch):
    """PCONV_RESAMPLE_ROWS = 1 / 2 / 4, the rows a workgroup of slice_kernel / uslice_kernel stages in LDS: bit for bit
    the oracle and the call without the variable.  rows_per_block (csrc/resample.hip) halves the setting while it does
    not divide the tile's rows or needs more than 64 KiB:
        1x3x64x128   4 rows per tile           1 -> 1, 2 -> 2, 4 -> 4
        1x3x96x128   6 rows per tile           1 -> 1, 2 -> 2, 4 -> 2
        1x3x48x128   3 rows per tile           1 -> 1, 2 -> 1, 4 -> 1
        1x3x64x8192  4 rows, 32 KiB each       1 -> 1, 2 -> 2, 4 -> 2
    The backward kernels do NOT share this function: csrc/backward.hip and csrc/backward_ordered.hip each have a
    rows_per_block of their own that reads no option (a function of the shape alone).  The ordered backward is run under
    every setting all the same, at the first two shapes, and stays the oracle's bits."""
    from pseudocylindrical_convolution_amd import _native
    from test_gpu_backward_ordered import slice_pair, uslice_pair
    n, c, height, width = shape
    assert rows == {v: OC.rows_per_block(height // 16, width, int(v)) for v in OC.RESAMPLE_ROWS}
    pads = (0,) if width > 1024 else (0, 1)
    for pad in pads:
        g = torch.Generator().manual_seed(3 + pad)
        if op == "slice":
            x = torch.rand(n, c, height, width, generator=g)
            gop, cop = P().SphereSliceOp(16, 0, pad, W16, 0, False), O.SphereSliceOp(16, 0, pad, W16)
        else:
            x = torch.rand(16 * n, c, height // 16 + 2 * pad, width + 2 * pad, generator=g)
            gop, cop = P().SphereUsliceOp(16, 0, pad, W16, 0, False), O.SphereUsliceOp(16, 0, pad, W16)
        want = cop.forward(x)[0]
        inner = (lambda t: t[:, :, pad:t.shape[2] - pad, pad:t.shape[3] - pad]) if (pad and op == "slice") else (lambda t: t)
        xg = x.to(DEV)

        def run():
            gop.forward(xg)[0].fill_(float("nan"))    # the op owns its output buffer: every call must write all of it
            return gop.forward(xg)[0].clone()

        monkeypatch.delenv("PCONV_RESAMPLE_ROWS", raising=False)
        assert _native.option("PCONV_RESAMPLE_ROWS") == 2
        plain = run()
        assert torch.equal(inner(plain).cpu(), inner(want))
        for value in OC.RESAMPLE_ROWS:
            monkeypatch.setenv("PCONV_RESAMPLE_ROWS", value)
            assert _native.option("PCONV_RESAMPLE_ROWS") == int(value)
            got = run()                               # (slice writes the interior of a padded stack only)
            assert torch.equal(inner(got), inner(plain)), (op, shape, pad, value, int((inner(got) != inner(plain)).sum()))
    if shape in (OC.RESAMPLE_CASES[0][0], OC.RESAMPLE_CASES[1][0]):
        with P().ordered_backward(True):
            for value in OC.RESAMPLE_ROWS:
                monkeypatch.setenv("PCONV_RESAMPLE_ROWS", value)
                if op == "slice":
                    gop, cop, grad = slice_pair(W16, 1, shape, 5)
                else:
                    gop, cop, grad = uslice_pair(W16, 1, (16 * n, c, height // 16 + 2, width + 2), 6)
                assert torch.equal(gop.backward(grad.to(DEV))[0].cpu(), cop.backward(grad)[0]), (op, shape, value)


# ---- d. the rest ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout,shape", [(192, 96, (16, 34, 1026)), (96, 192, (16, 34, 1026)), (192, 192, (16, 34, 1026)),
                                            (192, 768, (16, 18, 514)), (192, 192, (16, 3, 70)), (96, 96, (2, 5, 7))])
def test_staggered_resident_1x1_equals_unstaggered(cin, cout, shape, hip_backend, monkeypatch):
    """PCONV_CONV1X1_STAGGER = 1 and 3 (the second wave of every SIMD of conv1x1_rb_kernel sleeps before its loop; a wait,
    no arithmetic) on the shapes of test_resident_1x1_equals_tiled_kernel under PCONV_CONV1X1=resident: the outputs of
    the unstaggered launch, and the oracle's fmaf chain on the first rows of tile 0"""
    from pseudocylindrical_convolution_amd import _native
    tn, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(47)
    x = torch.randn(tn, cin, h, w, generator=g, device=DEV)
    wt = torch.randn(cout, cin, 1, 1, generator=g, device=DEV) * (1.0 / np.sqrt(cin))
    b, sl = torch.randn(cout, generator=g, device=DEV), torch.rand(cout, generator=g, device=DEV)
    res = torch.randn(tn, cout, h, w, generator=g, device=DEV)
    limit = torch.tensor([w, (w * 7) // 8, w // 2 + 1, 64, 65, 1, w, 130] * 2, dtype=torch.int32).clamp(max=w).to(DEV)
    owner = type("Owner", (), {})()
    probe = _Probe()
    monkeypatch.setattr(P(), "conv_probe", probe)
    monkeypatch.setenv("PCONV_CONV1X1", "resident")

    def variants():
        _poison(res.shape, 2)
        first = P().tile_conv2d(owner, x, wt, b, 1, sl, limit, 16, residual=res, trim=True, ring=2)
        _poison(res.shape)
        return [first, P().tile_conv2d(owner, x, wt, None, 1, None, limit, 16)]

    monkeypatch.delenv("PCONV_CONV1X1_STAGGER", raising=False)
    assert _native.option("PCONV_CONV1X1_STAGGER") == -1
    plain = variants()
    kept = []
    for value in OC.STAGGER:
        monkeypatch.setenv("PCONV_CONV1X1_STAGGER", value)
        assert _native.option("PCONV_CONV1X1_STAGGER") == int(value) > 0
        kept.append(variants())
        for i, (a, r) in enumerate(zip(plain, kept[-1])):
            assert torch.equal(a, r), "stagger %s, variant %d: %d outputs differ" % (value, i, int((a != r).sum()))
    assert all(r[0].startswith("conv1x1_rb_kernel<") for r in probe.records) and len(probe.records) == 6
    rows = min(h, 3)
    ref = O.conv2d_chain(x[:1, :, :rows].cpu().contiguous(), wt.cpu(), None, 1, None)
    assert torch.equal(plain[1][:1, :, :rows].cpu(), ref)      # tile 0 is live over its whole width


def _batch(ent, n, h, w, seed):
    sym = torch.randint(0, 8, (ent.npart * n, ent.ngroup, h, w), generator=torch.Generator().manual_seed(seed)).float().cuda()
    return ent.fill(sym).contiguous()


def test_clear_every_call_keeps_the_streams(hip_backend, monkeypatch):
    """PCONV_ENGINE_CLEAR_EVERY_CALL=1 (every call starts from zeroed context / activation buffers): batch A, batch B
    and A again through one engine give, call by call, the streams of the default engine, and both decode them"""
    _clean(monkeypatch)
    ent = _net(56)
    h, w, n = 4, 128, 3
    a, b = _batch(ent, n, h, w, 41), _batch(ent, n, h, w, 43)
    plain = _engine(ent, h, w, n)
    monkeypatch.setenv("PCONV_ENGINE_CLEAR_EVERY_CALL", "1")
    clearing = _engine(ent, h, w, n)
    monkeypatch.delenv("PCONV_ENGINE_CLEAR_EVERY_CALL")
    assert (plain.option("PCONV_ENGINE_CLEAR_EVERY_CALL"), clearing.option("PCONV_ENGINE_CLEAR_EVERY_CALL")) == (0, 1)
    first = None
    for k, sym in enumerate((a, b, a)):
        want = plain.encode(sym)
        assert clearing.encode(sym) == want, "call %d" % k
        assert torch.equal(clearing.decode(want), sym) and torch.equal(plain.decode(want), sym), "call %d" % k
        first = want if first is None else first
    assert want == first and plain.encode(b) != first


def test_rate_on_group_streams_gives_the_same_bits(hip_backend, monkeypatch):
    """PCONV_ENGINE_RATE_STREAMS=groups (rate() forks every lock-step group onto its own stream and joins): the float64
    bits and the float32 map of the default engine, on three frames = two groups, for a batch and then for a second one"""
    _clean(monkeypatch)
    ent = _net(56)
    h, w, n = 4, 128, 3
    assert len(_groups(n)) > 1
    plain = _engine(ent, h, w, n)
    monkeypatch.setenv("PCONV_ENGINE_RATE_STREAMS", "groups")
    forked = _engine(ent, h, w, n)
    monkeypatch.delenv("PCONV_ENGINE_RATE_STREAMS")
    assert (plain.option("PCONV_ENGINE_RATE_STREAMS"), forked.option("PCONV_ENGINE_RATE_STREAMS")) == (0, 1)
    seen = []
    for seed in (45, 47):
        sym = _batch(ent, n, h, w, seed)
        shapes = ((n, ent.npart, ent.ngroup), (n, ent.npart * h, w))
        _poison(shapes[0], dtype=torch.float64)
        got = forked.rate(sym)                      # (first, into poisoned memory: nothing holds these figures yet)
        _poison(shapes[0], dtype=torch.float64)
        _poison(shapes[1])
        got_bits, got_map = forked.rate(sym, rate_map=True)
        want = plain.rate(sym)
        want_bits, want_map = plain.rate(sym, rate_map=True)
        torch.cuda.synchronize()
        assert torch.equal(want.view(torch.int64), want_bits.view(torch.int64))
        assert torch.equal(got.view(torch.int64), want.view(torch.int64))
        assert torch.equal(got_bits.view(torch.int64), want.view(torch.int64))
        assert torch.equal(got_map.view(torch.int32), want_map.view(torch.int32))
        assert bool((want > 0).any()) and bool(torch.isfinite(want).all())
        seen.append(want.clone())
    assert not torch.equal(seen[0], seen[1])


@pytest.mark.parametrize("env", OC.REST_SETS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_host_side_engine_options_keep_the_streams(env, hip_backend, monkeypatch):
    """the options that had no row in any GPU test: PCONV_EE_BULK0=valu (the encoder's input layer on the vector kernel),
    PCONV_ENGINE_WORKERS, PCONV_ENGINE_BLOCKING_SYNC and PCONV_ENGINE_SPIN_US (how the host threads of a decode wait)
    and PCONV_ENGINE_TIMING (one stderr line per call): the default engine's streams, decoded to the symbols"""
    names = {"PCONV_EE_BULK0", "PCONV_ENGINE_WORKERS", "PCONV_ENGINE_BLOCKING_SYNC", "PCONV_ENGINE_SPIN_US", "PCONV_ENGINE_TIMING"}
    assert set(env) <= names
    h, w = OC.EE_SHAPE
    n = 3
    ent, sym, ref = _reference(56, n, h, w, 29, monkeypatch)
    _clean(monkeypatch)
    default_forms = _engine(ent, h, w, n).encoder_forms
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = _engine(ent, h, w, n)
    for k, v in env.items():
        assert eng.option(k) == (1 if v == "valu" else int(v)), (env, k)
    if "PCONV_EE_BULK0" in env:
        assert eng.encoder_forms[0] == 0 != default_forms[0] and eng.encoder_forms[1:] == default_forms[1:]
    if "PCONV_ENGINE_BLOCKING_SYNC" in env:
        assert eng.lib.pconv_ee_wait_mode(eng.handle) == 1
    assert eng.encode(sym) == ref
    assert torch.equal(eng.decode(ref), sym)
    assert torch.equal(eng.decode(ref), sym)
