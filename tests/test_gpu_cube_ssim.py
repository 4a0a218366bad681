"""GPU: WS-SSIM of cube pictures (weighted_ssim_kernel of csrc/weighted_metrics.hip on the tile passes of csrc/ssim_tile.h;
cube_pad_f32_kernel of csrc/cube.hip at any depth).  The SSIM kernel computes its map in fp32 and is held to the float64
twin within 1e-5 per plane -- the bound tests/test_gpu_sphere_metrics.py holds the same fp32 map to -- and to the ERP
kernel; the continuation is held to its twin bit for bit.  Then batches and slices, stale memory, the wrappers' operand
contract and the command line.

Which edge of the kernels as built each case reaches.  weighted_ssim_kernel: one workgroup of 256 lanes per tile of 32 rows
x 64 columns and plane, a lane 8 rows of one column, the staged tile 42 x 74 with its halo; weighted_sum_kernel adds a
plane's tile partials.
  1x1       one pixel, one lane adds          7x13      one ragged tile
  33x65     one past a tile both ways: four tiles, three of them one pixel wide or high
  37x51     two tiles down                    250x500   64 tiles, the last of each row and column ragged
  faces of 2, 7, 37, 64 at depth 5: padded faces of 12, 17, 47 and 74 columns, the last two tiles wide for both kernels
"""
import numpy as np
import pytest
import torch

import cube_ssim_cases as SC
import stale_memory as SM
from cube_ssim_cases import KINDS, LAYOUTS, case_id

pytestmark = pytest.mark.gpu

BOUND = 1e-5      # tests/test_gpu_sphere_metrics.py::_close: the fp32 map against float64

_twins = {}


def _twin(key, make):
    """a CPU reference, computed once and shared"""
    if key not in _twins:
        _twins[key] = make()
    return _twins[key]


def _plane(name, h, w):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    return _twin(("plane", name, h, w), lambda: WM.WeightPlane(SC.plane(name, h, w)))


def _pair(shape):
    return _twin(("pair", shape), lambda: SC.pair(*shape))


@pytest.mark.parametrize("name", SC.PLANES)
@pytest.mark.parametrize("shape", SC.SHAPES, ids=case_id)
def test_kernel_is_the_float64_twin(hip_backend, shape, name):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    n, c, h, w = shape
    x, y = _pair(shape)
    wt = _plane(name, h, w)
    want = _twin(("ssim", shape, name), lambda: WM.ssim(x, y, wt))
    got = WM.ssim(x.cuda(), y.cuda(), wt)
    print("%s %s: the kernel is within %.3g of the twin" % (case_id(shape), name, (got - want).abs().max().item()))
    assert got.dtype == torch.float64 and got.device.type == "cpu" and tuple(got.shape) == (n, c)
    assert ((got - want).abs() <= BOUND).all(), (got, want)
    on_device = WM.ssim_device(x.cuda(), y.cuda(), wt)
    assert on_device.is_cuda and SM.same_bits(on_device.cpu(), got)                 # ... and the second call gives the same bits
    assert ((WM.ssim(x.cuda(), x.cuda(), wt) - 1).abs() <= BOUND).all()             # x == y is allowed


@pytest.mark.parametrize("shape", SC.SHAPES, ids=case_id)
def test_kernel_with_the_erp_plane_is_the_erp_kernel(hip_backend, shape):
    from pseudocylindrical_convolution_amd import sphere_metrics, weighted_metrics as WM
    n, c, h, w = shape
    x, y = _pair(shape)
    got = WM.ssim_figure(x.cuda(), y.cuda(), _plane("erp", h, w))
    want = sphere_metrics.metrics(x.cuda(), y.cuda())[:, 1]
    print("%s: the weighted kernel is within %.3g of the ERP kernel" % (case_id(shape), (got - want).abs().max().item()))
    assert ((got - want).abs() <= BOUND).all(), (got, want)


@pytest.mark.parametrize("plane", [(33, 65), (37, 51)], ids=case_id)
def test_a_frame_alone_in_a_batch_and_in_a_slice(hip_backend, plane):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    h, w = plane
    x, y = (t.cuda() for t in SC.pair(5, 3, h, w))
    wt = _plane("band", h, w)
    whole = WM.ssim(x, y, wt)
    assert SM.same_bits(WM.ssim(x, y, wt), whole)                                   # a second call
    for f in range(5):
        assert SM.same_bits(WM.ssim(x[f:f + 1], y[f:f + 1], wt), whole[f:f + 1])    # alone; a contiguous slice at an offset
    assert SM.same_bits(WM.ssim(x[1:4], y[1:4], wt), whole[1:4])
    assert SM.same_bits(WM.ssim(x[2:3].clone(), y[2:3].clone(), wt), whole[2:3])    # alone, in memory of its own


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", SC.GPU_FACES)
def test_continuation_of_depth_5_is_the_twin(hip_backend, kind, a):
    from pseudocylindrical_convolution_amd import PCONV, _metric_ops, cube
    y = SC.frames(2, 3, 6 * a, a, 3)
    depth = cube.SSIM_PAD
    A = a + 2 * depth
    table = torch.from_numpy(np.array(cube.pad_table(kind, a, depth)))
    want = cube.pad_torch(y, table, depth)
    guard = 64
    flat = torch.full((want.numel() + 2 * guard,), 7.0, device="cuda")
    out = flat[guard:guard + want.numel()].view(want.shape)
    got = _metric_ops.cube_pad_depth(y.cuda(), table.cuda(), depth, out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (2, 3, 6 * A, A)
    assert SM.same_bits(got.cpu(), want), "max abs diff %g" % (got.cpu() - want).abs().max().item()
    host = flat.cpu()
    assert (host[:guard] == 7.0).all().item() and (host[-guard:] == 7.0).all().item()
    assert SM.same_bits(cube.pad(y.cuda(), kind, depth).cpu(), want)                 # the public entry: its own cached table
    # depth 3 through the new entry: the bits of pconv_cube_pad_f32
    table3 = cube.pad_table_on(kind, a, "cuda")
    assert SM.same_bits(_metric_ops.cube_pad_depth(y.cuda(), table3, 3), PCONV.cube_pad_f32(y.cuda(), table3))
    const = torch.full((1, 1, 6 * a, a), 0.3, device="cuda")
    assert torch.equal(cube.pad(const, kind, depth), torch.full((1, 1, 6 * A, A), 0.3, device="cuda"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", SC.GPU_FACES)
def test_ws_ssim_on_the_gpu_is_the_cpu_figure(hip_backend, kind, a):
    """... and constant pictures p, q score the closed form.  In the fp32 map a window of constants has mu = p T and
    blur(x^2) = p^2 T, T the two-pass fp32 sum of the taps, so sigma_x^2 = p^2 (T - T^2) and 2 s_xy - s_x^2 - s_y^2 =
    -(p - q)^2 (T - T^2): the map misses the closed form by (p - q)^2 |1 - T| / C2 of its value.  T is 22 fmaf roundings
    of partial sums below 1, and the rounding of the taps in each pass, away from 1: at most 24 * 2^-24 = 1.4e-6, so 1e-5
    holds for (p - q)^2 <= 1e-5 * 9e-4 / 1.4e-6 = 0.0063: p = 1/2 and q = 9/16 are 1/16 apart, (p - q)^2 = 0.0039.
    (p = 1/4, q = 3/4 give 0.6002 for 0.60006 in this map and in the ERP kernel's alike: C2 is small against fp32's
    cancellation in sigma^2.)"""
    from pseudocylindrical_convolution_amd import cube
    x, y = SC.pair(2, 3, 6 * a, a)
    want = _twin(("ws_ssim", kind, a), lambda: cube.ws_ssim_planes(x, y, cube.spec(kind, "faces")))
    p, q = 0.5, 0.5625
    closed = (2 * p * q + SC.C1) / (p * p + q * q + SC.C1)
    for layout in LAYOUTS:
        sp = cube.spec(kind, layout)
        px, py = cube.pack(x, layout).contiguous().cuda(), cube.pack(y, layout).contiguous().cuda()
        got = cube.ws_ssim_planes(px, py, sp)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3) and ((got - want).abs() <= BOUND).all(), (layout, got - want)
        figure = cube.ws_ssim(px, py, sp)
        assert tuple(figure.shape) == (2,) and ((figure - want.mean(dim=1)).abs() <= BOUND).all()
        const = cube.ws_ssim(torch.full_like(px, p), torch.full_like(px, q), sp)
        assert ((const - closed).abs() <= BOUND).all(), (layout, const - closed)
    print("%s a = %d: the GPU figure is within %.3g of the twin" % (kind, a, (got - want).abs().max().item()))


def test_results_do_not_depend_on_what_fresh_memory_held(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import cube
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    x, y = (t.cuda() for t in SC.pair(2, 3, 37, 51))
    wt = _plane("band", 37, 51)
    a = 7
    cx, cy = (t.cuda() for t in SC.pair(2, 3, 6 * a, a))
    results = {}
    for name, regime in SM.regimes(monkeypatch):
        with regime():
            results[name] = [WM.ssim(x, y, wt), cube.pad(cx, "eac", depth=5).cpu(), cube.pad(cx, "cmp", depth=8).cpu(),
                             cube.ws_ssim_planes(cx, cy, cube.spec("eac", "faces"))]
    for name in SM.KINDS:
        assert all(SM.same_bits(a, b) for a, b in zip(results[name], results["plain"])), name


def _forms(t, dim=0):
    """(name, refused form) of a good operand: the wrong type, the wrong device, one short and one more along `dim` (the
    wrong shape), a view that is not contiguous, the same from an offset into its memory, and no tensor at all"""
    wrong = torch.float64 if t.dtype != torch.float64 else torch.float32
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1] + 1,), dtype=t.dtype, device=t.device)
    return [("dtype", t.to(wrong)), ("device", t.cpu()), ("short", t.narrow(dim, 0, t.shape[dim] - 1).contiguous()),
            ("shape", torch.cat([t, t.narrow(dim, 0, 1)], dim=dim)), ("strided", wide[..., :-1:2]), ("offset", wide[..., 1::2]),
            ("no tensor", None)]


def test_every_new_wrapper_refuses_a_bad_operand_before_the_library(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import _metric_ops, _native, cube
    from pseudocylindrical_convolution_amd._native import PconvError
    real, calls = _native.call, []

    def recording(fn, *args):
        calls.append(fn)
        return real(fn, *args)
    monkeypatch.setattr(_native, "call", recording)
    n, c, h, w = 2, 3, 5, 7
    x, y = SC.pair(n, c, h, w)
    ssim = dict(x=x.cuda(), y=y.cuda(), weights=torch.ones(h, w, dtype=torch.float64, device="cuda"))
    a, depth = 4, 5
    A = a + 2 * depth
    pad = dict(x=SC.frames(n, c, 6 * a, a).cuda(), table=cube.pad_table_on("cmp", a, "cuda", depth),
               out=torch.zeros(n, c, 6 * A, A, device="cuda"))
    wrappers = [("weighted_ssim", lambda o: _metric_ops.weighted_ssim_device(o["x"], o["y"], o["weights"], 35.0), ssim, ("x", "y", "weights")),
                ("cube_pad_depth", lambda o: _metric_ops.cube_pad_depth(o["x"], o["table"], depth, o.get("out")), pad, ("x", "table", "out"))]
    checked = 0
    for what, run, operands, names in wrappers:
        run(operands)                                                   # the good call goes through
        assert calls, what
        for name in names:
            for form, bad in _forms(operands[name], 2 if (what, name) == ("cube_pad_depth", "x") else 0):
                if name == "out" and form == "no tensor":
                    continue                                            # (None: a new one is made)
                if name == "x" and form in ("short", "shape", "dtype"):
                    # x defines the shapes: what does not fit it is then named as another operand
                    expect = r"%s: (x|y|table) must be|%s: x: " % (what, what)
                else:
                    expect = r"%s: %s must be" % (what, name)
                del calls[:]
                with pytest.raises(PconvError, match=expect):
                    run(dict(operands, **{name: bad}))
                assert calls == [], (what, name, form, calls)
                checked += 1
    assert checked >= 38
    del calls[:]
    for total in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(PconvError, match="total"):
            _metric_ops.weighted_ssim_device(ssim["x"], ssim["y"], ssim["weights"], total)
    u8 = torch.zeros(n, h, w, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(PconvError, match="weighted_ssim: x must be"):     # no uint8 form
        _metric_ops.weighted_ssim_device(u8, u8, ssim["weights"], 35.0)
    for bad_depth in (0, 9):
        with pytest.raises(PconvError, match="cube_pad_depth: depth must be"):
            _metric_ops.cube_pad_depth(pad["x"], pad["table"], bad_depth)
    with pytest.raises(PconvError, match="cube_pad_depth: table must be"):     # the table of another depth
        _metric_ops.cube_pad_depth(pad["x"], cube.pad_table_on("cmp", a, "cuda"), depth)
    assert calls == []


def test_cli_rd_and_test_with_cube_ssim(hip_backend, tmp_path, monkeypatch, capsys):
    """--rd --projection eac --cube-ssim reports what --test --projection eac --cube-ssim reports of the file: the same
    reconstruction, so the same figure; every other line is what it is without the flag"""
    import re
    import cube_cases as CC
    from pseudocylindrical_convolution_amd import cube, pseudo_codec as PC
    from test_cli import _models
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cuda")
    a = 64
    y = cube.from_erp(CC.smooth(2 * a, 4 * a), a, cube.spec("eac", "3x2"), clamp=True)
    PC.write_image("cube.png", PC.tensor2img(y))
    common = ["--ssim", "--model-idx", "3"]
    rd = ["--rd", "--projection", "eac", "--img-list", "cube.png"] + common
    PC.main(["--enc", "--projection", "eac", "--container", "--img-list", "cube.png", "--code-list", "cube.pcv"] + common)
    test = ["--test", "--projection", "eac", "--code-list", "cube.pcv", "--img-list", "cube.png"]
    outs = {}
    for name, argv in (("rd", rd), ("rd+", rd + ["--cube-ssim"]), ("test", test), ("test+", test + ["--cube-ssim"])):
        capsys.readouterr()
        PC.main(argv)
        outs[name] = capsys.readouterr().out.splitlines()
    new = lambda l: l.lstrip().startswith("CUBE-WS-SSIM:")
    for name in ("rd", "test"):
        assert not any(new(l) for l in outs[name])
        assert [l for l in outs[name + "+"] if not new(l)] == outs[name]
        assert len([l for l in outs[name + "+"] if new(l)]) == 2 and new(outs[name + "+"][-1])       # the image and the average
    figures = lambda lines: re.findall(r"CUBE-WS-SSIM:([0-9.]+)", "\n".join(lines))
    assert len(figures(outs["rd+"])) == 2 and figures(outs["rd+"]) == figures(outs["test+"])
    assert all(0 < float(v) <= 1 for v in figures(outs["rd+"]))
