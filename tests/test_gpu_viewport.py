"""GPU: rectilinear viewports of ERP frames (csrc/viewport.hip).  The map kernel against the float64 numpy map (equal:
tests/test_viewport_cpu.py holds the shared cases away from every rounding boundary), the renderer bit for bit against
its torch twin run on the CPU on the same map (itself held to a numpy loop there), the strided write into one slot of a
view stack, CodecEngine.decode_views and the metrics.

Which edge of the kernels as built each case reaches.  Map: 256 grid columns per workgroup, one row.  Renderer: a
workgroup takes 4 rows x 64 columns of the view, a lane one pixel, its ss x ss records and the C planes of one frame
(grid.y = n).
  32x64 -> 9x15 ss1       one tile, exact
  50x99 -> 37x70 ss2      an odd source width (the half turn at the poles is 49), every footprint at a pole, a ragged
                          tile in both directions (70 = 64 + 6, 37 = 9 * 4 + 1)
  6x2100 -> 5x300 ss1     wider than any tile of either kernel (2 map tiles, 5 renderer tiles)
  32x64 -> 37x70 ss3      an inexact scale, float32(1 / 9)
  50x99 -> 9x15 ss4       sixteen records per pixel
  50x99 -> 5x300 ss2      600 grid columns: three map tiles
"""
import numpy as np
import pytest
import torch

from viewport_cases import CASES, case_id

pytestmark = pytest.mark.gpu

U = 1 << 16
BATCHES = [(2, 3), (1, 1), (3, 2)]


def _frames(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255. * 1.5 - 0.25   # some of it outside [0, 1]


_cache = {}


def _map(case):
    """the float64 numpy map of a case, computed once"""
    from pseudocylindrical_convolution_amd import viewport
    if case not in _cache:
        h, w, vh, vw, ss, angles = case
        _cache[case] = torch.from_numpy(viewport.source_map_numpy(h, w, vh * ss, vw * ss, viewport.view(*angles)))
    return _cache[case]


def _twin(case, n, c, clamp):
    """the CPU twin's result on the numpy map, computed once per (case, n, c); the clamp applied to a copy"""
    from pseudocylindrical_convolution_amd import viewport
    key = (case, n, c)
    if key not in _cache:
        h, w, vh, vw, ss, _ = case
        _cache[key] = viewport.render_torch(_frames(n, c, h, w), _map(case), vh, vw, ss, False)
    return _cache[key].clamp(0.0, 1.0) if clamp else _cache[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_map_kernel_is_the_float64_map(hip_backend, case):
    from pseudocylindrical_convolution_amd import PCONV, viewport
    h, w, vh, vw, ss, angles = case
    v = viewport.view(*angles)
    got = PCONV.viewport_map(h, w, vh * ss, vw * ss, v)
    assert got.dtype == torch.int32 and tuple(got.shape) == (vh * ss, vw * ss, 2) and got.is_cuda
    diff = got.cpu() != _map(case)
    assert not diff.any().item(), "%d records differ, first at %s" % (diff.any(2).sum(), diff.any(2).nonzero()[:1])
    assert torch.equal(viewport.source_map(h, w, vh * ss, vw * ss, v, "cuda"), got)


@pytest.mark.parametrize("n,c", BATCHES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_renderer_is_the_twin(hip_backend, case, n, c):
    from pseudocylindrical_convolution_amd import PCONV
    h, w, vh, vw, ss, _ = case
    x = _frames(n, c, h, w).cuda()
    assert x.min().item() < 0.0 and x.max().item() > 1.0
    q = _map(case).cuda()
    for clamp in (False, True):
        want = _twin(case, n, c, clamp)
        got = PCONV.viewport_render_f32(x, q, vh, vw, ss, clamp)
        assert got.shape == (n, 1, c, vh, vw)
        got = got[:, 0].cpu()
        assert torch.equal(got, want), "max abs diff %g" % (got - want).abs().max().item()
        if clamp:
            assert got.min().item() >= 0.0 and got.max().item() <= 1.0


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[4]], ids=case_id)
def test_a_view_goes_into_its_slot_and_nowhere_else(hip_backend, case):
    """slot k of an (n, V, C, vh, vw) buffer through the frame stride: the slot starts as NaN and is written in full, the
    other slots and 64-element guards on either side keep their sentinel; the map inside guards as well"""
    from pseudocylindrical_convolution_amd import PCONV, viewport
    h, w, vh, vw, ss, angles = case
    n, c, views, guard = 2, 3, 3, 64
    x = _frames(n, c, h, w).cuda()
    gh, gw = vh * ss, vw * ss
    mflat = torch.full((2 * gh * gw + 2 * guard,), -(1 << 30), dtype=torch.int32, device="cuda")
    q = mflat[guard:guard + 2 * gh * gw].view(gh, gw, 2)
    assert PCONV.viewport_map(h, w, gh, gw, viewport.view(*angles), out=q).data_ptr() == q.data_ptr()
    assert torch.equal(q.cpu(), _map(case))
    mhost = mflat.cpu()
    assert (mhost[:guard] == -(1 << 30)).all().item() and (mhost[guard + 2 * gh * gw:] == -(1 << 30)).all().item()
    numel = n * views * c * vh * vw
    want = _twin(case, n, c, False)
    for k in range(views):
        flat = torch.full((numel + 2 * guard,), 77.0, device="cuda")
        out = flat[guard:guard + numel].view(n, views, c, vh, vw)
        out[:, k] = float("nan")
        assert PCONV.viewport_render_f32(x, q, vh, vw, ss, False, out, k).data_ptr() == out.data_ptr()
        host = flat.cpu()
        assert not torch.isnan(host).any().item()
        stack = host[guard:guard + numel].view(n, views, c, vh, vw)
        assert torch.equal(stack[:, k], want)
        others = [s for s in range(views) if s != k]
        assert (stack[:, others] == 77.0).all().item()
        assert (host[:guard] == 77.0).all().item() and (host[guard + numel:] == 77.0).all().item()


def test_a_frame_gives_the_same_bits_alone_and_in_a_batch(hip_backend):
    from pseudocylindrical_convolution_amd import viewport
    v = viewport.view(123.25, -33.5, -170, 100.5, 40)
    x = _frames(3, 3, 50, 99, seed=9).cuda()
    r = viewport.Renderer(50, 99, [v], (37, 70), ss=3, device="cuda")
    batch = r.render(x)
    for i in range(3):
        assert torch.equal(r.render(x[i:i + 1].contiguous()), batch[i:i + 1])
        for ch in range(3):
            assert torch.equal(r.render(x[i:i + 1, ch:ch + 1].contiguous()), batch[i:i + 1, :, ch:ch + 1])


def test_renderer_on_the_device_is_the_twin(hip_backend):
    """viewport.Renderer with the device's own maps: explicit ss, plan's ss and plan's prefilter, against the CPU
    renderer (the twin on numpy's maps; the prefilter's resize has its own bit-exact twin)"""
    from pseudocylindrical_convolution_amd import viewport
    x = _frames(2, 3, 50, 99, seed=3)
    views = [viewport.view(*case[5]) for case in CASES[:4]]
    for size, ss in (((9, 15), 2), ((37, 70), None), ((5, 6), None)):
        gpu = viewport.Renderer(50, 99, views, size, ss, "cuda")
        cpu = viewport.Renderer(50, 99, views, size, ss)
        assert gpu.plans == cpu.plans and all(q.is_cuda for q in gpu.maps)
        for clamp in (False, True):
            got = gpu.render(x.cuda(), clamp)
            assert got.is_cuda and got.shape == (2, 4, 3) + size
            assert torch.equal(got.cpu(), cpu.render(x, clamp))
        one = viewport.render(x.cuda(), views[2], size, ss, clamp=True)
        assert torch.equal(one.cpu(), cpu.render(x, True)[:, 2])
    assert any(p[:2] != (50, 99) for p in cpu.plans)          # 5x6 views of 120 degrees: the reduced source
    out = torch.full((2, 4, 3, 5, 6), float("nan"), device="cuda")
    assert gpu.render(x.cuda(), out=out) is out and torch.equal(out.cpu(), cpu.render(x))


def test_refusals_come_from_the_host(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, viewport, erp_rotate, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    v = viewport.view(30, 20, 10, 90, 67.5)
    x = torch.zeros(1, 1, 8, 16).cuda()
    q = PCONV.viewport_map(8, 16, 8, 12, v)
    for bad in (x.double(), x[0], x.int(), x.cpu()):
        with pytest.raises(PconvError):
            PCONV.viewport_render_f32(bad, q, 4, 6, 2)
    for bad_map in (q.long(), q[:4], q.cpu(), q.float()):
        with pytest.raises(PconvError, match="map"):
            PCONV.viewport_render_f32(x, bad_map, 4, 6, 2)
    with pytest.raises(PconvError, match="map"):
        PCONV.viewport_render_f32(x, q, 4, 6, 1)
    with pytest.raises(PconvError, match="ss"):
        PCONV.viewport_render_f32(x, q, 4, 6, 5)
    with pytest.raises(PconvError, match="out must"):
        PCONV.viewport_render_f32(x, q, 4, 6, 2, False, torch.empty(1, 2, 1, 4, 4).cuda())
    with pytest.raises(PconvError, match="slot"):
        PCONV.viewport_render_f32(x, q, 4, 6, 2, False, torch.empty(1, 2, 1, 4, 6).cuda(), 2)
    with pytest.raises(PconvError, match="GPU device"):
        PCONV.viewport_map(8, 16, 8, 12, v, device="cpu")
    for bad in ((180 * U, 0, 0, U, U), (0, 0, 0, U - 1, U), (0, 0, 0, U, 170 * U + 1)):
        with pytest.raises(PconvError, match="out of range"):
            PCONV.viewport_map(8, 16, 8, 12, bad)
    with pytest.raises(PconvError):
        PCONV.viewport_map(1, 16, 8, 12, v)
    with pytest.raises(PconvError):
        PCONV.viewport_map(8, 16, 1, 12, v)
    with pytest.raises(PconvError):
        viewport.Renderer(8, 16, [v], (4, 6), device="cuda").render(x.cpu())
    # the C ABI, each refusal with its message
    lib = _native.hip_lib()
    render = lib.pconv_viewport_render_f32
    table = erp_rotate.phases().cuda()
    out = torch.empty(1, 1, 1, 4, 6).cuda()
    good = [x.data_ptr(), out.data_ptr(), q.data_ptr(), table.data_ptr()]
    for k in range(4):
        args = list(good)
        args[k] = None
        assert render(*args, 1, 1, 8, 16, 4, 6, 2, 24, 0, None) == -1 and b"null pointer" in lib.pconv_last_error()
    assert render(good[0] + 2, *good[1:], 1, 1, 8, 16, 4, 6, 2, 24, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert render(good[0], good[1], good[2] + 4, good[3], 1, 1, 8, 16, 4, 6, 2, 24, 0, None) == -1
    assert b"aligned" in lib.pconv_last_error()
    assert render(*good, 1, 1, 1, 16, 4, 6, 2, 24, 0, None) == -1 and b"source side" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, (1 << 20) + 1, 4, 6, 2, 24, 0, None) == -1 and b"source side" in lib.pconv_last_error()
    assert render(*good, 1, 1, 1 << 15, 1 << 14, 4, 6, 2, 24, 0, None) == -1 and b"source plane" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 16, 1, 6, 2, 6, 0, None) == -1 and b"view side" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 16, 4, 6, 0, 24, 0, None) == -1 and b"supersampling" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 16, 4, 6, 5, 24, 0, None) == -1 and b"supersampling" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 16, 1 << 13, 1 << 13, 2, 1 << 26, 0, None) == -1 and b"map of" in lib.pconv_last_error()
    assert render(*good, 1, 16, 8, 16, 1 << 13, 1 << 12, 1, 1 << 29, 0, None) == -1 and b"output frame" in lib.pconv_last_error()
    assert render(*good, 70000, 1, 8, 16, 4, 6, 2, 24, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert render(*good, 0, 1, 8, 16, 4, 6, 2, 24, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 16, 4, 6, 2, 23, 0, None) == -1 and b"stride" in lib.pconv_last_error()
    assert render(good[0], good[0], good[2], good[3], 1, 1, 8, 16, 4, 6, 2, 24, 0, None) == -1
    assert b"distinct" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(q.data_ptr(), 8, 16, 8, 12, 180 * U, 0, 0, U, U, None) == -1
    assert b"out of range" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(q.data_ptr(), 8, 16, 8, 12, 0, 0, 0, 171 * U, U, None) == -1
    assert b"field of view" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(q.data_ptr() + 4, 8, 16, 8, 12, 0, 0, 0, U, U, None) == -1 and b"aligned" in lib.pconv_last_error()
    torch.cuda.synchronize()


def _codec():
    from test_gpu_engine import _codec as codec
    return codec()


def test_codec_engine_decodes_to_views(hip_backend):
    from pseudocylindrical_convolution_amd import erp_rotate, viewport
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 256, (2, 3, 256, 512), generator=g).float() / 255.).cuda()
    size = (43, 64)
    r = viewport.Renderer(256, 512, viewport.paper_views(size)[::5], size, device="cuda")
    assert r.ss == 3 and len(r.views) == 3
    streams = eng.encode(x)
    frames, views = eng.decode_views(streams, 256, 512, r)
    assert torch.equal(frames, eng.decode(streams, 256, 512))
    assert views.is_cuda and views.shape == (2, 3, 3, 43, 64) and torch.equal(views, r.render(frames, clamp=True))
    assert views.min().item() >= 0.0 and views.max().item() <= 1.0
    # in a rotated orientation: the views are those of the picture turned back
    rot = erp_rotate.units(40, -60.5, 15)
    streams = eng.encode(x, rotation=rot)
    frames, views = eng.decode_views(streams, 256, 512, r, rotation=rot)
    assert torch.equal(frames, eng.decode(streams, 256, 512, rotation=rot))
    assert torch.equal(views, r.render(frames, clamp=True))
    # at a reduced size: the views are those of the picture at the source's size
    x = (torch.randint(0, 256, (1, 3, 300, 600), generator=g).float() / 255.).cuda()
    r = viewport.Renderer(300, 600, viewport.paper_views(size)[::5], size, device="cuda")
    streams = eng.encode(x, code_size=(256, 512))
    frames, views = eng.decode_views(streams, 256, 512, r, out_size=(300, 600))
    assert frames.shape == (1, 3, 300, 600) and torch.equal(frames, eng.decode(streams, 256, 512, out_size=(300, 600)))
    assert torch.equal(views, r.render(frames, clamp=True))
    with pytest.raises(viewport.PconvError):
        eng.decode_views(streams, 256, 512, r)                # the renderer was built for 300 x 600


def test_metrics_on_the_device_are_those_of_cpu_copies(hip_backend):
    """the tolerance of tests/test_gpu_sphere_metrics.py for the uniform weighting: 1e-4 dB and 1e-5"""
    from pseudocylindrical_convolution_amd import sphere_metrics as S, viewport
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 64, 128, generator=g)
    y = (x + 0.05 * torch.randn(2, 3, 64, 128, generator=g)).clamp(0, 1)
    size = (21, 32)
    views = viewport.paper_views(size)
    got = viewport.metrics(viewport.Renderer(64, 128, views, size, device="cuda"), x.cuda(), y.cuda())
    want = viewport.metrics(viewport.Renderer(64, 128, views, size), x, y)
    assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == (2, 2)
    dpsnr = (S.psnr(got[:, 0]) - S.psnr(want[:, 0])).abs().max().item()
    dssim = (got[:, 1] - want[:, 1]).abs().max().item()
    print("viewport metrics: dPSNR %.3g dB, dSSIM %.3g" % (dpsnr, dssim))
    assert dpsnr <= 1e-4 and dssim <= 1e-5, (dpsnr, dssim)
    same = viewport.metrics(viewport.Renderer(64, 128, views, size, device="cuda"), x.cuda(), x.cuda())
    assert torch.equal(same[:, 0], torch.zeros(2, dtype=torch.float64)) and (same[:, 1] - 1).abs().max().item() <= 1e-12
