"""GPU: the sphere rotation of ERP frames (csrc/erp_rotate.hip).  The map kernel against the float64 numpy map (equal:
tests/test_erp_rotate_cpu.py holds the shared cases away from every rounding boundary), the sampler bit for bit against
its torch twin run on the CPU on the same map (itself held to a numpy loop there), and CodecEngine's rotation=.

Which edge of the kernels as built each shape reaches.  Map: 256 columns per workgroup, one row.  Sampler: a workgroup
takes 4 rows x 64 columns, a lane one pixel, and walks the C planes of one frame (grid.y = n).
  32x64      one column tile, exact; 8 row groups
  50x100     ragged in both directions (100 = 64 + 36, 50 = 12 * 4 + 2)
  48x130     three sampler tiles per row, the last of 2 columns
  6x2100     wider than any tile of either kernel (9 map tiles, 33 sampler tiles); every footprint near a pole
  50x99      an odd width: the half turn at the poles is floor(w / 2) = 49
"""
import ctypes

import numpy as np
import pytest
import torch

from erp_rotate_cases import CASES, case_id

pytestmark = pytest.mark.gpu

SAMPLER_CASES = [(2, 3) + CASES[0], (3, 2) + CASES[5], (2, 3) + CASES[10], (1, 1) + CASES[15], (2, 3, 50, 99, (30, 20, 10)),
                 (1, 1, 50, 99, (0, -90, 45))]


def _frames(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255. * 1.5 - 0.25   # some of it outside [0, 1]


_twin_cache = {}


def _twin(case, inverse, clamp):
    """the CPU twin's result on the numpy map, computed once per (case, inverse, clamp)"""
    from pseudocylindrical_convolution_amd import erp_rotate
    key = (case, inverse, clamp)
    if key not in _twin_cache:
        n, c, h, w, angles = case
        q = torch.from_numpy(erp_rotate.source_map_numpy(h, w, erp_rotate.units(*angles), inverse))
        _twin_cache[key] = erp_rotate.rotate_torch(_frames(n, c, h, w), q, clamp)
    return _twin_cache[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_map_kernel_is_the_float64_map(hip_backend, case):
    from pseudocylindrical_convolution_amd import PCONV, erp_rotate
    h, w, angles = case
    rot = erp_rotate.units(*angles)
    for inverse in (False, True):
        got = PCONV.erp_rotation_map(h, w, rot, inverse)
        assert got.dtype == torch.int32 and tuple(got.shape) == (h, w, 2) and got.is_cuda
        want = erp_rotate.source_map_numpy(h, w, rot, inverse)
        diff = got.cpu().numpy() != want
        assert not diff.any(), "%d records differ, first at %s" % (diff.any(2).sum(), np.argwhere(diff.any(2))[:1])
        assert torch.equal(erp_rotate.source_map(h, w, rot, inverse, "cuda"), got)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("case", SAMPLER_CASES, ids=lambda c: "n%dc%d_" % c[:2] + case_id(c[2:]))
def test_sampler_is_the_twin(hip_backend, case, clamp):
    from pseudocylindrical_convolution_amd import PCONV, erp_rotate
    n, c, h, w, angles = case
    rot = erp_rotate.units(*angles)
    x = _frames(n, c, h, w).cuda()
    for inverse in (False, True):
        want = _twin(case, inverse, clamp)
        q = torch.from_numpy(erp_rotate.source_map_numpy(h, w, rot, inverse)).cuda()
        got = PCONV.erp_remap_f32(x, q, clamp).cpu()
        assert got.shape == want.shape == (n, c, h, w)
        assert torch.equal(got, want), "max abs diff %g" % (got - want).abs().max().item()
        if clamp:
            assert got.min().item() >= 0.0 and got.max().item() <= 1.0
        # the public entry: the device's own map
        assert torch.equal(erp_rotate.rotate(x, rot, inverse, clamp).cpu(), want)


@pytest.mark.parametrize("case", [(2, 3, 50, 99, (30, 20, 10)), (2, 3) + CASES[10], (1, 1) + CASES[15]],
                         ids=lambda c: case_id(c[2:]))
def test_nothing_is_left_unwritten_and_nothing_written_outside(hip_backend, case):
    """out and the map start as NaN / a sentinel inside larger buffers: every element of both results is written and
    the guards around them keep their sentinel"""
    from pseudocylindrical_convolution_amd import PCONV, erp_rotate
    n, c, h, w, angles = case
    rot = erp_rotate.units(*angles)
    x = _frames(n, c, h, w).cuda()
    guard, numel = 64, n * c * h * w
    flat = torch.full((numel + 2 * guard,), 77.0, device="cuda")
    out = flat[guard:guard + numel].view(n, c, h, w)
    out.fill_(float("nan"))
    mflat = torch.full((2 * h * w + 2 * guard,), -(1 << 30), dtype=torch.int32, device="cuda")
    q = mflat[guard:guard + 2 * h * w].view(h, w, 2)
    assert PCONV.erp_rotation_map(h, w, rot, False, out=q).data_ptr() == q.data_ptr()
    assert np.array_equal(q.cpu().numpy(), erp_rotate.source_map_numpy(h, w, rot))
    mhost = mflat.cpu()
    assert (mhost[:guard] == -(1 << 30)).all().item() and (mhost[guard + 2 * h * w:] == -(1 << 30)).all().item()
    got = PCONV.erp_remap_f32(x, q, False, out)
    assert got.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any().item()
    assert torch.equal(out.cpu(), _twin(case, False, False))
    host = flat.cpu()
    assert (host[:guard] == 77.0).all().item() and (host[guard + numel:] == 77.0).all().item()


def test_a_frame_gives_the_same_bits_alone_and_in_a_batch(hip_backend):
    from pseudocylindrical_convolution_amd import erp_rotate
    rot = erp_rotate.units(123.25, -33.5, -170)
    x = _frames(3, 3, 50, 99, seed=9).cuda()
    batch = erp_rotate.rotate(x, rot)
    for i in range(3):
        assert torch.equal(erp_rotate.rotate(x[i:i + 1].contiguous(), rot), batch[i:i + 1])
        for ch in range(3):
            assert torch.equal(erp_rotate.rotate(x[i:i + 1, ch:ch + 1].contiguous(), rot), batch[i:i + 1, ch:ch + 1])


def test_refusals_come_from_the_host(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, erp_rotate, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    rot = erp_rotate.units(30, 20, 10)
    x = torch.zeros(1, 1, 8, 16).cuda()
    q = PCONV.erp_rotation_map(8, 16, rot)
    for bad in (x.double(), x[0], x.int()):                                        # wrong dtype or rank
        with pytest.raises(PconvError):
            PCONV.erp_remap_f32(bad, q)
        with pytest.raises(PconvError):
            erp_rotate.rotate(bad, rot)
    with pytest.raises(PconvError, match="GPU tensor"):
        PCONV.erp_remap_f32(x.cpu(), q.cpu())
    for bad_map in (q.long(), q[:4], q.cpu(), q.float()):
        with pytest.raises(PconvError, match="map"):
            PCONV.erp_remap_f32(x, bad_map)
    with pytest.raises(PconvError, match="out must"):
        PCONV.erp_remap_f32(x, q, False, torch.empty(1, 1, 8, 8).cuda())
    with pytest.raises(PconvError, match="distinct"):
        PCONV.erp_remap_f32(x, q, False, x)
    for bad in ((180 << 16, 0, 0), (0, (90 << 16) + 1, 0), (0, 0, (-180 << 16) - 1)):   # an out-of-range angle
        with pytest.raises(PconvError, match="out of range"):
            PCONV.erp_rotation_map(8, 16, bad)
        with pytest.raises(PconvError):
            erp_rotate.rotate(x, bad)
    with pytest.raises(PconvError):
        PCONV.erp_rotation_map(1, 16, rot)                                          # a side of 1
    with pytest.raises(PconvError):
        PCONV.erp_rotation_map(8, 1, rot)
    with pytest.raises(PconvError):
        erp_rotate.rotate(torch.zeros(1, 1, 1, 16).cuda(), rot)
    with pytest.raises(PconvError, match="GPU device"):
        PCONV.erp_rotation_map(8, 16, rot, device="cpu")
    lib = _native.hip_lib()
    table = erp_rotate.phases().cuda()
    out = torch.empty_like(x)
    good = [x.data_ptr(), out.data_ptr(), q.data_ptr(), table.data_ptr()]
    for k in range(4):
        args = list(good)
        args[k] = None
        assert lib.pconv_erp_remap_f32(*args, 1, 1, 8, 16, 0, None) == -1 and b"null pointer" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 1, 1, 1, 16, 0, None) == -1 and b"outside" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 70000, 1, 8, 16, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(good[0] + 2, *good[1:], 1, 1, 8, 16, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert lib.pconv_erp_rotation_map(q.data_ptr(), 8, 16, 180 << 16, 0, 0, 0, None) == -1
    assert b"out of range" in lib.pconv_last_error()
    torch.cuda.synchronize()


def test_exact_permutations(hip_backend):
    """the permutations of tests/test_erp_rotate_cpu.py on the device (180 degrees is written -180: yaw, roll < 180)"""
    from pseudocylindrical_convolution_amd import erp_rotate
    for h, w in ((32, 64), (50, 100), (48, 130)):
        x = _frames(2, 3, h, w).cuda()
        for k in (1, 3, w // 2 - 1, -5):
            rot = erp_rotate.units(k * 360.0 / w, 0, 0)
            assert torch.equal(erp_rotate.rotate(x, rot), torch.roll(x, -k, 3)), (h, w, k)
            assert torch.equal(erp_rotate.rotate(x, rot, inverse=True), torch.roll(x, k, 3)), (h, w, k)
    for h, w in ((32, 64), (50, 100)):
        x = _frames(2, 3, h, w).cuda()
        half = erp_rotate.units(-180, 0, -180)
        assert torch.equal(erp_rotate.rotate(x, half), torch.roll(x.flip(2, 3), w // 2, 3))
    assert erp_rotate.rotate(x, None) is x


def _codec():
    from test_gpu_engine import _codec as codec
    return codec()


def test_codec_engine_codes_in_a_rotated_orientation(hip_backend):
    from pseudocylindrical_convolution_amd import erp_rotate
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    r = erp_rotate.units(40, -60.5, 15)
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 256, (2, 3, 256, 512), generator=g).float() / 255.).cuda()
    turned = erp_rotate.rotate(x, r, clamp=True)
    streams = eng.encode(x, rotation=r)
    assert streams == eng.encode(turned)
    plain = eng.decode(streams, 256, 512)
    want = erp_rotate.rotate(plain, r, inverse=True, clamp=True)
    got = eng.decode(streams, 256, 512, rotation=r)
    assert got.shape == (2, 3, 256, 512) and torch.equal(got, want)
    bits, rec = eng.evaluate(x, rotation=r)
    assert torch.equal(rec, want)
    assert torch.equal(bits, eng.rate(turned)) and torch.equal(bits, eng.rate(x, rotation=r))
    # None and zeros change nothing
    assert eng.encode(turned, rotation=None) == streams == eng.encode(turned, rotation=(0, 0, 0))
    assert torch.equal(eng.decode(streams, 256, 512, rotation=None), plain)


def test_codec_engine_rotates_resizes_and_pads_in_that_order(hip_backend):
    """300 x 600 frames coded at 250 x 500, a size that needs the pad: rotate -> resize -> pad on the way in, crop ->
    resize -> rotate back on the way out, each call against the explicit composition"""
    from pseudocylindrical_convolution_amd import erp_resample, erp_rotate, erp_size
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    r = erp_rotate.units(40, -60.5, 15)
    g = torch.Generator().manual_seed(4)
    x = (torch.randint(0, 256, (2, 3, 300, 600), generator=g).float() / 255.).cuda()
    coded = erp_size.pad(erp_resample.resize(erp_rotate.rotate(x, r, clamp=True), 250, 500, clamp=True))
    assert coded.shape == (2, 3, 256, 512)
    streams = eng.encode(x, code_size=(250, 500), rotation=r)
    assert streams == eng.encode(coded)
    want = erp_rotate.rotate(erp_resample.resize(erp_size.crop(eng.decode(streams, 256, 512), 250, 500), 300, 600, clamp=True),
                             r, inverse=True, clamp=True)
    got = eng.decode(streams, 250, 500, out_size=(300, 600), rotation=r)
    assert got.shape == (2, 3, 300, 600) and torch.equal(got, want)
    assert torch.equal(eng.evaluate(x, code_size=(250, 500), rotation=r)[1], want)
