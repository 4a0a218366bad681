"""GPU: the sphere-aware Lanczos-3 resize (csrc/erp_resample.hip) bit for bit against its torch twin run on the CPU
(erp_resample.resize_torch, itself held to a numpy loop in test_erp_resample_cpu.py), and CodecEngine's code_size /
out_size.

Which edge of the kernels as built each shape reaches.  Rows pass: a workgroup takes R rows x 1024 output columns, R = 4
while 4 staged spans fit 64 KiB of LDS (ratios up to about 3.9), 2 up to about 7.9, else 1; the span is staged with
16-byte loads where w % 4 == 0, else 4-byte loads.  Columns pass: 1024 columns per workgroup, 4 per lane; mode 2 (16-byte
loads on every row) where w2 % 4 == 0 and (w2 // 2) % 4 == 0, mode 1 (4-byte loads on rows that crossed a pole) where
only w2 % 4 == 0, mode 0 (4-byte accesses, ragged last quad) otherwise.
  48x96 -> 24x48     R = 4, 16-byte staging, wrapped halo on both sides of the one tile; columns mode 2
  40x64 -> 64x96     enlarging (T = 6, several lanes per source sample); mode 2
  50x70 -> 33x45     4-byte staging (w % 4 = 2), odd w2: mode 0 with a ragged last quad, unaligned rows
  64x128 -> 8x16     T = 48 on both axes, R = 1
  4x32 -> 6x48       poles in every output row (the clamp after the reflection included), mode 2 on turned rows
  6x5000 -> 6x2500   three column tiles, the last ragged (452); mode 1
  6x2500 -> 6x5001   five column tiles, the last ragged (905), 2500 -> 5001 has no short period; mode 0
  48x96 -> 48x96     identity (five taps, one of them 1)
  24x48 -> 96x192    4:1 enlarging
added, because no shape above reaches them:
  7x20 -> 5x12       n = C = 1: 7 rows leave the last group of R = 4 ragged; mode 1 with real pole taps (w2 // 2 = 6)
  5x80 -> 4x16       n = C = 1: ratio 5, R = 2 with a ragged last group
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH_SHAPES = [(48, 96, 24, 48), (40, 64, 64, 96), (50, 70, 33, 45), (64, 128, 8, 16), (4, 32, 6, 48),
                (6, 5000, 6, 2500), (6, 2500, 6, 5001)]
SINGLE_SHAPES = [(48, 96, 48, 96), (24, 48, 96, 192), (7, 20, 5, 12), (5, 80, 4, 16)]
CASES = [(2, 3) + s for s in BATCH_SHAPES] + [(1, 1) + s for s in SINGLE_SHAPES]


def _frames(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255.


_twin_cache = {}


def _twin(case, clamp):
    """the CPU twin's result, computed once per (case, clamp)"""
    from pseudocylindrical_convolution_amd import erp_resample
    if (case, clamp) not in _twin_cache:
        n, c, h, w, h2, w2 = case
        _twin_cache[(case, clamp)] = erp_resample.resize_torch(_frames(n, c, h, w), h2, w2, clamp)
    return _twin_cache[(case, clamp)]


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%dc%d_%dx%d_to_%dx%d" % c)
def test_kernels_are_the_twin(hip_backend, case, clamp):
    from pseudocylindrical_convolution_amd import erp_resample
    n, c, h, w, h2, w2 = case
    want = _twin(case, clamp)
    got = erp_resample.resize(_frames(n, c, h, w).cuda(), h2, w2, clamp=clamp).cpu()
    assert got.shape == want.shape == (n, c, h2, w2)
    assert torch.equal(got, want), "max abs diff %g" % (got - want).abs().max().item()
    if clamp:
        assert got.min().item() >= 0.0 and got.max().item() <= 1.0
    if (h, w) == (h2, w2):
        assert torch.equal(got, _frames(n, c, h, w))


@pytest.mark.parametrize("case", [(2, 3, 50, 70, 33, 45), (2, 3, 6, 5000, 6, 2500), (2, 3, 64, 128, 8, 16)],
                         ids=lambda c: "%dx%d_to_%dx%d" % c[2:])
def test_nothing_is_left_unwritten_and_nothing_written_outside(hip_backend, case):
    """out and the workspace start as NaN: every element of the result is written; the guards around `out` and behind
    the workspace keep their sentinel"""
    from pseudocylindrical_convolution_amd import PCONV, _native
    n, c, h, w, h2, w2 = case
    x = _frames(n, c, h, w).cuda()
    guard, numel = 64, n * c * h2 * w2
    flat = torch.full((numel + 2 * guard,), 77.0, device="cuda")
    out = flat[guard:guard + numel].view(n, c, h2, w2)
    out.fill_(float("nan"))
    nbytes = _native.call("pconv_erp_resample_workspace_bytes", n, c, h, w, h2, w2)
    assert nbytes == 4 * n * c * h * w2
    wsf = torch.full((nbytes // 4 + guard,), float("nan"), device="cuda")
    wsf[nbytes // 4:] = 77.0
    got = PCONV.erp_resample_f32(x, h2, w2, False, out, wsf.view(torch.uint8))
    assert got.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any().item()
    assert torch.equal(out.cpu(), _twin(case, False))
    host = flat.cpu()
    assert (host[:guard] == 77.0).all().item() and (host[guard + numel:] == 77.0).all().item()
    assert not torch.isnan(wsf[:nbytes // 4]).any().item() and (wsf[nbytes // 4:] == 77.0).all().item()


def test_a_frame_gives_the_same_bits_alone_and_in_a_batch(hip_backend):
    from pseudocylindrical_convolution_amd import erp_resample
    x = _frames(3, 3, 50, 70, seed=9).cuda()
    batch = erp_resample.resize(x, 33, 45)
    for i in range(3):
        assert torch.equal(erp_resample.resize(x[i:i + 1].contiguous(), 33, 45), batch[i:i + 1])


def test_refusals_come_from_the_host(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, erp_resample, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    with pytest.raises(PconvError, match="8:1"):
        PCONV.erp_resample_f32(torch.zeros(1, 1, 4, 90).cuda(), 4, 10)              # 9:1
    with pytest.raises(PconvError):
        erp_resample.resize(torch.zeros(1, 1, 4, 90).cuda(), 4, 10)
    with pytest.raises(PconvError):
        PCONV.erp_resample_f32(torch.zeros(1, 1, 1, 8).cuda(), 2, 8)                # a side of 1
    with pytest.raises(PconvError):
        PCONV.erp_resample_f32(torch.zeros(1, 1, 8, 8).cuda(), 8, 1)
    with pytest.raises(PconvError, match="GPU tensor"):
        PCONV.erp_resample_f32(torch.zeros(1, 1, 8, 8), 4, 4)                       # a CPU tensor
    lib = _native.hip_lib()
    x = torch.zeros(1, 1, 8, 8).cuda()
    fx, wx = (t.cuda() for t in erp_resample.taps(8, 4))
    good = [x.data_ptr(), x.data_ptr(), x.data_ptr(), fx.data_ptr(), wx.data_ptr(), 12, fx.data_ptr(), wx.data_ptr(), 12]
    for k in (0, 1, 2, 3, 4, 6, 7):
        args = list(good)
        args[k] = None
        assert lib.pconv_erp_resample_f32(*args, 1, 1, 8, 8, 4, 4, 0, None) == -1
        assert b"null pointer" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_f32(*good, 1, 1, 8, 72, 4, 8, 0, None) == -1 and b"8:1" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_f32(*good, 1, 1, 8, 8, 4, 1, 0, None) == -1 and b"outside" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_f32(*good, 70000, 1, 8, 8, 4, 4, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    taps = ctypes.c_int()
    assert lib.pconv_host_lanczos_taps(90, 10, None, None, ctypes.addressof(taps)) == -1
    torch.cuda.synchronize()


def _codec():
    from test_gpu_engine import _codec as codec
    return codec()


def test_codec_engine_codes_at_a_reduced_size(hip_backend):
    from pseudocylindrical_convolution_amd import erp_resample
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 256, (2, 3, 512, 1024), generator=g).float() / 255.).cuda()
    small = erp_resample.resize(x, 256, 512, clamp=True)
    streams = eng.encode(x, code_size=(256, 512))
    assert streams == eng.encode(small)
    rec_small = eng.decode(streams, 256, 512)
    want = erp_resample.resize(rec_small, 512, 1024, clamp=True)
    got = eng.decode(streams, 256, 512, out_size=(512, 1024))
    assert got.shape == (2, 3, 512, 1024) and torch.equal(got, want)
    bits, rec = eng.evaluate(x, code_size=(256, 512))
    assert torch.equal(rec, want)
    assert torch.equal(bits, eng.rate(small))
    # None changes nothing
    assert eng.encode(small, code_size=None) == streams
    assert torch.equal(eng.decode(streams, 256, 512, out_size=None), rec_small)


def test_codec_engine_resizes_and_pads_together(hip_backend):
    """code_size = 250 x 500, a size the codec does not take as it is: 300 x 600 frames are resized, then padded to
    256 x 512, and come back by the crop, then the resize -- each call against the explicit composition"""
    from pseudocylindrical_convolution_amd import erp_resample, erp_size
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    g = torch.Generator().manual_seed(4)
    x = (torch.randint(0, 256, (2, 3, 300, 600), generator=g).float() / 255.).cuda()
    coded = erp_size.pad(erp_resample.resize(x, 250, 500, clamp=True))
    assert coded.shape == (2, 3, 256, 512)
    streams = eng.encode(x, code_size=(250, 500))
    assert streams == eng.encode(coded)
    want = erp_resample.resize(erp_size.crop(eng.decode(streams, 256, 512), 250, 500), 300, 600, clamp=True)
    got = eng.decode(streams, 250, 500, out_size=(300, 600))
    assert got.shape == (2, 3, 300, 600) and torch.equal(got, want)
    assert torch.equal(eng.evaluate(x, code_size=(250, 500))[1], want)
