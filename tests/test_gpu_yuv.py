"""GPU: YUV 4:2:0 frames.  The two kernels of csrc/yuv.hip bit for bit (torch.equal) against the torch statement of the
definition in pseudocylindrical_convolution_amd/yuv.py (itself held to a per-pixel loop in tests/test_yuv_cpu.py), for
all three formats; FramePipe(pix_fmt=...) host to host; ws_psnr_yuv."""
import functools

import pytest
import torch

from test_yuv_cpu import random_frames

pytestmark = pytest.mark.gpu

FORMATS = ["yuv420p", "nv12", "yuv420p10le"]
# (h, w): the smallest sizes at which each part of the kernels can go wrong
SIZES = [
    (2, 2),        # the wrap neighbour is the sample itself; the coded frame is all pad
    (4, 6),        # w/2 odd: the column parity flips across the poles
    (6, 10),       # 90-byte frames: the second frame starts 2-mod-4
    (256, 32),     # codable: no pad
    (258, 1030),   # two rows into the next 256-row block, more than one pass of 256 lanes x 4, ragged ends
]
DEFAULT = ("bt709", "limited")
# both matrices and both ranges at one size, the defaults elsewhere
CASES = [(h, w) + DEFAULT for h, w in SIZES] + [(6, 10, "bt709", "full"), (6, 10, "bt601", "limited"), (6, 10, "bt601", "full")]


@functools.lru_cache(maxsize=None)
def source(n, h, w, fmt):
    """seeded frame buffers; 10-bit ones hold 0, 1023 and samples above 1023 (taken modulo 1024) in every plane"""
    from pseudocylindrical_convolution_amd import yuv
    buf = random_frames(n, h, w, fmt, seed=h * 31 + w + n)
    if fmt == "yuv420p10le":
        wide = buf.to(torch.int32)
        for plane in yuv.plane_views_of(wide, h, w, fmt):
            flat = plane.reshape(n, -1)      # (a copy for nv12 only, which is 8-bit)
            flat[:, 0], flat[:, -1] = 0, 1023
            if flat.shape[1] > 3:
                flat[:, 1], flat[:, 2] = 1024 + 77, 65535
        buf = wide.to(torch.uint16)
    return buf


@functools.lru_cache(maxsize=None)
def twin_rgb(n, h, w, fmt, matrix, rng):
    from pseudocylindrical_convolution_amd import yuv
    return yuv.to_rgb(source(n, h, w, fmt), h, w, fmt, matrix, rng)


@functools.lru_cache(maxsize=None)
def reconstruction(n, h, w):
    """a coded-size tensor in [0, 1] with the exact ends in it"""
    from pseudocylindrical_convolution_amd import erp_size
    H, W, top = erp_size.coded_size(h, w)
    x = torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(h + 3 * w + n))
    x[:, :, top, 0], x[:, :, top + h - 1, w - 1] = 0.0, 1.0
    return x


@functools.lru_cache(maxsize=None)
def twin_frames(n, h, w, fmt, matrix, rng):
    from pseudocylindrical_convolution_amd import yuv
    return yuv.from_rgb(reconstruction(n, h, w), h, w, fmt, matrix, rng)


def at_offset(t, offset):
    """a copy of the CPU tensor t on the GPU, `offset` elements into a buffer filled with 77; returns (view, buffer)"""
    flat = torch.full((t.numel() + offset + 1,), 77, dtype=torch.int32).to(t.dtype).cuda()
    view = flat[offset:offset + t.numel()].view(t.shape)
    view.copy_(t.cuda())
    return view, flat


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w,matrix,rng", CASES)
def test_ingest_kernel_is_the_definition(hip_backend, h, w, matrix, rng, fmt, n):
    from pseudocylindrical_convolution_amd import PCONV, erp_size, yuv
    buf, want = source(n, h, w, fmt), twin_rgb(n, h, w, fmt, matrix, rng)
    got = PCONV.frames_yuv420_to_f32(buf.cuda(), h, w, fmt, matrix, rng)
    assert tuple(got.shape) == (n, 3) + erp_size.coded_size(h, w)[:2] and torch.equal(got.cpu(), want)
    assert torch.equal(yuv.to_rgb(buf.cuda(), h, w, fmt, matrix, rng), got)          # the package's dispatch
    # the frames at the odd offsets of a buffer that the element size allows
    for offset in (1, 3):
        view, _ = at_offset(buf, offset)
        assert view.data_ptr() % (2 * view.element_size()) == view.element_size()
        assert torch.equal(PCONV.frames_yuv420_to_f32(view, h, w, fmt, matrix, rng).cpu(), want)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w,matrix,rng", CASES)
def test_egress_kernel_is_the_definition(hip_backend, h, w, matrix, rng, fmt, n):
    from pseudocylindrical_convolution_amd import PCONV, yuv
    x, want = reconstruction(n, h, w).cuda(), twin_frames(n, h, w, fmt, matrix, rng)
    got = PCONV.frames_f32_to_yuv420(x, h, w, fmt, matrix, rng)
    assert got.dtype == yuv.dtype(fmt) and torch.equal(got.cpu(), want)
    assert torch.equal(yuv.from_rgb(x, h, w, fmt, matrix, rng).cpu(), want)          # the package's dispatch
    for offset in (1, 3):
        view, flat = at_offset(torch.zeros_like(want), offset)
        PCONV.frames_f32_to_yuv420(x, h, w, fmt, matrix, rng, out=view)
        host = flat.cpu()
        assert torch.equal(host[offset:-1].view(want.shape), want)
        assert (host[:offset].to(torch.int32) == 77).all() and int(host[-1]) == 77   # nothing written outside the frames


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(4, 6), (258, 1030)])
def test_ingest_is_the_pad_of_the_converted_frame(hip_backend, h, w, fmt):
    from pseudocylindrical_convolution_amd import PCONV, yuv
    buf = source(3, h, w, fmt)
    plain = yuv.to_rgb_torch(buf, h, w, fmt, pad=False)
    assert tuple(plain.shape) == (3, 3, h, w)
    assert torch.equal(PCONV.erp_pad_f32(plain.cuda()), PCONV.frames_yuv420_to_f32(buf.cuda(), h, w, fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(6, 10), (258, 1030)])
def test_egress_reads_the_crop_only(hip_backend, h, w, fmt):
    from pseudocylindrical_convolution_amd import PCONV, erp_size
    H, W, top = erp_size.coded_size(h, w)
    x = torch.full((3, 3, H, W), float("nan"))
    x[:, :, top:top + h, :w] = reconstruction(3, h, w)[:, :, top:top + h, :w]
    assert torch.equal(PCONV.frames_f32_to_yuv420(x.cuda(), h, w, fmt).cpu(), twin_frames(3, h, w, fmt, *DEFAULT))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("matrix,rng", [DEFAULT, ("bt601", "full")])
def test_egress_clamps_values_outside_the_unit_range(hip_backend, fmt, matrix, rng):
    from pseudocylindrical_convolution_amd import PCONV, erp_size, yuv
    h, w = 6, 10
    H, W, top = erp_size.coded_size(h, w)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(2, 3, H, W, generator=g) * 3 - 1                       # [-1, 2)
    x[0, :, top, :6] = torch.tensor([[-1., 2., -1., 2., 0., 1.], [2., -1., -1., 2., 1., 0.], [-1., -1., 2., 2., 1., 1.]])
    want = yuv.from_rgb(x, h, w, fmt, matrix, rng)
    assert torch.equal(want, yuv.from_rgb(x.clamp(0, 1), h, w, fmt, matrix, rng))
    assert torch.equal(PCONV.frames_f32_to_yuv420(x.cuda(), h, w, fmt, matrix, rng).cpu(), want)


def test_kernels_refuse_bad_arguments(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    lib = _native.hip_lib()
    good = torch.zeros((1, 36), dtype=torch.uint8).cuda()
    coded = torch.zeros((1, 3, 256, 16)).cuda()
    assert tuple(PCONV.frames_yuv420_to_f32(good, 4, 6, "yuv420p").shape) == (1, 3, 256, 16)
    with pytest.raises(PconvError, match="even"):
        PCONV.frames_yuv420_to_f32(torch.zeros((1, 45), dtype=torch.uint8).cuda(), 5, 6, "yuv420p")     # odd height
    with pytest.raises(PconvError, match="even"):
        PCONV.frames_f32_to_yuv420(coded, 4, 5, "nv12")                                                # odd width
    with pytest.raises(PconvError, match="unknown"):
        PCONV.frames_yuv420_to_f32(good, 4, 6, "yuv444p")
    with pytest.raises(PconvError, match="unknown"):
        PCONV.frames_f32_to_yuv420(coded, 4, 6, "yuv420p", matrix="bt2020")
    with pytest.raises(PconvError, match="GPU tensor"):
        PCONV.frames_yuv420_to_f32(good.cpu(), 4, 6, "yuv420p")
    with pytest.raises(PconvError, match="GPU tensor"):
        PCONV.frames_f32_to_yuv420(coded.cpu(), 4, 6, "yuv420p")
    with pytest.raises(PconvError):
        PCONV.frames_yuv420_to_f32(good, 4, 6, "yuv420p10le")                                          # uint8 for 10 bits
    with pytest.raises(PconvError):
        PCONV.frames_f32_to_yuv420(torch.zeros((1, 3, 256, 32)).cuda(), 4, 6, "yuv420p")               # not the coded size
    # a float tensor that is 4 bytes off a 16-byte boundary: refused by the library, on the host
    flat = torch.zeros(coded.numel() + 1).cuda()
    skew = flat[1:].view(coded.shape)
    assert skew.data_ptr() % 16 == 4 and skew.is_contiguous()
    with pytest.raises(PconvError, match="16-byte aligned"):
        PCONV.frames_yuv420_to_f32(good, 4, 6, "yuv420p", out=skew)
    with pytest.raises(PconvError, match="16-byte aligned"):
        PCONV.frames_f32_to_yuv420(skew, 4, 6, "yuv420p")
    # straight at the C ABI: null pointers, sizes, the frame count, the width the LDS staging holds, the enums
    a, b = good.data_ptr(), coded.data_ptr()
    for args in ((None, b, 1, 4, 6, 0, 0, 0), (a, None, 1, 4, 6, 0, 0, 0), (a, b, 1, 3, 6, 0, 0, 0), (a, b, 1, 4, 0, 0, 0, 0),
                 (a, b, 65536, 4, 6, 0, 0, 0), (a, b, 0, 4, 6, 0, 0, 0), (a, b, 1, 4, 11522, 0, 0, 0),
                 (a, b, 1, 4, 6, 3, 0, 0), (a, b, 1, 4, 6, 0, 2, 0), (a, b, 1, 4, 6, 0, 0, -1), (a + 1, b, 1, 4, 6, 2, 0, 0)):
        assert lib.pconv_frames_yuv420_to_f32(*args, None) == -1 and b"frames_yuv420_to_f32" in lib.pconv_last_error()
        swapped = (args[1], args[0]) + args[2:]
        assert lib.pconv_frames_f32_to_yuv420(*swapped, None) == -1 and b"frames_f32_to_yuv420" in lib.pconv_last_error()
    torch.cuda.synchronize()
    assert not good.any() and not coded.any() and not flat.any()     # nothing was launched on them


def test_frame_pipe_yuv_host_to_host(hip_backend):
    """FramePipe(pix_fmt=...) at 250x500 around the codec with random weights: take() is the twin's padded conversion,
    what comes back through give() / wait() is from_rgb of the reconstruction; without pix_fmt the pipe hands out today's
    tensors"""
    from test_gpu_engine import _codec
    from pseudocylindrical_convolution_amd import erp_size, yuv
    from pseudocylindrical_convolution_amd.engine import CodecEngine, FramePipe
    from pseudocylindrical_convolution_amd._native import PconvError
    n, h, w = 2, 250, 500
    H, W, top = erp_size.coded_size(h, w)
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    for fmt, matrix, rng in (("yuv420p10le", "bt709", "limited"), ("nv12", "bt601", "full")):
        pipe = FramePipe(n, h, w, "cuda:0", pix_fmt=fmt, matrix=matrix, range=rng)
        assert pipe.coded == (H, W)
        batches = [random_frames(n, h, w, fmt, seed=50 + k).pin_memory() for k in range(2)]
        with pytest.raises(PconvError):
            pipe.prefetch(torch.zeros((n, h, w, 3), dtype=torch.uint8), 0)
        pipe.prefetch(batches[0], 0)
        for k in range(2):
            frames = pipe.take(k)
            if k == 0:
                pipe.prefetch(batches[1], 1)
            assert tuple(frames.shape) == (n, 3, H, W)
            assert torch.equal(frames.cpu(), yuv.to_rgb(batches[k], h, w, fmt, matrix, rng))
            rec = eng.decode(eng.encode(frames), H, W)
            host = pipe.give(rec, k)
            assert host.is_pinned() and host.dtype == yuv.dtype(fmt) and tuple(host.shape) == (n, yuv.frame_elems(h, w))
            assert torch.equal(pipe.wait(k), yuv.from_rgb(rec.cpu(), h, w, fmt, matrix, rng))
    plain = FramePipe(n, h, w, "cuda:0", pad=True)
    img = torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(60), dtype=torch.uint8).pin_memory()
    plain.prefetch(img, 0)
    assert torch.equal(plain.take(0), hip_backend.frames_u8_to_f32_erp(img.cuda()))


def test_ws_psnr_yuv_on_the_gpu(hip_backend):
    from pseudocylindrical_convolution_amd import sphere_metrics, yuv
    h, w = 250, 500
    for fmt in FORMATS:
        a, b = random_frames(2, h, w, fmt, seed=70).cuda(), random_frames(2, h, w, fmt, seed=71).cuda()
        got = yuv.ws_psnr_yuv(a, b, h, w, fmt)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3)
        peak = float((1 << yuv.depth(fmt)) - 1)
        pa, pb = yuv.plane_views(a.cpu(), h, w, fmt), yuv.plane_views(b.cpu(), h, w, fmt)
        for c in range(3):
            p, q = ((yuv._codes(t[c], fmt).float() / peak)[:, None].contiguous().cuda() for t in (pa, pb))
            want = sphere_metrics.ws_psnr(p, q)
            assert torch.isfinite(want).all() and ((got[:, c] - want).abs() <= 1e-9 * want.abs()).all()
        assert torch.isinf(yuv.ws_psnr_yuv(a, a, h, w, fmt)).all() and (yuv.ws_psnr_yuv(a, a, h, w, fmt) > 0).all()
