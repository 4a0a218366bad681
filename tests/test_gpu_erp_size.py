"""GPU: panoramas of any size.  The three kernels of csrc/erp_size.hip bit for bit against the padding rule
(numpy), the codec on h x w frames against today's path on the padded frames, FramePipe at a size the frame
kernels refuse, and the command line end to end (--native-size)."""
import numpy as np
import pytest
import torch

from test_erp_size_cpu import drive_native_size, numpy_pad

pytestmark = pytest.mark.gpu

SIZES = [(250, 500), (200, 333), (37, 50), (2880, 5760)]


def rule_index(h, w):
    """the rule of include/pconv_hip.h as numpy index arrays: (rows (H,), cols (H, W))"""
    H, W = 256 * ((h + 255) // 256), 16 * ((w + 15) // 16)
    top, m = (H - h) // 2, (W - w + 1) // 2
    y = np.arange(H) - top
    flip = (y < 0) | (y >= h)
    y = np.clip(np.where(y < 0, -1 - y, np.where(y >= h, 2 * h - 1 - y, y)), 0, h - 1)
    xc = np.arange(W)
    x = np.where(xc < w, xc, np.where(xc - w < m, w - 1, 0))
    cols = np.where(flip[:, None], (x[None, :] + w // 2) % w, x[None, :])
    return y, cols


def np_pad(a):
    """(..., h, w) -> (..., H, W)"""
    rows, cols = rule_index(*a.shape[-2:])
    return a[..., rows[:, None], cols]


def test_vectorised_rule_is_the_loop():
    a = np.random.default_rng(0).random((3, 37, 50)).astype(np.float32)
    assert np.array_equal(np_pad(a), numpy_pad(a))


def _u8(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", SIZES)
def test_u8_to_f32_erp_kernel_is_the_rule(hip_backend, n, h, w):
    from pseudocylindrical_convolution_amd import PCONV
    img = _u8(n, h, w, h + w + n)
    # img2tensor's arithmetic, then the rule
    want = np_pad((torch.from_numpy(img.numpy().transpose(0, 3, 1, 2).astype(np.float32)) / 255.).numpy())
    got = PCONV.frames_u8_to_f32_erp(img.cuda()).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    # the image at an odd byte offset of its buffer
    flat = torch.zeros(img.numel() + 1, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(img.shape)
    view.copy_(img.cuda())
    assert view.data_ptr() % 2 == 1
    assert np.array_equal(PCONV.frames_u8_to_f32_erp(view).cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", SIZES)
def test_erp_pad_f32_kernel_is_the_rule(hip_backend, n, h, w):
    from pseudocylindrical_convolution_amd import PCONV, erp_size
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(n * 7 + h))
    got = PCONV.erp_pad_f32(x.cuda())
    assert np.array_equal(got.cpu().numpy(), np_pad(x.numpy()))
    assert torch.equal(erp_size.pad(x.cuda()), got)                     # the package's dispatch


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", SIZES)
def test_f32_to_u8_crop_kernel_is_tensor2img_of_the_crop(hip_backend, n, h, w):
    from pseudocylindrical_convolution_amd import PCONV, erp_size
    H, W, top = erp_size.coded_size(h, w)
    g = torch.Generator().manual_seed(n + w)
    rec = torch.rand(n, 3, H, W, generator=g) * 1.006 - 0.001           # ClipData's leak past [0, 1] included
    want = (rec[..., top:top + h, :w] * 255.).numpy().transpose(0, 2, 3, 1).astype(np.uint8)
    got = PCONV.frames_f32_to_u8_crop(rec.cuda(), h, w).cpu().numpy()
    assert got.shape == (n, h, w, 3) and np.array_equal(got, want)
    flat = torch.full((n * h * w * 3 + 2,), 77, dtype=torch.uint8, device="cuda")
    PCONV.frames_f32_to_u8_crop(rec.cuda(), h, w, out=flat[1:-1].view(n, h, w, 3))
    host = flat.cpu().numpy()
    assert host[0] == 77 and host[-1] == 77                              # nothing written outside the image
    assert np.array_equal(host[1:-1].reshape(n, h, w, 3), want)


def test_kernels_refuse_bad_arguments(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd._native import PconvError
    with pytest.raises(PconvError):
        PCONV.frames_u8_to_f32_erp(torch.zeros((1, 1, 8, 3), dtype=torch.uint8).cuda())     # h < 2
    with pytest.raises(PconvError):
        PCONV.erp_pad_f32(torch.zeros((1, 3, 4, 30000)).cuda())                           # row beyond LDS
    with pytest.raises(PconvError):
        PCONV.frames_f32_to_u8_crop(torch.zeros((1, 3, 250, 512)).cuda(), 250, 500)       # not the coded size


def _codec():
    from test_gpu_engine import _codec as codec
    return codec()


@pytest.mark.parametrize("n,h,w", [(2, 500, 1000), (1, 1920, 3840), (1, 2880, 5760)])
def test_codec_engine_codes_any_size_as_the_padded_frame(hip_backend, n, h, w):
    from pseudocylindrical_convolution_amd import erp_size
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(h))
    padded = torch.from_numpy(np_pad(x.numpy()))
    H, W, top = erp_size.coded_size(h, w)
    streams = eng.encode(x.cuda())
    assert streams == eng.encode(padded.cuda())
    rec = eng.decode(streams, h, w)
    full = eng.decode(streams, H, W)
    assert rec.shape == (n, 3, h, w) and torch.equal(rec, full[:, :, top:top + h, :w])


@pytest.mark.parametrize("h,w,pad", [(500, 1000, True), (250, 333, None)])
def test_frame_pipe_any_size_host_to_host(hip_backend, h, w, pad):
    """pad=True pads any size; the default pads where today's frame kernels refuse the width (333 % 4 != 0)"""
    from pseudocylindrical_convolution_amd import erp_size
    from pseudocylindrical_convolution_amd.engine import FramePipe
    n = 2
    H, W, top = erp_size.coded_size(h, w)
    pipe = FramePipe(n, h, w, "cuda:0", pad=pad)
    assert pipe.coded == (H, W)
    batches = [_u8(n, h, w, 40 + k).pin_memory() for k in range(2)]
    pipe.prefetch(batches[0], 0)
    for k in range(2):
        frames = pipe.take(k)
        if k == 0:
            pipe.prefetch(batches[1], 1)
        want = np_pad((torch.from_numpy(batches[k].numpy().transpose(0, 3, 1, 2).astype(np.float32)) / 255.).numpy())
        assert tuple(frames.shape) == (n, 3, H, W) and np.array_equal(frames.cpu().numpy(), want)
        rec = (frames * 0.5 + 0.25).contiguous()
        pipe.give(rec, k)
        got = pipe.wait(k).numpy()
        assert np.array_equal(got, (rec[..., top:top + h, :w] * 255.).cpu().numpy().transpose(0, 2, 3, 1).astype(np.uint8))


@pytest.mark.parametrize("h,w", [(250, 500), (500, 1000)])
def test_cli_native_size_on_the_gpu(hip_backend, tmp_path, monkeypatch, capsys, h, w):
    drive_native_size(tmp_path, monkeypatch, capsys, h, w, "cuda:0")
