"""GPU: WS-PSNR / WS-SSIM (csrc/sphere_metrics.hip: ms_forward_kernel<T, 1, 1>, ms_close_kernel<1>).  The HIP kernel
against the float64 torch path, the uint8 form bit for bit against frames_u8_to_f32 + the float form, batching and
repeat determinism, the uniform weighting against pytorch_ssim, refused inputs, a codec frame of a non-codable size
scored at its own height, and the command line's --test --ws against the float64 path on the same PNGs."""
import numpy as np
import pytest
import torch

from test_sphere_metrics_cpu import SHAPES, drive_ws, pair

pytestmark = pytest.mark.gpu


def _close(got, want):
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    dpsnr = (S.psnr(got[:, 0]) - S.psnr(want[:, 0])).abs().max().item()
    dssim = (got[:, 1] - want[:, 1]).abs().max().item()
    assert dpsnr <= 1e-4 and dssim <= 1e-5, (dpsnr, dssim)


@pytest.mark.parametrize("shape", SHAPES + [(3, 3, 255, 510), (8, 3, 2048, 4096)])
@pytest.mark.parametrize("weighting", ["ws", "uniform"])
def test_kernel_is_the_float64_path(hip_backend, shape, weighting):
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    x, y = pair(shape, sum(shape) + 1)
    got = S.metrics(x.cuda(), y.cuda(), weighting)
    assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == (shape[0], 2)
    want = S.metrics_torch(x.cuda(), y.cuda(), weighting)   # float64 on the device: the CPU path's definitions
    _close(got, want)
    if shape[0] * shape[2] * shape[3] <= 1 << 20:
        _close(got, S.metrics(x, y, weighting))             # the CPU path itself


@pytest.mark.parametrize("n,h,w", [(1, 7, 13), (2, 64, 128), (3, 250, 500), (2, 37, 51)])
def test_uint8_form_is_bitwise_the_float_form(hip_backend, n, h, w):
    from pseudocylindrical_convolution_amd import PCONV, sphere_metrics as S
    g = torch.Generator().manual_seed(h * w)
    u = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    v = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    if w % 4 == 0:
        fu, fv = PCONV.frames_u8_to_f32(u.cuda()), PCONV.frames_u8_to_f32(v.cuda())
    else:   # img2tensor's arithmetic on the host (frames_u8_to_f32 takes widths % 4 == 0)
        fu, fv = ((t.permute(0, 3, 1, 2).float() / 255.).contiguous().cuda() for t in (u, v))
    for weighting in ("ws", "uniform"):
        a = S.metrics(u.cuda(), v.cuda(), weighting)
        assert torch.equal(a, S.metrics(fu, fv, weighting))
        _close(a, S.metrics(u, v, weighting))


def test_frames_give_the_same_bits_alone_in_a_batch_and_again(hip_backend):
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    x, y = pair((8, 3, 300, 600), 8)
    xc, yc = x.cuda(), y.cuda()
    batch = S.metrics(xc, yc)
    assert torch.equal(batch, S.metrics(xc, yc))
    for i in range(8):
        assert torch.equal(S.metrics(xc[i:i + 1], yc[i:i + 1]), batch[i:i + 1])
    assert torch.equal(S.metrics(xc[5:8].contiguous(), yc[5:8].contiguous()), batch[5:8])


def test_uniform_is_pytorch_ssim_on_the_gpu(hip_backend):
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    from pseudocylindrical_convolution_amd.PCONV_operator import pytorch_ssim
    x, y = pair((3, 3, 512, 1024), 4)
    xc, yc = x.cuda(), y.cuda()
    got = S.ws_ssim(xc, yc, "uniform")
    for i in range(3):
        assert abs(got[i].item() - pytorch_ssim.ssim(xc[i:i + 1], yc[i:i + 1]).item()) <= 1e-5
    assert torch.equal(S.ws_psnr(xc, xc), torch.full((3,), float("inf"), dtype=torch.float64))
    assert torch.allclose(S.ws_ssim(xc, xc), torch.ones(3, dtype=torch.float64), rtol=0, atol=1e-12)


def test_refused_inputs(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd._native import PconvError
    x, y = pair((1, 3, 16, 32), 2)
    xc, yc = x.cuda(), y.cuda()
    u = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device="cuda")
    bad = [
        (x, y),                                                   # CPU tensors
        (xc, y),                                                  # device mix
        (xc, yc.double()),                                        # dtype
        (xc, u),                                                  # dtype mix
        (xc, yc[:, :, :15].contiguous()),                         # shape
        (xc.transpose(2, 3), yc.transpose(2, 3)),                 # not contiguous
        (xc[0], yc[0]),                                           # not a batch
        (u[..., :2].contiguous(), u[..., :2].contiguous()),       # uint8 that is not (n, h, w, 3)
        (xc[:0], yc[:0]),                                         # no frame
    ]
    for a, b in bad:
        with pytest.raises(PconvError):
            PCONV.ws_metrics(a, b)
    with pytest.raises(PconvError):
        PCONV.ws_metrics(xc, yc, "s-psnr")
    assert PCONV.ws_metrics(xc, yc).shape == (1, 2)


def test_codec_frame_of_any_size_is_scored_at_its_own_height(hip_backend):
    from pseudocylindrical_convolution_amd import erp_size, sphere_metrics as S
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    from test_gpu_engine import _codec
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    h, w = 1000, 2000
    assert erp_size.coded_size(h, w)[:2] == (1024, 2000)
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(9)).cuda()
    rec = eng.decode(eng.encode(x), h, w)
    assert rec.shape == (1, 3, h, w)
    got = S.metrics(x, rec)
    _close(got, S.metrics_torch(x, rec))
    # the weights are those of h = 1000 rows, not of the coded 1024
    assert not torch.allclose(got, S.metrics_torch(erp_size.pad(x), erp_size.pad(rec)), rtol=0, atol=1e-9)


@pytest.mark.parametrize("sizes,native", [([(512, 1024)], False), ([(500, 1000)], True)])
def test_cli_ws_on_the_gpu(hip_backend, tmp_path, monkeypatch, capsys, sizes, native):
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    rows, images = drive_ws(tmp_path, monkeypatch, capsys, "cuda:0", sizes, native)
    for row, (src, dec), (h, w) in zip(rows, images, sizes):
        assert src.shape == dec.shape == (h, w, 3)
        m = S.metrics(torch.from_numpy(src)[None], torch.from_numpy(dec)[None])   # the float64 path on the PNGs
        assert abs(row[3] - S.psnr(m[0, 0].item())) <= 1e-4 and abs(row[4] - m[0, 1].item()) <= 1e-5
        assert np.isfinite(row[3])
