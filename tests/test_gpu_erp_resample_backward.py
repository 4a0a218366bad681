"""GPU: the ordered backward of the sphere-aware resize (csrc/erp_resample_backward.hip,
pconv_erp_resample_backward_f32) bit for bit against its torch twin run on the CPU on the same tables (itself held to a
plain float32 loop in tests/test_erp_resample_backward_cpu.py), erp_resample.resize and the renderer's prefilter
gradient under autograd, and two reproducible optimiser steps of --code-size.

Which edge of the kernels as built each case reaches.  Columns pass: grid (h, ceil(w2 / 1024), n C), a lane owns 4
adjacent columns.  Rows pass: a workgroup takes R = 4 rows x 1024 source columns and stages the gmid columns they reach.
  9x16 -> 5x12        16-byte loads on the entries that did not cross a pole only (w2 // 2 = 6); one ragged row group
  6x10 -> 15x37       4-byte paths, a ragged last quad; the whole gmid row staged; lists of 20 and more entries
  16x32 -> 2x4        T = 48: every output row crosses a pole; the staged span is the whole row of 4
  2x2 -> 5x6          w < T_x, h < T_y: a destination met several times by one row's taps
  4x1100 -> 6x2300    two source tiles in the rows pass (a wrapped span that is not the whole row), three in the columns pass
  5x2300 -> 3x1100    three source tiles in the rows pass, two in the columns pass; 16-byte staging (w2 % 4 == 0)
  8x16 -> 8x16        the identity table: 16-byte loads on all entries (w2 // 2 = 8)"""
import ctypes

import pytest
import torch

import erp_resample_backward_cases as B
from erp_resample_backward_cases import CASES, case_id

pytestmark = pytest.mark.gpu

_cache = {}


def _twin(case, n=None):
    """the CPU twin's result, computed once per (case, batch)"""
    from pseudocylindrical_convolution_amd import erp_resample
    if (case, n) not in _cache:
        _cache[(case, n)] = erp_resample.resize_backward_torch(B.gradient(case, n=n), case[2], case[3])
    return _cache[(case, n)]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernels_are_the_twin(hip_backend, case):
    from pseudocylindrical_convolution_amd import PCONV
    n, c, h, w, h2, w2 = case
    g = B.gradient(case).cuda()
    got = PCONV.erp_resample_backward_f32(g, h, w)
    assert got.shape == (n, c, h, w) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), _twin(case))
    # a gin that held something else is overwritten in full
    gin = torch.full((n, c, h, w), float("nan"), device="cuda")
    assert PCONV.erp_resample_backward_f32(g, h, w, gin).data_ptr() == gin.data_ptr()
    assert torch.equal(gin.cpu(), _twin(case))
    if case == B.IDENTITY:
        assert torch.equal(got.view(torch.int32), g.view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_frame_alone_and_in_a_batch_give_the_same_bits(hip_backend, case):
    from pseudocylindrical_convolution_amd import PCONV
    n, c, h, w, h2, w2 = case
    batch = B.gradient(case, n=3)
    got = PCONV.erp_resample_backward_f32(batch.cuda(), h, w)
    assert torch.equal(got.cpu(), _twin(case, 3))
    alone = PCONV.erp_resample_backward_f32(batch[1:2].contiguous().cuda(), h, w)
    assert torch.equal(alone, got[1:2])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_views_off_the_16_byte_grid_take_the_scalar_paths(hip_backend, case):
    """gradient, result and workspace each one float past a 16-byte boundary: 4-byte accesses, the same bits"""
    from pseudocylindrical_convolution_amd import PCONV, _native
    n, c, h, w, h2, w2 = case
    g = B.gradient(case)
    gbuf = torch.zeros(g.numel() + 1, device="cuda")
    gv = gbuf[1:].view(g.shape)
    gv.copy_(g)
    obuf = torch.full((n * c * h * w + 1,), float("nan"), device="cuda")
    ov = obuf[1:].view(n, c, h, w)
    nbytes = _native.call("pconv_erp_resample_backward_workspace_bytes", n, c, h, w, h2, w2)
    ws = torch.empty(nbytes + 4, dtype=torch.uint8, device="cuda")[4:]
    assert gv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4 and ws.data_ptr() % 16 == 4
    PCONV.erp_resample_backward_f32(gv, h, w, ov, ws)
    assert torch.equal(ov.cpu(), _twin(case))
    assert bool(torch.isnan(obuf[0]))


def test_refusals_come_from_the_host(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, erp_resample, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    lib = _native.hip_lib()
    h, w, h2, w2 = 8, 8, 4, 4
    g = torch.rand(1, 1, h2, w2, device="cuda")
    gin = torch.full((1, 1, h, w), 7.0, device="cuda")
    ws = torch.empty(4 * h * w2, dtype=torch.uint8, device="cuda")
    wx, wy = (erp_resample.taps(a, b)[1].cuda() for a, b in ((w, w2), (h, h2)))
    sx, ex, _ = (t.cuda() for t in erp_resample.reverse_taps(w, w2, 0))
    sy, ey, cy = (t.cuda() for t in erp_resample.reverse_taps(h, h2, 1))
    p = lambda t: t.data_ptr()
    tx, ty = wx.shape[1], wy.shape[1]
    good = [p(g), p(gin), p(ws), p(wx), tx, p(sx), p(ex), p(wy), ty, p(sy), p(ey), p(cy)]
    for k, what in ((0, b"null pointer"), (1, b"null pointer"), (2, b"null pointer"), (3, b"null pointer"), (7, b"null pointer"),
                    (5, b"null list pointer"), (6, b"null list pointer"), (9, b"null list pointer"),
                    (10, b"null list pointer"), (11, b"null list pointer")):
        args = list(good)
        args[k] = None
        assert lib.pconv_erp_resample_backward_f32(*args, 1, 1, h, w, h2, w2, None) == -1
        assert what in lib.pconv_last_error()
    same = list(good)
    same[1] = same[0]
    assert lib.pconv_erp_resample_backward_f32(*same, 1, 1, h, w, h2, w2, None) == -1 and b"distinct" in lib.pconv_last_error()
    for k in (4, 8):
        args = list(good)
        args[k] += 1
        assert lib.pconv_erp_resample_backward_f32(*args, 1, 1, h, w, h2, w2, None) == -1
        assert b"tap counts" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_backward_f32(*good, 1, 1, h, 72, h2, 8, None) == -1 and b"8:1" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_backward_f32(*good, 1, 1, h, w, h2, 1, None) == -1 and b"outside" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_backward_f32(*good, 70000, 1, h, w, h2, w2, None) == -1 and b"planes" in lib.pconv_last_error()
    wide = list(good)
    wide[4] = erp_resample.taps(64, 1 << 15)[1].shape[1]      # 512:1 in width: a tile would gather from the whole row of 2^15
    assert lib.pconv_erp_resample_backward_f32(*wide, 1, 1, h, 64, h2, 1 << 15, None) == -1 and b"exceeds LDS" in lib.pconv_last_error()
    assert lib.pconv_erp_resample_backward_workspace_bytes(0, 1, h, w, h2, w2) == -1
    with pytest.raises(PconvError, match="float32"):
        PCONV.erp_resample_backward_f32(g.double(), h, w)
    with pytest.raises(PconvError, match="contiguous"):
        PCONV.erp_resample_backward_f32(g.expand(1, 1, h2, w2).transpose(2, 3), h, w)
    with pytest.raises(PconvError, match="gin must be"):
        PCONV.erp_resample_backward_f32(g, h, w, torch.empty(1, 1, h, w + 1, device="cuda"))
    with pytest.raises(PconvError, match="8:1"):
        PCONV.erp_resample_backward_f32(g, 40, w)
    torch.cuda.synchronize()
    assert bool((gin == 7.0).all())        # nothing was launched
    assert lib.pconv_erp_resample_backward_f32(*good, 1, 1, h, w, h2, w2, None) == 0
    assert torch.equal(gin.cpu(), erp_resample.resize_backward_torch(g.cpu(), h, w))


def test_resize_under_autograd_is_the_twin_with_and_without_clamp(hip_backend):
    from pseudocylindrical_convolution_amd import erp_resample
    n, c, h, w, h2, w2 = B.CLAMPED
    x = B.frames(B.CLAMPED, seed=3, lo=-0.5, hi=1.5).cuda().requires_grad_()
    g = B.gradient(B.CLAMPED, seed=3)
    for clamp in (False, True):
        x.grad = None
        out = erp_resample.resize(x, h2, w2, clamp=clamp)
        assert out.grad_fn is not None and torch.equal(out.detach(), erp_resample.resize(x.detach(), h2, w2, clamp=clamp))
        out.backward(g.cuda())
        raw = erp_resample.resize(x.detach(), h2, w2).cpu()
        inside = (raw >= 0) & (raw <= 1)
        assert bool(inside.any()) and not bool(inside.all())
        masked = torch.where(inside, g, torch.zeros(())) if clamp else g
        assert torch.equal(x.grad.cpu(), erp_resample.resize_backward_torch(masked, h, w))
    assert erp_resample.resize(x.detach(), h2, w2).grad_fn is None


def test_prefilter_gradient_on_the_gpu_is_the_cpu_gradient(hip_backend):
    """one view on the source as it is, one on a reduced source: two terms, whose float32 sum is commutative"""
    from pseudocylindrical_convolution_amd import viewport
    views = [viewport.view(30, 20, 10, 20, 15), viewport.view(0, 0, 0, 120, 90)]
    gpu = viewport.Renderer(64, 128, views, (4, 6), device="cuda", prefilter_grad=True)
    cpu = viewport.Renderer(64, 128, views, (4, 6), prefilter_grad=True)
    assert gpu.plans == cpu.plans and gpu.plans[0][:2] == (64, 128) and gpu.plans[1][:2] != (64, 128)
    cpu.maps = [q.cpu() for q in gpu.maps]      # the same records on both sides
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(2, 3, 64, 128, generator=gen)
    g = torch.randn(2, 2, 3, 4, 6, generator=gen)
    grads = []
    for r, dev in ((gpu, "cuda"), (cpu, "cpu")):
        xd = x.to(dev).requires_grad_()
        out = r.render(xd, clamp=True)
        assert out.grad_fn is not None and torch.equal(out.detach(), r.render(xd.detach(), clamp=True))
        out.backward(g.to(dev))
        grads.append(xd.grad.cpu())
    assert bool((grads[0] != 0).any()) and torch.equal(grads[0], grads[1])


def _model_steps(monkeypatch):
    """two Adam steps of CMPNetV2M (16 channels) on one 320 x 768 frame coded at 256 x 512, the smallest size the model
    codes, under --deterministic --conv native-all --optim native --loss ws --code-size, the library's convolution
    made to raise"""
    from pseudocylindrical_convolution_amd import model_zoo_v2 as Z, optim, train

    def refuse(*a, **k):
        raise AssertionError("--conv native-all --loss ws --code-size reached torch.nn.functional.conv2d")

    monkeypatch.setattr(torch.nn.functional, "conv2d", refuse)
    args = train.build_parser().parse_args(["--conv", "native-all", "--loss", "ws", "--base", "--optim", "native",
                                            "--deterministic", "--height", "320", "--width", "768", "--code-size", "512x256"])
    torch.manual_seed(0)
    net = Z.CMPNetV2M(8, 16, 16, 16, opt=False, init=False, device_id=0).to("cuda:0")
    net.train()
    params = [p for name, p in net.named_parameters() if name != "quant.count"]
    opt = optim.Adam(params, lr=1e-3)
    x = torch.rand(1, 3, 320, 768, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    with train.native_conv_mode("native-all"), train.deterministic_mode():
        for _ in range(2):
            mse, ssim, _ = train.forward_losses(args, net, x, None, None, train.make_sim_func(args, "cuda:0"))
            opt.zero_grad()
            (mse + 0.1 * (1 - ssim)).backward()
            opt.step(clip=0.1)
    assert opt.last_grad_norm.item() > 0
    return [p.detach().clone() for p in params]


def test_two_steps_with_code_size_give_the_same_bits_twice(hip_backend, monkeypatch):
    a, b = _model_steps(monkeypatch), _model_steps(monkeypatch)
    assert len(a) > 10 and all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    assert all(bool(torch.isfinite(p).all()) for p in a)
