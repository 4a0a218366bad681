"""Sphere-weighted quality of ERP images: WS-PSNR (Sun, Lu, Yu, IEEE SPL 2017) and its SSIM form, WS-SSIM.

Row j of an h-row ERP frame covers an area of the sphere proportional to w_j = cos(((j + 0.5)/h - 0.5)·pi);
weighting="uniform" sets every w_j = 1 (plain PSNR / SSIM over the ERP grid).  Per frame, with N = C·w·Σ_j w_j:
  WS-MSE  = Σ_c Σ_j Σ_i w_j·(x - y)² / N     (difference and square in fp32, sums in fp64)
  WS-PSNR = 10·log10(1 / WS-MSE) dB          (peak 1.0, as psnr_f; +inf for identical frames)
  WS-SSIM = Σ_c Σ_j Σ_i w_j·ssim_map / N     (pytorch_ssim's map: 11-tap Gaussian, sigma 1.5, zero padding of 5 on
                                             all four borders, so the seam is not wrapped; C1 = 0.01², C2 = 0.03²)
Inputs are two batches of the same shape: float32 (n, C, h, w) as the codec holds them (not clamped), or uint8
(n, h, w, 3) as read_image / FramePipe hold them, each value read as float(u8) / 255 (img2tensor's arithmetic).

GPU tensors go to the HIP kernel of csrc/sphere_metrics.hip (PCONV.ws_metrics: one fused pass over the frames,
fp32 map, fp64 sums, no atomics).  CPU tensors go to the float64 torch implementation below, which the oracle
backend and the CPU tests use; like erp_size's torch gather it is not a fallback for GPU tensors.

As a training loss: loss_terms(x, y) gives the same [WS-MSE, WS-SSIM] per frame on the inputs' device and attached
to autograd.  For GPU tensors its backward is one more HIP kernel (PCONV.ws_metrics_backward: a gather, no atomics,
the upstream gradients read on the device).  include/pconv_hip.h states the gradient; backward_torch is the same
statement in torch.  With blur the zero-padded g⊗g filter (its own transpose), x the other picture, y the picture
that receives the gradient, and gm, gs the frame's upstream gradients:
  mux = blur(x)  muy = blur(y)  sx2 = blur(x²) - mux²  sy2 = blur(y²) - muy²  sxy = blur(xy) - mux·muy
  A1 = 2·mux·muy + C1   A2 = 2·sxy + C2   B1 = mux² + muy² + C1   B2 = sx2 + sy2 + C2   S = A1·A2 / (B1·B2)
  b = -S / B2      c = 2·A1 / (B1·B2)      a = 2·mux·A2 / (B1·B2) - 2·muy·S / B1 - mux·c - 2·muy·b
  ks_j = gs·w_j / N      km_j = 2·gm·w_j / N
  dL/dy = blur(ks·a) + 2·y·blur(ks·b) + x·blur(ks·c) + km·(y - x)
Both metrics are symmetric: the gradient with respect to x is the same with x and y swapped.

WS-MS-SSIM (the second half of this module; include/pconv_hip.h states it in full): five scales of 2x2 means (`pool`),
v_s the weighted mean of cs = A2 / B2 at scales 0-3 and of the full map at scale 4, each with the row weights of a frame
of that scale's height, and WS-MS-SSIM = Π max(v_s, 0)^β_s (`BETAS`).  ms_metrics / ws_ms_ssim score, ms_loss_terms is
the autograd entry, ms_scales_torch and ms_backward_torch are the torch statements the same kernels, launched once per
scale, are held to.  Frames of at least 16 x 16.
"""
import math

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from ._native import PconvError
from .PCONV_operator import backend

WEIGHTINGS = ("ws", "uniform")
WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def weights(h, weighting="ws"):
    """float64 (h,) row weights: cos(((j + 0.5)/h - 0.5)·pi), or ones for "uniform" """
    if weighting not in WEIGHTINGS:
        raise ValueError("weighting must be one of %s, got %r" % (WEIGHTINGS, weighting))
    if weighting == "uniform":
        return torch.ones(h, dtype=torch.float64)
    j = torch.arange(h, dtype=torch.float64)
    # (j + 0.5)/h - 0.5 with an exact integer numerator: rows j and h-1-j get the same weight bit for bit
    return torch.cos((2 * j + 1 - h) / (2.0 * h) * math.pi)


def _as_planes(t):
    """the batch as float32 (n, C, h, w), as the kernel reads it"""
    if t.dim() != 4:
        raise PconvError("sphere metrics: 4-D batches expected, got %s" % (tuple(t.shape),))
    if t.dtype == torch.uint8 and t.shape[3] == 3:
        return (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    if t.dtype == torch.float32:
        return t
    raise PconvError("sphere metrics: float32 (n, C, h, w) or uint8 (n, h, w, 3) expected, got %s %s"
                     % (t.dtype, tuple(t.shape)))


def gaussian():
    """the normalised 11-tap Gaussian of pytorch_ssim (sigma 1.5) as float64 python numbers"""
    g = [math.exp(-(k - WINDOW // 2) ** 2 / (2 * SIGMA ** 2)) for k in range(WINDOW)]
    return [v / sum(g) for v in g]


def _blur(t, g):
    """t (..., h, w) filtered by the window g⊗g with zero padding of 5 on all four borders: two passes of shifted
    sums, in t's dtype and on its device"""
    h, w = t.shape[-2:]
    p = F.pad(t, (WINDOW // 2,) * 4)
    rows = sum(g[k] * p[..., :, k:k + w] for k in range(WINDOW))
    return sum(g[k] * rows[..., k:k + h, :] for k in range(WINDOW))


def _check(x, y, weighting, what="sphere metrics", min_side=0):
    if weighting not in WEIGHTINGS:
        raise ValueError("weighting must be one of %s, got %r" % (WEIGHTINGS, weighting))
    if x.dtype != y.dtype or x.shape != y.shape or x.device != y.device:
        raise PconvError("%s: the two batches differ: %s %s %s vs %s %s %s"
                         % (what, x.device, x.dtype, tuple(x.shape), y.device, y.dtype, tuple(y.shape)))
    if x.dim() != 4:
        raise PconvError("%s: 4-D batches expected, got %s" % (what, tuple(x.shape)))
    h, w = (x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:])
    if h < min_side or w < min_side:
        raise PconvError("%s: h and w must be at least %d, got %dx%d" % (what, min_side, w, h))


def _row_weights(t, weighting):
    """the row weights of t (n, C, h, w) as float64 (1, 1, h, 1) on its device, and N = C·w·Σ_j w_j"""
    _, c, h, w = t.shape
    wr = weights(h, weighting).to(t.device)
    return wr.view(1, 1, h, 1), c * w * float(wr.sum())


def _moments(x, y, g):
    """mux, muy, A2 = 2·sxy + C2, B2 = sx2 + sy2 + C2 and the squares they are made of, in x's dtype"""
    mux, muy = _blur(x, g), _blur(y, g)
    mux_sq, muy_sq, mux_muy = mux * mux, muy * muy, mux * muy
    s1, s2, s12 = _blur(x * x, g) - mux_sq, _blur(y * y, g) - muy_sq, _blur(x * y, g) - mux_muy
    return mux, muy, mux_sq, muy_sq, mux_muy, 2 * s12 + C2, s1 + s2 + C2


def _ssim_map(moments, full):
    """the full map l·cs, or cs = A2 / B2 alone, from _moments' tuple"""
    _, _, mux_sq, muy_sq, mux_muy, A2, B2 = moments
    return ((2 * mux_muy + C1) * A2) / ((mux_sq + muy_sq + C1) * B2) if full else A2 / B2


def _terms_torch(a, b, weighting):
    """float64 (n, 2) [WS-MSE, WS-SSIM] of float32 (n, C, h, w) batches on their device, differentiable: the
    definitions above in float64 torch"""
    wr, norm = _row_weights(a, weighting)
    e2 = ((a - b) * (a - b)).double()
    ssim_map = _ssim_map(_moments(a.double(), b.double(), gaussian()), True)
    return torch.stack([(e2 * wr).sum(dim=(1, 2, 3)) / norm, (ssim_map * wr).sum(dim=(1, 2, 3)) / norm], dim=1)


def metrics_torch(x, y, weighting="ws"):
    """float64 (n, 2) [WS-MSE, WS-SSIM]: the definitions above in float64 torch, on the batches' device (the CPU
    path of `metrics`, and the reference the GPU tests compare the kernel with)"""
    _check(x, y, weighting)
    return _terms_torch(_as_planes(x), _as_planes(y), weighting).cpu()


def metrics(x, y, weighting="ws"):
    """float64 CPU tensor (n, 2): [:, 0] WS-MSE, [:, 1] WS-SSIM of each frame; the HIP kernel for GPU tensors,
    the float64 torch path for CPU tensors"""
    if weighting not in WEIGHTINGS:
        raise ValueError("weighting must be one of %s, got %r" % (WEIGHTINGS, weighting))
    if x.is_cuda or y.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "ws_metrics"):
            raise PconvError("sphere metrics: the active backend has no ws_metrics kernel for a GPU tensor")
        return ops.ws_metrics(x, y, weighting)
    return metrics_torch(x, y, weighting)


def psnr(mse):
    """10·log10(1 / mse), +inf for mse == 0 (elementwise on a float64 tensor, or a float)"""
    if torch.is_tensor(mse):
        return torch.where(mse > 0, 10 * torch.log10(1. / mse), torch.full_like(mse, math.inf))
    return 10 * math.log10(1. / mse) if mse > 0 else math.inf


def ws_psnr(x, y, weighting="ws"):
    """float64 (n,) WS-PSNR in dB of each frame"""
    return psnr(metrics(x, y, weighting)[:, 0])


def ws_ssim(x, y, weighting="ws"):
    """float64 (n,) WS-SSIM of each frame"""
    return metrics(x, y, weighting)[:, 1]


class _WsTerms(torch.autograd.Function):
    """[WS-MSE, WS-SSIM] per frame of GPU tensors: the forward kernel, and its backward kernel once per input that
    needs a gradient"""

    @staticmethod
    def forward(ctx, x, y, weighting, ops):
        ctx.save_for_backward(x, y)
        ctx.weighting, ctx.ops = weighting, ops
        return ops.ws_metrics_device(x, y, weighting)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        gout = gout.contiguous()
        gx = ctx.ops.ws_metrics_backward(y, x, gout, ctx.weighting) if ctx.needs_input_grad[0] else None
        gy = ctx.ops.ws_metrics_backward(x, y, gout, ctx.weighting) if ctx.needs_input_grad[1] else None
        return gx, gy, None, None


def loss_terms(x, y, weighting="ws"):
    """float64 (n, 2) [WS-MSE, WS-SSIM] of each frame, on the inputs' device and attached to autograd: the values
    of `metrics`, as a loss.  x, y: float (n, C, h, w) batches of one shape (uint8 carries no gradient and is
    refused).  GPU tensors (float32, contiguous or made so): the HIP kernel forward, the HIP kernel backward.  CPU
    tensors: the float64 torch statement, differentiated by torch"""
    _check(x, y, weighting, "sphere loss")
    if not x.is_floating_point():
        raise PconvError("sphere loss: float (n, C, h, w) batches expected (uint8 frames carry no gradient), got %s %s"
                         % (x.dtype, tuple(x.shape)))
    if x.is_cuda:
        if x.dtype != torch.float32:
            raise PconvError("sphere loss: float32 GPU tensors expected, got %s" % x.dtype)
        ops = backend.ops()
        if not (hasattr(ops, "ws_metrics_device") and hasattr(ops, "ws_metrics_backward")):
            raise PconvError("sphere loss: the active backend has no ws_metrics kernels for a GPU tensor")
        return _WsTerms.apply(x.contiguous(), y.contiguous(), weighting, ops)
    return _terms_torch(x, y, weighting)


def _coefficients(moments, full):
    """(a, b, c) of the module's head from _moments' tuple: the derivatives of the full map with respect to muy,
    blur(y²) and blur(xy), or (full=False) those of cs = A2 / B2 alone"""
    mux, muy, mux_sq, muy_sq, mux_muy, A2, B2 = moments
    if full:
        A1, B1 = 2 * mux_muy + C1, mux_sq + muy_sq + C1
        D = B1 * B2
        S = (A1 * A2) / D
        b = -S / B2
        c = (2 * A1) / D
        a = (2 * mux) * A2 / D - (2 * muy) * S / B1 - mux * c - (2 * muy) * b
    else:
        S = A2 / B2
        b = -S / B2
        c = 2 / B2
        a = (-mux * c) - (2 * muy) * b
    return a, b, c


def _own(x, y, k, abc, g):
    """a scale's own gradient with respect to y: (blur(k·a) + (2y)·blur(k·b)) + x·blur(k·c)"""
    a, b, c = abc
    return (_blur(k * a, g) + (2 * y) * _blur(k * b, g)) + x * _blur(k * c, g)


def backward_torch(x, y, gout, weighting="ws", dt=torch.float64):
    """the gradient of Σ_f gout[f, 0]·WS-MSE_f + gout[f, 1]·WS-SSIM_f with respect to y, by the explicit formula of
    the module's head, in torch: the statement the HIP kernel is held to.  x, y (n, C, h, w); gout (n, 2).  ks and km
    are formed in float64 and rounded once to dt; everything else runs in dt, operation by operation in the kernel's
    order (the 11-tap sums as shifted sums, k-ascending, horizontal pass first).  Returns dt (n, C, h, w)"""
    if x.shape != y.shape or x.dim() != 4 or tuple(gout.shape) != (x.shape[0], 2):
        raise PconvError("sphere loss: (n, C, h, w) batches of one shape and gout (n, 2) expected, got %s %s %s"
                         % (tuple(x.shape), tuple(y.shape), tuple(gout.shape)))
    n = x.shape[0]
    wr, norm = _row_weights(x, weighting)
    gout = gout.detach().double().to(x.device)
    ks = (gout[:, 1].view(n, 1, 1, 1) * wr / norm).to(dt)
    km = (2.0 * gout[:, 0].view(n, 1, 1, 1) * wr / norm).to(dt)
    x, y = x.detach().to(dt), y.detach().to(dt)
    g = gaussian()
    return _own(x, y, ks, _coefficients(_moments(x, y, g), True), g) + km * (y - x)


# ---- WS-MS-SSIM: five scales of 2x2 means, cs at scales 0-3 and the full map at scale 4 (include/pconv_hip.h) ----
BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # Wang, Simoncelli, Bovik 2003
SCALES, MIN_SIDE = len(BETAS), 1 << (len(BETAS) - 1)


def pool(t):
    """the next scale of t (..., h, w): ((p00 + p01) + (p10 + p11))·0.25 over 2x2 blocks in t's dtype, in this order;
    an odd last row or column belongs to no block and is dropped"""
    h, w = t.shape[-2] // 2 * 2, t.shape[-1] // 2 * 2
    t = t[..., :h, :w]
    return ((t[..., 0::2, 0::2] + t[..., 0::2, 1::2]) + (t[..., 1::2, 0::2] + t[..., 1::2, 1::2])) * 0.25


def ms_scales_torch(x, y, weighting="ws", dt=torch.float64):
    """(n, 5) [v_0..v_4] in dtype dt on the batches' device, differentiable: v_s the weighted mean of cs (s < 4) or
    of the full SSIM map (s = 4) of the s-th scale, with the row weights of an (h >> s)-row frame.  x, y: float
    (n, C, h, w) or uint8 (n, h, w, 3), h, w >= 16"""
    _check(x, y, weighting, min_side=MIN_SIDE)
    a, b = (_as_planes(t) if t.dtype == torch.uint8 else t for t in (x, y))
    a, b = a.to(dt), b.to(dt)
    g, vs = gaussian(), []
    for s in range(SCALES):
        wr, norm = _row_weights(a, weighting)
        m = _ssim_map(_moments(a, b, g), s == SCALES - 1)
        vs.append(((m.double() * wr).sum(dim=(1, 2, 3)) / norm).to(dt))
        if s < SCALES - 1:
            a, b = pool(a), pool(b)
    return torch.stack(vs, dim=1)


def ms_product(v):
    """WS-MS-SSIM (n,) of float64 (n, 5) scale values: Π max(v_s, 0)^β_s for s ascending; 0 for a frame with any
    v_s <= 0, with a zero (not a NaN) gradient there"""
    positive = v > 0
    p = torch.where(positive, v, torch.ones_like(v))
    ms = p[:, 0] ** BETAS[0]
    for s in range(1, SCALES):
        ms = ms * p[:, s] ** BETAS[s]
    return torch.where(positive.all(dim=1), ms, torch.zeros_like(ms))


def _ms_terms_torch(a, b, weighting):
    """float64 (n, 2) [WS-MSE, WS-MS-SSIM] of float (n, C, h, w) batches on their device, differentiable"""
    wr, norm = _row_weights(a, weighting)
    e2 = ((a - b) * (a - b)).double()
    mse = (e2 * wr).sum(dim=(1, 2, 3)) / norm
    return torch.stack([mse, ms_product(ms_scales_torch(a, b, weighting, torch.float64))], dim=1)


def ms_metrics(x, y, weighting="ws"):
    """float64 CPU tensor (n, 2): [:, 0] WS-MSE, [:, 1] WS-MS-SSIM of each frame; the HIP kernels for GPU tensors,
    the float64 torch path for CPU tensors"""
    _check(x, y, weighting, min_side=MIN_SIDE)
    if x.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "ws_msssim"):
            raise PconvError("sphere metrics: the active backend has no ws_msssim kernel for a GPU tensor")
        return ops.ws_msssim(x, y, weighting)[0][:, SCALES:].contiguous()
    with torch.no_grad():
        return _ms_terms_torch(_as_planes(x), _as_planes(y), weighting)


def ws_ms_ssim(x, y, weighting="ws"):
    """float64 (n,) WS-MS-SSIM of each frame"""
    return ms_metrics(x, y, weighting)[:, 1]


class _WsMsTerms(torch.autograd.Function):
    """[WS-MSE, WS-MS-SSIM] per frame of GPU tensors: the forward kernels, whose pyramid and values are kept, and the
    backward kernels once per input that needs a gradient"""

    @staticmethod
    def forward(ctx, x, y, weighting, ops):
        values, workspace = ops.ws_msssim_device(x, y, weighting)
        ctx.save_for_backward(x, y)
        ctx.weighting, ctx.ops, ctx.values, ctx.workspace = weighting, ops, values, workspace
        return values[:, SCALES:].contiguous()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        gout = gout.contiguous()
        back = ctx.ops.ws_msssim_backward
        gx = back(y, x, ctx.workspace, ctx.values, gout, ctx.weighting, swapped=True) if ctx.needs_input_grad[0] else None
        gy = back(x, y, ctx.workspace, ctx.values, gout, ctx.weighting) if ctx.needs_input_grad[1] else None
        return gx, gy, None, None


def ms_loss_terms(x, y, weighting="ws"):
    """float64 (n, 2) [WS-MSE, WS-MS-SSIM] of each frame, on the inputs' device and attached to autograd: the values
    of `ms_metrics`, as a loss, with the contract of `loss_terms`.  A frame with any v_s <= 0 has WS-MS-SSIM 0 and a
    zero gradient of it"""
    _check(x, y, weighting, "sphere loss", MIN_SIDE)
    if not x.is_floating_point():
        raise PconvError("sphere loss: float (n, C, h, w) batches expected (uint8 frames carry no gradient), got %s %s"
                         % (x.dtype, tuple(x.shape)))
    if x.is_cuda:
        if x.dtype != torch.float32:
            raise PconvError("sphere loss: float32 GPU tensors expected, got %s" % x.dtype)
        ops = backend.ops()
        if not (hasattr(ops, "ws_msssim_device") and hasattr(ops, "ws_msssim_backward")):
            raise PconvError("sphere loss: the active backend has no ws_msssim kernels for a GPU tensor")
        return _WsMsTerms.apply(x.contiguous(), y.contiguous(), weighting, ops)
    return _ms_terms_torch(x, y, weighting)


def ms_backward_torch(x, y, gout, weighting="ws", dt=torch.float64):
    """the gradient of Σ_f gout[f, 0]·WS-MSE_f + gout[f, 1]·WS-MS-SSIM_f with respect to y, by the explicit chain of
    include/pconv_hip.h, in torch: the statement the HIP kernels are held to.  x, y (n, C, h, w); gout (n, 2).  The
    factors u_s, k and km are formed in float64 and rounded once to dt; everything else runs in dt, operation by
    operation in the kernels' order.  Returns dt (n, C, h, w)"""
    _check(x, y, weighting, "sphere loss", MIN_SIDE)
    if tuple(gout.shape) != (x.shape[0], 2):
        raise PconvError("sphere loss: gout (n, 2) expected, got %s for %s" % (tuple(gout.shape), tuple(x.shape)))
    n = x.shape[0]
    gout = gout.detach().double().to(x.device)
    gm, gs = gout[:, 0], gout[:, 1]
    x, y = x.detach().to(dt), y.detach().to(dt)
    v = ms_scales_torch(x, y, weighting, dt).double()
    ms = ms_product(v)
    positive = (v > 0).all(dim=1)
    safe = torch.where(v > 0, v, torch.ones_like(v))
    g, xs, ys, own = gaussian(), [x], [y], []
    for s in range(1, SCALES):
        xs.append(pool(xs[-1]))
        ys.append(pool(ys[-1]))
    for s in range(SCALES):
        a, b = xs[s], ys[s]
        wr, norm = _row_weights(a, weighting)
        u = torch.where(positive, gs * BETAS[s] * ms / safe[:, s], torch.zeros_like(gs))
        k = (u.view(n, 1, 1, 1) * wr / norm).to(dt)
        own.append(_own(a, b, k, _coefficients(_moments(a, b, g), s == SCALES - 1), g))
    grad = own[SCALES - 1]
    for s in range(SCALES - 2, -1, -1):
        up = torch.zeros_like(own[s])
        h2, w2 = grad.shape[-2:]
        up[..., :2 * h2, :2 * w2] = (0.25 * grad).repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
        grad = own[s] + up
    wr, norm = _row_weights(x, weighting)
    km = (2.0 * gm.view(n, 1, 1, 1) * wr / norm).to(dt)
    return grad + km * (y - x)
