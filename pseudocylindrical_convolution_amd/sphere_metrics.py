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
"""
import math

import torch
import torch.nn.functional as F

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


def metrics_torch(x, y, weighting="ws"):
    """float64 (n, 2) [WS-MSE, WS-SSIM]: the definitions above in float64 torch, on the batches' device (the CPU
    path of `metrics`, and the reference the GPU tests compare the kernel with)"""
    if x.dtype != y.dtype or x.shape != y.shape or x.device != y.device:
        raise PconvError("sphere metrics: the two batches differ: %s %s %s vs %s %s %s"
                         % (x.device, x.dtype, tuple(x.shape), y.device, y.dtype, tuple(y.shape)))
    a, b = _as_planes(x), _as_planes(y)
    n, c, h, w = a.shape
    wr = weights(h, weighting).to(a.device)
    norm = c * w * float(wr.sum())
    wr = wr.view(1, 1, h, 1)
    e2 = ((a - b) * (a - b)).double()
    a, b = a.double(), b.double()
    g = gaussian()
    mu1, mu2 = _blur(a, g), _blur(b, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = _blur(a * a, g) - mu1_sq, _blur(b * b, g) - mu2_sq, _blur(a * b, g) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return torch.stack([(e2 * wr).sum(dim=(1, 2, 3)) / norm, (ssim_map * wr).sum(dim=(1, 2, 3)) / norm], dim=1).cpu()


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
