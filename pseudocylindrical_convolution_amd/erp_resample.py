"""Panoramas at a reduced size: the sphere-aware Lanczos-3 resize (include/pconv_hip.h, pconv_erp_resample_f32).

float32 (n, C, h, w) -> (n, C, h2, w2), separable Lanczos-3 with pixel centres at (j + 1/2) / size, the kernel
stretched by max(1, in / out) when an axis shrinks.  The horizontal pass wraps the seam (source column modulo w);
the vertical pass continues the sphere across the poles as erp_size.py does (mirrored row, longitude turned by half
a revolution: column (i + w2 // 2) % w2 of the intermediate picture).  Both sums run over the taps in ascending
order with one fp32 rounding per product and per addition, so the HIP kernels of csrc/erp_resample.hip
(PCONV.erp_resample_f32) and `resize_torch` below give the same bits.

The tap tables come from one place, pconv_host_lanczos_taps (host C, double), through ctypes: `taps`.
`resize` dispatches like erp_size.pad: the HIP kernels for GPU tensors, the torch twin for CPU tensors (the oracle
backend).
"""
import ctypes
import functools

import numpy as np
import torch

from . import _native
from ._native import PconvError
from .PCONV_operator import backend

MAX_SHRINK = 8   # n_in <= 8 * n_out on each axis


@functools.lru_cache(maxsize=64)
def _taps(n_in, n_out):
    count = ctypes.c_int()
    _native.call("pconv_host_lanczos_taps", n_in, n_out, None, None, ctypes.addressof(count))
    first = np.empty(n_out, dtype=np.int32)
    weights = np.empty((n_out, count.value), dtype=np.float32)
    _native.call("pconv_host_lanczos_taps", n_in, n_out, first.ctypes.data, weights.ctypes.data, ctypes.addressof(count))
    return torch.from_numpy(first), torch.from_numpy(weights)


def taps(n_in, n_out):
    """(first int32 (n_out,), weights float32 (n_out, T)) CPU tensors of one axis n_in -> n_out: source sample
    first[i] + t weighs weights[i, t] in output sample i (rows shorter than T end in +0.0).  Do not write to them:
    the tables are cached"""
    return _taps(int(n_in), int(n_out))


def _check(x, h2, w2):
    if x.dim() != 4 or x.dtype != torch.float32:
        raise PconvError("erp resize: float32 (n, C, h, w) expected, got %s %s" % (x.dtype, tuple(x.shape)))
    h2, w2 = int(h2), int(w2)
    for n_in, n_out in ((x.shape[2], h2), (x.shape[3], w2)):
        if not (2 <= n_in <= 1 << 20 and 2 <= n_out <= 1 << 20):
            raise PconvError("erp resize: a side of %d -> %d is outside 2 .. 2^20" % (n_in, n_out))
        if n_in > MAX_SHRINK * n_out:
            raise PconvError("erp resize: %d -> %d shrinks by more than %d:1" % (n_in, n_out, MAX_SHRINK))
    return h2, w2


def resize_torch(x, h2, w2, clamp=False):
    """the definition in torch, float32 operation by operation, on any device (the CPU path and the kernels' twin)"""
    h2, w2 = _check(x, h2, w2)
    h, w = x.shape[2:]
    fx, wx = (t.to(x.device) for t in taps(w, w2))
    fy, wy = (t.to(x.device) for t in taps(h, h2))
    fx, fy = fx.long(), fy.long()
    mid = None
    for t in range(wx.shape[1]):
        term = x.index_select(3, torch.remainder(fx + t, w)) * wx[:, t]
        mid = term if mid is None else mid + term
    turned = torch.remainder(torch.arange(w2, device=x.device) + w2 // 2, w2)
    out = None
    for t in range(wy.shape[1]):
        r = fy + t
        flip = (r < 0) | (r >= h)
        r = torch.where(r < 0, -1 - r, torch.where(r >= h, 2 * h - 1 - r, r)).clamp(0, h - 1)
        rows = mid.index_select(2, r)
        if bool(flip.any()):
            rows = torch.where(flip[:, None], rows.index_select(3, turned), rows)
        term = rows * wy[:, t, None]
        out = term if out is None else out + term
    return out.clamp(0.0, 1.0) if clamp else out


def resize(x, h2, w2, clamp=False, out=None):
    """float32 (n, C, h, w) -> (n, C, h2, w2): the HIP kernels for GPU tensors, the torch twin on the CPU.
    clamp=True bounds the result to [0, 1] (Lanczos overshoots at edges)"""
    h2, w2 = _check(x, h2, w2)
    if x.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "erp_resample_f32"):
            raise PconvError("erp resize: the active backend has no erp_resample_f32 kernel for a GPU tensor")
        return ops.erp_resample_f32(x.contiguous(), h2, w2, clamp, out)
    res = resize_torch(x, h2, w2, clamp)
    if out is not None:
        out.copy_(res)
        return out
    return res
