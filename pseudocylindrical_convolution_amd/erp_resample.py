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

Training through the resize.  `resize` of a tensor that requires grad is attached to autograd through one Function whose
backward is the adjoint gx = Ax^T Ay^T g in a defined order (include/pconv_hip.h, pconv_erp_resample_backward_f32): first
the vertical adjoint, g (h2, w2) -> gmid (h, w2), then the horizontal one, gmid -> gx (h, w).  Every destination has one
fp32 accumulator; its terms are the table entries (output index ascending, then tap t ascending, the padded taps of
weight +0.0 included) that read it in the forward -- through the pole rule and the clamp vertically, where an entry that
crossed a pole takes g at column (c - w2 // 2) % w2, through the wrap horizontally; coinciding taps are terms of their
own; the first product starts the chain, every further term is one fp32 product and one fp32 addition; a destination
without a term gets +0; gmid is float32.  `reverse_taps` builds that order once per axis on the host (a CSR list per
source index from the very table `taps` returns), the kernels of csrc/erp_resample_backward.hip
(PCONV.erp_resample_backward_f32) gather along it without atomics, and `resize_backward_torch` is their twin: the same
bits.  clamp=True has torch.clamp's gradient: zero where the unclamped value lay outside [0, 1].
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


@functools.lru_cache(maxsize=64)
def _reverse_taps(n_in, n_out, pole):
    count = _native.call("pconv_host_lanczos_reverse_size", n_in, n_out)
    start, entry = np.empty(n_in + 1, dtype=np.int32), np.empty(count, dtype=np.int32)
    crossed = np.zeros(count, dtype=np.uint8)
    _native.call("pconv_host_lanczos_reverse", n_in, n_out, pole, start.ctypes.data, entry.ctypes.data, crossed.ctypes.data)
    return torch.from_numpy(start), torch.from_numpy(entry), torch.from_numpy(crossed)


def reverse_taps(n_in, n_out, pole):
    """(start int32 (n_in + 1,), entry int32 (n_out T,), crossed uint8 (n_out T,)) CPU tensors: the table of `taps`
    transposed (pconv_host_lanczos_reverse).  List k = entry[start[k]:start[k + 1]] holds the table entries e = i T + t
    that read source index k, ascending: a stable counting sort of the forward walk by destination, (first[i] + t) %
    n_in for pole=0 (the horizontal pass), the pole rule and the clamp for pole=1 (the vertical pass), where crossed says
    which entries crossed a pole (all zero for pole=0).  Built at the first backward of a size and cached: do not write
    to them"""
    return _reverse_taps(int(n_in), int(n_out), 1 if pole else 0)


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


def _adjoint_torch(g, weights, lists, turned=None):
    """one pass of the backward on the last-but-one axis (turned: the vertical pass, its half turn) or the last axis:
    vectorised in rounds, round k adds the k-th entry of every list that has one"""
    start, entry, crossed = (t.to(g.device) for t in lists)
    start, entry = start.long(), entry.long()
    flat, T = weights.to(g.device).reshape(-1), weights.shape[1]
    vertical = turned is not None
    n_in = start.numel() - 1
    shape = g.shape[:2] + ((n_in, g.shape[3]) if vertical else (g.shape[2], n_in))
    acc = torch.zeros(shape, dtype=torch.float32, device=g.device)
    length = start[1:] - start[:-1]
    alive = torch.nonzero(length > 0).flatten()      # the destinations that still have an entry in round k
    k = 0
    while alive.numel():
        at = start[alive] + k
        e = entry[at]
        i, wt = torch.div(e, T, rounding_mode="floor"), flat[e]
        if vertical:
            rows = g.index_select(2, i)
            flip = crossed[at] != 0
            if bool(flip.any()):
                rows = torch.where(flip[:, None], rows.index_select(3, turned), rows)
            term = rows * wt[:, None]
            acc[:, :, alive] = term if k == 0 else acc[:, :, alive] + term
        else:
            term = g.index_select(3, i) * wt
            acc[:, :, :, alive] = term if k == 0 else acc[:, :, :, alive] + term
        k += 1
        alive = alive[length[alive] > k]
    return acc


def resize_backward_torch(g, h, w):
    """the gradient of resize_torch (clamp=False) with respect to x, in the order of include/pconv_hip.h
    (pconv_erp_resample_backward_f32), float32 operation by operation on any device (the CPU path and the kernels'
    twin): float32 (n, C, h2, w2) -> (n, C, h, w)"""
    if g.dim() != 4 or g.dtype != torch.float32:
        raise PconvError("erp resize: a float32 (n, C, h2, w2) gradient expected, got %s %s" % (g.dtype, tuple(g.shape)))
    h, w = int(h), int(w)
    h2, w2 = g.shape[2:]
    if not (2 <= h <= 1 << 20 and 2 <= w <= 1 << 20):
        raise PconvError("erp resize: a side of %dx%d is outside 2 .. 2^20" % (w, h))
    _check(g.new_empty((1, 1, h, w)), h2, w2)
    turned = torch.remainder(torch.arange(w2, device=g.device) - w2 // 2, w2)
    gmid = _adjoint_torch(g, taps(h, h2)[1], reverse_taps(h, h2, 1), turned)
    return _adjoint_torch(gmid, taps(w, w2)[1], reverse_taps(w, w2, 0))


def _forward(x, h2, w2, clamp=False, out=None):
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


class _Resize(torch.autograd.Function):
    """the resize under autograd: the forward is the caller's unclamped one; the backward the ordered adjoint, the
    kernels for GPU tensors and resize_backward_torch for CPU tensors: the same bits.  clamp: torch.clamp's gradient,
    zero where the unclamped value lay outside [0, 1] (the mask is saved only then)"""

    @staticmethod
    def forward(ctx, x, h2, w2, clamp):
        out = _forward(x, h2, w2)
        ctx.source, ctx.clamp = tuple(x.shape[2:]), clamp
        if clamp:
            ctx.save_for_backward((out >= 0.0) & (out <= 1.0))
            out = out.clamp_(0.0, 1.0)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.clamp:
            g = torch.where(ctx.saved_tensors[0], g, torch.zeros((), dtype=g.dtype, device=g.device))
        g = g.contiguous()
        h, w = ctx.source
        if g.is_cuda:
            ops = backend.ops()
            if not hasattr(ops, "erp_resample_backward_f32"):
                raise PconvError("erp resize: the active backend has no erp_resample_backward_f32 kernel for a GPU tensor")
            return ops.erp_resample_backward_f32(g, h, w), None, None, None
        return resize_backward_torch(g, h, w), None, None, None


def resize(x, h2, w2, clamp=False, out=None):
    """float32 (n, C, h, w) -> (n, C, h2, w2): the HIP kernels for GPU tensors, the torch twin on the CPU.
    clamp=True bounds the result to [0, 1] (Lanczos overshoots at edges).  With grad mode on and x requiring a gradient
    the result is attached to autograd (one Function; `_Resize`): the values are the same, the backward is the ordered
    one of include/pconv_hip.h (pconv_erp_resample_backward_f32), its lists built at the first backward of a size.
    out= is refused then"""
    h2, w2 = _check(x, h2, w2)
    if torch.is_grad_enabled() and x.requires_grad:
        if out is not None:
            raise PconvError("erp resize: out= cannot be combined with a gradient: the result of an input that requires "
                             "grad is a new tensor attached to autograd")
        return _Resize.apply(x, h2, w2, bool(clamp))
    return _forward(x, h2, w2, clamp, out)
