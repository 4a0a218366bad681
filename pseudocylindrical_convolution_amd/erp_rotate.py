"""Panoramas in a rotated orientation: the sphere rotation of ERP frames (include/pconv_hip.h, pconv_erp_rotation_map /
pconv_erp_remap_f32).

float32 (n, C, h, w) -> (n, C, h, w): the same sphere, turned so that the source point at longitude yaw, latitude pitch
lands in the centre of the picture, roll turning the picture about that centre -- the sphere-rotation step of 360Lib
and the sphere-rotation SEI of HEVC / VVC, whose units and ranges the angles follow.  A rotation is a triple of int32 in
units of 2^-16 degree (`units` makes it from degrees, rounding once), or None for "no rotation"; everything downstream
holds the integers, so encoder and decoder build the same map.

Output pixel d reads the source at s = M d, M = Rz(yaw) Ry(-pitch) Rx(roll) (`matrix`, host C in double through
ctypes); the way back uses the transpose.  `source_map` turns M into one record per output pixel, the source position
in 1/256 pixel (fp64: the HIP kernel on a GPU, `source_map_numpy` on the CPU); `rotate_torch` / the HIP sampler read the
source there with a 6 x 6 Lanczos-3 footprint whose weights come from `phases` (host C in double through ctypes),
columns wrapped at the seam, rows continued across the poles as erp_size.py and erp_resample.py continue them.  Both
sums run in ascending order with one fp32 rounding per product and per addition, so the HIP kernel of
csrc/erp_rotate.hip (PCONV.erp_remap_f32) and `rotate_torch` give the same bits on the same map.

`rotate` dispatches like erp_resample.resize: the HIP kernels for GPU tensors, the twin for CPU tensors (the oracle
backend).
"""
import ctypes
import functools

import numpy as np
import torch

from . import _native
from ._native import PconvError
from .PCONV_operator import backend

PHASES = 256   # positions per pixel (PCONV_ERP_ROTATE_PHASES)
TAPS = 6       # Lanczos-3 (PCONV_ERP_ROTATE_TAPS)
UNIT = 1 << 16   # units per degree
_RANGE = ((-180 * UNIT, 180 * UNIT - 1), (-90 * UNIT, 90 * UNIT), (-180 * UNIT, 180 * UNIT - 1))


def check(rotation):
    """the integer triple (yaw, pitch, roll) of `rotation`, or None for None and for (0, 0, 0); PconvError for
    anything that is not three integers in the SEI's ranges"""
    if rotation is None:
        return None
    try:
        triple = tuple(rotation)
        if len(triple) != 3 or any(int(v) != v for v in triple):
            raise TypeError
        triple = tuple(int(v) for v in triple)
    except (TypeError, ValueError):
        raise PconvError("erp rotate: a rotation is three integers in units of 2^-16 degree (erp_rotate.units), got %r"
                         % (rotation,))
    for name, v, (lo, hi) in zip(("yaw", "pitch", "roll"), triple, _RANGE):
        if not lo <= v <= hi:
            raise PconvError("erp rotate: %s %d is outside %d .. %d (units of 2^-16 degree)" % (name, v, lo, hi))
    return triple if any(triple) else None


def units(yaw, pitch, roll):
    """degrees -> the integer triple in units of 2^-16 degree, rounded once; None for (0, 0, 0).  yaw and roll in
    [-180, 180), pitch in [-90, 90]: values out of range are refused, not wrapped"""
    return check(tuple(int(round(float(v) * UNIT)) for v in (yaw, pitch, roll)))


def degrees(rotation):
    """the triple in degrees ((0, 0, 0) for None)"""
    return tuple(v / float(UNIT) for v in (check(rotation) or (0, 0, 0)))


@functools.lru_cache(maxsize=64)
def _matrix(rotation, inverse):
    m = np.empty((3, 3), dtype=np.float64)
    _native.call("pconv_host_erp_rotation_matrix", rotation[0], rotation[1], rotation[2], 1 if inverse else 0, m.ctypes.data)
    m.setflags(write=False)
    return m


def matrix(rotation, inverse=False):
    """M (3, 3) float64, read-only: output direction d reads the source at M d (inverse=True: the transpose)"""
    return _matrix(check(rotation) or (0, 0, 0), bool(inverse))


@functools.lru_cache(maxsize=1)
def phases():
    """the phase table, float32 (PHASES, TAPS) CPU tensor: row p weighs the samples base - 2 .. base + 3 of a position
    p / PHASES past `base`.  Do not write to it: the table is cached"""
    table = np.empty((PHASES, TAPS), dtype=np.float32)
    _native.call("pconv_host_lanczos_phases", table.ctypes.data)
    return torch.from_numpy(table)


def _check_size(h, w):
    h, w = int(h), int(w)
    if not (2 <= h <= 1 << 20 and 2 <= w <= 1 << 20):
        raise PconvError("erp rotate: a side of %dx%d is outside 2 .. 2^20" % (w, h))
    if 4 * h * w >= 1 << 31:
        raise PconvError("erp rotate: a plane of %dx%d float32 is 2^31 bytes or more" % (w, h))
    return h, w


def source_coordinates(h, w, rotation, inverse=False):
    """(u, v) float64 (h, w): the source column and row, in pixels, that output pixel (j, i) reads (the rule before its
    quantisation)"""
    h, w = _check_size(h, w)
    m = matrix(rotation, inverse)
    theta = ((np.arange(w, dtype=np.float64) + 0.5) / w - 0.5) * (2.0 * np.pi)
    phi = (0.5 - (np.arange(h, dtype=np.float64) + 0.5) / h) * np.pi
    cp, sp = np.cos(phi)[:, None], np.sin(phi)[:, None]
    d = (cp * np.cos(theta)[None, :], cp * np.sin(theta)[None, :], sp * np.ones((1, w)))
    sx, sy, sz = (m[r, 0] * d[0] + m[r, 1] * d[1] + m[r, 2] * d[2] for r in range(3))
    u = (np.arctan2(sy, sx) / (2.0 * np.pi) + 0.5) * w - 0.5
    v = (0.5 - np.arctan2(sz, np.hypot(sx, sy)) / np.pi) * h - 0.5
    return u, v


def source_map_numpy(h, w, rotation, inverse=False):
    """the map in float64 on the host: int32 (h, w, 2), [..., 0] = rint(u * PHASES) modulo w * PHASES, [..., 1] =
    rint(v * PHASES)"""
    u, v = source_coordinates(h, w, rotation, inverse)
    qu = np.mod(np.rint(u * PHASES).astype(np.int64), int(w) * PHASES)
    qv = np.rint(v * PHASES).astype(np.int64)
    return np.stack([qu, qv], axis=2).astype(np.int32)


@functools.lru_cache(maxsize=4)
def _source_map(h, w, rotation, inverse, device):
    device = torch.device(device)
    if device.type == "cuda":
        ops = backend.ops()
        if not hasattr(ops, "erp_rotation_map"):
            raise PconvError("erp rotate: the active backend has no erp_rotation_map kernel for a GPU device")
        return ops.erp_rotation_map(h, w, rotation, inverse, device)
    return torch.from_numpy(source_map_numpy(h, w, rotation, inverse))


@functools.lru_cache(maxsize=4)
def _reverse_lists(h, w, rotation, inverse, device):
    """the reverse lists of the backward (viewport.reverse_lists) of the cached map: 144 bytes per pixel, the last 4 kept"""
    from . import viewport
    return viewport.reverse_lists(_source_map(h, w, rotation, inverse, device), h, w)


def source_map(h, w, rotation, inverse=False, device=None):
    """int32 (h, w, 2) map of an h x w frame on `device`: from the HIP kernel for a GPU device, from source_map_numpy
    on the CPU (the two agree except where a position lies within 1e-10 of a rounding boundary).  The last 4 maps are
    kept: a map is 8 bytes per pixel, 268 MB at 8192x4096.  Do not write to it"""
    h, w = _check_size(h, w)
    rotation = check(rotation) or (0, 0, 0)
    device = torch.device("cpu" if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _source_map(h, w, rotation, bool(inverse), str(device))


def _check(x, map=None):
    if x.dim() != 4 or x.dtype != torch.float32:
        raise PconvError("erp rotate: float32 (n, C, h, w) expected, got %s %s" % (x.dtype, tuple(x.shape)))
    h, w = _check_size(*x.shape[2:])
    if map is not None and (map.dtype != torch.int32 or tuple(map.shape) != (h, w, 2) or map.device != x.device):
        raise PconvError("erp rotate: the map must be int32 (%d, %d, 2) on the frames' device, got %s %s on %s"
                         % (h, w, map.dtype, tuple(map.shape), map.device))
    return h, w


def sample_torch(x, map):
    """the 6 x 6 footprint of every record of `map` (int32 (.., .., 2): any grid, not only the frames' own) on float32
    (n, C, h, w) frames, float32 operation by operation: (n, C) + map.shape[:2].  What rotate_torch and
    viewport.render_torch sample with"""
    h, w = x.shape[2:]
    table = phases().to(x.device)
    q = map.long()
    col0, row0 = torch.div(q[..., 0], PHASES, rounding_mode="floor") - 2, torch.div(q[..., 1], PHASES, rounding_mode="floor") - 2
    wx, wy = table[torch.remainder(q[..., 0], PHASES)], table[torch.remainder(q[..., 1], PHASES)]   # (h, w, TAPS)
    cols = [torch.remainder(col0 + b, w) for b in range(TAPS)]
    turned = [torch.remainder(c + w // 2, w) for c in cols]
    out = None
    for a in range(TAPS):
        r = row0 + a
        crossed = (r < 0) | (r >= h)
        r = torch.where(r < 0, -1 - r, torch.where(r >= h, 2 * h - 1 - r, r)).clamp(0, h - 1)
        line = None
        for b in range(TAPS):
            term = x[:, :, r, torch.where(crossed, turned[b], cols[b])] * wx[..., b]
            line = term if line is None else line + term
        term = line * wy[..., a]
        out = term if out is None else out + term
    return out


def rotate_torch(x, map, clamp=False):
    """the sampler in torch, float32 operation by operation, on any device (the CPU path and the kernel's twin)"""
    _check(x, map)
    out = sample_torch(x, map)
    return out.clamp(0.0, 1.0) if clamp else out


def rotate(x, rotation, inverse=False, clamp=False, out=None):
    """float32 (n, C, h, w) -> (n, C, h, w) in the orientation `rotation` (inverse=True: back from it): the HIP
    kernels for GPU tensors, the twin on the CPU.  clamp=True bounds the result to [0, 1] (Lanczos overshoots at
    edges).  rotation None (or all zeros): x itself comes back, nothing runs.  With grad mode on and x requiring a
    gradient the result is attached to autograd through viewport's Function with ss = 1 and the frame as the grid: the
    ordered backward of include/pconv_hip.h (pconv_remap_backward_f32; the kernel on the GPU, its twin on the CPU: the
    same bits), its lists built at the first backward and cached like the map; out= is refused then"""
    rotation = check(rotation)
    if rotation is None:
        return x
    h, w = _check(x)
    map = source_map(h, w, rotation, inverse, x.device)
    if torch.is_grad_enabled() and x.requires_grad:
        if out is not None:
            raise PconvError("erp rotate: out= cannot be combined with a gradient: the result of an input that requires "
                             "grad is a new tensor attached to autograd")
        from . import viewport   # (viewport imports this module)
        key = (h, w, rotation, bool(inverse), str(map.device))
        views = [(map, lambda: _reverse_lists(*key), 1)]
        return viewport._Remap.apply(x, lambda t: rotate(t, rotation, inverse).unsqueeze(1), views, bool(clamp))[:, 0]
    if x.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "erp_remap_f32"):
            raise PconvError("erp rotate: the active backend has no erp_remap_f32 kernel for a GPU tensor")
        return ops.erp_remap_f32(x.contiguous(), map, clamp, out)
    res = rotate_torch(x, map, clamp)
    if out is not None:
        out.copy_(res)
        return out
    return res
