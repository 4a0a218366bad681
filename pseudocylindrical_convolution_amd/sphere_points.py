"""Sphere-sampled quality of ERP panoramas: S-PSNR-NN, S-PSNR-I and CPP-PSNR (include/pconv_hip.h,
pconv_sphere_points_*; csrc/sphere_points.hip).

WS-PSNR compares two pictures on one ERP grid.  The three metrics here read both pictures at the same points of the
sphere instead, so the pictures may have ANY two sizes and neither is resampled onto the other's grid: the
reconstruction of a file coded at a reduced size (--code-size) is scored as it is against the source as it is.

Point: a direction as two float64, longitude t in [-pi, pi] and latitude p in [-pi/2, pi/2], in the ERP convention of
erp_rotate.py.  A point set is float64 (P, 2) of (t, p) in a fixed order, 1 <= P < 2^28:
  icosphere(level)    the 10 * 4^level + 2 vertices of a subdivided icosahedron; level 8 (655 362 points, the size of
                      360Lib's point file) is the default of the S-PSNR figures.  360Lib's own file is not part of
                      this project, so equality of the figures with 360Lib's is NOT claimed;
  load_points(path)   a text file of degrees: whoever has 360Lib's file gets its set;
  cpp_grid(h, w)      the valid pixels of a Craster parabolic picture of h x w (CPP-PSNR).
Record of a point for a picture of h x w, all in float64, in this order, no transcendental (`records_numpy`; the HIP
kernel gives EQUAL records, with no exception near a rounding boundary):
  u = ((t / (2 pi)) + 0.5) * w - 0.5        v = (0.5 - (p / pi)) * h - 0.5
  qu = rint(u * 256) modulo w * 256         qv = rint(v * 256)                     int32 (P, 2)
Sample, interp="lanczos" (S-PSNR-I, CPP-PSNR): erp_rotate.sample_torch at the record, the 6 x 6 Lanczos-3 footprint with
the seam wrapped and the poles continued, fp32 operation by operation.  interp="nearest" (S-PSNR-NN): column =
floor((qu + 128) / 256) mod w, row = floor((qv + 128) / 256) through the pole rule (a row that crossed a pole takes
column + floor(w / 2) mod w), then clamped; the pixel itself.
Error: d = a - b and e = d * d in fp32, a from picture x, b from picture y; MSE[f][c] = (sum of e over the points, in
fp64) / P; a figure is 10 log10(1 / mean over the channels of MSE[f]) as sphere_metrics.psnr gives it.

Limits.  Positions are quantised to 1/256 pixel before the nearest / Lanczos choice.  S-PSNR-I uses this project's
Lanczos-3 sampler, not 360Lib's interpolator.  The RGB channels are averaged where 360Lib reports Y, U and V; `mse`
returns the per-channel values, so a caller with planar YUV gets per-plane figures.  The 4:2:0 path (yuv.py, chroma
siting) is out of scope.  Memory: a PointSet keeps 8 bytes per point and picture size on the device (the last 4 sizes):
5 MB at level 8, about 180 MB per size for the CPP grid of 8192 x 4096.

GPU tensors go to the HIP kernels (PCONV.sphere_points_*: `mse` is one fused pass, sample + error + a sum in a fixed
order, no atomics, nothing of size P written); CPU tensors go to the torch twins below (the oracle backend and the CPU
tests).  The twins are no fallback: a GPU tensor on a backend without the kernels is a PconvError.
"""
import collections
import functools
import math

import numpy as np
import torch

from . import erp_rotate, sphere_metrics
from ._native import PconvError
from .PCONV_operator import backend

PHASES = erp_rotate.PHASES
INTERPS = ("lanczos", "nearest")
MAX_POINTS = (1 << 28) - 1
LEVEL = 8          # icosphere(8): 655 362 points
KEPT_SIZES = 4     # record tensors a PointSet keeps


def _unit_to_points(v):
    """unit vectors (P, 3) -> (t, p): t = atan2(y, x) (0 at the poles), p = asin(z)"""
    t = np.arctan2(v[:, 1], v[:, 0])
    t[(v[:, 0] == 0) & (v[:, 1] == 0)] = 0.0
    return np.stack([t, np.arcsin(np.clip(v[:, 2], -1.0, 1.0))], axis=1)


@functools.lru_cache(maxsize=4)
def icosphere_vertices(level):
    """float64 (10 * 4^level + 2, 3), read-only: the unit vectors of `icosphere`, in its order"""
    level = int(level)
    if not 0 <= level <= 10:
        raise PconvError("sphere points: icosphere level %d is outside 0 .. 10" % level)
    lat = math.atan(0.5)
    v = [(0.0, 0.0, 1.0)]
    v += [(math.cos(lat) * math.cos(2 * math.pi * k / 5), math.cos(lat) * math.sin(2 * math.pi * k / 5), math.sin(lat))
          for k in range(5)]
    v += [(math.cos(lat) * math.cos(2 * math.pi * (k + 0.5) / 5), math.cos(lat) * math.sin(2 * math.pi * (k + 0.5) / 5),
           -math.sin(lat)) for k in range(5)]
    v += [(0.0, 0.0, -1.0)]
    v = np.array(v, dtype=np.float64)
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    faces = []
    for k in range(5):
        a, b, c, d = 1 + k, 1 + (k + 1) % 5, 6 + k, 6 + (k + 1) % 5
        faces += [(0, a, b), (a, c, b), (b, c, d), (c, 11, d)]
    faces = np.array(faces, dtype=np.int64)
    for _ in range(level):
        count = v.shape[0]
        ends = np.stack([faces, faces[:, (1, 2, 0)]], axis=2).reshape(-1, 2)     # edges v0v1, v1v2, v2v0 of each face
        lo, hi = ends.min(axis=1), ends.max(axis=1)
        _, first, inverse = np.unique(lo * count + hi, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")        # the edges by first appearance
        rank = np.empty_like(order)
        rank[order] = np.arange(order.size)
        mid = v[lo[first[order]]] + v[hi[first[order]]]
        mid /= np.sqrt((mid * mid).sum(axis=1, keepdims=True))
        v = np.concatenate([v, mid], axis=0)
        m = (count + rank[inverse.reshape(-1)]).reshape(-1, 3)                   # m01, m12, m20 of each face
        faces = np.stack([np.stack([faces[:, 0], m[:, 0], m[:, 2]], axis=1), np.stack([faces[:, 1], m[:, 1], m[:, 0]], axis=1),
                          np.stack([faces[:, 2], m[:, 2], m[:, 1]], axis=1), m], axis=1).reshape(-1, 3)
    v.setflags(write=False)
    return v


def icosphere(level=LEVEL):
    """float64 (10 * 4^level + 2, 2) points (t, p): the vertices of the icosahedron with its two poles on +-z (five
    vertices at latitude atan(1/2), longitudes 72 k degrees, five at -atan(1/2), longitudes 72 k + 36), each edge
    bisected `level` times, every new vertex put back on the sphere.  Order: the north pole, the upper five, the lower
    five, the south pole; then, level by level, the midpoints of the edges in the order in which the edges first appear
    when the faces are walked in order and each face's edges as (v0 v1, v1 v2, v2 v0); a face (v0, v1, v2) is replaced, in
    place, by (v0, m01, m20), (v1, m12, m01), (v2, m20, m12), (m01, m12, m20).  The 20 faces start as, for k = 0 .. 4
    with a, b the upper vertices k, k + 1 and c, d the lower ones: (north, a, b), (a, c, b), (b, c, d), (c, south, d).
    This is not 360Lib's point file (not available to this project): no equality with its figures is claimed"""
    return _unit_to_points(icosphere_vertices(level))


def cpp_grid(h, w):
    """float64 (P, 2) points (t, p): the valid pixels of a Craster parabolic picture of h x w in row-major order.  Pixel
    (j, i): X = ((i + 1/2)/w - 1/2) 2 pi, Y = (1/2 - (j + 1/2)/h) pi, p = 3 asin(Y / pi), t = X / (2 cos(2 p / 3) - 1),
    valid iff |t| <= pi: two thirds of the rectangle"""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise PconvError("sphere points: a CPP picture of %dx%d" % (w, h))
    X = ((np.arange(w, dtype=np.float64) + 0.5) / w - 0.5) * (2.0 * np.pi)
    Y = (0.5 - (np.arange(h, dtype=np.float64) + 0.5) / h) * np.pi
    p = 3.0 * np.arcsin(Y / np.pi)
    t = X[None, :] / (2.0 * np.cos(2.0 * p / 3.0) - 1.0)[:, None]
    valid = np.abs(t) <= np.pi
    pts = np.stack([t[valid], np.broadcast_to(p[:, None], t.shape)[valid]], axis=1)
    if pts.shape[0] == 0:
        raise PconvError("sphere points: the CPP picture of %dx%d has no valid pixel" % (w, h))
    return pts


def load_points(path, order="latlon"):
    """float64 (P, 2) points (t, p) from a text file of degrees, two numbers per line: (latitude, longitude) for
    order="latlon", (longitude, latitude) for "lonlat".  A first line with a single number (the count, as 360Lib's
    sphere files have it) is checked against the lines that follow; empty lines are skipped.  Latitudes in [-90, 90];
    longitudes in [-180, 360], those above 180 taken 360 lower"""
    if order not in ("latlon", "lonlat"):
        raise PconvError("sphere points: order must be 'latlon' or 'lonlat', got %r" % (order,))
    with open(path) as f:
        rows = [line.split() for line in f if line.strip()]
    count = None
    if rows and len(rows[0]) == 1:
        count, rows = int(rows[0][0]), rows[1:]
    if not rows or any(len(r) != 2 for r in rows) or (count is not None and count != len(rows)):
        raise PconvError("sphere points: %s: two numbers per line expected%s, got %d lines"
                         % (path, "" if count is None else " and %d lines after the count" % count, len(rows)))
    deg = np.array(rows, dtype=np.float64)
    lat, lon = (deg[:, 0], deg[:, 1]) if order == "latlon" else (deg[:, 1], deg[:, 0])
    if not (np.all(np.abs(lat) <= 90.0) and np.all((lon >= -180.0) & (lon <= 360.0))):
        raise PconvError("sphere points: %s: latitudes in [-90, 90] and longitudes in [-180, 360] degrees expected" % path)
    lon = np.where(lon > 180.0, lon - 360.0, lon)
    return np.stack([np.radians(lon), np.radians(lat)], axis=1)


def _check_size(h, w):
    h, w = int(h), int(w)
    if not (2 <= h <= 1 << 20 and 2 <= w <= 1 << 20):
        raise PconvError("sphere points: a side of %dx%d is outside 2 .. 2^20" % (w, h))
    if 4 * h * w >= 1 << 31:
        raise PconvError("sphere points: a plane of %dx%d float32 is 2^31 bytes or more" % (w, h))
    return h, w


class PointSet(object):
    """a point set: the host array (`points`, float64 (P, 2), read-only) and the record tensors made from it, the last
    KEPT_SIZES (picture size, device) pairs: 8 bytes per point each"""

    def __init__(self, points):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 2 or not 1 <= pts.shape[0] <= MAX_POINTS:
            raise PconvError("sphere points: float64 (P, 2) points, 1 <= P < 2^28, expected, got %s" % (pts.shape,))
        if not (np.all(np.abs(pts[:, 0]) <= np.pi) and np.all(np.abs(pts[:, 1]) <= np.pi / 2)):
            raise PconvError("sphere points: longitudes in [-pi, pi] and latitudes in [-pi/2, pi/2] expected")
        if pts is points:
            pts = pts.copy()
        pts.setflags(write=False)
        self.points = pts
        self._records = collections.OrderedDict()

    def __len__(self):
        return self.points.shape[0]

    def records(self, h, w, device=None):
        """int32 (P, 2) on `device` for a picture of h x w; do not write to it"""
        h, w = _check_size(h, w)
        device = torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (h, w, str(device))
        if key in self._records:
            self._records.move_to_end(key)
            return self._records[key]
        if device.type == "cuda":
            ops = backend.ops()
            if not hasattr(ops, "sphere_points_records"):
                raise PconvError("sphere points: the active backend has no sphere_points_records kernel for a GPU device")
            rec = ops.sphere_points_records(torch.tensor(self.points).to(device), h, w)   # (a copy: the points are not kept there)
        else:
            rec = torch.from_numpy(records_numpy(self.points, h, w))
        self._records[key] = rec
        while len(self._records) > KEPT_SIZES:
            self._records.popitem(last=False)
        return rec


def _pointset(pointset):
    return pointset if isinstance(pointset, PointSet) else PointSet(pointset)


def records_numpy(points, h, w):
    """int32 (P, 2) records of `points` (a PointSet or float64 (P, 2)) for a picture of h x w, in float64 on the host,
    operation by operation in the kernel's order"""
    h, w = _check_size(h, w)
    pts = points.points if isinstance(points, PointSet) else np.asarray(points, dtype=np.float64)
    u = ((pts[:, 0] / (2.0 * np.pi)) + 0.5) * float(w) - 0.5
    v = (0.5 - (pts[:, 1] / np.pi)) * float(h) - 0.5
    qu = np.mod(np.rint(u * float(PHASES)).astype(np.int64), w * PHASES)
    qv = np.rint(v * float(PHASES)).astype(np.int64)
    return np.stack([qu, qv], axis=1).astype(np.int32)


def records(pointset, h, w, device=None):
    """int32 (P, 2) records of a PointSet for a picture of h x w on `device`: the HIP kernel for a GPU device,
    records_numpy on the CPU -- equal, record for record.  Cached in the PointSet; do not write to it"""
    return _pointset(pointset).records(h, w, device)


def _as_planes(t):
    """the batch as float32 (n, C, h, w): uint8 (n, h, w, 3) through frames_u8_to_f32's arithmetic, float(u8) / 255"""
    if t.dim() != 4:
        raise PconvError("sphere points: 4-D batches expected, got %s" % (tuple(t.shape),))
    if t.dtype == torch.uint8 and t.shape[3] == 3:
        if t.is_cuda and hasattr(backend.ops(), "frames_u8_to_f32"):
            return backend.ops().frames_u8_to_f32(t.contiguous())
        return (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    if t.dtype == torch.float32:
        return t
    raise PconvError("sphere points: float32 (n, C, h, w) or uint8 (n, h, w, 3) expected, got %s %s" % (t.dtype, tuple(t.shape)))


def _check_interp(interp):
    if interp not in INTERPS:
        raise PconvError("sphere points: interp must be one of %s, got %r" % (INTERPS, interp))


def _check_records(x, rec):
    _check_size(*x.shape[2:])
    if rec.dtype != torch.int32 or rec.dim() != 2 or rec.shape[1] != 2 or rec.device != x.device:
        raise PconvError("sphere points: the records must be int32 (P, 2) on the frames' device, got %s %s on %s"
                         % (rec.dtype, tuple(rec.shape), rec.device))


def sample_torch(x, rec, interp="lanczos"):
    """float32 (n, C, h, w) -> (n, C, P): the frames read at the records `rec` (int32 (P, 2), of this h x w), in torch,
    float32 operation by operation, on any device: the CPU path of `sample` and the kernel's twin, bit for bit"""
    _check_interp(interp)
    x = _as_planes(x)
    _check_records(x, rec)
    if interp == "lanczos":
        return erp_rotate.sample_torch(x, rec[None])[:, :, 0]
    h, w = x.shape[2:]
    q = rec.long()
    col = torch.remainder(torch.div(q[:, 0] + PHASES // 2, PHASES, rounding_mode="floor"), w)
    r = torch.div(q[:, 1] + PHASES // 2, PHASES, rounding_mode="floor")
    crossed = (r < 0) | (r >= h)
    r = torch.where(r < 0, -1 - r, torch.where(r >= h, 2 * h - 1 - r, r)).clamp(0, h - 1)
    return x[:, :, r, torch.where(crossed, torch.remainder(col + w // 2, w), col)]


def sample(x, pointset, interp="lanczos", out=None):
    """float32 (n, C, h, w) (or uint8 (n, h, w, 3)) -> float32 (n, C, P): the panorama read at the directions of the point
    set.  The HIP kernel for GPU tensors, `sample_torch` for CPU tensors: the same bits"""
    _check_interp(interp)
    x = _as_planes(x)
    rec = records(pointset, x.shape[2], x.shape[3], x.device)
    if x.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "sphere_points_sample_f32"):
            raise PconvError("sphere points: the active backend has no sphere_points_sample_f32 kernel for a GPU tensor")
        return ops.sphere_points_sample_f32(x.contiguous(), rec, interp, out)
    res = sample_torch(x, rec, interp)
    if out is not None:
        out.copy_(res)
        return out
    return res


def _check_pair(x, y):
    if x.dim() != 4 or y.dim() != 4 or x.shape[:2] != y.shape[:2] or x.device != y.device:
        raise PconvError("sphere points: two batches of equal n and C on one device expected (any two sizes), got %s on %s "
                         "and %s on %s" % (tuple(x.shape), x.device, tuple(y.shape), y.device))


def mse_records_torch(x, rec_x, y, rec_y, interp="lanczos"):
    """float64 (n, C) on the frames' device: the definition in torch on given records -- both samples by sample_torch,
    the difference and its square in float32, torch's float64 sum over the points, divided by P.  Any summation order
    of these non-negative terms is within (P - 1) 2^-53 relative of the exact sum, so this and the kernel's fixed order
    differ by at most 2 (P - 1) 2^-53 relative"""
    d = sample_torch(x, rec_x, interp) - sample_torch(y, rec_y, interp)
    return (d * d).double().sum(dim=2) / rec_x.shape[0]


def mse_torch(x, y, pointset, interp="lanczos"):
    """float64 CPU tensor (n, C): `mse` by the torch twin, on the frames' device"""
    _check_interp(interp)
    x, y = _as_planes(x), _as_planes(y)
    _check_pair(x, y)
    ps = _pointset(pointset)
    return mse_records_torch(x, ps.records(x.shape[2], x.shape[3], x.device), y, ps.records(y.shape[2], y.shape[3], y.device),
                             interp).cpu()


def mse(x, y, pointset, interp="lanczos"):
    """float64 CPU tensor (n, C): per frame and channel the mean over the points of (a - b)^2, a the sample of x and b
    the sample of y at the same point of the sphere.  x and y: equal n and C, ANY two sizes, float32 (n, C, h, w) or
    uint8 (n, h, w, 3).  GPU tensors: the fused HIP kernel (the sum in the fixed order of include/pconv_hip.h: the same
    bits for a frame alone, anywhere in a batch, on any call); CPU tensors: mse_torch"""
    _check_interp(interp)
    x, y = _as_planes(x), _as_planes(y)
    _check_pair(x, y)
    if not x.is_cuda:
        return mse_torch(x, y, pointset, interp)
    ops = backend.ops()
    if not hasattr(ops, "sphere_points_mse"):
        raise PconvError("sphere points: the active backend has no sphere_points_mse kernel for a GPU tensor")
    ps = _pointset(pointset)
    return ops.sphere_points_mse(x.contiguous(), ps.records(x.shape[2], x.shape[3], x.device), y.contiguous(),
                                 ps.records(y.shape[2], y.shape[3], y.device), interp)


@functools.lru_cache(maxsize=2)
def icosphere_set(level=LEVEL):
    """the cached PointSet of icosphere(level)"""
    return PointSet(icosphere(level))


@functools.lru_cache(maxsize=2)
def cpp_set(h, w):
    """the cached PointSet of cpp_grid(h, w)"""
    return PointSet(cpp_grid(h, w))


def psnr_of(values):
    """float64 (n,) dB of float64 (n, C) MSE values: 10 log10(1 / mean over the channels), +inf for 0"""
    return sphere_metrics.psnr(values.mean(dim=1))


def s_psnr_nn(x, y, level=LEVEL):
    """float64 (n,) S-PSNR-NN in dB of each frame: icosphere(level), the nearest pixel of each picture"""
    return psnr_of(mse(x, y, icosphere_set(int(level)), "nearest"))


def s_psnr_i(x, y, level=LEVEL):
    """float64 (n,) S-PSNR-I in dB of each frame: icosphere(level), this project's 6 x 6 Lanczos-3 sampler"""
    return psnr_of(mse(x, y, icosphere_set(int(level)), "lanczos"))


def cpp_psnr(x, y, size=None):
    """float64 (n,) CPP-PSNR in dB of each frame: both pictures read with the Lanczos-3 sampler at the valid pixels of a
    Craster parabolic picture of size = (h, w), by default picture x's size"""
    if size is None:
        size = x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:]
    return psnr_of(mse(x, y, cpp_set(int(size[0]), int(size[1])), "lanczos"))
