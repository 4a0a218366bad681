"""Cubemap panoramas, CMP and EAC: cube <-> ERP on the sphere sampler (include/pconv_hip.h, pconv_cube_from_erp_map /
pconv_cube_pad_f32 / pconv_cube_to_erp_map; csrc/cube.hip).

Axes are erp_rotate.py's: the picture centre is (1, 0, 0), right is +y, up is +z.  The six faces, in this order, with
forward, right and up (`FACES`): F +x, R +y, B -x, L -y (up +z, right the next face's forward in yaw order), U +z and D -z
(the edge shared with F is U's bottom edge and D's top edge).  A face of a x a pixels has face coordinates s = 2 (c + 1/2)
/ a - 1, t = 1 - 2 (r + 1/2) / a at pixel centres; the plane coordinate is p = s for "cmp" and p = tan(pi/4 s) for "eac"
(inverse s = 4/pi atan(p)); the direction is forward + p_s right + p_t up, all in float64.  The face of a direction is
the axis of largest magnitude, ties in the order x, y, z (`>=`), the sign picking the face (`face_of`).

Layouts are index permutations, done here in torch: "faces" (n, C, 6a, a), the stack in the order above, is what every
kernel sees; "6x1" the six faces side by side, unrotated; "3x2" a top row L F R unrotated over a bottom row D B U, D and
U turned a quarter counter-clockwise and B a quarter clockwise, so that each row is continuous across its two inner
edges.  The 3x2 layout is meant as the CMP / EAC frame packing of 360Lib; equality with 360Lib's packing is not claimed.

ERP -> cube (`from_erp`): one map (`from_erp_map`: the record, in 1/256 pixel, of every sample of the face stack on the
ERP source) and viewport's renderer on it, the 6 x 6 Lanczos-3 sampler with an ss x ss average; an ss x ss block never
leaves its face.  Cube -> ERP (`to_erp`): the faces are first continued by PAD = 3 pixels across their edges (`pad`: the
ring read bilinearly from the neighbouring faces through `pad_table`, one level deep), then a second map (`to_erp_map`:
the record of every ERP sample on the padded stack seen as one plane of 6A x A, A = a + 6) and the same renderer; every
footprint stays inside its own padded face.  ss defaults to the source pixels per output pixel at the face centre / the
equator, at most 4; beyond 4 the source is to be reduced first (erp_resample.resize).

GPU tensors take the HIP kernels (PCONV.cube_*, PCONV.viewport_render_f32), CPU tensors the torch twins below
(`pad_torch`, viewport.render_torch): the same bits on the same map and table.  `from_erp` of a tensor that requires grad
goes through viewport's Function (the ordered backward of pconv_remap_backward_f32: the map is generic); `to_erp` under
autograd is refused unless grad=True is passed: then the continuation is `pad(.., grad=True)`, whose backward
`pad_backward` is the adjoint of the continuation as an ordered gather (pconv_cube_pad_backward_f32 over
`pad_reverse_lists`; `pad_backward_torch` is its twin, the same bits), and the renderer is viewport's Function again.

Scoring (the last section of this module): `area_weights` is the solid angle of every pixel of a cube
picture, `ws_mse` / `ws_psnr` / `ws_loss_terms` weigh two cube pictures by it (weighted_metrics.py), and `point_records` puts
the points of a sphere_points.PointSet on the padded stack, so that `points_mse`, `s_psnr_nn`, `s_psnr_i` and `cpp_psnr` read
cube and ERP pictures in any mix at the same points of the sphere, with no conversion in between.  `ws_ssim` is the
structural figure: every face continued by SSIM_PAD = 5 pixels, the radius of the SSIM window (`pad` takes a depth), and
the padded stacks scored by weighted_metrics.ssim with the ring weighted zero, so that a window at a face edge sees the
neighbouring face and no window of a weighted pixel reads outside its own padded face.  `ws_ssim_loss_terms` is the same
figure attached to autograd (pad(.., grad=True) and weighted_metrics.ssim_loss_terms): with `ws_loss_terms` the two terms
of train.py --loss cube-ws.

Limits.  The ring is bilinear and one level deep, so within 3 pixels of a face edge the way back reads a slightly softer
continuation than the sphere itself.  For "eac" the extended plane ends before its horizon: |s| and |t| of a ring pixel
are held at 7/4, which only faces of a <= 6 reach (at depth 5, ws_ssim's: a <= 11).  ss is chosen for the face centre /
the equator.  ws_ssim itself is forward only (ws_ssim_loss_terms carries the gradient, the SSIM's held to a bound, not
to the bit), has no multi-scale form, and claims no equality with 360Lib's figure.
"""
import collections
import functools
import math

import numpy as np
import torch

from . import erp_rotate, viewport
from ._native import PconvError
from .PCONV_operator import backend

PHASES = erp_rotate.PHASES
KINDS = {"cmp": 1, "eac": 2}        # PCONV_CUBE_CMP, PCONV_CUBE_EAC: the container's code too
LAYOUTS = {"faces": 0, "6x1": 1, "3x2": 2}   # the container's code
PAD = 3                             # PCONV_CUBE_PAD: the continuation of the way back to ERP and of the point records
SSIM_PAD = 5                        # the continuation of ws_ssim: the radius of the 11-tap SSIM window
MAX_DEPTH = 8                       # PCONV_CUBE_MAX_DEPTH
MAX_FACE = 9453                     # PCONV_CUBE_MAX_FACE: 24 (a + 6)^2 < 2^31
MAX_SS = viewport.MAX_SS
RING_LIMIT = 1.75                   # |s|, |t| of an "eac" ring pixel are held here (depth 3: faces of a <= 6; 5: a <= 11)
FACE_NAMES = "FRBLUD"
# (6, 3, 3): forward, right, up of each face
FACES = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]],
                  [[0, 1, 0], [-1, 0, 0], [0, 0, 1]],
                  [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],
                  [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
                  [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                  [[0, 0, -1], [0, 1, 0], [1, 0, 0]]], dtype=np.float64)
FACES.setflags(write=False)

Spec = collections.namedtuple("Spec", "kind layout")


def spec(kind, layout="3x2"):
    """the checked, hashable description of a cube picture: Spec(kind, layout), kind "cmp" or "eac", layout "faces",
    "6x1" or "3x2".  A Spec passes through"""
    if isinstance(kind, Spec):
        kind, layout = kind
    if kind not in KINDS:
        raise PconvError("cube: kind must be one of %s, got %r" % (sorted(KINDS), kind))
    if layout not in LAYOUTS:
        raise PconvError("cube: layout must be one of %s, got %r" % (sorted(LAYOUTS), layout))
    return Spec(kind, layout)


def _spec(sp, layout=None):
    sp = sp if isinstance(sp, Spec) else Spec(sp, "3x2")
    return spec(sp.kind, sp.layout if layout is None else layout)


def _kind(kind):
    if isinstance(kind, Spec):
        kind = kind.kind
    if kind not in KINDS:
        raise PconvError("cube: kind must be one of %s, got %r" % (sorted(KINDS), kind))
    return kind


def check_face(a):
    if int(a) != a or not 2 <= int(a) <= MAX_FACE:
        raise PconvError("cube: a face size of %r is outside 2 .. %d" % (a, MAX_FACE))
    return int(a)


def _check_ss(ss):
    if int(ss) != ss or not 1 <= int(ss) <= MAX_SS:
        raise PconvError("cube: ss = %r supersampling is outside 1 .. %d" % (ss, MAX_SS))
    return int(ss)


def _check_erp(h, w):
    try:
        return erp_rotate._check_size(h, w)
    except PconvError as exc:
        raise PconvError(str(exc).replace("erp rotate:", "cube: the ERP frame:"))


def erp_size(a):
    """(2a, 4a): the ERP size whose equator has the pixel density of the face centres' ring"""
    a = check_face(a)
    return 2 * a, 4 * a


def face_size(h, w):
    """round(w / 4), at least 2"""
    return max(2, int(math.floor(int(w) / 4.0 + 0.5)))


def picture_size(a, layout):
    """(height, width) of a cube picture of face size a in `layout`"""
    a = check_face(a)
    return {"faces": (6 * a, a), "6x1": (a, 6 * a), "3x2": (2 * a, 3 * a)}[spec("cmp", layout).layout]


def face_size_of(shape, layout):
    """the face size of a cube picture of `shape` = (.., height, width) in `layout`; PconvError when it is none"""
    layout = spec("cmp", layout).layout
    hh, ww = int(shape[-2]), int(shape[-1])
    a = {"faces": ww, "6x1": hh, "3x2": hh // 2}[layout]
    if a < 2 or picture_size(a, layout) != (hh, ww):
        raise PconvError("cube: a picture of %dx%d is no %r layout of square faces" % (ww, hh, layout))
    return a


# ---- geometry: float64 numpy ----

def plane_of(kind, s):
    return np.tan((np.pi / 4.0) * s) if _kind(kind) == "eac" else s


def face_of_plane(kind, p):
    return (4.0 / np.pi) * np.arctan(p) if _kind(kind) == "eac" else p


def direction(kind, face, s, t):
    """float64 (3, ...): forward + p_s right + p_t up of face(s) `face` at face coordinates s, t (not normalised)"""
    face = np.asarray(face)
    ps, pt = plane_of(kind, np.asarray(s, dtype=np.float64)), plane_of(kind, np.asarray(t, dtype=np.float64))
    fr = FACES[face]                                   # (..., 3, 3)
    return np.stack([fr[..., 0, k] + ps * fr[..., 1, k] + pt * fr[..., 2, k] for k in range(3)])


def face_of(d):
    """the face of direction(s) d (3, ...): the axis of largest magnitude, ties in the order x, y, z; the sign picks"""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in d)
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    return np.where((ax >= ay) & (ax >= az), np.where(x >= 0.0, 0, 2),
                    np.where(ay >= az, np.where(y >= 0.0, 1, 3), np.where(z >= 0.0, 4, 5)))


def tie_margin(d):
    """how far, relative to the largest magnitude, direction(s) d lie from a face tie"""
    m = np.sort(np.abs(np.stack([np.asarray(v, dtype=np.float64) for v in d])), axis=0)
    return (m[2] - m[1]) / m[2]


def face_st(kind, d, face=None):
    """(g, s, t): the face direction(s) d fall on (or `face`) and the face coordinates there"""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in d)
    g = face_of((x, y, z)) if face is None else np.asarray(face)
    fr = FACES[g]
    dot = lambda k: x * fr[..., k, 0] + y * fr[..., k, 1] + z * fr[..., k, 2]
    along = dot(0)
    return g, face_of_plane(kind, dot(1) / along), face_of_plane(kind, dot(2) / along)


def face_position(kind, a, d):
    """(g, u', v'): the face of d and the position on it in pixels, u' = (s + 1) a / 2 - 1/2, v' = (1 - t) a / 2 - 1/2"""
    g, s, t = face_st(kind, d)
    return g, (s + 1.0) * a / 2.0 - 0.5, (1.0 - t) * a / 2.0 - 0.5


def face_grid(kind, a, ss=1):
    """float64 (3, 6 a ss, a ss): the direction of every sample of the face stack's grid"""
    gs = check_face(a) * _check_ss(ss)
    s = (2.0 * (np.arange(gs, dtype=np.float64) + 0.5) / gs - 1.0)[None, :]
    t = (1.0 - 2.0 * (np.arange(gs, dtype=np.float64) + 0.5) / gs)[:, None]
    return np.concatenate([direction(kind, f, s, t) for f in range(6)], axis=1)


def erp_coordinates(d, h, w):
    """(u, v) float64: the column and row, in pixels of an h x w ERP frame, of direction(s) d (the rule before its
    quantisation; erp_rotate.py's)"""
    sx, sy, sz = d
    u = (np.arctan2(sy, sx) / (2.0 * np.pi) + 0.5) * w - 0.5
    v = (0.5 - np.arctan2(sz, np.hypot(sx, sy)) / np.pi) * h - 0.5
    return u, v


def from_erp_coordinates(kind, a, ss, h, w):
    """(u, v) float64 (6 a ss, a ss): where on the h x w ERP source each sample of the face stack reads"""
    h, w = _check_erp(h, w)
    return erp_coordinates(face_grid(kind, a, ss), h, w)


def from_erp_map_numpy(kind, a, ss, h, w):
    """the ERP -> cube map in float64 on the host: int32 (6 a ss, a ss, 2) records of erp_rotate.py's form"""
    u, v = from_erp_coordinates(kind, a, ss, h, w)
    qu = np.mod(np.rint(u * PHASES).astype(np.int64), int(w) * PHASES)
    qv = np.rint(v * PHASES).astype(np.int64)
    return np.stack([qu, qv], axis=2).astype(np.int32)


def erp_grid(gh, gw):
    """float64 (3, gh, gw): the direction of every pixel of a gh x gw ERP frame (erp_rotate.py's)"""
    theta = ((np.arange(gw, dtype=np.float64) + 0.5) / gw - 0.5) * (2.0 * np.pi)
    phi = (0.5 - (np.arange(gh, dtype=np.float64) + 0.5) / gh) * np.pi
    cp, sp = np.cos(phi)[:, None], np.sin(phi)[:, None]
    return np.stack([cp * np.cos(theta)[None, :], cp * np.sin(theta)[None, :], sp * np.ones((1, gw))])


def to_erp_coordinates(kind, a, h, w, ss):
    """(g, u', v') of every sample of the (h ss) x (w ss) ERP grid: its face and the position there, clamped to
    [-1/2, a - 1/2]"""
    a, ss = check_face(a), _check_ss(ss)
    h, w = _check_erp(h, w)
    g, u, v = face_position(kind, a, erp_grid(h * ss, w * ss))
    return g, np.clip(u, -0.5, a - 0.5), np.clip(v, -0.5, a - 0.5)


def to_erp_map_numpy(kind, a, h, w, ss):
    """the cube -> ERP map in float64 on the host: int32 (h ss, w ss, 2), qu = rint((u' + 3) 256), qv = rint((v' + 3 +
    g A) 256) on the padded stack seen as one plane of 6A x A"""
    g, u, v = to_erp_coordinates(kind, a, h, w, ss)
    A = int(a) + 2 * PAD
    qu = np.rint((u + PAD) * PHASES).astype(np.int64)
    qv = np.rint((v + PAD + g.astype(np.float64) * A) * PHASES).astype(np.int64)
    return np.stack([qu, qv], axis=2).astype(np.int32)


def check_depth(a, depth=PAD):
    """the checked (a, depth) of a continuation: depth in 1 .. MAX_DEPTH, the padded stack 24 (a + 2 depth)^2 below 2^31
    bytes"""
    a = check_face(a)
    if int(depth) != depth or not 1 <= int(depth) <= MAX_DEPTH:
        raise PconvError("cube: a depth of %r is outside 1 .. %d" % (depth, MAX_DEPTH))
    if 24 * (a + 2 * int(depth)) ** 2 >= 1 << 31:
        raise PconvError("cube: a face size of %d continued by %d: the padded stack is 2^31 bytes or more" % (a, depth))
    return a, int(depth)


def ring_pixels(a, depth=PAD):
    """(R, Q) int64 arrays of 4 depth (a + depth) elements (12 a + 36 at depth 3): the pixels of a padded face outside
    its interior, in ring order (row after row, column after column)"""
    a, depth = check_depth(a, depth)
    A = a + 2 * depth
    outside = np.ones((A, A), dtype=bool)
    outside[depth:depth + a, depth:depth + a] = False
    return np.nonzero(outside)


def ring_directions(kind, a, depth=PAD):
    """float64 (3, 6, 4 depth (a + depth)): the direction of every ring pixel, on its own face's extended plane"""
    R, Q = ring_pixels(a, depth)
    s = 2.0 * ((Q - depth) + 0.5) / a - 1.0
    t = 1.0 - 2.0 * ((R - depth) + 0.5) / a
    if _kind(kind) == "eac":
        s, t = np.clip(s, -RING_LIMIT, RING_LIMIT), np.clip(t, -RING_LIMIT, RING_LIMIT)
    return np.stack([direction(kind, f, s, t) for f in range(6)], axis=1)


def ring_coordinates(kind, a, depth=PAD):
    """(g, u', v') (6, 4 depth (a + depth)): the face each ring pixel's direction falls on and the position there, clamped
    to [0, a - 1]"""
    g, u, v = face_position(kind, a, ring_directions(kind, a, depth))
    return g, np.clip(u, 0.0, a - 1.0), np.clip(v, 0.0, a - 1.0)


@functools.lru_cache(maxsize=8)
def _pad_table(kind, a, depth=PAD):
    g, u, v = ring_coordinates(kind, a, depth)
    table = np.stack([g, np.rint(u * PHASES).astype(np.int64), np.rint(v * PHASES).astype(np.int64)], axis=2)
    table = np.ascontiguousarray(table.reshape(-1, 3).astype(np.int32))
    table.setflags(write=False)
    return table


def pad_table(kind, a, depth=PAD):
    """int32 (6 (A^2 - a^2), 3), A = a + 2 depth, read-only: (g, qu, qv) of every ring pixel, face after face in ring
    order, built in float64 on the host.  Cached per (kind, a, depth)"""
    return _pad_table(_kind(kind), *check_depth(a, depth))


@functools.lru_cache(maxsize=4)
def _pad_table_on(kind, a, device, depth=PAD):
    return torch.from_numpy(np.array(_pad_table(kind, a, depth))).to(device)


def _device(device):
    device = torch.device("cpu" if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def pad_table_on(kind, a, device=None, depth=PAD):
    """pad_table as a tensor on `device`, uploaded once (the last 4 kept); do not write to it"""
    a, depth = check_depth(a, depth)
    return _pad_table_on(_kind(kind), a, str(_device(device)), depth)


# ---- layouts ----

def _check_stack(y, what="cube"):
    if y.dim() != 4 or y.dtype != torch.float32 or y.shape[2] != 6 * y.shape[3]:
        raise PconvError("%s: a float32 face stack (n, C, 6a, a) expected, got %s %s" % (what, y.dtype, tuple(y.shape)))
    return check_face(y.shape[3])


def pack(faces, layout):
    """the face stack (n, C, 6a, a) in `layout`: "faces" itself, "6x1" (n, C, a, 6a), "3x2" (n, C, 2a, 3a)"""
    layout = spec("cmp", layout).layout
    a = _check_stack(faces)
    if layout == "faces":
        return faces
    F, R, B, L, U, D = (faces[:, :, k * a:(k + 1) * a] for k in range(6))
    if layout == "6x1":
        return torch.cat([F, R, B, L, U, D], dim=3)
    bottom = torch.cat([torch.rot90(D, 1, (2, 3)), torch.rot90(B, -1, (2, 3)), torch.rot90(U, 1, (2, 3))], dim=3)
    return torch.cat([torch.cat([L, F, R], dim=3), bottom], dim=2)


def unpack(y, layout):
    """the face stack (n, C, 6a, a) of a cube picture in `layout`: the inverse of `pack`"""
    layout = spec("cmp", layout).layout
    if y.dim() != 4 or y.dtype != torch.float32:
        raise PconvError("cube: a float32 (n, C, height, width) picture expected, got %s %s" % (y.dtype, tuple(y.shape)))
    a = face_size_of(y.shape, layout)
    if layout == "faces":
        return y
    if layout == "6x1":
        return torch.cat([y[:, :, :, k * a:(k + 1) * a] for k in range(6)], dim=2)
    top, bottom = y[:, :, :a], y[:, :, a:]
    L, F, R = (top[:, :, :, k * a:(k + 1) * a] for k in range(3))
    D, B, U = (torch.rot90(bottom[:, :, :, k * a:(k + 1) * a], q, (2, 3)) for k, q in ((0, -1), (1, 1), (2, -1)))
    return torch.cat([F, R, B, L, U, D], dim=2)


# ---- maps on a device ----

@functools.lru_cache(maxsize=4)
def _from_erp_map(kind, a, ss, h, w, device):
    device = torch.device(device)
    if device.type == "cuda":
        ops = backend.ops()
        if not hasattr(ops, "cube_from_erp_map"):
            raise PconvError("cube: the active backend has no cube_from_erp_map kernel for a GPU device")
        return ops.cube_from_erp_map(kind, a, ss, h, w, device)
    return torch.from_numpy(from_erp_map_numpy(kind, a, ss, h, w))


@functools.lru_cache(maxsize=4)
def _to_erp_map(kind, a, h, w, ss, device):
    device = torch.device(device)
    if device.type == "cuda":
        ops = backend.ops()
        if not hasattr(ops, "cube_to_erp_map"):
            raise PconvError("cube: the active backend has no cube_to_erp_map kernel for a GPU device")
        return ops.cube_to_erp_map(kind, a, h, w, ss, device)
    return torch.from_numpy(to_erp_map_numpy(kind, a, h, w, ss))


@functools.lru_cache(maxsize=4)
def _reverse_lists(kind, a, ss, h, w, device):
    return viewport.reverse_lists(_from_erp_map(kind, a, ss, h, w, device), h, w)


def _check_map_size(gh, gw):
    if 8 * gh * gw >= 1 << 31:
        raise PconvError("cube: a map of %dx%d records is 2^31 bytes or more" % (gw, gh))


def from_erp_map(kind, a, ss, h, w, device=None):
    """int32 (6 a ss, a ss, 2) on `device`: the HIP kernel for a GPU device, from_erp_map_numpy on the CPU (the two agree
    except where a position lies within the evaluation error of a rounding boundary).  The last 4 maps are kept; do not
    write to it"""
    kind, a, ss = _kind(kind), check_face(a), _check_ss(ss)
    h, w = _check_erp(h, w)
    _check_map_size(6 * a * ss, a * ss)
    return _from_erp_map(kind, a, ss, h, w, str(_device(device)))


def to_erp_map(kind, a, h, w, ss, device=None):
    """int32 (h ss, w ss, 2) on `device`, on the padded stack: the HIP kernel for a GPU device, to_erp_map_numpy on the
    CPU (equal away from rounding boundaries and face ties).  The last 4 maps are kept; do not write to it"""
    kind, a, ss = _kind(kind), check_face(a), _check_ss(ss)
    h, w = _check_erp(h, w)
    _check_map_size(h * ss, w * ss)
    return _to_erp_map(kind, a, h, w, ss, str(_device(device)))


# ---- the face continuation ----

def pad_torch(y, table, depth=PAD):
    """the face continuation in torch, float32 operation by operation, on any device (the CPU path and the kernel's
    twin): the face stack (n, C, 6a, a) and the int32 (6 (A^2 - a^2), 3) table of `depth` -> (n, C, 6A, A), A = a + 2 depth"""
    a, depth = check_depth(_check_stack(y, "cube pad"), depth)
    A = a + 2 * depth
    ring = A * A - a * a
    if table.dtype != torch.int32 or tuple(table.shape) != (6 * ring, 3) or table.device != y.device:
        raise PconvError("cube pad: the table must be int32 (%d, 3) on the faces' device, got %s %s on %s"
                         % (6 * ring, table.dtype, tuple(table.shape), table.device))
    n, c = y.shape[:2]
    out = torch.zeros((n, c, 6, A, A), dtype=torch.float32, device=y.device)
    out[:, :, :, depth:depth + a, depth:depth + a] = y.reshape(n, c, 6, a, a)
    rec = table.long()
    g = rec[:, 0].clamp(0, 5)
    x0, y0 = (rec[:, 1] >> 8).clamp(0, a - 1), (rec[:, 2] >> 8).clamp(0, a - 1)
    x1, y1 = (x0 + 1).clamp(max=a - 1), (y0 + 1).clamp(max=a - 1)
    fx, fy = (rec[:, 1] & (PHASES - 1)).float() / PHASES, (rec[:, 2] & (PHASES - 1)).float() / PHASES
    r0, r1 = g * a + y0, g * a + y1
    x00, x01, x10, x11 = y[:, :, r0, x0], y[:, :, r0, x1], y[:, :, r1, x0], y[:, :, r1, x1]
    top = x00 + fx * (x01 - x00)
    bot = x10 + fx * (x11 - x10)
    value = top + fy * (bot - top)
    R, Q = (torch.from_numpy(v).to(y.device) for v in ring_pixels(a, depth))
    face = torch.arange(6, device=y.device).repeat_interleave(ring)
    out[:, :, face, R.repeat(6), Q.repeat(6)] = value
    return out.reshape(n, c, 6 * A, A)


def pad_numpy(y, table, depth=PAD):
    """pad_torch in numpy, float32 operation by operation: a float32 array (n, C, 6a, a) and the int32 table of `depth`
    -> (n, C, 6A, A)"""
    y, rec = np.asarray(y, dtype=np.float32), np.asarray(table).astype(np.int64)
    n, c, _, a = y.shape
    a, depth = check_depth(a, depth)
    A = a + 2 * depth
    out = np.zeros((n, c, 6, A, A), dtype=np.float32)
    out[:, :, :, depth:depth + a, depth:depth + a] = y.reshape(n, c, 6, a, a)
    g = np.clip(rec[:, 0], 0, 5)
    x0, y0 = np.clip(rec[:, 1] >> 8, 0, a - 1), np.clip(rec[:, 2] >> 8, 0, a - 1)
    x1, y1 = np.minimum(x0 + 1, a - 1), np.minimum(y0 + 1, a - 1)
    fx = (rec[:, 1] & (PHASES - 1)).astype(np.float32) / np.float32(PHASES)
    fy = (rec[:, 2] & (PHASES - 1)).astype(np.float32) / np.float32(PHASES)
    r0, r1 = g * a + y0, g * a + y1
    top = y[:, :, r0, x0] + fx * (y[:, :, r0, x1] - y[:, :, r0, x0])
    bot = y[:, :, r1, x0] + fx * (y[:, :, r1, x1] - y[:, :, r1, x0])
    R, Q = ring_pixels(a, depth)
    out[:, :, np.repeat(np.arange(6), R.size), np.tile(R, 6), np.tile(Q, 6)] = top + fy * (bot - top)
    return out.reshape(n, c, 6 * A, A)


@functools.lru_cache(maxsize=4)
def _pad_reverse_lists(kind, a, depth, device):
    from . import _native
    table = np.ascontiguousarray(_pad_table(kind, a, depth))
    count = _native.call("pconv_host_cube_pad_reverse_size", a, depth)
    start, entry = np.empty(6 * a * a + 1, dtype=np.int32), np.empty(count, dtype=np.int32)
    _native.call("pconv_host_cube_pad_reverse", table.ctypes.data, a, depth, start.ctypes.data, entry.ctypes.data)
    return torch.from_numpy(start).to(device), torch.from_numpy(entry).to(device)


def pad_reverse_lists(kind, a, depth=PAD, device=None):
    """(start, entry): the transpose of the face continuation as one list per pixel of the face stack, int32 tensors of
    6 a^2 + 1 and 24 (A^2 - a^2) elements on `device` (pconv_host_cube_pad_reverse: entry e = 4 ring_index + corner,
    ascending within each list).  Built on the host from pad_table, once per (kind, a, depth) and device (the last 4 kept);
    do not write to them"""
    a, depth = check_depth(a, depth)
    return _pad_reverse_lists(_kind(kind), a, depth, str(_device(device)))


def _check_padded(g, a, depth, what="cube pad backward"):
    a, depth = check_depth(a, depth)
    A = a + 2 * depth
    if not torch.is_tensor(g) or g.dim() != 4 or g.dtype != torch.float32 or tuple(g.shape[2:]) != (6 * A, A):
        raise PconvError("%s: a float32 gradient (n, C, %d, %d) of the padded stack expected, got %s"
                         % (what, 6 * A, A, "%s %s" % (g.dtype, tuple(g.shape)) if torch.is_tensor(g) else type(g).__name__))
    return a, depth, A


def pad_backward_torch(g, table, lists, a, depth=PAD):
    """the gradient of pad_torch with respect to the face stack, in the order of include/pconv_hip.h
    (pconv_cube_pad_backward_f32), float32 operation by operation on any device (the CPU path and the kernel's twin):
    float32 (n, C, 6A, A), the table the forward read and its `pad_reverse_lists` -> (n, C, 6a, a).  Every pixel has one
    accumulator that starts from the gradient of its own interior copy; the terms g_ring * coef of its list are added
    front to back, coef = float(cx cy) 2^-16 with cx = px or 256 - px, cy = py or 256 - py by the entry's corner.
    Vectorised in rounds: round k adds the k-th entry of every list that has one"""
    a, depth, A = _check_padded(g, a, depth)
    ring = A * A - a * a
    if table.dtype != torch.int32 or tuple(table.shape) != (6 * ring, 3) or table.device != g.device:
        raise PconvError("cube pad backward: the table must be int32 (%d, 3) on the gradient's device, got %s %s on %s"
                         % (6 * ring, table.dtype, tuple(table.shape), table.device))
    start, entry = (t.to(g.device).long() for t in lists)
    if start.numel() != 6 * a * a + 1 or entry.numel() != 24 * ring:
        raise PconvError("cube pad backward: the lists are not those of a face size of %d at depth %d" % (a, depth))
    n, c = g.shape[:2]
    g5 = g.reshape(n, c, 6, A, A)
    acc = g5[:, :, :, depth:depth + a, depth:depth + a].reshape(n, c, 6 * a * a).clone()
    R, Q = (torch.from_numpy(v).to(g.device) for v in ring_pixels(a, depth))
    face = torch.arange(6, device=g.device).repeat_interleave(ring)
    at_ring = g5[:, :, face, R.repeat(6), Q.repeat(6)]               # (n, C, 6 ring): gout at ring pixel i
    rec = table.long()
    px, py = rec[:, 1] & (PHASES - 1), rec[:, 2] & (PHASES - 1)
    length = start[1:] - start[:-1]
    alive = torch.nonzero(length > 0).flatten()      # the destinations that still have an entry in round k
    k = 0
    while alive.numel():
        e = entry[start[alive] + k]
        i, corner = e >> 2, e & 3
        cx = torch.where((corner & 1) != 0, px[i], PHASES - px[i])
        cy = torch.where((corner & 2) != 0, py[i], PHASES - py[i])
        coef = (cx * cy).float() * torch.tensor(np.float32(1.0 / (PHASES * PHASES)), device=g.device)
        acc[:, :, alive] = acc[:, :, alive] + at_ring[:, :, i] * coef
        k += 1
        alive = alive[length[alive] > k]
    return acc.reshape(n, c, 6 * a, a)


def pad_backward(g, kind, a, depth=PAD):
    """float32 (n, C, 6a, a): the gradient of `pad` with respect to the face stack, from the gradient g (n, C, 6A, A) of the
    padded stack: the adjoint of the continuation in the order of include/pconv_hip.h.  The HIP kernel for GPU tensors
    (pconv_cube_pad_backward_f32: a gather over `pad_reverse_lists`, no atomics), pad_backward_torch for CPU tensors: the
    same bits"""
    kind = _kind(kind)
    a, depth, _ = _check_padded(g, a, depth)
    table = _pad_table_on(kind, a, str(g.device), depth)
    lists = _pad_reverse_lists(kind, a, depth, str(g.device))
    if g.is_cuda:
        from . import _metric_ops
        return _metric_ops.cube_pad_backward(g.contiguous(), table, lists, a, depth)
    return pad_backward_torch(g, table, lists, a, depth)


class _Pad(torch.autograd.Function):
    """`pad` under autograd (pad(.., grad=True)): the forward as it is, the backward `pad_backward`, on either device"""

    @staticmethod
    def forward(ctx, y, kind, depth):
        ctx.kind, ctx.depth, ctx.a = kind, depth, y.shape[3]
        return pad(y, kind, depth)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return pad_backward(g.contiguous(), ctx.kind, ctx.a, ctx.depth), None, None


def pad(y, kind, depth=PAD, grad=False):
    """the face stack (n, C, 6a, a) continued by `depth` pixels (1 .. MAX_DEPTH, by default PAD) across every face edge:
    (n, C, 6A, A), A = a + 2 depth.  The HIP kernel for GPU tensors (pconv_cube_pad_f32 at depth PAD, otherwise
    pconv_cube_pad_depth_f32), pad_torch for CPU tensors: the same bits.  grad=True attaches the result to autograd: the
    same values, and `pad_backward` as the backward (its lists built at the first backward and cached like the table)"""
    kind = _kind(kind)
    a, depth = check_depth(_check_stack(y, "cube pad"), depth)
    if grad:
        return _Pad.apply(y, kind, depth)
    table = _pad_table_on(kind, a, str(y.device), depth)
    if y.is_cuda and depth != PAD:
        from . import _metric_ops
        return _metric_ops.cube_pad_depth(y.contiguous(), table, depth)
    if y.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "cube_pad_f32"):
            raise PconvError("cube: the active backend has no cube_pad_f32 kernel for a GPU tensor")
        return ops.cube_pad_f32(y.contiguous(), table)
    return pad_torch(y, table, depth)


# ---- the conversions ----

def _render(x, map, vh, vw, ss, clamp):
    if x.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "viewport_render_f32"):
            raise PconvError("cube: the active backend has no viewport_render_f32 kernel for a GPU tensor")
        return ops.viewport_render_f32(x.contiguous(), map, vh, vw, ss, clamp)[:, 0]
    return viewport.render_torch(x, map, vh, vw, ss, clamp)


def _default_ss(ratio, what, sizes):
    if ratio > MAX_SS:
        raise PconvError("cube: %s covers %.2f source pixels per pixel, more than %d: reduce the source first with "
                         "erp_resample.resize" % (what % sizes, ratio, MAX_SS))
    return min(MAX_SS, max(1, int(math.ceil(ratio - 1e-9))))


def from_erp_ss(a, h, w):
    """the default supersampling of from_erp: clamp(ceil(w / (4a) - 1e-9), 1, 4); a ratio above 4 is refused"""
    return _default_ss(w / (4.0 * a), "a face of %d from a %dx%d ERP frame", (a, w, h))


def to_erp_ss(a, h, w):
    """the default supersampling of to_erp: clamp(ceil(4a / w - 1e-9), 1, 4); a ratio above 4 is refused"""
    return _default_ss(4.0 * a / w, "a %dx%d ERP frame from faces of %d", (w, h, a))


def from_erp(x, a=None, spec="cmp", ss=None, clamp=False, layout=None):
    """float32 (n, C, h, w) ERP frames -> the cube picture of face size a (default face_size(h, w)) in the spec's layout
    (`spec`: a Spec or a kind; layout= overrides its layout).  ss=None: from_erp_ss.  clamp=True bounds the result to
    [0, 1].  The HIP kernels for GPU tensors, the twin on the CPU.  With grad mode on and x requiring a gradient the
    result is attached to autograd through viewport's Function: the ordered backward of pconv_remap_backward_f32, its
    lists built at the first backward and cached like the map"""
    sp = _spec(spec, layout)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise PconvError("cube: float32 (n, C, h, w) expected, got %s %s" % (x.dtype, tuple(x.shape)))
    h, w = _check_erp(*x.shape[2:])
    a = face_size(h, w) if a is None else check_face(a)
    ss = from_erp_ss(a, h, w) if ss is None else _check_ss(ss)
    map = from_erp_map(sp.kind, a, ss, h, w, x.device)
    if torch.is_grad_enabled() and x.requires_grad:
        key = (sp.kind, a, ss, h, w, str(map.device))
        views = [(map, lambda: _reverse_lists(*key), ss)]
        faces = viewport._Remap.apply(x, lambda t: _render(t, map, 6 * a, a, ss, False).unsqueeze(1), views, bool(clamp))[:, 0]
    else:
        faces = _render(x, map, 6 * a, a, ss, clamp)
    return pack(faces, sp.layout)


@functools.lru_cache(maxsize=4)
def _to_erp_reverse_lists(kind, a, h, w, ss, device):
    A = a + 2 * PAD
    return viewport.reverse_lists(_to_erp_map(kind, a, h, w, ss, device), 6 * A, A)


def to_erp(y, size=None, spec="cmp", ss=None, clamp=False, layout=None, grad=False):
    """a float32 cube picture in the spec's layout -> ERP frames (n, C, h, w) of `size` = (h, w), default erp_size(a).
    ss=None: to_erp_ss.  The HIP kernels for GPU tensors, the twins on the CPU.  A picture that requires grad is refused
    unless grad=True: the face continuation has no backward without the opt-in.  grad=True attaches the result to autograd
    through pad(.., grad=True) (pconv_cube_pad_backward_f32) and viewport's Function (pconv_remap_backward_f32 over the
    reverse lists of the to-ERP map on the padded stack seen as one 6A x A plane, built at the first backward and cached
    like the map): the same values, both backwards ordered"""
    sp = _spec(spec, layout)
    if not grad and torch.is_grad_enabled() and torch.is_tensor(y) and y.requires_grad:
        raise PconvError("cube: to_erp of a tensor that requires grad: the face continuation (pconv_cube_pad_f32) has no backward "
                         "without the opt-in; pass grad=True, detach the picture, or train on the ERP side")
    faces = unpack(y, sp.layout)
    a = _check_stack(faces)
    h, w = _check_erp(*(erp_size(a) if size is None else size))
    ss = to_erp_ss(a, h, w) if ss is None else _check_ss(ss)
    map = to_erp_map(sp.kind, a, h, w, ss, y.device)
    if grad and torch.is_grad_enabled() and y.requires_grad:
        key = (sp.kind, a, h, w, ss, str(map.device))
        views = [(map, lambda: _to_erp_reverse_lists(*key), ss)]
        padded = pad(faces.contiguous(), sp.kind, PAD, grad=True)
        return viewport._Remap.apply(padded, lambda t: _render(t, map, h, w, ss, False).unsqueeze(1), views, bool(clamp))[:, 0]
    return _render(pad(faces.contiguous(), sp.kind), map, h, w, ss, clamp)


# ---- scoring cube pictures on the sphere: area weights (WS-PSNR) and points of the sphere (S-PSNR, CPP-PSNR) ----
#
# Weights.  Pixel (r, c) of a face covers, on the face's plane, the rectangle between the edges p_c, p_c+1 and q_r, q_r+1,
# edge k at plane_of(kind, (2k - a) / a).  With F(p, q) = atan(p q / sqrt(1 + (p^2 + q^2))) its solid angle is
#   omega = (F(p1, q1) + F(p0, q0)) - (F(p0, q1) + F(p1, q0))
# -- the four-corner formula grouped so that the plane is symmetric under the eight symmetries of the square bit for bit (the
# edges are odd in k - a/2, F is odd in each argument and symmetric in the two): the plane is the same on all six faces and
# in every orientation a layout turns a face to.  rule="density" is the pointwise Jacobian at the pixel centre times the
# pixel's area (2/a)^2 in face coordinates: p'(s) p'(t) / (1 + p_s^2 + p_t^2)^(3/2), p' = 1 for "cmp" -- the (1 + d^2/r^2)^
# (-3/2) of the JVET WS-PSNR proposal -- and (pi/4)(1 + p^2) for "eac".  It is offered so that a figure can be compared with
# tools that use it; equality with 360Lib's figures is not claimed.
#
# Points.  `point_records` is the record of a point of the sphere on the padded stack (pconv_cube_points_records): with it
# sphere_points' fused kernel reads a cube picture on either side, with no conversion to ERP in between.

RULES = ("solid-angle", "density")


def _pack_numpy(stack, layout):
    """`pack` of one (6a, a) plane in numpy, any dtype"""
    a = stack.shape[1]
    if layout == "faces":
        return stack
    F, R, B, L, U, D = (stack[k * a:(k + 1) * a] for k in range(6))
    if layout == "6x1":
        return np.concatenate([F, R, B, L, U, D], axis=1)
    bottom = np.concatenate([np.rot90(D, 1), np.rot90(B, -1), np.rot90(U, 1)], axis=1)
    return np.concatenate([np.concatenate([L, F, R], axis=1), bottom], axis=0)


def face_weights(kind, a, rule="solid-angle"):
    """float64 (a, a): the weight of every pixel of one face (the same on all six)"""
    kind, a = _kind(kind), check_face(a)
    if rule not in RULES:
        raise PconvError("cube: rule must be one of %s, got %r" % (RULES, rule))
    if rule == "density":
        p = plane_of(kind, (2.0 * np.arange(a, dtype=np.float64) + 1.0 - a) / a)
        dp = (np.pi / 4.0) * (1.0 + p * p) if kind == "eac" else np.ones_like(p)
        return (dp[None, :] * dp[:, None]) / (1.0 + (p[None, :] ** 2 + p[:, None] ** 2)) ** 1.5 * (2.0 / a) ** 2
    e = plane_of(kind, (2.0 * np.arange(a + 1, dtype=np.float64) - a) / a)
    p, q = e[None, :], e[:, None]
    corner = np.arctan((p * q) / np.sqrt(1.0 + (p * p + q * q)))
    return (corner[1:, 1:] + corner[:-1, :-1]) - (corner[1:, :-1] + corner[:-1, 1:])


def area_weights(kind, a, layout="faces", rule="solid-angle"):
    """float64 numpy of picture_size(a, layout): the area on the sphere of every pixel of a cube picture -- its exact solid
    angle (the faces sum to 4 pi), or with rule="density" the Jacobian at its centre times (2/a)^2 -- laid out by the
    layout's own permutation"""
    layout = spec(kind, layout).layout
    return np.ascontiguousarray(_pack_numpy(np.tile(face_weights(kind, a, rule), (6, 1)), layout))


@functools.lru_cache(maxsize=8)
def _weight_plane(sp, a, rule):
    from . import weighted_metrics
    return weighted_metrics.WeightPlane(area_weights(sp.kind, a, sp.layout, rule))


def weight_plane(spec, a, rule="solid-angle"):
    """the cached weighted_metrics.WeightPlane of area_weights(spec.kind, a, spec.layout, rule)"""
    if rule not in RULES:
        raise PconvError("cube: rule must be one of %s, got %r" % (RULES, rule))
    return _weight_plane(_spec(spec), check_face(a), rule)


def _picture_face(x, sp):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise PconvError("cube: a 4-D batch of cube pictures expected")
    return face_size_of(x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:], sp.layout)


def ws_mse(x, y, spec):
    """float64 CPU tensor (n, C): the squared error of two cube pictures of one spec, every pixel weighted by its solid
    angle (weighted_metrics.mse on weight_plane(spec, a)).  float32 (n, C, height, width) or uint8 (n, height, width, 3)"""
    from . import weighted_metrics
    sp = _spec(spec)
    return weighted_metrics.mse(x, y, weight_plane(sp, _picture_face(x, sp)))


def ws_psnr(x, y, spec):
    """float64 (n,) WS-PSNR in dB of each cube picture: 10 log10(1 / mean over the channels of ws_mse)"""
    from . import weighted_metrics
    sp = _spec(spec)
    return weighted_metrics.psnr(x, y, weight_plane(sp, _picture_face(x, sp)))


def ws_loss_terms(x, y, spec):
    """float64 (n,) on the pictures' device, attached to autograd: the per-frame mean over the channels of ws_mse
    (weighted_metrics.loss_terms).  With from_erp's backward a model's ERP output is trained against a cube original:
    ws_loss_terms(from_erp(output, a, spec), original, spec)"""
    from . import weighted_metrics
    sp = _spec(spec)
    return weighted_metrics.loss_terms(x, y, weight_plane(sp, _picture_face(x, sp)))


# WS-SSIM.  An SSIM window is 11 x 11 pixels of a plane, and a cube picture is six planes that are neighbours on the
# sphere, not in any layout.  So both pictures are unpacked to face stacks and every face is continued by SSIM_PAD = 5
# pixels, the window's radius (`pad` at depth 5); the padded stacks (n, C, 6A, A), A = a + 10, are scored by
# weighted_metrics.ssim with a plane that holds face_weights in every interior and zero on every ring.  The ring is as deep
# as the window's radius, so the window of an interior pixel never leaves its own padded face: the zero padding of the
# plane's borders and the neighbouring face's ring in the stack are read by ring pixels' windows only, and those weigh
# zero.  What a window sees beyond a face edge is the neighbouring face, read bilinearly.

@functools.lru_cache(maxsize=8)
def _ssim_plane(kind, a, rule):
    from . import weighted_metrics
    A = a + 2 * SSIM_PAD
    plane = np.zeros((6, A, A), dtype=np.float64)
    plane[:, SSIM_PAD:SSIM_PAD + a, SSIM_PAD:SSIM_PAD + a] = face_weights(kind, a, rule)
    return weighted_metrics.WeightPlane(plane.reshape(6 * A, A))


def ssim_plane(kind, a, rule="solid-angle"):
    """the cached weighted_metrics.WeightPlane (6A, A), A = a + 2 SSIM_PAD, of ws_ssim: face_weights(kind, a, rule) in the
    interior of every padded face, zero on every ring"""
    if rule not in RULES:
        raise PconvError("cube: rule must be one of %s, got %r" % (RULES, rule))
    return _ssim_plane(_kind(kind), check_depth(a, SSIM_PAD)[0], rule)


def ws_ssim_planes(x, y, spec, rule="solid-angle"):
    """float64 CPU tensor (n, C): the WS-SSIM of every plane of two cube pictures of one spec and face size, float32 (n, C,
    height, width) or uint8 (n, height, width, 3): both unpacked to face stacks, every face continued by SSIM_PAD pixels
    from its neighbours (`pad`), the SSIM map of the padded stacks weighed by each interior pixel's solid angle
    (weighted_metrics.ssim on ssim_plane).  GPU tensors: the HIP kernels; CPU tensors: the twins (float64 map).  Forward
    only: a tensor that requires grad is refused.
    Limits: the ring is bilinear and one level deep, as for to_erp, so within 5 pixels of an edge a window reads a slightly
    softer neighbour than the sphere itself; equality with 360Lib's WS-SSIM is not claimed; no multi-scale form, no 4:2:0"""
    from . import weighted_metrics
    sp = _spec(spec)
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.shape != y.shape or x.dtype != y.dtype or x.device != y.device:
        raise PconvError("cube ws_ssim: two cube pictures of one kind, layout, face size, type and device expected, got %s and %s"
                         % tuple("%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__
                                 for t in (x, y)))
    if x.requires_grad or y.requires_grad:
        raise PconvError("cube ws_ssim: a tensor that requires grad: the weighted SSIM and the face continuation are forward only; "
                         "detach the pictures")
    a = _picture_face(x, sp)
    stacks = [pad(unpack(weighted_metrics._as_planes(t).float(), sp.layout).contiguous(), sp.kind, SSIM_PAD) for t in (x, y)]
    return weighted_metrics.ssim(stacks[0], stacks[1], ssim_plane(sp.kind, a, rule))


def ws_ssim(x, y, spec, rule="solid-angle"):
    """float64 (n,) WS-SSIM of each cube picture: the mean over the channels of ws_ssim_planes"""
    from . import weighted_metrics
    return weighted_metrics.channel_mean(ws_ssim_planes(x, y, spec, rule))


def ws_ssim_loss_terms(x, y, spec, rule="solid-angle"):
    """float64 (n,) on the pictures' device, attached to autograd: ws_ssim's figure as a loss term.  x, y: float32 (n, C,
    height, width) cube pictures of one spec and face size (uint8 carries no gradient and is refused).  Both are unpacked,
    continued by SSIM_PAD pixels with pad(.., grad=True) and scored by weighted_metrics.ssim_loss_terms on ssim_plane.  The
    rings weigh zero but their gradient is not zero -- ring pixels lie in the windows of weighted pixels -- and
    `pad_backward` carries it to the neighbouring faces.  GPU tensors: HIP kernels all the way, forward and backward; CPU
    tensors: pad_torch / pad_backward_torch and the float64 torch statement of the SSIM.  ws_ssim's limits hold"""
    from . import weighted_metrics
    sp = _spec(spec)
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.shape != y.shape or x.dtype != y.dtype or x.device != y.device \
            or x.dim() != 4 or x.dtype != torch.float32:
        raise PconvError("cube ws_ssim loss: two float32 (n, C, height, width) cube pictures of one kind, layout, face size and "
                         "device expected (uint8 frames carry no gradient), got %s and %s"
                         % tuple("%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__
                                 for t in (x, y)))
    a = _picture_face(x, sp)
    stacks = [pad(unpack(t, sp.layout).contiguous(), sp.kind, SSIM_PAD, grad=torch.is_grad_enabled() and t.requires_grad)
              for t in (x, y)]
    return weighted_metrics.ssim_loss_terms(stacks[0], stacks[1], ssim_plane(sp.kind, a, rule))


def point_directions(pointset):
    """float64 (P, 3), C order: (cos p cos t, cos p sin t, sin p) of the points (t, p) of a PointSet or a (P, 2) array: the
    array the record kernel and its twin both read"""
    pts = pointset.points if hasattr(pointset, "points") else np.asarray(pointset, dtype=np.float64)
    cp = np.cos(pts[:, 1])
    return np.ascontiguousarray(np.stack([cp * np.cos(pts[:, 0]), cp * np.sin(pts[:, 0]), np.sin(pts[:, 1])], axis=1))


def point_positions(kind, a, dirs):
    """(g, u', v') of directions (P, 3): the face and the position on it before the clamp, in the kernel's order"""
    return face_position(kind, check_face(a), np.asarray(dirs, dtype=np.float64).T)


def point_records_numpy(pointset, kind, a):
    """int32 (P, 2): the records of a point set on the padded stack of a cube of face size a, in float64 on the host,
    operation by operation in the kernel's order (pconv_cube_points_records).  The upper clamp is a - 1/2 - 1/256"""
    kind, a = _kind(kind), check_face(a)
    g, u, v = point_positions(kind, a, point_directions(pointset))
    hi = a - 0.5 - 1.0 / PHASES
    u, v = np.clip(u, -0.5, hi), np.clip(v, -0.5, hi)
    A = a + 2 * PAD
    qu = np.rint((u + PAD) * PHASES).astype(np.int64)
    qv = np.rint((v + PAD + g.astype(np.float64) * A) * PHASES).astype(np.int64)
    return np.stack([qu, qv], axis=1).astype(np.int32)


KEPT_RECORDS = 4     # record tensors kept per point set


def point_records(pointset, kind, a, device=None):
    """int32 (P, 2) on `device`: the HIP kernel for a GPU device, point_records_numpy on the CPU -- equal for "cmp", and for
    "eac" away from rounding boundaries.  A PointSet keeps its last KEPT_RECORDS; do not write to it"""
    from . import _metric_ops, sphere_points
    kind, a, device = _kind(kind), check_face(a), _device(device)
    ps = sphere_points._pointset(pointset)
    kept = ps.__dict__.setdefault("_cube_records", collections.OrderedDict())
    key = (kind, a, str(device))
    if key in kept:
        kept.move_to_end(key)
        return kept[key]
    if device.type == "cuda":
        rec = _metric_ops.cube_points_records(torch.from_numpy(point_directions(ps)).to(device), kind, a)
    else:
        rec = torch.from_numpy(point_records_numpy(ps, kind, a))
    kept[key] = rec
    while len(kept) > KEPT_RECORDS:
        kept.popitem(last=False)
    return rec


def _points_operand(t, sp, ps):
    """(the plane the sampler reads, its records): the padded stack of a cube picture, or an ERP picture as it is"""
    from . import sphere_points
    t = sphere_points._as_planes(t)
    if sp is None:
        return t, ps.records(t.shape[2], t.shape[3], t.device)
    sp = _spec(sp)
    faces = unpack(t, sp.layout).contiguous()
    return pad(faces, sp.kind), point_records(ps, sp.kind, _check_stack(faces), t.device)


def points_mse(x, y, pointset, interp="lanczos", x_spec=None, y_spec=None):
    """float64 CPU tensor (n, C): sphere_points.mse with either operand a cube picture.  An operand with a spec is a cube
    picture in that spec's layout (unpack, pad, point_records); an operand with None is an ERP picture (sphere_points'
    own records).  Any mix of projections, kinds and sizes.  GPU tensors: the fused pconv_sphere_points_mse_f32; CPU
    tensors: sphere_points.mse_records_torch's samples and errors, summed in the header's order (weighted_metrics.
    ordered_sum) instead of torch's: the same bits as the kernel"""
    from . import sphere_points, weighted_metrics
    sphere_points._check_interp(interp)
    ps = sphere_points._pointset(pointset)
    px, rx = _points_operand(x, x_spec, ps)
    py, ry = _points_operand(y, y_spec, ps)
    sphere_points._check_pair(px, py)
    if px.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "sphere_points_mse"):
            raise PconvError("cube: the active backend has no sphere_points_mse kernel for a GPU tensor")
        return ops.sphere_points_mse(px.contiguous(), rx, py.contiguous(), ry, interp)
    d = sphere_points.sample_torch(px, rx, interp) - sphere_points.sample_torch(py, ry, interp)
    return (weighted_metrics.ordered_sum((d * d).double()) / rx.shape[0]).cpu()


def _level_set(level):
    from . import sphere_points
    return sphere_points.icosphere_set(sphere_points.LEVEL if level is None else int(level))


def s_psnr_nn(x, y, x_spec=None, y_spec=None, level=None):
    """float64 (n,) S-PSNR-NN in dB: icosphere(level, default 8), the nearest pixel of each picture"""
    from . import sphere_points
    return sphere_points.psnr_of(points_mse(x, y, _level_set(level), "nearest", x_spec, y_spec))


def s_psnr_i(x, y, x_spec=None, y_spec=None, level=None):
    """float64 (n,) S-PSNR-I in dB: icosphere(level, default 8), the 6 x 6 Lanczos-3 sampler"""
    from . import sphere_points
    return sphere_points.psnr_of(points_mse(x, y, _level_set(level), "lanczos", x_spec, y_spec))


def cpp_psnr(x, y, x_spec=None, y_spec=None, size=None):
    """float64 (n,) CPP-PSNR in dB: both pictures read at the valid pixels of a Craster parabolic picture of `size`, by
    default erp_size(a) of the first cube operand (x's own size when neither is one)"""
    from . import sphere_points
    if size is None:
        for t, sp in ((x, x_spec), (y, y_spec)):
            if sp is not None:
                size = erp_size(_picture_face(t, _spec(sp)))
                break
        else:
            size = x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:]
    return sphere_points.psnr_of(points_mse(x, y, sphere_points.cpp_set(int(size[0]), int(size[1])), "lanczos", x_spec, y_spec))
