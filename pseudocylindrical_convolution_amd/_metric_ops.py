"""Bindings of the weighted metrics, of the cube's point records and of its face continuation of any depth, forward and
backward (include/pconv_hip.h, pconv_weighted_mse_*, pconv_weighted_ssim_f32, pconv_weighted_ssim_backward_f32,
pconv_cube_points_records, pconv_cube_pad_depth_f32, pconv_cube_pad_backward_f32): what PCONV.py's wrappers are for the
older entry points, kept here because PCONV.py's public names are closed.  weighted_metrics.py and cube.py are the users.

Every wrapper holds PCONV.py's operand contract: an operand of the wrong type, device, shape or layout is refused with a
PconvError that names it, before the library is reached (`_native.call` is looked up at each call, so a test can watch
it).  Attribute comparisons only: nothing is copied and nothing waits.
"""
import torch

from . import _native
from ._native import PconvError

CUBE_KINDS = {"cmp": 1, "eac": 2}   # PCONV_CUBE_CMP, PCONV_CUBE_EAC
CUBE_MAX_FACE = 9453                # PCONV_CUBE_MAX_FACE
CUBE_MAX_DEPTH = 8                  # PCONV_CUBE_MAX_DEPTH
POINTS_MAX = (1 << 28) - 1
MAX_SIDE = 1 << 20
MAX_PLANES = 65535


def _ptr(t):
    return t.data_ptr()


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _operand(t, what, name, shape, dtype, device=None):
    """operand `name` of `what`: a contiguous GPU tensor of `dtype` and of exactly `shape` (None: any extent), on `device`
    when one is given.  Returns its shape"""
    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.dim() == len(shape) \
        and all(e is None or e == s for e, s in zip(shape, t.shape)) and (device is None or t.device == device)
    if not ok:
        want = "(%s)" % ", ".join("*" if e is None else str(int(e)) for e in shape)
        got = "%s %s on %s%s" % (t.dtype, tuple(t.shape), t.device, "" if t.is_contiguous() else ", not contiguous") \
            if isinstance(t, torch.Tensor) else type(t).__name__
        raise PconvError("%s: %s must be a contiguous %s tensor of %s on %s, got %s"
                         % (what, name, str(dtype).split(".")[1], want, "a GPU" if device is None else device, got))
    return tuple(t.shape)


def _total(what, total):
    total = float(total)
    if not 0.0 < total < float("inf"):
        raise PconvError("%s: total, the weights' sum, must be a positive finite number, got %r" % (what, total))
    return total


def _frames(what, x, y, weights, float_only):
    """the checks the forward and the backward share; (n, c, h, w) and whether the frames are uint8"""
    if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and not float_only:
        n, h, w, c = _operand(x, what, "x", (None, None, None, 3), torch.uint8)
        _operand(y, what, "y", (n, h, w, 3), torch.uint8, x.device)
    else:
        n, c, h, w = _operand(x, what, "x", (None,) * 4, torch.float32)
        _operand(y, what, "y", (n, c, h, w), torch.float32, x.device)
    _operand(weights, what, "weights", (h, w), torch.float64, x.device)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and 4 * h * w < 1 << 31 and 1 <= n * c <= MAX_PLANES):
        raise PconvError("%s: x: %d planes of %dx%d: sides of 1 .. 2^20, a plane below 2^31 bytes and n * C of 1 .. %d expected"
                         % (what, n * c, w, h, MAX_PLANES))
    return (n, c, h, w), x.dtype == torch.uint8


def weighted_mse_device(x, y, weights, total):
    """float64 (n, C) on the inputs' device: (sum over the pixels of weights * (x - y)^2) / total per plane, in the order of
    include/pconv_hip.h (pconv_weighted_mse_f32 / _u8).  x, y: contiguous float32 (n, C, H, W) or uint8 (n, H, W, 3) GPU
    tensors of one shape; weights: contiguous float64 (H, W) on the same device; total: a positive finite float.  Two
    launches; nothing waits"""
    what = "weighted_mse"
    (n, c, h, w), u8 = _frames(what, x, y, weights, False)
    total = _total(what, total)
    nbytes = _native.call("pconv_weighted_mse_workspace_bytes", n, c, h, w)
    workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)   # one fp64 partial per plane and chunk
    out = torch.empty((n, c), dtype=torch.float64, device=x.device)
    _native.call("pconv_weighted_mse_u8" if u8 else "pconv_weighted_mse_f32", _ptr(x), _ptr(y), _ptr(weights), total, n, c, h, w,
                 _ptr(workspace), _ptr(out), _stream(x.device))
    return out


def weighted_mse_backward(x, y, weights, total, gout):
    """float32 (n, C, H, W): the gradient of sum(gout * weighted_mse_device(x, y, weights, total)) with respect to y
    (pconv_weighted_mse_backward_f32); gout contiguous float64 (n, C) on the same device, read by the kernel.  One launch.
    For the gradient with respect to x swap x and y"""
    what = "weighted_mse_backward"
    (n, c, h, w), _ = _frames(what, x, y, weights, True)
    _operand(gout, what, "gout", (n, c), torch.float64, x.device)
    total = _total(what, total)
    grad = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    _native.call("pconv_weighted_mse_backward_f32", _ptr(x), _ptr(y), _ptr(weights), total, _ptr(gout), n, c, h, w, _ptr(grad),
                 _stream(x.device))
    return grad


def weighted_ssim_device(x, y, weights, total):
    """float64 (n, C) on the inputs' device: (sum over the pixels of weights * the SSIM map of (x, y)) / total per plane, in
    the order of include/pconv_hip.h (pconv_weighted_ssim_f32).  x, y: contiguous float32 (n, C, H, W) GPU tensors of one
    shape; weights: contiguous float64 (H, W) on the same device; total: a positive finite float.  Two launches; nothing
    waits"""
    what = "weighted_ssim"
    (n, c, h, w), _ = _frames(what, x, y, weights, True)
    total = _total(what, total)
    nbytes = _native.call("pconv_weighted_ssim_workspace_bytes", n, c, h, w)
    workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)   # one fp64 partial per plane and tile
    out = torch.empty((n, c), dtype=torch.float64, device=x.device)
    _native.call("pconv_weighted_ssim_f32", _ptr(x), _ptr(y), _ptr(weights), total, n, c, h, w, _ptr(workspace), _ptr(out),
                 _stream(x.device))
    return out


def weighted_ssim_backward(x, y, weights, total, gout):
    """float32 (n, C, H, W): the gradient of sum(gout * weighted_ssim_device(x, y, weights, total)) with respect to y
    (pconv_weighted_ssim_backward_f32); gout contiguous float64 (n, C) on the same device, read by the kernel.  One launch.
    For the gradient with respect to x swap x and y"""
    what = "weighted_ssim_backward"
    (n, c, h, w), _ = _frames(what, x, y, weights, True)
    _operand(gout, what, "gout", (n, c), torch.float64, x.device)
    total = _total(what, total)
    grad = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    _native.call("pconv_weighted_ssim_backward_f32", _ptr(x), _ptr(y), _ptr(weights), total, _ptr(gout), n, c, h, w, _ptr(grad),
                 _stream(x.device))
    return grad


def cube_pad_backward(g, table, lists, a, depth, out=None):
    """float32 (n, C, 6 a, a): the gradient of cube_pad_depth with respect to the face stack, in the order of include/
    pconv_hip.h (pconv_cube_pad_backward_f32).  g: contiguous float32 (n, C, 6 A, A) on a GPU, A = a + 2 depth; table: the
    int32 (6 (A^2 - a^2), 3) table the forward read; lists: (start, entry), int32 of 6 a^2 + 1 and 24 (A^2 - a^2) elements
    (cube.pad_reverse_lists), all on g's device.  One launch; out must not be g"""
    what = "cube_pad_backward"
    a, depth = int(a), int(depth)
    if not 1 <= depth <= CUBE_MAX_DEPTH:
        raise PconvError("%s: depth must be 1 .. %d, got %r" % (what, CUBE_MAX_DEPTH, depth))
    A = a + 2 * depth
    if not (a >= 2 and 24 * A * A < 1 << 31):
        raise PconvError("%s: a face size from 2 up with the padded stack below 2^31 bytes expected, got %d at depth %d"
                         % (what, a, depth))
    n, c, _, _ = _operand(g, what, "g", (None, None, 6 * A, A), torch.float32)
    if not 1 <= n * c <= MAX_PLANES:
        raise PconvError("%s: g: n * C of 1 .. %d expected, got %d" % (what, MAX_PLANES, n * c))
    ring = A * A - a * a
    _operand(table, what, "table", (6 * ring, 3), torch.int32, g.device)
    try:
        start, entry = lists
    except (TypeError, ValueError):
        raise PconvError("%s: lists must be the pair (start, entry), got %s" % (what, type(lists).__name__))
    _operand(start, what, "lists[0]", (6 * a * a + 1,), torch.int32, g.device)
    _operand(entry, what, "lists[1]", (24 * ring,), torch.int32, g.device)
    if out is None:
        out = torch.empty((n, c, 6 * a, a), dtype=torch.float32, device=g.device)
    else:
        _operand(out, what, "out", (n, c, 6 * a, a), torch.float32, g.device)
    _native.call("pconv_cube_pad_backward_f32", _ptr(g), _ptr(out), _ptr(table), _ptr(start), _ptr(entry), n, c, a, depth,
                 _stream(g.device))
    return out


def cube_pad_depth(x, table, depth, out=None):
    """float32 (n, C, 6 A, A), A = a + 2 depth: the face stack x (contiguous float32 (n, C, 6 a, a) on a GPU) continued by
    `depth` pixels, 1 .. CUBE_MAX_DEPTH, across every face edge; table: contiguous int32 (6 (A^2 - a^2), 3) on the same
    device, from cube.pad_table(kind, a, depth) (pconv_cube_pad_depth_f32).  One launch; out must not be x"""
    what = "cube_pad_depth"
    depth = int(depth)
    if not 1 <= depth <= CUBE_MAX_DEPTH:
        raise PconvError("%s: depth must be 1 .. %d, got %r" % (what, CUBE_MAX_DEPTH, depth))
    n, c, h6, a = _operand(x, what, "x", (None,) * 4, torch.float32)
    A = a + 2 * depth
    if not (h6 == 6 * a and a >= 2 and 24 * A * A < 1 << 31 and 1 <= n * c <= MAX_PLANES):
        raise PconvError("%s: x: a face stack (n, C, 6 a, a) expected, a from 2 up with the padded stack below 2^31 bytes and "
                         "n * C of 1 .. %d, got %s at depth %d" % (what, MAX_PLANES, (n, c, h6, a), depth))
    _operand(table, what, "table", (6 * (A * A - a * a), 3), torch.int32, x.device)
    if out is None:
        out = torch.empty((n, c, 6 * A, A), dtype=torch.float32, device=x.device)
    else:
        _operand(out, what, "out", (n, c, 6 * A, A), torch.float32, x.device)
    _native.call("pconv_cube_pad_depth_f32", _ptr(x), _ptr(out), _ptr(table), n, c, a, depth, _stream(x.device))
    return out


def cube_points_records(dirs, kind, a, out=None):
    """int32 (P, 2) GPU tensor: the records of the directions `dirs` (contiguous float64 (P, 3) on the device) on the padded
    stack of a "cmp" / "eac" cube of face size a (cube.py, pconv_cube_points_records).  One launch, fp64"""
    what = "cube_points_records"
    count, _ = _operand(dirs, what, "dirs", (None, 3), torch.float64)
    if kind not in CUBE_KINDS:
        raise PconvError("%s: kind must be one of %s, got %r" % (what, sorted(CUBE_KINDS), kind))
    a = int(a)
    if not (2 <= a <= CUBE_MAX_FACE and 1 <= count <= POINTS_MAX):
        raise PconvError("%s: dirs: %d points on faces of %d: 1 <= P < 2^28 and a of 2 .. %d expected" % (what, count, a, CUBE_MAX_FACE))
    if out is None:
        out = torch.empty((count, 2), dtype=torch.int32, device=dirs.device)
    else:
        _operand(out, what, "out", (count, 2), torch.int32, dirs.device)
    _native.call("pconv_cube_points_records", _ptr(dirs), _ptr(out), count, CUBE_KINDS[kind], a, _stream(dirs.device))
    return out
