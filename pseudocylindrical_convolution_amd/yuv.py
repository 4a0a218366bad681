"""Planar 4:2:0 YCbCr frames in and out of the codec (include/pconv_hip.h, "YUV 4:2:0 frames"; csrc/yuv.hip).

A frame is one contiguous buffer, as a raw .yuv file holds it; h and w are even and at least 2:
  yuv420p      uint8   Y (h, w), then U (h/2, w/2), then V (h/2, w/2)
  nv12         uint8   Y (h, w), then interleaved UV (h/2, w/2, 2)
  yuv420p10le  uint16  (host little-endian) the planes of yuv420p, values 0..1023; a sample above 1023 is taken
                       modulo 1024
A batch is a tensor (n, frame_elems(h, w)) of the format's dtype.  With d the bit depth and s = 2^(d-8):
  range  "limited" (default): yo = 16s, ys = 219s, co = 128s, cs = 224s;  "full": yo = 0, ys = 2^d - 1,
         co = 2^(d-1), cs = 2^d - 1
  matrix "bt709" (default): Kr = 0.2126, Kb = 0.0722;  "bt601": Kr = 0.299, Kb = 0.114; in double, in this order,
         Kg = 1.0 - Kr - Kb, a = 2*(1 - Kr), dd = 2*(1 - Kb), b = Kb*dd/Kg, c = Kr*a/Kg, each then rounded once to
         float32 (`coefficients`: the seven floats the C side holds too)
Chroma is sited as H.26x type 0: co-sited with the even luma columns, midway between luma rows 2j and 2j+1.  The
longitude seam wraps, the poles clamp.  All arithmetic is float32, one rounding per operation (no contraction).

Ingest (`to_rgb`): chroma up, vertical first -- luma row 2j reads 0.25f*C[max(j-1, 0)] + 0.75f*C[j], row 2j+1 reads
0.75f*C[j] + 0.25f*C[min(j+1, h/2-1)] -- then horizontal: column 2i is V[i], column 2i+1 is 0.5f*(V[i] +
V[(i+1) % (w/2)]) (every intermediate is exact for code values up to 1023).  y = (Y - yo)/ys, cb = (Cb - co)/cs,
cr = (Cr - co)/cs, correctly rounded; R = y + a*cr, G = (y - b*cb) - c*cr, B = y + dd*cb, each clamped to [0, 1];
the frame is then padded to the coded size by the pole / seam rule of erp_size.py.

Egress (`from_rgb`): rows top..top+h-1 and columns 0..w-1 of the coded frame, clamped to [0, 1];
y = (Kr*R + Kg*G) + Kb*B, cb = (B - y)/dd, cr = (R - y)/a; chroma down: v = 0.5f*(p[2j] + p[2j+1]) per column, then
C[i] = (0.25f*v[(2i-1) mod w] + 0.5f*v[2i]) + 0.25f*v[2i+1]; q = clamp(floor((p*scale + offset) + 0.5f), 0, 2^d - 1)
with (ys, yo) for luma and (cs, co) for chroma.

GPU tensors go to the HIP kernels (PCONV.frames_yuv420_to_f32 / frames_f32_to_yuv420).  CPU tensors go to the torch
float32 statement below (`to_rgb_torch`, `from_rgb_torch`), the twin the tests hold the kernels to bit for bit; like
erp_size.pad_torch it is not a fallback for GPU tensors.
"""
import os

import numpy as np
import torch

from . import erp_size, sphere_metrics
from ._native import PconvError
from .PCONV import YUV_FORMATS as FORMATS, YUV_RANGES as RANGES   # name -> (C constant, dtype, bit depth) / C constant
from .PCONV_operator import backend

MATRICES = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}   # name -> (Kr, Kb); the names of PCONV.YUV_MATRICES


def _fmt(fmt):
    if fmt not in FORMATS:
        raise PconvError("yuv: unknown pixel format %r (one of %s)" % (fmt, ", ".join(sorted(FORMATS))))
    return FORMATS[fmt]


def _check_size(h, w):
    h, w = int(h), int(w)
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise PconvError("yuv: a 4:2:0 frame needs even sides of at least 2, got %dx%d" % (w, h))
    return h, w


def depth(fmt):
    return _fmt(fmt)[2]


def dtype(fmt):
    return _fmt(fmt)[1]


def frame_elems(h, w, fmt=None):
    """samples of one frame: h*w luma + 2 * (h/2)*(w/2) chroma"""
    h, w = _check_size(h, w)
    return h * w * 3 // 2


def frame_bytes(h, w, fmt):
    return frame_elems(h, w) * (2 if depth(fmt) > 8 else 1)


def coefficients(matrix="bt709", range="limited", fmt="yuv420p", double=False):
    """dict of the definition's constants: yo, ys, co, cs, qmax and Kr, Kg, Kb, a, b, c, dd -- float32 values (as
    Python floats) unless double=True (the unrounded doubles, for the float64 statement)"""
    if matrix not in MATRICES:
        raise PconvError("yuv: unknown matrix %r (one of %s)" % (matrix, ", ".join(sorted(MATRICES))))
    if range not in RANGES:
        raise PconvError("yuv: unknown range %r (one of %s)" % (range, ", ".join(sorted(RANGES))))
    d = depth(fmt)
    s = 1 << (d - 8)
    Kr, Kb = MATRICES[matrix]
    Kg = 1.0 - Kr - Kb
    a = 2 * (1 - Kr)
    dd = 2 * (1 - Kb)
    b = Kb * dd / Kg
    c = Kr * a / Kg
    k = dict(Kr=Kr, Kg=Kg, Kb=Kb, a=a, b=b, c=c, dd=dd)
    if not double:
        k = {name: float(np.float32(v)) for name, v in k.items()}
    if range == "limited":
        k.update(yo=16.0 * s, ys=219.0 * s, co=128.0 * s, cs=224.0 * s)
    else:
        k.update(yo=0.0, ys=float((1 << d) - 1), co=float(1 << (d - 1)), cs=float((1 << d) - 1))
    k["qmax"] = float((1 << d) - 1)
    return k


def _batch(buf, h, w, fmt):
    """the batch as (n, frame_elems); a single frame (frame_elems,) counts as n = 1"""
    _, dt, _ = _fmt(fmt)
    elems = frame_elems(h, w)
    if buf.dim() == 1:
        buf = buf[None]
    if buf.dtype != dt or buf.dim() != 2 or buf.shape[1] != elems:
        raise PconvError("yuv: %s frames of %dx%d are %s (n, %d), got %s %s"
                         % (fmt, w, h, dt, elems, buf.dtype, tuple(buf.shape)))
    return buf


def plane_views(buf, h, w, fmt):
    """(Y (n, h, w), U (n, h/2, w/2), V (n, h/2, w/2)) views into the batch, in its own dtype (nv12's U and V are
    strided).  Writing through them fills the buffer"""
    return plane_views_of(_batch(buf, h, w, fmt), h, w, fmt)


def _codes(t, fmt):
    """code values as int32: uint16 samples modulo 1024"""
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).to(torch.int32) & 1023
    return t.to(torch.int32)


def planes(buf, h, w, fmt):
    """float32 (n, 1, h, w), (n, 1, h/2, w/2), (n, 1, h/2, w/2) = sample / (2^d - 1), on the batch's device.  The
    quotient is formed in float64 and rounded once: torch divides a GPU tensor by a scalar as a product with the
    reciprocal, which in float32 is not the correctly rounded quotient; in float64 its error is far below the distance
    of any code / (2^d - 1) from a float32 rounding boundary, so every device gives the same bits"""
    peak = float((1 << depth(fmt)) - 1)
    return tuple((_codes(p, fmt).to(torch.float64) / peak).to(torch.float32).unsqueeze(1).contiguous()
                 for p in plane_views(buf, h, w, fmt))


def ws_psnr_yuv(a, b, h, w, fmt, weighting="ws"):
    """float64 (n, 3): WS-PSNR in dB of the Y, U and V planes of two batches of frames (sphere_metrics.ws_psnr on
    `planes`; the chroma planes are ERP grids of h/2 rows)"""
    return torch.stack([sphere_metrics.ws_psnr(p, q, weighting) for p, q in zip(planes(a, h, w, fmt), planes(b, h, w, fmt))],
                       dim=1)


# -- the definition in torch: the CPU twin ----------------------------------------------------------------------------
def chroma_up(c, dt=torch.float32):
    """(n, h/2, w/2) code values -> (n, h, w) in `dt`: vertical first (poles clamp), then horizontal (seam wraps)"""
    c = c.to(dt)
    n, h2, w2 = c.shape
    up = torch.cat([c[:, :1], c[:, :-1]], 1)        # C[max(j-1, 0)]
    down = torch.cat([c[:, 1:], c[:, -1:]], 1)      # C[min(j+1, h/2-1)]
    v = torch.stack([0.25 * up + 0.75 * c, 0.75 * c + 0.25 * down], 2).reshape(n, 2 * h2, w2)
    return torch.stack([v, 0.5 * (v + torch.roll(v, -1, 2))], 3).reshape(n, 2 * h2, 2 * w2)


def to_rgb_torch(buf, h, w, fmt, matrix="bt709", range="limited", pad=True, dt=torch.float32):
    """the ingest of the definition in torch: (n, frame_elems) -> `dt` (n, 3, H, W) at the coded size (pad=False:
    (n, 3, h, w), the converted frame before the pole / seam pad).  dt=torch.float64 is the float64 statement, with
    the constants unrounded"""
    k = coefficients(matrix, range, fmt, double=dt == torch.float64)
    Y, U, V = (_codes(p, fmt) for p in plane_views(buf, h, w, fmt))
    y = (Y.to(dt) - k["yo"]) / k["ys"]
    cb = (chroma_up(U, dt) - k["co"]) / k["cs"]
    cr = (chroma_up(V, dt) - k["co"]) / k["cs"]
    r = y + k["a"] * cr
    g = (y - k["b"] * cb) - k["c"] * cr
    b = y + k["dd"] * cb
    rgb = torch.stack([r, g, b], 1).clamp(0, 1)
    return erp_size.pad_torch(rgb) if pad else rgb


def ycc_torch(x, h, w, fmt, matrix="bt709", range="limited", dt=torch.float32):
    """the egress of the definition up to the quantiser's argument: (y (n, h, w), cb, cr (n, h/2, w/2)) in `dt`"""
    k = coefficients(matrix, range, fmt, double=dt == torch.float64)
    H, W, top = erp_size.coded_size(h, w)
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, H, W):
        raise PconvError("yuv: (n, 3, %d, %d) expected for %dx%d frames, got %s" % (H, W, w, h, tuple(x.shape)))
    p = x[:, :, top:top + h, :w].to(dt).clamp(0, 1)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    y = (k["Kr"] * r + k["Kg"] * g) + k["Kb"] * b

    def down(c):
        v = 0.5 * (c[:, 0::2] + c[:, 1::2])
        return (0.25 * torch.roll(v, 1, 2)[:, :, 0::2] + 0.5 * v[:, :, 0::2]) + 0.25 * v[:, :, 1::2]

    return y, down((b - y) / k["dd"]), down((r - y) / k["a"])


def from_rgb_torch(x, h, w, fmt, matrix="bt709", range="limited", dt=torch.float32):
    """the egress of the definition in torch: (n, 3, H, W) at the coded size -> (n, frame_elems) of the format"""
    k = coefficients(matrix, range, fmt, double=dt == torch.float64)
    y, cb, cr = ycc_torch(x, h, w, fmt, matrix, range, dt)
    quant = lambda p, scale, offset: torch.floor((p * scale + offset) + 0.5).clamp(0, k["qmax"]).to(torch.int32)
    out = torch.empty((x.shape[0], frame_elems(h, w)), dtype=torch.int32)
    Y, U, V = plane_views_of(out, h, w, fmt)
    Y.copy_(quant(y, k["ys"], k["yo"]))
    U.copy_(quant(cb, k["cs"], k["co"]))
    V.copy_(quant(cr, k["cs"], k["co"]))
    return out.to(dtype(fmt))


def plane_views_of(buf, h, w, fmt):
    """plane_views without the dtype check (an int32 staging buffer of the same layout)"""
    n, h2, w2 = buf.shape[0], h // 2, w // 2
    y = buf[:, :h * w].view(n, h, w)
    if fmt == "nv12":
        uv = buf[:, h * w:].view(n, h2, w2, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, buf[:, h * w:h * w + h2 * w2].view(n, h2, w2), buf[:, h * w + h2 * w2:].view(n, h2, w2)


# -- dispatch -----------------------------------------------------------------------------------------------------------
def to_rgb(buf, h, w, fmt, matrix="bt709", range="limited", out=None):
    """(n, frame_elems) frames -> float32 (n, 3, H, W) RGB at the coded size: the HIP kernel for GPU tensors, the
    torch statement on the CPU"""
    if buf.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "frames_yuv420_to_f32"):
            raise PconvError("yuv: the active backend has no frames_yuv420_to_f32 kernel for a GPU tensor")
        return ops.frames_yuv420_to_f32(_batch(buf, h, w, fmt), h, w, fmt, matrix, range, out)
    rgb = to_rgb_torch(buf, h, w, fmt, matrix, range)
    return rgb if out is None else out.copy_(rgb)


def from_rgb(x, h, w, fmt, matrix="bt709", range="limited", out=None):
    """float32 (n, 3, H, W) RGB at the coded size -> (n, frame_elems) frames of h x w: the HIP kernel for GPU
    tensors, the torch statement on the CPU"""
    if x.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "frames_f32_to_yuv420"):
            raise PconvError("yuv: the active backend has no frames_f32_to_yuv420 kernel for a GPU tensor")
        return ops.frames_f32_to_yuv420(x, h, w, fmt, matrix, range, out)
    buf = from_rgb_torch(x, h, w, fmt, matrix, range)
    return buf if out is None else out.copy_(buf)


# -- raw .yuv files ------------------------------------------------------------------------------------------------------
def _np_dtype(fmt):
    return np.dtype("<u2") if depth(fmt) > 8 else np.dtype("u1")


def count_frames(path, h, w, fmt):
    """frames in a raw file; PconvError when its length is not a whole number of frames"""
    size, per = os.path.getsize(path), frame_bytes(h, w, fmt)
    if size % per:
        raise PconvError("yuv: %s holds %d bytes, not a whole number of %s frames of %dx%d (%d bytes each)"
                         % (path, size, fmt, w, h, per))
    return size // per


def read_frames(path, h, w, fmt, start=0, count=None):
    """frames start .. start+count-1 (count=None: to the end) of a raw .yuv file as a CPU tensor (count, frame_elems)"""
    total = count_frames(path, h, w, fmt)
    start = int(start)
    count = total - start if count is None else int(count)
    if start < 0 or count < 1 or start + count > total:
        raise PconvError("yuv: frames %d..%d asked of %s, which holds %d" % (start, start + count - 1, path, total))
    elems = frame_elems(h, w)
    data = np.fromfile(path, dtype=_np_dtype(fmt), count=count * elems, offset=start * frame_bytes(h, w, fmt))
    return torch.from_numpy(data.astype(data.dtype.newbyteorder("="), copy=False).reshape(count, elems))


def write_frames(path, buf, h, w, fmt, append=False):
    """write (or append) a CPU batch (n, frame_elems) to a raw .yuv file; returns the number of frames written"""
    buf = _batch(buf, h, w, fmt)
    if buf.is_cuda:
        raise PconvError("yuv: write_frames takes a CPU tensor")
    with open(path, "ab" if append else "wb") as f:
        f.write(buf.contiguous().numpy().astype(_np_dtype(fmt), copy=False).tobytes())
    return buf.shape[0]
