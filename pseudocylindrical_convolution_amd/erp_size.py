"""Panoramas of any size: the pole / seam padding rule (include/pconv_hip.h, pconv_erp_coded_size).

An h x w ERP frame is coded at `coded_size(h, w)` = (H, W, top): H = 256*ceil(h/256), W = 16*ceil(w/16),
top = (H - h) // 2.  The extra rows continue the sphere across the two poles (mirrored rows, longitude turned by
half a revolution), the extra columns continue the seam (left half of the pad repeats the last column, right half
the first).  The rule is a pure gather, so uint8 and float inputs pad to the same bits; decoding crops
rec[:, :, top:top + h, :w].  A codable size (h % 256 == 0, w % 16 == 0) maps to itself.

On the GPU the HIP kernels of csrc/erp_size.hip apply it (PCONV.erp_pad_f32, frames_u8_to_f32_erp,
frames_f32_to_u8_crop); `pad` falls back to the torch gather below only for CPU tensors (the oracle backend).
"""
import torch

from ._native import PconvError
from .PCONV_operator import backend

TILE_ROWS = 256   # 16 latitude tiles x the analysis transform's 16x down-sampling
COLS = 16


def coded_size(h, w):
    """(H, W, top) of an h x w ERP frame: the Python mirror of pconv_erp_coded_size"""
    h, w = int(h), int(w)
    if h < 2 or w < 2 or h > 1 << 20 or w > 1 << 20:
        raise ValueError("ERP size %dx%d: each side must be in 2..2^20" % (w, h))
    H = TILE_ROWS * -(-h // TILE_ROWS)
    W = COLS * -(-w // COLS)
    return H, W, (H - h) // 2


def codable(h, w):
    """True when the codec takes h x w as it is (the padding rule is the identity)"""
    return h % TILE_ROWS == 0 and w % COLS == 0 and h > 0 and w > 0


def gather_index(h, w):
    """(rows (H,), flip (H,) bool, cols (W,), flipped cols (W,)) long / bool tensors of the rule"""
    H, W, top = coded_size(h, w)
    y = torch.arange(H) - top
    flip = (y < 0) | (y >= h)
    y = torch.where(y < 0, -1 - y, torch.where(y >= h, 2 * h - 1 - y, y)).clamp(0, h - 1)
    xc = torch.arange(W)
    m = (W - w + 1) // 2
    x = torch.where(xc < w, xc, torch.where(xc - w < m, torch.full_like(xc, w - 1), torch.zeros_like(xc)))
    return y, flip, x, (x + w // 2) % w


def pad_torch(x):
    """(..., h, w) -> (..., H, W) by the rule, on any device and dtype (the CPU path)"""
    h, w = x.shape[-2:]
    rows, flip, cols, cols_f = (t.to(x.device) for t in gather_index(h, w))
    r = x.index_select(-2, rows)
    return torch.where(flip[:, None], r.index_select(-1, cols_f), r.index_select(-1, cols))


def crop(rec, h, w):
    """the decoder's side of the rule: (..., H, W) -> (..., h, w), contiguous"""
    H, W, top = coded_size(h, w)
    if tuple(rec.shape[-2:]) != (H, W):
        raise PconvError("erp crop: %s is not the coded size %dx%d of %dx%d" % (tuple(rec.shape[-2:]), W, H, w, h))
    return rec[..., top:top + h, :w].contiguous()


def pad(frames):
    """float32 (n, 3, h, w) -> (n, 3, H, W): the HIP kernel for GPU tensors, the torch gather on the CPU"""
    if frames.is_cuda:
        ops = backend.ops()
        if not hasattr(ops, "erp_pad_f32"):
            raise PconvError("erp pad: the active backend has no erp_pad_f32 kernel for a GPU tensor")
        return ops.erp_pad_f32(frames.contiguous())
    return pad_torch(frames)
