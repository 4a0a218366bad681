"""Shared by tests/test_backward_ordered_cpu.py and tests/test_gpu_backward_ordered.py: the reverse lists of the
ordered backward kernels built in numpy from the forward tables, the float32 walk of a list exactly as
include/pconv_hip.h ("the order") states it, and the numpy twin of the quantiser's fixed-shape reduction."""
import numpy as np
import torch

from ref_ops_cases import NPART

F32 = np.float32


def P(a):
    return a.ctypes.data


def forward_taps(kind, weight, rows, width):
    """(widths, tap_col, tap_coef) of pconv_host_slice_taps / pconv_host_uslice_taps for an ERP of `rows` x `width`"""
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd._native import call
    rule = "pconv_host_slice_widths" if kind == "slice" else "pconv_host_tile_widths"
    wd = PCONV.tile_widths(weight, NPART, rows, width, rule)
    col, coef = np.zeros(NPART * width, np.int32), np.zeros(NPART * width * 4, F32)
    call("pconv_host_%s_taps" % kind, P(wd), NPART, width, P(col), P(coef))
    return wd, col, coef


def host_tap_reverse(kind, wd, col, coef, width):
    """pconv_host_tap_reverse's lists: (start, src, coef)"""
    from pseudocylindrical_convolution_amd._native import call
    uslice = int(kind == "uslice")
    n = call("pconv_host_tap_reverse_size", P(wd), NPART, width, uslice)
    start, src, rc = np.zeros(NPART * width + 1, np.int32), np.zeros(n, np.int32), np.zeros(n, F32)
    assert call("pconv_host_tap_reverse", P(wd), NPART, width, P(col), P(coef), uslice, P(start), P(src), P(rc)) == n
    return start, src, rc


def numpy_tap_reverse(kind, wd, col, coef, width):
    """the same lists from the forward table: source column ascending, taps -1, 0, +1, +2, grouped by destination"""
    lists = [[] for _ in range(NPART * width)]
    for t in range(NPART):
        period = int(wd[t]) if kind == "uslice" else width
        nsrc = width if kind == "uslice" else min(int(wd[t]), width)
        for tw in range(nsrc):
            e = t * width + tw
            for j in (-1, 0, 1, 2):
                lists[t * width + (int(col[e]) + j) % period].append((tw, coef[e * 4 + j + 1]))
    start = np.cumsum([0] + [len(li) for li in lists]).astype(np.int32)
    flat = [x for li in lists for x in li]
    return start, np.array([s for s, _ in flat], np.int32), np.array([c for _, c in flat], F32)


def walk(src_rows, start, src, coef, key):
    """ordered sum of one destination over the leading axes of src_rows (..., columns): the accumulator starts at
    +0; per entry one float32 product, then one float32 add"""
    acc = np.zeros(src_rows.shape[:-1], F32)
    for k in range(int(start[key]), int(start[key + 1])):
        acc = acc + src_rows[..., int(src[k])] * coef[k]
    return acc


def walk_slice(grad, wd, lists, rows_per_tile, width, pad):
    """grad: the tile-stack gradient (n*npart, c, rows + 2 pad, width + 2 pad) -> the ERP gradient, by the lists"""
    g = grad.numpy()
    n, c = g.shape[0] // NPART, g.shape[1]
    out = np.zeros((n, c, rows_per_tile * NPART, width), F32)
    for t in range(NPART):
        rows = g[t::NPART, :, pad:pad + rows_per_tile, pad:pad + width]       # (n, c, rows, width)
        for j in range(width):
            out[:, :, t * rows_per_tile:(t + 1) * rows_per_tile, j] = walk(rows, *lists, t * width + j)
    return torch.from_numpy(out)


def walk_uslice(grad, wd, lists, rows_per_tile, width, pad):
    """grad: the ERP gradient (n, c, rows * npart, width) -> the tile-stack gradient, zero outside the interior"""
    g = grad.numpy()
    n, c = g.shape[:2]
    out = np.zeros((n * NPART, c, rows_per_tile + 2 * pad, width + 2 * pad), F32)
    for t in range(NPART):
        rows = g[:, :, t * rows_per_tile:(t + 1) * rows_per_tile, :]
        for i in range(int(wd[t])):
            out[t::NPART, :, pad:pad + rows_per_tile, pad + i] = walk(rows, *lists, t * width + i)
    return torch.from_numpy(out)


def project_table(theta, phi, fov, h_out, w_out, hs, ws):
    from pseudocylindrical_convolution_amd._native import call
    th, ph = np.asarray(theta, F32), np.asarray(phi, F32)
    tf = np.zeros(len(th) * h_out * w_out * 2, F32)
    call("pconv_host_project_table", P(th), P(ph), len(th), fov, h_out, w_out, hs, ws, P(tf))
    return tf


def host_project_reverse(tf, nview, inner, hs, ws, near):
    from pseudocylindrical_convolution_amd._native import call
    n = call("pconv_host_project_reverse_size", nview, inner, int(near))
    start, smp, wgt = np.zeros(hs * ws + 1, np.int32), np.zeros(n, np.int32), np.zeros(n, F32)
    assert call("pconv_host_project_reverse", P(tf), nview, inner, hs, ws, int(near), P(start), P(smp), P(wgt)) == n
    return start, smp, wgt


def numpy_project_reverse(tf, nview, inner, hs, ws, near):
    """the forward walk (viewport pixel, then view, then corner) in the oracle's arithmetic, stably sorted by pixel"""
    t = tf.reshape(nview, inner, 2)
    pix, smp, wgt = [], [], []
    for ps in range(inner):
        for tb in range(nview):
            fx, fy = t[tb, ps]
            if near:
                tw = int(np.floor(float(fx) + 0.5)) % ws
                th = min(int(np.floor(float(fy) + 0.5)), hs - 1)
                corners = [(th * ws + tw, F32(1))]
            else:
                tw, th = int(np.floor(fx)), int(np.floor(fy))
                pw, ph = (tw + 1) % ws, min(th + 1, hs - 1)
                tx, ty = F32(fx - F32(tw)), F32(fy - F32(th))
                ntx, nty = F32(1.0 - float(tx)), F32(1.0 - float(ty))
                corners = [(th * ws + tw, F32(ntx * nty)), (th * ws + pw, F32(tx * nty)),
                           (ph * ws + tw, F32(ntx * ty)), (ph * ws + pw, F32(tx * ty))]
            for p, w in corners:
                pix.append(p), smp.append(tb * inner + ps), wgt.append(w)
    order = np.argsort(np.array(pix), kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(np.array(pix), minlength=hs * ws))]).astype(np.int32)
    return start, np.array(smp, np.int32)[order], np.array(wgt, F32)[order]


def walk_projects(grad, lists, nview, inner, shape):
    """grad (n*nview, c, h_out, w_out), read as (view, plane, pixel) -> (gradient, count) of shape (n, c, hs, ws)"""
    n, c, hs, ws = shape
    g = grad.numpy().reshape(nview, n * c, inner)
    start, smp, wgt = lists
    gin, cnt = np.zeros((n * c, hs * ws), F32), np.zeros((n * c, hs * ws), F32)
    for p in np.nonzero(start[1:] > start[:-1])[0]:
        acc, k = np.zeros(n * c, F32), F32(0)
        for e in range(int(start[p]), int(start[p + 1])):
            tb, ps = divmod(int(smp[e]), inner)
            acc = acc + wgt[e] * g[tb, :, ps]
            k = F32(k + wgt[e])
        gin[:, p], cnt[:, p] = acc, k
    return torch.from_numpy(gin.reshape(shape)), torch.from_numpy(cnt.reshape(shape))


def quant_twin(x, val, idx, tab, widths, npart):
    """g_weight of the ordered quantiser backward, bit for bit (include/pconv_hip.h, "quant"): x, val, idx
    (tn, c, h, w) and tab (c, levels) as float32 arrays, widths the tiles' valid widths"""
    tn, c, h, w = x.shape
    levels, hw = tab.shape[1], h * w
    live = (np.arange(hw) % w)[None, :] < np.asarray(widths)[np.arange(tn) % npart][:, None]      # (tn, hw)
    diff = (val.astype(F32) - x.astype(F32)).astype(np.float64).reshape(tn, c, hw)
    q = idx.astype(np.int64).reshape(tn, c, hw)
    acc = np.zeros((tn, c, levels, 256), np.float64)
    ti, ci = np.meshgrid(np.arange(tn), np.arange(c), indexing="ij")
    for e in range(hw):                               # lane e mod 256 meets its elements in ascending order
        on = np.broadcast_to(live[:, e][:, None], (tn, c))
        acc[ti[on], ci[on], q[:, :, e][on], e % 256] += diff[:, :, e][on]
    s = 128
    while s:                                          # the fixed tree over the lanes
        acc[..., :s] = acc[..., :s] + acc[..., s:2 * s]
        s //= 2
    part = acc[..., 0]                                # (tn, c, levels)
    total = np.zeros((c, levels), np.float64)
    for t in range(tn):                               # planes in ascending order, fp64, rounded once
        total = total + part[t]
    bins = total.astype(F32)
    g_w, run = np.zeros((c, levels), F32), np.zeros(c, F32)
    for j in range(levels - 1, -1, -1):               # the suffix sum of quant_weight_grad_kernel
        run = run + bins[:, j]
        g_w[:, j] = run * tab[:, j] if j else run
    return g_w
