"""What the CPU and the GPU tests of the resize's ordered backward share (include/pconv_hip.h,
pconv_erp_resample_backward_f32): the cases, their gradients, the forward walk of an axis and its lists in numpy, and the
definition itself as a plain loop over the table entries in forward order (float32, or float64 for the bounds)."""
import numpy as np
import torch

# (n, C, h, w, h2, w2)
CASES = [
    (1, 2, 9, 16, 5, 12),        # shrink; w2 % 4 == 0 but w2 // 2 = 6: 16-byte loads on the entries that did not cross only
    (2, 1, 6, 10, 15, 37),       # enlargement; odd width; 4-byte paths; long horizontal lists
    (1, 1, 16, 32, 2, 4),        # 8:1, the longest T; every output row crosses a pole
    (1, 1, 2, 2, 5, 6),          # w < T_x and h < T_y: one destination hit several times by one row's taps
    (1, 3, 4, 1100, 6, 2300),    # more than one 1024-column tile in both passes; enlargement
    (1, 3, 5, 2300, 3, 1100),    # the same, shrinking
    (1, 2, 8, 16, 8, 16),        # the table is (0, 0, 1, 0, 0, 0) per row: the backward returns g bit for bit
]
IDENTITY = CASES[6]
CLAMPED = CASES[0]
SMALL = [CASES[0], CASES[1], CASES[2], CASES[3], CASES[6]]


def case_id(case):
    return "%dx%dx%dx%d-to-%dx%d" % case


def gradient(case, seed=0, n=None):
    """a gradient of the case's output: torch.rand, so finite and without -0"""
    c, h2, w2 = case[1], case[4], case[5]
    g = torch.Generator().manual_seed(seed + 131 * h2 + w2)
    return torch.rand((case[0] if n is None else n, c, h2, w2), generator=g)


def frames(case, seed=0, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed + 17 * case[2] + case[3])
    return torch.rand(case[:4], generator=g) * (hi - lo) + lo


def axis_walk(n_in, n_out, pole):
    """(dest int64 (n_out, T), crossed bool (n_out, T), weights float32 (n_out, T)): the source index every table entry
    (i, t) reads -- the wrap for pole=0, the pole rule and then the clamp for pole=1 -- and whether it crossed a pole"""
    from pseudocylindrical_convolution_amd import erp_resample
    first, weights = (t.numpy() for t in erp_resample.taps(n_in, n_out))
    r = first.astype(np.int64)[:, None] + np.arange(weights.shape[1], dtype=np.int64)
    if not pole:
        return np.mod(r, n_in), np.zeros(r.shape, dtype=bool), weights
    crossed = (r < 0) | (r >= n_in)
    r = np.clip(np.where(r < 0, -1 - r, np.where(r >= n_in, 2 * n_in - 1 - r, r)), 0, n_in - 1)
    return r, crossed, weights


def numpy_lists(n_in, n_out, pole):
    """(start, entry, crossed): a stable argsort of the forward walk (i, t) by destination"""
    dest, crossed, _ = axis_walk(n_in, n_out, pole)
    entry = np.argsort(dest.reshape(-1), kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(dest.reshape(-1), minlength=n_in))])
    return start, entry, crossed.reshape(-1)[entry].astype(np.uint8)


def walk(g, h, w, dtype=np.float32, absolute=False):
    """the definition as a plain loop: the vertical adjoint walks the entries (j, t) of the vertical table in forward
    order and adds wy[j][t] g[j][i] to row rho of gmid (the first term of a row starts its chain), i = c or (c - w2 // 2)
    % w2 for an entry that crossed a pole; the horizontal adjoint then walks (i, t) of the horizontal table and adds
    wx[i][t] gmid[:, i] to column (fx[i] + t) % w.  Every operation is one rounding of `dtype` (numpy arrays of one
    dtype).  absolute=True: |weights| (with |g|: the sum of the absolute terms, what an error bound is relative to)"""
    g = np.ascontiguousarray(g.numpy().astype(dtype))
    n, c, h2, w2 = g.shape
    dest_y, crossed, wy = axis_walk(h, h2, 1)
    dest_x, _, wx = axis_walk(w, w2, 0)
    wy, wx = wy.astype(dtype), wx.astype(dtype)
    if absolute:
        g, wy, wx = np.abs(g), np.abs(wy), np.abs(wx)
    back = np.mod(np.arange(w2) - w2 // 2, w2)
    gmid, started = np.zeros((n, c, h, w2), dtype=dtype), np.zeros(h, dtype=bool)
    for j in range(h2):
        for t in range(wy.shape[1]):
            r = dest_y[j, t]
            term = wy[j, t] * (g[:, :, j, back] if crossed[j, t] else g[:, :, j, :])
            gmid[:, :, r] = gmid[:, :, r] + term if started[r] else term
            started[r] = True
    gx, started = np.zeros((n, c, h, w), dtype=dtype), np.zeros(w, dtype=bool)
    for i in range(w2):
        for t in range(wx.shape[1]):
            col = dest_x[i, t]
            term = wx[i, t] * gmid[:, :, :, i]
            gx[:, :, :, col] = gx[:, :, :, col] + term if started[col] else term
            started[col] = True
    assert gx.dtype == dtype and gmid.dtype == dtype
    return torch.from_numpy(gx)


def term_counts(h, w, h2, w2):
    """float64 (h, w): the number of terms behind gx[r][c], those of its own list plus those of the gmid row it reads"""
    nv = np.bincount(axis_walk(h, h2, 1)[0].reshape(-1), minlength=h)
    nh = np.bincount(axis_walk(w, w2, 0)[0].reshape(-1), minlength=w)
    return torch.from_numpy((nv[:, None] + nh[None, :]).astype(np.float64))
