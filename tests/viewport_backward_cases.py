"""What the CPU and the GPU tests of the renderer's ordered backward share (include/pconv_hip.h,
pconv_remap_backward_f32): the cases -- those of viewport_cases.py and two sources that exist for the backward only --
their numpy maps, gradients, the lists in numpy, and the order itself as a plain sequential float32 loop."""
import numpy as np
import torch

from viewport_cases import CASES as FORWARD_CASES, case_id

TINY = [
    (4, 4, 3, 5, 2, (30, 20, 10, 90, 67.5)),    # w < 6: every tap column coincides with another, and the rows fold
    (2, 64, 4, 6, 1, (100, 10, 0, 60, 60)),     # h = 2: the whole footprint lies in the pole rule and the clamp
]
CASES = TINY + list(FORWARD_CASES)
BATCHES = [(2, 3), (1, 1), (3, 2)]
# three views of a 32 x 64 source at 9 x 15 whose plan gives ss = 1, 2 and 4 on the source as it is
VIEWS3 = [(30, 20, 10, 60, 40), (-75.5, 80, 0, 100, 60), (123.25, -33.5, -170, 140, 50)]
P, T = 256, 6

_maps = {}


def source_map(case):
    """the float64 numpy map of a case as an int32 tensor, computed once"""
    from pseudocylindrical_convolution_amd import viewport
    if case not in _maps:
        h, w, vh, vw, ss, angles = case
        _maps[case] = torch.from_numpy(viewport.source_map_numpy(h, w, vh * ss, vw * ss, viewport.view(*angles)))
    return _maps[case]


def gradient(n, c, vh, vw, seed=0):
    g = torch.Generator().manual_seed(seed + 977 * vh + vw)
    return torch.randn((n, c, vh, vw), generator=g)


def destinations(map, h, w):
    """int64 (gh * gw, 6, 6): the source pixel row * w + column that tap (a, b) of every record reads, by the sampler's
    rule"""
    q = map.numpy().reshape(-1, 2).astype(np.int64)
    col, row = q[:, 0] // P, q[:, 1] // P
    taps = np.arange(T, dtype=np.int64)
    r = row[:, None] - 2 + taps
    crossed = (r < 0) | (r >= h)
    r = np.clip(np.where(r < 0, -1 - r, np.where(r >= h, 2 * h - 1 - r, r)), 0, h - 1)
    c = np.mod(col[:, None] - 2 + taps, w)
    turned = np.mod(c + w // 2, w)
    return r[:, :, None] * w + np.where(crossed[:, :, None], turned[:, None, :], c[:, None, :])


def numpy_lists(map, h, w):
    """(start, entry) int64: a stable argsort of the forward walk (s, a, b) by destination"""
    dest = destinations(map, h, w).reshape(-1)
    entry = np.argsort(dest, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(dest, minlength=h * w))])
    return start, entry


def weights(map):
    """(wy, wx) float32 (gh * gw, 6): the phase-table rows of every record"""
    from pseudocylindrical_convolution_amd import erp_rotate
    table = erp_rotate.phases().numpy()
    q = map.numpy().reshape(-1, 2).astype(np.int64)
    return table[np.mod(q[:, 1], P)], table[np.mod(q[:, 0], P)]


def pixel_of_sample(vh, vw, ss):
    s = np.arange(vh * ss * vw * ss)
    return (s // (vw * ss)) // ss * vw + (s % (vw * ss)) // ss


def sequential_scatter(g, map, h, w, vh, vw, ss, into=None):
    """the definition as a plain loop: walk s, a, b in forward order and add ((g' wy[a]) wx[b]) to the destination's
    float32 accumulator, one float32 rounding per operation"""
    n, c = g.shape[:2]
    dest = destinations(map, h, w)
    wy, wx = weights(map)
    pix = pixel_of_sample(vh, vw, ss)
    flat = g.numpy().reshape(n, c, vh * vw)
    if ss > 1:
        flat = flat * np.float32(1.0 / (ss * ss))
    assert flat.dtype == np.float32
    acc = np.zeros((n, c, h * w), dtype=np.float32) if into is None else into.numpy().reshape(n, c, h * w).copy()
    for s in range(dest.shape[0]):
        gs = flat[:, :, pix[s]]
        for a in range(T):
            ga = gs * wy[s, a]
            for b in range(T):
                acc[:, :, dest[s, a, b]] += ga * wx[s, b]
    assert acc.dtype == np.float32
    return torch.from_numpy(acc.reshape(n, c, h, w))


def scatter64(g, map, h, w, vh, vw, ss, absolute=False):
    """the adjoint in float64 from the numpy destinations (np.add.at; no order to speak of): float64 (n, C, h, w).
    absolute=True: the sum of the absolute terms, what a rounding-error bound is relative to"""
    n, c = g.shape[:2]
    dest = destinations(map, h, w)
    wy, wx = (t.astype(np.float64) for t in weights(map))
    flat = g.double().numpy().reshape(n, c, vh * vw)[:, :, pixel_of_sample(vh, vw, ss)]      # (n, c, S)
    if ss > 1:
        flat = flat * np.float64(np.float32(1.0 / (ss * ss)))
    terms = flat[:, :, :, None, None] * (wy[:, :, None] * wx[:, None, :])
    if absolute:
        terms = np.abs(terms)
    acc = np.zeros((n, c, h * w), dtype=np.float64)
    for i in range(n):
        for j in range(c):
            np.add.at(acc[i, j], dest.reshape(-1), terms[i, j].reshape(-1))
    return torch.from_numpy(acc.reshape(n, c, h, w))


def render64(x, map, ss):
    """the forward in float64: torch through erp_rotate.sample_torch on a double tensor plus the float64 average"""
    from pseudocylindrical_convolution_amd import erp_rotate
    out = sum(erp_rotate.sample_torch(x, map[p::ss, t::ss]) for p in range(ss) for t in range(ss))
    return out / (ss * ss) if ss > 1 else out
