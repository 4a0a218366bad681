"""Shared by tests/test_cube_metrics_cpu.py (CPU) and tests/test_gpu_cube_metrics.py (GPU): the cases of the weighted
metric (weighted_metrics.py) and of the cube's point records (cube.point_records).

Planes of the weighted metric sit on the edges of the reduction (chunks of 1024 pixels, 256 lanes of four, a second stage
of 256 lanes): 1x1 (one lane, one pixel), 1x255 (not every lane), 3x341 = 1023, 32x32 = 1024 (one full chunk), 5x205 =
1025 (a second chunk of one pixel), 37x71 = 2627 (odd, ragged), 513x512 = 262 656 pixels = 256.5 chunks, so 257 partials:
the second stage wraps its 256 lanes; and the face stacks of a = 2, 3, 13 (12x2, 18x3, 78x13).

Point sets of the record tests lie at least BOUNDARY_MARGIN (in 1/256 pixel) from a rounding boundary and TIE_MARGIN
(relative) from a face tie for every (kind, a) they are used with: test_cube_metrics_cpu.py asserts it, so the GPU tests
owe equality with no exception, for EAC too.
"""
import numpy as np
import torch

KINDS = ("cmp", "eac")
PLANES = [(1, 1), (1, 255), (3, 341), (32, 32), (5, 205), (37, 71), (513, 512), (12, 2), (18, 3), (78, 13)]
BATCHES = [(1, 1), (2, 3)]
U8_PLANES = [(5, 205), (37, 71)]
FACE_SIZES = (2, 3, 13)
BOUNDARY_MARGIN = 1e-7
TIE_MARGIN = 1e-9

# (name, face sizes): the point sets of the record tests
# (icosphere(3) and finer have vertices on the 45-degree meridians, exact face ties: level 2 has none)
POINT_SETS = [("icosphere2", (2, 3, 8, 13)), ("cpp_10x22", (3, 8, 13)), ("erp_24x50", (2, 3, 8, 13)), ("erp_52x99", (3, 12)),
              ("erp_16x32", (8,))]
# (h, w, a): ERP grids whose pixel centres are the points, against cube.to_erp_map_numpy(kind, a, h, w, 1); in the first
# two some centres lie beyond the records' tighter clamp
ERP_GRIDS = [(24, 50, 8), (52, 99, 3), (16, 32, 8), (24, 50, 13)]


def case_id(case):
    return "_".join(str(v) for v in case) if isinstance(case, (tuple, list)) else str(case)


def erp_points(h, w):
    """float64 (h w, 2) points (t, p): the pixel centres of an h x w ERP frame, row-major"""
    theta = ((np.arange(w, dtype=np.float64) + 0.5) / w - 0.5) * (2.0 * np.pi)
    phi = (0.5 - (np.arange(h, dtype=np.float64) + 0.5) / h) * np.pi
    return np.stack([np.broadcast_to(theta[None, :], (h, w)).ravel(), np.broadcast_to(phi[:, None], (h, w)).ravel()], axis=1)


_sets = {}


def point_set(name):
    """the PointSet of a name of POINT_SETS (made once)"""
    from pseudocylindrical_convolution_amd import sphere_points
    if name not in _sets:
        kind, _, size = name.partition("_")
        if kind.startswith("icosphere"):
            pts = sphere_points.icosphere(int(kind[len("icosphere"):]))
        else:
            h, w = (int(v) for v in size.split("x"))
            pts = sphere_points.cpp_grid(h, w) if kind == "cpp" else erp_points(h, w)
        _sets[name] = sphere_points.PointSet(pts)
    return _sets[name]


def frames(n, c, h, w, seed=0):
    """8-bit noise stretched to [-0.25, 1.25]: some of it outside [0, 1]"""
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255. * 1.5 - 0.25


def frames_u8(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 77 * h + w)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def weights(h, w, seed=0):
    """float64 (h, w) numpy: positive weights over two decades, with a few exact zeros (a mask) when there is room"""
    rng = np.random.RandomState(seed + 31 * h + w)
    plane = 10.0 ** rng.uniform(-1.0, 1.0, size=(h, w))
    if h * w >= 16:
        plane.ravel()[rng.choice(h * w, size=h * w // 16, replace=False)] = 0.0
    return plane


def field(d):
    """g = (0.3 x + 0.2 y z + 0.1 sin 5z + 0.05 cos 7xy)^2 at unit directions d (3, ...)"""
    x, y, z = d
    return (0.3 * x + 0.2 * y * z + 0.1 * np.sin(5 * z) + 0.05 * np.cos(7 * x * y)) ** 2


def boundary_margin(q):
    """how far the float64 positions q (already multiplied by 256) lie from a rounding boundary (k + 1/2)"""
    return float(np.min(np.abs(q - np.floor(q) - 0.5)))
