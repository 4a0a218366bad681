"""The shared cases of the sphere-sampled metrics (sphere_points.py): picture sizes, cross-size pairs, point sets and
seeded pictures, for test_sphere_points_cpu.py and test_gpu_sphere_points.py."""
import functools
import math

import numpy as np
import torch

SIZES = [(8, 16),
         (6, 4),       # w < 6: tap columns coincide; h small enough that the pole rule and the clamp coincide
         (50, 100),
         (48, 130)]
PAIRS = [((50, 100), (24, 48)), ((8, 16), (6, 4))]
BATCHES = [(1, 1), (3, 3), (1, 3), (3, 1)]     # (n, C)
INTERPS = ["lanczos", "nearest"]
HAND_SIZE = (8, 16)    # the size whose phases the hand-made set hits


def handmade():
    """both poles, t = +-pi exactly, and positions whose phase in a picture of HAND_SIZE is 0, 128 and 255 on both axes"""
    h, w = HAND_SIZE
    pts = [(0.0, math.pi / 2), (0.0, -math.pi / 2), (math.pi, 0.3), (-math.pi, -0.3), (math.pi, math.pi / 2),
           (-math.pi, -math.pi / 2), (1.0, math.pi / 2), (-2.0, -math.pi / 2)]
    for k in (0, 128, 255):
        for i, j in ((0, 0), (5, 3), (14, 6), (7, 0)):
            u, v = i + k / 256., j + k / 256.
            pts.append((((u + 0.5) / w - 0.5) * 2 * math.pi, (0.5 - (v + 0.5) / h) * math.pi))
    return np.array(pts, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def pointset(name):
    """one PointSet per name, shared by the tests (its records are cached inside)"""
    from pseudocylindrical_convolution_amd import sphere_points as SP
    if name == "ico2":
        return SP.PointSet(SP.icosphere(2))        # 162 points: fewer than one lane group
    if name == "ico4":
        return SP.PointSet(SP.icosphere(4))        # 2562 points: three chunks of 1024, the last one partial
    if name == "cpp8x16":
        return SP.PointSet(SP.cpp_grid(8, 16))
    if name == "cpp50x100":
        return SP.PointSet(SP.cpp_grid(50, 100))
    if name == "hand":
        return SP.PointSet(handmade())
    raise KeyError(name)


POINTSETS = ["ico2", "ico4", "cpp8x16", "cpp50x100", "hand"]


def picture(n, c, h, w, seed=0):
    """float32 (n, C, h, w) in [0, 1), seeded"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * h + w)
    return torch.rand(n, c, h, w, generator=g)


def sum_bound(count):
    """the relative difference allowed between two float64 summation orders of `count` non-negative terms: each is
    within (count - 1) 2^-53 relative of the exact sum"""
    return 2.0 * (count - 1) * 2.0 ** -53
