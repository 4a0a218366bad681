"""Shared by tests/test_cube_cpu.py (CPU) and tests/test_gpu_cube.py (GPU): the cube <-> ERP cases, all of them away from
every rounding boundary and face tie (test_cube_cpu.py asserts it, so the GPU tests owe equality with no exception).

Face sizes 8, 13 (odd), 67 (ragged against the 64-wide tile), 300 (wider than one 256-column map tile); ERP sizes 16x32,
26x52, 50x99 (odd width), 134x268.  Cube -> ERP, three of the listed sizes are used at ss = 2 only, because their own pixel
centres sit exactly on face ties: a grid width of 4 modulo 8 (52, 268) has centres on the 45-degree meridians, where
|x| = |y|; an odd width (99) has a column at longitude 0 and a height of 2 modulo 4 (50) a row at latitude 45 degrees,
where |x| = |z|.  Their ss = 2 grids (52x104, 100x198, 268x536) have no such centre.  At ss = 1 the sizes 24x50, 52x99
(odd width) and 132x270 stand beside 16x32.
"""
import numpy as np
import torch

KINDS = ("cmp", "eac")

# (a, ss, h, w): ERP h x w -> faces of a
FROM_ERP = [(8, 1, 16, 32), (8, 2, 16, 32), (13, 1, 26, 52), (13, 2, 50, 99), (67, 1, 134, 268), (67, 2, 134, 268),
            (300, 1, 134, 268), (13, 1, 50, 99)]
# (a, h, w, ss): faces of a -> ERP h x w
TO_ERP = [(8, 16, 32, 1), (8, 16, 32, 2), (13, 26, 52, 2), (13, 24, 50, 1), (13, 52, 99, 1), (67, 134, 268, 2), (67, 132, 270, 1),
          (67, 50, 99, 2), (300, 132, 270, 1)]
FACE_SIZES = (8, 13, 67, 300)


def case_id(case):
    return "_".join(str(v) for v in case)


def frames(n, c, h, w, seed=0):
    """8-bit noise stretched to [-0.25, 1.25]: some of it outside [0, 1]"""
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255. * 1.5 - 0.25


def smooth(h, w, c=3):
    """a smooth panorama, float32 (1, c, h, w) in [0, 1]: low-order polynomials of the direction of each pixel"""
    from pseudocylindrical_convolution_amd import cube
    x, y, z = cube.erp_grid(h, w)
    planes = [0.5 + 0.2 * x + 0.15 * y * z + 0.1 * (z * z - x * x),
              0.5 + 0.25 * y - 0.1 * x * z + 0.1 * x * y * z,
              0.5 - 0.2 * z + 0.15 * x * y + 0.1 * (y * y - z * z)]
    return torch.from_numpy(np.stack(planes[:c])[None]).float().contiguous()


def boundary_margin(q):
    """how far the float64 positions q (already multiplied by 256) lie from a rounding boundary (k + 1/2)"""
    return float(np.min(np.abs(q - np.floor(q) - 0.5)))
