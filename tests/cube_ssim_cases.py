"""Shared by tests/test_cube_ssim_cpu.py (CPU) and tests/test_gpu_cube_ssim.py (GPU): the cases of the weighted SSIM
(weighted_metrics.ssim), of the face continuation of any depth (cube.pad(.., depth)) and of cube.ws_ssim.

Planes of the weighted SSIM sit on the edges of its tiling (32 rows x 64 columns per workgroup, 8 rows of one column per
lane, a halo of 5): 1x1 (one pixel, every window mostly padding), 7x13 (one ragged tile), 33x65 (one past a tile in both
directions: four tiles, three of them one pixel wide or high), 37x51 (two tiles down, the halo of the second reaches the
first), 250x500 (8 x 8 tiles, the last of each row and column ragged).  Face sizes 2, 7, 37 and 64: the padded faces of
depth 5 are 12, 17, 47 and 74 pixels wide, the last one crossing the 64-column tile of both kernels.
"""
import numpy as np
import torch

KINDS = ("cmp", "eac")
LAYOUTS = ("faces", "6x1", "3x2")
SHAPES = [(1, 1, 1, 1), (2, 3, 7, 13), (1, 3, 33, 65), (2, 3, 37, 51), (1, 3, 250, 500)]
ERP_SHAPES = [(1, 1, 1, 1), (2, 3, 7, 13), (1, 3, 37, 51)]
FACES = (2, 7, 37)
GPU_FACES = (2, 7, 37, 64)
PLANES = ("erp", "ones", "band")
C1, C2 = 0.01 ** 2, 0.03 ** 2


def case_id(case):
    return "_".join(str(v) for v in case) if isinstance(case, (tuple, list)) else str(case)


def frames(n, c, h, w, seed=0):
    """8-bit noise in [0, 1]"""
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255.


def pair(n, c, h, w):
    """two pictures that are alike: noise, and the noise with a tenth of other noise added"""
    x = frames(n, c, h, w, 1)
    return x, (x + 0.1 * (frames(n, c, h, w, 2) - 0.5)).clamp(0, 1)


def plane(name, h, w):
    """float64 (h, w) numpy: "erp" the cosine of each row, "ones", "band" random positive weights with the middle third of
    the rows zeroed (a mask; a plane of fewer than three rows keeps its weights)"""
    from pseudocylindrical_convolution_amd import sphere_metrics
    if name == "erp":
        return np.repeat(sphere_metrics.weights(h).numpy()[:, None], w, axis=1)
    if name == "ones":
        return np.ones((h, w))
    rng = np.random.RandomState(31 * h + w)
    wt = 10.0 ** rng.uniform(-1.0, 1.0, size=(h, w))
    if h >= 3:
        wt[h // 3:2 * h // 3] = 0.0
    return wt


def quarter_turn(kind, a):
    """int64 (6 a a,): for every pixel of the face stack, row-major, the stack pixel whose centre a quarter turn of yaw
    carries onto it -- built in float64 from cube.direction, face_of and face_position, and checked to land on pixel
    centres: turned[k] = picture[index[k]] is the picture of the scene turned by +90 degrees about the z axis"""
    from pseudocylindrical_convolution_amd import cube
    d = cube.face_grid(kind, a)                                     # (3, 6a, a)
    back = np.stack([d[1], -d[0], d[2]])                            # the direction a turn by +90 degrees carries here
    g, u, v = cube.face_position(kind, a, back)
    assert np.abs(u - np.rint(u)).max() < 1e-9 and np.abs(v - np.rint(v)).max() < 1e-9
    index = (g * a + np.rint(v).astype(np.int64)) * a + np.rint(u).astype(np.int64)
    assert np.array_equal(np.sort(index.ravel()), np.arange(6 * a * a))
    return index.ravel()


def turned(picture, index):
    """the face stack (n, C, 6a, a) with its pixels permuted by `index`"""
    n, c, h, w = picture.shape
    return picture.reshape(n, c, -1)[:, :, torch.from_numpy(index)].reshape(n, c, h, w).contiguous()


def zero_padded(stack, depth):
    """the face stack (n, C, 6a, a) with every face surrounded by `depth` zeros: (n, C, 6A, A), the uncontinued form"""
    n, c, _, a = stack.shape
    A = a + 2 * depth
    out = torch.zeros(n, c, 6, A, A, dtype=stack.dtype, device=stack.device)
    out[:, :, :, depth:depth + a, depth:depth + a] = stack.reshape(n, c, 6, a, a)
    return out.reshape(n, c, 6 * A, A)


def scene(d):
    """an analytic scene on unit directions d (3, ...), in [0, 1]: stripes that cross every cube edge obliquely"""
    x, y, z = d
    return 0.5 + 0.2 * np.sin(9.0 * x + 5.0 * y * z) + 0.15 * np.cos(7.0 * y - 6.0 * z) + 0.1 * np.sin(11.0 * z * x)


def distortion(d):
    """an analytic distortion on unit directions: a finer pattern of a twentieth of the scene's range"""
    x, y, z = d
    return 0.05 * np.sin(23.0 * x - 17.0 * y) * np.cos(19.0 * z + 13.0 * x * y)


def rendered(kind, a, yaw):
    """(x, y) float32 (1, 1, 6a, a): the scene and the distorted scene turned by `yaw` radians about z, evaluated in
    float64 at the direction of every pixel of the face stack: nothing is resampled"""
    from pseudocylindrical_convolution_amd import cube
    d = cube.face_grid(kind, a)
    d = d / np.sqrt((d * d).sum(axis=0))
    c, s = np.cos(yaw), np.sin(yaw)
    d = np.stack([c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2]])
    x = scene(d)
    as_picture = lambda v: torch.from_numpy(v).float()[None, None].contiguous()
    return as_picture(x), as_picture(x + distortion(d))
