"""Shared by tests/test_cube_loss_cpu.py and tests/test_gpu_cube_loss.py: the cases, the inputs and the float64 statements
the ordered backward of the face continuation (include/pconv_hip.h, pconv_cube_pad_backward_f32) and the backward of the
weighted SSIM (pconv_weighted_ssim_backward_f32) are held to.

The float64 statements are the forwards written as differentiable float64 torch, differentiated by torch:
  pad64       the face continuation: interior copies, ring pixels the bilinear read of the table's record
  sampler64   the 6 x 6 sampler over a map with the ss x ss average (what viewport.render_torch computes), optionally with
              the absolute values of its weights: the adjoint of that with |g| upstream bounds the sum of the magnitudes
              of the terms every gradient element is made of
Bounds.  u = 2^-24.  An ordered float32 sum of L terms, each a rounded product, started from one more value, is within
(L + 1) u sum|terms| of the exact sum to first order; the continuation's coefficients are exact and those of a ring pixel
add to 1, so sum|terms| <= (L + 1) max|g|.  The issue's bound for pad_backward is 4 u L max|g| with L the longest list
+ 1."""
import numpy as np
import torch

U24 = 2.0 ** -24
KINDS = ("cmp", "eac")
DEPTHS = (1, 3, 5, 8)
LIST_FACES = (2, 3, 7)                   # the host lists and the twin on the CPU
GPU_FACES = (2, 3, 7, 12, 67)            # 67: 6 * 67^2 = 26934 pixels, 105 workgroups of 256 and a remainder of 54
PLANES = ((1, 1), (2, 5))                # five planes: one group of four and one of one


def depths(a):
    """the depths of DEPTHS that check_depth allows for a face size of a"""
    from pseudocylindrical_convolution_amd import cube
    from pseudocylindrical_convolution_amd._native import PconvError
    ok = []
    for depth in DEPTHS:
        try:
            cube.check_depth(a, depth)
            ok.append(depth)
        except PconvError:
            pass
    return ok


def pad_cases(faces):
    return [(kind, a, depth) for kind in KINDS for a in faces for depth in depths(a)]


def pad_id(case):
    return "%s-a%d-d%d" % case


def gradient(n, c, h, w, seed):
    """a float32 (n, c, h, w) upstream gradient of unit scale, fixed by the seed"""
    return torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(seed))


def frames(n, c, h, w, seed):
    return torch.rand((n, c, h, w), generator=torch.Generator().manual_seed(seed))


def longest(lists):
    start = lists[0].long()
    return int((start[1:] - start[:-1]).max())


def unpack64(y):
    """cube.unpack of a "3x2" picture (n, C, 2a, 3a) of any float type: the face stack F, R, B, L, U, D"""
    a = y.shape[2] // 2
    top, bottom = y[:, :, :a], y[:, :, a:]
    left, front, right = (top[:, :, :, k * a:(k + 1) * a] for k in range(3))
    down, back, up = (torch.rot90(bottom[:, :, :, k * a:(k + 1) * a], q, (2, 3)) for k, q in ((0, -1), (1, 1), (2, -1)))
    return torch.cat([front, right, back, left, up, down], dim=2)


def pad64(y, kind, depth):
    """the face continuation of a float64 face stack (n, C, 6a, a) in differentiable float64 torch: (n, C, 6A, A)"""
    from pseudocylindrical_convolution_amd import cube
    n, c, _, a = y.shape
    A = a + 2 * depth
    ring = A * A - a * a
    rec = torch.from_numpy(np.array(cube.pad_table(kind, a, depth))).long()
    g = rec[:, 0].clamp(0, 5)
    x0, y0 = (rec[:, 1] >> 8).clamp(0, a - 1), (rec[:, 2] >> 8).clamp(0, a - 1)
    x1, y1 = (x0 + 1).clamp(max=a - 1), (y0 + 1).clamp(max=a - 1)
    fx, fy = (rec[:, 1] & 255).double() / 256.0, (rec[:, 2] & 255).double() / 256.0
    r0, r1 = g * a + y0, g * a + y1
    top = y[:, :, r0, x0] + fx * (y[:, :, r0, x1] - y[:, :, r0, x0])
    bot = y[:, :, r1, x0] + fx * (y[:, :, r1, x1] - y[:, :, r1, x0])
    value = top + fy * (bot - top)
    R, Q = (torch.from_numpy(v) for v in cube.ring_pixels(a, depth))
    face = torch.arange(6).repeat_interleave(ring)
    out = torch.nn.functional.pad(y.reshape(n, c, 6, a, a), (depth,) * 4).clone()
    out[:, :, face, R.repeat(6), Q.repeat(6)] = value
    return out.reshape(n, c, 6 * A, A)


def sampler64(x, map, vh, vw, ss, absolute=False):
    """the 6 x 6 Lanczos-3 sampler over `map` (int32 (vh ss, vw ss, 2)) with the ss x ss average, of a float64 (n, C, h, w)
    source, in differentiable float64 torch: (n, C, vh, vw).  absolute=True: with the magnitudes of the weights"""
    from pseudocylindrical_convolution_amd import erp_rotate
    n, c, h, w = x.shape
    table = erp_rotate.phases().double()
    if absolute:
        table = table.abs()
    q = map.long()
    col0, row0 = torch.div(q[..., 0], 256, rounding_mode="floor") - 2, torch.div(q[..., 1], 256, rounding_mode="floor") - 2
    wx, wy = table[q[..., 0] % 256], table[q[..., 1] % 256]
    out = 0
    for i in range(6):
        r = row0 + i
        crossed = (r < 0) | (r >= h)
        r = torch.where(r < 0, -1 - r, torch.where(r >= h, 2 * h - 1 - r, r)).clamp(0, h - 1)
        for j in range(6):
            col = torch.remainder(col0 + j, w)
            col = torch.where(crossed, torch.remainder(col + w // 2, w), col)
            out = out + x[:, :, r, col] * wx[..., j] * wy[..., i]
    return out.reshape(n, c, vh, ss, vw, ss).mean(dim=(3, 5))


# ---- the weighted SSIM ----

# tests/test_gpu_sphere_loss.py's shapes: the smallest at which tiling (32 x 64), halo (10) and window (11) can go wrong
SSIM_SHAPES = [
    (1, 1, 1, 1),      # single pixel
    (2, 3, 5, 3),      # frame smaller than the window
    (1, 2, 13, 17),    # odd sides below one tile
    (1, 1, 64, 128),   # whole 32 x 64 tiles
    (1, 3, 33, 65),    # one row and one column past a tile edge
    (3, 1, 37, 70),    # several frames with a remainder
    (1, 3, 75, 150),   # several tiles on both axes with remainders
]
EAC_PLANE = "eac-12"   # cube.ssim_plane("eac", 12) on (1, 2, 132, 22): zero rings of 5 around six interiors
SSIM_CASES = [(shape, plane) for shape in SSIM_SHAPES for plane in ("random", "zero-block")] + [((1, 2, 132, 22), EAC_PLANE)]


def ssim_id(case):
    return "%s-%s" % ("x".join(str(v) for v in case[0]), case[1])


def zero_block(h, w):
    """(r0, r1, c0, c1): the middle half of each side, empty for a side below 2"""
    return h // 4, h // 4 + h // 2, w // 4, w // 4 + w // 2


def weight_plane(case):
    from pseudocylindrical_convolution_amd import cube, weighted_metrics
    (n, c, h, w), name = case
    if name == EAC_PLANE:
        return cube.ssim_plane("eac", 12)
    wt = np.random.RandomState(h * 1000 + w).rand(h, w) + 0.1       # random, positive
    if name == "zero-block":
        r0, r1, c0, c1 = zero_block(h, w)
        wt[r0:r1, c0:c1] = 0.0
    return weighted_metrics.WeightPlane(wt)


def ssim_inputs(case):
    """x = rand, y = x + 0.1 randn, neither clamped (float32, CPU), and gout, random per plane, away from zero"""
    shape = case[0]
    g = torch.Generator().manual_seed(sum(shape) + len(case[1]))
    x = torch.rand(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    v = torch.randn(shape[:2], generator=g, dtype=torch.float64)
    return x, y, v + torch.sign(v) * 0.25


_ssim_twins = {}


def ssim_twins(case):
    """(x, y, plane, gout, float64 twin, e32, G) of a case, computed once on the CPU, shared and left unchanged"""
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    key = ssim_id(case)
    if key not in _ssim_twins:
        x, y, gout = ssim_inputs(case)
        plane = weight_plane(case)
        g64 = WM.ssim_backward_torch(x, y, plane, gout, dt=torch.float64)
        g32 = WM.ssim_backward_torch(x, y, plane, gout, dt=torch.float32)
        _ssim_twins[key] = (x, y, plane, gout, g64, (g32.double() - g64).abs().max().item(), g64.abs().max().item())
    return _ssim_twins[key]
