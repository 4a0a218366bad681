"""CPU: scoring cube pictures on the sphere.  The cube's area weights (cube.area_weights), the weighted metric's torch twin
(weighted_metrics.py) against independent float64 statements, the cube's point records (cube.point_records_numpy) against
the cube -> ERP map and the face stack, the margins that let tests/test_gpu_cube_metrics.py ask for equality with no
exception, the library's host-side refusals, the wrappers' operand contract, and --cube-metrics on the oracle backend."""
import math
import re

import numpy as np
import pytest
import torch

import cube_metrics_cases as MC
from cube_metrics_cases import KINDS, case_id
from pseudocylindrical_convolution_amd import _metric_ops, _native, cube, sphere_metrics, sphere_points
from pseudocylindrical_convolution_amd import weighted_metrics as WM
from pseudocylindrical_convolution_amd._native import PconvError

LAYOUTS = ("faces", "6x1", "3x2")


# ---- 1. the cube's weights ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", [2, 3, 13, 64, 256])
def test_solid_angles_are_positive_symmetric_and_fill_the_sphere(kind, a):
    w = cube.face_weights(kind, a)
    assert w.dtype == np.float64 and w.shape == (a, a) and (w > 0).all()
    assert abs(w.sum() - 4.0 * math.pi / 6.0) <= 1e-12
    for k in range(4):      # the eight symmetries of the square, bit for bit
        assert np.array_equal(np.rot90(w, k), w) and np.array_equal(np.rot90(w, k).T, w)
    stack = cube.area_weights(kind, a)
    assert stack.shape == (6 * a, a) and all(np.array_equal(stack[f * a:(f + 1) * a], w) for f in range(6))
    assert abs(stack.sum() - 4.0 * math.pi) <= 6e-12


def test_the_ratio_of_the_largest_to_the_smallest_pixel():
    ratio = lambda kind, a: cube.face_weights(kind, a).max() / cube.face_weights(kind, a).min()
    assert abs(ratio("cmp", 64) - 5.03) < 0.005 and abs(ratio("cmp", 256) - 5.16) < 0.005 and abs(ratio("eac", 64) - 1.40) < 0.005
    assert ratio("cmp", 256) < 3 * math.sqrt(3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_weights_are_laid_out_by_the_layouts_own_permutation(kind, layout):
    a = 5
    index = torch.arange(6 * a * a, dtype=torch.float32).reshape(1, 1, 6 * a, a)
    where = cube.pack(index, layout)[0, 0].long().numpy()           # which stack pixel each picture pixel is
    for rule in cube.RULES:
        stack = cube.area_weights(kind, a, "faces", rule)
        got = cube.area_weights(kind, a, layout, rule)
        assert got.shape == cube.picture_size(a, layout) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, stack.ravel()[where])
    plane = cube.weight_plane(cube.spec(kind, layout), a)
    assert plane is cube.weight_plane(cube.spec(kind, layout), a) and np.array_equal(plane.weights, cube.area_weights(kind, a, layout))
    assert plane.total == math.fsum(plane.weights.ravel().tolist()) and abs(plane.total - 4 * math.pi) < 1e-12
    with pytest.raises(PconvError, match="rule"):
        cube.area_weights(kind, a, layout, "area")


@pytest.mark.parametrize("kind", KINDS)
def test_density_rule_agrees_with_the_solid_angle(kind):
    exact, density = cube.face_weights(kind, 64), cube.face_weights(kind, 64, "density")
    rel = np.abs(density / exact - 1.0).max()
    print("density against solid angle at a = 64, %s: %.3g relative" % (kind, rel))
    assert rel <= 2.5e-4


_sphere_mean = []


def _field_sphere_mean():
    """the cos-weighted mean of the field over an ERP grid of 4096 x 8192, in float64, row block by row block"""
    if not _sphere_mean:
        h, w = 4096, 8192
        theta = ((np.arange(w, dtype=np.float64) + 0.5) / w - 0.5) * (2.0 * np.pi)
        ct, st = np.cos(theta)[None, :], np.sin(theta)[None, :]
        total = weight = 0.0
        for j0 in range(0, h, 256):
            phi = (0.5 - (np.arange(j0, j0 + 256, dtype=np.float64) + 0.5) / h) * np.pi
            cp, sp = np.cos(phi)[:, None], np.sin(phi)[:, None]
            total += float((MC.field((cp * ct, cp * st, sp * np.ones_like(ct))) * cp).sum())
            weight += float(cp.sum()) * w
        _sphere_mean.append(total / weight)
    return _sphere_mean[0]


@pytest.mark.parametrize("kind", KINDS)
def test_weighted_mean_of_a_field_is_its_sphere_mean(kind):
    want = _field_sphere_mean()
    miss = {}
    for a in (32, 64):
        d = cube.face_grid(kind, a)
        g = MC.field(d / np.sqrt((d * d).sum(axis=0)))
        w = cube.area_weights(kind, a)
        miss[a] = (abs((g * w).sum() / w.sum() - want) / want, abs(g.mean() - want) / want)
    print("%s: weighted miss %.3g (a = 32), %.3g (a = 64), ratio %.3f; uniform miss %.3g, %.1f times the weighted one"
          % (kind, miss[32][0], miss[64][0], miss[32][0] / miss[64][0], miss[32][1], miss[32][1] / miss[32][0]))
    assert miss[32][0] < 1e-4
    assert miss[32][1] >= 10 * miss[32][0] and miss[64][1] >= 10 * miss[64][0]
    assert 3.5 <= miss[32][0] / miss[64][0] <= 4.5


# ---- 2. the weighted metric's twin ----

def _reference_sum(values):
    """the header's order in plain python floats"""
    def tree(lanes):
        s = 128
        while s >= 1:
            for l in range(s):
                lanes[l] = lanes[l] + lanes[l + s]
            s //= 2
        return lanes[0]

    def stage(items, per_lane_stride, block):
        out = []
        for first in range(0, len(items), block):
            lanes = [0.0] * 256
            for l in range(256):
                for k in range(first + l, min(first + block, len(items)), per_lane_stride):
                    lanes[l] = lanes[l] + items[k]
            out.append(tree(lanes))
        return out
    partials = stage(values, 256, 1024)
    return stage(partials, 256, max(len(partials), 1))[0]


@pytest.mark.parametrize("count", [1, 255, 1023, 1024, 1025, 2627, 257 * 1024 - 300])
def test_ordered_sum_is_the_headers_order(count):
    g = torch.Generator().manual_seed(count)
    terms = torch.rand(2, count, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 6, (2, count), generator=g).double()
    got = WM.ordered_sum(terms)
    assert got.shape == (2,) and got[0].item() == _reference_sum(terms[0].tolist()) and got[1].item() == _reference_sum(terms[1].tolist())
    assert abs(got[0].item() - math.fsum(terms[0].tolist())) <= 1e-12 * got[0].item()


@pytest.mark.parametrize("plane", [(37, 71), (32, 32), (5, 205)], ids=case_id)
def test_mse_with_the_erp_plane_is_ws_mse(plane):
    h, w = plane
    x, y = MC.frames(2, 3, h, w, 1), MC.frames(2, 3, h, w, 2)
    got = WM.mse(x, y, WM.erp_plane(h, w))
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3)
    want = sphere_metrics.metrics(x, y)[:, 0]
    assert ((got.mean(dim=1) - want).abs() <= 1e-12 * want).all()
    assert torch.equal(WM.psnr(x, y, WM.erp_plane(h, w)), sphere_metrics.psnr(got.mean(dim=1)))
    assert WM.psnr(x, x, WM.erp_plane(h, w)).tolist() == [math.inf, math.inf]


@pytest.mark.parametrize("plane", MC.PLANES, ids=case_id)
def test_mse_with_ones_is_the_mean_squared_difference(plane):
    h, w = plane
    x, y = MC.frames(2, 3, h, w, 1), MC.frames(2, 3, h, w, 2)
    d = x - y
    want = (d * d).double().mean(dim=(2, 3))
    got = WM.mse(x, y, np.ones((h, w)))
    assert ((got - want).abs() <= 1e-12 * want).all()
    # ... and with any plane it is the weighted mean, within the rounding of two summation orders
    wt = MC.weights(h, w)
    want = ((d * d).double() * torch.from_numpy(wt)).sum(dim=(2, 3)) / wt.sum()
    assert ((WM.mse(x, y, wt) - want).abs() <= 1e-12 * want + 1e-300).all()


@pytest.mark.parametrize("plane", MC.U8_PLANES, ids=case_id)
def test_u8_frames_are_read_as_u8_over_255(plane):
    h, w = plane
    x, y = MC.frames_u8(2, h, w, 1), MC.frames_u8(2, h, w, 2)
    wt = WM.WeightPlane(MC.weights(h, w))
    as_float = lambda t: (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    assert torch.equal(WM.mse(x, y, wt), WM.mse(as_float(x), as_float(y), wt))


def test_the_twins_gradient_is_the_closed_form():
    n, c, h, w = 2, 3, 37, 71
    x, y = MC.frames(n, c, h, w, 1).requires_grad_(True), MC.frames(n, c, h, w, 2).requires_grad_(True)
    plane = WM.WeightPlane(MC.weights(h, w))
    terms = WM.loss_terms(x, y, plane)
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (n,) and terms.requires_grad
    assert torch.equal(terms.detach(), WM.channel_mean(WM.mse_device(x.detach(), y.detach(), plane)))
    coef = torch.tensor([0.75, -1.5], dtype=torch.float64)
    gx, gy = torch.autograd.grad((terms * coef).sum(), (x, y))
    assert gx.dtype == torch.float32 and gx.shape == x.shape
    wt = torch.from_numpy(np.array(plane.weights))
    want = coef[:, None, None, None] * 2.0 * wt * (y.detach().double() - x.detach().double()) / (plane.total * c)
    # k is rounded once to fp32, y - x and the product are fp32 operations: three roundings of 2^-24 each
    bound = 4 * 2.0 ** -24 * want.abs() + 1e-44
    assert ((gy.double() - want).abs() <= bound).all() and ((gx.double() + want).abs() <= bound).all()
    assert (want != 0).any() and (gy[:, :, wt == 0] == 0).all()


def test_loss_terms_gradcheck_in_float64():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 2, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.rand(2, 2, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
    plane = WM.WeightPlane(MC.weights(3, 5, seed=1) + 0.1)
    assert torch.autograd.gradcheck(lambda a, b: WM.loss_terms(a, b, plane), (x, y))


def test_bad_planes_and_operands_are_refused_by_name():
    ok = np.ones((3, 4))
    for bad, word in ((-ok, "negative"), (ok * np.nan, "not finite"), (ok * np.inf, "not finite"), (ok * 0, "all zero"),
                      (ok.astype(np.float32), "float64"), (np.ones(5), "float64"), (torch.ones(3, 4), "float64")):
        with pytest.raises(PconvError, match=word):
            WM.WeightPlane(bad)
    masked = ok.copy()
    masked[0, 1] = 0.0
    assert WM.WeightPlane(masked).total == 11.0 and WM.WeightPlane(torch.from_numpy(masked)).total == 11.0
    x = torch.zeros(1, 1, 3, 4)
    with pytest.raises(PconvError, match="weight plane is 4x3"):
        WM.mse(torch.zeros(1, 1, 3, 5), torch.zeros(1, 1, 3, 5), ok)
    with pytest.raises(PconvError, match="one shape"):
        WM.mse(x, torch.zeros(1, 2, 3, 4), ok)
    with pytest.raises(PconvError, match="uint8 frames carry no gradient"):
        WM.loss_terms(torch.zeros(1, 3, 4, 3, dtype=torch.uint8), torch.zeros(1, 3, 4, 3, dtype=torch.uint8), np.ones((3, 4)))


def test_the_library_refuses_on_the_host():
    """no launch: every refusal comes before (this runs without a GPU)"""
    lib = _native.hip_lib()
    D = 4096      # never dereferenced
    fwd = lambda *a: lib.pconv_weighted_mse_f32(*a)
    cases = [((None, D, D, 1.0, 1, 1, 4, 4, D, D, None), b"null"), ((D + 2, D, D, 1.0, 1, 1, 4, 4, D, D, None), b"aligned"),
             ((D, D, D + 4, 1.0, 1, 1, 4, 4, 2 * D, 3 * D, None), b"aligned"), ((D, D, 2 * D, 1.0, 1, 1, 0, 4, 3 * D, 4 * D, None), b"side"),
             ((D, D, 2 * D, 1.0, 1, 1, (1 << 20) + 1, 1, 3 * D, 4 * D, None), b"side"),
             ((D, D, 2 * D, 1.0, 1, 1, 1 << 15, 1 << 14, 3 * D, 4 * D, None), b"2^31"), ((D, D, 2 * D, 1.0, 256, 256, 4, 4, 3 * D, 4 * D, None), b"planes"),
             ((D, D, 2 * D, 0.0, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"), ((D, D, 2 * D, math.inf, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"),
             ((D, D, 2 * D, math.nan, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"), ((D, D, 2 * D, -1.0, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"),
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 4 * D, D + 8, None), b"alias"), ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 2 * D + 8, 5 * D, None), b"alias"),
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 3 * D + 8, 5 * D, None), b"alias")]
    for args, word in cases:
        assert fwd(*args) < 0 and word in lib.pconv_last_error(), (args, lib.pconv_last_error())
    assert lib.pconv_weighted_mse_u8(D, D, 2 * D, 1.0, 1, 4, 4, 4, 3 * D, 4 * D, None) < 0 and b"C = 4" in lib.pconv_last_error()
    assert lib.pconv_weighted_mse_workspace_bytes(2, 3, 5, 205) == 8 * 6 * 2 and lib.pconv_weighted_mse_workspace_bytes(1, 1, 0, 4) < 0
    back = lambda *a: lib.pconv_weighted_mse_backward_f32(*a)
    for args, word in (((D, D, 2 * D, 1.0, None, 1, 1, 4, 4, 4 * D, None), b"null"), ((D, D, 2 * D, 1.0, 3 * D + 4, 1, 1, 4, 4, 4 * D, None), b"aligned"),
                       ((D, D, 2 * D, 0.0, 3 * D, 1, 1, 4, 4, 4 * D, None), b"positive finite"), ((D, D, 2 * D, 1.0, 3 * D, 1, 1, 4, 4, D + 16, None), b"alias"),
                       ((D, D, 2 * D, 1.0, 3 * D, 1, 1, 4, 4, 2 * D + 8, None), b"alias")):
        assert back(*args) < 0 and word in lib.pconv_last_error(), (args, lib.pconv_last_error())
    rec = lambda *a: lib.pconv_cube_points_records(*a)
    for args, word in (((None, D, 4, 1, 8, None), b"null"), ((D, 2 * D, 4, 3, 8, None), b"kind"), ((D, 2 * D, 4, 1, 1, None), b"face size"),
                       ((D, 2 * D, 0, 1, 8, None), b"points"), ((D, 2 * D, 1 << 28, 1, 8, None), b"points"), ((D + 4, 2 * D, 4, 1, 8, None), b"aligned"),
                       ((D, D + 64, 4, 1, 8, None), b"overlap")):
        assert rec(*args) < 0 and word in lib.pconv_last_error(), (args, lib.pconv_last_error())


def test_wrappers_refuse_cpu_operands_before_the_library(monkeypatch):
    calls = []
    monkeypatch.setattr(_native, "call", lambda fn, *args: calls.append(fn))
    x, wt = torch.zeros(1, 1, 3, 4), torch.ones(3, 4, dtype=torch.float64)
    with pytest.raises(PconvError, match="weighted_mse: x must be"):
        _metric_ops.weighted_mse_device(x, x, wt, 12.0)
    with pytest.raises(PconvError, match="weighted_mse_backward: x must be"):
        _metric_ops.weighted_mse_backward(x, x, wt, 12.0, torch.ones(1, 1, dtype=torch.float64))
    with pytest.raises(PconvError, match="cube_points_records: dirs must be"):
        _metric_ops.cube_points_records(torch.zeros(4, 3, dtype=torch.float64), "cmp", 8)
    assert calls == []


# ---- 3. points of the sphere on a cube picture ----

def _positions(name, kind, a):
    d = cube.point_directions(MC.point_set(name))
    g, u, v = cube.point_positions(kind, a, d)
    return d, g, u, v


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(name, a) for name, sizes in MC.POINT_SETS for a in sizes], ids=case_id)
def test_shared_point_sets_are_away_from_boundaries_and_ties(kind, case):
    name, a = case
    d, g, u, v = _positions(name, kind, a)
    assert np.allclose((d * d).sum(axis=1), 1.0, atol=1e-15, rtol=0)
    assert cube.tie_margin(d.T).min() >= MC.TIE_MARGIN
    hi = a - 0.5 - 1.0 / 256
    qu = (np.clip(u, -0.5, hi) + 3) * 256
    qv = (np.clip(v, -0.5, hi) + 3 + g * (a + 6.0)) * 256
    assert MC.boundary_margin(qu) >= MC.BOUNDARY_MARGIN and MC.boundary_margin(qv) >= MC.BOUNDARY_MARGIN
    rec = cube.point_records_numpy(MC.point_set(name), kind, a)
    assert rec.dtype == np.int32 and rec.shape == (d.shape[0], 2)
    assert np.array_equal(rec[:, 0], np.rint(qu)) and np.array_equal(rec[:, 1], np.rint(qv))
    assert torch.equal(cube.point_records(MC.point_set(name), kind, a), torch.from_numpy(rec))
    assert cube.point_records(MC.point_set(name), kind, a) is cube.point_records(MC.point_set(name), kind, a)


def test_some_shared_points_lie_beyond_the_tighter_clamp():
    beyond = 0
    for kind in KINDS:
        for name, sizes in MC.POINT_SETS:
            for a in sizes:
                _, _, u, v = _positions(name, kind, a)
                beyond += int(((u > a - 0.5 - 1.0 / 256) | (v > a - 0.5 - 1.0 / 256)).sum())
    assert beyond >= 8


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", MC.ERP_GRIDS, ids=case_id)
def test_records_at_an_erp_grid_are_the_cube_to_erp_map(kind, grid):
    h, w, a = grid
    rec = cube.point_records_numpy(MC.erp_points(h, w), kind, a).reshape(h, w, 2)
    map = cube.to_erp_map_numpy(kind, a, h, w, 1)
    g, u, v = cube.to_erp_coordinates(kind, a, h, w, 1)
    hi = a - 0.5 - 1.0 / 256
    below = (u <= hi) & (v <= hi)
    assert below.sum() >= 0.95 * h * w
    assert np.array_equal(rec[below], map[below])
    # beyond the new clamp the record stops at it, 1/256 short of the map's own limit
    far = ~below
    edge = int(np.rint((hi + 3) * 256))
    assert (rec[..., 0][u > hi] == edge).all() and (rec[..., 1][v > hi] == edge + g[v > hi] * (a + 6) * 256).all()
    print("%s %dx%d a = %d: %d of %d centres beyond the clamp, %d records differ" % (kind, w, h, a, far.sum(), h * w, (rec != map).any(axis=2).sum()))
    assert (rec != map).any(axis=2).sum() <= far.sum()
    if (h, w, a) in ((24, 50, 8), (52, 99, 3)):
        assert far.sum() >= 2
    # the sampler on these records is the conversion itself, bit for bit, at those pixels
    y = MC.frames(1, 2, 6 * a, a, seed=3)
    got = sphere_points.sample_torch(cube.pad(y, kind), torch.from_numpy(rec.reshape(-1, 2)), "lanczos").reshape(1, 2, h, w)
    want = cube.to_erp(y, (h, w), kind, ss=1, layout="faces")
    where = torch.from_numpy(below)
    assert torch.equal(got[:, :, where], want[:, :, where])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(name, a) for name, sizes in MC.POINT_SETS for a in sizes], ids=case_id)
def test_nearest_mode_reads_face_pixels_never_the_ring(kind, case):
    name, a = case
    A = a + 6
    stack = torch.arange(6 * a * a, dtype=torch.float32).reshape(1, 1, 6, a, a)
    padded = torch.full((1, 1, 6, A, A), -1.0)                      # a ring no face pixel equals
    padded[:, :, :, 3:3 + a, 3:3 + a] = stack
    rec = cube.point_records(MC.point_set(name), kind, a)
    got = sphere_points.sample_torch(padded.reshape(1, 1, 6 * A, A), rec, "nearest")[0, 0]
    assert (got >= 0).all()
    _, g, u, v = _positions(name, kind, a)
    hi = a - 0.5 - 1.0 / 256
    u, v = np.clip(u, -0.5, hi), np.clip(v, -0.5, hi)
    # the position is quantised to 1/256 pixel before the nearest choice, halves up
    col, row = np.floor(np.rint(u * 256) / 256 + 0.5).astype(np.int64), np.floor(np.rint(v * 256) / 256 + 0.5).astype(np.int64)
    assert col.min() >= 0 and col.max() <= a - 1 and row.min() >= 0 and row.max() <= a - 1
    assert np.array_equal(got.numpy(), stack[0, 0].numpy()[g, row, col])
    # ... which is round(v'), round(u') wherever the position is not within 1/512 of a half
    clear = (np.abs(u - np.floor(u) - 0.5) > 1.0 / 512) & (np.abs(v - np.floor(v) - 0.5) > 1.0 / 512)
    # (a position clamped to -1/2 is on a half, and so is the middle of a face of even size, where the icosphere has vertices)
    assert clear.sum() >= 0.5 * clear.size
    assert np.array_equal(col[clear], np.floor(u[clear] + 0.5)) and np.array_equal(row[clear], np.floor(v[clear] + 0.5))


@pytest.mark.parametrize("interp", sphere_points.INTERPS)
def test_points_mse_takes_any_mix_of_projections(interp):
    ps = MC.point_set("icosphere2")
    erp = MC.frames(2, 3, 16, 32, 1).clamp(0, 1)
    cmp_ = cube.from_erp(erp, 8, "cmp", layout="3x2")
    eac = cube.from_erp(erp, 13, "eac", layout="6x1")
    zero = cube.points_mse(cmp_, cmp_, ps, interp, "cmp", "cmp")
    assert zero.dtype == torch.float64 and tuple(zero.shape) == (2, 3) and (zero == 0).all()
    both = cube.points_mse(cmp_, eac, ps, interp, cube.spec("cmp", "3x2"), cube.spec("eac", "6x1"))
    assert torch.equal(both, cube.points_mse(eac, cmp_, ps, interp, cube.spec("eac", "6x1"), cube.spec("cmp", "3x2")))
    mixed = cube.points_mse(erp, eac, ps, interp, None, cube.spec("eac", "6x1"))
    assert (both > 0).all() and (mixed > 0).all()
    # two ERP operands: sphere_points' own metric, up to the order of the sum
    other = MC.frames(2, 3, 20, 36, 2)
    plain = cube.points_mse(erp, other, ps, interp)
    want = sphere_points.mse(erp, other, ps, interp)
    assert ((plain - want).abs() <= 2 * len(ps) * 2.0 ** -53 * want).all()
    # the layouts are permutations: a picture scores the same in each
    faces = cube.unpack(cmp_, "3x2")
    assert torch.equal(cube.points_mse(faces, erp, ps, interp, cube.spec("cmp", "faces")), cube.points_mse(cmp_, erp, ps, interp, "cmp"))
    with pytest.raises(PconvError, match="layout"):
        cube.points_mse(erp, erp, ps, interp, "cmp")


def test_figures_on_cube_pictures():
    smooth = cube.from_erp(torch.from_numpy(np.stack([0.5 + 0.3 * cube.erp_grid(32, 64)[k] for k in range(3)])[None]).float(), 16, "eac")
    noisy = (smooth + 0.02 * MC.frames(1, 3, 32, 48, 5)).clamp(0, 1)
    figures = [f(smooth, noisy, "eac", "eac", level=3)[0].item() for f in (cube.s_psnr_nn, cube.s_psnr_i)]
    figures += [cube.cpp_psnr(smooth, noisy, "eac", "eac")[0].item(), cube.ws_psnr(smooth, noisy, "eac")[0].item()]
    assert all(20 < v < 50 for v in figures), figures
    assert cube.cpp_psnr(smooth, noisy, "eac", "eac").item() == cube.cpp_psnr(smooth, noisy, "eac", "eac", size=(32, 64)).item()
    assert torch.equal(cube.ws_mse(smooth, noisy, "eac").mean(dim=1), cube.ws_loss_terms(smooth, noisy, "eac"))
    # uniform error, uniform weights or not: the same figure; an error in a corner counts less on the sphere than in the plane
    a = 16
    x = torch.zeros(1, 1, 6 * a, a)
    y = x.clone()
    y[0, 0, 0, 0] = 0.5                                             # a corner pixel of F
    sp = cube.spec("cmp", "faces")
    plain = ((x - y) ** 2).double().mean().item()
    assert cube.ws_mse(x, y, sp).item() < 0.45 * plain
    assert abs(cube.ws_mse(x, x + 0.25, sp).item() - 0.0625) < 1e-15


def test_erp_output_is_trained_against_a_cube_original():
    """ws_loss_terms(from_erp(x), target): the composite's gradient against the same statement in float64 autograd"""
    h, w, a = 24, 48, 12
    sp = cube.spec("eac", "3x2")
    x = MC.frames(1, 2, h, w, seed=2).requires_grad_(True)
    target = MC.frames(1, 2, 2 * a, 3 * a, seed=4)
    loss = cube.ws_loss_terms(cube.from_erp(x, a, sp), target, sp)
    (gx,) = torch.autograd.grad(loss.sum(), x)
    assert gx.shape == x.shape and gx.dtype == torch.float32 and (gx != 0).any()
    # the outer factor alone: d loss / d picture is the closed form; the inner factor is from_erp's own tested backward
    pic = cube.from_erp(x.detach(), a, sp).requires_grad_(True)
    (gp,) = torch.autograd.grad(cube.ws_loss_terms(pic, target, sp).sum(), pic)
    wt = torch.from_numpy(cube.area_weights("eac", a, "3x2"))
    want = 2.0 * wt * (pic.detach().double() - target.double()) / (cube.weight_plane(sp, a).total * 2)
    assert ((gp.double() - want).abs() <= 4 * 2.0 ** -24 * want.abs() + 1e-44).all()
    (chained,) = torch.autograd.grad(cube.from_erp(x, a, sp), x, gp)
    assert torch.equal(gx, chained)


# ---- 4. the command line ----

def test_cli_cube_metrics_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models
    import cube_cases as CC
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cpu")
    sp = cube.spec("eac", "3x2")
    y = cube.from_erp(CC.smooth(64, 128), 32, sp, clamp=True)
    PC.write_image("cube.png", PC.tensor2img(y))
    PC.main(["--enc", "--projection", "eac", "--container", "--img-list", "cube.png", "--code-list", "cube.pcv", "--ssim", "--model-idx", "3"])
    capsys.readouterr()
    test = ["--test", "--projection", "eac", "--code-list", "cube.pcv", "--img-list", "cube.png"]
    PC.main(test)
    plain = capsys.readouterr().out
    assert "CUBE-WS" not in plain and "CUBE-S-PSNR" not in plain and len(re.findall("CUBE-PSNR", plain)) == 2
    PC.main(test + ["--cube-metrics"])
    out = capsys.readouterr().out
    lines = out.splitlines()
    added = [l for l in lines if l.lstrip().startswith(("CUBE-WS-PSNR", "CUBE-S-PSNR-NN"))]
    assert [l for l in lines if l not in added] == plain.splitlines()      # nothing else moved
    at = [k for k, l in enumerate(lines) if "CUBE-PSNR" in l]
    assert len(at) == 2 and all(lines[k + 1].lstrip().startswith("CUBE-WS-PSNR:") and lines[k + 2].lstrip().startswith("CUBE-S-PSNR-NN:")
                                for k in at)
    assert lines[at[0] + 1].startswith(" CUBE-WS") and lines[at[1] + 1].startswith("CUBE-WS")     # per image, then the average
    picture = PC.img2tensor(PC.read_image("cube.png"), "cpu")
    t2 = PC.PseudoDecoder(56, 0)
    PC.load_models(t2, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    back = t2("cube.pcv")
    want = (cube.ws_psnr(picture, back, sp).item(), cube.s_psnr_nn(picture, back, sp, sp).item(), cube.s_psnr_i(picture, back, sp, sp).item(),
            cube.cpp_psnr(picture, back, sp, sp).item())
    assert re.findall(r"CUBE-WS-PSNR:([0-9.]+)dB", out) == ["%.2f" % want[0]] * 2
    assert re.findall(r"CUBE-S-PSNR-NN:([0-9.]+)dB, CUBE-S-PSNR-I:([0-9.]+)dB, CUBE-CPP-PSNR:([0-9.]+)dB", out) == \
        [tuple("%.2f" % v for v in want[1:])] * 2
    assert all(np.isfinite(want)) and all(0 < v < 60 for v in want)      # (the test's models are random: a few dB)
    # the refusals, by name
    for argv in (["--test", "--cube-metrics", "--code-list", "cube.pcv", "--img-list", "cube.png"],
                 ["--enc", "--projection", "eac", "--container", "--cube-metrics", "--img-list", "cube.png", "--code-list", "x.pcv"],
                 ["--dec", "--cube-metrics", "--code-list", "cube.pcv", "--out-list", "y.png"]):
        with pytest.raises(SystemExit):
            PC.main(argv)
        assert "--cube-metrics" in capsys.readouterr().err
