"""CPU: cubemap panoramas, CMP and EAC (pseudocylindrical_convolution_amd/cube.py).  The geometry and its tie rule, the
shared cases held off every rounding boundary and face tie, from_erp against sphere_points.sample (code that predates the
cube), the face continuation, to_erp, the round trip against two passes of erp_rotate.rotate, the layouts, container
version 5, the file codec and the command line on the oracle backend, and autograd.

Which edge of the kernels as built each shape reaches (the CPU twins take the same shapes; tests/test_gpu_cube.py runs
the kernels).  Map kernels: 256 columns per workgroup, one grid row.  Pad kernel: 4 rows x 64 columns of the padded
plane per workgroup, a lane one pixel, grid.y = n * C.  Renderer: 4 rows x 64 columns of the view.
  a = 8      A = 14: one column tile of every kernel; the ring (132 pixels) outweighs the interior (64); ss = 2 puts 16
             samples in a map row
  a = 13     odd: a face centre pixel at s = t = 0; A = 19, 6 A = 114 rows = 28 row groups + 2 rows
  a = 67     A = 73 = 64 + 9: ragged against the 64-wide tile of the pad kernel and the renderer; a ss = 134 map columns
  a = 300    a map row of 300 records: wider than one 256-column map tile (two tiles, the second of 44); A = 306, five
             pad tiles per row, the last of 50
  16x32, 26x52, 134x268   ERP grids of one, one and two map tiles per row (ss = 2: 536 = 2 * 256 + 24, three)
  50x99      an odd width: a column at longitude 0; with ss = 2, 198 columns
  24x50, 52x99, 132x270   stand in at ss = 1 for sizes whose own pixel centres are face ties (tests/cube_cases.py)
  (2, 3) and (1, 1)       grid.y = 6 and 1 planes

Measured bounds (profiles/cube.txt; one smooth picture, 64x128 <-> a = 32, on the CPU):
  ring of pad(from_erp(x)) against x read at the ring pixels' own directions: largest |difference| 0.00619 (cmp),
  0.00965 (eac); the bound is twice that
  round trip PSNR: two rotations 82.04 dB (the yardstick); cmp 78.73 dB (gap 3.31), eac 80.50 dB (gap 1.53); with
  nearest-pixel reads 50.27 / 54.08 dB, 28.47 / 26.43 dB below the sampler's
"""
import re

import numpy as np
import pytest
import torch

import cube_cases as CC
from cube_cases import KINDS, case_id
from pseudocylindrical_convolution_amd import container as C
from pseudocylindrical_convolution_amd import cube, erp_rotate, sphere_points
from pseudocylindrical_convolution_amd._native import PconvError
from pseudocylindrical_convolution_amd.frame_geometry import FrameGeometry

RING_MEASURED = {"cmp": 0.00619, "eac": 0.00965}
ROUND_TRIP_GAP = {"cmp": 3.31, "eac": 1.53}          # dB below two rotations
OVER_NEAREST = {"cmp": 28.47, "eac": 26.43}          # dB above the nearest-pixel round trip


def _points(d):
    """directions (3, ...) -> sphere_points' (P, 2) of (longitude, latitude), with the arithmetic of the map kernels"""
    return np.stack([np.arctan2(d[1], d[0]), np.arctan2(d[2], np.hypot(d[0], d[1]))], axis=-1).reshape(-1, 2)


def _psnr(a, b):
    return 10.0 * np.log10(1.0 / ((a - b).double() ** 2).mean().item())


# ---- 1. geometry ----

@pytest.mark.parametrize("kind", KINDS)
def test_direction_face_and_back(kind):
    g = np.random.default_rng(5)
    for face in range(6):
        s, t = g.uniform(-0.999, 0.999, 500), g.uniform(-0.999, 0.999, 500)
        d = cube.direction(kind, face, s, t)
        got, s2, t2 = cube.face_st(kind, d * g.uniform(0.1, 10.0, 500))        # the length does not matter
        assert (got == face).all()
        assert np.abs(s2 - s).max() < 1e-12 and np.abs(t2 - t).max() < 1e-12
        back = cube.direction(kind, got, s2, t2)
        assert np.abs(back - d).max() < 1e-12
    # the table: right x up = forward, F R B L turn in yaw order, F's top edge is U's bottom edge, its bottom D's top
    for f, r, u in cube.FACES:
        assert np.array_equal(np.cross(r, u), f)
    for k in range(4):
        assert np.array_equal(cube.FACES[k, 1], cube.FACES[(k + 1) % 4, 0]) and np.array_equal(cube.FACES[k, 2], [0, 0, 1])
    s = np.linspace(-0.9, 0.9, 7)
    top, bottom = cube.direction(kind, 0, s, np.ones(7)), cube.direction(kind, 0, s, -np.ones(7))
    _, su, tu = cube.face_st(kind, top, face=4)
    _, sd, td = cube.face_st(kind, bottom, face=5)
    assert np.abs(su - s).max() < 1e-12 and np.abs(tu + 1).max() < 1e-12
    assert np.abs(sd - s).max() < 1e-12 and np.abs(td - 1).max() < 1e-12


def test_tie_rule_on_the_edges_and_corners():
    """ties go to x, then y, then z; the sign picks the face.  The host C function states the same rule"""
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    edges = [(sx, sy, 0) for sx in (1, -1) for sy in (1, -1)] + [(sx, 0, sz) for sx in (1, -1) for sz in (1, -1)] + \
        [(0, sy, sz) for sy in (1, -1) for sz in (1, -1)]
    corners = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    assert len(edges) == 12 and len(corners) == 8
    for d in edges + corners:
        want = (0 if d[0] > 0 else 2) if d[0] != 0 else (1 if d[1] > 0 else 3)
        assert int(cube.face_of(np.array(d, dtype=np.float64))) == want, d
        assert lib.pconv_host_cube_face_of(float(d[0]), float(d[1]), float(d[2])) == want, d
        assert cube.tie_margin(np.array(d, dtype=np.float64)) == 0.0
    for face in range(6):
        f = cube.FACES[face, 0]
        assert int(cube.face_of(f)) == face and lib.pconv_host_cube_face_of(*[float(v) for v in f]) == face


# ---- 2. the cases stay off the boundaries ----

@pytest.mark.parametrize("kind", KINDS)
def test_cases_stay_off_rounding_boundaries_and_face_ties(kind):
    for a, ss, h, w in CC.FROM_ERP:
        u, v = cube.from_erp_coordinates(kind, a, ss, h, w)
        assert CC.boundary_margin(u * 256) >= 1e-7 and CC.boundary_margin(v * 256) >= 1e-7, (a, ss, h, w)
        assert cube.tie_margin(cube.face_grid(kind, a, ss)).min() >= 1e-9      # (a face's own samples: never near a tie)
    for a, h, w, ss in CC.TO_ERP:
        g, u, v = cube.to_erp_coordinates(kind, a, h, w, ss)
        A = a + 2 * cube.PAD
        assert CC.boundary_margin((u + 3) * 256) >= 1e-7 and CC.boundary_margin((v + 3 + g * A) * 256) >= 1e-7, (a, h, w, ss)
        assert cube.tie_margin(cube.erp_grid(h * ss, w * ss)).min() >= 1e-9, (a, h, w, ss)
        assert u.min() >= -0.5 and u.max() <= a - 0.5 and v.min() >= -0.5 and v.max() <= a - 0.5
    for a in CC.FACE_SIZES:
        # the table is built on the host alone, so its ties (the ring's diagonal pixels, |s| = |t|, are exact ties of
        # the other two axes for every a) are decided by the stated rule once and for all; its positions are held off
        # the rounding boundaries like the maps'
        g, u, v = cube.ring_coordinates(kind, a)
        assert CC.boundary_margin(u * 256) >= 1e-7 and CC.boundary_margin(v * 256) >= 1e-7, a
        assert (g != np.arange(6)[:, None]).all()         # the ring never reads its own face


# ---- 3. from_erp against code that exists without the cube ----

_erp_cache = {}


def _erp(n, c, h, w):
    if (n, c, h, w) not in _erp_cache:
        _erp_cache[(n, c, h, w)] = CC.frames(n, c, h, w)
    return _erp_cache[(n, c, h, w)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [c for c in CC.FROM_ERP if c[1] == 1], ids=case_id)
def test_from_erp_is_sphere_points_sample_at_the_face_pixel_centres(kind, case):
    a, ss, h, w = case
    # the face pixel-centre directions, built here
    centre = (np.arange(a) + 0.5) / a
    s, t = (2.0 * centre - 1.0)[None, :], (1.0 - 2.0 * centre)[:, None]
    ps, pt = (np.tan(np.pi / 4.0 * s), np.tan(np.pi / 4.0 * t)) if kind == "eac" else (s, t)
    table = {0: ((1, 0, 0), (0, 1, 0), (0, 0, 1)), 1: ((0, 1, 0), (-1, 0, 0), (0, 0, 1)), 2: ((-1, 0, 0), (0, -1, 0), (0, 0, 1)),
             3: ((0, -1, 0), (1, 0, 0), (0, 0, 1)), 4: ((0, 0, 1), (0, 1, 0), (-1, 0, 0)), 5: ((0, 0, -1), (0, 1, 0), (1, 0, 0))}
    d = np.concatenate([np.stack([f[k] + ps * r[k] + pt * u[k] for k in range(3)]) for f, r, u in (table[i] for i in range(6))],
                       axis=1)
    points = sphere_points.PointSet(_points(d))
    x = _erp(2, 3, h, w)
    records = points.records(h, w).numpy().reshape(6 * a, a, 2)
    assert np.array_equal(records, cube.from_erp_map_numpy(kind, a, 1, h, w))          # the records match everywhere
    want = sphere_points.sample(x, points).reshape(2, 3, 6 * a, a)
    got = cube.from_erp(x, a, kind, ss=1, layout="faces")
    assert torch.equal(got, want)
    assert torch.equal(cube.from_erp(x, a, kind, ss=1, clamp=True, layout="faces"), want.clamp(0.0, 1.0))


def test_default_supersampling_and_its_refusal():
    assert cube.erp_size(8) == (16, 32) and cube.face_size(16, 32) == 8 and cube.face_size(50, 99) == 25
    assert cube.face_size(2, 2) == 2 and cube.face_size(50, 102) == 26
    assert [cube.from_erp_ss(8, 16, w) for w in (16, 32, 33, 64, 65, 128)] == [1, 1, 2, 2, 3, 4]
    assert [cube.to_erp_ss(a, 16, 32) for a in (4, 8, 9, 16, 17, 32)] == [1, 1, 2, 2, 3, 4]
    with pytest.raises(PconvError, match="erp_resample.resize"):
        cube.from_erp_ss(8, 16, 129)
    with pytest.raises(PconvError, match="erp_resample.resize"):
        cube.to_erp_ss(33, 16, 32)
    with pytest.raises(PconvError, match="erp_resample.resize"):
        cube.from_erp(torch.zeros(1, 1, 80, 160), 8)
    x = _erp(1, 1, 16, 32)
    assert cube.from_erp(x, 4, layout="faces").shape == (1, 1, 24, 4)                  # ss = 2 by default
    assert torch.equal(cube.from_erp(x, 4, layout="faces"), cube.from_erp(x, 4, ss=2, layout="faces"))
    for bad in (1, cube.MAX_FACE + 1, 2.5):
        with pytest.raises(PconvError, match="face size"):
            cube.from_erp(x, bad)
    for bad in (0, 5):
        with pytest.raises(PconvError, match="ss"):
            cube.from_erp(x, 8, ss=bad)
    with pytest.raises(PconvError):
        cube.spec("cmq")
    with pytest.raises(PconvError):
        cube.spec("cmp", "2x3")
    assert cube.spec("eac") == ("eac", "3x2") and hash(cube.spec("eac", "6x1")) == hash(cube.Spec("eac", "6x1"))


# ---- 4. the face continuation ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", [8, 13, 67])
def test_pad_constant_interior_and_a_numpy_loop(kind, a):
    A = a + 6
    table = torch.from_numpy(np.array(cube.pad_table(kind, a)))
    assert table.shape == (6 * (12 * a + 36), 3) and table.dtype == torch.int32
    const = torch.full((1, 2, 6 * a, a), 0.3)
    assert torch.equal(cube.pad_torch(const, table), torch.full((1, 2, 6 * A, A), 0.3))
    y = CC.frames(2, 3, 6 * a, a, seed=3)
    got = cube.pad_torch(y, table)
    assert torch.equal(cube.pad(y, kind), got)
    assert np.array_equal(cube.pad_numpy(y.numpy(), table.numpy()), got.numpy())
    assert torch.equal(got.reshape(2, 3, 6, A, A)[:, :, :, 3:3 + a, 3:3 + a], y.reshape(2, 3, 6, a, a))      # a bit copy
    if a == 67:
        return
    # a plain loop over the table, float32 operation by operation
    src, out = y.numpy(), got.numpy().reshape(2, 3, 6, A, A)
    R, Q = cube.ring_pixels(a)
    rec = table.numpy()
    f32 = np.float32
    for face in range(6):
        for k in range(R.size):
            g, qu, qv = (int(v) for v in rec[face * R.size + k])
            x0, y0 = qu >> 8, qv >> 8
            x1, y1 = min(x0 + 1, a - 1), min(y0 + 1, a - 1)
            fx, fy = f32(qu & 255) / f32(256), f32(qv & 255) / f32(256)
            plane = src[:, :, g * a:(g + 1) * a]
            top = plane[:, :, y0, x0] + fx * (plane[:, :, y0, x1] - plane[:, :, y0, x0])
            bot = plane[:, :, y1, x0] + fx * (plane[:, :, y1, x1] - plane[:, :, y1, x0])
            want = top + fy * (bot - top)
            assert want.dtype == np.float32 and np.array_equal(want, out[:, :, face, R[k], Q[k]]), (face, k)


_smooth = {}


def _smooth_case(kind):
    """the smooth 64x128 picture, its faces of a = 32 and the way back: computed once per kind"""
    if kind not in _smooth:
        x = CC.smooth(64, 128)
        faces = cube.from_erp(x, 32, kind, layout="faces")
        _smooth[kind] = (x, faces, cube.to_erp(faces, None, kind, layout="faces"))
    return _smooth[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_the_ring_continues_the_sphere(kind):
    x, faces, _ = _smooth_case(kind)
    a, A = 32, 38
    padded = cube.pad(faces, kind).reshape(1, 3, 6, A, A)
    R, Q = cube.ring_pixels(a)
    want = sphere_points.sample(x, _points(cube.ring_directions(kind, a))).reshape(1, 3, 6, -1)
    worst = (padded[:, :, :, R, Q] - want).abs().max().item()
    print("ring: largest |difference| %.5f (%s)" % (worst, kind))
    assert worst <= 2 * RING_MEASURED[kind]


# ---- 5. to_erp ----

@pytest.mark.parametrize("kind", KINDS)
def test_to_erp_of_constants_and_of_face_indices(kind):
    for a, h, w, ss in ((13, 26, 52, 1), (13, 50, 99, 2)):
        const = torch.full((1, 2, 6 * a, a), 0.7)
        out = cube.to_erp(const, (h, w), kind, ss=ss, layout="faces")
        assert out.shape == (1, 2, h, w) and (out - 0.7).abs().max().item() <= 4e-6
        index = torch.arange(6.0).repeat_interleave(a).reshape(1, 1, 6 * a, 1).expand(1, 1, 6 * a, a).contiguous()
        out = cube.to_erp(index, (h, w), kind, ss=ss, layout="faces")
        g, u, v = cube.to_erp_coordinates(kind, a, h, w, 1)
        # every footprint of the pixel's ss x ss samples inside its own face
        inside = (u >= 3.5) & (u <= a - 4.5) & (v >= 3.5) & (v <= a - 4.5)
        assert set(g[inside].tolist()) == set(range(6))
        got = out[0, 0].numpy()[inside]
        assert np.abs(got - g[inside]).max() <= 4e-6 * 5


# ---- 6. the round trip ----

@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_against_two_rotations(kind):
    x, faces, back = _smooth_case(kind)
    rot = erp_rotate.units(30, 20, 10)
    yardstick = _psnr(erp_rotate.rotate(erp_rotate.rotate(x, rot), rot, inverse=True), x)
    got = _psnr(back, x)
    a, h, w = 32, 64, 128
    nearest = sphere_points.sample_torch(x, cube.from_erp_map(kind, a, 1, h, w).reshape(-1, 2), "nearest").reshape(1, 3, 6 * a, a)
    nearest = sphere_points.sample_torch(cube.pad(nearest, kind), cube.to_erp_map(kind, a, h, w, 1).reshape(-1, 2), "nearest")
    low = _psnr(nearest.reshape(1, 3, h, w), x)
    print("round trip: two rotations %.2f dB, %s %.2f dB, nearest pixel %.2f dB" % (yardstick, kind, got, low))
    assert got >= yardstick - ROUND_TRIP_GAP[kind] - 1.0
    assert got - low >= OVER_NEAREST[kind] - 1.0


# ---- 7. layouts ----

@pytest.mark.parametrize("kind", KINDS)
def test_layouts(kind):
    _, faces, _ = _smooth_case(kind)
    a = 32
    noise = CC.frames(2, 3, 6 * 13, 13, seed=8)
    for layout in ("faces", "6x1", "3x2"):
        for y in (faces, noise):
            packed = cube.pack(y, layout)
            assert tuple(packed.shape[2:]) == cube.picture_size(y.shape[3], layout)
            assert cube.face_size_of(packed.shape, layout) == y.shape[3]
            assert torch.equal(cube.unpack(packed, layout), y)
    y = cube.pack(faces, "3x2")
    assert torch.equal(y[:, :, :a, a:2 * a], faces[:, :, :a]) and torch.equal(y[:, :, :a, :a], faces[:, :, 3 * a:4 * a])   # F, L
    inner = [(y[:, :, r0:r0 + a, c] - y[:, :, r0:r0 + a, c - 1]).abs().mean().item() for r0 in (0, a) for c in (a, 2 * a)]
    seam = (y[:, :, a] - y[:, :, a - 1]).abs().mean().item()
    assert max(inner) < seam, (inner, seam)
    six = cube.pack(faces, "6x1")
    assert torch.equal(six[:, :, :, a:2 * a], faces[:, :, a:2 * a])
    with pytest.raises(PconvError, match="layout"):
        cube.unpack(torch.zeros(1, 1, 20, 31), "3x2")
    assert torch.equal(cube.from_erp(_smooth_case(kind)[0], 32, cube.spec(kind)), y)       # the spec's layout by default
    assert torch.equal(cube.to_erp(y, None, cube.spec(kind)), _smooth_case(kind)[2])


# ---- 8. container ----

def test_container_version_5_and_the_bytes_of_versions_1_to_4():
    payload = b"\x01\x02\x03"
    # literals: what pack_any gave for these fields before version 5 existed
    assert C.pack_any(payload, 256, 512, 3, True, 56).hex() == "504356430101030e1000200003000000010203"
    assert C.pack_any(payload, 250, 500, 2, False, 112).hex() == "504356430200021cfa000000f401000003000000010203"
    assert C.pack_any(payload, 250, 500, 2, False, 112, source=(300, 600)).hex() == \
        "504356430300021cfa000000f40100002c0100005802000003000000010203"
    assert C.pack_any(payload, 250, 500, 1, True, 192, source=(300, 600), rotation=(30 << 16, -(20 << 16), 7)).hex() == \
        "5043564304010130fa000000f40100002c0100005802000000001e000000ecff0700000003000000010203"
    assert C.pack_any(payload, 256, 512, 1, True, 192, rotation=(1, 0, 0)).hex() == \
        "50435643040101300001000000020000000100000002000001000000000000000000000003000000010203"
    assert C.pack_any(payload, 256, 512, 3, True, 56, projection=None) == C.pack_any(payload, 256, 512, 3, True, 56)
    # version 5
    blob = C.pack_any(payload, 128, 256, 3, True, 56, projection=("eac", "3x2", 64))
    assert len(blob) == C.HEADER_BYTES_PROJECTED + 3 == 51 and blob[4] == 5
    assert blob[36:44] == bytes([2, 2, 0, 0, 64, 0, 0, 0]) and blob[24:36] == bytes(12)
    head, body = C.unpack(blob)
    assert body == payload
    assert head == {"height": 128, "width": 256, "model_idx": 3, "ssim": True, "valid_dim": 56, "projection": ("eac", "3x2", 64)}
    blob = C.pack_any(payload, 100, 200, 3, False, 56, source=(128, 256), rotation=(5, -6, 7), projection=("cmp", "faces", 64))
    head, _ = C.unpack(blob)
    assert head["projection"] == ("cmp", "faces", 64) and head["rotation"] == (5, -6, 7)
    assert (head["source_height"], head["source_width"], head["height"], head["width"]) == (128, 256, 100, 200)
    geo = FrameGeometry.from_header(head)
    assert geo.projection == cube.spec("cmp", "faces") and geo.face == 64 and geo.picture == (384, 64) and geo.pixels == 6 * 64 * 64
    assert C.unpack(C.pack_any(payload, model_idx=3, ssim=False, valid_dim=56, **geo.header_fields()))[0] == head
    assert FrameGeometry.for_picture((128, 192), None, None, cube.spec("eac")) == FrameGeometry((128, 256), None, None, cube.spec("eac"))
    assert FrameGeometry((128, 256)).projection is None and FrameGeometry((128, 256)).picture == (128, 256)
    # refusals, by name
    for bad, word in ((("xyz", "3x2", 64), "kind"), ((3, "3x2", 64), "kind"), (("eac", "2x3", 64), "layout"), (("eac", 7, 64), "layout"),
                      (("eac", "3x2", 1), "face size"), (("eac", "3x2", 9454), "face size"), (("eac", "3x2", 60), "face size"),
                      (("eac", "3x2", 64.5), "face size")):
        with pytest.raises(C.ContainerError, match=word):
            C.pack_any(payload, 128, 256, 3, True, 56, projection=bad)
    broken = bytearray(C.pack_any(payload, 128, 256, 3, True, 56, projection=("eac", "3x2", 64)))
    for offset, value, word in ((36, 3, "kind"), (37, 9, "layout"), (38, 1, "reserved"), (40, 63, "face size")):
        data = bytearray(broken)
        data[offset] = value
        with pytest.raises(C.ContainerError, match=word):
            C.unpack(bytes(data))
    with pytest.raises(PconvError, match="2a x 4a"):
        FrameGeometry((128, 250), None, None, cube.spec("eac"))
    with pytest.raises(PconvError, match="layout"):
        FrameGeometry.for_picture((128, 190), None, None, cube.spec("eac"))


# ---- 9. the codec on the oracle backend, the command line, autograd ----

def test_frame_geometry_converts_first_and_last():
    sp = cube.spec("eac", "3x2")
    y = cube.from_erp(CC.smooth(64, 128), 32, sp, clamp=True)
    rot = erp_rotate.units(30, 20, 10)
    geo, plain = FrameGeometry.for_picture(y.shape[2:], (48, 100), rot, sp), FrameGeometry((64, 128), (48, 100), rot)
    assert geo.source == (64, 128) and geo.picture == (64, 96) and geo != plain
    erp = cube.to_erp(y, None, sp, clamp=True)
    assert torch.equal(geo.to_coded(y), plain.to_coded(erp))
    rec = torch.rand(1, 3, *geo.coded, generator=torch.Generator().manual_seed(4))
    assert torch.equal(geo.from_coded(rec), cube.from_erp(plain.from_coded(rec), 32, sp, clamp=True))
    assert torch.equal(geo.from_coded(rec, to_source="erp"), plain.from_coded(rec))
    assert torch.equal(geo.from_coded(rec, to_source=False), plain.from_coded(rec, to_source=False))


def test_cli_projection_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    """--enc --projection eac --container of a 3x2 cube picture of a = 32, then --dec and --test of the file: layout and
    size come from the header alone; the stream is that of coding to_erp(y) directly"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cpu")
    sp = cube.spec("eac", "3x2")
    y = cube.from_erp(CC.smooth(64, 128), 32, sp, clamp=True)
    PC.write_image("cube.png", PC.tensor2img(y))
    common = ["--ssim", "--model-idx", "3"]
    PC.main(["--enc", "--projection", "eac", "--container", "--img-list", "cube.png", "--code-list", "cube.pcv"] + common)
    out = capsys.readouterr().out
    head, payload = C.read("cube.pcv")
    assert head == {"height": 64, "width": 128, "model_idx": 3, "ssim": True, "valid_dim": 56, "projection": ("eac", "3x2", 32)}
    assert C.header_bytes("cube.pcv") == 48
    assert re.findall(r"bitrate: ([0-9.]+)bpp", out) == ["%.3f" % (len(payload) * 8 / float(6 * 32 * 32))]
    # the payload is today's path on the ERP frame of the twin
    picture = PC.img2tensor(PC.read_image("cube.png"), "cpu")
    erp = cube.to_erp(picture, None, sp, clamp=True)
    t1 = PC.PseudoEncoder(56, device_id=0)
    PC.load_models(t1, "demo/ssim/4_56_encoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    plain = FrameGeometry((64, 128))
    t1(plain.to_coded(erp), "direct.pcv", {"model_idx": 3, "ssim": True}, plain)
    dhead, dpayload = C.read("direct.pcv")
    assert "projection" not in dhead and dpayload == payload
    with pytest.raises(ValueError, match="headerless"):
        t1(plain.to_coded(erp), "x.bin", None, FrameGeometry((64, 128), None, None, sp))
    # --dec: the cube picture, from the header alone
    PC.main(["--dec", "--code-list", "cube.pcv", "direct.pcv", "--out-list", "dec.png", "dec_direct.png"])
    dec, dec_direct = PC.read_image("dec.png"), PC.read_image("dec_direct.png")
    assert dec.shape == (64, 96, 3) and dec_direct.shape == (64, 128, 3)
    t2 = PC.PseudoDecoder(56, 0)
    PC.load_models(t2, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    back = cube.from_erp(t2("direct.pcv"), 32, sp, clamp=True)
    assert back.shape == (1, 3, 64, 96) and torch.equal(t2("cube.pcv"), back) and np.array_equal(PC.tensor2img(back), dec)
    capsys.readouterr()
    # --test: the existing lines on the ERP the codec saw, bpp over the cube picture's pixels, and CUBE-PSNR
    PC.main(["--test", "--projection", "eac", "--code-list", "cube.pcv", "--img-list", "cube.png"])
    out = capsys.readouterr().out
    rate, psnr, ssim = re.findall(r"Bitrate:([0-9.]+)bpp, PSNR:([0-9.]+)dB, SSIM:([0-9.]+)", out)[0]
    assert rate == "%.3f" % (len(payload) * 8 / float(6 * 32 * 32)) and np.isfinite(float(psnr)) and np.isfinite(float(ssim))
    figures = re.findall(r"CUBE-PSNR:([0-9.]+)dB", out)
    assert len(figures) == 2 and figures[0] == figures[1] == "%.2f" % _psnr(picture, back)
    with pytest.raises(C.ContainerError, match="records the projection"):
        PC.main(["--test", "--projection", "cmp", "--code-list", "cube.pcv", "--img-list", "cube.png"])
    with pytest.raises(C.ContainerError, match="--projection"):
        PC.decoding_yuv(["cube.pcv"], "out.yuv", dict(fmt="yuv420p", matrix="bt709", range="limited"), model_idx=3, mse=False)
    capsys.readouterr()
    # the refusals: no --container, with --yuv, with --dec, --cube-layout alone
    enc = ["--enc", "--img-list", "cube.png", "--code-list", "x.bin"] + common
    for extra, word in ((["--projection", "eac"], "--projection"), (["--projection", "eac", "--container", "--raw"], "--projection"),
                        (["--projection", "eac", "--container", "--native-size"], "--projection"),
                        (["--projection", "eac", "--container", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "yuv420p"],
                         "--projection"), (["--cube-layout", "6x1", "--container"], "--cube-layout")):
        with pytest.raises(SystemExit):
            PC.main(enc + extra)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        PC.main(["--dec", "--projection", "eac", "--code-list", "cube.pcv", "--out-list", "y.png"])
    assert "--projection" in capsys.readouterr().err


@pytest.mark.parametrize("kind", KINDS)
def test_from_erp_under_autograd_and_to_erp_refused(kind):
    a, ss, h, w = 8, 2, 16, 32
    x = CC.frames(1, 2, h, w, seed=2).requires_grad_(True)
    y = cube.from_erp(x, a, kind, ss=ss, layout="3x2")
    assert y.requires_grad and torch.equal(y.detach(), cube.from_erp(x.detach(), a, kind, ss=ss, layout="3x2"))
    g = CC.frames(1, 2, 2 * a, 3 * a, seed=4)
    (gx,) = torch.autograd.grad(y, x, g)
    # the twin: the same forward written in differentiable torch (float64), by autograd
    xd = x.detach().double().requires_grad_(True)
    table = erp_rotate.phases().double()
    q = cube.from_erp_map(kind, a, ss, h, w).long()
    col0, row0 = torch.div(q[..., 0], 256, rounding_mode="floor") - 2, torch.div(q[..., 1], 256, rounding_mode="floor") - 2
    wx, wy = table[q[..., 0] % 256], table[q[..., 1] % 256]
    out = 0
    for i in range(6):
        r = row0 + i
        crossed = (r < 0) | (r >= h)
        r = torch.where(r < 0, -1 - r, torch.where(r >= h, 2 * h - 1 - r, r)).clamp(0, h - 1)
        for j in range(6):
            c = torch.remainder(col0 + j, w)
            c = torch.where(crossed, torch.remainder(c + w // 2, w), c)
            out = out + xd[:, :, r, c] * wx[..., j] * wy[..., i]
    faces = out.reshape(1, 2, 6 * a, ss, a, ss).mean(dim=(3, 5))
    (want,) = torch.autograd.grad(cube.pack(faces.float(), "3x2").double(), xd, g.double())
    assert (gx.double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    assert torch.equal(gx, torch.autograd.grad(cube.from_erp(x, a, kind, ss=ss, layout="3x2"), x, g)[0])      # in a defined order
    with pytest.raises(PconvError, match="no backward"):
        cube.to_erp(y, None, kind, layout="3x2")
    with pytest.raises(PconvError, match="no backward"):
        cube.to_erp(y.detach().requires_grad_(True), None, kind, layout="3x2")
    assert cube.to_erp(y.detach(), None, kind, layout="3x2").shape == (1, 2, 16, 32)
