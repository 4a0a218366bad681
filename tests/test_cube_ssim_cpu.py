"""CPU: WS-SSIM of cube pictures.  The weighted SSIM's float64 twin (weighted_metrics.ssim_torch) against independent
statements, the face continuation of any depth (cube.pad(.., depth)) against the depth-3 one and its numpy twin,
cube.ws_ssim on constant pictures, under a quarter turn of the cube, on identical pictures and in every layout, the
orientation test, the refusals, and --cube-ssim on the oracle backend."""
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cube_ssim_cases as SC
from cube_ssim_cases import KINDS, LAYOUTS, case_id
from pseudocylindrical_convolution_amd import _metric_ops, _native, cube, sphere_metrics
from pseudocylindrical_convolution_amd import weighted_metrics as WM
from pseudocylindrical_convolution_amd._native import PconvError


# ---- 1. the weighted SSIM's twin ----

@pytest.mark.parametrize("shape", SC.ERP_SHAPES, ids=case_id)
def test_ssim_with_the_erp_plane_is_ws_ssim(shape):
    n, c, h, w = shape
    x, y = SC.pair(n, c, h, w)
    got = WM.ssim(x, y, WM.erp_plane(h, w))
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, c) and got.device.type == "cpu"
    want = sphere_metrics.metrics_torch(x, y)[:, 1]
    assert ((WM.channel_mean(got) - want).abs() <= 1e-12).all(), (WM.channel_mean(got) - want)
    assert torch.equal(WM.ssim_figure(x, y, WM.erp_plane(h, w)), WM.channel_mean(got))


def _direct_ssim(x, y, wt):
    """the definition once more, in float64: the 11 x 11 window g (x) g as one convolution with zero padding of 5, the map,
    the weighted mean"""
    g = torch.tensor([math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)], dtype=torch.float64)
    g = g / g.sum()
    window = (g[:, None] * g[None, :])[None, None]
    n, c, h, w = x.shape
    blur = lambda t: F.conv2d(t.reshape(n * c, 1, h, w), window, padding=5).reshape(n, c, h, w)
    x, y = x.double(), y.double()
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    ssim_map = ((2 * mx * my + SC.C1) * (2 * sxy + SC.C2)) / ((mx * mx + my * my + SC.C1) * (sxx + syy + SC.C2))
    wt = torch.from_numpy(wt)
    return (ssim_map * wt).sum(dim=(2, 3)) / wt.sum()


@pytest.mark.parametrize("name", ["ones", "band"])
@pytest.mark.parametrize("shape", [(2, 3, 7, 13), (1, 3, 37, 51)], ids=case_id)
def test_ssim_over_ones_and_over_a_mask_is_the_direct_statement(shape, name):
    n, c, h, w = shape
    x, y = SC.pair(n, c, h, w)
    wt = SC.plane(name, h, w)
    assert (wt == 0).any() == (name == "band")
    got = WM.ssim(x, y, wt)
    want = _direct_ssim(x, y, wt)
    assert ((got - want).abs() <= 1e-12).all(), (got - want)
    assert (got < 1).all() and (got > 0.5).all()
    # the masked rows do not count: changing them changes nothing ...
    if name == "band":
        x2 = x.clone()
        x2[:, :, h // 3 + 5:2 * h // 3 - 5] = 0.5           # (the rows no window of a weighted pixel reaches)
        if 2 * h // 3 - 5 > h // 3 + 5:
            assert not torch.equal(x2, x) and ((WM.ssim(x2, y, wt) - got).abs() <= 1e-15).all()


def test_identical_pictures_score_one_and_u8_frames_are_read_as_floats():
    x, _ = SC.pair(2, 3, 12, 20)
    assert ((WM.ssim(x, x, SC.plane("band", 12, 20)) - 1).abs() <= 1e-12).all()
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randint(0, 256, (2, 9, 14, 3), generator=g, dtype=torch.uint8) for _ in range(2))
    as_float = lambda t: (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    assert torch.equal(WM.ssim(a, b, np.ones((9, 14))), WM.ssim(as_float(a), as_float(b), np.ones((9, 14))))


# ---- 2. the continuation of any depth ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", SC.FACES)
def test_continuation_of_any_depth(kind, a):
    y = SC.frames(2, 2, 6 * a, a, 3)
    table3 = torch.from_numpy(np.array(cube.pad_table(kind, a)))
    assert np.array_equal(cube.pad_table(kind, a, 3), cube.pad_table(kind, a))
    today = cube.pad_torch(y, table3)
    assert torch.equal(cube.pad_torch(y, table3, depth=3), today) and torch.equal(cube.pad(y, kind, depth=3), today)
    assert torch.equal(cube.pad(y, kind), today)
    for depth in (1, 5, 8):
        A = a + 2 * depth
        table = cube.pad_table(kind, a, depth)
        assert table.dtype == np.int32 and table.shape == (6 * (A * A - a * a), 3) and not table.flags.writeable
        assert cube.pad_table(kind, a, depth) is table                              # cached per depth
        R, Q = cube.ring_pixels(a, depth)
        assert R.size == 4 * depth * (a + depth) and np.array_equal(np.lexsort((Q, R)), np.arange(R.size))      # ring order
        got = cube.pad_torch(y, torch.from_numpy(np.array(table)), depth)
        assert tuple(got.shape) == (2, 2, 6 * A, A) and torch.equal(cube.pad(y, kind, depth), got)
        assert np.array_equal(cube.pad_numpy(y.numpy(), table, depth), got.numpy())
        faces = got.reshape(2, 2, 6, A, A)
        assert torch.equal(faces[:, :, :, depth:depth + a, depth:depth + a], y.reshape(2, 2, 6, a, a))
        const = torch.full((1, 1, 6 * a, a), 0.3)
        assert torch.equal(cube.pad(const, kind, depth), torch.full((1, 1, 6 * A, A), 0.3))     # corners included
    # the ring of depth 3 is the inner part of the ring of depth 5 wherever the EAC limit does not bind
    if kind == "cmp" or a >= 12:
        deep = cube.pad(y, kind, 5).reshape(2, 2, 6, a + 10, a + 10)[:, :, :, 2:-2, 2:-2]
        assert torch.equal(deep.reshape(2, 2, 6 * (a + 6), a + 6), today)


def test_the_eac_limit_binds_at_depth_5_for_faces_up_to_11():
    """the outermost ring pixel lies at |s| = 1 + (2 depth - 1) / a: beyond 7/4 for a < 4 (2 depth - 1) / 3"""
    for depth, last in ((3, 6), (5, 11)):
        for a in (last, last + 1):
            Q = cube.ring_pixels(a, depth)[1]
            s = np.abs(2.0 * ((Q - depth) + 0.5) / a - 1.0)
            assert (s.max() > cube.RING_LIMIT) == (a == last)


# ---- 3. cube.ws_ssim ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("a", SC.FACES)
def test_constant_pictures_score_the_closed_form(kind, layout, a):
    """x = p and y = q everywhere: every window sees constants, so every map value is (2pq + C1) / (p^2 + q^2 + C1): any
    window that read a zero or an unfilled ring pixel would miss it"""
    p, q = 0.25, 0.75
    sp = cube.spec(kind, layout)
    x, y = (torch.full((2, 3) + cube.picture_size(a, layout), v) for v in (p, q))
    want = (2 * p * q + SC.C1) / (p * p + q * q + SC.C1)
    got = cube.ws_ssim(x, y, sp)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and ((got - want).abs() <= 1e-9).all(), got - want
    planes = cube.ws_ssim_planes(x, y, sp)
    assert tuple(planes.shape) == (2, 3) and ((planes - want).abs() <= 1e-9).all()
    # what the continuation is for: the same stacks, uncontinued, read zeros and each other across every edge
    plain = WM.ssim_figure(cube.unpack(x, layout), cube.unpack(y, layout), cube.weight_plane(cube.spec(kind, "faces"), a))
    assert ((plain - want).abs() > 1e-3).all(), plain - want


# What the float64 twin itself measures under a quarter turn: 9.5e-7 (cmp, a = 7), 1.6e-6 (cmp, 12), 2.2e-6 (eac, 7),
# 3.3e-6 (eac, 12).  The pixel permutation is exact; the continuation is not symmetric to the bit: a ring pixel on the
# diagonal of a padded face's corner has a direction that ties between two neighbouring faces, the tie rule (x, y, z with
# >=) picks one, and a quarter turn carries that pixel to one where the rule picks the other neighbour (16 to 26 ring
# pixels of U and of D read another face); elsewhere the bilinear read rounds in another order (1.2e-7).  1e-9 is
# therefore widened to what the twin measures.
TURN_BOUND = 5e-6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", [7, 12])
def test_a_quarter_turn_of_the_cube_leaves_the_figure(kind, a):
    index = SC.quarter_turn(kind, a)
    x, y = SC.pair(2, 3, 6 * a, a)
    sp = cube.spec(kind, "faces")
    before, after = cube.ws_ssim(x, y, sp), cube.ws_ssim(SC.turned(x, index), SC.turned(y, index), sp)
    print("%s a = %d: the figure moves by %.3g under a quarter turn" % (kind, a, (before - after).abs().max().item()))
    assert not torch.equal(SC.turned(x, index), x) and (before < 0.999).all()
    assert ((before - after).abs() <= TURN_BOUND).all(), before - after
    # four quarter turns are the identity
    back = x
    for _ in range(4):
        back = SC.turned(back, index)
    assert torch.equal(back, x)


@pytest.mark.parametrize("kind", KINDS)
def test_identical_pictures_and_layouts(kind):
    a = 7
    x, y = SC.pair(2, 3, 6 * a, a)
    faces = cube.spec(kind, "faces")
    assert ((cube.ws_ssim(x, x, faces) - 1).abs() <= 1e-12).all()
    want = cube.ws_ssim(x, y, faces)
    for layout in ("6x1", "3x2"):
        sp = cube.spec(kind, layout)
        assert torch.equal(cube.ws_ssim(cube.pack(x, layout), cube.pack(y, layout), sp), want)
    # uint8 pictures are read as float(u8) / 255
    u8 = lambda t: (t * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(cube.ws_ssim(u8(x), u8(y), faces), cube.ws_ssim(u8(x).permute(0, 3, 1, 2).float() / 255., u8(y).permute(0, 3, 1, 2).float() / 255., faces))
    assert torch.equal(cube.ws_ssim(x, y, faces, rule="solid-angle"), want)
    assert not torch.equal(cube.ws_ssim(x, y, faces, rule="density"), want)
    assert cube.ssim_plane(kind, a) is cube.ssim_plane(kind, a)
    plane = cube.ssim_plane(kind, a).weights.reshape(6, a + 10, a + 10)
    assert np.array_equal(plane[:, 5:-5, 5:-5], np.broadcast_to(cube.face_weights(kind, a), (6, a, a)))
    assert np.count_nonzero(plane) == 6 * a * a and abs(cube.ssim_plane(kind, a).total - 4 * math.pi) < 1e-12      # the ring is zero


@pytest.mark.parametrize("kind", KINDS)
def test_the_figure_depends_less_on_the_cubes_orientation_when_faces_are_continued(kind):
    """a sanity test: an analytic scene and distortion evaluated at the pixel directions, at yaw 0 and at yaw 45 degrees,
    where the former edges are face centres.  The scene is the same, so the figure should be; the continued form moves
    less than half as much as the form whose faces end in zeros.  Measured in the float64 twin at a = 32: cmp 1.8e-4
    against 2.2e-3, eac 2.2e-4 against 2.3e-3"""
    a = 32
    sp = cube.spec(kind, "faces")
    continued, ended = [], []
    for yaw in (0.0, math.pi / 4):
        x, y = SC.rendered(kind, a, yaw)
        continued.append(cube.ws_ssim(x, y, sp).item())
        ended.append(WM.ssim_figure(SC.zero_padded(x, cube.SSIM_PAD), SC.zero_padded(y, cube.SSIM_PAD), cube.ssim_plane(kind, a)).item())
    moved, moved_ended = abs(continued[0] - continued[1]), abs(ended[0] - ended[1])
    print("%s: continued %.6f / %.6f (moves %.3g), ended in zeros %.6f / %.6f (moves %.3g)"
          % (kind, continued[0], continued[1], moved, ended[0], ended[1], moved_ended))
    assert 0.9 < continued[0] < 0.99
    assert 2 * moved < moved_ended


# ---- 4. refusals ----

def test_bad_operands_are_refused_by_name():
    a = 7
    x = SC.frames(1, 3, 6 * a, a)
    faces = cube.spec("cmp", "faces")
    with pytest.raises(PconvError, match="one kind, layout, face size"):
        cube.ws_ssim(x, SC.frames(1, 3, 6 * 8, 8), faces)                       # another face size
    with pytest.raises(PconvError, match="one kind, layout, face size"):
        cube.ws_ssim(x, cube.pack(x, "6x1"), faces)                             # another layout
    with pytest.raises(PconvError, match="no '3x2' layout"):
        cube.ws_ssim(x, x, cube.spec("cmp", "3x2"))
    with pytest.raises(PconvError, match="kind"):
        cube.ws_ssim(x, x, "erp")
    with pytest.raises(PconvError, match="rule"):
        cube.ws_ssim(x, x, faces, rule="area")
    with pytest.raises(PconvError, match="requires grad"):
        cube.ws_ssim(x.clone().requires_grad_(True), x, faces)
    with pytest.raises(PconvError, match="requires grad"):
        WM.ssim(x, x.clone().requires_grad_(True), np.ones((6 * a, a)))
    with pytest.raises(PconvError, match="weight plane is 7x41"):
        WM.ssim(x, x, np.ones((6 * a - 1, a)))
    with pytest.raises(PconvError, match="one shape"):
        WM.ssim(x, x[:, :2], np.ones((6 * a, a)))
    for depth in (0, 9, -1, 2.5):
        with pytest.raises(PconvError, match="depth"):
            cube.pad(x, "cmp", depth)
        with pytest.raises(PconvError, match="depth"):
            cube.pad_table("cmp", a, depth)
    assert cube.check_depth(9453, 3) == (9453, 3)
    with pytest.raises(PconvError, match="2\\^31"):
        cube.check_depth(9453, 4)
    with pytest.raises(PconvError, match="2\\^31"):
        cube.ring_pixels(9450, 5)
    with pytest.raises(PconvError, match="table must be int32"):
        cube.pad_torch(x, torch.from_numpy(np.array(cube.pad_table("cmp", a))), depth=5)


def test_the_library_refuses_on_the_host():
    """no launch: every refusal comes before (this runs without a GPU)"""
    lib = _native.hip_lib()
    D = 4096      # never dereferenced
    fwd = lambda *a: lib.pconv_weighted_ssim_f32(*a)
    cases = [((None, D, D, 1.0, 1, 1, 4, 4, D, D, None), b"null"), ((D + 2, D, D, 1.0, 1, 1, 4, 4, D, D, None), b"aligned"),
             ((D, D, D + 4, 1.0, 1, 1, 4, 4, 2 * D, 3 * D, None), b"aligned"), ((D, D, 2 * D, 1.0, 1, 1, 0, 4, 3 * D, 4 * D, None), b"side"),
             ((D, D, 2 * D, 1.0, 1, 1, (1 << 20) + 1, 1, 3 * D, 4 * D, None), b"side"),
             ((D, D, 2 * D, 1.0, 1, 1, 1 << 15, 1 << 14, 3 * D, 4 * D, None), b"2^31"), ((D, D, 2 * D, 1.0, 256, 256, 4, 4, 3 * D, 4 * D, None), b"planes"),
             ((D, D, 2 * D, 0.0, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"), ((D, D, 2 * D, math.inf, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"),
             ((D, D, 2 * D, math.nan, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"), ((D, D, 2 * D, -1.0, 1, 1, 4, 4, 3 * D, 4 * D, None), b"positive finite"),
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 4 * D, D + 8, None), b"alias"),          # out inside x
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 4 * D, 2 * D + 8, None), b"alias"),      # out inside y
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, D + 8, 5 * D, None), b"alias"),          # the workspace inside x
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 2 * D + 8, 5 * D, None), b"alias"),      # ... inside y
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 3 * D + 8, 5 * D, None), b"alias"),      # ... inside the weights
             ((D, 2 * D, 3 * D, 1.0, 1, 1, 4, 4, 5 * D, 5 * D, None), b"alias")]          # ... on out
    for args, word in cases:
        assert fwd(*args) < 0 and word in lib.pconv_last_error(), (args, lib.pconv_last_error())
    # one fp64 partial per plane and tile of 32 x 64
    assert lib.pconv_weighted_ssim_workspace_bytes(2, 3, 33, 65) == 8 * 6 * 4 and lib.pconv_weighted_ssim_workspace_bytes(1, 1, 1, 1) == 8
    assert lib.pconv_weighted_ssim_workspace_bytes(1, 1, 0, 4) < 0
    pad = lambda *a: lib.pconv_cube_pad_depth_f32(*a)
    for args, word in (((None, D, 2 * D, 1, 1, 8, 5, None), b"null"), ((D, 2 * D + 2, 3 * D, 1, 1, 8, 5, None), b"aligned"),
                       ((D, 2 * D, 3 * D, 1, 1, 1, 5, None), b"face size"), ((D, 2 * D, 3 * D, 1, 1, 8, 0, None), b"depth"),
                       ((D, 2 * D, 3 * D, 1, 1, 8, 9, None), b"depth"), ((D, 2 * D, 3 * D, 1, 1, 9453, 4, None), b"2^31"),
                       ((D, 2 * D, 3 * D, 1, 1, 9450, 5, None), b"2^31"), ((D, 2 * D, 3 * D, 70000, 1, 8, 5, None), b"planes"),
                       ((D, D, 3 * D, 1, 1, 8, 5, None), b"distinct")):
        assert pad(*args) < 0 and word in lib.pconv_last_error(), (args, lib.pconv_last_error())


def test_wrappers_refuse_cpu_operands_before_the_library(monkeypatch):
    calls = []
    monkeypatch.setattr(_native, "call", lambda fn, *args: calls.append(fn))
    x, wt = torch.zeros(1, 1, 12, 2), torch.ones(12, 2, dtype=torch.float64)
    with pytest.raises(PconvError, match="weighted_ssim: x must be"):
        _metric_ops.weighted_ssim_device(x, x, wt, 24.0)
    with pytest.raises(PconvError, match="cube_pad_depth: x must be"):
        _metric_ops.cube_pad_depth(x, torch.from_numpy(np.array(cube.pad_table("cmp", 2, 5))), 5)
    with pytest.raises(PconvError, match="cube_pad_depth: depth must be"):
        _metric_ops.cube_pad_depth(x, None, 9)
    assert calls == []


# ---- 5. the command line ----

def test_cli_cube_ssim_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
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
    picture = PC.img2tensor(PC.read_image("cube.png"), "cpu")
    t2 = PC.PseudoDecoder(56, 0)
    PC.load_models(t2, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    want = cube.ws_ssim(picture, t2("cube.pcv"), sp).item()
    assert 0 < want < 1
    outs = {}
    for name, extra in (("plain", []), ("ssim", ["--cube-ssim"]), ("both", ["--cube-metrics", "--cube-ssim"])):
        PC.main(test + extra)
        outs[name] = capsys.readouterr().out.splitlines()
    new = lambda l: l.lstrip().startswith("CUBE-WS-SSIM:")
    metrics = lambda l: l.lstrip().startswith(("CUBE-WS-PSNR:", "CUBE-S-PSNR-NN:"))       # the lines of --cube-metrics
    assert not any(new(l) for l in outs["plain"])                                   # absent without the flag
    for name in ("ssim", "both"):
        lines = outs[name]
        assert [l for l in lines if not new(l) and not metrics(l)] == outs["plain"]     # nothing else moved
        assert len([l for l in lines if metrics(l)]) == (4 if name == "both" else 0)
        at = [k for k, l in enumerate(lines) if new(l)]
        assert len(at) == 2                                                         # the image, then the average
        assert lines[at[0]].startswith(" CUBE-WS-SSIM:") and lines[at[1]].startswith("CUBE-WS-SSIM:") and at[1] == len(lines) - 1
        last_cube = "CUBE-S-PSNR-NN" if name == "both" else "CUBE-PSNR"             # after all existing cube lines
        assert all(last_cube in lines[k - 1] for k in at)
        assert re.findall(r"CUBE-WS-SSIM:([0-9.]+)", "\n".join(lines)) == ["%.4f" % want] * 2
    # the refusals, by name
    for argv in (["--test", "--cube-ssim", "--code-list", "cube.pcv", "--img-list", "cube.png"],
                 ["--enc", "--projection", "eac", "--container", "--cube-ssim", "--img-list", "cube.png", "--code-list", "x.pcv"],
                 ["--dec", "--cube-ssim", "--code-list", "cube.pcv", "--out-list", "y.png"]):
        with pytest.raises(SystemExit):
            PC.main(argv)
        assert "--cube-ssim" in capsys.readouterr().err
