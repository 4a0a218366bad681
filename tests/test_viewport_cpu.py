"""Rectilinear viewports (viewport.py, --view, --vp) without a GPU: units and refusals, the host basis against numpy, the
margin that lets the GPU test ask for an equal map, the torch twin against a per-pixel numpy loop of the rule, the
supersampled view as the ordered block mean of the ss = 1 view, the exact centre, the analytic truth, the anti-aliasing
plan, the paper's directions, the metrics and the command line on the oracle backend."""
import ctypes
import re

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import erp_rotate as R, viewport as V
from pseudocylindrical_convolution_amd._native import PconvError

from viewport_cases import ANGLES, CASES, case_id

P = V.PHASES
U = 1 << 16


def _frames(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255. * 1.5 - 0.25   # some of it outside [0, 1]


def test_units_round_once_and_refuse_by_name():
    assert V.view(30, 20, 10, 90, 67.5) == (30 * U, 20 * U, 10 * U, 90 * U, 67 * U + U // 2)
    assert V.view(-75.5, 90, 0, 60, 60) == (-75 * U - U // 2, 90 * U, 0, 60 * U, 60 * U)
    assert V.view(10.8, 0, 0, 100.5, 40)[0] == round(10.8 * U)
    assert V.view(-180, -90, -180, 1, 170) == (-180 * U, -90 * U, -180 * U, U, 170 * U)
    # square pixels: tan(vfov / 2) / tan(hfov / 2) = vh / vw
    v = V.view(0, 0, 0, 90, size=(171, 256))
    assert v[4] == round(np.degrees(2 * np.arctan(171 / 256.)) * U)
    assert V.view(0, 0, 0, 90, size=(64, 64))[4] == 90 * U
    for bad, name in (((180, 0, 0, 90, 90), "yaw"), ((0, 90.001, 0, 90, 90), "pitch"), ((0, 0, -180.001, 90, 90), "roll"),
                      ((0, 0, 0, 0.5, 90), "hfov"), ((0, 0, 0, 170.001, 90), "hfov"), ((0, 0, 0, 90, 171), "vfov"),
                      ((0, 0, 0, 90, 0), "vfov")):
        with pytest.raises(PconvError, match=name):
            V.view(*bad)
    with pytest.raises(PconvError, match="vfov"):
        V.view(0, 0, 0, 120, size=(1000, 100))      # the square pixels' vfov would be 173.4 degrees
    with pytest.raises(PconvError, match="vfov"):
        V.view(0, 0, 0, 90)
    for bad in ((1, 2, 3, 4), (1.5, 0, 0, U, U), "abcde", None, (0, 0, 0, U - 1, U), (0, 0, 0, U, 170 * U + 1)):
        with pytest.raises(PconvError):
            V.check(bad)
    assert V.check([1, 2, 3, U, 2 * U]) == (1, 2, 3, U, 2 * U)
    for bad in ((1, 8), (8, 1), (8, (1 << 20) + 1), "x", (8,)):
        with pytest.raises(PconvError):
            V.view(0, 0, 0, 90, size=bad)
    with pytest.raises(PconvError):
        V.source_map(1, 8, 4, 4, V.view(0, 0, 0, 90, 90))
    with pytest.raises(PconvError):
        V.source_map(8, 16, 1, 4, V.view(0, 0, 0, 90, 90))
    x, q = torch.zeros(1, 1, 8, 16), torch.zeros(8, 8, 2, dtype=torch.int32)
    for args in ((x, q, 4, 4, 5), (x, q, 4, 4, 0), (x, q, 4, 4, 1), (x, q.long(), 4, 4, 2), (x.double(), q, 4, 4, 2),
                 (x[0], q, 4, 4, 2), (x, q, 1, 16, 2)):
        with pytest.raises(PconvError):
            V.render_torch(*args)
    with pytest.raises(PconvError):
        V.Renderer(8, 16, [], (4, 4))
    with pytest.raises(PconvError):
        V.Renderer(8, 16, [V.view(0, 0, 0, 90, 90)], (4, 4), ss=1).render(torch.zeros(1, 1, 8, 8))


def _numpy_matrix(yaw, pitch, roll):
    y, p, r = (np.deg2rad(np.float64(v)) for v in (yaw, -pitch, roll))
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    return rz @ ry @ rx


@pytest.mark.parametrize("angles", ANGLES + [(-180, 0, -180, 1, 170), (10.8, 0, 33, 170, 1)], ids=str)
def test_host_basis_is_numpy(angles):
    v = V.view(*angles)
    m, tx, ty = V.basis(v)
    deg = tuple(k / float(U) for k in v)
    assert m.dtype == np.float64 and m.shape == (3, 3)
    assert np.abs(m - _numpy_matrix(*deg[:3])).max() <= 1e-15
    assert np.array_equal(m, R.matrix(v[:3]))
    for got, fov in ((tx, deg[3]), (ty, deg[4])):
        want = np.tan(np.deg2rad(np.float64(fov)) / 2)
        assert abs(got - want) <= 4e-16 * max(1.0, want)


def test_host_refuses_bad_arguments():
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    out = (ctypes.c_double * 11)()
    addr = ctypes.addressof(out)
    assert lib.pconv_host_viewport_basis(1, 2, 3, U, U, None) == -1 and b"null pointer" in lib.pconv_last_error()
    for bad in ((180 * U, 0, 0, U, U), (0, 90 * U + 1, 0, U, U), (0, 0, -180 * U - 1, U, U)):
        assert lib.pconv_host_viewport_basis(*bad, addr) == -1 and b"out of range" in lib.pconv_last_error()
    for bad in ((0, 0, 0, U - 1, U), (0, 0, 0, U, 170 * U + 1), (0, 0, 0, 0, U), (0, 0, 0, U, -U)):
        assert lib.pconv_host_viewport_basis(*bad, addr) == -1 and b"field of view" in lib.pconv_last_error()
    assert lib.pconv_host_viewport_basis(0, 0, 0, 170 * U, U, addr) == 0
    # the launching entry points check before they launch: nothing here reaches a device
    ok = (1, 2, 3, 90 * U, 60 * U)
    assert lib.pconv_viewport_map(None, 8, 8, 4, 4, *ok, None) == -1 and b"null pointer" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 1, 8, 4, 4, *ok, None) == -1 and b"source side" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 1 << 15, 1 << 15, 4, 4, *ok, None) == -1 and b"source plane" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 8, 8, 1, 4, *ok, None) == -1 and b"grid side" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 8, 8, 4, (1 << 22) + 1, *ok, None) == -1 and b"grid side" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 8, 8, 1 << 14, 1 << 14, *ok, None) == -1 and b"map of" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4100, 8, 8, 4, 4, *ok, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 8, 8, 4, 4, 180 * U, 0, 0, U, U, None) == -1 and b"out of range" in lib.pconv_last_error()
    assert lib.pconv_viewport_map(4096, 8, 8, 4, 4, 0, 0, 0, U, 171 * U, None) == -1 and b"field of view" in lib.pconv_last_error()
    good = [4096, 8192, 16384, 32768]
    render = lib.pconv_viewport_render_f32
    for k in range(4):
        args = list(good)
        args[k] = None
        assert render(*args, 1, 1, 8, 8, 4, 4, 1, 16, 0, None) == -1 and b"null pointer" in lib.pconv_last_error()
    assert render(*good, 70000, 1, 8, 8, 4, 4, 1, 16, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert render(*good, 0, 3, 8, 8, 4, 4, 1, 48, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 1, 4, 4, 1, 16, 0, None) == -1 and b"source side" in lib.pconv_last_error()
    assert render(*good, 1, 1, 1 << 15, 1 << 14, 4, 4, 1, 16, 0, None) == -1 and b"source plane" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 8, 1, 4, 1, 4, 0, None) == -1 and b"view side" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 8, 4, (1 << 20) + 1, 1, 1 << 23, 0, None) == -1 and b"view side" in lib.pconv_last_error()
    for ss in (0, 5, -1):
        assert render(*good, 1, 1, 8, 8, 4, 4, ss, 16, 0, None) == -1 and b"supersampling" in lib.pconv_last_error()
    assert render(*good, 1, 1, 8, 8, 1 << 13, 1 << 13, 2, 1 << 26, 0, None) == -1 and b"map of" in lib.pconv_last_error()
    assert render(*good, 1, 16, 8, 8, 1 << 13, 1 << 12, 1, 1 << 29, 0, None) == -1 and b"output frame" in lib.pconv_last_error()
    assert render(*good, 1, 3, 8, 8, 4, 4, 1, 47, 0, None) == -1 and b"stride" in lib.pconv_last_error()
    assert render(4098, 8192, 16384, 32768, 1, 1, 8, 8, 4, 4, 1, 16, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert render(4096, 8192, 16388, 32768, 1, 1, 8, 8, 4, 4, 1, 16, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert render(4096, 4096, 16384, 32768, 1, 1, 8, 8, 4, 4, 1, 16, 0, None) == -1 and b"distinct" in lib.pconv_last_error()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shared_cases_keep_their_margin(case):
    """u * P and v * P of the float64 map stay 1e-6 away from a rounding boundary (the device's fp64 evaluation is within
    about 1e-10 of numpy's)"""
    h, w, vh, vw, ss, angles = case
    u, v = V.source_coordinates(h, w, vh * ss, vw * ss, V.view(*angles))
    assert u.shape == v.shape == (vh * ss, vw * ss)
    for t in (u * P, v * P):
        margin = np.abs(t - np.floor(t) - 0.5).min()
        assert margin >= 1e-6, margin


def _loop(x, q, vh, vw, ss, clamp):
    """the rule of include/pconv_hip.h pixel by pixel: numpy float32 scalars, python integers"""
    t = R.phases().numpy()
    n, c, h, w = x.shape
    out = np.empty((n, c, vh, vw), dtype=np.float32)
    for j in range(vh):
        for i in range(vw):
            pixel = None
            for p in range(ss):
                for s in range(ss):
                    qu, qv = int(q[j * ss + p, i * ss + s, 0]), int(q[j * ss + p, i * ss + s, 1])
                    col, fx, row, fy = qu // P, qu % P, qv // P, qv % P
                    acc = None
                    for a in range(6):
                        r = row - 2 + a
                        crossed = r < 0 or r >= h
                        r = -1 - r if r < 0 else (2 * h - 1 - r if r >= h else r)
                        r = min(max(r, 0), h - 1)
                        line = None
                        for b in range(6):
                            cc = (col - 2 + b) % w
                            if crossed:
                                cc = (cc + w // 2) % w
                            term = t[fx, b] * x[:, :, r, cc]
                            line = term if line is None else line + term
                        term = t[fy, a] * line
                        acc = term if acc is None else acc + term
                    pixel = acc if pixel is None else pixel + acc
            if ss > 1:
                pixel = pixel * np.float32(1.0 / (ss * ss))
            out[:, :, j, i] = pixel
    return np.clip(out, np.float32(0), np.float32(1)) if clamp else out


@pytest.mark.parametrize("k", [0, 1, 3, 4])
def test_twin_is_the_per_pixel_loop(k):
    h, w, vh, vw, ss, angles = CASES[k]
    if k == 1:
        vh, vw = 13, 22          # the loop in python: a smaller view of the same source, angles and ss
    clamp = k >= 3
    v = V.view(*angles)
    x = _frames(1, 2, h, w, seed=k)
    q = V.source_map(h, w, vh * ss, vw * ss, v)
    assert q.dtype == torch.int32 and tuple(q.shape) == (vh * ss, vw * ss, 2)
    assert np.array_equal(q.numpy(), V.source_map_numpy(h, w, vh * ss, vw * ss, v))
    assert 0 <= int(q[..., 0].min()) and int(q[..., 0].max()) < w * P
    assert -P // 2 <= int(q[..., 1].min()) and int(q[..., 1].max()) <= h * P - P // 2
    got = V.render_torch(x, q, vh, vw, ss, clamp)
    want = _loop(x.numpy(), q.numpy(), vh, vw, ss, clamp)
    assert got.dtype == torch.float32 and got.shape == (1, 2, vh, vw) and np.array_equal(got.numpy(), want)
    assert torch.equal(V.render(x, v, (vh, vw), ss, clamp), got)
    r = V.Renderer(h, w, [v, v], (vh, vw), ss)
    out = torch.full((1, 2, 2, vh, vw), float("nan"))
    assert r.render(x, clamp, out=out) is out and torch.equal(out[:, 0], got) and torch.equal(out[:, 1], got)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_supersampling_is_the_ordered_block_mean_of_the_fine_view(case):
    h, w, vh, vw, ss, angles = case
    v = V.view(*angles)
    x = _frames(2, 3, h, w, seed=5)
    fine = V.render(x, v, (vh * ss, vw * ss), 1)
    want = None
    for p in range(ss):
        for t in range(ss):
            want = fine[..., p::ss, t::ss] if want is None else want + fine[..., p::ss, t::ss]
    if ss > 1:
        want = want * np.float32(1.0 / (ss * ss))
    assert torch.equal(V.render(x, v, (vh, vw), ss), want)
    assert torch.equal(V.render(x, v, (vh, vw), ss, clamp=True), want.clamp(0.0, 1.0))


@pytest.mark.parametrize("roll", [33, 0, -170, 90.25])
def test_the_centre_pixel_is_the_source_pixel_it_looks_at(roll):
    """odd vh, vw, ss = 1, yaw / pitch at the centre of an ERP pixel: d = (1, 0, 0), phase 0 on both axes, whose table
    row is (0, 0, 1, 0, 0, 0), whatever the roll (73.8 degrees is not representable: still phase 0)"""
    h, w, row, col = 50, 100, 12, 70
    yaw, pitch = ((col + 0.5) / w - 0.5) * 360.0, (0.5 - (row + 0.5) / h) * 180.0
    assert (round(yaw, 9), pitch) == (73.8, 45.0)
    x = _frames(2, 3, h, w, seed=1)
    for vh, vw, hfov, vfov in ((9, 15, 90, 67.5), (21, 31, 120, 30), (3, 3, 1, 170)):
        got = V.render(x, V.view(yaw, pitch, roll, hfov, vfov), (vh, vw), 1)
        assert torch.equal(got[:, :, vh // 2, vw // 2], x[:, :, row, col])


def _g(d):
    """the degree-3 function of tests/test_erp_rotate_cpu.py at the directions d (3, ...), normalised here"""
    x, y, z = d / np.sqrt((d * d).sum(0))
    return 0.5 + 0.2 * x * y + 0.15 * z + 0.1 * (x * x - z * z) * y


def _erp_directions(h, w):
    theta = ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi
    phi = (0.5 - (np.arange(h) + 0.5) / h) * np.pi
    return np.stack([np.cos(phi)[:, None] * np.cos(theta)[None, :], np.cos(phi)[:, None] * np.sin(theta)[None, :],
                     np.sin(phi)[:, None] * np.ones((1, w))])


@pytest.mark.parametrize("angles", ANGLES, ids=str)
def test_a_smooth_function_on_the_sphere_is_seen_at_its_analytic_value(angles):
    """a float64 numpy model of the rule gives at most 8.1e-4 from a 32x64 source and 4.5e-4 from 64x128 (the Lanczos-3
    error of a degree-3 harmonic on these grids); the bounds are 1.5 x the model, the first the one the rotation test
    uses for the same sampler.  A wrong sign misses by 0.1 or more"""
    v = V.view(*angles)
    truth = _g(V.directions(21, 31, v))
    err = {}
    for (h, w), bound in (((32, 64), 1.2e-3), ((64, 128), 6.7e-4)):
        x = torch.from_numpy(_g(_erp_directions(h, w))).float()[None, None]
        got = V.render(x, v, (21, 31), 1)[0, 0].double().numpy()
        err[h] = np.abs(got - truth).max()
        print("%s from %dx%d: max error %.3g" % (angles, w, h, err[h]))
        assert err[h] <= bound
    assert err[64] <= 0.6 * err[32]


def test_plan():
    paper = lambda size: V.view(0, 0, 0, 90, size=size)
    assert V.plan(2048, 4096, paper((171, 256)), 171, 256) == (1609, 3218, 4)
    assert V.plan(2048, 4096, paper((683, 1024)), 683, 1024) == (2048, 4096, 2)
    # 1024 columns at 256x171: 4 / pi = 1.27 source pixels per pixel at the centre of a 90 degree view, so two samples;
    # one sample serves where the view is no coarser than the source, from 76 degrees down
    assert abs(V.ratio(512, 1024, paper((171, 256)), 171, 256) - 4 / np.pi) <= 1e-4
    assert V.plan(512, 1024, paper((171, 256)), 171, 256) == (512, 1024, 2)
    assert V.plan(512, 1024, V.view(0, 0, 0, 76, size=(171, 256)), 171, 256) == (512, 1024, 1)
    assert V.plan(512, 1024, V.view(0, 0, 0, 60, size=(171, 256)), 171, 256) == (512, 1024, 1)
    # the thresholds: the ratio itself decides, to 1e-9
    t = lambda r: V.view(0, 0, 0, np.degrees(2 * np.arctan(r * np.pi * 64 / 1024.)), size=(64, 64))
    assert [V.plan(512, 1024, t(r), 64, 64)[2] for r in (0.5, 0.99, 1.01, 1.99, 2.01, 2.99, 3.01, 3.99)] == [1, 1, 2, 2, 3, 3, 4, 4]
    h2, w2, ss = V.plan(512, 1024, t(5.0), 64, 64)
    assert ss == 4 and w2 % 2 == 0 and abs(w2 - 1024 * 4 / 5.0) <= 2 and h2 == round(512 * w2 / 1024.)
    # the taller axis decides where the pixels are not square
    assert V.plan(512, 1024, V.view(0, 0, 0, 20, 52), 64, 64) == (512, 1024, 3)      # 0.90 across, 2.48 down
    # beyond 4 x 8 source pixels per pixel the prefilter is refused
    assert V.plan(2048, 4096, paper((14, 42)), 14, 42)[2] == 4         # 31 x
    with pytest.raises(PconvError, match="source pixels per pixel"):
        V.plan(2048, 4096, paper((13, 39)), 13, 39)                     # 33 x
    with pytest.raises(PconvError):
        V.Renderer(2048, 4096, [paper((13, 39))], (13, 39))


def test_paper_views():
    from pseudocylindrical_convolution_amd.PCONV_operator.ops import MultiProject
    views = V.paper_views((171, 256))
    assert len(views) == 14 == len(MultiProject.THETAS)
    vfov = round(np.degrees(2 * np.arctan(171 / 256.)) * U)
    assert views[0] == (-90 * U, 0, 0, 90 * U, vfov) and views[1] == (0, 0, 0, 90 * U, vfov)
    assert views[3] == (-180 * U, 0, 0, 90 * U, vfov)                  # theta = 1 is written -180
    assert views[4] == (-90 * U, 45 * U, 0, 90 * U, vfov) and views[8][1] == -45 * U
    assert views[12][:3] == (0, 90 * U, 0) and views[13][:3] == (0, -90 * U, 0)
    for v, theta, phi in zip(views, MultiProject.THETAS, MultiProject.PHIS):
        assert V.check(v) == v and v[1] == round(phi * 180 * U) and (v[0] - round(theta * 180 * U)) % (360 * U) == 0
    assert len(set(views)) == 14


def test_metrics_of_the_rendered_views():
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    from pseudocylindrical_convolution_amd.PCONV_operator import pytorch_ssim
    h, w, size = 64, 128, (21, 32)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, h, w, generator=g)
    y = (x + 0.05 * torch.randn(2, 3, h, w, generator=g)).clamp(0, 1)
    views = [V.view(30, 20, 10, 90, size=size), V.view(-100, -60, 0, 70, size=size)]
    r = V.Renderer(h, w, views, size)
    same = V.metrics(r, x, x)
    assert same.dtype == torch.float64 and same.shape == (2, 2)
    assert torch.equal(same[:, 0], torch.zeros(2, dtype=torch.float64)) and (same[:, 1] - 1).abs().max().item() <= 1e-12
    got = V.metrics(r, x, y)
    # by hand, view by view
    per_view = []
    for v in views:
        vx, vy = V.render(x, v, size), V.render(y, v, size)
        mse = ((vx.double() - vy.double()) ** 2).mean(dim=(1, 2, 3))
        e32 = ((vx - vy) * (vx - vy)).double().mean(dim=(1, 2, 3))      # the metric squares the float32 difference
        ssim = torch.stack([pytorch_ssim.ssim(vx[i:i + 1], vy[i:i + 1]).double() for i in range(2)])
        one = V.metrics(V.Renderer(h, w, [v], size), x, y)
        assert (one[:, 0] - e32).abs().max().item() <= 1e-15 and (one[:, 0] - mse).abs().max().item() <= 1e-9
        assert (one[:, 1] - ssim).abs().max().item() <= 1e-5
        assert torch.equal(one, S.metrics(vx, vy, "uniform"))
        per_view.append(one)
    assert (got - (per_view[0] + per_view[1]) / 2).abs().max().item() <= 1e-15
    assert 1e-4 < got[:, 0].min().item() and got[:, 1].max().item() < 0.999


def test_cli_views_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    """--enc --rotate --container of a 256 x 512 PNG; --dec --view writes the view of the picture in the source's
    orientation; --test --vp adds its lines and leaves the others alone; the refusals"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cpu")
    h, w = 256, 512
    _write_png("src.png", h, w, 2)
    common = ["--ssim", "--model-idx", "3", "--height", str(h), "--width", str(w)]
    PC.main(["--enc", "--rotate", "40,-60.5,15", "--container", "--img-list", "src.png", "--code-list", "src.pcv"] + common)
    capsys.readouterr()
    PC.main(["--dec", "--code-list", "src.pcv", "--out-list", "dec.png", "--view", "123.25,-33.5,10,100.5",
             "--view-size", "96x54", "--view-out", "view.png"])
    out = capsys.readouterr().out
    assert "Decoding src.pcv, output to dec.png" in out and "view.png" in out
    seen = PC.read_image("view.png")
    assert seen.shape == (54, 96, 3)
    t2 = PC.PseudoDecoder(56, 0)
    PC.load_models(t2, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    picture = t2("src.pcv")
    assert np.array_equal(PC.tensor2img(picture), PC.read_image("dec.png"))
    view = V.view(123.25, -33.5, 10, 100.5, size=(54, 96))
    assert V.plan(h, w, view, 54, 96)[2] == 3
    assert np.array_equal(PC.tensor2img(V.render(picture, view, (54, 96), clamp=True)), seen)
    capsys.readouterr()
    # --test --ws --vp: the lines of --test --ws as they were (the figures computed here), then one more per image and
    # for the average
    PC.main(["--test", "--code-list", "src.pcv", "--img-list", "src.png", "--ws", "--vp"])
    lines = capsys.readouterr().out.splitlines()
    src = PC.img2tensor(PC.read_image("src.png"), "cpu")
    first = PC._VIEWPORT.format(PC.bitrate("src.pcv", h, w), *PC.ViewportMetrics(0)(src, picture))
    ws = PC._WS.format(*PC.SphericalMetrics(0)(PC.read_image("src.png"), PC.tensor2img(picture)))
    r = V.Renderer(h, w, V.paper_views((85, 128)), (85, 128))
    assert r.ss == 2
    mse, ssim = V.metrics(r, src, picture)[0].tolist()
    vp = "VP-PSNR:%.2fdB, VP-SSIM:%.4f (14 views 128x85, ss=2)" % (10 * np.log10(1 / mse), ssim)
    assert lines == ["Decoding src.pcv, compare it to src.png ", " " + first, " " + ws, " " + vp, "-" * 53,
                     "Average Performance", "-" * 53, first, ws, vp]
    # --vp WxH: that size for every picture
    assert PC.ViewportScore(0, (40, 60))(src, picture)[2] == "(14 views 60x40, ss=3)"
    test = ["--test", "--code-list", "src.pcv", "--img-list", "src.png"]
    # the refusals
    dec = ["--dec", "--code-list", "src.pcv", "--out-list", "y.png"]
    for argv, flag in ((dec + ["--vp"], "--vp"),
                       (["--enc", "--img-list", "src.png", "--code-list", "x.bin", "--vp"] + common, "--vp"),
                       (test + ["--vp", "axb"], "--vp"), (test + ["--vp", "1x40"], "--vp"),
                       (["--test", "--code-list", "src.pcv", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "yuv420p", "--vp"], "--vp"),
                       (test + ["--view", "0,0,0,90", "--view-size", "96x54", "--view-out", "v.png"], "--view"),
                       (dec + ["--view", "0,0,0,90", "--view-out", "v.png"], "--view-size"),
                       (dec + ["--view", "0,0,0,90", "--view-size", "96x54"], "--view-out"),
                       (dec + ["--view", "0,0,0,90", "--view-size", "96x54", "--view-out", "v.png", "--view-out-file", "v.txt"],
                        "--view-out-file"),
                       (dec + ["--view-size", "96x54"], "--view-size"), (dec + ["--view-out", "v.png"], "--view-out"),
                       (dec + ["--view", "0,0,0", "--view-size", "96x54", "--view-out", "v.png"], "--view"),
                       (dec + ["--view", "180,0,0,90", "--view-size", "96x54", "--view-out", "v.png"], "--view"),
                       (dec + ["--view", "0,0,0,171", "--view-size", "96x54", "--view-out", "v.png"], "--view"),
                       (dec + ["--view", "0,0,0,90", "--view-size", "96", "--view-out", "v.png"], "--view-size"),
                       (["--dec", "--code-list", "src.pcv", "--yuv-out", "o.yuv", "--pix-fmt", "yuv420p", "--view", "0,0,0,90",
                         "--view-size", "96x54", "--view-out", "v.png"], "--view")):
        with pytest.raises(SystemExit):
            PC.main(argv)
        assert flag in capsys.readouterr().err, argv
