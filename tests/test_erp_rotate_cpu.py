"""The sphere rotation of ERP frames (erp_rotate.py, container version 4, --rotate) without a GPU: the host matrix and
phase table against independent float64 evaluations, the torch twin against a per-pixel numpy loop of the rule, the
exact permutations, the analytic truth, the margin that lets the GPU test ask for an equal map, the container, the
frame geometry and the command line on the oracle backend."""
import re

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import container as C
from pseudocylindrical_convolution_amd import erp_resample, erp_rotate as R, erp_size
from pseudocylindrical_convolution_amd._native import PconvError
from pseudocylindrical_convolution_amd.frame_geometry import FrameGeometry

from erp_rotate_cases import ANGLES, CASES, case_id

P = R.PHASES


def _frames(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255.


def _numpy_matrix(yaw, pitch, roll):
    y, p, r = (np.deg2rad(np.float64(v)) for v in (yaw, -pitch, roll))
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    return rz @ ry @ rx


def test_units_round_once_and_refuse_what_is_out_of_range():
    assert R.units(0, 0, 0) is None and R.units(-0.0, 0.0000001, 0) is None
    assert R.units(30, 20, 10) == (30 << 16, 20 << 16, 10 << 16)
    assert R.units(-75.5, 90, 0) == (-75 * 65536 - 32768, 90 << 16, 0)
    assert R.units(10.8, 0, 0) == (round(10.8 * 65536), 0, 0)
    assert R.units(-180, -90, -180) == (-180 << 16, -90 << 16, -180 << 16)
    assert R.units(179.99999, 0, 179.99999) == ((180 << 16) - 1, 0, (180 << 16) - 1)
    for bad in ((180, 0, 0), (0, 90.001, 0), (0, -90.001, 0), (0, 0, 180), (-180.001, 0, 0), (540, 0, 0)):
        with pytest.raises(PconvError):
            R.units(*bad)
    for bad in ((1, 2), (1.5, 0, 0), "abc", (180 << 16, 0, 0)):
        with pytest.raises(PconvError):
            R.check(bad)
    assert R.check((0, 0, 0)) is None and R.check(None) is None and R.check([1, 2, 3]) == (1, 2, 3)
    assert R.degrees(R.units(123.25, -33.5, -170)) == (123.25, -33.5, -170.0)


@pytest.mark.parametrize("angles", ANGLES + [(-180, 0, -180), (10.8, 0, 0), (0, 0, 33)], ids=str)
def test_host_matrix_is_the_numpy_product(angles):
    rot = R.units(*angles)
    m = R.matrix(rot)
    want = _numpy_matrix(*R.degrees(rot))
    assert m.dtype == np.float64 and m.shape == (3, 3)
    assert np.abs(m - want).max() <= 1e-15
    assert np.abs(m @ m.T - np.eye(3)).max() <= 1e-15
    assert np.array_equal(R.matrix(rot, inverse=True), m.T)
    # the source point at longitude yaw, latitude pitch lands in the centre of the picture
    yaw, pitch, _ = (np.deg2rad(v) for v in R.degrees(rot))
    centre = np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)])
    assert np.abs(m @ np.array([1.0, 0, 0]) - centre).max() <= 1e-15


def test_host_refuses_bad_arguments():
    import ctypes
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    m = (ctypes.c_double * 9)()
    assert lib.pconv_host_erp_rotation_matrix(1, 2, 3, 0, None) == -1 and b"null pointer" in lib.pconv_last_error()
    for bad in ((180 << 16, 0, 0), (0, (90 << 16) + 1, 0), (0, 0, (-180 << 16) - 1)):
        assert lib.pconv_host_erp_rotation_matrix(*bad, 0, ctypes.addressof(m)) == -1
        assert b"out of range" in lib.pconv_last_error()
    assert lib.pconv_host_lanczos_phases(None) == -1
    # the launching entry points check before they launch: nothing here reaches a device
    assert lib.pconv_erp_rotation_map(None, 8, 8, 1, 2, 3, 0, None) == -1 and b"null pointer" in lib.pconv_last_error()
    assert lib.pconv_erp_rotation_map(4096, 1, 8, 1, 2, 3, 0, None) == -1 and b"outside" in lib.pconv_last_error()
    assert lib.pconv_erp_rotation_map(4096, 8, 8, 180 << 16, 0, 0, 0, None) == -1 and b"out of range" in lib.pconv_last_error()
    assert lib.pconv_erp_rotation_map(4096, 1 << 15, 1 << 15, 1, 2, 3, 0, None) == -1 and b"2^31" in lib.pconv_last_error()
    assert lib.pconv_erp_rotation_map(4100, 8, 8, 1, 2, 3, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    good = [4096, 8192, 16384, 32768]
    for k in range(4):
        args = list(good)
        args[k] = None
        assert lib.pconv_erp_remap_f32(*args, 1, 1, 8, 8, 0, None) == -1 and b"null pointer" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 1, 1, 8, 1, 0, None) == -1 and b"outside" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 1, 1, (1 << 20) + 1, 8, 0, None) == -1 and b"outside" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 1, 1, 1 << 15, 1 << 14, 0, None) == -1 and b"2^31" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 70000, 1, 8, 8, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(*good, 0, 3, 8, 8, 0, None) == -1 and b"planes" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(4098, 8192, 16384, 32768, 1, 1, 8, 8, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(4096, 8192, 16388, 32768, 1, 1, 8, 8, 0, None) == -1 and b"aligned" in lib.pconv_last_error()
    assert lib.pconv_erp_remap_f32(4096, 4096, 16384, 32768, 1, 1, 8, 8, 0, None) == -1 and b"distinct" in lib.pconv_last_error()


def test_phase_table():
    t = R.phases()
    assert t.dtype == torch.float32 and tuple(t.shape) == (P, 6) == (256, R.TAPS)
    assert t[0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    t64 = t.double().numpy()
    assert np.abs(t64.sum(1) - 1.0).max() <= 6 * 2.0 ** -24
    # phase P - p is phase p seen from the next sample: the reversed row (for p = 0: row 0 shifted by one tap)
    for p in range(1, P):
        assert np.abs(t64[p][::-1] - t64[P - p]).max() <= 2.0 ** -23
    assert t[0].flip(0).tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    # an independent float64 evaluation: numpy's normalised sinc
    x = np.arange(P)[:, None] / float(P) - np.arange(-2, 4)[None, :]
    raw = np.sinc(x) * np.sinc(x / 3.0)
    want = raw / raw.sum(1, keepdims=True)
    assert np.abs(t64 - want).max() <= 2.0 ** -23
    assert np.abs(t64).sum(1).max() <= 1.55 and np.abs(t64).sum(1).argmax() == P // 2


def _loop(x, q, clamp):
    """the rule of include/pconv_hip.h pixel by pixel: numpy float32 scalars, python integers"""
    t = R.phases().numpy()
    n, c, h, w = x.shape
    out = np.empty_like(x)
    for j in range(h):
        for i in range(w):
            qu, qv = int(q[j, i, 0]), int(q[j, i, 1])
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
            out[:, :, j, i] = acc
    return np.clip(out, np.float32(0), np.float32(1)) if clamp else out


@pytest.mark.parametrize("k", range(4))
def test_twin_is_the_per_pixel_loop(k):
    h, w, angles = CASES[5 * k]          # each shape once, each angle set once
    inverse, clamp = bool(k % 2), k >= 2
    rot = R.units(*angles)
    x = _frames(1, 2, h, w, seed=k) * 1.5 - 0.25   # some of it outside [0, 1]
    q = R.source_map(h, w, rot, inverse)
    assert q.dtype == torch.int32 and tuple(q.shape) == (h, w, 2)
    assert np.array_equal(q.numpy(), R.source_map_numpy(h, w, rot, inverse))
    assert 0 <= int(q[..., 0].min()) and int(q[..., 0].max()) < w * P
    assert -P // 2 <= int(q[..., 1].min()) and int(q[..., 1].max()) <= h * P - P // 2
    got = R.rotate_torch(x, q, clamp)
    want = _loop(x.numpy(), q.numpy(), clamp)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert torch.equal(R.rotate(x, rot, inverse, clamp), got)
    out = torch.empty_like(x)
    assert R.rotate(x, rot, inverse, clamp, out=out) is out and torch.equal(out, got)


def test_exact_permutations():
    """a yaw of k columns is a roll of the picture, a half turn of yaw and roll its point reflection: phase 0 on both
    axes, whose row is exactly (0, 0, 1, 0, 0, 0).  180 degrees of yaw or roll is outside the ranges of the rule
    (yaw, roll < 180): the half turns are written -180, the same rotations"""
    for h, w in ((32, 64), (50, 100), (48, 130)):
        x = _frames(2, 3, h, w)
        for k in (1, 3, w // 2 - 1, -5):
            rot = R.units(k * 360.0 / w, 0, 0)      # 10.8 degrees at w = 100 is not representable: still phase 0
            assert torch.equal(R.rotate(x, rot), torch.roll(x, -k, 3)), (h, w, k)
            assert torch.equal(R.rotate(x, rot, inverse=True), torch.roll(x, k, 3)), (h, w, k)
    for h, w in ((32, 64), (50, 100)):
        x = _frames(2, 3, h, w)
        half = R.units(-180, 0, -180)
        assert torch.equal(R.rotate(x, half), torch.roll(x.flip(2, 3), w // 2, 3))
        assert torch.equal(R.rotate(x, half, inverse=True), torch.roll(x.flip(2, 3), w // 2, 3))
    with pytest.raises(PconvError):
        R.units(180, 0, 180)
    x = _frames(1, 1, 8, 16)
    assert R.rotate(x, None) is x and R.rotate(x, (0, 0, 0)) is x and R.rotate(x, R.units(0, 0, 0), clamp=True) is x


def _truth(h, w, m=None):
    """g(d) = 0.5 + 0.2xy + 0.15z + 0.1(x^2 - z^2)y on the h x w grid, at M d when m is given"""
    theta = ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi
    phi = (0.5 - (np.arange(h) + 0.5) / h) * np.pi
    d = np.stack([np.cos(phi)[:, None] * np.cos(theta)[None, :], np.cos(phi)[:, None] * np.sin(theta)[None, :],
                  np.sin(phi)[:, None] * np.ones((1, w))])
    if m is not None:
        d = np.einsum("rk,khw->rhw", m, d)
    x, y, z = d
    return 0.5 + 0.2 * x * y + 0.15 * z + 0.1 * (x * x - z * z) * y


@pytest.mark.parametrize("angles", [(30, 20, 10), (-75.5, 90, 0), (123.25, -33.5, -170)], ids=str)
def test_a_smooth_function_on_the_sphere_is_rotated_to_its_analytic_value(angles):
    """a float64 numpy model of the rule gives 7.9e-4 .. 8.0e-4 at 32x64 and 4.3e-4 .. 4.4e-4 at 64x128 (the Lanczos-3
    error of a degree-3 harmonic on these grids); the bounds are 1.5 x the model.  A wrong sign or pole rule misses
    by 0.1 or more"""
    rot = R.units(*angles)
    err = {}
    for (h, w), bound in (((32, 64), 1.2e-3), ((64, 128), 6.5e-4)):
        x = torch.from_numpy(_truth(h, w)).float()[None, None]
        got = R.rotate(x, rot)[0, 0].double().numpy()
        err[h] = np.abs(got - _truth(h, w, R.matrix(rot))).max()
        print("%s %dx%d max error %.3g" % (angles, w, h, err[h]))
        assert err[h] <= bound
        back = R.rotate(x, rot, inverse=True)[0, 0].double().numpy()
        assert np.abs(back - _truth(h, w, R.matrix(rot, inverse=True))).max() <= bound
    assert err[64] <= 0.6 * err[32]
    x = torch.from_numpy(_truth(32, 64)).float()[None, None]
    there_and_back = R.rotate(R.rotate(x, rot), rot, inverse=True)
    trip = (there_and_back - x).abs().max().item()
    print("%s round trip %.3g" % (angles, trip))
    assert trip <= 1.5e-3


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shared_cases_keep_their_margin(case):
    """u * P and v * P of the float64 map stay 1e-6 away from a rounding boundary (the device's fp64 evaluation is within
    about 1e-10 of numpy's), in both directions"""
    h, w, angles = case
    for inverse in (False, True):
        u, v = R.source_coordinates(h, w, R.units(*angles), inverse)
        for t in (u * P, v * P):
            margin = np.abs(t - np.floor(t) - 0.5).min()
            assert margin >= 1e-6, (inverse, margin)


def test_container_v4_round_trip_and_errors(tmp_path):
    args = dict(height=2048, width=4096, model_idx=3, ssim=True, valid_dim=56)
    rot = R.units(123.25, -33.5, -170)
    blob = C.pack_any(b"\x01\x02\x03", rotation=rot, **args)
    assert len(blob) == 40 + 3 == C.HEADER_BYTES_ROTATED + 3 and blob[:4] == b"PCVC" and blob[4] == 4
    assert C.HEADER_BYTES_SOURCE == 28
    head, payload = C.unpack(blob)
    assert payload == b"\x01\x02\x03" and head == dict(args, rotation=rot)
    # the layout: version 3's, the source size always present, then three signed angles, then the length
    assert blob[:40] == b"PCVC\x04\x01\x03\x0e" + b"".join(v.to_bytes(4, "little") for v in (2048, 4096, 2048, 4096)) + \
        b"".join(v.to_bytes(4, "little", signed=True) for v in rot) + (3).to_bytes(4, "little")
    both = C.unpack(C.pack_any(b"", height=250, width=500, model_idx=0, ssim=False, valid_dim=192, source=(300, 600),
                               rotation=rot))[0]
    assert (both["height"], both["width"], both["source_height"], both["source_width"], both["rotation"]) == \
        (250, 500, 300, 600, rot)
    # no rotation: the bytes of versions 1, 2 and 3 as before
    for extra in ({}, {"source": (4096, 8192)}, {"height": 2880, "width": 5760}):
        plain = C.pack_any(b"xyz", **dict(args, **extra))
        assert plain == C.pack_any(b"xyz", rotation=None, **dict(args, **extra)) == \
            C.pack_any(b"xyz", rotation=(0, 0, 0), **dict(args, **extra))
        assert "rotation" not in C.unpack(plain)[0]
    assert C.pack_any(b"xyz", rotation=(0, 0, 0), **args) == C.pack(b"xyz", **args)
    # angles out of range, in pack and in a file
    for bad in ((180 << 16, 0, 0), (0, (90 << 16) + 1, 0), (0, 0, (-180 << 16) - 1), (1, 2)):
        with pytest.raises(C.ContainerError):
            C.pack_any(b"", rotation=bad, **args)
    with pytest.raises(C.ContainerError):
        C.unpack(blob[:24] + (180 << 16).to_bytes(4, "little", signed=True) + blob[28:])
    # truncated, over-long, unknown version
    for bad in (blob[:30], blob[:39], blob[:-1], blob + b"\x00", blob[:4] + b"\x05" + blob[5:], blob[:4] + b"\x00" + blob[5:]):
        with pytest.raises(C.ContainerError):
            C.unpack(bad)
    # sniff reads enough for the longest header
    boxed = str(tmp_path / "a.pcv")
    C.write_any(boxed, b"\x05" * 40, rotation=rot, source=(300, 600), **dict(args, height=256, width=512))
    assert C.sniff(boxed) == dict(args, height=256, width=512, source_height=300, source_width=600, rotation=rot)
    assert C.header_bytes(boxed) == 40 and C.read(boxed)[1] == b"\x05" * 40


@pytest.mark.parametrize("source,content", [((256, 512), None), ((250, 500), None), ((300, 600), (250, 500))], ids=str)
def test_geometry_rotates_first_and_back_last(source, content):
    rot = R.units(30, 20, 10)
    geo, plain = FrameGeometry(source, content, rot), FrameGeometry(source, content)
    assert geo.rotated and geo.rotation == rot and not plain.rotated and plain.rotation is None
    assert geo != plain and FrameGeometry(source, content, (0, 0, 0)) == plain == FrameGeometry(source, content, None)
    assert (geo.source, geo.content, geo.coded, geo.pixels) == (plain.source, plain.content, plain.coded, plain.pixels)
    assert set(plain.header_fields()) == {"height", "width", "source"}
    assert set(geo.header_fields()) == {"height", "width", "source", "rotation"} and geo.header_fields()["rotation"] == rot
    blob = C.pack_any(b"\x01", model_idx=3, ssim=True, valid_dim=56, **geo.header_fields())
    assert blob[4] == 4
    again = FrameGeometry.from_header(C.unpack(blob)[0])
    assert again == geo and hash(again) == hash(geo) and FrameGeometry.for_raw(*source) == FrameGeometry(source)
    with pytest.raises(PconvError):
        FrameGeometry(source, content, (180 << 16, 0, 0))
    x = torch.rand(1, 3, *source, generator=torch.Generator().manual_seed(3))
    turned = R.rotate(x, rot, clamp=True)
    assert torch.equal(geo.to_coded(x), plain.to_coded(turned))
    rec = torch.rand(1, 3, *geo.coded, generator=torch.Generator().manual_seed(4))
    assert torch.equal(geo.from_coded(rec), R.rotate(plain.from_coded(rec), rot, inverse=True, clamp=True))
    assert torch.equal(geo.from_coded(rec, to_source=False), plain.from_coded(rec, to_source=False))


def test_cli_rotate_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    """--enc --rotate --container of a 256 x 512 PNG, then --dec and --test of the file"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cpu")
    h, w = 256, 512
    _write_png("src.png", h, w, 2)
    common = ["--ssim", "--model-idx", "3", "--height", str(h), "--width", str(w)]
    rot = R.units(40, -60.5, 15)
    PC.main(["--enc", "--rotate", "40,-60.5,15", "--container", "--img-list", "src.png", "--code-list", "src.pcv"] + common)
    out = capsys.readouterr().out
    head, payload = C.read("src.pcv")
    assert head == {"height": h, "width": w, "model_idx": 3, "ssim": True, "valid_dim": 56, "rotation": rot}
    assert C.header_bytes("src.pcv") == 40
    assert re.findall(r"bitrate: ([0-9.]+)bpp", out) == ["%.3f" % (len(payload) * 8 / float(h * w))]
    # the payload is today's path on the twin-rotated picture
    turned = R.rotate(PC.img2tensor(PC.read_image("src.png"), "cpu"), rot, clamp=True)
    t1 = PC.PseudoEncoder(56, device_id=0)
    PC.load_models(t1, "demo/ssim/4_56_encoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    t1(turned, "direct.pcv", {"model_idx": 3, "ssim": True})
    dhead, dpayload = C.read("direct.pcv")
    assert "rotation" not in dhead and dpayload == payload
    with pytest.raises(ValueError, match="headerless"):
        t1(turned, "x.bin", None, FrameGeometry((h, w), None, rot))
    # --dec restores a picture of the source's size in the source's orientation: the direct file's decode, turned back
    PC.main(["--dec", "--code-list", "src.pcv", "direct.pcv", "--out-list", "dec.png", "dec_direct.png"])
    dec, dec_direct = PC.read_image("dec.png"), PC.read_image("dec_direct.png")
    assert dec.shape == dec_direct.shape == (h, w, 3)
    t2 = PC.PseudoDecoder(56, 0)
    PC.load_models(t2, "demo/ssim/4_56_decoder.pt", "demo/ssim/4_56_ent.pt", "cpu")
    back = R.rotate(t2("direct.pcv"), rot, inverse=True, clamp=True)
    assert np.array_equal(PC.tensor2img(back), dec) and torch.equal(t2("src.pcv"), back)
    capsys.readouterr()
    # --test scores against the unrotated source; --rotate there must agree with the file
    PC.main(["--test", "--rotate", "40,-60.5,15", "--code-list", "src.pcv", "--img-list", "src.png"])
    out = capsys.readouterr().out
    rate, psnr, ssim = re.findall(r"Bitrate:([0-9.]+)bpp, PSNR:([0-9.]+)dB, SSIM:([0-9.]+)", out)[0]
    assert rate == "%.3f" % (len(payload) * 8 / float(h * w)) and np.isfinite(float(psnr)) and np.isfinite(float(ssim))
    with pytest.raises(C.ContainerError, match="records the rotation"):
        PC.main(["--test", "--rotate", "41,-60.5,15", "--code-list", "src.pcv", "--img-list", "src.png"])
    # a rotated file does not go to --yuv-out, whose path stops before the rotation
    with pytest.raises(C.ContainerError, match="--rotate"):
        PC.decoding_yuv(["src.pcv"], "out.yuv", dict(fmt="yuv420p", matrix="bt709", range="limited"), model_idx=3, mse=False)
    capsys.readouterr()
    # the refusals: no --container, angles out of range or malformed, with --yuv, with --dec
    enc = ["--enc", "--img-list", "src.png", "--code-list", "x.bin"] + common
    for extra in (["--rotate", "40,-60.5,15"], ["--rotate", "40,-60.5,15", "--container", "--raw"],
                  ["--rotate", "180,0,0", "--container"], ["--rotate", "0,91,0", "--container"],
                  ["--rotate", "40,-60.5", "--container"], ["--rotate", "a,b,c", "--container"],
                  ["--rotate", "40,-60.5,15", "--container", "--yuv", "a.yuv", "--size", "512x256", "--pix-fmt", "yuv420p"]):
        with pytest.raises(SystemExit):
            PC.main(enc + extra)
        assert "--rotate" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        PC.main(["--dec", "--rotate", "40,-60.5,15", "--code-list", "src.pcv", "--out-list", "y.png"])
    assert "--rotate" in capsys.readouterr().err
