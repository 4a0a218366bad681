"""Panoramas of any size (erp_size.py, container version 2, --native-size) without a GPU: the padding rule
against an independent numpy loop, the C and Python definitions of the coded size, the container format, and
the command line end to end on the oracle backend at 250x500."""
import ctypes
import re

import numpy as np
import pytest
import torch

from pseudocylindrical_convolution_amd import container as C
from pseudocylindrical_convolution_amd import erp_size

SHAPES = [(250, 500), (200, 333), (37, 50), (257, 17)]


def numpy_pad(img):
    """the rule of include/pconv_hip.h stated as a loop over coded pixels: (c, h, w) -> (c, H, W)"""
    c, h, w = img.shape
    H = 256 * ((h + 255) // 256)
    W = 16 * ((w + 15) // 16)
    top, p = (H - h) // 2, W - w
    m = (p + 1) // 2
    out = np.empty((c, H, W), dtype=img.dtype)
    for yc in range(H):
        y, flip = yc - top, False
        if y < 0:
            y, flip = -1 - y, True
        elif y >= h:
            y, flip = 2 * h - 1 - y, True
        y = min(max(y, 0), h - 1)
        for xc in range(W):
            x = xc if xc < w else (w - 1 if xc - w < m else 0)
            if flip:
                x = (x + w // 2) % w
            out[:, yc, xc] = img[:, y, x]
    return out


def test_coded_size_c_and_python_agree():
    from pseudocylindrical_convolution_amd import _native
    try:
        lib = _native.hip_lib()
    except _native.PconvError:
        lib = None
    H, W, top = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ph, pw, pt = ctypes.byref(H), ctypes.byref(W), ctypes.byref(top)
    for h in range(2, 1101):
        for w in range(2, 1101):
            got = erp_size.coded_size(h, w)
            if lib is not None:
                assert lib.pconv_erp_coded_size(h, w, ph, pw, pt) == 0
                want = (H.value, W.value, top.value)
            else:
                Hd = 256 * -(-h // 256)
                want = (Hd, 16 * -(-w // 16), (Hd - h) // 2)
            assert got == want, (h, w, got, want)
    if lib is not None:
        assert lib.pconv_erp_coded_size(1, 64, ph, pw, pt) < 0 and b"below 2x2" in lib.pconv_last_error()
    for bad in ((1, 64), (64, 1), (0, 0)):
        with pytest.raises(ValueError):
            erp_size.coded_size(*bad)
    # codable sizes are fixed points
    assert erp_size.coded_size(512, 1024) == (512, 1024, 0) and erp_size.codable(512, 1024)
    assert erp_size.coded_size(2880, 5760) == (3072, 5760, 96) and not erp_size.codable(2880, 5760)


@pytest.mark.parametrize("h,w", SHAPES)
def test_cpu_padding_is_the_numpy_rule(h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    u8 = torch.randint(0, 256, (2, 3, h, w), generator=g, dtype=torch.uint8)
    x = u8.float() / 255.
    want = np.stack([numpy_pad(f) for f in x.numpy()])
    got = erp_size.pad(x)
    assert got.shape == want.shape and np.array_equal(got.numpy(), want)
    # a gather: uint8 first then / 255 gives the same bits
    assert torch.equal(erp_size.pad_torch(u8).float() / 255., got)
    # the crop inverts it
    assert torch.equal(erp_size.crop(got, h, w), x)


def test_pad_is_the_identity_at_codable_sizes():
    x = torch.rand(1, 3, 256, 32)
    assert torch.equal(erp_size.pad(x), x)


def test_container_v2_round_trip_and_errors():
    blob = C.pack_any(b"\x01\x02\x03", height=2880, width=5760, model_idx=3, ssim=True, valid_dim=56)
    assert len(blob) == C.HEADER_BYTES_ANY + 3 == 23 and blob[:4] == b"PCVC" and blob[4] == 2
    head, payload = C.unpack(blob)
    assert payload == b"\x01\x02\x03"
    assert head == {"height": 2880, "width": 5760, "model_idx": 3, "ssim": True, "valid_dim": 56}
    assert C.unpack(C.pack_any(b"", height=37, width=50, model_idx=0, ssim=False, valid_dim=192))[0]["width"] == 50
    # a codable size: version 1, byte for byte what pack writes
    for h, w in ((256, 512), (2048, 4096), (512, 16)):
        args = dict(height=h, width=w, model_idx=8, ssim=False, valid_dim=192)
        assert C.pack_any(b"xyz", **args) == C.pack(b"xyz", **args)
    # truncated, over-long, unknown version, wrong magic, size out of range
    for bad in (blob[:10], blob[:18], blob[:-1], blob + b"\x00", blob[:4] + b"\x03" + blob[5:], b"XXXX" + blob[4:],
                blob[:8] + b"\x01\x00\x00\x00" + blob[12:]):
        with pytest.raises(C.ContainerError):
            C.unpack(bad)
    with pytest.raises(C.ContainerError):
        C.pack_any(b"", height=1, width=64, model_idx=0, ssim=True, valid_dim=56)
    with pytest.raises(C.ContainerError):
        C.pack(b"", height=250, width=512, model_idx=0, ssim=True, valid_dim=56)     # pack itself is unchanged


def test_sniff_and_header_bytes(tmp_path):
    boxed, raw, v1 = str(tmp_path / "a.pcv"), str(tmp_path / "a.bin"), str(tmp_path / "b.pcv")
    C.write_any(boxed, b"\x05" * 40, height=250, width=500, model_idx=3, ssim=True, valid_dim=56)
    C.write_any(v1, b"\x05" * 40, height=256, width=512, model_idx=3, ssim=True, valid_dim=56)
    with open(raw, "wb") as f:
        f.write(bytes(range(7, 90)))
    assert C.sniff(boxed) == {"height": 250, "width": 500, "model_idx": 3, "ssim": True, "valid_dim": 56}
    assert C.sniff(v1)["height"] == 256 and C.sniff(raw) is None
    assert (C.header_bytes(boxed), C.header_bytes(v1), C.header_bytes(raw)) == (20, 16, 0)
    head, payload = C.read(boxed)
    assert payload == b"\x05" * 40 and head["width"] == 500
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    assert PC.bitrate(boxed, 250, 500) == 40 * 8 / (250. * 500.)


def _write_png(path, img_hwc):
    from PIL import Image
    Image.fromarray(img_hwc).save(path)


def drive_native_size(tmp_path, monkeypatch, capsys, h, w, device):
    """--enc --native-size --container of an h x w PNG, then --dec and --test of the file"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, device)
    g = np.random.default_rng(5)
    yy, xx = np.linspace(0, 1, h)[:, None, None], np.linspace(0, 1, w)[None, :, None]
    img = (0.5 + 0.3 * np.sin(6.28318 * 2 * xx + g.random(3)) * np.cos(3.14159 * yy) + 0.05 * g.random((h, w, 3)))
    img = (img.clip(0, 1) * 255).astype(np.uint8)
    _write_png("src.png", img)
    common = ["--ssim", "--model-idx", "3"]
    PC.main(["--enc", "--native-size", "--container", "--img-list", "src.png", "--code-list", "src.pcv"] + common)
    out = capsys.readouterr().out
    head, payload = C.read("src.pcv")
    assert head == {"height": h, "width": w, "model_idx": 3, "ssim": True, "valid_dim": 56}
    assert C.header_bytes("src.pcv") == 20
    assert re.findall(r"bitrate: ([0-9.]+)bpp", out) == ["%.3f" % (len(payload) * 8 / float(h * w))]
    # the payload is today's path on the numpy-padded frame of the coded size (BGR as read_image returns it)
    bgr = PC.read_image("src.png")
    padded = numpy_pad(np.ascontiguousarray(bgr.transpose(2, 0, 1))).transpose(1, 2, 0)
    PC.write_image("padded.png", padded)
    PC.main(["--enc", "--container", "--img-list", "padded.png", "--code-list", "padded.pcv", "--height",
             str(padded.shape[0]), "--width", str(padded.shape[1])] + common)
    phead, ppayload = C.read("padded.pcv")
    assert (phead["height"], phead["width"]) == padded.shape[:2] and ppayload == payload
    # --dec: an image of the original size, the crop of the padded file's decode
    PC.main(["--dec", "--code-list", "src.pcv", "padded.pcv", "--out-list", "dec.png", "dec_padded.png"])
    dec, dec_padded = PC.read_image("dec.png"), PC.read_image("dec_padded.png")
    H, W, top = erp_size.coded_size(h, w)
    assert (H, W) != (h, w) and padded.shape == (H, W, 3)
    assert dec.shape == (h, w, 3) and dec_padded.shape == (H, W, 3)
    assert np.array_equal(dec, dec_padded[top:top + h, :w])
    capsys.readouterr()
    # --test at the original size, bpp over h * w
    rows = PC.decoding_and_test(["src.pcv"], ["src.png"], 3, False, 0)
    assert abs(rows[0][0] - len(payload) * 8 / float(h * w)) < 1e-12 and np.isfinite(rows[0][1])
    # --native-size needs the container
    with pytest.raises(AssertionError):
        PC.main(["--enc", "--native-size", "--img-list", "src.png", "--code-list", "x.bin"] + common)


def test_cli_native_size_on_the_oracle(oracle_backend, tmp_path, monkeypatch, capsys):
    drive_native_size(tmp_path, monkeypatch, capsys, 250, 500, "cpu")
