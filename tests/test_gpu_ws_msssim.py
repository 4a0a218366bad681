"""GPU: WS-MS-SSIM forward (csrc/sphere_metrics.hip: ms_forward_kernel once per scale, ms_close_kernel<5>).  The
pyramid the kernels write bit for bit against `pool` in float32, the WS-MSE column bit for bit against ws_metrics, the
last scale bit for bit against ws_metrics of the pooled frames, every scale value and the product against the float64
statement within bounds taken from the float32 map, the uint8 form, batching and repeat determinism, the clamp, and
refused arguments."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the smallest shapes at which the pyramid, the 32 x 64 tiling, the halos and the dropped odd rows can go wrong
SHAPES = [
    (1, 1, 16, 16),     # one pixel at scale 4
    (2, 3, 17, 19),     # an odd side at every scale: 17 -> 8 -> 4 -> 2 -> 1
    (1, 2, 33, 65),     # one row and one column past a tile edge
    (1, 1, 64, 128),    # whole tiles
    (3, 1, 37, 70),     # several frames with a remainder
    (1, 3, 75, 150),    # 75 -> 37 -> 18 -> 9 -> 4
    (1, 1, 130, 258),   # a remainder past a tile edge at scale 1 as well
]
HALF_FLAT = "half-flat"   # (1, 1, 64, 128) whose upper half is the constant 0.5 in both pictures: B2 ~ C2
CASES = SHAPES + [HALF_FLAT]
WEIGHTINGS = ["ws", "uniform"]


def inputs(case):
    """x = rand, y = x + 0.1·randn, neither clamped (float32, CPU), seeded from the shape"""
    shape = (1, 1, 64, 128) if case == HALF_FLAT else case
    g = torch.Generator().manual_seed(sum(shape) + (100 if case == HALF_FLAT else 0))
    x = torch.rand(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    if case == HALF_FLAT:
        x[:, :, :32] = 0.5
        y[:, :, :32] = 0.5
    return x, y


@pytest.mark.parametrize("case", CASES, ids=str)
def test_pyramid_is_pool_bit_for_bit(hip_backend, case):
    from pseudocylindrical_convolution_amd import PCONV, sphere_metrics as S
    x, y = (t.to(DEV) for t in inputs(case))
    n, c, h, w = x.shape
    values, workspace = PCONV.ws_msssim_device(x, y)
    assert values.dtype == torch.float64 and values.shape == (n, 7) and values.device == x.device
    assert workspace.dtype == torch.uint8 and workspace.device == x.device
    levels = PCONV.ws_msssim_levels(workspace, n, c, h, w)
    assert len(levels) == 4
    px, py = x, y
    for s, (lx, ly) in enumerate(levels, 1):
        px, py = S.pool(px), S.pool(py)
        assert lx.shape == ly.shape == (n, c, h >> s, w >> s) and lx.dtype == torch.float32
        assert torch.equal(lx, px) and torch.equal(ly, py), (case, s)


# (528, 1040) is 33 x 65 at scale 4: one row and one column past a tile edge, several tiles' partials at the last scale
@pytest.mark.parametrize("shape", [(1, 1, 16, 16), (2, 3, 17, 19), (1, 1, 130, 258), (1, 1, 528, 1040)], ids=str)
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_last_scale_is_ws_ssim_of_the_pooled_frames(hip_backend, shape, weighting):
    """v_4 has the bits of WS-SSIM of (x_4, y_4): the single-scale metric is the chain of one scale, which runs the last
    scale's map, sums and normalisation"""
    from pseudocylindrical_convolution_amd import PCONV
    x, y = (t.to(DEV) for t in inputs(shape))
    got, workspace = PCONV.ws_msssim(x, y, weighting)
    x4, y4 = (t.contiguous() for t in PCONV.ws_msssim_levels(workspace, *shape)[-1])
    assert torch.equal(got[:, 4], PCONV.ws_metrics(x4, y4, weighting)[:, 1]), (shape, weighting)


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_values_are_the_float64_twin(hip_backend, case, weighting):
    """each v_s within 1e-5 of the float64 statement on the device (the project's bound for the float32 SSIM map
    against its float64 path); WS-MS-SSIM within 1.2e-5: Σβ = 1.0001 and v_s >= 0.9 on these inputs, so 1e-5 per scale
    propagates to at most 1.0001 / 0.9 · 1e-5"""
    from pseudocylindrical_convolution_amd import PCONV, sphere_metrics as S
    x, y = (t.to(DEV) for t in inputs(case))
    got, _ = PCONV.ws_msssim(x, y, weighting)
    assert got.device.type == "cpu" and got.dtype == torch.float64
    assert torch.equal(got[:, 5], PCONV.ws_metrics(x, y, weighting)[:, 0])       # WS-MSE: the bits of ws_metrics
    twin = S.ms_scales_torch(x, y, weighting, torch.float64).cpu()
    assert bool((twin >= 0.9).all()), twin
    dv = (got[:, :5] - twin).abs().max().item()
    dms = (got[:, 6] - S.ms_product(twin)).abs().max().item()
    print("ws_msssim %s %s: dv %.3g dms %.3g" % (case, weighting, dv, dms))
    assert dv <= 1e-5 and dms <= 1.2e-5, (case, weighting, dv, dms)
    assert torch.equal(S.ms_metrics(x, y, weighting), got[:, 5:])
    assert torch.equal(S.ws_ms_ssim(x, y, weighting), got[:, 6])


def test_mid_size_against_the_cpu_path(hip_backend):
    from pseudocylindrical_convolution_amd import sphere_metrics as S
    shape = (2, 3, 512, 1024)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    for weighting in WEIGHTINGS:
        got = S.ms_metrics(x.to(DEV), y.to(DEV), weighting)
        twin = S.ms_scales_torch(x.to(DEV), y.to(DEV), weighting, torch.float64).cpu()
        assert bool((twin >= 0.9).all()), twin
        want = S.ms_metrics(x, y, weighting)                                     # the CPU path itself
        assert (got[:, 1] - S.ms_product(twin)).abs().max().item() <= 1.2e-5
        assert (got[:, 1] - want[:, 1]).abs().max().item() <= 1.2e-5
        assert (S.psnr(got[:, 0]) - S.psnr(want[:, 0])).abs().max().item() <= 1e-4


@pytest.mark.parametrize("n,h,w", [(1, 64, 128), (2, 37, 51)])
def test_uint8_form_is_bitwise_the_float_form(hip_backend, n, h, w):
    from pseudocylindrical_convolution_amd import PCONV
    g = torch.Generator().manual_seed(h * w)
    u = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    v = (u.int() + torch.randint(-25, 26, u.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    if w % 4 == 0:
        fu, fv = PCONV.frames_u8_to_f32(u.to(DEV)), PCONV.frames_u8_to_f32(v.to(DEV))
    else:   # img2tensor's arithmetic on the host (frames_u8_to_f32 takes widths % 4 == 0)
        fu, fv = ((t.permute(0, 3, 1, 2).float() / 255.).contiguous().to(DEV) for t in (u, v))
    for weighting in WEIGHTINGS:
        a, wa = PCONV.ws_msssim_device(u.to(DEV), v.to(DEV), weighting)
        b, wb = PCONV.ws_msssim_device(fu, fv, weighting)
        assert torch.equal(a, b)
        for la, lb in zip(PCONV.ws_msssim_levels(wa, n, 3, h, w), PCONV.ws_msssim_levels(wb, n, 3, h, w)):
            assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])


def test_same_bits_again_alone_and_in_a_batch(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV
    x, y = (t.to(DEV) for t in inputs((3, 1, 37, 70)))
    batch, _ = PCONV.ws_msssim_device(x, y)
    assert torch.equal(batch, PCONV.ws_msssim_device(x, y)[0])
    for k in range(3):
        alone, _ = PCONV.ws_msssim_device(x[k:k + 1].contiguous(), y[k:k + 1].contiguous())
        assert torch.equal(alone, batch[k:k + 1])
    assert torch.equal(PCONV.ws_msssim_device(y, x)[0], batch)                   # symmetric, bit for bit


def test_identical_and_inverted_frames(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV
    x, _ = (t.to(DEV) for t in inputs((2, 3, 17, 19)))
    same, _ = PCONV.ws_msssim(x, x.clone())
    assert torch.equal(same[:, 5], torch.zeros(2, dtype=torch.float64))
    assert (same[:, :5] - 1).abs().max().item() <= 1e-12 and (same[:, 6] - 1).abs().max().item() <= 1e-12
    inverted, _ = PCONV.ws_msssim(x, (1 - x).contiguous())
    assert bool((inverted[:, :5] <= 0).any(dim=1).all())
    assert torch.equal(inverted[:, 6], torch.zeros(2, dtype=torch.float64))      # a clamped frame gives exactly 0


def test_refused_inputs(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV
    from pseudocylindrical_convolution_amd._native import PconvError
    x, y = inputs((1, 3, 16, 32))
    xc, yc = x.to(DEV), y.to(DEV)
    u = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV)
    bad = [
        (x, y),                                                   # CPU tensors
        (xc, y),                                                  # device mix
        (xc, yc.double()),                                        # dtype
        (xc, u),                                                  # dtype mix
        (xc, yc[:, :, :, :31].contiguous()),                      # shape
        (xc.transpose(2, 3), yc.transpose(2, 3)),                 # not contiguous
        (xc[0], yc[0]),                                           # not a batch
        (u[..., :2].contiguous(), u[..., :2].contiguous()),       # uint8 that is not (n, h, w, 3)
        (xc[:0], yc[:0]),                                         # no frame
    ]
    for a, b in bad:
        with pytest.raises(PconvError):
            PCONV.ws_msssim(a, b)
    for a, b in [(xc[:, :, :15].contiguous(), yc[:, :, :15].contiguous()),
                 (xc[..., :15].contiguous(), yc[..., :15].contiguous()), (u[:, :15].contiguous(), u[:, :15].contiguous())]:
        with pytest.raises(PconvError, match="h and w must be at least 16"):
            PCONV.ws_msssim(a, b)
    with pytest.raises(PconvError):
        PCONV.ws_msssim(xc, yc, "s-psnr")
    assert PCONV.ws_msssim(xc, yc)[0].shape == (1, 7) and PCONV.ws_msssim(u, u)[0].shape == (1, 7)


def test_refusals_of_the_native_entries(hip_backend):
    """each returns -1 with a message, before any launch (the pointers are never dereferenced)"""
    from pseudocylindrical_convolution_amd import _native
    lib = _native.hip_lib()
    dummy = 4096
    bad = [
        (None, dummy, 1, 1, 16, 16, 0, dummy, dummy, b"null pointer"),
        (dummy, None, 1, 1, 16, 16, 0, dummy, dummy, b"null pointer"),
        (dummy, dummy, 1, 1, 16, 16, 0, None, dummy, b"null pointer"),
        (dummy, dummy, 1, 1, 16, 16, 0, dummy, None, b"null pointer"),
        (dummy, dummy, 1, 1, 16, 16, 0, dummy + 4, dummy, b"8-byte aligned"),
        (dummy, dummy, 1, 1, 16, 16, 2, dummy, dummy, b"unknown weighting"),
        (dummy, dummy, 0, 1, 16, 16, 0, dummy, dummy, b"frame count"),
        (dummy, dummy, 1, 4097, 16, 16, 0, dummy, dummy, b"channel count"),
        (dummy, dummy, 1, 1, 0, 16, 0, dummy, dummy, b"frame size"),
        (dummy, dummy, 1, 1, 15, 16, 0, dummy, dummy, b"h and w must be at least 16"),
        (dummy, dummy, 1, 1, 16, 15, 0, dummy, dummy, b"h and w must be at least 16"),
        (dummy, dummy, 1, 1, 16384, 32768, 0, dummy, dummy, b"2^31 bytes"),
    ]
    for case in bad:
        rc = lib.pconv_ws_msssim_f32(*case[:9], None)
        assert rc == -1 and b"ws_msssim_f32" in lib.pconv_last_error() and case[9] in lib.pconv_last_error(), case
    rc = lib.pconv_ws_msssim_u8(dummy, dummy, 1, 3, 15, 16, 0, dummy, dummy, None)
    assert rc == -1 and b"ws_msssim_u8" in lib.pconv_last_error() and b"at least 16" in lib.pconv_last_error()
    rc = lib.pconv_ws_msssim_u8(dummy, dummy, 1, 1, 16, 16, 0, dummy, dummy, None)
    assert rc == -1 and b"3 channels" in lib.pconv_last_error()
    for fn in (lib.pconv_ws_msssim_workspace_bytes, lib.pconv_ws_msssim_backward_workspace_bytes):
        assert fn(1, 1, 15, 16) < 0 and b"h and w must be at least 16" in lib.pconv_last_error()
        assert fn(0, 1, 16, 16) < 0 and fn(1, 0, 16, 16) < 0
    # the pyramid is one third of the two inputs, the coarse gradients one third of one input
    n, c, h, w = 2, 3, 512, 1024
    pyramid = sum(2 * n * c * (h >> s) * (w >> s) * 4 for s in range(1, 5))
    tiles = sum(-(-(h >> s) // 32) * -(-(w >> s) // 64) for s in range(5))
    assert lib.pconv_ws_msssim_workspace_bytes(n, c, h, w) == pyramid + n * tiles * 16
    assert lib.pconv_ws_msssim_backward_workspace_bytes(n, c, h, w) == pyramid // 2
    assert pyramid < 2 * n * c * h * w * 4 / 3


def test_cli_ms_ssim_on_the_gpu(hip_backend, tmp_path, monkeypatch, capsys):
    """--test --ws --ms-ssim and --rd --ws --ms-ssim: one more line per image and for the average, one more column,
    within 1.2e-5 of the float64 path on the same pictures; without the flag the lines and rows are as before"""
    import re
    from pseudocylindrical_convolution_amd import pseudo_codec as PC, sphere_metrics as S
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, DEV)
    H, W = 256, 512
    common = ["--ssim", "--model-idx", "3", "--height", str(H), "--width", str(W)]
    _write_png("img.png", H, W, 0)
    PC.main(["--enc", "--img-list", "img.png", "--code-list", "code.bin"] + common)
    PC.main(["--dec", "--code-list", "code.bin", "--out-list", "dec.png"] + common)
    capsys.readouterr()
    for mode in (["--test", "--code-list", "code.bin"], ["--rd"]):
        PC.main(mode + ["--ws", "--img-list", "img.png"] + common)
        plain = capsys.readouterr().out
        PC.main(mode + ["--ws", "--ms-ssim", "--img-list", "img.png"] + common)
        out = capsys.readouterr().out
        assert "WS-MS-SSIM" not in plain
        assert [f for f in re.findall(r"^( ?)WS-MS-SSIM:[0-9.]+$", out, flags=re.M)] == [" ", ""]
        assert [l for l in out.splitlines() if "WS-MS-SSIM" not in l] == plain.splitlines()
    src, dec = PC.read_image("img.png"), PC.read_image("dec.png")
    want = S.ws_ms_ssim(torch.from_numpy(src)[None], torch.from_numpy(dec)[None])[0].item()      # the float64 path
    before = PC.decoding_and_test(["code.bin"], ["img.png"], 3, False, 0, H, W, ws=True)
    for rows in (PC.decoding_and_test(["code.bin"], ["img.png"], 3, False, 0, H, W, ws=True, ms_ssim=True),
                 PC.rate_distortion(["img.png"], 3, False, 0, H, W, ws=True, ms_ssim=True)):
        assert len(rows) == 1 and len(rows[0]) == 6 and tuple(rows[0][1:5]) == tuple(before[0][1:])
        assert abs(rows[0][5] - want) <= 1.2e-5 and 0 < rows[0][5] < 1
    with pytest.raises(AssertionError, match="--ms-ssim needs --ws"):
        PC.main(["--rd", "--ms-ssim", "--img-list", "img.png"] + common)
