"""GPU: cubemap panoramas, CMP and EAC (csrc/cube.hip).  The two map kernels against the float64 numpy maps (equal:
tests/test_cube_cpu.py holds the shared cases away from every rounding boundary and face tie), the face continuation bit
for bit against its torch twin run on the CPU on the same table, the conversions bit for bit against their CPU twins on
the same maps, stale memory, the refusals, and CodecEngine's projection=.

Which edge of the kernels as built each shape reaches.  Map kernels: 256 columns per workgroup, one grid row.  Pad kernel:
4 rows x 64 columns of the padded plane (6 A x A, A = a + 6) per workgroup, a lane one pixel, grid.y = n * C.  Renderer
(viewport.hip, unchanged): 4 rows x 64 columns of the view, grid.y = n.
  a = 8      A = 14: one column tile of every kernel; 84 padded rows = 21 row groups, exact; more ring than interior
  a = 13     odd; A = 19, 114 padded rows = 28 row groups + 2 rows: ragged in both directions
  a = 67     A = 73 = 64 + 9: two pad tiles per row, the second of 9 columns; the view of from_erp is 67 wide, ragged too
  a = 300    a map row of 300 records: two map tiles, the second of 44; A = 306: five pad tiles per row, the last of 50
  16x32, 26x52, 134x268   ERP grids of one, one and two map tiles per row (ss = 2: 536 columns, three tiles)
  50x99      an odd width; with ss = 2, 198 columns
  24x50, 52x99, 132x270   stand in at ss = 1 for sizes whose own pixel centres are face ties (tests/cube_cases.py)
  (2, 3) and (1, 1)       grid.y = 6 and 1 planes (pad), 2 and 1 frames (renderer)
"""
import numpy as np
import pytest
import torch

import cube_cases as CC
import stale_memory as SM
from cube_cases import KINDS, case_id

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CC.FROM_ERP, ids=case_id)
def test_from_erp_map_kernel_is_the_float64_map(hip_backend, kind, case):
    from pseudocylindrical_convolution_amd import PCONV, cube
    a, ss, h, w = case
    got = PCONV.cube_from_erp_map(kind, a, ss, h, w)
    assert got.dtype == torch.int32 and tuple(got.shape) == (6 * a * ss, a * ss, 2) and got.is_cuda
    diff = got.cpu().numpy() != cube.from_erp_map_numpy(kind, a, ss, h, w)
    assert not diff.any(), "%d records differ, first at %s" % (diff.any(2).sum(), np.argwhere(diff.any(2))[:1])
    assert torch.equal(cube.from_erp_map(kind, a, ss, h, w, "cuda"), got)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CC.TO_ERP, ids=case_id)
def test_to_erp_map_kernel_is_the_float64_map(hip_backend, kind, case):
    from pseudocylindrical_convolution_amd import PCONV, cube
    a, h, w, ss = case
    got = PCONV.cube_to_erp_map(kind, a, h, w, ss)
    assert got.dtype == torch.int32 and tuple(got.shape) == (h * ss, w * ss, 2) and got.is_cuda
    diff = got.cpu().numpy() != cube.to_erp_map_numpy(kind, a, h, w, ss)
    assert not diff.any(), "%d records differ, first at %s" % (diff.any(2).sum(), np.argwhere(diff.any(2))[:1])
    assert torch.equal(cube.to_erp_map(kind, a, h, w, ss, "cuda"), got)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 3, 13), (2, 3, 67), (1, 1, 8), (1, 1, 300)], ids=case_id)
def test_pad_kernel_is_the_twin(hip_backend, kind, shape):
    """inside a larger buffer that starts as NaN between sentinels: every element is written, none outside"""
    from pseudocylindrical_convolution_amd import PCONV, cube
    n, c, a = shape
    A = a + 6
    y = CC.frames(n, c, 6 * a, a, seed=5)
    table = torch.from_numpy(np.array(cube.pad_table(kind, a)))
    want = cube.pad_torch(y, table)
    guard, numel = 64, n * c * 6 * A * A
    flat = torch.full((numel + 2 * guard,), 77.0, device="cuda")
    out = flat[guard:guard + numel].view(n, c, 6 * A, A)
    out.fill_(float("nan"))
    got = PCONV.cube_pad_f32(y.cuda(), table.cuda(), out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.cpu(), want), "max abs diff %g" % (got.cpu() - want).abs().max().item()
    host = flat.cpu()
    assert (host[:guard] == 77.0).all().item() and (host[guard + numel:] == 77.0).all().item()
    assert torch.equal(cube.pad(y.cuda(), kind).cpu(), want)                     # the public entry: its own cached table
    const = torch.full((1, 1, 6 * a, a), 0.3, device="cuda")
    assert torch.equal(cube.pad(const, kind), torch.full((1, 1, 6 * A, A), 0.3, device="cuda"))


_twins = {}


def _twin(key, make):
    if key not in _twins:
        _twins[key] = make()
    return _twins[key]


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(2, 3, 13, 2, 50, 99), (2, 3, 67, 1, 134, 268), (1, 1, 8, 2, 16, 32), (1, 1, 300, 1, 134, 268)],
                         ids=case_id)
def test_from_erp_is_the_twin(hip_backend, kind, case, clamp):
    from pseudocylindrical_convolution_amd import cube
    n, c, a, ss, h, w = case
    x = CC.frames(n, c, h, w)                               # some of it outside [0, 1]
    for layout in ("faces", "3x2"):
        want = _twin(("from", kind, case, clamp, layout), lambda: cube.from_erp(x, a, kind, ss=ss, clamp=clamp, layout=layout))
        got = cube.from_erp(x.cuda(), a, kind, ss=ss, clamp=clamp, layout=layout).cpu()
        assert got.shape == want.shape and torch.equal(got, want), "max abs diff %g" % (got - want).abs().max().item()
    if clamp:
        assert got.min().item() >= 0.0 and got.max().item() <= 1.0


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(2, 3, 13, 52, 99, 1), (2, 3, 67, 50, 99, 2), (1, 1, 8, 16, 32, 2), (1, 1, 300, 132, 270, 1),
                                  (2, 3, 67, 134, 268, 2)], ids=case_id)
def test_to_erp_is_the_twin(hip_backend, kind, case, clamp):
    from pseudocylindrical_convolution_amd import cube
    n, c, a, h, w, ss = case
    y = CC.frames(n, c, 6 * a, a, seed=7)
    for layout in ("faces", "3x2"):
        packed = cube.pack(y, layout)
        want = _twin(("to", kind, case, clamp, layout), lambda: cube.to_erp(packed, (h, w), kind, ss=ss, clamp=clamp, layout=layout))
        got = cube.to_erp(packed.cuda(), (h, w), kind, ss=ss, clamp=clamp, layout=layout).cpu()
        assert got.shape == want.shape == (n, c, h, w)
        assert torch.equal(got, want), "max abs diff %g" % (got - want).abs().max().item()
    if clamp:
        assert got.min().item() >= 0.0 and got.max().item() <= 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_results_do_not_depend_on_what_fresh_memory_held(hip_backend, monkeypatch, kind):
    """every torch.empty the conversions make -- maps, the padded stack, the pictures -- starts as NaN / a pattern"""
    from pseudocylindrical_convolution_amd import cube
    a, h, w = 13, 50, 99
    x, y = CC.frames(2, 3, h, w).cuda(), CC.frames(2, 3, 6 * a, a, seed=7).cuda()
    results = []
    for name, regime in SM.regimes(monkeypatch):
        for cache in (cube._from_erp_map, cube._to_erp_map):
            cache.cache_clear()                   # the maps are made again inside the regime
        with regime() as made:
            results.append((name, cube.from_erp(x, a, kind, ss=2, layout="faces"), cube.pad(y, kind),
                            cube.to_erp(y, (h, w), kind, ss=2, layout="faces"),
                            cube.from_erp_map(kind, a, 2, h, w, "cuda"), cube.to_erp_map(kind, a, h, w, 2, "cuda")))
        assert name == "plain" or made, "the regime saw no allocation"
    for name, *tensors in results[1:]:
        for got, want in zip(tensors, results[0][1:]):
            assert SM.same_bits(got, want), name
    for cache in (cube._from_erp_map, cube._to_erp_map):
        cache.cache_clear()


def test_refusals_come_from_the_host(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, cube, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    lib = _native.hip_lib()
    a, A = 8, 14
    y = torch.zeros(1, 1, 6 * a, a).cuda()
    table = cube.pad_table_on("cmp", a, "cuda")
    out = torch.empty(1, 1, 6 * A, A).cuda()
    q = torch.empty(6 * a, a, 2, dtype=torch.int32).cuda()
    e = torch.empty(16, 32, 2, dtype=torch.int32).cuda()
    bad = lambda rc, word: rc == -1 and word in lib.pconv_last_error()
    # the pad kernel
    good = [y.data_ptr(), out.data_ptr(), table.data_ptr()]
    for k in range(3):
        args = list(good)
        args[k] = None
        assert bad(lib.pconv_cube_pad_f32(*args, 1, 1, a, None), b"null pointer")
        args[k] = good[k] + 2
        assert bad(lib.pconv_cube_pad_f32(*args, 1, 1, a, None), b"aligned")
    assert bad(lib.pconv_cube_pad_f32(*good, 1, 1, 1, None), b"face size")
    assert bad(lib.pconv_cube_pad_f32(*good, 1, 1, 9454, None), b"face size")
    assert bad(lib.pconv_cube_pad_f32(*good, 70000, 1, a, None), b"planes")
    assert bad(lib.pconv_cube_pad_f32(*good, 0, 1, a, None), b"planes")
    assert bad(lib.pconv_cube_pad_f32(good[0], good[0], good[2], 1, 1, a, None), b"distinct")
    # the two map kernels
    assert bad(lib.pconv_cube_from_erp_map(None, 1, a, 1, 16, 32, None), b"null pointer")
    assert bad(lib.pconv_cube_to_erp_map(None, 1, a, 16, 32, 1, None), b"null pointer")
    assert bad(lib.pconv_cube_from_erp_map(q.data_ptr() + 4, 1, a, 1, 16, 32, None), b"aligned")
    assert bad(lib.pconv_cube_to_erp_map(e.data_ptr() + 4, 1, a, 16, 32, 1, None), b"aligned")
    for kind in (0, 3):
        assert bad(lib.pconv_cube_from_erp_map(q.data_ptr(), kind, a, 1, 16, 32, None), b"kind")
        assert bad(lib.pconv_cube_to_erp_map(e.data_ptr(), kind, a, 16, 32, 1, None), b"kind")
    for face in (1, 9454):
        assert bad(lib.pconv_cube_from_erp_map(q.data_ptr(), 1, face, 1, 16, 32, None), b"face size")
        assert bad(lib.pconv_cube_to_erp_map(e.data_ptr(), 1, face, 16, 32, 1, None), b"face size")
    for ss in (0, 5):
        assert bad(lib.pconv_cube_from_erp_map(q.data_ptr(), 1, a, ss, 16, 32, None), b"supersampling")
        assert bad(lib.pconv_cube_to_erp_map(e.data_ptr(), 1, a, 16, 32, ss, None), b"supersampling")
    for h, w in ((1, 32), (16, 1), (16, (1 << 20) + 1)):
        assert bad(lib.pconv_cube_from_erp_map(q.data_ptr(), 1, a, 1, h, w, None), b"outside")
        assert bad(lib.pconv_cube_to_erp_map(e.data_ptr(), 1, a, h, w, 1, None), b"outside")
    assert bad(lib.pconv_cube_from_erp_map(q.data_ptr(), 1, a, 1, 1 << 15, 1 << 15, None), b"2^31 bytes")
    assert bad(lib.pconv_cube_to_erp_map(e.data_ptr(), 1, a, 1 << 14, 1 << 14, 1, None), b"2^31 bytes")
    assert bad(lib.pconv_cube_from_erp_map(q.data_ptr(), 1, 9000, 1, 16, 32, None), b"2^31 bytes")
    # the wrappers
    with pytest.raises(PconvError, match="GPU tensor"):
        PCONV.cube_pad_f32(y.cpu(), table.cpu())
    with pytest.raises(PconvError, match="face stack"):
        PCONV.cube_pad_f32(torch.zeros(1, 1, 40, a).cuda(), table)
    for bad_table in (table.long(), table[:5], table.cpu(), table.float()):
        with pytest.raises(PconvError, match="table"):
            PCONV.cube_pad_f32(y, bad_table)
    with pytest.raises(PconvError, match="out must"):
        PCONV.cube_pad_f32(y, table, torch.empty(1, 1, 6 * A, A + 1).cuda())
    with pytest.raises(PconvError, match="kind"):
        PCONV.cube_from_erp_map("xyz", a, 1, 16, 32)
    with pytest.raises(PconvError, match="GPU device"):
        PCONV.cube_to_erp_map("cmp", a, 16, 32, 1, device="cpu")
    with pytest.raises(PconvError, match="face size"):
        PCONV.cube_from_erp_map("cmp", 1, 1, 16, 32)
    with pytest.raises(PconvError, match="no backward"):
        cube.to_erp(y.clone().requires_grad_(True), None, "cmp", layout="faces")
    torch.cuda.synchronize()
    # nothing was launched: the destinations still hold what they held
    out.fill_(5.0)
    assert lib.pconv_cube_pad_f32(good[0], good[1], good[2], 1, 1, 9454, None) == -1
    torch.cuda.synchronize()
    assert (out == 5.0).all().item()


def test_from_erp_backward_is_the_twin(hip_backend):
    """the gradient through from_erp on the device equals the CPU twin's, bit for bit (the ordered backward)"""
    from pseudocylindrical_convolution_amd import cube
    a, ss, h, w = 13, 2, 50, 99
    g = CC.frames(2, 3, 2 * a, 3 * a, seed=4)
    grads = []
    for device in ("cpu", "cuda"):
        x = CC.frames(2, 3, h, w).to(device).requires_grad_(True)
        # the device's forward on the numpy map, so that both sides walk the same records
        y = cube.from_erp(x, a, "eac", ss=ss, layout="3x2")
        grads.append(torch.autograd.grad(y, x, g.to(device))[0].cpu())
    assert torch.equal(grads[0], grads[1])


def _codec():
    from test_gpu_engine import _codec as codec
    return codec()


def test_cli_rd_and_test_with_a_projection(hip_backend, tmp_path, monkeypatch, capsys):
    """--rd --projection scores without a file what --enc --projection --container and --test report of one: the same
    reconstruction, so the same PSNR, SSIM and CUBE-PSNR; bpp over the cube picture's pixels"""
    import re
    from pseudocylindrical_convolution_amd import container, cube, pseudo_codec as PC
    from test_cli import _models
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cuda")
    a = 64
    y = cube.from_erp(CC.smooth(2 * a, 4 * a), a, cube.spec("cmp", "6x1"), clamp=True)
    PC.write_image("cube.png", PC.tensor2img(y))
    common = ["--ssim", "--model-idx", "3"]
    PC.main(["--rd", "--projection", "cmp", "--cube-layout", "6x1", "--img-list", "cube.png"] + common)
    rd = capsys.readouterr().out
    PC.main(["--enc", "--projection", "cmp", "--cube-layout", "6x1", "--container", "--img-list", "cube.png", "--code-list",
             "cube.pcv"] + common)
    head, payload = container.read("cube.pcv")
    assert head["projection"] == ("cmp", "6x1", a) and (head["height"], head["width"]) == (2 * a, 4 * a)
    capsys.readouterr()
    PC.main(["--test", "--code-list", "cube.pcv", "--img-list", "cube.png"])
    test = capsys.readouterr().out
    figures = lambda text: re.findall(r"PSNR:([0-9.]+)dB, SSIM:([0-9.]+)", text)
    assert len(figures(rd)) == 2 and figures(rd) == figures(test)                 # the image's line and the average's
    cubes = lambda text: re.findall(r"CUBE-PSNR:([0-9.]+)dB", text)
    assert len(cubes(rd)) == 2 and cubes(rd) == cubes(test) and float(cubes(rd)[0]) > 0
    real = len(payload) * 8 / float(6 * a * a)
    estimate = float(re.findall(r"Bitrate:([0-9.]+)bpp", rd)[0])
    assert abs(estimate - real) <= 0.002 + 0.01 * real                            # rate.py: within a few bits of the stream
    assert re.findall(r"Bitrate:([0-9.]+)bpp", test)[0] == "%.3f" % real


def test_codec_engine_codes_cube_pictures(hip_backend):
    from pseudocylindrical_convolution_amd import cube
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec()
    eng = CodecEngine(56, 0, enc, dec)
    a = 64
    sp = cube.spec("eac", "3x2")
    y = cube.from_erp(CC.smooth(128, 256).expand(2, 3, 128, 256).contiguous(), a, sp, clamp=True)
    y[1] = y[1].flip(1)
    erp_twin = cube.to_erp(y, None, sp, clamp=True)                    # the CPU twin's ERP frame
    assert torch.equal(cube.to_erp(y.cuda(), None, sp, clamp=True).cpu(), erp_twin)
    streams = eng.encode(y.cuda(), projection=sp)
    assert streams == eng.encode(erp_twin.cuda())
    rec_erp = eng.decode(streams, 128, 256)
    rec = eng.decode(streams, 128, 256, projection=sp)
    assert rec.shape == y.shape and torch.equal(rec, cube.from_erp(rec_erp, a, sp, clamp=True))
    bits = eng.rate(y.cuda(), projection=sp)
    assert torch.equal(bits, eng.rate(erp_twin.cuda()))
    ebits, erec = eng.evaluate(y.cuda(), projection=sp)
    assert torch.equal(ebits, bits) and torch.equal(erec, rec)
    with pytest.raises(Exception, match="2a x 4a"):
        eng.decode(streams, 128, 250, projection=sp)
