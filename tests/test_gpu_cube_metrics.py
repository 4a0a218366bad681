"""GPU: scoring cube pictures on the sphere (csrc/weighted_metrics.hip, cube_points_records_kernel of csrc/cube.hip).  Every
kernel against its CPU twin bit for bit -- tests/test_cube_metrics_cpu.py holds the twins to independent statements and
the shared point sets away from every rounding boundary and face tie -- then batches, offset views, stale memory, the
composite training gradient and the wrappers' operand contract.

Which edge of the kernels as built each plane reaches.  weighted_mse_kernel: one workgroup of 256 lanes per chunk of 1024
pixels and plane, a lane the pixels l, l + 256, l + 512, l + 768; weighted_sum_kernel: one workgroup per plane, lane l the
partials l, l + 256, ...; weighted_mse_backward_kernel: the same grid, 16-byte accesses when H*W is a multiple of 4 and
every pointer 16-byte aligned, else 4-byte ones.
  1x1       one pixel: 255 lanes add nothing            1x255     lane 255 adds nothing
  3x341     1023 pixels: one short of a chunk           32x32     exactly one chunk; the wide backward
  5x205     1025: a second chunk of one pixel           37x71     2627, odd: three chunks, the last ragged; narrow backward
  513x512   256.5 chunks -> 257 partials: the second stage's lane 0 adds two; the wide backward on many workgroups
  12x2, 18x3, 78x13   the face stacks of a = 2, 3, 13
  (1, 1) and (2, 3)   grid.y = 1 and 6 planes
"""
import numpy as np
import pytest
import torch

import cube_metrics_cases as MC
import stale_memory as SM
from cube_metrics_cases import KINDS, case_id

pytestmark = pytest.mark.gpu

_twins = {}


def _twin(key, make):
    """a CPU reference, computed once and shared"""
    if key not in _twins:
        _twins[key] = make()
    return _twins[key]


def _case(batch, plane):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    (n, c), (h, w) = batch, plane
    x, y = MC.frames(n, c, h, w, 1), MC.frames(n, c, h, w, 2)
    wt = _twin(("plane", plane), lambda: WM.WeightPlane(MC.weights(h, w)))
    return x, y, wt


def _gradients(x, y, wt, coef):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    x, y = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    terms = WM.loss_terms(x, y, wt)
    gx, gy = torch.autograd.grad((terms * coef.to(terms.device)).sum(), (x, y))
    return terms.detach().cpu(), gx.cpu(), gy.cpu()


def _coef(n):
    return torch.tensor([0.75, -1.5, 3.0][:n], dtype=torch.float64)


@pytest.mark.parametrize("batch", MC.BATCHES, ids=case_id)
@pytest.mark.parametrize("plane", MC.PLANES, ids=case_id)
def test_mse_and_its_gradient_are_the_twins(hip_backend, plane, batch):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    x, y, wt = _case(batch, plane)
    want = _twin(("mse", batch, plane), lambda: WM.mse(x, y, wt))
    got = WM.mse(x.cuda(), y.cuda(), wt)
    assert got.dtype == torch.float64 and got.device.type == "cpu" and SM.same_bits(got, want), (got, want)
    on_device = WM.mse_device(x.cuda(), y.cuda(), wt)
    assert on_device.is_cuda and SM.same_bits(on_device.cpu(), want)
    coef = _coef(batch[0])
    wt_terms, wgx, wgy = _twin(("grad", batch, plane), lambda: _gradients(x, y, wt, coef))
    terms, gx, gy = _gradients(x.cuda(), y.cuda(), wt, coef)
    assert SM.same_bits(terms, wt_terms)
    assert SM.same_bits(gy, wgy) and SM.same_bits(gx, wgx), "max abs diff %g" % (gy - wgy).abs().max().item()
    assert torch.equal(gx, -gy)      # (x - y and y - x are negations of each other in fp32)


@pytest.mark.parametrize("plane", MC.U8_PLANES, ids=case_id)
def test_u8_frames_give_the_bits_of_their_float_form(hip_backend, plane):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    h, w = plane
    x, y = MC.frames_u8(2, h, w, 1), MC.frames_u8(2, h, w, 2)
    wt = WM.WeightPlane(MC.weights(h, w))
    want = WM.mse(x, y, wt)                                              # the twin: float(u8) / 255 in float32
    got = WM.mse(x.cuda(), y.cuda(), wt)
    assert SM.same_bits(got, want)
    as_float = lambda t: (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    assert SM.same_bits(WM.mse(as_float(x).cuda(), as_float(y).cuda(), wt), want)


@pytest.mark.parametrize("plane", [(5, 205), (32, 32), (513, 512)], ids=case_id)
def test_a_frame_alone_and_inside_a_batch(hip_backend, plane):
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    h, w = plane
    x, y, wt = _case((3, 2), plane)
    x, y = x.cuda(), y.cuda()
    whole = WM.mse(x, y, wt)
    coef = _coef(3)
    _, gx, gy = _gradients(x, y, wt, coef)
    for f in range(3):
        assert SM.same_bits(WM.mse(x[f:f + 1], y[f:f + 1], wt), whole[f:f + 1])
        _, gx1, gy1 = _gradients(x[f:f + 1], y[f:f + 1], wt, coef[f:f + 1])
        assert SM.same_bits(gx1, gx[f:f + 1]) and SM.same_bits(gy1, gy[f:f + 1])


def _at_offset(t, elements):
    """a contiguous view of the same values `elements` elements into a larger buffer"""
    buf = torch.full((t.numel() + 8,), 7.0, dtype=t.dtype, device=t.device)
    view = buf[elements:elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elements * t.element_size()
    return view


@pytest.mark.parametrize("plane", [(32, 32), (37, 71), (513, 512)], ids=case_id)
def test_views_at_4_byte_offsets_give_the_dense_bits(hip_backend, plane):
    """4 and 8 modulo 16: the wide backward gives way to the narrow one, the forward reads as ever"""
    from pseudocylindrical_convolution_amd import _metric_ops
    x, y, wt = _case((2, 3), plane)
    x, y, w = x.cuda(), y.cuda(), wt.on("cuda")
    gout = torch.tensor([[0.5, -1.0, 2.0], [1.5, 0.25, -3.0]], dtype=torch.float64, device="cuda")
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    want = _metric_ops.weighted_mse_device(x, y, w, wt.total)
    grad = _metric_ops.weighted_mse_backward(x, y, w, wt.total, gout)
    for ox, oy, ow in ((1, 0, 0), (0, 2, 0), (1, 2, 0), (3, 1, 0), (0, 0, 1), (2, 1, 1)):
        xo, yo, wo = _at_offset(x, ox), _at_offset(y, oy), _at_offset(w, ow)
        assert xo.data_ptr() % 16 == 4 * ox and yo.data_ptr() % 16 == 4 * oy and wo.data_ptr() % 16 == 8 * ow
        assert SM.same_bits(_metric_ops.weighted_mse_device(xo, yo, wo, wt.total), want)
        assert SM.same_bits(_metric_ops.weighted_mse_backward(xo, yo, wo, wt.total, gout), grad)
    # u8 frames at any byte offset
    ux, uy = MC.frames_u8(2, *plane, seed=1).cuda(), MC.frames_u8(2, *plane, seed=2).cuda()
    base = _metric_ops.weighted_mse_device(ux, uy, w, wt.total)
    assert SM.same_bits(_metric_ops.weighted_mse_device(_at_offset(ux, 1), _at_offset(uy, 3), w, wt.total), base)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(name, a) for name, sizes in MC.POINT_SETS for a in sizes], ids=case_id)
def test_point_records_kernel_is_the_float64_twin(hip_backend, kind, case):
    from pseudocylindrical_convolution_amd import _metric_ops, cube
    name, a = case
    ps = MC.point_set(name)
    want = cube.point_records_numpy(ps, kind, a)
    dirs = torch.from_numpy(cube.point_directions(ps)).cuda()
    guard = 16
    flat = torch.full((2 * len(ps) + 2 * guard,), 77, dtype=torch.int32, device="cuda")
    out = flat[guard:guard + 2 * len(ps)].view(len(ps), 2)
    got = _metric_ops.cube_points_records(dirs, kind, a, out)
    assert got.data_ptr() == out.data_ptr()
    diff = got.cpu().numpy() != want
    assert not diff.any(), "%d records differ, first at %s" % (diff.any(1).sum(), np.argwhere(diff.any(1))[:1])
    host = flat.cpu()
    assert (host[:guard] == 77).all().item() and (host[-guard:] == 77).all().item()
    assert torch.equal(cube.point_records(ps, kind, a, "cuda").cpu(), torch.from_numpy(want))


def _pictures():
    """(operand, spec) by name: ERP pictures of two sizes and cube pictures of both kinds, three layouts, three sizes"""
    from pseudocylindrical_convolution_amd import cube
    erp = MC.frames(2, 3, 16, 32, 1)
    return {"erp": (erp, None), "erp2": (MC.frames(2, 3, 24, 50, 2), None),
            "cmp8": (cube.from_erp(erp, 8, "cmp", layout="3x2"), cube.spec("cmp", "3x2")),
            "eac13": (MC.frames(2, 3, 13, 78, 3), cube.spec("eac", "6x1")),
            "cmp3": (MC.frames(2, 3, 18, 3, 4), cube.spec("cmp", "faces")),
            "eac8": (cube.from_erp(erp, 8, "eac", layout="faces"), cube.spec("eac", "faces"))}


MIXES = [("cmp8", "eac8"), ("eac13", "cmp8"), ("erp", "eac13"), ("cmp3", "erp2"), ("erp", "erp2"), ("eac8", "eac8")]


@pytest.mark.parametrize("interp", ["lanczos", "nearest"])
@pytest.mark.parametrize("points", ["icosphere2", "cpp_10x22", "erp_24x50"])
@pytest.mark.parametrize("mix", MIXES, ids=case_id)
def test_points_mse_is_the_twin_in_every_mode_and_mix(hip_backend, mix, points, interp):
    from pseudocylindrical_convolution_amd import cube
    pics = _twin("pictures", _pictures)
    (x, xs), (y, ys) = pics[mix[0]], pics[mix[1]]
    ps = MC.point_set(points)
    for sp in (xs, ys):     # the records the two sides use are equal: the shared sets' margins hold for these sizes
        if sp is not None:
            a = cube._picture_face(x if sp is xs else y, sp)
            assert torch.equal(cube.point_records(ps, sp.kind, a, "cuda").cpu(), cube.point_records(ps, sp.kind, a))
    want = _twin(("points", mix, points, interp), lambda: cube.points_mse(x, y, ps, interp, xs, ys))
    got = cube.points_mse(x.cuda(), y.cuda(), ps, interp, xs, ys)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3) and SM.same_bits(got, want), (got, want)
    if mix[0] == mix[1]:
        assert (got == 0).all()
    one = cube.points_mse(x[1:].cuda(), y[1:].cuda(), ps, interp, xs, ys)
    assert SM.same_bits(one, want[1:])                                  # a frame alone


def test_figures_on_the_gpu_are_the_cpu_figures(hip_backend):
    from pseudocylindrical_convolution_amd import cube
    pics = _twin("pictures", _pictures)
    (x, xs), (y, ys) = pics["cmp8"], pics["eac13"]
    for f, kw in ((cube.s_psnr_nn, dict(level=2)), (cube.s_psnr_i, dict(level=2)), (cube.cpp_psnr, {})):
        assert SM.same_bits(f(x.cuda(), y.cuda(), xs, ys, **kw), f(x, y, xs, ys, **kw))
    noisy = (x + 0.05 * MC.frames(2, 3, 16, 24, 9))
    assert SM.same_bits(cube.ws_psnr(x.cuda(), noisy.cuda(), xs), cube.ws_psnr(x, noisy, xs))
    assert SM.same_bits(cube.ws_mse(x.cuda(), noisy.cuda(), xs), cube.ws_mse(x, noisy, xs))


def test_results_do_not_depend_on_what_fresh_memory_held(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import cube, sphere_points
    from pseudocylindrical_convolution_amd import weighted_metrics as WM
    x, y, wt = _case((2, 3), (37, 71))
    x, y = x.cuda(), y.cuda()
    ps = sphere_points.PointSet(MC.point_set("erp_24x50").points)
    pics = _twin("pictures", _pictures)
    (cx, xs), (cy, ys) = pics["cmp8"], pics["eac13"]
    cx, cy = cx.cuda(), cy.cuda()
    results = {}
    for name, regime in SM.regimes(monkeypatch):
        with regime():
            ps.__dict__.pop("_cube_records", None)                       # the records are made again under every fill
            ps._records.clear()
            results[name] = [WM.mse(x, y, wt), *_gradients(x, y, wt, _coef(2)), cube.point_records(ps, "eac", 13, "cuda").cpu(),
                             cube.points_mse(cx, cy, ps, "lanczos", xs, ys), cube.points_mse(cx, cy, ps, "nearest", xs, ys),
                             cube.ws_mse(cx, cx * 0.5, xs)]
    for name in SM.KINDS:
        assert all(SM.same_bits(a, b) for a, b in zip(results[name], results["plain"])), name


def test_composite_training_gradient_is_the_twins(hip_backend):
    """an ERP output trained against a cube original: ws_loss_terms(from_erp(x), target) at 24x48 <-> a = 12"""
    from pseudocylindrical_convolution_amd import cube
    h, w, a = 24, 48, 12
    for kind, layout in (("eac", "3x2"), ("cmp", "faces")):
        sp = cube.spec(kind, layout)
        x = MC.frames(2, 3, h, w, seed=2)
        target = MC.frames(2, 3, *cube.picture_size(a, layout), seed=4)
        coef = _coef(2)

        def run(dev):
            xd = x.to(dev).requires_grad_(True)
            loss = cube.ws_loss_terms(cube.from_erp(xd, a, sp), target.to(dev), sp)
            (g,) = torch.autograd.grad((loss * coef.to(dev)).sum(), xd)
            return loss.detach().cpu(), g.cpu()
        want_loss, want = run("cpu")
        loss, got = run("cuda")
        assert SM.same_bits(loss, want_loss)
        assert SM.same_bits(got, want), "max abs diff %g" % (got - want).abs().max().item()
        assert (got != 0).any()


def _forms(t, dim=0):
    """(name, refused form) of a good operand: the wrong type, the wrong device, one short and one more along `dim` (the
    wrong shape), and a view that is not contiguous"""
    wrong = torch.float64 if t.dtype != torch.float64 else torch.float32
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]
    return [("dtype", t.to(wrong)), ("device", t.cpu()), ("short", t.narrow(dim, 0, t.shape[dim] - 1).contiguous()),
            ("shape", torch.cat([t, t.narrow(dim, 0, 1)], dim=dim)), ("strided", wide), ("no tensor", None)]


def test_every_new_wrapper_refuses_a_bad_operand_before_the_library(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd import _metric_ops, _native
    from pseudocylindrical_convolution_amd._native import PconvError
    real, calls = _native.call, []

    def recording(fn, *args):
        calls.append(fn)
        return real(fn, *args)
    monkeypatch.setattr(_native, "call", recording)
    n, c, h, w = 2, 3, 5, 7
    good = dict(x=MC.frames(n, c, h, w, 1).cuda(), y=MC.frames(n, c, h, w, 2).cuda(), weights=torch.ones(h, w, dtype=torch.float64, device="cuda"),
                gout=torch.ones(n, c, dtype=torch.float64, device="cuda"))
    u8 = dict(x=MC.frames_u8(n, h, w, 1).cuda(), y=MC.frames_u8(n, h, w, 2).cuda(), weights=good["weights"])
    dirs = torch.from_numpy(np.ascontiguousarray(np.eye(3)[[0, 1, 2, 0]])).cuda()
    wrappers = [("weighted_mse", lambda o: _metric_ops.weighted_mse_device(o["x"], o["y"], o["weights"], 35.0), good, ("x", "y", "weights")),
                ("weighted_mse", lambda o: _metric_ops.weighted_mse_device(o["x"], o["y"], o["weights"], 35.0), u8, ("y", "weights")),
                ("weighted_mse_backward", lambda o: _metric_ops.weighted_mse_backward(o["x"], o["y"], o["weights"], 35.0, o["gout"]), good,
                 ("x", "y", "weights", "gout")),
                ("cube_points_records", lambda o: _metric_ops.cube_points_records(o["dirs"], "cmp", 8, o.get("out")),
                 dict(dirs=dirs, out=torch.zeros(4, 2, dtype=torch.int32, device="cuda")), ("dirs", "out"))]
    checked = 0
    for what, run, operands, names in wrappers:
        run(operands)                                                   # the good call goes through
        assert calls, what
        for name in names:
            for form, bad in _forms(operands[name], 1 if name == "dirs" else 0):     # (any number of points is a point set)
                if name == "out" and form == "no tensor":
                    continue                                            # (None: a new one is made)
                if name == "x" and form in ("short", "shape", "dtype"):
                    # x defines the shapes and picks the entry: what does not fit it is then named as y
                    expect = r"%s: (x|y) must be" % what
                else:
                    expect = r"%s: %s must be" % (what, name)
                del calls[:]
                with pytest.raises(PconvError, match=expect):
                    run(dict(operands, **{name: bad}))
                assert calls == [], (what, name, form, calls)
                checked += 1
    assert checked >= 60
    del calls[:]
    for total in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(PconvError, match="total"):
            _metric_ops.weighted_mse_device(good["x"], good["y"], good["weights"], total)
    with pytest.raises(PconvError, match="kind"):
        _metric_ops.cube_points_records(dirs, "erp", 8)
    with pytest.raises(PconvError, match="dirs: 4 points on faces of 1"):
        _metric_ops.cube_points_records(dirs, "cmp", 1)
    assert calls == []


def test_cli_rd_and_test_with_cube_metrics(hip_backend, tmp_path, monkeypatch, capsys):
    """--rd --projection --cube-metrics reports what --test --projection --cube-metrics reports of the file: the same
    reconstruction, so the same four figures; without the flag both outputs are what they were"""
    import re
    import cube_cases as CC
    from pseudocylindrical_convolution_amd import cube, pseudo_codec as PC
    from test_cli import _models
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cuda")
    a = 64
    y = cube.from_erp(CC.smooth(2 * a, 4 * a), a, cube.spec("cmp", "6x1"), clamp=True)
    PC.write_image("cube.png", PC.tensor2img(y))
    common = ["--ssim", "--model-idx", "3"]
    rd = ["--rd", "--projection", "cmp", "--cube-layout", "6x1", "--img-list", "cube.png"] + common
    PC.main(["--enc", "--projection", "cmp", "--cube-layout", "6x1", "--container", "--img-list", "cube.png", "--code-list", "cube.pcv"] + common)
    test = ["--test", "--projection", "cmp", "--cube-layout", "6x1", "--code-list", "cube.pcv", "--img-list", "cube.png"]
    outs = {}
    for name, argv in (("rd", rd), ("rd+", rd + ["--cube-metrics"]), ("test", test), ("test+", test + ["--cube-metrics"])):
        capsys.readouterr()
        PC.main(argv)
        outs[name] = capsys.readouterr().out.splitlines()
    new = lambda l: l.lstrip().startswith(("CUBE-WS-PSNR:", "CUBE-S-PSNR-NN:"))
    for name in ("rd", "test"):
        assert not any(new(l) for l in outs[name])
        assert [l for l in outs[name + "+"] if not new(l)] == outs[name]
        assert len([l for l in outs[name + "+"] if new(l)]) == 4                  # two lines for the image, two for the average
    figures = lambda lines: re.findall(r"CUBE-(?:WS|S|CPP)-PSNR(?:-NN|-I)?:([0-9.]+)dB", "\n".join(lines))
    assert len(figures(outs["rd+"])) == 8 and figures(outs["rd+"]) == figures(outs["test+"])
    picture = PC.img2tensor(PC.read_image("cube.png"), "cuda")
    assert all(0 < float(v) < 100 for v in figures(outs["rd+"])) and picture.shape == (1, 3, a, 6 * a)
