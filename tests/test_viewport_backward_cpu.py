"""The ordered backward of the viewport renderer and of the sphere rotation without a GPU (include/pconv_hip.h,
pconv_remap_backward_f32): the host lists against a numpy construction, the torch twin against the definition as a plain
sequential float32 loop and against the float64 adjoint within a derived bound, the adjoint identity, Renderer.render and
erp_rotate.rotate under autograd, the refusals, viewport.loss_terms and train.py --loss vp on the oracle backend."""
import os
import socket

import numpy as np
import pytest
import torch

import train_resume_cases as R
import viewport_backward_cases as B
from viewport_backward_cases import CASES, case_id

U24 = 2.0 ** -24


def _free_port():
    """a port nothing listens on now (the process groups of earlier tests leave listeners of their own choosing behind)"""
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _job(base_dir, extra):
    R._port[0] = _free_port() - 1
    return R.job(base_dir, extra)


def _lists(case):
    from pseudocylindrical_convolution_amd import viewport
    return viewport.reverse_lists(B.source_map(case), case[0], case[1])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_lists_are_a_stable_sort_of_the_forward_walk(case):
    h, w, vh, vw, ss, _ = case
    start, entry = _lists(case)
    assert start.dtype == torch.int32 and entry.dtype == torch.int32
    assert start.numel() == h * w + 1 and entry.numel() == 36 * vh * ss * vw * ss
    want_start, want_entry = B.numpy_lists(B.source_map(case), h, w)
    assert np.array_equal(start.numpy(), want_start) and np.array_equal(entry.numpy(), want_entry)
    assert start[0].item() == 0 and start[-1].item() == entry.numel()
    e, s = entry.numpy().astype(np.int64), start.numpy()
    inner = np.ones(e.size, dtype=bool)
    inner[s[:-1][s[:-1] < e.size]] = False          # the first entry of each list has no predecessor in it
    assert (np.diff(e)[inner[1:]] > 0).all()         # ascending within each list
    assert np.array_equal(np.sort(e), np.arange(e.size))


def test_host_lists_refuse_bad_arguments_before_writing():
    from pseudocylindrical_convolution_amd._native import PconvError, call, hip_lib
    q = np.ascontiguousarray(B.source_map(B.TINY[0]).numpy())
    start, entry = np.full(17, -7, dtype=np.int32), np.full(36 * 60, -7, dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    assert call("pconv_host_remap_reverse_size", 6, 10) == 36 * 60
    assert hip_lib().pconv_host_remap_reverse_size(1 << 13, 1 << 13) < 0
    for hole in range(3):
        args = [ptr(q), 6, 10, 4, 4, ptr(start), ptr(entry)]
        args[(0, 5, 6)[hole]] = None
        with pytest.raises(PconvError, match="null pointer"):
            call("pconv_host_remap_reverse", *args)
    for bad, reason in (((6, 10, 1, 4), "source side"), ((6, 10, 1 << 15, 1 << 15), "source plane"), ((1, 10, 4, 4), "grid side"),
                        ((1 << 14, 1 << 14, 4, 4), "map of"), ((1 << 13, 1 << 13, 4, 4), "do not fit int32")):
        with pytest.raises(PconvError, match=reason):
            call("pconv_host_remap_reverse", ptr(q), bad[0], bad[1], bad[2], bad[3], ptr(start), ptr(entry))
    assert (start == -7).all() and (entry == -7).all()
    assert call("pconv_host_remap_reverse", ptr(q), 6, 10, 4, 4, ptr(start), ptr(entry)) == 36 * 60


@pytest.mark.parametrize("case", B.TINY + [CASES[2]], ids=case_id)
def test_twin_is_the_sequential_float32_walk_bit_for_bit(case):
    from pseudocylindrical_convolution_amd import viewport
    h, w, vh, vw, ss, _ = case
    q, lists = B.source_map(case), _lists(case)
    for n, c in B.BATCHES:
        g = B.gradient(n, c, vh, vw)
        want = B.sequential_scatter(g, q, h, w, vh, vw, ss)
        got = viewport.render_backward_torch(g, q, lists, h, w, vh, vw, ss)
        assert got.dtype == torch.float32 and torch.equal(got, want)
        first = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(5))
        again = viewport.render_backward_torch(g, q, lists, h, w, vh, vw, ss, accumulate_into=first)
        assert torch.equal(again, B.sequential_scatter(g, q, h, w, vh, vw, ss, into=first))
        untouched = (lists[0][1:] == lists[0][:-1]).view(h, w)
        assert torch.equal(again[:, :, untouched], first[:, :, untouched])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_twin_is_within_the_chains_bound_of_the_float64_adjoint(case):
    """a term is three roundings (g' for ss > 1, and the two products), a list of L terms L additions, and the float64
    adjoint's 1 / ss^2 differs from float32(1 / ss^2) by one more: |twin - f64| <= (L + 4) 2^-24 sum|term| per pixel"""
    from pseudocylindrical_convolution_amd import viewport
    h, w, vh, vw, ss, _ = case
    n, c = B.BATCHES[0]
    q, lists = B.source_map(case), _lists(case)
    g = B.gradient(n, c, vh, vw, seed=1)
    x = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
    B.render64(x, q, ss).backward(g.double())
    twin = viewport.render_backward_torch(g, q, lists, h, w, vh, vw, ss)
    length = (lists[0][1:] - lists[0][:-1]).view(1, 1, h, w).double()
    bound = (length + 4) * U24 * B.scatter64(g, q, h, w, vh, vw, ss, absolute=True)
    err = (twin.double() - x.grad).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print("twin vs float64 adjoint %s: worst error %.3g of its bound, longest list %d" % (case_id(case), worst, int(length.max())))
    assert bool((err <= bound).all())
    assert bool((twin[(length == 0).expand_as(twin)] == 0).all())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_adjoint_identity_in_float64(case):
    """<render(x), g> = <x, backward(g)>, the backward taken from the destinations in float64"""
    h, w, vh, vw, ss, _ = case
    n, c = B.BATCHES[0]
    q = B.source_map(case)
    x = torch.rand((n, c, h, w), dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    g = B.gradient(n, c, vh, vw, seed=2)
    lhs = (B.render64(x, q, ss) * g.double()).sum().item()
    rhs = (x * B.scatter64(g, q, h, w, vh, vw, ss)).sum().item()
    if ss > 1:   # scatter64 holds the float32 factor of the definition, render64 the exact one
        rhs *= (1.0 / (ss * ss)) / float(np.float32(1.0 / (ss * ss)))
    scale = (x * B.scatter64(g, q, h, w, vh, vw, ss, absolute=True)).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)


def _renderer3(device="cpu"):
    from pseudocylindrical_convolution_amd import viewport
    r = viewport.Renderer(32, 64, [viewport.view(*a) for a in B.VIEWS3], (9, 15), device=device)
    assert r.ss == (1, 2, 4) and all(p[:2] == (32, 64) for p in r.plans)
    return r


def test_renderer_under_autograd_is_three_chained_twin_calls():
    from pseudocylindrical_convolution_amd import viewport
    r = _renderer3()
    x = torch.rand(2, 3, 32, 64, generator=torch.Generator().manual_seed(3)).requires_grad_()
    out = r.render(x)
    assert out.grad_fn is not None and torch.equal(out.detach(), r.render(x.detach()))
    assert r._lists == [None] * 3                                    # nothing is built before the first backward
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(4))
    out.backward(g)
    want = None
    for k in range(3):
        want = viewport.render_backward_torch(g[:, k].contiguous(), r.maps[k], r.lists(k), 32, 64, 9, 15, r.plans[k][2],
                                              accumulate_into=want)
    assert torch.equal(x.grad, want)
    with torch.no_grad():
        assert r.render(x).grad_fn is None


def test_rotate_under_autograd_is_the_twin_with_ss_1():
    from pseudocylindrical_convolution_amd import erp_rotate, viewport
    rot = erp_rotate.units(123.25, -33.5, -170)
    x = torch.rand(2, 3, 50, 99, generator=torch.Generator().manual_seed(6)).requires_grad_()
    out = erp_rotate.rotate(x, rot)
    assert out.grad_fn is not None and torch.equal(out.detach(), erp_rotate.rotate(x.detach(), rot))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    out.backward(g)
    q = erp_rotate.source_map(50, 99, rot)
    assert torch.equal(x.grad, viewport.render_backward_torch(g, q, viewport.reverse_lists(q, 50, 99), 50, 99, 50, 99, 1))
    assert erp_rotate.rotate(x, None) is x


def test_clamp_masks_as_torch_clamp_does():
    from pseudocylindrical_convolution_amd import viewport
    r = _renderer3()
    x = (torch.rand(1, 2, 32, 64, generator=torch.Generator().manual_seed(8)) * 1.5 - 0.25).requires_grad_()
    raw = r.render(x.detach())
    assert bool((raw < 0).any()) and bool((raw > 1).any())
    out = r.render(x, clamp=True)
    assert torch.equal(out.detach(), r.render(x.detach(), clamp=True))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    out.backward(g)
    leaf = raw.clone().requires_grad_()
    leaf.clamp(0.0, 1.0).backward(g)                                 # torch.clamp's own mask
    assert bool((leaf.grad == 0).any())
    want = None
    for k in range(3):
        want = viewport.render_backward_torch(leaf.grad[:, k].contiguous(), r.maps[k], r.lists(k), 32, 64, 9, 15,
                                              r.plans[k][2], accumulate_into=want)
    assert torch.equal(x.grad, want)


def test_the_three_refusals_name_their_reason():
    from pseudocylindrical_convolution_amd import erp_rotate, viewport
    from pseudocylindrical_convolution_amd._native import PconvError
    r = _renderer3()
    x = torch.rand(1, 1, 32, 64).requires_grad_()
    with pytest.raises(PconvError, match="out= cannot be combined with a gradient"):
        r.render(x, out=torch.empty(1, 3, 1, 9, 15))
    assert r.render(x.detach(), out=torch.empty(1, 3, 1, 9, 15)).grad_fn is None
    with pytest.raises(PconvError, match="out= cannot be combined with a gradient"):
        erp_rotate.rotate(x, erp_rotate.units(1, 2, 3), out=torch.empty(1, 1, 32, 64))
    v = viewport.view(0, 0, 0, 120, 90)
    assert viewport.plan(64, 128, v, 4, 6)[:2] != (64, 128)
    small = viewport.Renderer(64, 128, [v], (4, 6))
    big = torch.rand(1, 1, 64, 128)
    assert small.render(big).shape == (1, 1, 1, 4, 6)
    with pytest.raises(PconvError, match="carries no gradient"):
        small.render(big.requires_grad_())
    huge = torch.zeros(2, dtype=torch.int32).expand(1 << 13, 1 << 13, 2)   # no memory behind it: refused before it is read
    with pytest.raises(PconvError, match="beyond int32"):
        viewport.reverse_lists(huge, 32, 64)


def test_loss_terms_are_the_metrics():
    from pseudocylindrical_convolution_amd import viewport
    r = _renderer3()
    g = torch.Generator().manual_seed(10)
    x = torch.rand(2, 3, 32, 64, generator=g)
    y = (x + 0.1 * torch.randn(x.shape, generator=g)).requires_grad_()
    terms = viewport.loss_terms(r, x, y)
    assert terms.dtype == torch.float64 and terms.shape == (2, 2) and terms.requires_grad
    assert torch.equal(terms.detach().cpu(), viewport.metrics(r, x, y.detach()))
    terms.sum().backward()
    assert y.grad is not None and bool(torch.isfinite(y.grad).all()) and bool((y.grad != 0).any())


def test_train_with_the_vp_loss_on_the_cpu(oracle_backend, tmp_path, monkeypatch):
    """--loss vp --device cpu for two steps: finishes, logs finite mse / ssim / rate, constructs neither MultiProject nor
    SSIM; the renderer is the one --test --vp would score with"""
    import torch.distributed as dist
    from pseudocylindrical_convolution_amd import train

    def refuse(*a, **k):
        raise AssertionError("--loss vp must not construct the reference's viewport loss")

    monkeypatch.setattr(train, "MultiProject", refuse)
    monkeypatch.setattr(train, "SSIM", refuse)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
    args = train.build_parser().parse_args(
        ["--device", "cpu", "--loss", "vp", "--synthetic", "2", "--height", "256", "--width", "512", "--batch-size", "1",
         "--test-batch-size", "1", "--acc-batch", "1", "--epochs", "1", "--max-steps", "2", "--valid-dim", "8",
         "--channels", "16", "--code-dim", "16", "--workers", "0", "--no-opt", "--mean", "0", "--beta", "0.1",
         "--alpha", "0.05", "--base-dir", str(tmp_path)])
    assert args.vp_size is None and train.make_sim_func(args, "cpu") is None
    try:
        hist = train.Job(0, 1, args)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(hist) == 1
    (loss, mse, ssim, rate), ls = hist[0]
    assert all(np.isfinite(v) for v in (loss, mse, ssim, rate)) and mse > 0 and -1 <= ssim <= 1 and rate > 0
    assert len(ls) == 1 and np.isfinite(ls[0]) and ls[0] > 0          # gamma mse + beta (1 - ssim) + alpha rate
    log = open(os.path.join(str(tmp_path), "save_models", "ent_normal_16_8_16_logs_0.txt")).read()
    assert log.count("Train Epoch: 1") == 2 and "Test set:" in log and "nan" not in log.lower()
    renderer = train.vp_renderer(args, torch.empty(1, 3, 256, 512))
    assert (renderer.vh, renderer.vw) == (85, 128) and len(renderer.views) == 14
    assert any(l is not None for l in renderer._lists)


def test_vp_size_and_the_loss_choice_parse():
    from pseudocylindrical_convolution_amd import train
    args = train.build_parser().parse_args(["--loss", "vp", "--vp-size", "96x64"])
    assert args.loss == "vp" and args.vp_size == (64, 96)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--loss", "vp", "--vp-size", "96"])


@pytest.mark.timeout(600)
def test_resume_refuses_a_changed_vp_loss_by_name(oracle_backend, tmp_path):
    extra = ["--base", "--loss", "vp", "--vp-size", "48x32"]
    _job(tmp_path, extra + ["--stop-after", "1"])
    for changed, name in ((["--base"], "--loss"), (["--base", "--loss", "vp"], "--vp-size"),
                          (["--base", "--loss", "vp", "--vp-size", "48x30"], "--vp-size")):
        with pytest.raises(ValueError, match="written with %s = " % name):
            _job(tmp_path, changed + ["--resume"])
    _job(tmp_path / "old", ["--base", "--stop-after", "1"])
    assert "vp_size" not in R.state(tmp_path / "old", ["--base"])["fingerprint"]      # a file of before --vp-size resumes
