"""Training on cube pictures without a GPU: the host lists of the face continuation's backward (include/pconv_hip.h,
pconv_host_cube_pad_reverse), its torch twin against float64 autograd of the forward, the statement of the weighted SSIM's
gradient (weighted_metrics.ssim_backward_torch), the composites cube.ws_ssim_loss_terms and cube.to_erp(grad=True) against
float64 autograd of their statements, the refusals, and two steps of train.py --loss cube-ws on the oracle backend."""
import os
import socket

import numpy as np
import pytest
import torch

import cube_loss_cases as L
from cube_loss_cases import U24
from pseudocylindrical_convolution_amd import _metric_ops, _native, cube, sphere_metrics, viewport, weighted_metrics as WM
from pseudocylindrical_convolution_amd._native import PconvError

CASES = L.pad_cases(L.LIST_FACES)


# ---- 1. the reverse lists ----

def _corners(table, a):
    """(6 ring, 4) int64: the pixel of the face stack each corner of each ring pixel reads, reduced as the forward does"""
    rec = np.asarray(table).astype(np.int64)
    g = np.clip(rec[:, 0], 0, 5)
    x0, y0 = np.clip(rec[:, 1] >> 8, 0, a - 1), np.clip(rec[:, 2] >> 8, 0, a - 1)
    x1, y1 = np.minimum(x0 + 1, a - 1), np.minimum(y0 + 1, a - 1)
    return np.stack([(g * a + yy) * a + xx for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))], axis=1)


@pytest.mark.parametrize("case", CASES, ids=L.pad_id)
def test_host_lists_are_sorted_complete_and_owned(case):
    kind, a, depth = case
    A = a + 2 * depth
    start, entry = cube.pad_reverse_lists(kind, a, depth)
    assert start.dtype == torch.int32 and entry.dtype == torch.int32
    total = 24 * (A * A - a * a)
    assert _native.call("pconv_host_cube_pad_reverse_size", a, depth) == total
    assert tuple(start.shape) == (6 * a * a + 1,) and tuple(entry.shape) == (total,)
    start, entry = start.numpy().astype(np.int64), entry.numpy().astype(np.int64)
    assert start[0] == 0 and start[-1] == total and np.all(np.diff(start) >= 0)
    assert np.array_equal(np.sort(entry), np.arange(total))                  # every (ring pixel, corner) exactly once
    owner = np.repeat(np.arange(6 * a * a), np.diff(start))
    same_list = owner[1:] == owner[:-1]
    assert np.all(entry[1:][same_list] > entry[:-1][same_list])             # ascending within each list
    want = _corners(cube.pad_table(kind, a, depth), a)
    assert np.array_equal(want[entry >> 2, entry & 3], owner)               # every entry decodes to its list's pixel
    if a == 2:
        # the clamp at a - 1 makes corners coincide: two entries of one ring pixel in one list
        twice = same_list & ((entry[1:] >> 2) == (entry[:-1] >> 2))
        assert twice.any()
    assert cube.pad_reverse_lists(kind, a, depth)[0] is cube.pad_reverse_lists(kind, a, depth)[0]     # cached


def test_lists_are_built_from_the_table_the_forward_reads():
    """a table of out-of-range records is reduced as the forward reduces it, and zero coefficients stay listed"""
    a, depth = 3, 1
    A = a + 2 * depth
    ring = A * A - a * a
    table = np.zeros((6 * ring, 3), dtype=np.int32)
    table[:, 0] = np.arange(6 * ring) % 9 - 2              # faces -2 .. 6
    table[:, 1] = (np.arange(6 * ring) % 7 - 2) * 256      # columns -2 .. 4, phase 0: the x1 corners weigh nothing
    table[:, 2] = 5 * 256 + 128
    start, entry = np.empty(6 * a * a + 1, dtype=np.int32), np.empty(24 * ring, dtype=np.int32)
    assert _native.call("pconv_host_cube_pad_reverse", table.ctypes.data, a, depth, start.ctypes.data, entry.ctypes.data) == 24 * ring
    owner = np.repeat(np.arange(6 * a * a), np.diff(start.astype(np.int64)))
    e = entry.astype(np.int64)
    assert np.array_equal(_corners(table, a)[e >> 2, e & 3], owner)


# ---- 2. the twin against float64 autograd of the forward ----

@pytest.mark.parametrize("case", CASES, ids=L.pad_id)
def test_twin_is_the_float64_adjoint(case):
    """bound 4 u L max|g|, L the longest list + 1: float32 summation error only, the coefficients are exact; the sum of
    gin over a plane is the sum of gout to the same bound, since the coefficients of a ring pixel add to 1"""
    kind, a, depth = case
    A = a + 2 * depth
    g = L.gradient(2, 2, 6 * A, A, seed=a * 10 + depth)
    lists = cube.pad_reverse_lists(kind, a, depth)
    table = cube.pad_table_on(kind, a, None, depth)
    got = cube.pad_backward_torch(g, table, lists, a, depth)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 2, 6 * a, a)
    assert torch.equal(got, cube.pad_backward(g, kind, a, depth))
    y = L.frames(2, 2, 6 * a, a, seed=1).double().requires_grad_(True)
    out = L.pad64(y, kind, depth)
    assert (out.detach() - cube.pad_torch(y.detach().float(), table, depth).double()).abs().max().item() < 1e-6     # the same forward
    (want,) = torch.autograd.grad(out, y, g.double())
    bound = 4 * U24 * (L.longest(lists) + 1) * g.abs().max().item()
    err = (got.double() - want).abs().max().item()
    print("pad backward %s: L %d err %.3g bound %.3g" % (L.pad_id(case), L.longest(lists) + 1, err, bound))
    assert err <= bound
    sums = (got.double().sum(dim=(2, 3)) - g.double().sum(dim=(2, 3))).abs().max().item()
    assert sums <= bound, (sums, bound)


@pytest.mark.parametrize("kind", L.KINDS)
def test_pad_under_autograd_is_opt_in(kind):
    a, depth = 7, 5
    A = a + 2 * depth
    y = L.frames(1, 3, 6 * a, a, seed=3).requires_grad_(True)
    out = cube.pad(y, kind, depth, grad=True)
    assert out.requires_grad and torch.equal(out.detach(), cube.pad(y.detach(), kind, depth))
    g = L.gradient(1, 3, 6 * A, A, seed=4)
    (got,) = torch.autograd.grad(out, y, g)
    assert torch.equal(got, cube.pad_backward(g, kind, a, depth))
    assert torch.equal(got, torch.autograd.grad(cube.pad(y, kind, depth, grad=True), y, g)[0])       # in a defined order
    with pytest.raises(PconvError, match="padded stack"):
        cube.pad_backward(g[:, :, 1:], kind, a, depth)
    with pytest.raises(PconvError, match="depth"):
        cube.pad_backward(g, kind, a, 9)
    with pytest.raises(PconvError, match="lists are not those"):
        cube.pad_backward_torch(g, cube.pad_table_on(kind, a, None, depth), cube.pad_reverse_lists(kind, a, 3), a, depth)


# ---- 3. the statement of the weighted SSIM's gradient ----

class _Planes(torch.autograd.Function):
    """the float64 statement of the weighted SSIM per plane, its backward ssim_backward_torch"""

    @staticmethod
    def forward(ctx, x, y, plane):
        ctx.save_for_backward(x, y)
        ctx.plane = plane
        m = sphere_metrics._ssim_map(sphere_metrics._moments(x, y, sphere_metrics.gaussian()), True)
        return (m * plane.on()).sum(dim=(2, 3)) / plane.total

    @staticmethod
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        return WM.ssim_backward_torch(y, x, ctx.plane, gout), WM.ssim_backward_torch(x, y, ctx.plane, gout), None


def test_ssim_statement_passes_gradcheck():
    rs = np.random.RandomState(5)
    plane = WM.WeightPlane(rs.rand(7, 9) + 0.1)
    x = torch.from_numpy(rs.rand(2, 2, 7, 9))
    y = torch.from_numpy(x.numpy() + 0.1 * rs.randn(2, 2, 7, 9)).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda p, q: _Planes.apply(p, q, plane), (xg, y))          # ssim_backward_torch itself
    assert torch.autograd.gradcheck(lambda q: WM.ssim_loss_terms(x, q, plane), (y,))           # the CPU entry, by torch
    terms = WM.ssim_loss_terms(x, y, plane)
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (2,) and terms.requires_grad
    assert torch.allclose(terms.detach(), WM.channel_mean(WM.ssim_torch(x, y.detach(), plane)), rtol=0, atol=1e-15)
    gout = torch.from_numpy(rs.randn(2))
    (auto,) = torch.autograd.grad(terms, y, gout)
    want = WM.ssim_backward_torch(x, y.detach(), plane, (gout / 2.0)[:, None].expand(2, 2))    # the channel mean's share
    assert (auto - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_ssim_statement_is_the_erp_statement_for_the_cosine_plane():
    h, w = 24, 40
    rs = np.random.RandomState(6)
    x = torch.from_numpy(rs.rand(2, 1, h, w))
    y = torch.from_numpy(x.numpy() + 0.1 * rs.randn(2, 1, h, w))
    g = torch.from_numpy(rs.randn(2))
    want = sphere_metrics.backward_torch(x, y, torch.stack([torch.zeros(2, dtype=torch.float64), g], dim=1), dt=torch.float64)
    got = WM.ssim_backward_torch(x, y, WM.erp_plane(h, w), g[:, None], dt=torch.float64)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_a_zero_block_has_a_gradient_in_its_border_and_none_deeper_in():
    h, w = 40, 44
    rs = np.random.RandomState(7)
    wt = rs.rand(h, w) + 0.1
    wt[8:32, 10:36] = 0.0
    x = torch.from_numpy(rs.rand(1, 2, h, w).astype(np.float32))
    y = x + 0.1 * torch.from_numpy(rs.randn(1, 2, h, w).astype(np.float32))
    gout = torch.tensor([[1.0, -0.5]], dtype=torch.float64)
    for dt in (torch.float64, torch.float32):
        got = WM.ssim_backward_torch(x, y, wt, gout, dt=dt)
        assert got.dtype == dt
        # a pixel's gradient gathers k a, k b, k c over its 11 x 11 window: up to 5 pixels inside the block some k of the
        # window is not zero; deeper in every k is zero, and so is every term
        border = torch.ones(24, 26, dtype=torch.bool)
        border[5:-5, 5:-5] = False
        block = got[:, :, 8:32, 10:36]
        assert (block[:, :, border] != 0).all()
        assert (block[:, :, ~border] == 0).all() and (~border).sum() == 14 * 16
    # uint8 carries no gradient; the forward entries keep refusing a tensor that requires grad
    u8 = torch.zeros((1, h, w, 3), dtype=torch.uint8)
    with pytest.raises(PconvError, match="uint8"):
        WM.ssim_loss_terms(u8, u8, wt)
    for fn in (WM.ssim, WM.ssim_device, WM.ssim_torch):
        with pytest.raises(PconvError, match="requires grad"):
            fn(x, y.clone().requires_grad_(True), wt)
    with pytest.raises(PconvError, match="gout"):
        WM.ssim_backward_torch(x, y, wt, gout[:, :1])
    with pytest.raises(PconvError, match="GPU"):
        WM.ssim_backward(x, y, wt, gout)


# ---- 4. the composites against float64 autograd of their statements, a = 12, "3x2" ----

@pytest.mark.parametrize("kind", L.KINDS)
def test_ws_ssim_loss_terms_against_float64_autograd(kind):
    """The statement is cube.ws_ssim's: both pictures unpacked, continued by 5 pixels in float32 (pad's bits), the
    float64 SSIM of the padded stacks weighed by ssim_plane, the channel mean.  Its float64 gradient: the SSIM
    differentiated at the padded stacks the forward holds, then through the continuation as a function of real numbers
    (pad64).  The entry differs from it by (1) the rounding of the padded stack's gradient g to float32, at most u |g| per
    element, which the continuation's adjoint (coefficients >= 0, a list of at most L - 1 entries plus the pixel's own
    copy) carries to at most u L max|g|, and (2) the float32 sums of pad_backward, 4 u L max|g|: 5 u L max|g| in all"""
    a = 12
    sp = cube.spec(kind, "3x2")
    x = L.frames(1, 2, 2 * a, 3 * a, seed=11)
    y = (x + 0.1 * L.gradient(1, 2, 2 * a, 3 * a, seed=12)).requires_grad_(True)
    terms = cube.ws_ssim_loss_terms(x, y, sp)
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (1,) and terms.requires_grad
    assert abs(terms.item() - cube.ws_ssim(x, y.detach(), sp).item()) <= 1e-14
    (got,) = torch.autograd.grad(terms, y, torch.ones(1, dtype=torch.float64))
    assert got.dtype == torch.float32 and got.shape == y.shape
    # the statement in float64
    plane = cube.ssim_plane(kind, a)
    yd = y.detach().double().requires_grad_(True)
    real = L.pad64(L.unpack64(yd), kind, cube.SSIM_PAD)
    held = cube.pad(cube.unpack(y.detach(), "3x2").contiguous(), kind, cube.SSIM_PAD).double()
    stack_y = held + (real - real.detach())          # the values the forward holds, the derivative of the real map
    stack_y.retain_grad()
    stack_x = cube.pad(cube.unpack(x, "3x2").contiguous(), kind, cube.SSIM_PAD).double()
    m = sphere_metrics._ssim_map(sphere_metrics._moments(stack_x, stack_y, sphere_metrics.gaussian()), True)
    want_terms = WM.channel_mean((m * plane.on()).sum(dim=(2, 3)) / plane.total)
    want_terms.sum().backward()
    want, g_stack = yd.grad, stack_y.grad
    lists = cube.pad_reverse_lists(kind, a, cube.SSIM_PAD)
    bound = 5 * U24 * (L.longest(lists) + 1) * g_stack.abs().max().item()
    err = (got.double() - want).abs().max().item()
    print("ws_ssim_loss_terms %s: G %.3g err %.3g bound %.3g" % (kind, want.abs().max().item(), err, bound))
    assert err <= bound
    # the rings weigh zero and still carry a gradient to the neighbouring faces
    A = a + 2 * cube.SSIM_PAD
    ring = g_stack.reshape(1, 2, 6, A, A).clone()
    ring[:, :, :, 5:5 + a, 5:5 + a] = 0
    assert ring.abs().max().item() > 1e-3 * g_stack.abs().max().item()
    # both pictures at once: the gradient of x is that of y with the pictures exchanged (the SSIM is symmetric)
    xb, yb = x.clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    cube.ws_ssim_loss_terms(xb, yb, sp).sum().backward()
    assert torch.equal(yb.grad, got)
    xc = x.clone().requires_grad_(True)
    cube.ws_ssim_loss_terms(y.detach(), xc, sp).sum().backward()
    assert torch.equal(xb.grad, xc.grad)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("ss", [1, 2])
def test_to_erp_with_grad_against_float64_autograd(kind, ss):
    """to_erp is linear: sampler(pad(unpack(y))).  The float32 backward walks, per element of the padded stack, the remap
    list (at most Lr terms of two products each, times 1/ss^2 for ss > 1: Lr + 3 roundings deep) and then, per face pixel,
    the continuation's list (Lp roundings deep with its product and the start value).  With S the same adjoint in float64
    over the magnitudes (|weights|, |g|) -- the sum of the magnitudes of all terms an element is made of -- the error is
    at most (Lr + 3 + Lp) u S per element to first order; 1.01 covers the higher orders"""
    a = 12
    sp = cube.spec(kind, "3x2")
    h, w = cube.erp_size(a)
    A = a + 2 * cube.PAD
    y = L.frames(1, 2, 2 * a, 3 * a, seed=21).requires_grad_(True)
    out = cube.to_erp(y, None, sp, ss=ss, grad=True)
    assert out.requires_grad and torch.equal(out.detach(), cube.to_erp(y.detach(), None, sp, ss=ss))
    g = L.gradient(1, 2, h, w, seed=22)
    (got,) = torch.autograd.grad(out, y, g)
    assert got.dtype == torch.float32 and got.shape == y.shape
    assert torch.equal(got, torch.autograd.grad(cube.to_erp(y, None, sp, ss=ss, grad=True), y, g)[0])       # in a defined order
    map = cube.to_erp_map(kind, a, h, w, ss)
    yd = y.detach().double().requires_grad_(True)
    want64 = L.sampler64(L.pad64(L.unpack64(yd), kind, cube.PAD), map, h, w, ss)
    assert (want64.detach() - out.detach().double()).abs().max().item() <= 1e-5
    (want,) = torch.autograd.grad(want64, yd, g.double())
    ya = y.detach().double().requires_grad_(True)
    (S,) = torch.autograd.grad(L.sampler64(L.pad64(L.unpack64(ya), kind, cube.PAD), map, h, w, ss, absolute=True), ya,
                               g.double().abs())
    Lr = L.longest(viewport.reverse_lists(map, 6 * A, A))
    Lp = L.longest(cube.pad_reverse_lists(kind, a, cube.PAD)) + 1
    bound = 1.01 * (Lr + 3 + Lp) * U24 * S
    err = (got.double() - want).abs()
    print("to_erp grad %s ss %d: Lr %d Lp %d G %.3g err %.3g bound %.3g" % (kind, ss, Lr, Lp, want.abs().max().item(),
                                                                        err.max().item(), bound.max().item()))
    assert (err <= bound).all()
    # clamp: torch.clamp's gradient
    big = (3.0 * y.detach() - 1.0).requires_grad_(True)
    clamped = cube.to_erp(big, None, sp, ss=ss, clamp=True, grad=True)
    plain = cube.to_erp(big.detach(), None, sp, ss=ss)
    assert torch.equal(clamped.detach(), plain.clamp(0.0, 1.0))
    (gc,) = torch.autograd.grad(clamped, big, g)
    (gm,) = torch.autograd.grad(cube.to_erp(big, None, sp, ss=ss, grad=True), big, g * ((plain >= 0) & (plain <= 1)))
    assert torch.equal(gc, gm)


# ---- 5. refusals ----

def test_the_opt_ins_are_opt_ins():
    a = 8
    y = L.frames(1, 2, 2 * a, 3 * a, seed=31).requires_grad_(True)
    with pytest.raises(PconvError, match="no backward"):
        cube.to_erp(y, None, "cmp", layout="3x2")
    with pytest.raises(PconvError, match="requires grad"):
        cube.ws_ssim(y.detach(), y, cube.spec("cmp", "3x2"))
    with torch.no_grad():
        assert not cube.to_erp(y, None, "cmp", layout="3x2", grad=True).requires_grad
    assert not cube.to_erp(y.detach(), None, "cmp", layout="3x2", grad=True).requires_grad
    with pytest.raises(PconvError, match="uint8"):
        u8 = torch.zeros((1, 2 * a, 3 * a, 3), dtype=torch.uint8)
        cube.ws_ssim_loss_terms(u8, u8, cube.spec("cmp", "3x2"))
    with pytest.raises(PconvError, match="one kind, layout, face size"):
        cube.ws_ssim_loss_terms(y, y[:, :, :, :a], cube.spec("cmp", "3x2"))


def test_the_library_refuses_on_the_host():
    """no launch: every refusal comes before (this runs without a GPU)"""
    lib = _native.hip_lib()
    D = 4096      # never dereferenced
    err = lambda: lib.pconv_last_error()
    pad = lambda *args: lib.pconv_cube_pad_backward_f32(*args)
    for args, word in (((None, 2 * D, 3 * D, 4 * D, 5 * D, 1, 1, 8, 5, None), b"null"), ((D, None, 3 * D, 4 * D, 5 * D, 1, 1, 8, 5, None), b"null"),
                       ((D, 2 * D, None, 4 * D, 5 * D, 1, 1, 8, 5, None), b"null"), ((D, 2 * D, 3 * D, None, 5 * D, 1, 1, 8, 5, None), b"null list"),
                       ((D, 2 * D, 3 * D, 4 * D, None, 1, 1, 8, 5, None), b"null list"), ((D, D, 3 * D, 4 * D, 5 * D, 1, 1, 8, 5, None), b"distinct"),
                       ((D + 2, 2 * D, 3 * D, 4 * D, 5 * D, 1, 1, 8, 5, None), b"aligned"), ((D, 2 * D, 3 * D, 4 * D + 1, 5 * D, 1, 1, 8, 5, None), b"aligned"),
                       ((D, 2 * D, 3 * D, 4 * D, 5 * D, 1, 1, 1, 5, None), b"face size"), ((D, 2 * D, 3 * D, 4 * D, 5 * D, 1, 1, 8, 0, None), b"depth"),
                       ((D, 2 * D, 3 * D, 4 * D, 5 * D, 1, 1, 8, 9, None), b"depth"), ((D, 2 * D, 3 * D, 4 * D, 5 * D, 1, 1, 9453, 4, None), b"2^31"),
                       ((D, 2 * D, 3 * D, 4 * D, 5 * D, 70000, 1, 8, 5, None), b"planes"), ((D, 2 * D, 3 * D, 4 * D, 5 * D, 0, 1, 8, 5, None), b"planes")):
        assert pad(*args) < 0 and b"cube_pad_backward_f32" in err() and word in err(), (args, err())
    assert lib.pconv_host_cube_pad_reverse_size(8, 5) == 24 * (18 * 18 - 64) and lib.pconv_host_cube_pad_reverse_size(9453, 3) == 24 * (9459 ** 2 - 9453 ** 2)
    for a, depth in ((1, 3), (8, 0), (8, 9), (9453, 4)):
        assert lib.pconv_host_cube_pad_reverse_size(a, depth) < 0
    start, entry = np.full(6 * 4 + 1, -7, dtype=np.int32), np.full(24 * 12, -7, dtype=np.int32)
    table = np.zeros((6 * 12, 3), dtype=np.int32)
    rev = lambda *args: lib.pconv_host_cube_pad_reverse(*args)
    for args in ((None, 2, 1, start.ctypes.data, entry.ctypes.data), (table.ctypes.data, 2, 1, None, entry.ctypes.data),
                 (table.ctypes.data, 2, 1, start.ctypes.data, None), (table.ctypes.data, 1, 1, start.ctypes.data, entry.ctypes.data),
                 (table.ctypes.data, 2, 9, start.ctypes.data, entry.ctypes.data)):
        assert rev(*args) < 0
    assert (start == -7).all() and (entry == -7).all()                  # nothing is written unless every argument passes
    ssim = lambda *args: lib.pconv_weighted_ssim_backward_f32(*args)
    G = 8 * D
    for args, word in (((None, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, G, None), b"null"), ((D, None, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, G, None), b"null"),
                       ((D, 2 * D, None, 1.0, 4 * D, 1, 1, 4, 4, G, None), b"null"), ((D, 2 * D, 3 * D, 1.0, None, 1, 1, 4, 4, G, None), b"null"),
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, None, None), b"null"), ((D + 2, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, G, None), b"aligned"),
                       ((D, 2 * D, 3 * D + 4, 1.0, 4 * D, 1, 1, 4, 4, G, None), b"aligned"), ((D, 2 * D, 3 * D, 1.0, 4 * D + 4, 1, 1, 4, 4, G, None), b"aligned"),
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, G + 1, None), b"aligned"), ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 0, 4, G, None), b"side"),
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, (1 << 20) + 1, G, None), b"side"), ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 1 << 15, 1 << 14, G, None), b"2^31"),
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 256, 256, 4, 4, G, None), b"planes"), ((D, 2 * D, 3 * D, 0.0, 4 * D, 1, 1, 4, 4, G, None), b"positive finite"),
                       ((D, 2 * D, 3 * D, float("inf"), 4 * D, 1, 1, 4, 4, G, None), b"positive finite"),
                       ((D, 2 * D, 3 * D, float("nan"), 4 * D, 1, 1, 4, 4, G, None), b"positive finite"),
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, D + 8, None), b"alias"),           # the gradient inside x
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, 2 * D, None), b"alias"),           # ... on y
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, 3 * D + 8, None), b"alias"),       # ... inside the weights
                       ((D, 2 * D, 3 * D, 1.0, 4 * D, 1, 1, 4, 4, 4 * D, None), b"alias")):          # ... on gout
        assert ssim(*args) < 0 and b"weighted_ssim_backward_f32" in err() and word in err(), (args, err())


def test_wrappers_refuse_cpu_operands_before_the_library(monkeypatch):
    calls = []
    monkeypatch.setattr(_native, "call", lambda fn, *args: calls.append(fn))
    x, wt = torch.zeros(1, 1, 12, 2), torch.ones(12, 2, dtype=torch.float64)
    with pytest.raises(PconvError, match="weighted_ssim_backward: x must be"):
        _metric_ops.weighted_ssim_backward(x, x, wt, 24.0, torch.ones(1, 1, dtype=torch.float64))
    with pytest.raises(PconvError, match="cube_pad_backward: g must be"):
        _metric_ops.cube_pad_backward(torch.zeros(1, 1, 6 * 12, 12), None, None, 2, 5)
    with pytest.raises(PconvError, match="cube_pad_backward: depth must be"):
        _metric_ops.cube_pad_backward(x, None, None, 2, 9)
    assert calls == []


# ---- 6. training ----

def _free_port():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def test_train_with_the_cube_ws_loss_on_the_cpu(oracle_backend, tmp_path, monkeypatch):
    """--loss cube-ws --device cpu for two steps on 256 x 512, the smallest frame the model takes as it is: finishes, logs
    finite terms, constructs neither MultiProject nor SSIM, goes through the two new backwards, and the parameters change"""
    import torch.distributed as dist
    from pseudocylindrical_convolution_amd import train

    def refuse(*a, **k):
        raise AssertionError("--loss cube-ws must not construct the reference's viewport loss")

    monkeypatch.setattr(train, "MultiProject", refuse)
    monkeypatch.setattr(train, "SSIM", refuse)
    seen, sums = [], []
    real_pad_backward, real_losses = cube.pad_backward, train.forward_losses
    monkeypatch.setattr(cube, "pad_backward", lambda g, kind, a, depth=cube.PAD: (seen.append((kind, a, depth)), real_pad_backward(g, kind, a, depth))[1])

    def losses(args, model, *rest):
        sums.append(sum(p.detach().double().abs().sum().item() for p in model.parameters()))
        return real_losses(args, model, *rest)

    monkeypatch.setattr(train, "forward_losses", losses)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
    argv = ["--device", "cpu", "--loss", "cube-ws", "--cube-kind", "eac", "--synthetic", "2", "--height", "256", "--width", "512",
            "--batch-size", "1", "--test-batch-size", "1", "--acc-batch", "1", "--epochs", "1", "--max-steps", "2", "--valid-dim", "8",
            "--channels", "16", "--code-dim", "16", "--workers", "0", "--no-opt", "--mean", "0", "--beta", "0.1", "--alpha", "0.05",
            "--base-dir", str(tmp_path)]
    args = train.build_parser().parse_args(argv)
    assert args.loss == "cube-ws" and args.cube_kind == "eac" and args.cube_face is None and "cube-ws" in train.OWN_LOSSES
    assert train.make_sim_func(args, "cpu") is None
    defaults = train.build_parser().parse_args([])
    assert defaults.loss == "viewport" and defaults.cube_kind is None and defaults.cube_face is None
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
    assert log.count("Train Epoch: 1") == 2 and "Test set:" in log and "nan" not in log.lower() and "eac cube picture" in log
    assert ("eac", 128, cube.SSIM_PAD) in seen                         # the face continuation's backward ran, faces of w / 4
    assert len(sums) >= 3 and sums[0] != sums[1] and sums[1] != sums[2]      # both steps moved the parameters
