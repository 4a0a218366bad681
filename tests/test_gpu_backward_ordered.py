"""GPU: the ordered (atomic-free) backward kernels under PCONV.ordered_backward(True).  Slice, uslice and the
viewport sampling walk the oracle's own order, so they are held to the oracle BIT FOR BIT (tests/test_gpu_backward.py
keeps holding the default, float-atomic form to 1e-5 / 1e-4); the quantiser's level sums have a fixed shape of their
own and are held bit for bit to its numpy twin (tests/backward_ordered_cases.py) and to the default form's bound of
the oracle."""
import numpy as np
import pytest
import torch

import backward_ordered_cases as B
from oracle import pconv_cpu as O
from ref_ops_cases import NPART, PHI, THETA, W16, WEIGHTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


@pytest.fixture(autouse=True)
def ordered():
    with P().ordered_backward(True):
        yield
    assert P().backward_is_ordered() is False


def slice_pair(weight, pad, shape, seed):
    """(GPU op, oracle op, gradient of the tile stack) after a forward call of both at `shape`"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    gop, cop = P().SphereSliceOp(NPART, 0, pad, weight, 0, False), O.SphereSliceOp(NPART, 0, pad, weight)
    gop.forward(x.to(DEV))
    return gop, cop, torch.randn(cop.forward(x)[0].shape, generator=g)


def uslice_pair(weight, pad, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    gop, cop = P().SphereUsliceOp(NPART, 0, pad, weight, 0, False), O.SphereUsliceOp(NPART, 0, pad, weight)
    gop.forward(x.to(DEV))
    return gop, cop, torch.randn(cop.forward(x)[0].shape, generator=g)


SMALL = [("WNOPT", 24), ("WNOPT", 40), ("WFULL", 72)]


# ---- slice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pad", [((2, 2, 256, 512), 1), ((1, 3, 512, 1024), 0)])
def test_slice_backward_is_the_oracle(shape, pad):
    gop, cop, grad = slice_pair(W16, pad, shape, 1)
    assert torch.equal(gop.backward(grad.to(DEV))[0].cpu(), cop.backward(grad)[0])


@pytest.mark.parametrize("wset,width", SMALL)
def test_slice_backward_is_the_oracle_on_narrow_and_wrapping_tiles(wset, width):
    for rows in (16, 32):
        for pad in (0, 1, 2):
            gop, cop, grad = slice_pair(WEIGHTS[wset], pad, (2, 2, rows, width), rows + pad)
            got, want = gop.backward(grad.to(DEV))[0].cpu(), cop.backward(grad)[0]
            assert torch.equal(got, want), (rows, pad, int((got != want).sum()))


# ---- uslice --------------------------------------------------------------------------------------------------------
def uslice_check(weight, pad, shape, seed):
    gop, cop, grad = uslice_pair(weight, pad, shape, seed)
    want = cop.backward(grad)[0]
    gop.backward(grad.to(DEV))
    gop._top[1].fill_(NAN)                      # the op's output buffer: the kernel itself must write every zero
    got = gop.backward(grad.to(DEV))[0].cpu()
    assert torch.equal(got, want), (shape, pad, int((got != want).sum()))
    widths = O.widths_v3(weight, NPART, (shape[2] - 2 * pad) * NPART, shape[3] - 2 * pad)
    for t in range(NPART):                      # exactly zero outside the valid interior
        keep = torch.zeros(got.shape[2:], dtype=torch.bool)
        keep[pad:got.shape[2] - pad, pad:pad + int(widths[t])] = True
        assert (got[t::NPART][:, :, ~keep] == 0).all()


def test_uslice_backward_is_the_oracle():
    uslice_check(W16, 2, (32, 2, 18, 516), 2)


@pytest.mark.parametrize("wset,width", SMALL)
def test_uslice_backward_is_the_oracle_on_narrow_and_wrapping_tiles(wset, width):
    for rows in (1, 2):
        for pad in (0, 1, 2):
            uslice_check(WEIGHTS[wset], pad, (2 * NPART, 2, rows + 2 * pad, width + 2 * pad), rows + pad)


# ---- projects --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("view,shape", [((12, 18), (2, 3, 32, 64)), ((96, 144), (1, 2, 256, 512))])
def test_projects_backward_is_the_oracle(near, view, shape):
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*shape, generator=g)
    gop, cop = P().ProjectsOp(view[0], view[1], THETA, PHI, 0.5, near, 0, False), O.ProjectsOp(view[0], view[1], THETA, PHI, 0.5, near)
    gop.forward(x.to(DEV))
    grad = torch.randn(cop.forward(x)[0].shape, generator=g)
    want, want_count = cop.backward(grad)
    gop.backward(grad.to(DEV))
    gop._top[1].fill_(NAN)                      # pixels no sample reaches must come back 0: there is no memset
    gop._top[2].fill_(NAN)
    got, got_count = (t.cpu() for t in gop.backward(grad.to(DEV)))
    assert torch.equal(got, want) and torch.equal(got_count, want_count)
    if view == (12, 18):
        assert (want_count == 0).any()          # pixels with empty lists are among the cases


# ---- quantiser ---------------------------------------------------------------------------------------------------------
def quant_ops(shape, ntop):
    c = shape[1]
    gctx, octx = P().PseudoContextOp(NPART, 20, W16, 0, False), O.PseudoContextOp(NPART, 20, W16)
    gop = P().PseudoQuantOp(c, 8, NPART, 0.9, 100, ntop, 0.1, gctx.addr(), 0, False)
    cop = O.PseudoQuantOp(c, 8, NPART, 0.9, 100, ntop, 0.1, octx.addr())
    return gop, cop


def quant_inputs(shape, ntop, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g) * 1.2 - 0.1
    weight = torch.zeros(shape[1], 8)
    weight[:, 0] = 1. / 9
    weight[:, 1:] = float(np.log(1. / 9))
    weight += torch.rand(shape[1], 8, generator=g) * 0.05
    return x, weight, [torch.randn(shape, generator=g) for _ in range(ntop)]


# test_quant_backward's shape; a plane of 300 elements (no multiple of 256); a width that is no multiple of 4
@pytest.mark.parametrize("shape,ntop", [((16, 192, 2, 64), 1), ((16, 192, 2, 64), 2), ((16, 6, 3, 100), 2), ((32, 5, 2, 66), 1)])
def test_quant_backward_is_its_twin_and_within_the_default_bound(shape, ntop):
    O.set_detmath(True)
    x, weight, grads = quant_inputs(shape, ntop)
    gop, cop = quant_ops(shape, ntop)
    xg, gg = x.to(DEV), [t.to(DEV) for t in grads]
    og = gop.forward(xg, weight.to(DEV), torch.zeros(shape[1], 8, device=DEV), False)
    with P().ordered_backward(False):
        atomic = [t.clone() for t in gop.backward(gg, xg, og[0])]
    got = gop.backward(gg, xg, og[0])
    assert torch.equal(got[0], atomic[0])                      # g_in: elementwise, the same expressions
    assert torch.equal(got[2], atomic[2])
    widths = O.widths_v3(W16, NPART, shape[2] * NPART, shape[3])
    twin = B.quant_twin(x.numpy(), og[0].cpu().numpy(), gop._top[1].cpu().numpy(), gop._top["tab"].cpu().numpy(), widths, NPART)
    assert torch.equal(got[1].cpu(), torch.from_numpy(twin))   # g_weight: the fixed shape, bit for bit
    oc = cop.forward(x, weight, torch.zeros(shape[1], 8), False)
    want = cop.backward(grads, x, oc[0])
    for a, b, tol in ((got[0], want[0], 1e-6), (got[1], want[1], 1e-4)):   # the bounds of test_quant_backward
        assert (a.cpu() - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())
    assert torch.equal(got[2].cpu(), want[2])


# ---- independence of batch neighbours -----------------------------------------------------------------------------------
def test_each_frame_of_a_batch_gets_the_bits_it_gets_alone():
    # slice: the tile stack is frame-major
    gop, _, grad = slice_pair(WEIGHTS["WNOPT"], 1, (2, 3, 32, 40), 3)
    both = gop.backward(grad.to(DEV))[0].clone()
    for i in range(2):
        alone = gop.backward(grad[i * NPART:(i + 1) * NPART].contiguous().to(DEV))[0]
        assert torch.equal(alone[0], both[i])
    gop, _, grad = uslice_pair(W16, 2, (2 * NPART, 3, 2 + 4, 128 + 4), 4)
    both = gop.backward(grad.to(DEV))[0].clone()
    for i in range(2):
        alone = gop.backward(grad[i:i + 1].contiguous().to(DEV))[0]
        assert torch.equal(alone, both[i * NPART:(i + 1) * NPART])
    # projects: the viewport stack is (view, frame, channel)
    g = torch.Generator().manual_seed(5)
    gop = P().ProjectsOp(12, 18, THETA, PHI, 0.5, False, 0, False)
    y = gop.forward(torch.randn(2, 3, 32, 64, generator=g).to(DEV))[0]
    grad = torch.randn(y.shape, generator=g)
    both = [t.clone() for t in gop.backward(grad.to(DEV))]
    for i in range(2):
        gop.forward(torch.zeros(1, 3, 32, 64, device=DEV))
        part = grad.view(len(THETA), 2, 3, 12, 18)[:, i].contiguous().view(len(THETA), 3, 12, 18)
        alone = gop.backward(part.to(DEV))
        assert torch.equal(alone[0][0], both[0][i]) and torch.equal(alone[1][0], both[1][i])
    # quantiser: the input gradient (the level gradient is a sum over the batch by definition)
    shape = (2 * NPART, 6, 3, 100)
    x, weight, grads = quant_inputs(shape, 2)
    gop, _ = quant_ops(shape, 2)
    xg, gg = x.to(DEV), [t.to(DEV) for t in grads]
    og = gop.forward(xg, weight.to(DEV), torch.zeros(6, 8, device=DEV), False)
    both = gop.backward(gg, xg, og[0])[0].clone()
    for i in range(2):
        sl = slice(i * NPART, (i + 1) * NPART)
        xa = xg[sl].contiguous()
        oa = gop.forward(xa, weight.to(DEV), torch.zeros(6, 8, device=DEV), False)
        alone = gop.backward([t[sl].contiguous() for t in gg], xa, oa[0])[0]
        assert torch.equal(alone, both[sl])


# ---- a whole graph of the project's own ops: the same seed gives the same bits ---------------------------------------------
def test_a_graph_of_the_projects_own_ops_trains_to_the_same_bits_twice(hip_backend):
    from pseudocylindrical_convolution_amd.PCONV_operator import (MultiProject, PseudoContextV2, PseudoQUANTV2, SphereSlice,
                                                                  SphereUslice)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gain = torch.nn.Parameter(torch.ones(1, 3, 1, 1))
            self.ctx = PseudoContextV2(NPART, True, device=0)
            self.slice = SphereSlice(NPART, pad=0, opt=True, device=0)
            self.quant = PseudoQUANTV2(3, 8, NPART, self.ctx, device_id=0)
            self.uslice = SphereUslice(NPART, pad=0, opt=True, device=0)
            self.project = MultiProject(24, 36, 0.5, False, 0)

        def forward(self, x):
            return self.project(self.uslice(self.quant(self.slice(x * self.gain))))

    def run():
        torch.manual_seed(11)
        x = torch.rand(2, 3, 256, 512, generator=torch.Generator().manual_seed(7)).to(DEV)
        net = Net().to(DEV).train()
        with torch.no_grad():
            target = MultiProject(24, 36, 0.5, False, 0).to(DEV)(x).clone()
        opt = torch.optim.Adam([net.quant.weight, net.gain], lr=1e-2)
        first = None
        for _ in range(3):
            opt.zero_grad()
            ((net(x) - target) ** 2).mean().backward()
            if first is None:
                first = [net.quant.weight.grad.clone(), net.gain.grad.clone()]
            opt.step()
        return first, [net.quant.weight.detach().clone(), net.gain.detach().clone()]

    P().backward_launches.clear()
    (ga, pa), (gb, pb) = run(), run()
    for a, b in zip(ga + pa, gb + pb):
        assert torch.equal(a, b)
    assert ga[0].abs().sum() > 0 and ga[1].abs().sum() > 0      # the gradients reach both parameters
    ran = P().backward_launches
    for name in ("pconv_sphere_slice_backward", "pconv_sphere_uslice_backward", "pconv_project_backward", "pconv_quant_backward"):
        assert ran[name + "_ordered"] == 6 and ran[name] == 0, dict(ran)


# ---- the switch ------------------------------------------------------------------------------------------------------------
def test_switch_off_gives_the_atomic_kernels_again():
    PC = P()
    gop, _, grad = slice_pair(W16, 0, (1, 1, 32, 72), 6)
    gd = grad.to(DEV)
    PC.backward_launches.clear()
    gop.backward(gd)
    assert dict(PC.backward_launches) == {"pconv_sphere_slice_backward_ordered": 1}
    with PC.ordered_backward(False):
        assert PC.backward_is_ordered() is False
        gop.backward(gd)
        assert PC.backward_launches["pconv_sphere_slice_backward"] == 1
    assert PC.backward_is_ordered() is True
    with pytest.raises(ZeroDivisionError):
        with PC.ordered_backward(False):
            1 / 0
    assert PC.backward_is_ordered() is True                    # restored after an exception too
    gop.backward(gd)
    assert PC.backward_launches["pconv_sphere_slice_backward_ordered"] == 2
    # the reverse tables live beside the forward tables and leave with them
    assert any(k[0] == "reverse" for k in gop._tabs)
    gop.to(1)
    assert gop._tabs == {}
