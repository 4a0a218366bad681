"""The oracle's GDN references against each other and against the module formula, on the CPU.

`gdn_chain` is the float32 restatement the GPU tests hold the fused kernel to bit for bit
(tests/test_gpu_gdn.py); `gdn_f64` is the same formula in float64 with a plain matmul.  The bound between
them is derived, not measured.  With u = 2^-24 (half an ulp of float32) and K = ch:
  * the norm is a sum of K + 1 non-negative terms (K products gamma * x^2 and beta), each square rounded once
    and each accumulation rounded once: no cancellation, relative error <= (K + 2) u;
  * the square root halves a relative error: (K + 2) / 2 u, plus one rounding of its own;
  * one rounding for the divide (inverse: the multiply), one for the residual add (relative to the sum).
So |err| <= ((K + 2) / 2 + 2) u |y| + u |residual + y|, y = the GDN output before the residual.
"""
import pytest
import torch

from oracle import pconv_cpu as O

U = 2.0 ** -24
LIMITS = [134, 128, 129, 127, 64, 65, 63, 1, 0, 33, 134, 100, 130, 6, 70, 134]


def bound(ch, y64, out64):
    """the bound above, element by element: y64 the float64 GDN output before the residual, out64 after it"""
    return ((ch + 2) / 2 + 2) * U * y64.abs() + U * out64.abs()


def draw(tn, ch, h, w, scale, seed, hard=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tn, ch, h, w, generator=g) * scale
    gamma = 0.01 * torch.rand(ch, ch, generator=g) + 0.1 * torch.eye(ch)
    beta = torch.rand(ch, generator=g) + 0.5
    res = torch.randn(tn, ch, h, w, generator=g) * scale
    if hard:
        # rows of gamma that are all zero with beta at the module's beta_min (the norm is exactly beta), entries of
        # gamma up to 1 elsewhere, and exact zeros in the input
        gamma = torch.rand(ch, ch, generator=g)
        dead = torch.arange(ch) % 7 == 3
        gamma[dead] = 0
        beta[dead] = 1e-6
        x[torch.rand(x.shape, generator=g) < 0.05] = 0
    return x, gamma, beta, res


def check(got, x, gamma, beta, inverse, res, limit, npart):
    y64 = O.gdn_f64(x, gamma, beta, inverse, None, limit, npart)
    out64 = O.gdn_f64(x, gamma, beta, inverse, res, limit, npart)
    err = (got.double() - out64).abs()
    room = bound(x.shape[1], y64, out64)
    worst = (err - room).max().item()
    print("ch %d inverse %d: max err / bound = %.3g" % (x.shape[1], inverse, (err / room.clamp(min=1e-300)).max().item()))
    assert worst <= 0, "error exceeds the derived bound by %g" % worst
    return out64


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape,scale,hard", [((3, 192, 3, 70), 1.0, False), ((3, 192, 3, 70), 1e-3, False),
                                              ((3, 192, 3, 70), 1e3, False), ((3, 192, 3, 70), 1.0, True),
                                              ((2, 40, 3, 37), 1.0, False), ((2, 24, 2, 9), 1.0, True)])
def test_gdn_chain_within_derived_bound_of_float64(shape, scale, hard, inverse):
    """(a) gdn_chain against gdn_f64 under the bound of the module docstring: with and without residual and trim"""
    x, gamma, beta, res = draw(*shape, scale, seed=71, hard=hard)
    w = shape[3]
    limit = torch.tensor(LIMITS, dtype=torch.int32).clamp(max=w)
    limit = torch.roll(limit, -4)  # (tiles 0.. get 64, 65, 63, 1, 0, 33 clamped to w: few tiles, every kind of limit)
    for r, lim, npart in ((None, None, 0), (res, None, 0), (res, limit, 16), (None, limit, 16)):
        got = O.gdn_chain(x, gamma, beta, inverse, r, lim, npart)
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        out64 = check(got, x, gamma, beta, inverse, r, lim, npart)
        if lim is not None:
            whole = O.gdn_chain(x, gamma, beta, inverse, r)
            for t in range(shape[0]):
                at = int(lim[t % 16])
                assert got[t, :, :, at:].abs().sum().item() == 0
                assert torch.equal(got[t, :, :, :at], whole[t, :, :, :at])
        assert out64.abs().sum() > 0
    if hard:
        # where gamma's row is zero the norm is beta exactly: x / sqrt(beta) with two roundings, nothing else
        dead = torch.arange(shape[1]) % 7 == 3
        # (float64 sqrt rounded to float32 is the correctly rounded float32 sqrt; torch's float32 CPU sqrt is not always)
        root = torch.sqrt(beta[dead].double()).float().view(1, -1, 1, 1)
        plain = O.gdn_chain(x, gamma, beta, inverse)
        assert torch.equal(plain[:, dead], x[:, dead] * root if inverse else x[:, dead] / root)
        assert (plain[x == 0] == 0).all()


@pytest.mark.parametrize("inverse", [False, True])
def test_module_formula_within_derived_bound_of_float64(oracle_backend, inverse):
    """(b) PseudoGDNV2._formula on the oracle backend (pinned to the reference's own code by
    test_reference_wrappers.py) against gdn_f64 on the module's effective parameters and the context's fill widths,
    under the same bound.  The formula's mask blend (norm * mask + 1 - mask) rounds once more where mask = 1: at most
    2 u of sqrt(norm) >= 1, which these parameters give (beta >= 1) -- inside the bound, which charges the K + 1 term
    sum its worst case"""
    from pseudocylindrical_convolution_amd.PCONV_operator import PseudoContextV2, PseudoGDNV2
    torch.manual_seed(3)
    ctx = PseudoContextV2(16, True, device=0)
    gdn = PseudoGDNV2(192, 16, ctx, 0, inverse=inverse)
    with torch.no_grad():
        gdn.gamma.add_(torch.rand_like(gdn.gamma) * 0.02)
        gdn.beta.add_(torch.rand_like(gdn.beta) * 0.1)
    x = torch.randn(16, 192, 2, 128)
    ctx.setup_context(128)
    with torch.no_grad():
        got = gdn._formula(x)
        gamma, beta = gdn.effective()
    limit = ctx.produce_fill_param(0, 2, 128).to(torch.int32)
    assert limit.numel() == 16 and int(limit.min()) < 128 <= int(limit.max())
    check(got, x, gamma, beta, inverse, None, limit, 16)
    for t in range(16):
        assert got[t, :, :, int(limit[t]):].abs().sum().item() == 0
