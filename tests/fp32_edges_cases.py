"""Shared by tests/test_fp32_edges_cpu.py and tests/test_gpu_fp32_edges.py: the bit comparator, the input recipes that
drive the bit-exact kernels to float32's edges (subnormals, signed zeros, overflow), and the shapes they run at.

A regime is a pair of exponents (ex, ew): `randn` inputs times 2^ex, `randn / sqrt(cin k k)` weights times 2^ew, the
bias times 2^(ex + ew) -- exact powers of two, applied in float64 and rounded to float32 once.

  R1 (-70, -70)   normal inputs, every product and every output subnormal
  R2 (0, -140)    subnormal weights
  R3 (-126, 0)    two thirds of the inputs subnormal
  R4 (-100, -49)  products at the underflow edge: outputs are a few units of 2^-149, or exact zeros
  R5 (100, 27)    outputs around 2^127: some overflow to Inf
  R6              signed zeros: x = -0 everywhere / x = +0 against negated weights; bias absent, +0, -0

Nothing here turns torch.set_flush_denormal on; the oracle library keeps subnormals on the CPU (asserted by the CPU
test through the shares below)."""
import math

import numpy as np
import torch

FLT_MAX = 3.4028234663852886e38
FLT_MIN = 2.0 ** -126          # smallest normal
SUB = 2.0 ** -130              # "a subnormal"

# ---- the comparator ------------------------------------------------------------------------------------------------


def is_subnormal(t):
    a = t.abs()
    return (a > 0) & (a < FLT_MIN)


def shares(t):
    """fractions of subnormal / zero / -0 / Inf / NaN entries of a float32 tensor"""
    t = t.detach().cpu().contiguous()
    n = float(max(t.numel(), 1))
    neg0 = (t == 0) & (t.view(torch.int32) < 0)
    return {"sub": int(is_subnormal(t).sum()) / n, "zero": int((t == 0).sum()) / n, "neg0": int(neg0.sum()) / n,
            "inf": int(torch.isinf(t).sum()) / n, "nan": int(torch.isnan(t).sum()) / n}


def shares_text(t):
    s = shares(t)
    return "sub %.3f zero %.3f (-0 %.3f) inf %.3f nan %.3f" % (s["sub"], s["zero"], s["neg0"], s["inf"], s["nan"])


def differing(a, b):
    """mask of the entries whose bits differ; two NaNs in one place are equal whatever their payload"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (a.view(torch.int32) != b.view(torch.int32)) & ~(torch.isnan(a) & torch.isnan(b))


def same_bits(got, ref, what=""):
    """bit equality (the sign of zero counts).  On failure: how many entries differ and how many of those are
    subnormal, zero or non-finite on either side"""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(ref.shape))
    bad = differing(got, ref)
    nbad = int(bad.sum())
    if nbad:
        g, r = got[bad], ref[bad]
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(
            "%s: %d of %d entries differ; of those subnormal on either side %d, zero %d, non-finite %d; first at %s: got %r "
            "(0x%08x), expected %r (0x%08x)"
            % (what, nbad, bad.numel(), int((is_subnormal(g) | is_subnormal(r)).sum()), int(((g == 0) | (r == 0)).sum()),
               int((~torch.isfinite(g) | ~torch.isfinite(r)).sum()), first, got[first].item(),
               got.view(torch.int32)[first].item() & 0xffffffff, ref[first].item(),
               ref.view(torch.int32)[first].item() & 0xffffffff))


def flushed(t):
    """t with every subnormal replaced by +0"""
    return torch.where(is_subnormal(t), torch.zeros_like(t), t)


# ---- regimes of the convolutions -----------------------------------------------------------------------------------

REGIMES = {"R1": (-70, -70), "R2": (0, -140), "R3": (-126, 0), "R4": (-100, -49), "R5": (100, 27)}
R6 = [(xs, bias) for xs in ("x-0", "w-neg") for bias in ("none", "+0", "-0")]
ALL_REGIMES = list(REGIMES) + ["R6:%s:%s" % v for v in R6]

# (tn, cin, h, w, cout, k, stride, setting): one shape per instantiation class conv_kernel_name can return
CONV_SHAPES = [(1, 24, 5, 40, 16, 3, 1, "default")] + \
    [(1, 24, 5, 40, cout, 3, s, "default") for cout in (32, 96, 192) for s in (1, 2)] + \
    [(1, 32, 3, 40, cout, 1, s, "default") for cout in (32, 96, 192) for s in (1, 2)] + \
    [(1, 32, 3, 40, cout, 1, 1, "resident") for cout in (96, 192)]
CONV_SETTINGS = {"default": {}, "resident": {"PCONV_CONV1X1": "resident"}}


def conv_kernel_class(cfg):
    """the kernel name (without template arguments) the shape must reach"""
    tn, cin, h, w, cout, k, s, setting = cfg
    if setting == "resident":
        return "conv1x1_rb_kernel"
    return "conv_small_kernel" if (cout <= 16 and k == 3 and s == 1) else "conv_mfma_kernel"


def scaled(t, e):
    """t * 2^e, rounded to float32 once"""
    return (t.double() * (2.0 ** e)).float()


def slopes(cout, g):
    """PReLU slopes that include 0, a subnormal, a negative value and 1"""
    sl = torch.rand(cout, generator=g)
    sl[:4] = torch.tensor([0.0, SUB, -0.5, 1.0])
    return sl


def conv_inputs(cfg, regime, seed=77):
    """x, weight, bias (or None), slopes, residual of one shape in one regime; the residual is at the outputs' scale"""
    tn, cin, h, w, cout, k, stride = cfg[:7]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tn, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / np.sqrt(cin * k * k))
    b = torch.randn(cout, generator=g)
    sl = slopes(cout, g)
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    res = torch.randn(tn, cout, ho, wo, generator=g)
    if regime in REGIMES:
        ex, ew = REGIMES[regime]
        x, wt = scaled(x, ex), scaled(wt, ew)
        inside = -149 <= ex + ew <= 127
        b = scaled(b, ex + ew) if inside else torch.zeros(cout)
        res = scaled(res, max(min(ex + ew, 127), -149))
    else:
        _, xs, bias = regime.split(":")
        if xs == "x-0":
            x = torch.full_like(x, -0.0)
        else:
            x, wt = torch.zeros_like(x), -wt
        b = {"none": None, "+0": torch.zeros(cout), "-0": torch.full((cout,), -0.0)}[bias]
        res = torch.where(torch.rand(res.shape, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    return x, wt, b, sl, res


def chain_overflows_both_ways(x, wt, b, stride):
    """mask of the outputs whose float64 chain (products, partial sums, the bias) leaves float32's range in both signs:
    the only places where the fmaf chain may meet Inf - Inf"""
    k = wt.shape[2]
    cols = torch.nn.functional.unfold(x.double(), k, stride=stride)                 # (tn, cin k k, L), chain order
    terms = wt.double().reshape(wt.shape[0], -1)[None, :, :, None] * cols[:, None]  # (tn, cout, K, L)
    part = terms.cumsum(2)
    if b is not None:
        bias = b.double().view(1, -1, 1, 1).expand(terms.shape[0], -1, 1, terms.shape[3])
        part = torch.cat([part, part[:, :, -1:] + bias], 2)
        terms = torch.cat([terms, bias], 2)
    hi = torch.maximum(part.amax(2), terms.amax(2)) > FLT_MAX
    lo = torch.minimum(part.amin(2), terms.amin(2)) < -FLT_MAX
    tn, cout = x.shape[0], wt.shape[0]
    ho, wo = (x.shape[2] - k) // stride + 1, (x.shape[3] - k) // stride + 1
    return (hi & lo).reshape(tn, cout, ho, wo)


def regime_condition(regime, out, x=None, wt=None, b=None, stride=1):
    """None when the oracle's output `out` has the property the regime exists for, else what is missing"""
    s = shares(out)
    if regime in ("R1", "R2"):
        return None if s["sub"] >= 0.95 else "subnormal share %.3f < 0.95" % s["sub"]
    if regime == "R3":
        return None if s["sub"] >= 0.5 else "subnormal share %.3f < 0.5" % s["sub"]
    if regime == "R4":
        return None if s["sub"] > 0 and s["zero"] > 0 else "subnormal %.3f, zero %.3f: both kinds wanted" % (s["sub"], s["zero"])
    if regime == "R5":
        if s["inf"] < 0.02:
            return "Inf share %.3f < 0.02" % s["inf"]
        if s["nan"] and bool((torch.isnan(out) & ~chain_overflows_both_ways(x, wt, b, stride)).any()):
            return "NaN where the float64 chain does not overflow in both signs"
        return None
    # R6: with a zero bias (or none) the oracle's chain starts at +0 and returns +0 everywhere
    return None if s["zero"] == 1.0 and s["neg0"] == 0.0 else "zero %.3f, -0 %.3f: +0 everywhere wanted" % (s["zero"], s["neg0"])


# ---- GDN ---------------------------------------------------------------------------------------------------------------

GDN_BETA_MIN = 1e-6   # the module's beta_min (test_gpu_gdn.py's "hard" inputs)


def gdn_inputs(tn, ch, h, w, seed=301):
    """every third channel x 2^-80 (x * x underflows to 0), channels 5, 11, ... x 2^-70 (x * x is subnormal), channel 1 of +-0, channel 2 x 2^70 in every
    other column (x * x overflows, and with it the norm of every channel gamma couples to it: forward x / Inf = +-0,
    inverse x * Inf, 0 * Inf = NaN on the zero channel), beta at its re-parametrised minimum on every fourth channel,
    whose gamma rows couple to the tiny channels only (the norm there is beta_min plus subnormal products)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tn, ch, h, w, generator=g)
    x[:, 0::3] = scaled(x[:, 0::3], -80)
    x[:, 5::6] = scaled(x[:, 5::6], -70)
    x[:, 1] = torch.where(x[:, 1] < 0, torch.tensor(-0.0), torch.tensor(0.0))
    x[:, 2, :, 0::2] = scaled(x[:, 2, :, 0::2], 70)
    gamma = 0.01 * torch.rand(ch, ch, generator=g) + 0.1 * torch.eye(ch)
    beta = torch.rand(ch, generator=g) + 0.5
    beta[0::4] = GDN_BETA_MIN
    gamma[0::4] = 0          # on those channels the norm is exactly beta_min
    gamma[0::4, 0::3] = 0.01 * torch.rand(gamma[0::4, 0::3].shape, generator=g)   # ... plus the tiny channels' squares
    gamma[0::4, 5::6] = 0.01 * torch.rand(gamma[0::4, 5::6].shape, generator=g)
    res = torch.randn(tn, ch, h, w, generator=g)
    return x, gamma, beta, res


# ---- the entropy model: exact re-parametrisation by s = 2^-k ---------------------------------------------------------

ENT_SHAPES = [(2, 64, 1), (2, 80, 3)]
K_EXACT = 40
# the smallest multiple of 5 at which the oracle's streams differ from those at k = 40: from there on hidden activations
# are subnormal and the bits they lose reach the tables (measured on the oracle, asserted by test_fp32_edges_cpu.py)
K_SUB = 105           # at ENT_SHAPES[0]; (2, 80, 3) follows at 110
# the 28- and 48-group nets (test_gpu_wide_models.py's construction): 2 x 40 symbol planes, one frame -- the oracle's
# pass over a wide net is the cost of the test, and its smallest shape there (5 x 40) takes it 7 to 12 s
ENT_WIDE_SHAPE = (2, 40, 1)


def reparametrised(state, k):
    """the entropy net's state dict with every one of its three parameter nets scaled through by s = 2^-k: first
    layer's weights and bias x s, every later hidden bias x s, the last layer's weights x 1/s, its bias untouched.
    PReLU and the residual adds are positively homogeneous: in the normal range every hidden activation is s times
    what it was and the outputs are the same bits."""
    out = {}
    for name, t in state.items():
        t = t.clone()
        if name.endswith(".relu"):
            pass
        elif name.startswith("net.0."):
            t = scaled(t, -k)
        elif name.startswith("net.6."):
            t = scaled(t, k) if name.endswith(".weight") else t
        elif name.endswith(".bias"):
            t = scaled(t, -k)
        out[name] = t
    return out


def ent_symbols(ent, h, w, n, seed):
    sym = torch.randint(0, 8, (16 * n, ent.ngroup, h, w), generator=torch.Generator().manual_seed(seed)).float()
    return sym


# ---- pconv_expf's arguments and the quantiser's decision points ---------------------------------------------------

EXPF_CHANNELS = 2048
EXPF_PER_CALL = EXPF_CHANNELS * 7          # level 0 of a channel is not exponentiated


def _around(v, n=4):
    """every float within n ulp of v"""
    c = np.float32(v)
    out = [c]
    lo = hi = c
    for _ in range(n):
        lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
        hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
        out += [lo, hi]
    return out


def expf_arguments():
    """EXPF_PER_CALL float32 arguments: the edges first, then a linear grid over [-104, 89.5]"""
    edge = []
    for v in (-103.0, math.log(2.0 ** -126), 88.7228394, 0.0):
        edge += _around(v)
    edge += [np.float32(0.0), np.float32(-0.0), np.float32(SUB), np.float32(-SUB), np.float32(np.inf), np.float32(-np.inf),
             np.float32(np.nan)]
    edge = np.array(edge, np.float32)
    grid = np.linspace(-104.0, 89.5, EXPF_PER_CALL - edge.size).astype(np.float32)
    return torch.from_numpy(np.concatenate([edge, grid]))


def expf_weight():
    """(EXPF_CHANNELS, 8) quantiser weight whose columns 1..7 hold expf_arguments() (column 0 is copied, not
    exponentiated: it holds the arguments too, so that the copy is compared as well)"""
    a = expf_arguments().view(EXPF_CHANNELS, 7)
    return torch.cat([a[:, :1], a], 1).contiguous()


def neighbours(t):
    """t and its two float32 neighbours, as one flat float32 tensor"""
    a = t.detach().cpu().numpy().astype(np.float32).ravel()
    return torch.from_numpy(np.concatenate([a, np.nextafter(a, np.float32(-np.inf)), np.nextafter(a, np.float32(np.inf))]))


def quant_points(cum):
    """inputs at which the quantiser's decision flips, per channel, from the cumulative level table cum (c, 8): each
    level and each midpoint with both float neighbours, below level 0 and above the top level, and the specials.
    Returns (c, n)"""
    rows = []
    for ch in range(cum.shape[0]):
        lv = cum[ch].double()
        mid = ((lv[1:] + lv[:-1]) / 2).float()
        special = torch.tensor([0.0, -0.0, SUB, -SUB, FLT_MAX, -FLT_MAX, float("inf"), -float("inf"), float("nan")])
        below = (lv[0] - (lv[1] - lv[0])).float().view(1)
        above = (lv[-1] + (lv[-1] - lv[-2])).float().view(1)
        rows.append(torch.cat([neighbours(cum[ch]), neighbours(mid), neighbours(below), neighbours(above), special]))
    return torch.stack(rows)


def quant_tensor(points, tn, h, w):
    """(tn, c, h, w) whose channel ch cycles through points[ch], and the (tn, h, w) map of which point sits where"""
    c, n = points.shape
    idx = torch.arange(tn * h * w) % n
    x = points[:, idx].view(c, tn, h, w).permute(1, 0, 2, 3).contiguous()
    return x, idx.view(tn, h, w)


def per_point(t, where, live, n):
    """(c, n): the result t (tn, c, h, w) at the first live position of every point"""
    flat = t.detach().cpu().permute(1, 0, 2, 3).reshape(t.shape[1], -1)
    where, live = where.reshape(-1), live.reshape(-1)
    first = [int(((where == p) & live).nonzero()[0]) for p in range(n)]
    return flat[:, first].contiguous()


# ---- exact power-of-two scaling of the 3x3 kernels -----------------------------------------------------------------

SCALING_SHAPES = [(2, 192, 12, 70, 192), (1, 96, 10, 66, 128), (2, 48, 4, 130, 64)]
SCALINGS = [(-20, -20), (30, -10), (-40, 25)]
# (label, PCONV_CONV3X3, PCONV.WINO_FLAT_REMAINDER): which kernels take a shape under each is conv_plan's answer
SCALING_MODES = [("direct", "direct", True), ("wino", "wino", False), ("wino / flat", "wino", True),
                 ("wino42!", "wino42!", True), ("default", "wino42", True)]


def planned_kernels(P, cfg):
    """the probe names of the launches conv_plan gives a 3x3 stride-1 layer under the current settings"""
    tn, cin, h, w, cout = cfg
    launches, _ = P.conv_plan(cin, h, w, cout, 3, 1)
    return [(kind, P.CONV_KERNELS[kind].probe_name or "conv_mfma_kernel") for kind, _, _ in launches]
