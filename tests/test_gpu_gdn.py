"""The fused GDN (pconv_gdn) and the ragged / per-branch 1x1 convolutions against a bit-exact CPU restatement.

`O.gdn_chain` evaluates the GDN in float32 exactly as the numerics contract states it: the norm is the k-ascending
fmaf chain over the squares (x * x rounded on its own) with beta added last, then sqrt, divide (inverse: multiply),
+ residual, zeros from the tile's limit on -- each of them one correctly rounded operation of the oracle's C library.
(Not torch's: its float32 CPU sqrt is not always correctly rounded -- 0.7 % of random square roots were one ulp off
on one host, and against it 13 % of the first case's outputs differed from the kernel's by one ulp on another.)
The kernels are built with -ffp-contract=off -fno-fast-math, sqrtf and
`/` lower to correctly rounded sequences, so every dispatch branch of pconv_gdn must give the SAME BITS; tests
between kernel variants (test_gpu_ops.py) cannot see a mistake the variants share.  tests/test_gdn_ref_cpu.py holds
gdn_chain itself to a float64 evaluation and to the module's formula.

Which case reaches which branch of pconv_gdn (csrc/conv.hip), by setting
(default | PCONV_CONV1X1_WAYOUT=pipe | PCONV_CONV1X1_WAYOUT=batch | PCONV_CONV1X1=resident):

  branch of pconv_gdn                          reached by
  -------------------------------------------  ----------------------------------------------------------------
   1 resident<2>, residual                     resident: 19x192x3x134, 1x192x1x7, with a residual
   2 resident<2>, no residual                  resident: the same shapes, no residual
   3 resident<1>, residual                     resident: 3x96x5x70, 2x80x5x70 (cout guard), with a residual
   4 resident<1>, no residual                  resident: the same shapes, no residual
   5 quads (WAY 4), ch > 96, residual          default: 19x192x3x134 (full column tiles; the 6-column tile and
                                               1x192x1x7 / 1x192x2x3 leave by the element-wise fallback inside
                                               it); resident: 1x192x2x3 (w < 4: the resident form declines)
   6 quads (WAY 3), ch > 96, no residual       the same, no residual
   7 pipelined (WAY 2), ch > 96, residual      pipe: the three 192-channel shapes, with a residual
   8 pipelined (WAY 1), ch > 96, no residual   pipe: the same, no residual
   9 conv_epilogue, ch > 96                    batch: the three 192-channel shapes
  10 conv_epilogue, ch 33..96 (4-row tiles)    default / pipe / batch: 3x96x5x70, 2x80x5x70; every setting:
                                               2x40x3x70 (40 % 16 != 0: not resident-eligible, ragged last chunk)
  11 conv_epilogue, ch <= 32                   every setting: 2x24x3x70 (ragged last chunk)

1x1 branches of pconv_conv2d reached by test_conv1x1_* below (cases are tn, cin, h, w, cout, k, stride):

  resident 1x1 <2 | 1>, residual | none        resident: 3x192x3x134 -> 192, 3x96x5x70 -> 96, epilogue | plain call
  quads stride 1, cout > 96, res | none        default: cin 3, 100, 192 -> 192
  quads stride 1, cout 33..96, res | none      default: 20 -> 96, 96 -> 96, 200 -> 40 (cout guard: fallback inside)
  pipelined stride 1, residual: cout > 96      pipe: 192 -> 192, epilogue call
                               cout 33..96     pipe: 96 -> 96, epilogue call
                               cout <= 32      default: 20 -> 24, epilogue call
  conv_epilogue stride 1 (BY_TILE)             batch: 192 -> 192, 96 -> 96; pipe: their plain calls; default: 20 -> 24
                                               plain call
  quads stride 2, cout > 96, res | none        default: 3 -> 192 stride 2
  quads stride 2, cout 33..96, res | none      default: 20 -> 96 stride 2
  conv_epilogue stride 2, cout <= 32           default: 100 -> 24 stride 2
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import pconv_cpu as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")

# workgroup tile: 64 columns x 2 rows (ch > 96 or ch <= 32), x 4 rows (ch 33..96)
SHAPES = [
    (19, 192, 3, 134),  # two full column tiles + a 6-column one; a full row tile + one over the lower edge; t % npart wraps
    (3, 96, 5, 70),     # 4-row tiles; ch <= 96 generic and resident<1>
    (2, 80, 5, 70),     # cout guard inside a 96 block; resident-eligible (80 % 16 == 0)
    (2, 40, 3, 70),     # ragged last input chunk, ch > 32
    (2, 24, 3, 70),     # ch <= 32 tile, ragged chunk
    (1, 192, 1, 7),     # no full tile anywhere
    (1, 192, 2, 3),     # w < 4: the resident form must decline
]
# trims inside a full tile, on a tile boundary, one before and one after it, dead tiles (0 and 1), inside the ragged tile
LIMITS = [134, 128, 129, 127, 64, 65, 63, 1, 0, 33, 134, 100, 130, 6, 70, 134]
# With fewer than 16 tiles only the head of the pattern is used, and clamped to a narrow w its head is all `w`: such
# shapes ALSO run the pattern rotated, so that tiles 0.. meet 64 / 65 / 63, 1 / 0 / 33 and 6 as well
ROLLS = {19: (0,), 3: (0, 4, 7, 13), 2: (0, 4, 6, 8, 13), 1: (0, 7, 8, 13)}
KINDS = ("1", "1e-3", "1e3", "hard")
SETTINGS = {"default": {}, "pipe": {"PCONV_CONV1X1_WAYOUT": "pipe"}, "batch": {"PCONV_CONV1X1_WAYOUT": "batch"},
            "resident": {"PCONV_CONV1X1": "resident"}}


@pytest.fixture(autouse=True)
def _direct_conv(monkeypatch):
    """the direct tile convolution, as in test_gpu_ops.py (only the 3x3 stride-1 layers have another form)"""
    monkeypatch.setenv("PCONV_CONV3X3", "direct")


def P():
    from pseudocylindrical_convolution_amd import PCONV
    return PCONV


def select(monkeypatch, setting):
    """the library reads its options at every call"""
    for name in ("PCONV_CONV1X1", "PCONV_CONV1X1_WAYOUT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in SETTINGS[setting].items():
        monkeypatch.setenv(name, value)


def limit_sets(tn, w):
    base = torch.tensor(LIMITS, dtype=torch.int32).clamp(max=w)
    return [torch.roll(base, -r) for r in ROLLS[tn]]


def inside(t, p, fill=NAN):
    """t as the interior view of a padded GPU buffer filled with `fill`"""
    buf = torch.full((t.shape[0], t.shape[1], t.shape[2] + 2 * p, t.shape[3] + 2 * p), fill, device=DEV)
    buf[:, :, p:-p, p:-p] = t.to(DEV)
    return buf[:, :, p:-p, p:-p]


def same(got_gpu, ref, what):
    got = got_gpu.detach().cpu()
    assert got.shape == ref.shape, what
    if not torch.equal(got, ref):
        bad = (got != ref) | torch.isnan(got)
        where = bad.nonzero()[0].tolist()
        diff = (got - ref)[bad & torch.isfinite(got)].abs()
        raise AssertionError("%s: %d of %d elements differ, first at %s (got %r, expected %r), max abs diff %g"
                             % (what, int(bad.sum()), bad.numel(), where, got[tuple(where)].item(),
                                ref[tuple(where)].item(), diff.max().item() if diff.numel() else NAN))


def draw(tn, ch, h, w, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tn, ch, h, w, generator=g) * (1.0 if kind == "hard" else float(kind))
    gamma = 0.01 * torch.rand(ch, ch, generator=g) + 0.1 * torch.eye(ch)
    beta = torch.rand(ch, generator=g) + 0.5
    res = torch.randn(tn, ch, h, w, generator=g)
    if kind == "hard":
        # gamma entries up to 1, several all-zero rows with beta at the module's beta_min on those channels (the norm
        # is exactly beta), x exactly 0 at a seeded 5 % of the positions
        gamma = torch.rand(ch, ch, generator=g)
        dead = torch.arange(ch) % 7 == 3
        gamma[dead] = 0
        beta[dead] = 1e-6
        x[torch.rand(x.shape, generator=g) < 0.05] = 0
    return x, gamma, beta, res


class Case(object):
    """one shape with one input set: tensors on both sides, the norm chain once, every reference variant once"""

    def __init__(self, si, kind):
        tn, ch, h, w = SHAPES[si]
        self.x, self.gamma, self.beta, self.res = draw(tn, ch, h, w, kind, seed=100 + si)
        self.norm = O.gdn_norm_chain(self.x, self.gamma, self.beta)
        self.limits = limit_sets(tn, w)
        self.gx, self.ggamma, self.gbeta = self.x.to(DEV), self.gamma.to(DEV), self.beta.to(DEV)
        self.gres, self.gres_view = self.res.to(DEV), inside(self.res, 1)
        self.glimits = [l.to(DEV) for l in self.limits]
        self.owner = type("Owner", (), {})()   # (holds the packed gamma: one per case, its tensors stay alive)
        self.refs = {}

    def ref(self, inverse, has_res, li):
        key = (inverse, has_res, li)
        if key not in self.refs:
            self.refs[key] = O.gdn_chain(self.x, self.gamma, self.beta, inverse, self.res if has_res else None,
                                         None if li is None else self.limits[li], 0 if li is None else 16, norm=self.norm)
        return self.refs[key]


_CASE = {}


def case(si, kind):
    """the tests run shape by shape, input set by input set: one case is kept at a time"""
    if (si, kind) not in _CASE:
        _CASE.clear()
        _CASE[(si, kind)] = Case(si, kind)
    return _CASE[(si, kind)]


def _id(si):
    return "x".join(str(v) for v in SHAPES[si])


@pytest.mark.parametrize("si,kind,setting", [(si, kind, s) for si in range(len(SHAPES)) for kind in KINDS for s in SETTINGS],
                         ids=lambda v: _id(v) if isinstance(v, int) else str(v))
def test_gdn_bit_exact_on_every_branch(si, kind, setting, monkeypatch):
    """tile_gdn equals O.gdn_chain bit for bit: forward and inverse, without / with a dense residual / with a residual
    inside a NaN-filled padded buffer, dense and ring-buffer outputs, without limits and with every limit set"""
    c = case(si, kind)
    select(monkeypatch, setting)
    tn, ch, h, w = SHAPES[si]
    for inverse, li, has_res in itertools.product((False, True), [None] + list(range(len(c.limits))), (False, True)):
        ref = c.ref(inverse, has_res, li)
        limit, npart = (None, 0) if li is None else (c.glimits[li], 16)
        for res, ring in itertools.product((c.gres, c.gres_view) if has_res else (None,), (0, 2)):
            y = P().tile_gdn(c.owner, c.gx, c.ggamma, c.gbeta, inverse, limit, npart, res, ring)
            if ring:
                assert y._pconv_ring[1] == ring and not y.is_contiguous()
            same(y, ref, "%s %s %s inverse=%d limits=%s residual=%s ring=%d"
                 % (_id(si), kind, setting, inverse, None if li is None else c.limits[li].tolist()[:tn],
                    "none" if res is None else ("dense" if res is c.gres else "view"), ring))
    if kind == "hard":
        dead = torch.arange(ch) % 7 == 3
        plain = c.ref(False, False, None)
        # (float64 sqrt rounded to float32 is the correctly rounded float32 sqrt; torch's float32 CPU sqrt is not always)
        root = torch.sqrt(c.beta[dead].double()).float().view(1, -1, 1, 1)
        assert torch.equal(plain[:, dead], c.x[:, dead] / root)
        assert (plain[c.x == 0] == 0).all()


@pytest.mark.parametrize("si,setting", [(si, s) for si in range(len(SHAPES)) for s in SETTINGS],
                         ids=lambda v: _id(v) if isinstance(v, int) else str(v))
def test_gdn_reads_nothing_it_may_not(si, setting, monkeypatch):
    """NaN wherever the kernel may not look: around the input (interior view of a padded buffer, then the channel
    slice of a tensor with eight more channels), and from each tile's limit on in input and residual.  The output
    is finite everywhere, exactly 0 from the limit on, and equals the reference in the live columns"""
    c = case(si, "1")
    select(monkeypatch, setting)
    tn, ch, h, w = SHAPES[si]
    for li, lim in enumerate(c.limits):
        dead = torch.zeros(tn, 1, 1, w, dtype=torch.bool)
        for t in range(tn):
            dead[t, :, :, int(lim[t % 16]):] = True
        x = torch.where(dead, torch.tensor(NAN), c.x)
        res = torch.where(dead, torch.tensor(NAN), c.res)
        big = torch.full((tn, ch + 8, h, w), NAN, device=DEV)
        big[:, :ch] = x.to(DEV)
        for inverse, (xin, rin) in itertools.product((False, True), ((inside(x, 2), inside(res, 1)),
                                                                     (big[:, :ch], res.to(DEV)))):
            got = P().tile_gdn(c.owner, xin, c.ggamma, c.gbeta, inverse, c.glimits[li], 16, rin, 0).cpu()
            ref = c.ref(inverse, True, li)
            what = "%s %s inverse=%d limits=%s" % (_id(si), setting, inverse, lim.tolist()[:tn])
            assert torch.isfinite(got).all(), what
            assert (got[dead.expand_as(got)] == 0).all(), what
            same(got, ref, what)


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_module_follows_its_parameters(hip_backend, inverse):
    """PseudoGDNV2 under no_grad (the fused launch, residual, the context's limits, a ring-buffer output) against
    gdn_chain on the module's effective parameters, recomputed here from the raw ones.  The packed gamma slab and
    effective() are cached on parameter versions and data pointers: after each of three in-place updates, a
    load_state_dict, and a write through .data followed by backend.invalidate_derived(), the result is the
    reference for the NEW parameters and differs from the one before"""
    from pseudocylindrical_convolution_amd.PCONV_operator import PseudoContextV2, PseudoGDNV2, backend
    torch.manual_seed(3)
    ctx = PseudoContextV2(16, True, device=0)
    gdn = PseudoGDNV2(192, 16, ctx, 0, inverse=inverse)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(16, 192, 4, 128, generator=g)
    res = torch.randn(16, 192, 4, 128, generator=g)
    xg, rg = x.to(DEV), res.to(DEV)
    ctx.setup_context(128)
    limit = ctx.produce_fill_param(0, 4, 128).cpu().to(torch.int32)
    assert limit.numel() == 16 and int(limit.min()) < 128 <= int(limit.max())

    def expected():
        # LowerBound.forward and the re-parametrisation of PseudoGDNV2.effective, on the CPU
        ped = gdn.pedestal.cpu()
        beta = torch.max(gdn.beta.detach().cpu(), torch.ones(192) * gdn.beta_bound) ** 2 - ped
        gamma = torch.max(gdn.gamma.detach().cpu(), torch.ones(192, 192) * gdn.gamma_bound) ** 2 - ped
        return O.gdn_chain(x, gamma, beta, inverse, res, limit, 16), gamma, beta

    def run(what, before):
        with torch.no_grad():
            y = gdn(xg, rg, gdn.trim, ring=2)
        assert y._pconv_ring[1] == 2
        ref, gamma, beta = expected()
        eg, eb = gdn.effective()
        assert torch.equal(eg.cpu(), gamma) and torch.equal(eb.cpu(), beta), what
        same(y, ref, what)
        if before is not None:
            assert not torch.equal(y.cpu(), before), "%s: the result did not change" % what
        return y.cpu()

    y = run("initial parameters", None)
    for i in range(3):
        with torch.no_grad():
            gdn.gamma.add_(torch.rand(192, 192, generator=g).to(DEV) * 0.02)
            gdn.beta.add_(torch.rand(192, generator=g).to(DEV) * 0.1)
        y = run("in-place update %d" % (i + 1), y)
    state = {k: v.clone() for k, v in gdn.state_dict().items()}
    state["gamma"] += torch.rand(192, 192, generator=g).to(DEV) * 0.02
    state["beta"] += 0.05
    gdn.load_state_dict(state)
    y = run("load_state_dict", y)
    gdn.gamma.data.mul_(1.25)
    gdn.beta.data.add_(0.125)
    backend.invalidate_derived()
    run(".data write + invalidate_derived", y)


# ---- 1x1 convolutions: ragged cin, every way out, against the fmaf chain -----------------------------------------------

CONV_CASES = [
    # tn, cin, h, w, cout, k, stride
    (2, 3, 5, 70, 192, 1, 1), (2, 20, 5, 70, 96, 1, 1), (2, 100, 3, 70, 192, 1, 1), (1, 200, 3, 70, 40, 1, 1),
    (2, 3, 9, 139, 192, 1, 2), (2, 20, 9, 139, 96, 1, 2), (2, 100, 5, 139, 24, 1, 2),
    (2, 20, 3, 70, 24, 1, 1),   # (the 32-cout tile of the stride-1 layers: pipelined with a residual, generic without)
]
WAYOUT_CASES = [(3, 192, 3, 134, 192, 1, 1), (3, 96, 5, 70, 96, 1, 1)]

_CONV = {}


def conv_case(cfg):
    """inputs and chain references of one layer, once for all settings"""
    if cfg not in _CONV:
        tn, cin, h, w, cout, k, stride = cfg
        g = torch.Generator().manual_seed(131)
        x = torch.randn(tn, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / np.sqrt(cin * k * k))
        b = torch.randn(cout, generator=g)
        sl = torch.rand(cout, generator=g)
        ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
        res = torch.randn(tn, cout, ho, wo, generator=g)
        limits = limit_sets(tn, wo)
        act = res + O.conv2d_chain(x, wt, b, stride, sl)
        trimmed = []
        for lim in limits:
            r = act.clone()
            for t in range(tn):
                r[t, :, :, int(lim[t % 16]):] = 0
            trimmed.append(r)
        _CONV[cfg] = dict(x=x, wt=wt, b=b, sl=sl, res=res, limits=limits, trimmed=trimmed,
                          plain=O.conv2d_chain(x, wt, None, stride, None), owner=type("Owner", (), {})(),
                          gpu=[t.to(DEV) for t in (x, wt, b, sl, res)])
    return _CONV[cfg]


def run_conv_case(cfg, tag):
    c = conv_case(cfg)
    stride = cfg[6]
    xg, wg, bg, sg, rg = c["gpu"]
    for lim, ref in zip(c["limits"], c["trimmed"]):
        what = "%s %s limits=%s" % (cfg, tag, lim.tolist()[:cfg[0]])
        # PReLU + residual + trim, dense ...
        y = P().tile_conv2d(c["owner"], xg, wg, bg, stride, sg, lim.to(DEV), 16, residual=rg, trim=True)
        same(y, ref, what + " dense")
        # ... and on views: input and residual inside NaN-filled padded buffers, the output into a ring buffer
        y = P().tile_conv2d(c["owner"], inside(c["x"], 2), wg, bg, stride, sg, lim.to(DEV), 16,
                            residual=inside(c["res"], 1), trim=True, ring=2)
        assert not y.is_contiguous() and y._pconv_ring[1] == 2
        same(y, ref, what + " views")
    # plain: no bias, no epilogue
    same(P().tile_conv2d(c["owner"], xg, wg, None, stride, None), c["plain"], "%s %s plain" % (cfg, tag))


@pytest.mark.parametrize("cfg", CONV_CASES)
def test_conv1x1_ragged_cin_bit_exact_vs_fmaf_chain(cfg):
    """1x1 layers whose cin is no multiple of the 16-channel LDS stage (the stager re-reads the last real channel
    against zero weight rows), stride 1 and 2, every cout tile: the oracle's fmaf chain, then PReLU, + residual and
    trim as the same element-wise operations -- bit for bit"""
    run_conv_case(cfg, "default")


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("cfg", WAYOUT_CASES)
def test_conv1x1_every_way_out_bit_exact_vs_fmaf_chain(cfg, setting, monkeypatch):
    """each way out of the 1x1 layers (quads, pipelined, batches, the weight-resident kernel) against the chain WITH
    an epilogue (PReLU + residual + trim), not only against its siblings"""
    select(monkeypatch, setting)
    run_conv_case(cfg, setting)
