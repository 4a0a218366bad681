"""GPU: the bit-exact kernels at float32's edges -- subnormal inputs, weights, products and results, signed zeros,
overflow to Inf -- where every other GPU test draws unit-scale `randn`.  Compared with `same_bits` (the sign of zero
counts, two NaNs in one place are equal) against the oracle's chains; recipes, shapes and the comparator are in
tests/fp32_edges_cases.py, and tests/test_fp32_edges_cpu.py shows on the CPU that each recipe reaches the edge it is
named for and that the comparator notices a flushed subnormal, a lost sign of zero and a clamped Inf.

  1. direct convolution: conv_small_kernel, the three conv_mfma_kernel tilings for k 1 / 3 x stride 1 / 2,
     conv1x1_rb_kernel, in every regime R1-R6, with and without PReLU; residual, trim, the Dtow store at R1 and R5,
     sigmoid + gate at R1 (2e-6: expf)
  2. fused GDN on every dispatch setting, both directions
  3. the entropy model's three forms on nets whose hidden activations are scaled down to the subnormal range
  4. pconv_expf on the device over its whole range, the cumulative table, the quantiser's decisions at every level
  5. power-of-two scaling commutes with every 3x3 kernel (direct, F(2x2), its flat build, F(4x2), the row split)

When PCONV_TEST_REPORT_DIR is set, the shares of subnormal / zero / Inf entries of every case and whether equality
held are appended to fp32_edges.txt there."""
import os

import numpy as np
import pytest
import torch

import fp32_edges_cases as C
from fp32_edges_cases import same_bits
from oracle import pconv_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W16 = [15., 31., 54., 63., 63., 64., 64., 64., 64., 64., 64., 63., 63., 54., 31., 15.]


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)
    yield


def report(line):
    out = os.environ.get("PCONV_TEST_REPORT_DIR")
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, "fp32_edges.txt"), "a") as f:
                f.write(line + "\n")
        except OSError:
            pass


def check(failures, got, ref, what):
    """same_bits, collected: one run of a test names every case that differs"""
    try:
        same_bits(got, ref, what)
        report("%-100s equal      ref: %s" % (what, C.shares_text(ref)))
    except AssertionError as e:
        failures.append(str(e))
        report("%-100s DIFFERENT  ref: %s" % (what, C.shares_text(ref)))


def probe(P, monkeypatch):
    rec = type("Probe", (), {"records": []})()
    monkeypatch.setattr(P, "conv_probe", rec)
    return rec


def select(monkeypatch, settings, setting):
    for name in ("PCONV_CONV1X1", "PCONV_CONV1X1_WAYOUT", "PCONV_CONV_SMALL"):
        monkeypatch.delenv(name, raising=False)
    for name, value in settings[setting].items():
        monkeypatch.setenv(name, value)


def dev(t):
    return None if t is None else t.to(DEV)


def new_owner():
    """the stand-in for a layer: it caches the packed weight by the weight tensor's address and version, so every
    freshly uploaded weight gets its own (a new tensor may land on the address of one that was just freed)"""
    return type("Owner", (), {})()


# ---- 1. the direct convolution ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", C.CONV_SHAPES, ids=lambda c: "x".join(str(v) for v in c))
def test_direct_conv_every_class_every_regime(cfg, hip_backend, monkeypatch):
    P = hip_backend
    tn, cin, h, w, cout, k, stride, setting = cfg
    monkeypatch.setenv("PCONV_CONV3X3", "direct")
    select(monkeypatch, C.CONV_SETTINGS, setting)
    rec = probe(P, monkeypatch)
    failures = []
    for regime in C.ALL_REGIMES:
        x, wt, b, sl, _ = C.conv_inputs(cfg, regime)
        owner = new_owner()
        for slope in (None, sl):
            ref = O.conv2d_chain(x, wt, b, stride, slope)
            got = P.tile_conv2d(owner, dev(x), dev(wt), dev(b), stride, dev(slope))
            check(failures, got, ref, "conv %s %s prelu=%d" % (cfg, regime, slope is not None))
    names = set(r[0].split("<")[0] for r in rec.records)
    report("conv %s kernel: %s, %d launches" % (cfg, sorted(set(r[0] for r in rec.records)), len(rec.records)))
    assert names == {C.conv_kernel_class(cfg)} and len(rec.records) == 2 * len(C.ALL_REGIMES), names
    assert not failures, "\n".join(failures)


WAYOUT_SHAPES = [(1, 24, 5, 40, 16, 3, 1, "default"), (1, 24, 5, 40, 96, 3, 1, "default"), (1, 32, 3, 40, 192, 1, 1, "default"),
                 (1, 32, 3, 40, 96, 1, 1, "resident")]


@pytest.mark.parametrize("cfg", WAYOUT_SHAPES, ids=lambda c: "x".join(str(v) for v in c))
def test_direct_conv_fused_ways_out(cfg, hip_backend, monkeypatch):
    """residual, trim with column limits, the Dtow store at R1 and R5: the oracle's chain followed by the same
    element-wise operations.  Sigmoid + gate at R1 only, within 2e-6 (expf)"""
    P = hip_backend
    tn, cin, h, w, cout, k, stride, setting = cfg
    monkeypatch.setenv("PCONV_CONV3X3", "direct")
    select(monkeypatch, C.CONV_SETTINGS, setting)
    rec = probe(P, monkeypatch)
    failures = []
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    limit = torch.tensor([wo - 5], dtype=torch.int32)
    for regime in ("R1", "R5"):
        x, wt, b, sl, res = C.conv_inputs(cfg, regime)
        owner = new_owner()
        chain = O.conv2d_chain(x, wt, b, stride, sl)
        got = P.tile_conv2d(owner, dev(x), dev(wt), dev(b), stride, dev(sl), residual=dev(res))
        check(failures, got, res + chain, "conv %s %s residual" % (cfg, regime))
        ref = (res + chain).clone()
        ref[:, :, :, wo - 5:] = 0
        got = P.tile_conv2d(owner, dev(x), dev(wt), dev(b), stride, dev(sl), dev(limit), 1, residual=dev(res), trim=True)
        check(failures, got, ref, "conv %s %s residual + trim" % (cfg, regime))
        ref = chain.clone()
        ref[:, :, :, wo - 5:] = 0
        got = P.tile_conv2d(owner, dev(x), dev(wt), dev(b), stride, dev(sl), dev(limit), 1, trim=True)
        check(failures, got, ref, "conv %s %s trim" % (cfg, regime))
        for ring in (0, 2):
            got = P.tile_conv2d(owner, dev(x), dev(wt), dev(b), stride, dev(sl), d2w=True, ring=ring)
            check(failures, got, O.DtowOp(2, True).forward(chain)[0], "conv %s %s Dtow ring=%d" % (cfg, regime, ring))
    x, wt, b, sl, res = C.conv_inputs(cfg, "R1")
    gate = torch.randn(res.shape, generator=torch.Generator().manual_seed(5))
    got = P.tile_conv2d(new_owner(), dev(x), dev(wt), dev(b), stride, None, None, 0, sigmoid=True, gate=dev(gate)).cpu()
    ref = gate * torch.sigmoid(O.conv2d_chain(x, wt, b, stride, None))
    err = (got - ref).abs().max().item()
    report("conv %s R1 sigmoid + gate: max abs diff %.3g" % (cfg, err))
    assert err < 2e-6, err
    assert set(r[0].split("<")[0] for r in rec.records) == {C.conv_kernel_class(cfg)}
    assert not failures, "\n".join(failures)


# ---- 2. GDN ------------------------------------------------------------------------------------------------------------

def _gdn_shapes():
    from test_gpu_gdn import SHAPES
    smallest = min(SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3])
    return [smallest, (3, 96, 5, 70)]     # ... and one with whole 4-row tiles (resident<1> takes it)


@pytest.mark.parametrize("setting", ["default", "pipe", "batch", "resident"])
@pytest.mark.parametrize("shape", _gdn_shapes(), ids=lambda s: "x".join(str(v) for v in s))
def test_gdn_at_the_edges(shape, setting, hip_backend, monkeypatch):
    from test_gpu_gdn import SETTINGS
    P = hip_backend
    monkeypatch.setenv("PCONV_CONV3X3", "direct")
    select(monkeypatch, SETTINGS, setting)
    rec = probe(P, monkeypatch)
    x, gamma, beta, res = C.gdn_inputs(*shape)
    norm = O.gdn_norm_chain(x, gamma, beta)
    failures, owner = [], type("Owner", (), {})()
    for inverse in (False, True):
        for r in (None, res):
            ref = O.gdn_chain(x, gamma, beta, inverse, r, norm=norm)
            got = P.tile_gdn(owner, dev(x), dev(gamma), dev(beta), inverse, None, 0, dev(r), 0)
            check(failures, got, ref, "gdn %s %s inverse=%d residual=%d" % (shape, setting, inverse, r is not None))
    assert len(rec.records) == 4
    report("gdn %s %s kernels: %s" % (shape, setting, sorted(set(r[0] for r in rec.records))))
    assert not failures, "\n".join(failures)


# ---- 3. the entropy model's three forms -----------------------------------------------------------------------------

def _ent56():
    from test_gpu_entropy_mfma import _ent
    return _ent()


def _ent_wide(vd):
    from test_gpu_wide_models import _ent
    return _ent(vd)


def _oracle_streams(ent, sym, n):
    """the oracle's stream of every frame (one EntEncoder pass per frame on the CPU backend)"""
    import tempfile
    from pseudocylindrical_convolution_amd.PCONV_operator import backend
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from oracle import coder_cpu
    backend.use(O, coder_cpu)
    O.set_detmath(True)
    try:
        torch.manual_seed(0)
        cpu = PC.PseudoEncoder(4 * ent.ngroup, 0).ent
        cpu.load_state_dict({k: v.cpu() for k, v in ent.state_dict().items()})
        out = []
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "s.bin")
            for i in range(n):
                cpu.start(path)
                cpu(sym[16 * i:16 * i + 16].contiguous())
                with open(path, "rb") as f:
                    out.append(f.read())
        return out
    finally:
        backend.reset()


def _three_forms(ent, base, k, h, w, n, seed, monkeypatch, what):
    from pseudocylindrical_convolution_amd.engine import EntropyEngine
    ent.load_state_dict(C.reparametrised(base, k))
    sym_cpu = C.ent_symbols(ent, h, w, n, seed)
    sym = ent.fill(sym_cpu.to(DEV)).contiguous()
    want = _oracle_streams(ent, sym.cpu(), n)
    out, rates, forms = {}, {}, {}
    for mode in ("valu", "mfma"):
        monkeypatch.setenv("PCONV_EE_BULK", mode)
        eng = EntropyEngine(ent, h, w, n, DEV)
        forms[mode] = eng.encoder_forms
        out[mode] = eng.encode(sym)
        bits, pos = eng.rate(sym, rate_map=True)
        rates[mode] = (bits.cpu(), pos.cpu())
        assert torch.equal(eng.decode(out[mode]), sym), "%s: %s streams do not decode to the symbols" % (what, mode)
        del eng
    report("entropy %s forms valu %s mfma %s: valu==mfma %s, valu==oracle %s"
           % (what, sorted(set(forms["valu"])), sorted(set(forms["mfma"])), out["valu"] == out["mfma"], out["valu"] == want))
    assert set(forms["valu"]) == {0} and set(forms["mfma"]) - {0}, forms
    assert out["valu"] == out["mfma"], "%s: vector and matrix-core streams differ" % what
    assert out["valu"] == want, "%s: streams differ from the oracle's" % what
    assert torch.equal(rates["valu"][0], rates["mfma"][0]) and torch.equal(rates["valu"][1], rates["mfma"][1]), what


@pytest.mark.parametrize("k", [C.K_EXACT, C.K_SUB, C.K_SUB + 10])
@pytest.mark.parametrize("h,w,n", C.ENT_SHAPES)
def test_entropy_forms_agree_on_subnormal_activations(h, w, n, k, hip_backend, monkeypatch):
    ent = _ent56()
    base = {name: v.detach().cpu().clone() for name, v in ent.state_dict().items()}
    _three_forms(ent, base, k, h, w, n, 3 + h, monkeypatch, "vd 56 %dx%dx%d k=%d" % (h, w, n, k))


@pytest.mark.parametrize("vd", [112, 192])
def test_wide_entropy_forms_agree_on_subnormal_activations(vd, hip_backend, monkeypatch):
    ent = _ent_wide(vd)
    base = {name: v.detach().cpu().clone() for name, v in ent.state_dict().items()}
    h, w, n = C.ENT_WIDE_SHAPE
    _three_forms(ent, base, C.K_SUB, h, w, n, 100, monkeypatch, "vd %d %dx%dx%d k=%d" % (vd, h, w, n, C.K_SUB))


# ---- 4. pconv_expf on the device, the cumulative table, the quantiser's decisions ------------------------------

def _quant_ops(P, c):
    gctx = P.PseudoContextOp(16, 20, W16, 0, False)
    octx = O.PseudoContextOp(16, 20, W16)
    return (P.PseudoQuantOp(c, 8, 16, 0.9, 100, 2, 0.1, gctx.addr(), 0, False), P.PseudoDQuantOp(16, c, 8, gctx.addr(), 0, False),
            O.PseudoQuantOp(c, 8, 16, 0.9, 100, 2, 0.1, octx.addr()), O.PseudoDQuantOp(16, c, 8, octx.addr()))


def test_device_expf_and_level_tables(hip_backend):
    """quant_levels_kernel evaluates pconv_expf on 14 336 arguments per call: a grid over [-104, 89.5], every float
    within 4 ulp of -103, ln 2^-126, 88.7228394 and 0, +-0, subnormals, +-Inf, NaN -- the oracle library's table
    (the same header compiled for the host) bit for bit; dquant_levels_kernel's running sums likewise"""
    P = hip_backend
    c = C.EXPF_CHANNELS
    weight = C.expf_weight()
    gq, gd, oq, od = _quant_ops(P, c)
    x = torch.zeros(16, c, 1, 4)
    with torch.no_grad():
        gq.forward(dev(x), dev(weight), dev(torch.zeros(c, 8)), False)
        oq.forward(x, weight, torch.zeros(c, 8), False)
        gd.forward(dev(x), dev(weight))
        od.forward(x, weight)
    failures = []
    tab = gq._top["tab"].cpu()
    ref = oq.level_table()
    check(failures, tab, ref, "expf table (%d arguments)" % C.EXPF_PER_CALL)
    args = C.expf_arguments()
    sub = (args >= -103.0) & (args < float(np.log(2.0 ** -126)))
    assert int(C.is_subnormal(ref[:, 1:].reshape(-1)[sub]).sum()) > 0.9 * int(sub.sum()) > 500   # the subnormal-result range is there
    check(failures, gd._top["tab"].cpu(), od.level_table(), "cumulative table")
    assert not failures, "\n".join(failures)


def test_quantiser_decisions_at_every_level(hip_backend):
    """inputs on each cumulative level, on each midpoint between two levels, beside them, outside the table and at the
    specials, built from the DEVICE's table: values, indices and de-quantised values equal the oracle's in the 16-byte
    form (w = 64) and in the scalar form (w = 66), and the two forms give every point the same answer.  Every index is
    inside the alphabet (asserted on the oracle's) before it goes to the de-quantiser"""
    P = hip_backend
    c, tn, h = 6, 16, 2
    weight = torch.zeros(c, 8)
    weight[:, 0] = 1. / 9
    weight[:, 1:] = float(np.log(1. / 9))
    weight += torch.randn(c, 8, generator=torch.Generator().manual_seed(22)) * 0.2
    failures, forms = [], {}
    for width in (64, 66):
        gq, gd, oq, od = _quant_ops(P, c)
        with torch.no_grad():
            gd.forward(dev(torch.zeros(tn, c, h, width)), dev(weight))
            points = C.quant_points(gd._top["tab"].cpu().clone())
            n = points.shape[1]
            x, where = C.quant_tensor(points, tn, h, width)
            live = torch.zeros(tn, h, width, dtype=torch.bool)
            for t, lim in enumerate(O.widths_v3(W16, 16, 16 * h, width)):
                live[t, :, :int(lim)] = True
            assert len(set(where[live].tolist())) == n, "some decision points fell into dead columns only"
            gv, gi = gq.forward(dev(x), dev(weight), dev(torch.zeros(c, 8)), False)
            cv, ci = oq.forward(x, weight, torch.zeros(c, 8), False)
            assert float(gq.count_data_.abs().sum()) == 0.0      # (no histogram: the 16-byte form where w % 4 == 0)
            assert ci.min() >= 0 and ci.max() <= 7 and set(ci.unique().tolist()) == set(float(v) for v in range(8))
            check(failures, gi, ci, "quantiser indices w=%d" % width)
            check(failures, gv, cv, "quantiser values w=%d" % width)
            gdq = gd.forward(dev(ci), dev(weight))[0]
            check(failures, gdq, od.forward(ci, weight)[0], "de-quantised values w=%d" % width)
            forms[width] = [points] + [C.per_point(t, where, live, n) for t in (gv, gi, gdq)]
    for a, b, what in zip(forms[64], forms[66], ("decision points", "values", "indices", "de-quantised values")):
        check(failures, a, b, "16-byte form vs scalar form: %s" % what)
    assert not failures, "\n".join(failures)


# ---- 5. exact power-of-two scaling of every 3x3 kernel -------------------------------------------------------------

@pytest.mark.parametrize("cfg", C.SCALING_SHAPES, ids=lambda c: "x".join(str(v) for v in c))
def test_power_of_two_scaling_commutes_with_every_3x3_kernel(cfg, hip_backend, monkeypatch):
    """conv(x 2^a, w 2^b, bias 2^(a+b)) == conv(x, w, bias) 2^(a+b) bit for bit while everything stays normal: no hidden
    absolute constant, clamp or early underflow in any transform (Winograd's 1/6 and 1/24 scale with their operands)"""
    P = hip_backend
    tn, cin, h, w, cout = cfg
    g = torch.Generator().manual_seed(55)
    x = torch.randn(tn, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / np.sqrt(cin * 9))
    b = torch.randn(cout, generator=g)
    sl = C.slopes(cout, g)
    sl[1] = 0.25          # (a subnormal slope would leave the normal range)
    ho, wo = h - 2, w - 2
    res = torch.randn(tn, cout, ho, wo, generator=g)
    limit = torch.tensor([wo, 40, 64, 3, 65, 128, wo - 1, 1] * 2, dtype=torch.int32).clamp(max=wo)
    rec = probe(P, monkeypatch)
    failures, kernels = [], {}
    for label, mode, flat in C.SCALING_MODES:
        monkeypatch.setenv("PCONV_CONV3X3", mode)
        monkeypatch.setattr(P, "WINO_FLAT_REMAINDER", flat)
        planned = [name for _, name in C.planned_kernels(P, cfg)]

        def run(a, e):
            owner = new_owner()
            xs, ws, bs, rs = (dev(C.scaled(x, a)), dev(C.scaled(wt, e)), dev(C.scaled(b, a + e)), dev(C.scaled(res, a + e)))
            plain = P.tile_conv2d(owner, xs, ws, bs, 1, dev(sl)).cpu()
            fused = P.tile_conv2d(owner, xs, ws, bs, 1, dev(sl), dev(limit), 16, residual=rs, trim=True).cpu()
            return plain, fused

        rec.records.clear()
        base = run(0, 0)
        kernels[label] = [r[0].split("<")[0] for r in rec.records]
        assert kernels[label] == planned * 2, (label, kernels[label], planned)
        for (a, e) in C.SCALINGS:
            got = run(a, e)
            for y, y0, what in zip(got, base, ("PReLU", "PReLU + residual + trim")):
                assert torch.isfinite(y0).all() and not bool(C.is_subnormal(C.scaled(y0, a + e)).any())
                check(failures, y, C.scaled(y0, a + e), "scaling %s %s (%d, %d) %s" % (cfg, label, a, e, what))
    report("scaling %s kernels: %s" % (cfg, kernels))
    assert not failures, "\n".join(failures)
