"""CPU: the recipes and the comparator of tests/fp32_edges_cases.py, on the oracle alone.

  * same_bits has teeth: against the oracle's own output it rejects a copy with every subnormal flushed to +0, a copy
    with one -0 turned into +0 and a copy with one Inf clamped to FLT_MAX; it accepts NaN against NaN.
  * every regime reaches, on every shape the GPU test runs, the edge it is named for (the oracle keeps subnormals on the
    CPU: torch.set_flush_denormal is off, and nothing here turns it on).
  * the entropy net's re-parametrisation by 2^-k is exact at k = 40 (the oracle's streams equal the unscaled net's byte
    for byte), still exact at K_SUB - 5, and at K_SUB the streams differ: hidden activations have become subnormal.
  * the expf sweep holds what the issue lists, the quantiser's decision points hit every level, and the five modes of
    the scaling test reach every 3x3 kernel."""
import math

import numpy as np
import pytest
import torch

import fp32_edges_cases as C
from oracle import pconv_cpu as O


def _chain(cfg, regime, slope=False):
    x, wt, b, sl, _ = C.conv_inputs(cfg, regime)
    return O.conv2d_chain(x, wt, b, cfg[6], sl if slope else None), (x, wt, b)


def test_comparator_has_teeth():
    cfg = C.CONV_SHAPES[0]
    r1, _ = _chain(cfg, "R1")
    C.same_bits(r1, r1.clone(), "identical")
    with pytest.raises(AssertionError, match="subnormal on either side"):
        C.same_bits(C.flushed(r1), r1, "every subnormal flushed")
    assert int(C.differing(C.flushed(r1), r1).sum()) == int(C.is_subnormal(r1).sum()) > 0.95 * r1.numel()
    # a -0 among the oracle's outputs: R4 leaves products that underflow to -0 in front of a zero bias
    r4, _ = _chain(cfg, "R4")
    neg0 = ((r4 == 0) & (r4.view(torch.int32) < 0)).nonzero()
    assert len(neg0), "R4 has no -0 on this shape"
    one = r4.clone()
    one[tuple(neg0[0].tolist())] = 0.0
    assert torch.equal(one, r4)                       # torch.equal calls them equal ...
    with pytest.raises(AssertionError, match="1 of %d entries differ" % r4.numel()):
        C.same_bits(one, r4, "one -0 lost")           # ... the comparator does not
    r5, _ = _chain(cfg, "R5")
    inf = torch.isinf(r5).nonzero()
    one = r5.clone()
    first = tuple(inf[0].tolist())
    one[first] = math.copysign(C.FLT_MAX, r5[first].item())
    with pytest.raises(AssertionError, match="non-finite 1"):
        C.same_bits(one, r5, "one Inf clamped")
    # NaN equals NaN whatever the payload, and nothing else
    a = torch.tensor([float("nan"), 1.0])
    b = a.clone()
    b.view(torch.int32)[0] |= 0x1234
    C.same_bits(a, b, "payloads")
    with pytest.raises(AssertionError):
        C.same_bits(a, torch.tensor([0.0, 1.0]), "NaN against a number")


def test_nothing_flushes_on_this_host():
    assert C.is_subnormal(torch.tensor([C.SUB]))[0] and float(torch.tensor([C.SUB]) * 0.5) == C.SUB / 2
    x, sq = torch.tensor([2.0 ** -70]), torch.empty(1)
    O.lib().orc_square(O._p(x), O._p(sq), O.L(1))
    assert float(sq) == 2.0 ** -140


@pytest.mark.parametrize("cfg", C.CONV_SHAPES, ids=lambda c: "x".join(str(v) for v in c))
def test_regimes_reach_their_edges_on_every_shape(cfg):
    assert C.conv_kernel_class(cfg) in ("conv_small_kernel", "conv_mfma_kernel", "conv1x1_rb_kernel")
    for regime in C.ALL_REGIMES:
        out, (x, wt, b) = _chain(cfg, regime)
        missing = C.regime_condition(regime.split(":")[0], out, x, wt, b, cfg[6])
        assert missing is None, "%s %s: %s (%s)" % (cfg, regime, missing, C.shares_text(out))
    x, wt, b, sl, res = C.conv_inputs(cfg, "R2")
    assert C.shares(wt)["sub"] >= 0.95
    assert C.shares(C.conv_inputs(cfg, "R3")[0])["sub"] >= 0.6
    assert sl[0] == 0 and C.is_subnormal(sl[1:2])[0] and sl[2] < 0 and sl[3] == 1
    # the residuals of the fused ways out live at the outputs' scale
    assert C.shares(C.conv_inputs(cfg, "R1")[4])["sub"] >= 0.95 and C.shares(C.conv_inputs(cfg, "R5")[4])["inf"] > 0


def test_conv_shapes_cover_every_kernel_class(monkeypatch):
    """conv_kernel_name's answer for every shape, under the setting the GPU test runs it with"""
    from pseudocylindrical_convolution_amd import PCONV
    seen = set()
    for cfg in C.CONV_SHAPES:
        tn, cin, h, w, cout, k, stride, setting = cfg
        monkeypatch.delenv("PCONV_CONV1X1", raising=False)
        monkeypatch.delenv("PCONV_CONV_SMALL", raising=False)
        for name, value in C.CONV_SETTINGS[setting].items():
            monkeypatch.setenv(name, value)
        name = PCONV.conv_kernel_name(cout, k, stride, cin=cin, pixels=tn * h * w)
        assert name.split("<")[0] == C.conv_kernel_class(cfg), (cfg, name)
        seen.add(name)
    assert len(seen) == 1 + 12 + 2, sorted(seen)


def test_gdn_inputs_reach_their_edges():
    from test_gpu_gdn import SHAPES
    for shape in (min(SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3]), (3, 96, 5, 70)):
        x, gamma, beta, res = C.gdn_inputs(*shape)
        sq = x * x
        assert bool((sq[:, 0::3] == 0).all()) and C.shares(sq[:, 5::6])["sub"] > 0.95
        assert bool((x[:, 1] == 0).all()) and 0 < C.shares(x[:, 1])["neg0"] < 1
        assert C.shares(sq[:, 2, :, 0::2])["inf"] > 0.9 and bool(torch.isfinite(sq[:, 2, :, 1::2]).all())
        assert float(beta.min()) == np.float32(C.GDN_BETA_MIN)
        fwd = O.gdn_chain(x, gamma, beta, False)
        inv = O.gdn_chain(x, gamma, beta, True)
        assert C.shares(fwd)["neg0"] > 0.05 and C.shares(inv)["inf"] > 0.05 and C.shares(inv)["nan"] > 0
        # channels at beta_min see the tiny channels only: in the columns without the overflow their norm is beta_min
        # itself (the subnormal products vanish under it); in the others 0 * Inf makes it NaN
        norm = O.gdn_norm_chain(x, gamma, beta)
        assert bool((norm[:, 0::4, :, 1::2] == np.float32(C.GDN_BETA_MIN)).all())
        assert bool(torch.isnan(norm[:, 0::4, :, 0::2])[torch.isinf(sq[:, 2:3, :, 0::2]).expand_as(norm[:, 0::4, :, 0::2])].all())


# ---- the entropy net's re-parametrisation ---------------------------------------------------------------------------

def _streams(ent, sym, n, tmp_path):
    out = []
    path = str(tmp_path / "s.bin")
    for i in range(n):
        ent.start(path)
        ent(sym[16 * i:16 * i + 16].contiguous())
        with open(path, "rb") as f:
            out.append(f.read())
    return out


def test_reparametrisation_is_exact_until_activations_go_subnormal(oracle_backend, tmp_path):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    torch.manual_seed(1234)
    ent = PC.PseudoEncoder(56, 0).ent
    g = torch.Generator().manual_seed(7)
    base = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in ent.state_dict().items()}   # test_gpu_entropy_mfma._ent
    h, w, n = C.ENT_SHAPES[0]
    ent.load_state_dict(base)
    sym = ent.fill(C.ent_symbols(ent, h, w, n, 3 + h)).contiguous()
    plain = _streams(ent, sym, n, tmp_path)
    assert all(len(s) > 1000 for s in plain)
    got = {}
    for k in (C.K_EXACT, C.K_SUB - 5, C.K_SUB):
        scaled = C.reparametrised(base, k)
        assert torch.equal(scaled["net.6.conv.bias"], base["net.6.conv.bias"])
        assert torch.equal(scaled["net.0.conv.weight"].double() * 2.0 ** k, base["net.0.conv.weight"].double())
        ent.load_state_dict(scaled)
        got[k] = _streams(ent, sym, n, tmp_path)
    assert got[C.K_EXACT] == plain, "the re-parametrisation at k = %d is not exact" % C.K_EXACT
    assert got[C.K_SUB - 5] == plain, "k_sub is smaller than %d" % C.K_SUB
    assert got[C.K_SUB] != plain, "k_sub is larger than %d" % C.K_SUB
    assert C.K_SUB % 5 == 0 and C.K_SUB > C.K_EXACT


# ---- expf arguments, decision points, the scaling test's modes --------------------------------------------------

def test_expf_sweep_holds_what_it_should():
    a = C.expf_arguments()
    assert a.numel() == C.EXPF_PER_CALL and tuple(C.expf_weight().shape) == (C.EXPF_CHANNELS, 8)
    v = a.numpy()
    for centre in (-103.0, math.log(2.0 ** -126), 88.7228394, 0.0):
        c = np.float32(centre)
        lo = hi = c
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            assert lo in v and hi in v
        assert c in v
    bits = set(a.view(torch.int32).tolist())
    assert 0 in bits and -2 ** 31 in bits                                   # +0 and -0
    assert bool(C.is_subnormal(a).any()) and float("inf") in v and -float("inf") in v and bool(np.isnan(v).any())
    assert v[np.isfinite(v)].min() == -104.0 and v[np.isfinite(v)].max() == 89.5
    # the oracle's table over the sweep: the subnormal-result range is populated, overflow gives Inf, NaN stays NaN
    O.set_detmath(True)
    octx = O.PseudoContextOp(16, 20, [15., 31., 54., 63., 63., 64., 64., 64., 64., 64., 64., 63., 63., 54., 31., 15.])
    oq = O.PseudoQuantOp(C.EXPF_CHANNELS, 8, 16, 0.9, 100, 2, 0.1, octx.addr())
    oq.forward(torch.zeros(16, C.EXPF_CHANNELS, 1, 4), C.expf_weight(), torch.zeros(C.EXPF_CHANNELS, 8), False)
    e = oq.level_table()[:, 1:].reshape(-1)
    assert int(C.is_subnormal(e).sum()) > 1000 and int(torch.isinf(e).sum()) > 10 and int(torch.isnan(e).sum()) == 1
    fin = torch.isfinite(a) & (a > -87.0) & (a < 88.0)
    rel = (e[fin].double() / torch.exp(a[fin].double()) - 1).abs().max().item()
    assert rel < 3e-7, rel                                                  # (2 ulp: pconv_detmath.h)


def test_decision_points_hit_every_level():
    O.set_detmath(True)
    weight = torch.zeros(6, 8)
    weight[:, 0] = 1. / 9
    weight[:, 1:] = float(np.log(1. / 9))
    weight += torch.randn(6, 8, generator=torch.Generator().manual_seed(22)) * 0.2
    w16 = [15., 31., 54., 63., 63., 64., 64., 64., 64., 64., 64., 63., 63., 54., 31., 15.]
    octx = O.PseudoContextOp(16, 20, w16)
    od = O.PseudoDQuantOp(16, 6, 8, octx.addr())
    od.forward(torch.zeros(16, 6, 2, 64), weight)
    points = C.quant_points(od.level_table())
    assert points.shape == (6, 3 * 8 + 3 * 7 + 3 + 3 + 9)
    for width in (64, 66):
        x, where = C.quant_tensor(points, 16, 2, width)
        assert tuple(x.shape) == (16, 6, 2, width)
        val, idx = O.PseudoQuantOp(6, 8, 16, 0.9, 100, 2, 0.1, octx.addr()).forward(x, weight, torch.zeros(6, 8), False)
        assert set(idx.unique().tolist()) == set(float(v) for v in range(8))
        live = torch.zeros(16, 2, width, dtype=torch.bool)
        for t, lim in enumerate(O.widths_v3(w16, 16, 32, width)):
            live[t, :, :int(lim)] = True
        assert len(set(where[live].tolist())) == points.shape[1]
        per = C.per_point(idx, where, live, points.shape[1])
        # a level and its upper neighbour round to that level; the value below the lowest level to level 0
        assert bool((per[:, :8] == torch.arange(8.0)).all())


def test_scaling_modes_reach_every_3x3_kernel(monkeypatch):
    from pseudocylindrical_convolution_amd import PCONV
    kinds, split = set(), False
    for cfg in C.SCALING_SHAPES:
        for label, mode, flat in C.SCALING_MODES:
            monkeypatch.setenv("PCONV_CONV3X3", mode)
            monkeypatch.setattr(PCONV, "WINO_FLAT_REMAINDER", flat)
            plan = C.planned_kernels(PCONV, cfg)
            kinds |= set(kind for kind, _ in plan)
            split = split or (label == "default" and [kind for kind, _ in plan] in (["wino42", "wino"], ["wino42", "wino_flat"]))
    assert kinds == {"direct", "wino", "wino_flat", "wino42"} and split
    # every scaling keeps inputs, weights and outputs far inside the normal range
    assert all(-60 <= a <= 60 and -60 <= b <= 60 and -60 <= a + b <= 60 for a, b in C.SCALINGS)
