"""Cases shared by the tests that pin the oracle and the HIP ops to the REFERENCE's own kernels
(tests/test_reference_ops_cpu.py, tests/test_gpu_reference_golden.py) and by the fixture generator
(tests/golden/gen_golden.py).

A case is a name, an op family and its arguments.  `inputs(case)` draws the case's input tensors from fixed
seeds; `run(M, case, ins, dev)` drives the op classes of backend `M` -- oracle.pconv_cpu, the reference's CPU
module (oracle.ref_ops) or the product's PCONV -- through the same calls and returns every observable result
as CPU tensors, in a fixed order.  `interior(case, name, shape)` is the part of a result that no
unwritten-element mask may touch.

Shapes are the smallest that reach every branch: npart 16; 1, 2 and 4 rows per tile; widths at which polar
tiles are a few columns wide (W16 at 40, 72 and 128 columns gives 9, 17 and 30; the non-opt set at 24 and 40 gives
3 and 4, narrower than twice the pad), an all-full-width set in
which every tile wraps, the cosine rule, and the one weight total (3 * npart) at which the reference's two
width functions take different branches.

The masked 5x5 wavefront convolution is a family of its own (ECONV_CASES, `econv`): its reference kernels are
blocks of 128 cooperating threads, run by the cooperative launcher of oracle/ref_shim/.  Only the oracle's
summation order 0 has the reference's bits; the default order 1 and the HIP op are held under econv_bound.

MID_CASES are the same families on the weight sets other than W16 at 264, 520 and 131 columns: live only, kept
outside CASES / ALL_CASES / FIXTURE_CASES.  `check_against_oracle(case, got, want)` is the one rule that holds the
HIP ops' results to the oracle's on every case, small and mid (tests/test_gpu_ref_cases_vs_oracle.py).
"""
import collections

import numpy as np
import torch

NPART = 16
# tile widths in 1/64 of the ERP width: total > 3 * npart, the fixed-width branch (set_weight(16, opt=True))
W16 = [15., 31., 54., 63., 63., 64., 64., 64., 64., 64., 64., 63., 63., 54., 31., 15.]
WFULL = [64.] * 16                       # every tile as wide as the equator: only the wrap branches
# the other set of the operator layer, set_weight(16, opt=False) = ceil(64 cos(latitude of the tile centre)): the
# fixed-width branch too, and the narrowest tiles of all (W = 24 / 40 / 72 gives polar tiles of 3 / 4 / 8 columns)
WNOPT = [7., 19., 31., 41., 50., 57., 62., 64., 64., 62., 57., 50., 41., 31., 19., 7.]
WCOS = [1.0] * 16                        # total < 3 * npart: fractional weights, the cosine rule
WCOSB = [1.3, 1.2, 1.1, 1.0, 0.9, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.9, 1.0, 1.1, 1.2, 1.3]
WEDGE = [3.0] * 16                       # total == 3 * npart: _v2 takes the fixed widths, _v3 the cosine rule
WEIGHTS = dict(W16=W16, WNOPT=WNOPT, WFULL=WFULL, WCOS=WCOS, WCOSB=WCOSB, WEDGE=WEDGE)

THETA = [-0.5, 0, 0.5, 1, -0.5, 0, 0.5, 1, -0.5, 0, 0.5, 1, 0, 0]
PHI = [0, 0, 0, 0, 0.25, 0.25, 0.25, 0.25, -0.25, -0.25, -0.25, -0.25, 0.5, -0.5]


def _case(name, op, **kw):
    kw.update(name=name, op=op)
    return kw


def _cases():
    c = []
    # -- slice / uslice: n, c, rows per tile, ERP width, pad, weights --------------------------------------------
    for name, n, ch, h, w, pad, wt in [("h2_w72_p0", 1, 2, 2, 72, 0, "W16"), ("h4_w128_p1", 1, 1, 4, 128, 1, "W16"),
                                       ("h1_w40_p2_n2", 2, 1, 1, 40, 2, "W16"), ("h2_w72_p1_cos", 1, 1, 2, 72, 1, "WCOS"),
                                       ("h2_w72_p0_cosb", 2, 1, 2, 72, 0, "WCOSB"), ("h1_w40_p1_full", 1, 1, 1, 40, 1, "WFULL"),
                                       ("h2_w72_p0_edge", 1, 1, 2, 72, 0, "WEDGE"),
                                       ("h1_w24_p2_nopt", 1, 1, 1, 24, 2, "WNOPT"), ("h2_w40_p1_nopt", 2, 1, 2, 40, 1, "WNOPT"),
                                       ("h2_w72_p0_nopt", 1, 1, 2, 72, 0, "WNOPT")]:
        c.append(_case("slice_" + name, "slice", n=n, c=ch, h=h, w=w, pad=pad, weight=wt))
        if wt != "WEDGE":   # (there _v3's cosine rule would ask for tiles wider than the frame)
            c.append(_case("uslice_" + name, "uslice", n=n, c=ch, h=h, w=w, pad=pad, weight=wt))
    # -- pseudo context tables + pad (+ fill), entropy context tables + pad ---------------------------------------
    for name, n, ch, h, w, pad, wt in [("h2_w72_p1", 1, 1, 2, 72, 1, "W16"), ("h4_w128_p2", 1, 1, 4, 128, 2, "W16"),
                                       ("h1_w40_p2_n2", 2, 1, 1, 40, 2, "W16"), ("h2_w72_p0", 1, 1, 2, 72, 0, "W16"),
                                       ("h2_w72_p2_cos", 1, 1, 2, 72, 2, "WCOS"), ("h1_w40_p1_full", 1, 2, 1, 40, 1, "WFULL"),
                                       ("h1_w24_p2_nopt", 1, 1, 1, 24, 2, "WNOPT"), ("h2_w40_p1_nopt", 2, 1, 2, 40, 1, "WNOPT"),
                                       ("h2_w72_p0_nopt", 1, 1, 2, 72, 0, "WNOPT")]:
        for fill in (True, False):
            c.append(_case("pad_%s_%s" % (name, "filled" if fill else "dirty"), "pad", n=n, c=ch, h=h, w=w, pad=pad,
                           weight=wt, fill=fill))
    for name, n, ch, h, w, pad, wt in [("h2_w72_p1", 1, 1, 2, 72, 1, "W16"), ("h4_w128_p2", 1, 1, 4, 128, 2, "W16"),
                                       ("h1_w40_p2_n2", 2, 1, 1, 40, 2, "W16"), ("h2_w72_p2_cos", 1, 1, 2, 72, 2, "WCOS"),
                                       ("h1_w40_p1_full", 1, 2, 1, 40, 1, "WFULL"), ("h2_w72_p0", 1, 1, 2, 72, 0, "W16"),
                                       ("h1_w24_p2_nopt", 1, 1, 1, 24, 2, "WNOPT"), ("h2_w40_p1_nopt", 2, 1, 2, 40, 1, "WNOPT"),
                                       ("h2_w40_p0_nopt", 1, 1, 2, 40, 0, "WNOPT")]:
        for version in (0, 1):
            c.append(_case("epad_%s_v%d" % (name, version), "epad", n=n, c=ch, h=h, w=w, pad=pad, weight=wt,
                           version=version))
    for name, n, ch, h, w, pad, trim, fvalue, version in [("p0", 2, 2, 2, 72, 0, 0, 0, 0), ("p2", 1, 1, 1, 40, 2, 0, 0, 0),
                                                          ("p2_trim_v1", 2, 2, 4, 128, 2, 1, 3, 1),
                                                          ("p1_trim_neg_v2", 1, 1, 1, 40, 1, 1, -1, 2),
                                                          ("p0_v1", 1, 1, 2, 72, 0, 0, 0, 1), ("p1_h2", 1, 1, 2, 72, 1, 0, 0, 0),
                                                          ("p2_h2_trim_nopt", 2, 1, 2, 40, 2, 1, 2, 0)]:
        c.append(_case("fill_" + name, "fill", n=n, c=ch, h=h, w=w, pad=pad, trim=trim, fvalue=fvalue, version=version,
                       weight="WNOPT" if name.endswith("nopt") else "W16"))
    # -- quantiser ------------------------------------------------------------------------------------------------
    for name, n, ch, ntop, train, h, w, wt in [("ntop1", 1, 6, 1, False, 2, 72, "W16"), ("ntop2", 1, 3, 2, False, 1, 40, "W16"),
                                               ("ntop2_train", 1, 6, 2, True, 2, 72, "W16"),
                                               ("ntop1_train", 1, 3, 1, True, 1, 40, "W16"),
                                               ("ntop2_n2_nopt", 2, 3, 2, False, 1, 24, "WNOPT"),
                                               ("ntop1_h4", 1, 3, 1, False, 4, 72, "W16"),
                                               ("ntop2_h4_n2_train_nopt", 2, 3, 2, True, 4, 24, "WNOPT")]:
        c.append(_case("quant_" + name, "quant", n=n, c=ch, h=h, w=w, bins=8, ntop=ntop, train=train, weight=wt))
    # -- plain permutations and masks ----------------------------------------------------------------------------
    c.append(_case("dtow_s2", "dtow", shape=[16, 8, 2, 9], stride=2))
    c.append(_case("dtow_s3", "dtow", shape=[3, 18, 5, 7], stride=3))
    c.append(_case("context_reshape", "context_reshape", shape=[2, 12, 5, 7], ngroup=4))
    for k in (1, 2, 5, 6):
        c.append(_case("mask_constrain_%d" % k, "mask", constrain=k, ngroup=3, shape=[6, 6, 5, 5]))
    # -- entropy wavefront ops (everything but the masked convolution) ----------------------------------------
    for name, n, h, w, ng, cpg, wt in [("h1_w40_g4", 1, 1, 40, 4, 3, "W16"), ("h2_w72_g3_n2", 2, 2, 72, 3, 3, "W16"),
                                       ("h1_w40_g2_full", 1, 1, 40, 2, 3, "WFULL"), ("h1_w40_g2_c1", 1, 1, 40, 2, 1, "W16"),
                                       ("h4_w40_g2", 1, 4, 40, 2, 2, "W16"), ("h1_w24_g3_n2_nopt", 2, 1, 24, 3, 1, "WNOPT"),
                                       ("h2_w40_g2_nopt", 1, 2, 40, 2, 1, "WNOPT"),
                                       ("h1_w24_g2_nopt", 1, 1, 24, 2, 1, "WNOPT")]:
        c.append(_case("wave_" + name, "wave", n=n, h=h, w=w, ngroup=ng, cpg=cpg, weight=wt))
    # -- transcendental ops ---------------------------------------------------------------------------------------
    c.append(_case("gmm_loss", "gmm", m=257, ng=3))
    c.append(_case("gmm_table", "gmm_table", rows=720, ng=3))
    c.append(_case("gmm_table_batch", "gmm_table_batch", rows=720, ng=3))
    c.append(_case("projects_bilinear", "projects", near=False))
    c.append(_case("projects_nearest", "projects", near=True))
    return collections.OrderedDict((x["name"], x) for x in c)


def _econv_cases():
    c = []
    # -- the masked 5x5 wavefront convolution: entry point, constrain, pad_out, groups, input channels per group, rows
    #    per tile, width, weights, images, weight sets (group_out is 3 throughout).  The first four are stored.
    for name, entry, k, po, ng, gin, h, w, wt, n, nset in [
            ("plain_c5_p2_g4_i1_h1_w24_nopt", "forward", 5, 2, 4, 1, 1, 24, "WNOPT", 1, 1),
            ("act_c6_p0_g2_i3_h2_w40", "forward_act", 6, 0, 2, 3, 2, 40, "W16", 1, 1),
            ("batch_c6_p2_g2_i2_h1_w24_nopt_n2_s1", "forward_batch", 6, 2, 2, 2, 1, 24, "WNOPT", 2, 1),
            ("actbatch_c5_p0_g2_i1_h1_w40_n2_s2", "forward_act_batch", 5, 0, 2, 1, 1, 40, "W16", 2, 2),
            ("act_c6_p2_g4_i3_h4_w40", "forward_act", 6, 2, 4, 3, 4, 40, "W16", 1, 1),
            ("batch_c5_p0_g3_i2_h1_w72_n2_s2", "forward_batch", 5, 0, 3, 2, 1, 72, "W16", 2, 2),
            ("plain_c6_p2_g2_i3_h1_w40_full", "forward", 6, 2, 2, 3, 1, 40, "WFULL", 1, 1),
            ("actbatch_c6_p2_g3_i3_h2_w40_n2_s2", "forward_act_batch", 6, 2, 3, 3, 2, 40, "W16", 2, 2),
            ("plain_c5_p0_g4_i2_h2_w72", "forward", 5, 0, 4, 2, 2, 72, "W16", 1, 1),
            # the production shape: 14 groups, 42 -> 42 channels, one row per tile
            ("actbatch_c6_p2_g14_i3_h1_w24_nopt", "forward_act_batch", 6, 2, 14, 3, 1, 24, "WNOPT", 1, 1)]:
        c.append(_case("econv_" + name, "econv", entry=entry, constrain=k, pad_out=po, ngroup=ng, group_in=gin, h=h, w=w,
                       weight=wt, n=n, nset=nset))
    return collections.OrderedDict((x["name"], x) for x in c)


CASES = _cases()
# the masked convolution is a family of its own: held bit for bit only with the oracle's summation order 0, and
# stored in a fixture file of its own (ECONV_FIXTURE_FILE below)
ECONV_CASES = _econv_cases()
ALL_CASES = collections.OrderedDict(list(CASES.items()) + list(ECONV_CASES.items()))
TRANSCENDENTAL = ("gmm", "gmm_table", "gmm_table_batch", "quant", "projects")


def _mid_cases():
    """mid-size cases: the weight sets other than W16 at widths at which a kernel's loop over a row takes a second and
    a third trip with a ragged tail (264, 520: past 256 threads once and twice) and at an odd width (131: no tile row
    is 16-byte aligned, every 4-column form has to fall back or handle its tail).  They run live only -- against the
    reference on the CPU, against the oracle on the GPU -- and are stored nowhere."""
    c = []
    for wt in ("WNOPT", "WFULL", "WCOS", "WCOSB"):
        for w in (264, 520, 131):
            tag = "w%d_%s" % (w, wt[1:].lower())
            c.append(_case("mid_slice_" + tag, "slice", n=1, c=2, h=4, w=w, pad=1, weight=wt))
            c.append(_case("mid_uslice_" + tag, "uslice", n=1, c=2, h=4, w=w, pad=2, weight=wt))
            c.append(_case("mid_pad_" + tag, "pad", n=1, c=2, h=4, w=w, pad=2, weight=wt, fill=True))
            c.append(_case("mid_epad_" + tag, "epad", n=1, c=2, h=4, w=w, pad=2, weight=wt, version=1))
            c.append(_case("mid_fill_" + tag, "fill", n=1, c=2, h=4, w=w, pad=2, trim=1, fvalue=3, version=0, weight=wt))
            c.append(_case("mid_quant_" + tag, "quant", n=1, c=6, h=2, w=w, bins=8, ntop=2, train=False, weight=wt))
        tag = "w264_%s" % wt[1:].lower()
        c.append(_case("mid_wave_" + tag, "wave", n=1, h=2, w=264, ngroup=14, cpg=3, weight=wt))
        c.append(_case("mid_econv_" + tag, "econv", entry="forward_act_batch", constrain=6, pad_out=2, ngroup=14, group_in=3,
                       h=2, w=264, weight=wt, n=1, nset=1))
    return collections.OrderedDict((x["name"], x) for x in c)


# outside CASES / ALL_CASES / FIXTURE_CASES: the fixture files and the existing cases' name-derived seeds stay as they are
MID_CASES = _mid_cases()


def case_of(name):
    """the case of that name, small or mid"""
    return ALL_CASES[name] if name in ALL_CASES else MID_CASES[name]


def _gen(case):
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _quant_weight(c, bins, g):
    w = torch.zeros(c, bins)
    w[:, 0] = 1. / (bins + 1)
    w[:, 1:] = float(np.log(1. / (bins + 1)))
    return w + torch.rand(c, bins, generator=g) * 0.2


def inputs(case):
    """the case's input tensors (an ordered dict of CPU tensors), from seeds that depend on the case's name alone"""
    g, op, d = _gen(case), case["op"], collections.OrderedDict()
    rnd = lambda *s: torch.randn(*s, generator=g)
    if op in ("slice", "uslice"):
        n, c, h, w, p = case["n"], case["c"], case["h"], case["w"], case["pad"]
        img, tiles = (n, c, h * NPART, w), (n * NPART, c, h + 2 * p, w + 2 * p)
        d["x"], d["grad"] = (rnd(*img), rnd(*tiles)) if op == "slice" else (rnd(*tiles), rnd(*img))
    elif op in ("pad", "epad"):
        n, c, h, w, p = case["n"], case["c"], case["h"], case["w"], case["pad"]
        d["x"], d["grad"] = rnd(n * NPART, c, h, w), rnd(n * NPART, c, h + 2 * p, w + 2 * p)
    elif op == "fill":
        shape = (case["n"] * NPART, case["c"], case["h"] + 2 * case["pad"], case["w"] + 2 * case["pad"])
        d["x"], d["grad"] = rnd(*shape), rnd(*shape)
    elif op == "quant":
        shape = (case["n"] * NPART, case["c"], case["h"], case["w"])
        d["x"] = torch.rand(*shape, generator=g) * 1.4 - 0.2           # below the first and above the last level too
        d["x"].view(-1)[:4] = torch.tensor([-5.0, 5.0, 0.0, 1.0])
        d["weight"] = _quant_weight(case["c"], case["bins"], g)
        d["count"] = torch.rand(case["c"], case["bins"], generator=g) * 4.0
        d["count"][0, 0] = 0.0           # an empty first level: the split branch of the weight check
        d["count"][1, 5:] = 0.0          # empty top levels: the merge branch
        d["count"][2, :] = 0.0
        for k in range(case["ntop"]):
            d["grad%d" % k] = rnd(*shape)
    elif op == "dtow":
        d["x"] = rnd(*case["shape"])
    elif op == "context_reshape":
        n, c, h, w = case["shape"]
        d["x"], d["grad"] = rnd(n, c, h, w), rnd(n * h * w * case["ngroup"], c // case["ngroup"])
    elif op == "mask":
        d["w"], d["grad"] = rnd(*case["shape"]) + 3.0, rnd(*case["shape"]) + 3.0
    elif op == "wave":
        n, h, w, ng = case["n"], case["h"], case["w"], case["ngroup"]
        d["symbols"] = torch.randint(0, 8, (n * NPART, ng, h, w), generator=g).float()
        d["feat"] = rnd(n * NPART, ng * case["cpg"], h + 4, w + 4)
        d["feat2"] = rnd(n * NPART, ng * case["cpg"], h + 4, w + 4)
        d["dense"] = rnd(3 * n * NPART, ng * case["cpg"], h, w)
    elif op == "econv":
        # random everywhere -- the pad_in ring and the positions that are not yet causal too: the mask, not zeros in
        # the data, has to keep them out.  Bias and slopes are non-zero, the slopes inside (0, 1).
        cin, cout, nset = case["ngroup"] * case["group_in"], case["ngroup"] * 3, case["nset"]
        sets = (nset,) if "batch" in case["entry"] else ()
        d["x"] = rnd(case["n"] * NPART, cin, case["h"] + 4, case["w"] + 4)
        d["weight"] = rnd(*sets, cout, cin, 5, 5) * 0.1
        b = rnd(*sets, cout) * 0.1
        d["bias"] = torch.where(b.abs() < 1e-3, torch.full_like(b, 0.05), b)
        if "act" in case["entry"]:
            d["act"] = torch.rand(*sets, cout, generator=g) * 0.9 + 0.05
    elif op == "gmm":
        m, ng = case["m"], case["ng"]
        d["weight"] = torch.softmax(rnd(m, ng), 1).contiguous()
        d["delta"] = torch.exp(torch.rand(m, ng, generator=g) * 9.0 - 5.0)      # 0.007 .. 55
        d["mean"] = torch.rand(m, ng, generator=g) * 9.0 - 4.5                  # across and beyond the alphabet
        d["label"] = torch.randint(0, 8, (m, 1), generator=g).float() - 3.5
        d["top"] = rnd(m)
    elif op in ("gmm_table", "gmm_table_batch"):
        rows, ng = case["rows"], case["ng"]
        wgt = rnd(rows, ng) * 3.0
        delta = torch.exp(torch.rand(rows, ng, generator=g) * 11.0 - 6.0)       # 0.0025 .. 150
        delta[::17] = -delta[::17] * 0.01                                       # negative: the beta branch
        mean = torch.rand(rows, ng, generator=g) * 10.0 - 5.0
        if op == "gmm_table":    # each (1, ng, 24, rows / 24), read as flat [row][gaussian]
            d["weight"], d["delta"], d["mean"] = (t.view(1, ng, 24, rows // 24) for t in (wgt, delta, mean))
        else:   # sections weights | deltas | means, each (1, ng, 24, rows / 24) read as flat [row][gaussian]
            d["data"] = torch.stack([wgt.view(-1), delta.view(-1), mean.view(-1)]).view(3, ng, 24, rows // 24).contiguous()
        d["tnum"] = torch.tensor([rows - 20], dtype=torch.int32)
    elif op == "projects":
        d["x"], d["grad"] = rnd(1, 1, 32, 64), rnd(14, 1, 11, 16)
    else:
        raise KeyError(op)
    return d


def widths(case, rows_per_tile=None):
    """valid width of each tile of the case's tile stacks -- by the plain formulas of the two branches (no backend
    involved; the backends' own tables are compared with each other elsewhere)"""
    wt, w = np.asarray(WEIGHTS[case["weight"]], np.float32), case["w"]
    if case["op"] == "slice":
        fixed = not (float(wt.sum()) < 3 * NPART)
    else:
        fixed = float(wt.sum()) > 3 * NPART
    if fixed:
        return [int(float(np.float32(np.float32(wt[i] / np.float32(64)) * np.float32(w))) + 0.5) for i in range(NPART)]
    out = []
    for i in range(NPART):
        if i in (NPART // 2 - 1, NPART // 2):
            out.append(w)
            continue
        edge = ((i + 1) - 0.5 / case["h"]) / NPART if i < NPART // 2 else (i + 0.5 / case["h"]) / NPART
        out.append(int(float(np.float32(wt[i] * np.float32(w))) * np.cos((edge - 0.5) * float(np.float32(np.pi))) + 0.5))
    return out


def interior(case, name, shape):
    """bool array: the elements of result `name` that an unwritten-element mask must leave alone.  For a tile stack
    (tiles, c, h + 2 pad, w + 2 pad) that is rows pad .. pad + h and columns pad .. pad + width[tile]; every other
    result is interior as a whole."""
    keep = np.ones(shape, bool)
    pad = TILE_STACKS.get(case["op"], {}).get(name)
    if pad is None:
        return keep
    p = case[pad] if isinstance(pad, str) else pad
    wd = widths(case)
    keep[:] = False
    for t in range(shape[0]):
        keep[t, :, p:shape[2] - p, p:p + wd[t % NPART]] = True
    return keep


# results that are tile stacks, with the ring width their valid interior starts at
TILE_STACKS = {
    "slice": {"y": "pad"}, "uslice": {"gx": "pad"},
    "pad": {"y": "pad", "gx": 0, "filled": 0}, "epad": {"y": "pad", "gx": 0},
    "fill": {"y": 0, "gy": 0},
    "quant": {"val": 0, "idx": 0, "g_in": 0, "dq": 0},
    "wave": {"ctx": 2, "padded": 2, "padded_in": 2, "added": 2, "restart_ctx": 2},
    "econv": {"step0": "pad_out", "third": "pad_out", "last": "pad_out"},
}


def _is_oracle(M):
    return getattr(M, "__name__", "").endswith("pconv_cpu")


def _cpu(t):
    return t.detach().cpu().clone()


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a)).astype(np.int64))


def context_tables(M, ctx, kind, c, h, w, pad):
    """the tables a context hands to its ops, in one layout for the oracle and the reference: tile widths, source
    tile of each halo row, and per halo element destination row offset, source row offset, left source column and
    its lerp weight; for the entropy context also the wavefront order and the halo work lists"""
    out = collections.OrderedDict()
    if _is_oracle(M):
        t = ctx.produce_param(c, h, w, pad)
        out["widths"], out["halo_tile"] = _i32(t[0]), _i32(t[1]).view(NPART, -1)
        shape = (NPART, 2 * max(pad, 1) if kind == "pseudo" else 2 * pad, w)
        out["dst"], out["src"], out["col"] = _i32(t[2]).view(shape), _i32(t[3]).view(shape), _i32(t[4]).view(shape)
        out["lerp"] = torch.from_numpy(np.asarray(t[5], np.float32).copy()).view(shape)
        if kind == "entropy":
            total = int(t[7][h * NPART + w + pad - 1])
            out["halo_start"] = _i32(t[7][:h * NPART + w + pad])
            out["halo_list"] = _i32(t[6][:3 * total])
            idx, start = ctx.produce_param_group(h, w)
            out["wave_index"], out["wave_start"] = _i32(idx), _i32(start)
    else:
        t = ctx.produce_param(c, h, w, pad)
        if kind == "entropy":
            hindex, hindex2, param, param2, pad_idx = t
        else:
            param, hindex, hindex2 = t[0], t[2], t[3]
        out["widths"], out["halo_tile"] = hindex.cpu().long(), hindex2.cpu().long().view(NPART, -1)
        param = param.cpu()
        out["dst"], out["src"], out["col"] = param[..., 0].long(), param[..., 1].long(), param[..., 2].long()
        assert torch.equal(param[..., :3], param[..., :3].round())
        out["lerp"] = param[..., 3].contiguous()
        if kind == "entropy":
            total = int(pad_idx[h * NPART + w + pad - 1])
            out["halo_start"] = pad_idx.cpu().long()[:h * NPART + w + pad]
            out["halo_list"] = param2.cpu().view(-1).long()[:3 * total]
            idx, start = ctx.produce_param_group(h, w)
            out["wave_index"], out["wave_start"] = idx.cpu().long().view(-1), start.cpu().long().view(-1)
    return out


def run(M, case, ins, dev="cpu", tables=True):
    """drive backend M through the case; returns an ordered dict name -> CPU tensor.  `tables`: also read the
    context tables (oracle and reference only; the product keeps its tables in another layout)"""
    op, out = case["op"], collections.OrderedDict()
    x = {k: v.clone().to(dev) for k, v in ins.items()}
    wt = WEIGHTS.get(case.get("weight"))
    if op == "slice":
        o = M.SphereSliceOp(NPART, 0, case["pad"], wt, 0, False)
        out["y"] = _cpu(o.forward(x["x"])[0])
        out["gx"] = _cpu(o.backward(x["grad"])[0])
    elif op == "uslice":
        o = M.SphereUsliceOp(NPART, 0, case["pad"], wt, 0, False)
        out["y"] = _cpu(o.forward(x["x"])[0])
        out["gx"] = _cpu(o.backward(x["grad"])[0])
    elif op == "pad":
        ctx = M.PseudoContextOp(NPART, 20, wt, 0, False)
        ctx.start_context(case["w"])
        if tables and case["pad"] > 0:
            for k, v in context_tables(M, ctx, "pseudo", case["c"], case["h"], case["w"], case["pad"]).items():
                out["table_" + k] = v
        out["fill_param"] = _cpu(ctx.produce_fill_param(case["h"], case["w"])).long()
        xin = x["x"]
        if case["fill"]:
            xin = M.PseudoFillOp(0, NPART, 0, 0, ctx.addr(), 0, 0, False).forward(xin)[0]
            out["filled"] = _cpu(xin)
        o = M.PseudoPadOp(case["pad"], NPART, ctx.addr(), 0, False)
        out["y"] = _cpu(o.forward(xin)[0])
        out["gx"] = _cpu(o.backward(x["grad"])[0])
    elif op == "epad":
        ctx = M.PseudoEntropyContextOp(NPART, 20, case["version"], wt, 0, False)
        ctx.start_context(case["w"])
        if tables:
            for k, v in context_tables(M, ctx, "pseudo_entropy", case["c"], case["h"], case["w"], case["pad"]).items():
                out["table_" + k] = v
        o = M.PseudoEntropyPadOp(case["pad"], NPART, ctx.addr(), 0, False)
        out["y"] = _cpu(o.forward(x["x"])[0])
        out["gx"] = _cpu(o.backward(x["grad"])[0])
    elif op == "fill":
        v = case["version"]
        ctx = (M.PseudoContextOp(NPART, 20, wt, 0, False) if v == 0 else
               M.PseudoEntropyContextOp(NPART, 20, 1, wt, 0, False) if v == 1 else M.EntropyContextOp(NPART, 18, wt, 0, False))
        ctx.start_context(case["w"])
        o = M.PseudoFillOp(case["pad"], NPART, case["fvalue"], case["trim"], ctx.addr(), v, 0, False)
        out["y"] = _cpu(o.forward(x["x"])[0])
        out["gy"] = _cpu(o.backward(x["grad"])[0])
    elif op == "quant":
        ctx = M.PseudoContextOp(NPART, 20, wt, 0, False)
        ctx.start_context(case["w"])
        o = M.PseudoQuantOp(case["c"], case["bins"], NPART, 0.9, 1, case["ntop"], 0.1, ctx.addr(), 0, False)
        weight, count = x["weight"], x["count"]
        if case["train"]:
            o.forward(x["x"], weight, count, True)        # iteration 0: no check yet
        res = o.forward(x["x"], weight, count, case["train"])
        out["val"] = _cpu(res[0])
        if case["ntop"] > 1:
            out["idx"] = _cpu(res[1])
        out["weight_after"], out["count_after"] = _cpu(weight), _cpu(count)
        g = o.backward([x["grad%d" % k] for k in range(case["ntop"])], x["x"], res[0])
        out["g_in"], out["g_weight"], out["histogram"] = _cpu(g[0]), _cpu(g[1]), _cpu(g[2])
        sym = res[1] if case["ntop"] > 1 else None
        if sym is not None:
            dq = M.PseudoDQuantOp(NPART, case["c"], case["bins"], ctx.addr(), 0, False)
            out["dq"] = _cpu(dq.forward(sym.contiguous(), weight)[0])
    elif op == "dtow":
        for d2w in (True, False):
            o = M.DtowOp(case["stride"], d2w, 0, False)
            xin = x["x"] if d2w else x["x"].view(case["shape"][0], -1, case["shape"][2] * case["stride"],
                                                 case["shape"][3] * case["stride"]).contiguous()
            y = o.forward(xin)[0]
            out["y_d2w%d" % d2w] = _cpu(y)
            out["g_d2w%d" % d2w] = _cpu(o.backward(y.clone())[0])
    elif op == "context_reshape":
        o = M.ContextReshapeOp(case["ngroup"], 0, False)
        out["y"] = _cpu(o.forward(x["x"])[0])
        out["gx"] = _cpu(o.backward(x["grad"])[0])
    elif op == "mask":
        o = M.MaskConstrainOp(case["constrain"], case["ngroup"], 0, False)
        o.forward(x["w"])
        o.backward(x["grad"])
        out["w"], out["grad"] = _cpu(x["w"]), _cpu(x["grad"])
    elif op == "wave":
        _run_wave(M, case, x, out, dev, tables)
    elif op == "econv":
        _run_econv(M, case, x, out)
    elif op == "gmm":
        o = M.EntropyGmmOp(case["ng"], 0, 0, False)
        out["loss"] = _cpu(o.forward(x["weight"], x["delta"], x["mean"], x["label"])[0])
        for k, g in zip(("g_weight", "g_delta", "g_mean", "g_label"), o.backward(x["top"])):
            out[k] = _cpu(g)
    elif op == "gmm_table":
        o = M.EntropyGmmTableOp(8, 3.5, case["ng"], 65536, 1e-6, 0, False)
        n = int(ins["tnum"][0])
        out["table"] = _cpu(o.forward(x["weight"], x["delta"], x["mean"], ins["tnum"].clone())[0][:n])
        out["weight_after"], out["delta_after"] = _cpu(x["weight"].view(-1, case["ng"])[:n]), _cpu(x["delta"].view(-1, case["ng"])[:n])
    elif op == "gmm_table_batch":
        o = M.EntropyGmmTableOp(8, 3.5, case["ng"], 65536, 1e-6, 0, False)
        n = int(ins["tnum"][0])
        out["table"] = _cpu(o.forward_batch(x["data"], ins["tnum"].clone())[0][:n])
        out["data_after"] = _cpu(x["data"].view(3, -1)[:, :n * case["ng"]])
    elif op == "projects":
        o = M.ProjectsOp(11, 16, THETA, PHI, 0.5, case["near"], 0, False)
        out["y"] = _cpu(o.forward(x["x"])[0])
        g = o.backward(x["grad"])
        out["gx"], out["count"] = _cpu(g[0]), _cpu(g[1])
    else:
        raise KeyError(op)
    return out


def _run_wave(M, case, x, out, dev, tables):
    """the entropy model's wavefront ops without the masked convolution: the symbol scatter (DInput2Op), the halo
    run (EntropyCtxPadRun2Op, both `input` settings), the windowed add (EntropyAddOp) and the window extraction
    (DExtract2Op, label and batch forms), stepped over every diagonal of the frame"""
    n, h, w, ng = case["n"], case["h"], case["w"], case["ngroup"]
    ctx = M.EntropyContextOp(NPART, 18, WEIGHTS[case["weight"]], 0, False)
    ctx.start_context(w)
    addr = ctx.addr()
    if tables:
        for k, v in context_tables(M, ctx, "entropy", ng * case["cpg"], h, w, 2).items():
            out["table_" + k] = v
    data = M.PseudoFillOp(0, NPART, 0, 0, addr, 2, 0, False).forward(x["symbols"])[0]
    ipt = M.DInput2Op(ng, NPART, 2, -3.5, 3, addr, 0, False)
    pad_in = M.EntropyCtxPadRun2Op(2, NPART, ng, True, addr, 0, False)
    pad = M.EntropyCtxPadRun2Op(2, NPART, ng, False, addr, 0, False)
    add = M.EntropyAddOp(NPART, ng * case["cpg"], ng, 2, addr, 0, False)
    lab = M.DExtract2Op(NPART, ng, True, addr, 0, False)
    ext = M.DExtract2Op(NPART, ng, True, addr, 0, False)
    plain = M.DExtract2Op(NPART, ng, False, addr, 0, False)      # label = False: zero on step 0, one step behind after
    label = torch.zeros((n, 1, h * NPART, w), device=dev)
    nsteps = h * NPART + w + ng - 2
    counts, vectors, nlabel, labels, nplain, plains = [], [], [], [], [], []
    for _ in range(nsteps + 2):          # two steps past the end: every op must then leave its data alone
        b = ipt.forward(label)[0]
        padded_in = pad_in.forward(x["feat"])[0]
        padded = pad.forward(x["feat2"])[0]
        added = add.forward(padded, padded_in)[0]
        z, le = ext.forward_batch(x["dense"])
        k = int(le[0])
        counts.append(k)
        vectors.append(_cpu(z.reshape(-1)[:case["cpg"] * k]))
        label, ln = lab.forward(data)      # a compact vector: the first ln elements are this step's symbols
        nlabel.append(int(ln[0]))
        labels.append(_cpu(label.reshape(-1)[:int(ln[0])]))
        zp, lp = plain.forward(data)
        nplain.append(int(lp[0]))
        plains.append(_cpu(zp.reshape(-1)[:int(lp[0])]))
    out["ctx"] = _cpu(b)[:n * NPART]       # the replicas are copies of the first
    out["ctx_replicas_equal"] = torch.tensor([int(all(torch.equal(b[:n * NPART], b[r * n * NPART:(r + 1) * n * NPART])
                                                      for r in range(1, 3)))])
    out["padded_in"], out["padded"], out["added"] = _cpu(padded_in), _cpu(padded), _cpu(added)
    out["label_vectors"] = torch.cat(labels)
    out["batch_counts"], out["label_counts"] = torch.tensor(counts), torch.tensor(nlabel)
    out["batch_vectors"] = torch.cat(vectors)
    out["plain_counts"], out["plain_vectors"] = torch.tensor(nplain), torch.cat(plains)
    # restart(): every stepped op begins again at the first diagonal (the scatter zeroes its result, the extractions
    # return the first windows)
    for o in (ipt, pad_in, pad, add, ext, lab, plain):
        o.restart()
    again = []
    for _ in range(3):
        b = ipt.forward(label)[0]
        padded = pad.forward(pad_in.forward(x["feat"])[0])[0]
        added = add.forward(padded, x["feat2"])[0]
        z, le = ext.forward_batch(x["dense"])
        label, ln = lab.forward(data)
        zp, lp = plain.forward(data)
        again += [_cpu(z.reshape(-1)[:case["cpg"] * int(le[0])]), _cpu(label.reshape(-1)[:int(ln[0])]),
                  _cpu(zp.reshape(-1)[:int(lp[0])]), torch.tensor([float(le[0]), float(ln[0]), float(lp[0])])]
    out["restart_ctx"] = _cpu(b)[:n * NPART]
    out["restart_vectors"] = torch.cat(again)
    out["restart_added_window"] = _cpu(added)[:, :, 2:-2, 2:6]      # the first diagonals lie in the first columns


def econv_steps(case):
    """wavefront steps of the case's frame, and the step after which `third` is taken"""
    nsteps = case["h"] * NPART + case["w"] + case["ngroup"] - 2
    return nsteps, nsteps // 3


def _run_econv(M, case, x, out):
    """one masked layer (EntropyConv2Op, the case's entry point) stepped over every diagonal of the frame and two
    steps past the end, then restarted.  The op reuses one result tensor: each step adds its diagonals to it."""
    ng, po = case["ngroup"], case["pad_out"]
    ctx = M.EntropyContextOp(NPART, 18, WEIGHTS[case["weight"]], 0, False)
    ctx.start_context(case["w"])
    conv = M.EntropyConv2Op(NPART, ng * case["group_in"], ng, ng * 3, 5, case["constrain"], 2, po, ctx.addr(), 0, False)
    args = [x["x"], x["weight"], x["bias"]] + ([x["act"]] if "act" in x else [])
    step = getattr(conv, case["entry"])
    nsteps, third = econv_steps(case)
    for s in range(nsteps):
        y = step(*args)[0]
        if s == 0:
            out["step0"] = _cpu(y)
        if s == third:
            out["third"] = _cpu(y)
    out["last"] = _cpu(y)
    for _ in range(2):                     # past the end the op must leave its result alone
        y = step(*args)[0]
    out["past_the_end_unchanged"] = torch.tensor([int(torch.equal(_cpu(y), out["last"]))])
    conv.restart()                         # begins again at the first diagonal: step 0 zeroes the result
    for _ in range(3):
        y = step(*args)[0]
    out["restart_columns"] = _cpu(y)[:, :, :, :po + 4]      # the first diagonals lie in the first columns


def econv_diagonal(case, shape):
    """int array of a result's shape: the step that writes each element -- column + frame row + output group, the
    frame row being tile * rows per tile + row (entropy_conv_cuda_v2.cu: psum = tw + hp + tc); -1 on the pad_out ring"""
    h, w, po = case["h"], case["w"], case["pad_out"]
    d = np.full(shape, -1, np.int64)
    tile = (np.arange(shape[0]) % NPART)[:, None, None, None]
    group = (np.arange(shape[1]) // 3)[None, :, None, None]
    row, col = np.arange(h)[None, None, :, None], np.arange(w)[None, None, None, :]
    d[:, :, po:po + h, po:po + w] = col + tile * h + row + group
    return d


def econv_mask(case):
    """bool (cout, cin, 5, 5): the terms the causal channel limit lets through.  Output group tc at position
    (row, col) runs at step psum = col + row + tc; tap (kh, kw) reads position (row - 2 + kh, col - 2 + kw) and
    takes input channels below (psum - (row - 2 + kh) - (col - 2 + kw) [+ 1 for constrain 6]) * group_in =
    (tc + 4 - kh - kw [+ 1]) * group_in: the same for every position, so the layer is a dense masked convolution"""
    ng, gin = case["ngroup"], case["group_in"]
    tc = (np.arange(ng * 3) // 3)[:, None, None, None]
    ci = np.arange(ng * gin)[None, :, None, None]
    kh, kw = np.arange(5)[None, None, :, None], np.arange(5)[None, None, None, :]
    return ci < (tc + 4 - kh - kw + (1 if case["constrain"] == 6 else 0)) * gin


def econv_bound(case, ins):
    """per element of the padded result (float64 tensor): how far the masked convolution summed in the product's
    order (64 lanes over the tap-major index with fmaf, xor butterfly, bias) may lie from the reference's (products,
    128 threads each chaining its terms, seven tree levels, bias).  Either side is a sum of the same exact terms in
    which a term passes through at most d roundings, so it lies within gamma(d) * S of the exact value, with
    gamma(d) = d u / (1 - d u), u = 2^-24 and S = |bias| + sum |x| |w| over the unmasked terms:
        |y1 - y_ref| <= (gamma(d0) + gamma(d1)) * S
        d0 = 1 + ceil(25 group_in / 128) * ngroup + 7 + 1      product, per-thread chain, tree, bias
        d1 = ceil(25 channel / 64) + 6 + 1                      fmaf chain, butterfly, bias
    The _act entries multiply a negative sum by a slope in (0, 1): one more rounding on either side (d + 1), and
    nothing else -- where both sums are negative the slope shrinks their distance; where their signs differ, the
    positive one and slope * the negative one are no further apart than the two sums themselves.
    S is evaluated in float64 (a dense convolution of |x| with the masked |w|), with a relative margin of 1e-3 for
    that evaluation.  Zero on the pad_out ring."""
    ng, gin, po, h, w = case["ngroup"], case["group_in"], case["pad_out"], case["h"], case["w"]
    cin = ng * gin
    act = 1 if "act" in case["entry"] else 0
    d0 = 1 + -(-25 * gin // 128) * ng + 7 + 1 + act
    d1 = -(-25 * cin // 64) + 6 + 1 + act
    u = 2.0 ** -24
    gamma = lambda d: d * u / (1 - d * u)
    x = ins["x"].double().abs()
    wt, bias = ins["weight"].double().abs(), ins["bias"].double().abs()
    if wt.dim() == 4:
        wt, bias = wt[None], bias[None]
    wt = wt * torch.from_numpy(econv_mask(case))[None]
    n, nset = case["n"], wt.shape[0]
    per_set = max(n // nset, 1)
    S = torch.zeros(n * NPART, ng * 3, h + 2 * po, w + 2 * po, dtype=torch.float64)
    for img in range(n):
        k = img // per_set
        tiles = slice(img * NPART, (img + 1) * NPART)
        S[tiles, :, po:po + h, po:po + w] = torch.nn.functional.conv2d(x[tiles], wt[k]) + bias[k][None, :, None, None]
    return (gamma(d0) + gamma(d1)) * S * (1 + 1e-3)


def econv_within_bound(case, ins, got, ref):
    """asserts: results `got`, summed in the product's order, lie within econv_bound of the reference's `ref`, are
    exactly zero wherever the reference wrote nothing (not yet reached, outside the tile, the pad_out ring), and the
    flag agrees; returns the worst difference / bound"""
    bound = econv_bound(case, ins)
    po, worst = case["pad_out"], 0.0
    for key in ("step0", "third", "last", "restart_columns"):
        a, b = got[key].double(), ref[key].double()
        lim = bound if key != "restart_columns" else bound[:, :, :, :po + 4]
        assert tuple(a.shape) == tuple(b.shape) == tuple(lim.shape), key
        assert (a[b == 0] == 0).all(), "%s/%s: written where the reference wrote nothing" % (case["name"], key)
        diff = (a - b).abs()
        assert (diff <= lim).all(), "%s/%s: %g times the bound" % (case["name"], key, (diff / lim)[lim > 0].max().item())
        worst = max(worst, (diff / lim)[lim > 0].max().item())
    assert torch.equal(got["past_the_end_unchanged"], ref["past_the_end_unchanged"])
    return worst


def compare(case, got, ref, masks, exact=True, tol=None):
    """`got` against the reference's `ref` under the unwritten-element masks; returns a list of
    (name, worst absolute difference, scale, elements that differ) for the results that are not bit-equal"""
    report = []
    assert list(got.keys()) == list(ref.keys()), (list(got.keys()), list(ref.keys()))
    for name in ref:
        a, b = got[name], ref[name]
        assert tuple(a.shape) == tuple(b.shape), (case["name"], name, tuple(a.shape), tuple(b.shape))
        a, b = a.to(torch.float64), b.to(torch.float64)
        m = masks.get(name)
        if m is not None:
            keep = ~torch.as_tensor(m)
            a, b = a[keep], b[keep]
        bad = (a != b) & ~(torch.isnan(a) & torch.isnan(b))
        if bool(bad.any()):
            diff = (a - b).abs()
            diff[torch.isnan(diff)] = float("inf")
            report.append((name, float(diff.max()), float(b[torch.isfinite(b)].abs().max()) if b.numel() else 0.0, int(bad.sum())))
    return report


# -- the HIP ops against the oracle: one rule per result of each family -------------------------------------------
# ("equal",) bit for bit; ("scale", tol) |got - want| <= tol * max(1, |want|.max()); ("abs", tol) |got - want| <= tol.
# Each is the tightest bound the op already holds against the oracle in tests/test_gpu_ops.py (bit for bit: index
# work, gathers and lerps, the quantiser's forward, the masked convolution in the oracle's order 1, the CDF tables),
# tests/test_gpu_backward.py (1e-5 of scale for the backward sums of slice / uslice / pad / entropy pad, whose order
# differs; 1e-6 for the entropy pad's forward and the quantiser's input gradient; 1e-4 for the float-atomic sums;
# 1e-5 absolute for the GMM loss, 1e-4 of scale for its gradients) and, under ordered=True,
# tests/test_gpu_backward_ordered.py (slice, uslice and the viewport sampling walk the oracle's own order).
EQUAL = ("equal",)
_ORACLE_RULES = {
    "slice": {"y": EQUAL, "gx": ("scale", 1e-5)},
    "uslice": {"y": EQUAL, "gx": ("scale", 1e-5)},
    "pad": {"fill_param": EQUAL, "filled": EQUAL, "y": EQUAL, "gx": ("scale", 1e-5)},
    "epad": {"y": ("scale", 1e-6), "gx": ("scale", 1e-5)},
    "fill": {"y": EQUAL, "gy": EQUAL},
    "quant": {"val": EQUAL, "idx": EQUAL, "dq": EQUAL, "histogram": EQUAL, "weight_after": EQUAL, "count_after": EQUAL,
              "g_in": ("scale", 1e-6), "g_weight": ("scale", 1e-4)},
    "projects": {"y": EQUAL, "gx": ("scale", 1e-4), "count": ("scale", 1e-4)},
    "gmm": {"loss": ("abs", 1e-5), "g_weight": ("scale", 1e-4), "g_delta": ("scale", 1e-4), "g_mean": ("scale", 1e-4),
            "g_label": ("scale", 1e-4)},
}
_ORDERED_EQUAL = {"slice": ("gx",), "uslice": ("gx",), "projects": ("gx", "count")}
# every result of these is bit for bit (dtow, context_reshape and mask are permutations and masks; the wave ops index
# work; econv the oracle's CONV_ORDER 1; the CDF tables and the softmax written in place run the same polynomials)
_ALL_EQUAL = ("dtow", "context_reshape", "mask", "wave", "econv", "gmm_table", "gmm_table_batch")
BACKWARD_FAMILIES = ("slice", "uslice", "projects", "quant")      # what PCONV.ordered_backward(True) changes


def oracle_rule(case, name, ordered=False):
    """how result `name` of the case is held to the oracle's: ("equal",), ("scale", tol) or ("abs", tol)"""
    op = case["op"]
    if op in _ALL_EQUAL or (ordered and name in _ORDERED_EQUAL.get(op, ())):
        return EQUAL
    return _ORACLE_RULES[op][name]


def dead_columns(case, name, t):
    """bool mask of result `name`'s shape (a torch tensor `t` of that shape): the columns at or beyond each tile's valid
    width inside the rows and columns the op owns -- where slice `y` and the quantiser's `g_in` are exactly zero"""
    p = case["pad"] if case["op"] == "slice" else 0
    dead = torch.zeros(t.shape, dtype=torch.bool)
    for tile, v in enumerate(widths(case)):
        dead[tile::NPART, :, p:t.shape[2] - p, p + v:t.shape[3] - p] = True
    return dead


LIBM_ULPS = 1.0     # expf / logf of the C library and of the device library: each documented within 1 ulp


def quant_merge_bound(case, ins):
    """(channel, levels) float64: how far the level weights may lie from the oracle's after the training-mode merge
    of unused levels (pseudo_quant_cuda.cu:97-143).  That step is three libm calls per channel -- the oracle's are
    the C library's logf / expf, the product's the device library's through torch.log / torch.exp -- and there is no
    published polynomial for it: the reason is arithmetic, and the bound follows the step's own operations.  With
    sp(v) the float32 spacing at v, and either library within LIBM_ULPS of the exact function, so that two results
    of one call lie within 2 LIBM_ULPS sp(.) of each other:
        t = w[top] - log(k), k = levels - top > 1:   d_t = 2 L sp(log k) + sp(t)      (the subtraction rounds on either
                                                     side by half a spacing; k = 1: log 1 = 0 exactly, nothing moves)
        e_i = exp(w_i), i = 1, 2:                    d_i = e_i (exp(d_w_i) - 1) + 2 L sp(e_i)
        w0' = w0 + e_1:                              d_0 = d_1 + sp(w0')
        s = (e_1 + e_2) / 2:                         d_s = (d_1 + d_2) / 2 + sp(s)    (the halving is exact)
        m = log(s):                                  d_m = -log(1 - d_s / s) + 2 L sp(m)
    evaluated in float64 at the exact values, spacings taken a part in 1e5 above them and the whole with a relative
    margin of 1e-6 for that evaluation.  Zero for every weight the step leaves alone."""
    levels = case["bins"]
    w, cnt = ins["weight"].double().numpy().copy(), ins["count"].numpy()
    err = np.zeros_like(w)
    sp = lambda v: float(np.spacing(np.float32(abs(v) * (1 + 1e-5))))
    for i in range(case["c"]):
        j = levels - 1
        while j > 1 and not cnt[i, j] >= np.float32(1e-3):
            j -= 1
        k = levels - j
        if k > 1:
            t = w[i, j] - np.log(k)
            w[i, j:], err[i, j:] = t, 2 * LIBM_ULPS * sp(np.log(k)) + sp(t)
        if cnt[i, 0] < np.float32(1e-3):
            e = [np.exp(w[i, q]) for q in (1, 2)]
            d = [e[q] * np.expm1(err[i, q + 1]) + 2 * LIBM_ULPS * sp(e[q]) for q in (0, 1)]
            w0 = w[i, 0] + e[0]
            s, ds = (e[0] + e[1]) / 2, (d[0] + d[1]) / 2 + sp((e[0] + e[1]) / 2)
            m = np.log(s)
            w[i, 0], err[i, 0] = w0, d[0] + sp(w0)
            w[i, 1:3], err[i, 1:3] = m, -np.log1p(-ds / s) + 2 * LIBM_ULPS * sp(m)
    return torch.from_numpy(err) * (1 + 1e-6)


def check_against_oracle(case, got, want, ordered=False):
    """the one place that says how each result of each family is held to the oracle: `got` (the HIP ops', run with
    tables=False) against `want` (the oracle's, set_detmath(True), CONV_ORDER 1).  Returns the list of violations, one
    line each; empty when the case holds.  `ordered`: the results were computed under PCONV.ordered_backward(True).

    One departure from bit-equality, derived here: a training-mode quantiser case merges unused levels with libm
    calls (quant_merge_bound).  Its `weight_after` is held to that bound, `count_after` bit for bit, and every other
    result -- all of them computed from the merged weights -- to its usual rule against the oracle started from the
    weights `got` holds: the libm step is isolated, and nothing after it is any looser for it."""
    bad = []
    name = case["name"]
    expect = [k for k in want if not k.startswith("table_")]
    if [k for k in got if not k.startswith("table_")] != expect:
        return ["%s: results %s, the oracle's %s" % (name, list(got), expect)]
    merged = None
    if case["op"] == "quant" and case["train"]:
        ins = inputs(case)
        merged = quant_merge_bound(case, ins)
        if tuple(got["weight_after"].shape) == tuple(merged.shape) and bool(torch.isfinite(got["weight_after"]).all()):
            from oracle import pconv_cpu as O
            ins["weight"], ins["count"] = got["weight_after"].clone(), got["count_after"].clone()
            again = run(O, dict(case, train=False), ins)
            want = type(want)((k, v if k in ("weight_after", "count_after") else again[k]) for k, v in want.items())
    for key in expect:
        a, b = got[key], want[key]
        if tuple(a.shape) != tuple(b.shape):
            bad.append("%s/%s: shape %s, the oracle's %s" % (name, key, tuple(a.shape), tuple(b.shape)))
            continue
        if merged is not None and key == "weight_after":
            diff = (a.double() - b.double()).abs()
            if not bool((diff <= merged).all()):      # (NaN fails)
                bad.append("%s/%s: %g times the merge bound (worst |diff| %g)"
                           % (name, key, (diff / merged.clamp_min(1e-300)).max().item(), diff.max().item()))
            continue
        rule = oracle_rule(case, key, ordered)
        if case["op"] == "slice" and key == "y" and case["pad"] > 0:
            # the reference leaves the ring of a padded slice undefined: the interior, dead columns included
            p = case["pad"]
            a, b = a[:, :, p:-p, p:-p], b[:, :, p:-p, p:-p]
        if rule == EQUAL:
            if not torch.equal(a, b):
                ne = (a != b) if a.dtype == b.dtype else torch.ones(a.shape, dtype=torch.bool)
                worst = (a.double() - b.double()).abs()
                worst = worst[~torch.isnan(worst)].max().item() if bool((~torch.isnan(worst)).any()) else float("nan")
                bad.append("%s/%s: not bit-equal, %d elements differ, first at %s, max abs diff %g"
                           % (name, key, int(ne.sum()), tuple(ne.nonzero()[0].tolist()) if bool(ne.any()) else (), worst))
        else:
            tol = rule[1] * (max(1.0, b.abs().max().item()) if rule[0] == "scale" else 1.0)
            diff = (a.double() - b.double()).abs()
            worst = diff.max().item() if diff.numel() else 0.0
            if not worst <= tol:      # (NaN fails)
                bad.append("%s/%s: %g > %g (%s %g)" % (name, key, worst, tol, rule[0], rule[1]))
        if (case["op"], key) in (("slice", "y"), ("quant", "g_in")):
            dead = dead_columns(case, key, got[key])
            if bool((got[key][dead] != 0).any()):
                bad.append("%s/%s: %d non-zero elements in dead columns" % (name, key, int((got[key][dead] != 0).sum())))
    return bad


def gmm_loss_bound(ref_loss, erf_abs=1.2e-7):
    """per element: how far the GMM loss may move when erf is the product's published polynomial (|erff - erf| <
    erf_abs absolute, include/pconv_detmath.h) and not libm's.  loss = -log(p + 1e-7), p = sum_i w_i (fb_i - fa_i),
    fa / fb = 0.5 + 0.5 erf(.) rounded to float: each of fa, fb moves by at most 0.5 * erf_abs plus one rounding of
    a value below 1 (2^-24), so p moves by at most dp = sum_i w_i * 2 * (0.5 * erf_abs + 2^-24) plus the roundings
    of the weighted sum (4 * 2^-24 * p); the logarithm turns that into dp / (p + 1e-7 - dp); one more ulp of the
    result for its own rounding.  Rows whose probability is of the order of 1e-7 are ill-conditioned by
    construction, and the bound says so."""
    loss = ref_loss.double()
    big = torch.exp(-loss)                                    # P = p + 1e-7 of the reference
    wsum = 1.0 + 8 * 2.0 ** -23                               # the weights are a float softmax: they sum to 1
    dp = wsum * 2 * (0.5 * erf_abs + 2.0 ** -24) + 4 * 2.0 ** -24 * big
    # the other side's P' lies in [max(P - dp, 1e-7), P + dp] (its p is a probability, not below 0): where P - dp
    # stays above 1e-7 the loss moves by at most log(P / (P - dp)) <= dp / (P - dp); on the rows below, by at most
    # log((P + dp) / 1e-7) -- at most log(1 + 2 dp / 1e-7) = 2.0: those rows are held to that and no tighter
    well = big - dp > 1e-7
    bound = torch.where(well, dp / (big - dp).clamp_min(1e-7), torch.log((big + dp) / 1e-7))
    return bound + 2.0 ** -23 * loss.abs()


# -- the reference's results, with the elements it never writes ---------------------------------------------------
# The reference allocates its results uninitialised and leaves some elements unwritten (the ring of a padded slice,
# dead columns).  Which ones is found from evidence: the same cases run in two fresh processes whose allocator
# fills new memory with different bytes (glibc's MALLOC_PERTURB_); whatever differs between the two was never
# written.  The fill can only be chosen when a process starts, hence the child processes.
PERTURB = ("85", "170")


def dump_reference(path, names=None):
    """(child process) run the cases on the reference's CPU module, write every result to `path`"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.ref_ops import ref_ops
    R = ref_ops()
    arrays = {}
    # every small case, or the named ones (the mid cases run only when named)
    for name, case in (list(ALL_CASES.items()) + list(MID_CASES.items())):
        if (names and name not in names) or (not names and name in MID_CASES):
            continue
        for k, v in run(R, case, inputs(case)).items():
            arrays[name + "/" + k] = v.numpy()
    np.savez(path, **arrays)


def reference_results(tmpdir, names=None):
    """{case: {result: tensor}}, {case: {result: bool mask of unwritten elements}} from two child processes;
    asserts that no mask touches a valid interior"""
    import os
    import subprocess
    import sys
    here = os.path.abspath(__file__)
    procs, paths = [], []
    for fill in PERTURB:
        path = os.path.join(str(tmpdir), "ref_ops_%s.npz" % fill)
        env = dict(os.environ, MALLOC_PERTURB_=fill, OMP_NUM_THREADS="1")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [here, "dump", path] + list(names or [])
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        paths.append(path)
    for p in procs:
        log = p.communicate()[0].decode(errors="replace")
        assert p.returncode == 0, log[-3000:]
    a, b = (np.load(p) for p in paths)
    assert sorted(a.files) == sorted(b.files)
    results, masks = collections.OrderedDict(), collections.OrderedDict()
    for key in a.files:
        name, k = key.split("/")
        va, vb = a[key], b[key]
        # bytes, not values: two fills never agree in a whole element, NaN patterns included
        differ = (va.view(np.uint8).reshape(va.shape + (va.itemsize,)) != vb.view(np.uint8).reshape(vb.shape + (vb.itemsize,))).any(-1) \
            if va.size else np.zeros(va.shape, bool)
        results.setdefault(name, collections.OrderedDict())[k] = torch.from_numpy(np.where(differ, 0, va).astype(va.dtype))
        if differ.any():
            inside = differ & interior(case_of(name), k, va.shape)
            assert not inside.any(), "%s/%s: %d unwritten elements inside the valid interior" % (name, k, int(inside.sum()))
            masks.setdefault(name, collections.OrderedDict())[k] = differ
        masks.setdefault(name, collections.OrderedDict())
    ordered = collections.OrderedDict((n, results[n]) for n in list(ALL_CASES) + list(MID_CASES) if n in results)
    return ordered, masks


# -- fixtures: tests/golden/ref_ops_*.npz ------------------------------------------------------------------------
FIXTURE_FILES = collections.OrderedDict([
    ("ref_ops_slice.npz", ("slice", "uslice")),
    ("ref_ops_pad.npz", ("pad", "epad", "fill")),
    ("ref_ops_quant.npz", ("quant",)),
    ("ref_ops_wave.npz", ("wave",)),
    ("ref_ops_misc.npz", ("dtow", "context_reshape", "mask", "gmm", "gmm_table", "gmm_table_batch", "projects")),
])
# the cases that are stored (every family, every branch named in the module's docstring; the rest run live only)
FIXTURE_CASES = (
    "slice_h1_w40_p2_n2", "slice_h2_w72_p0_edge", "slice_h1_w24_p2_nopt", "uslice_h1_w40_p2_n2", "uslice_h2_w72_p1_cos",
    "uslice_h2_w40_p1_nopt",
    "pad_h2_w72_p1_filled", "pad_h2_w72_p0_dirty", "pad_h1_w24_p2_nopt_dirty",
    "epad_h1_w40_p2_n2_v1", "epad_h1_w24_p2_nopt_v0", "epad_h2_w72_p0_v1", "epad_h2_w40_p0_nopt_v0",
    "fill_p1_trim_neg_v2",
    "quant_ntop1_train", "quant_ntop2_n2_nopt",
    "wave_h1_w40_g2_c1", "wave_h1_w24_g2_nopt",
    "dtow_s2", "dtow_s3", "context_reshape", "mask_constrain_5", "mask_constrain_6", "gmm_loss", "gmm_table", "gmm_table_batch", "projects_bilinear", "projects_nearest",
)


# the masked convolution's file, outside FIXTURE_FILES (whose total size is capped as it stands): between them the
# stored cases hold all four entry points, both constraints, both pad_out values, the narrow WNOPT tiles, 1 and 2
# rows per tile, and batch entries with two weight sets and with one set for two images
ECONV_FIXTURE_FILE = "ref_ops_econv.npz"
ECONV_FIXTURE_CASES = (
    "econv_plain_c5_p2_g4_i1_h1_w24_nopt", "econv_act_c6_p0_g2_i3_h2_w40", "econv_batch_c6_p2_g2_i2_h1_w24_nopt_n2_s1",
    "econv_actbatch_c5_p0_g2_i1_h1_w40_n2_s2",
)


def write_fixtures(out_dir, results, masks, files=None, names=None):
    """one .npz per family: per case its arguments (JSON), inputs, the reference's results and the
    unwritten-element masks (bit-packed)"""
    import json
    import os
    sizes = {}
    for fname, ops in (files or FIXTURE_FILES).items():
        arrays = {}
        for name in (names or FIXTURE_CASES):
            case = ALL_CASES[name]
            if case["op"] not in ops:
                continue
            arrays[name + "/spec"] = np.array(json.dumps(case, sort_keys=True))
            for k, v in inputs(case).items():
                arrays[name + "/in/" + k] = v.numpy()
            for k, v in results[name].items():
                arrays[name + "/out/" + k] = v.numpy()
            for k, m in masks[name].items():
                assert not (m & interior(case, k, m.shape)).any()
                arrays[name + "/mask/" + k] = np.packbits(m.reshape(-1))
        path = os.path.join(out_dir, fname)
        np.savez_compressed(path, **arrays)
        sizes[fname] = os.path.getsize(path)
    return sizes


def write_econv_fixtures(out_dir, results, masks):
    return write_fixtures(out_dir, results, masks, {ECONV_FIXTURE_FILE: ("econv",)}, ECONV_FIXTURE_CASES)


def load_econv_fixtures(golden_dir):
    """{case name: (case, inputs, results, masks)} from tests/golden/ref_ops_econv.npz"""
    return load_fixtures(golden_dir, (ECONV_FIXTURE_FILE,))


def load_fixtures(golden_dir, files=None):
    """{case name: (case, inputs, results, masks)} from tests/golden/ref_ops_*.npz"""
    import json
    import os
    out = collections.OrderedDict()
    for fname in (files or FIXTURE_FILES):
        z = np.load(os.path.join(golden_dir, fname))
        names = [k[:-5] for k in z.files if k.endswith("/spec")]
        for name in names:
            case = json.loads(str(z[name + "/spec"]))
            ins, res, masks = collections.OrderedDict(), collections.OrderedDict(), {}
            for k in z.files:
                if k.startswith(name + "/in/"):
                    ins[k.split("/", 2)[2]] = torch.from_numpy(z[k])
                elif k.startswith(name + "/out/"):
                    res[k.split("/", 2)[2]] = torch.from_numpy(z[k])
            for k in z.files:
                if k.startswith(name + "/mask/"):
                    r = k.split("/", 2)[2]
                    masks[r] = np.unpackbits(z[k])[:res[r].numel()].astype(bool).reshape(tuple(res[r].shape))
            out[name] = (case, ins, res, masks)
    return out


if __name__ == "__main__":
    import sys
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump_reference(sys.argv[2], sys.argv[3:])
