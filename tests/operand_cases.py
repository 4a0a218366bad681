"""Shared by tests/test_operands_cpu.py (CPU) and tests/test_gpu_operands.py (GPU): the operand contract of PCONV.py.

For every tensor operand of every public entry point exactly one of two things happens: the call raises PconvError
naming the op and the operand, or it returns the bits of the same call with that operand as a dense, aligned float32
(int32, ...) GPU tensor of the stated shape.  ROWS has one row per (entry point, route): a recipe for the smallest
well-formed call -- the inputs of ref_ops_cases / conv_backward_cases / masked_conv_cases and the shapes of TILE_CONVS
in test_gpu_stale_memory.py with two tiles -- and per operand the element type and the PINNED outcome of the two
deformations that run for real, `strided` and `offset`: HONOURED (same bits) or REFUSED.  `dtype`, `device` and `short`
are always refused, and are only ever tried with the library replaced by a recorder: a wrapper that reaches the library
with such an operand fails the test and launches nothing.

The safety rule: no case launches a kernel with an operand whose storage does not cover a dense read of the operand's
stated shape from its first element.  `strided` (a double-width buffer, or a transposed dense buffer of the same size)
and `offset` (a buffer one element longer) satisfy it by construction; test_operands_cpu.py holds the builders to it.

What a refusal has to say: it begins with the op's name, and -- where the entry has more than one tensor operand -- holds
the operand's name as a word.  With one tensor operand the op's name identifies it; this is less than "naming the op
and the operand" everywhere, and it is what the harness holds.  The op's name is the class or function name; the
*_device forms of ws_metrics, ws_msssim and sphere_points_mse refuse under the name of the function they compute.  A
refusal of `offset` may come from the entry point's own argument check ("... must be 8-byte aligned"): any PconvError
counts there.

An (operand, deformation) pair is not applicable only for one of the three reasons below, named in the row.

NO_ADDRESS lists the public entries that take no tensor or never turn one into an address; test_operands_cpu.py holds
ROWS + NO_ADDRESS to exactly the public surface of PCONV.py (NOT_SWEPT, entries with a tensor and no row, is held
empty), so that a new wrapper has to be given a row.
"""
import collections
import inspect
import re

import torch

import conv_backward_cases as CB
import masked_conv_cases as MC
import ref_ops_cases as C

HONOURED, REFUSED = "honoured", "refused"
DEFORMATIONS = ("strided", "offset", "dtype", "device", "short")
ONE_ELEMENT = "a one-element operand has no strided form"
DEFINES_SHAPE = "the operand defines the call's shape"
NOT_A_TENSOR = "the operand is not a tensor that is turned into an address"
REASONS = (ONE_ELEMENT, DEFINES_SHAPE, NOT_A_TENSOR)

SENTINEL = -7.5      # what the buffer behind a view holds in its gaps; an in-place op must leave it there
OTHER_DTYPE = {torch.float32: torch.float64, torch.int32: torch.int64, torch.float64: torch.float32,
               torch.int64: torch.int32, torch.uint8: torch.int16, torch.uint16: torch.int32}


class Reached(AssertionError):
    """the recorder's verdict: a wrapper reached the library with an operand it had to refuse"""


# ---- the deformations ------------------------------------------------------------------------------------------------

def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else 113


def strided_forms(t):
    """[(form, view, buffer)]: views of `t`'s shape and values that are not dense.  'wide': buf[..., ::2] of a buffer twice
    as wide; 'transposed' (rank >= 2, and only where the result is not dense): t.transpose(-1, -2).contiguous()
    .transpose(-1, -2).  Either storage covers a dense read of the shape from the view's first element."""
    buf = torch.full(tuple(t.shape[:-1]) + (2 * t.shape[-1],), _sentinel(t.dtype), dtype=t.dtype, device=t.device)
    wide = buf[..., ::2]
    wide.copy_(t)
    forms = [("wide", wide, buf)]
    if t.dim() >= 2:
        tr = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        if not tr.is_contiguous():
            forms.append(("transposed", tr, tr))
    return forms


def offset_form(t):
    """(view, buffer): flat[1:].view(shape) of a buffer one element longer -- dense, element-aligned, and for 4-byte
    elements never 8- or 16-byte aligned"""
    buf = torch.full((t.numel() + 1,), _sentinel(t.dtype), dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view, buf


def other_dtype(t):
    return t.to(OTHER_DTYPE[t.dtype])


def other_device(t, device):
    return t.to(device)


def shorter(t):
    """one element fewer along the first dimension"""
    return t[:-1].clone()


def one_more(t):
    """a count operand: one more than it was"""
    return t + 1


def dense_read_covered(view):
    """the safety rule for one tensor: its storage holds numel() elements from its first element on"""
    return view.untyped_storage().nbytes() // view.element_size() - view.storage_offset() >= view.numel()


def bits(t):
    """the tensor's bits on the CPU: int32 for 4-byte elements (as conv_backward_cases.bits), bytes otherwise"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.uint8)


# ---- the table -------------------------------------------------------------------------------------------------------

Operand = collections.namedtuple("Operand", "name strided offset na short")
Row = collections.namedtuple("Row", "entry route op make operands inplace env")      # op: the name a refusal carries
Case = collections.namedtuple("Case", "args run prepare")


def opd(name, strided=REFUSED, offset=HONOURED, shorten=shorter, **na):
    """an operand: the pinned outcomes of `strided` and `offset`, how `short` is made, and name=reason for what does not
    apply"""
    if strided in REASONS:
        na["strided"] = strided
    if offset in REASONS:
        na["offset"] = offset
    assert all(k in DEFORMATIONS and v in REASONS for k, v in na.items()), na
    return Operand(name, strided, offset, na, None if "short" in na else shorten)


ROWS = []


def row(entry, operands, route="", inplace=(), env=None, op=None):
    def register(make, op=op):
        op = op or entry.split(".")[0]
        ROWS.append(Row(entry, route, op, make, tuple(operands), tuple(inplace), dict(env or {})))
        return make
    return register


def row_id(r):
    return r.entry + ("@" + r.route if r.route else "")


def X(name="x", **kw):
    """the operand that defines the shape of a call that _require_gpu guards: contiguous only, any 4-byte offset"""
    na = dict(short=DEFINES_SHAPE)
    na.update(kw.pop("na", {}))
    return opd(name, kw.get("strided", REFUSED), kw.get("offset", HONOURED), **na)


def A(dev, **kw):
    """the arguments of a call: tensors cloned to `dev`, everything else as it is"""
    out = collections.OrderedDict()
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().clone().to(dev)
        elif isinstance(v, (list, tuple)) and v and all(isinstance(t, torch.Tensor) for t in v):
            v = [t.detach().clone().to(dev) for t in v]
        out[k] = v
    return out


def R(**kw):
    return collections.OrderedDict(kw)


def get(args, name):
    """args[name], or args[root][i] for name = 'root[i]'"""
    m = re.match(r"^(\w+)\[(\d+)\]$", name)
    return args[m.group(1)][int(m.group(2))] if m else args[name]


def put(args, name, value):
    m = re.match(r"^(\w+)\[(\d+)\]$", name)
    if m and hasattr(args[m.group(1)], "_replace"):      # (a named tuple keeps its type: optim_step's segments)
        root = args[m.group(1)]
        args[m.group(1)] = root._replace(**{root._fields[int(m.group(2))]: value})
    elif m:
        args[m.group(1)] = list(args[m.group(1)])
        args[m.group(1)][int(m.group(2))] = value
    else:
        args[name] = value


# ---- the reference-pinned op classes ----------------------------------------------------------------------------------

def _ins(name):
    case = C.case_of(name)
    return case, C.inputs(case)


def _ordered(PC):
    """the backward sums in their defined order (PCONV.ordered_backward): the float-atomic default has no bits to hold"""
    return PC.ordered_backward(True)


def _simple(case_name, build, method, arg, key, operand_name=None, ordered=False):
    """a one-tensor method of an op built from a ref_ops case: build(PC, case) -> op"""
    def make(PC, dev):
        case, ins = _ins(case_name)
        op = build(PC, case)
        name = operand_name or arg

        def run(a):
            if ordered:
                with _ordered(PC):
                    return R(**{key: getattr(op, method)(a[name])[0]})
            return R(**{key: getattr(op, method)(a[name])[0]})
        return Case(A(dev, **{name: ins[arg]}), run, None)
    return make


def _ctx(PC, kind, case, version=None):
    wt = C.WEIGHTS[case["weight"]]
    if kind == "pseudo":
        ctx = PC.PseudoContextOp(C.NPART, 20, wt, 0, False)
    elif kind == "pentropy":
        ctx = PC.PseudoEntropyContextOp(C.NPART, 20, version, wt, 0, False)
    else:
        ctx = PC.EntropyContextOp(C.NPART, 18, wt, 0, False)
    ctx.start_context(case["w"])
    return ctx


def _keep(op, ctx):
    op._operand_ctx = ctx      # (the op borrows the context by its address string: keep it alive with the op)
    return op


row("DtowOp.forward", [X()])(_simple("dtow_s2", lambda PC, c: PC.DtowOp(c["stride"], True, 0, False), "forward", "x", "y"))
row("DtowOp.backward", [X("grad")])(
    _simple("dtow_s2", lambda PC, c: PC.DtowOp(c["stride"], False, 0, False), "backward", "x", "g", "grad"))
row("ContextReshapeOp.forward", [X()])(
    _simple("context_reshape", lambda PC, c: PC.ContextReshapeOp(c["ngroup"], 0, False), "forward", "x", "y"))


@row("ContextReshapeOp.backward", [opd("grad")])
def _context_reshape_backward(PC, dev):
    case, ins = _ins("context_reshape")
    op = PC.ContextReshapeOp(case["ngroup"], 0, False)
    x = ins["x"]
    return Case(A(dev, grad=ins["grad"]), lambda a: R(gx=op.backward(a["grad"])[0]), lambda a: op.forward(x.to(dev)))


GMM_OPERANDS = [X("weight"), opd("delta"), opd("mean"), opd("label")]


@row("EntropyGmmOp.forward", GMM_OPERANDS)
def _gmm_forward(PC, dev):
    case, ins = _ins("gmm_loss")
    op = PC.EntropyGmmOp(case["ng"], 0, 0, False)

    def run(a):
        loss = op.forward(a["weight"], a["delta"], a["mean"], a["label"])[0]
        return R(loss=loss, dw=op._top[1], dd=op._top[2], dm=op._top[3], dl=op._top[4])
    return Case(A(dev, **{k: ins[k] for k in ("weight", "delta", "mean", "label")}), run, None)


@row("EntropyGmmOp.backward", [opd("grad")])
def _gmm_backward(PC, dev):
    case, ins = _ins("gmm_loss")
    op = PC.EntropyGmmOp(case["ng"], 0, 0, False)
    good = [ins[k] for k in ("weight", "delta", "mean", "label")]

    def run(a):
        g = op.backward(a["grad"])
        return R(gw=g[0], gd=g[1], gm=g[2], gl=g[3])
    return Case(A(dev, grad=ins["top"]), run, lambda a: op.forward(*[t.to(dev) for t in good]))


def _mask(method, arg):
    def make(PC, dev):
        case, ins = _ins("mask_constrain_5")
        op = PC.MaskConstrainOp(case["constrain"], case["ngroup"], 0, False)

        def run(a):
            getattr(op, method)(a[arg])
            return R(**{arg: a[arg]})
        return Case(A(dev, **{arg: ins[arg]}), run, None)
    return make


row("MaskConstrainOp.forward", [X("w")], inplace=["w"])(_mask("forward", "w"))
row("MaskConstrainOp.backward", [X("grad")], inplace=["grad"])(_mask("backward", "grad"))

SLICE, PAD, EPAD, FILL = "slice_h1_w24_p2_nopt", "pad_h2_w40_p1_nopt_dirty", "epad_h1_w24_p2_nopt_v1", "fill_p2_h2_trim_nopt"
USLICE = "uslice_h2_w40_p1_nopt"


def _slice(PC, c):
    return PC.SphereSliceOp(C.NPART, 0, c["pad"], C.WEIGHTS[c["weight"]], 0, False)


def _uslice(PC, c):
    return PC.SphereUsliceOp(C.NPART, 0, c["pad"], C.WEIGHTS[c["weight"]], 0, False)


row("SphereSliceOp.forward", [X()])(_simple(SLICE, _slice, "forward", "x", "y"))
row("SphereSliceOp.backward", [X("grad")])(_simple(SLICE, _slice, "backward", "grad", "gx", ordered=True))
row("SphereUsliceOp.forward", [X()])(_simple(USLICE, _uslice, "forward", "x", "y"))
row("SphereUsliceOp.backward", [X("grad")])(_simple(USLICE, _uslice, "backward", "grad", "gx", ordered=True))


@row("SphereUsliceOp.forward_into", [X(), opd("out")], inplace=["out"])
def _uslice_into(PC, dev):
    case, ins = _ins(USLICE)
    op = _uslice(PC, case)
    n, c, h, w = case["n"], case["c"], case["h"], case["w"]
    out = torch.zeros(n, c, h * C.NPART, w)
    return Case(A(dev, x=ins["x"], out=out), lambda a: R(out=op.forward_into(a["x"], a["out"])), None)


def _pad(PC, c):
    ctx = _ctx(PC, "pseudo", c)
    return _keep(PC.PseudoPadOp(c["pad"], C.NPART, ctx.addr(), 0, False), ctx)


def _epad(PC, c):
    ctx = _ctx(PC, "pentropy", c, c["version"])
    return _keep(PC.PseudoEntropyPadOp(c["pad"], C.NPART, ctx.addr(), 0, False), ctx)


row("PseudoPadOp.forward", [X()])(_simple(PAD, _pad, "forward", "x", "y"))
row("PseudoPadOp.backward", [X("grad")])(_simple(PAD, _pad, "backward", "grad", "gx"))
row("PseudoEntropyPadOp.forward", [X()])(_simple(EPAD, _epad, "forward", "x", "y"))
row("PseudoEntropyPadOp.backward", [X("grad")])(_simple(EPAD, _epad, "backward", "grad", "gx"))


def _fill(method, arg, operand):
    def make(PC, dev):
        case, ins = _ins(FILL)
        ctx = _ctx(PC, "pseudo", case)
        op = _keep(PC.PseudoFillOp(case["pad"], C.NPART, case["fvalue"], case["trim"], ctx.addr(), 0, 0, False), ctx)

        def run(a):
            getattr(op, method)(a[operand])
            return R(**{operand: a[operand]})
        return Case(A(dev, **{operand: ins[arg]}), run, None)
    return make


row("PseudoFillOp.forward", [X()], inplace=["x"])(_fill("forward", "x", "x"))
row("PseudoFillOp.backward", [X("grad")], inplace=["grad"])(_fill("backward", "grad", "grad"))

QUANT = "quant_ntop2_n2_nopt"      # the h1_w24 geometry, two frames, value and index outputs


def _quant(PC, case):
    ctx = _ctx(PC, "pseudo", case)
    return _keep(PC.PseudoQuantOp(case["c"], case["bins"], C.NPART, 0.9, 1, case["ntop"], 0.1, ctx.addr(), 0, False), ctx)


# (`count` is the module's running histogram: read and written by torch arithmetic in training mode, never an address)
@row("PseudoQuantOp.forward", [X(), opd("weight"), opd("count", **{d: NOT_A_TENSOR for d in DEFORMATIONS})])
def _quant_forward(PC, dev):
    case, ins = _ins(QUANT)
    op = _quant(PC, case)

    def run(a):
        res = op.forward(a["x"], a["weight"], a["count"], False)
        return R(val=res[0], idx=res[1])
    return Case(A(dev, x=ins["x"], weight=ins["weight"], count=ins["count"]), run, None)


@row("PseudoQuantOp.backward", [opd("grads[0]", strided=HONOURED), opd("grads[1]", strided=HONOURED), X(), opd("out")])
def _quant_backward(PC, dev):
    case, ins = _ins(QUANT)
    op = _quant(PC, case)
    good = A(dev, x=ins["x"], weight=ins["weight"], count=ins["count"])

    def prepare(a):
        op.forward(good["x"], good["weight"], good["count"], False)

    def run(a):
        with _ordered(PC):
            g = op.backward(a["grads"], a["x"], a["out"])
        return R(g_in=g[0], g_w=g[1], hist=g[2])
    # (`out` stands for the forward's value output: any dense tensor of x's shape is read the same way)
    return Case(A(dev, grads=[ins["grad0"], ins["grad1"]], x=ins["x"], out=ins["x"] * 0.5), run, prepare)


@row("PseudoDQuantOp.forward", [X(), opd("weight")])
def _dquant_forward(PC, dev):
    case, ins = _ins(QUANT)
    ctx = _ctx(PC, "pseudo", case)
    op = _keep(PC.PseudoDQuantOp(C.NPART, case["c"], case["bins"], ctx.addr(), 0, False), ctx)
    g = torch.Generator().manual_seed(11)
    sym = torch.randint(0, case["bins"], tuple(ins["x"].shape), generator=g).float()
    return Case(A(dev, x=sym, weight=ins["weight"]), lambda a: R(y=op.forward(a["x"], a["weight"])[0]), None)


def _projects(PC, c):
    return PC.ProjectsOp(11, 16, C.THETA, C.PHI, 0.5, c["near"], 0, False)


row("ProjectsOp.forward", [X()])(_simple("projects_bilinear", _projects, "forward", "x", "y"))


@row("ProjectsOp.backward", [opd("grad")])
def _projects_backward(PC, dev):
    case, ins = _ins("projects_nearest")
    op = _projects(PC, case)
    x = ins["x"]

    def run(a):
        with _ordered(PC):
            g = op.backward(a["grad"])
        return R(gx=g[0], count=g[1])
    return Case(A(dev, grad=ins["grad"]), run, lambda a: op.forward(x.to(dev)))


# ---- the wavefront ops: three steps of a fresh op -------------------------------------------------------------------------

WAVE = "wave_h1_w24_g3_n2_nopt"
WAVE2 = "wave_h2_w40_g2_nopt"
STEPS = 3


def _wave(case_name, build, method, arg, key, compact=0):
    """compact: the result is a compact vector of which the op writes `compact` values per counted element (DExtract2Op:
    what lies behind them is whatever the op's buffer held)"""
    def make(PC, dev):
        case, ins = _ins(case_name)
        ctx = _ctx(PC, "entropy", case)
        op = _keep(build(PC, case, ctx.addr()), ctx)

        def run(a):
            for _ in range(STEPS):
                res = getattr(op, method)(a["x"])
            if compact:
                count = int(res[1][0])
                assert count > 0
                return R(**{key: res[0].reshape(-1)[:compact * count], "count": res[1]})
            return R(**{key: res[0]})
        return Case(A(dev, x=ins[arg] if isinstance(arg, str) else arg(case, ins)), run, None)
    return make


def _label(case, ins):
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 8, (case["n"], 1, case["h"] * C.NPART, case["w"]), generator=g).float()


row("DInput2Op.forward", [X()])(
    _wave(WAVE, lambda PC, c, addr: PC.DInput2Op(c["ngroup"], C.NPART, 2, -3.5, 3, addr, 0, False), "forward", _label, "ctx"))
row("EntropyCtxPadRun2Op.forward", [X()], inplace=["x"])(
    _wave(WAVE2, lambda PC, c, addr: PC.EntropyCtxPadRun2Op(2, C.NPART, c["ngroup"], False, addr, 0, False), "forward", "feat",
          "x"))
row("DExtract2Op.forward", [X()])(
    _wave(WAVE, lambda PC, c, addr: PC.DExtract2Op(C.NPART, c["ngroup"], True, addr, 0, False), "forward", "symbols", "top", compact=1))
row("DExtract2Op.forward_batch", [X()])(
    _wave(WAVE2, lambda PC, c, addr: PC.DExtract2Op(C.NPART, c["ngroup"], True, addr, 0, False), "forward_batch", "dense",
          "top", compact=C.case_of(WAVE2)["cpg"]))


@row("EntropyAddOp.forward", [X(), opd("y")], inplace=["x"])
def _entropy_add(PC, dev):
    case, ins = _ins(WAVE)
    ctx = _ctx(PC, "entropy", case)
    op = _keep(PC.EntropyAddOp(C.NPART, case["ngroup"] * case["cpg"], case["ngroup"], 2, ctx.addr(), 0, False), ctx)

    def run(a):
        for _ in range(STEPS):
            op.forward(a["x"], a["y"])
        return R(x=a["x"])
    return Case(A(dev, x=ins["feat"], y=ins["feat2"]), run, None)


def _econv(case_name, act):
    def make(PC, dev):
        case = C.ECONV_CASES[case_name]
        ins = C.inputs(case)
        ng = case["ngroup"]
        ctx = _ctx(PC, "entropy", case)
        op = _keep(PC.EntropyConv2Op(C.NPART, ng * case["group_in"], ng, ng * 3, 5, case["constrain"], 2, case["pad_out"],
                                     ctx.addr(), 0, False), ctx)
        names = ["x", "weight", "bias"] + (["act"] if act else [])

        def run(a):
            for _ in range(STEPS):
                res = getattr(op, case["entry"])(*[a[k] for k in names])
            return R(top=res[0])
        return Case(A(dev, **{k: ins[k] for k in names}), run, None)
    return make


ECONV = [X(), opd("weight"), opd("bias")]
# (the _batch entries take the number of weight sets from the weight's first extent)
ECONV_BATCH = [X(), opd("weight", short=DEFINES_SHAPE), opd("bias")]
row("EntropyConv2Op.forward", ECONV)(_econv("econv_plain_c5_p2_g4_i1_h1_w24_nopt", False))
row("EntropyConv2Op.forward_act", ECONV + [opd("act")])(_econv("econv_act_c6_p0_g2_i3_h2_w40", True))
row("EntropyConv2Op.forward_batch", ECONV_BATCH)(_econv("econv_batch_c6_p2_g2_i2_h1_w24_nopt_n2_s1", False))
row("EntropyConv2Op.forward_act_batch", ECONV_BATCH + [opd("act")])(_econv("econv_actbatch_c5_p0_g2_i1_h1_w40_n2_s2", True))

COUNT = dict(strided=ONE_ELEMENT, offset=NOT_A_TENSOR, dtype=NOT_A_TENSOR, device=NOT_A_TENSOR)


@row("EntropyGmmTableOp.forward", [X("weight"), opd("delta"), opd("mean"), opd("tnum", shorten=one_more, **COUNT)])
def _gmm_table(PC, dev):
    case, ins = _ins("gmm_table")
    op = PC.EntropyGmmTableOp(8, 3.5, case["ng"], 65536, 1e-6, 0, False)
    n = int(ins["tnum"][0])
    a = A(dev, weight=ins["weight"], delta=ins["delta"], mean=ins["mean"])
    # the count is read on the host: all rows, so that `short` is one more than the table was allocated for
    a["tnum"] = torch.tensor([case["rows"]], dtype=torch.int32)

    def run(a):
        table = op.forward(a["weight"], a["delta"], a["mean"], a["tnum"])[0]
        return R(table=table, weight=a["weight"], delta=a["delta"])      # (the softmax is written in place)
    return Case(a, run, None)


@row("EntropyGmmTableOp.forward_batch", [X("data"), opd("tnum", shorten=one_more, **COUNT)])
def _gmm_table_batch(PC, dev):
    case, ins = _ins("gmm_table_batch")
    op = PC.EntropyGmmTableOp(8, 3.5, case["ng"], 65536, 1e-6, 0, False)
    a = A(dev, data=ins["data"])
    a["tnum"] = torch.tensor([case["rows"]], dtype=torch.int32)

    def run(a):
        return R(table=op.forward_batch(a["data"], a["tnum"])[0], data=a["data"])
    return Case(a, run, None)


# ---- the tile convolutions and the GDN: the shapes of TILE_CONVS with two tiles -------------------------------------------

def _owner():
    return type("Owner", (), {})()


def _conv_inputs(shape, k, stride, seed=71):
    tn, cin, h, w, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tn, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / float(cin * k * k) ** 0.5)
    b, sl = torch.randn(cout, generator=g), torch.rand(cout, generator=g)
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    res, gate = torch.randn(tn, cout, ho, wo, generator=g), torch.rand(tn, cout, ho, wo, generator=g)
    limit = torch.tensor([wo - 3, wo // 2 + 1][:tn], dtype=torch.int32)
    return x, wt, b, sl, res, gate, limit


def _tile_conv(mode, shape, k, launches, gate):
    def make(PC, dev):
        tn, cin, h, w, cout = shape
        x, wt, b, sl, res, gt, limit = _conv_inputs(shape, k, 1)
        owner = _owner()

        def run(a):
            import os
            assert os.environ.get("PCONV_CONV3X3") == mode
            assert [l[0] for l in PC.conv_plan(cin, h, w, cout, k, 1, fused=gate)[0]] == launches
            y = PC.tile_conv2d(owner, a["x"], a["weight"], a["bias"], 1, a["slope"], a["col_limit"], tn,
                               gate=a.get("gate"), residual=a["residual"], trim=True)
            return R(y=y)
        args = A(dev, x=x, weight=wt, bias=b, slope=sl, col_limit=limit, residual=res)
        if gate:
            args["gate"] = gt.to(dev)
        return Case(args, run, None)
    return make


ROWS_VIEW = dict(strided=HONOURED, offset=HONOURED)      # _require_rows / _like_output: row-strided views, copies otherwise
# (cout and k are the weight's: it defines the call's shape together with x)
CONV_OPERANDS = [X(strided=HONOURED),
                 opd("weight", strided=HONOURED, short=DEFINES_SHAPE), opd("bias"), opd("slope"), opd("col_limit"), opd("residual", **ROWS_VIEW)]
for _route, _mode, _shape, _k, _launches, _gate in [
        ("direct", "direct", (2, 24, 6, 70, 64), 3, ["direct"], True),
        ("1x1", "direct", (2, 20, 5, 70, 96), 1, ["direct"], False),
        ("wino", "wino", (2, 96, 6, 66, 96), 3, ["wino"], False),
        ("wino_flat", "wino", (2, 96, 4, 70, 96), 3, ["wino_flat"], False),
        ("wino42", "wino42", (2, 24, 10, 40, 64), 3, ["wino42"], False)]:
    row("tile_conv2d", CONV_OPERANDS + ([opd("gate", **ROWS_VIEW)] if _gate else []), route=_route,
        env={"PCONV_CONV3X3": _mode})(_tile_conv(_mode, _shape, _k, _launches, _gate))


@row("tile_gdn", [X(strided=HONOURED), opd("gamma", strided=HONOURED), opd("beta", strided=HONOURED),
                  opd("col_limit"), opd("residual", **ROWS_VIEW)], env={"PCONV_CONV3X3": "direct"})
def _tile_gdn(PC, dev):
    tn, ch, h, w = 2, 24, 3, 70
    g = torch.Generator().manual_seed(77)
    x = torch.randn(tn, ch, h, w, generator=g)
    gamma = torch.rand(ch, ch, generator=g) * 0.1
    beta = torch.rand(ch, generator=g) + 0.5
    res = torch.randn(tn, ch, h, w, generator=g)
    limit = torch.tensor([w - 3, w // 2 + 1], dtype=torch.int32)
    owner = _owner()

    def run(a):
        return R(y=PC.tile_gdn(owner, a["x"], a["gamma"], a["beta"], False, a["col_limit"], tn, a["residual"]))
    return Case(A(dev, x=x, gamma=gamma, beta=beta, col_limit=limit, residual=res), run, None)


def _backward(fn, case, inputs):
    def make(PC, dev):
        x, weight, gout = inputs(case)
        stride = () if fn == "conv5x5_backward" else (case.s,)

        def run(a):
            gin, gw, gb = getattr(PC, fn)(a["x"], a["weight"], a["gout"], *stride)
            return R(gin=gin, gw=gw, gb=gb)
        return Case(A(dev, x=x, weight=weight, gout=gout), run, None)
    return make


BACKWARD_OPERANDS = [X(), opd("weight"), opd("gout")]
row("tile_conv2d_backward", BACKWARD_OPERANDS)(_backward("tile_conv2d_backward", CB.BY_NAME["c"], CB.inputs))
row("conv5x5_backward", BACKWARD_OPERANDS)(
    _backward("conv5x5_backward", MC.BY_NAME["b"], lambda c: tuple(MC.inputs(c)[i] for i in (0, 1, 3))))


@row("conv5x5", [X(), opd("weight"), opd("bias")])
def _conv5x5(PC, dev):
    x, weight, bias, _ = MC.inputs(MC.BY_NAME["b"])
    owner = _owner()
    return Case(A(dev, x=x, weight=weight, bias=bias), lambda a: R(y=PC.conv5x5(owner, a["x"], a["weight"], a["bias"])), None)


@row("leaky_clip_", [X()], inplace=["x"])
def _leaky_clip(PC, dev):
    x = torch.randn(3, 5, 7, 11, generator=torch.Generator().manual_seed(3)) * 2.0

    def run(a):
        PC.leaky_clip_(a["x"])
        return R(x=a["x"])
    return Case(A(dev, x=x), run, None)


# ---- the frame-side functions: 16 x 32 frames --------------------------------------------------------------------------

FH, FW = 16, 32


def _frames(n=2, c=3, h=FH, w=FW, seed=9):
    return torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(seed))


def _images(n=2, h=FH, w=FW, seed=2):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _with_out(fn, first, value, out_shape, out_dtype, extra=()):
    """fn(first, *extra, out=out): a function with a caller's output tensor"""
    def make(PC, dev):
        v = value()
        out = torch.zeros(out_shape(PC, v), dtype=out_dtype)

        def run(a):
            return R(out=getattr(PC, fn)(a[first], *extra, out=a["out"]))
        return Case(A(dev, **{first: v, "out": out}), run, None)
    return make


def _coded(PC, h=FH, w=FW):
    return PC.erp_coded_size(h, w)[:2]


OUT = opd("out")
row("frames_u8_to_f32", [X("img", offset=REFUSED), opd("out", offset=REFUSED)], inplace=["out"])(
    _with_out("frames_u8_to_f32", "img", _images, lambda PC, v: (2, 3, FH, FW), torch.float32))
row("frames_f32_to_u8", [X(offset=REFUSED), opd("out", offset=REFUSED)], inplace=["out"])(
    _with_out("frames_f32_to_u8", "x", _frames, lambda PC, v: (2, FH, FW, 3), torch.uint8))
row("frames_u8_to_f32_erp", [X("img"), opd("out", offset=REFUSED)], inplace=["out"])(
    _with_out("frames_u8_to_f32_erp", "img", _images, lambda PC, v: (2, 3) + _coded(PC), torch.float32))
row("erp_pad_f32", [X(), opd("out", offset=REFUSED)], inplace=["out"])(
    _with_out("erp_pad_f32", "x", _frames, lambda PC, v: (2, 3) + _coded(PC), torch.float32))


@row("frames_f32_to_u8_crop", [X(offset=REFUSED), opd("out")], inplace=["out"])
def _crop(PC, dev):
    H, W = _coded(PC)
    x = _frames(2, 3, H, W)
    out = torch.zeros(2, FH, FW, 3, dtype=torch.uint8)
    return Case(A(dev, x=x, out=out), lambda a: R(out=PC.frames_f32_to_u8_crop(a["x"], FH, FW, out=a["out"])), None)


@row("erp_remap_f32", [X(), opd("map", offset=REFUSED), opd("out")], inplace=["out"])
def _remap(PC, dev):
    from pseudocylindrical_convolution_amd import erp_rotate
    x = _frames()
    q = torch.from_numpy(erp_rotate.source_map_numpy(FH, FW, erp_rotate.units(30, 20, 10), False))
    out = torch.zeros(2, 3, FH, FW)
    return Case(A(dev, x=x, map=q, out=out), lambda a: R(out=PC.erp_remap_f32(a["x"], a["map"], out=a["out"])), None)


@row("erp_resample_f32", [X(), opd("out"), opd("workspace", offset=REFUSED)], inplace=["out"])
def _resample(PC, dev):
    x = _frames()
    h2, w2 = 12, 22
    out = torch.zeros(2, 3, h2, w2)

    def make_args():
        from pseudocylindrical_convolution_amd import _native
        nbytes = int(_native.hip_lib().pconv_erp_resample_workspace_bytes(2, 3, FH, FW, h2, w2))
        return A(dev, x=x, out=out, workspace=torch.zeros(nbytes, dtype=torch.uint8))
    return Case(make_args(), lambda a: R(out=PC.erp_resample_f32(a["x"], h2, w2, out=a["out"], workspace=a["workspace"])), None)


def _ws_pair():
    return _frames(seed=9), _frames(seed=10)


@row("ws_metrics_device", [X(), opd("y")], op="ws_metrics")
def _ws_metrics_device(PC, dev):
    x, y = _ws_pair()
    return Case(A(dev, x=x, y=y), lambda a: R(v=PC.ws_metrics_device(a["x"], a["y"])), None)


@row("ws_metrics", [X(), opd("y")])
def _ws_metrics(PC, dev):
    x, y = _ws_pair()
    return Case(A(dev, x=x, y=y), lambda a: R(v=PC.ws_metrics(a["x"], a["y"])), None)


@row("ws_metrics_backward", [X(), opd("y"), opd("gout")])
def _ws_metrics_backward(PC, dev):
    x, y = _ws_pair()
    gout = torch.rand(2, 2, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    return Case(A(dev, x=x, y=y, gout=gout), lambda a: R(g=PC.ws_metrics_backward(a["x"], a["y"], a["gout"])), None)


@row("ws_msssim_device", [X(), opd("y")], op="ws_msssim")
def _ws_msssim_device(PC, dev):
    x, y = _ws_pair()

    def run(a):
        values, workspace = PC.ws_msssim_device(a["x"], a["y"])
        return R(values=values, workspace=workspace)
    return Case(A(dev, x=x, y=y), run, None)


@row("ws_msssim", [X(), opd("y")])
def _ws_msssim(PC, dev):
    x, y = _ws_pair()

    def run(a):
        values, workspace = PC.ws_msssim(a["x"], a["y"])
        return R(values=values, workspace=workspace)
    return Case(A(dev, x=x, y=y), run, None)


@row("ws_msssim_backward", [X(), opd("y"), opd("workspace", offset=REFUSED), opd("values"), opd("gout")])
def _ws_msssim_backward(PC, dev):
    from pseudocylindrical_convolution_amd import _native
    x, y = _ws_pair()
    gout = torch.rand(2, 2, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    args = A(dev, x=x, y=y)
    if torch.device(dev).type == "cuda":      # (what the forward returned for x and y)
        args["values"], args["workspace"] = PC.ws_msssim_device(args["x"], args["y"])
    else:                                     # (the table's own checks, without a GPU: tensors of the right kinds)
        nbytes = int(_native.hip_lib().pconv_ws_msssim_workspace_bytes(2, 3, FH, FW))
        args["values"], args["workspace"] = torch.zeros(2, 7, dtype=torch.float64), torch.zeros(nbytes, dtype=torch.uint8)
    args["gout"] = gout.to(dev)
    args.move_to_end("values")
    args.move_to_end("gout")
    return Case(args, lambda a: R(g=PC.ws_msssim_backward(a["x"], a["y"], a["workspace"], a["values"], a["gout"])), None)


@row("erp_resample_backward_f32", [X("g"), opd("gin"), opd("workspace", offset=REFUSED)], inplace=["gin"])
def _resample_backward(PC, dev):
    from pseudocylindrical_convolution_amd import _native
    h2, w2 = 12, 22
    g = _frames(2, 3, h2, w2, seed=12)
    nbytes = int(_native.hip_lib().pconv_erp_resample_backward_workspace_bytes(2, 3, FH, FW, h2, w2))
    args = A(dev, g=g, gin=torch.zeros(2, 3, FH, FW), workspace=torch.zeros(nbytes, dtype=torch.uint8))
    return Case(args, lambda a: R(gin=PC.erp_resample_backward_f32(a["g"], FH, FW, gin=a["gin"], workspace=a["workspace"])), None)


YH, YW = 4, 6      # (the frames of tests/test_gpu_yuv.py's smallest case)


@row("frames_yuv420_to_f32", [X("buf"), opd("out", offset=REFUSED)], inplace=["out"])
def _yuv_in(PC, dev):
    buf = torch.randint(16, 236, (2, YH * YW * 3 // 2), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    out = torch.zeros((2, 3) + _coded(PC, YH, YW))
    return Case(A(dev, buf=buf, out=out), lambda a: R(out=PC.frames_yuv420_to_f32(a["buf"], YH, YW, "yuv420p", out=a["out"])), None)


@row("frames_f32_to_yuv420", [X(offset=REFUSED), opd("out")], inplace=["out"])
def _yuv_out(PC, dev):
    x = _frames(2, 3, *_coded(PC, YH, YW))
    out = torch.zeros(2, YH * YW * 3 // 2, dtype=torch.uint8)
    return Case(A(dev, x=x, out=out), lambda a: R(out=PC.frames_f32_to_yuv420(a["x"], YH, YW, "yuv420p", out=a["out"])), None)


# ---- maps, views, cube faces, sphere points ---------------------------------------------------------------------------------

def _view():
    from pseudocylindrical_convolution_amd import viewport
    return viewport.view(30.0, 20.0, 10.0, 90.0, 60.0)


VH, VW, SS = 4, 6, 2
CUBE_A = 4
MAP_OUT = [opd("out", offset=REFUSED)]      # (a map is read and written as 8-byte records)


def _map(fn, shape, call):
    def make(PC, dev):
        def run(a):
            return R(out=call(PC, a["out"]))
        return Case(A(dev, out=torch.zeros(shape, dtype=torch.int32)), run, None)
    return make


def _rotation():
    from pseudocylindrical_convolution_amd import erp_rotate
    return erp_rotate.units(30, 20, 10)


row("erp_rotation_map", MAP_OUT, inplace=["out"])(
    _map("erp_rotation_map", (FH, FW, 2), lambda PC, out: PC.erp_rotation_map(FH, FW, _rotation(), out=out)))
row("viewport_map", MAP_OUT, inplace=["out"])(
    _map("viewport_map", (VH * SS, VW * SS, 2), lambda PC, out: PC.viewport_map(FH, FW, VH * SS, VW * SS, _view(), out=out)))
row("cube_from_erp_map", MAP_OUT, inplace=["out"])(
    _map("cube_from_erp_map", (6 * CUBE_A, CUBE_A, 2), lambda PC, out: PC.cube_from_erp_map("cmp", CUBE_A, 1, FH, FW, out=out)))
row("cube_to_erp_map", MAP_OUT, inplace=["out"])(
    _map("cube_to_erp_map", (FH, FW, 2), lambda PC, out: PC.cube_to_erp_map("cmp", CUBE_A, FH, FW, 1, out=out)))


def _view_map():
    from pseudocylindrical_convolution_amd import viewport
    return torch.from_numpy(viewport.source_map_numpy(FH, FW, VH * SS, VW * SS, _view()))


@row("viewport_render_f32", [X(), opd("map", offset=REFUSED), opd("out")], inplace=["out"])
def _render(PC, dev):
    args = A(dev, x=_frames(), map=_view_map(), out=torch.zeros(2, 1, 3, VH, VW))
    return Case(args, lambda a: R(out=PC.viewport_render_f32(a["x"], a["map"], VH, VW, SS, out=a["out"])), None)


@row("remap_backward_f32", [X("gout"), opd("map", offset=REFUSED), opd("lists[0]"), opd("lists[1]"), opd("gin")], inplace=["gin"])
def _remap_backward(PC, dev):
    from pseudocylindrical_convolution_amd import viewport
    q = _view_map()
    lists = [t.cpu() for t in viewport.reverse_lists(q, FH, FW)]
    gout = _frames(2, 3, VH, VW, seed=13)
    args = A(dev, gout=gout, map=q, lists=lists, gin=torch.zeros(2, 3, FH, FW))
    return Case(args, lambda a: R(gin=PC.remap_backward_f32(a["gout"], a["map"], a["lists"], FH, FW, VH, VW, SS, gin=a["gin"])),
                None)


@row("cube_pad_f32", [X(), opd("table"), opd("out")], inplace=["out"])
def _cube_pad(PC, dev):
    import numpy as np
    from pseudocylindrical_convolution_amd import cube
    table = torch.as_tensor(np.array(cube.pad_table("cmp", CUBE_A)))
    A6 = CUBE_A + 6
    args = A(dev, x=_frames(2, 3, 6 * CUBE_A, CUBE_A), table=table, out=torch.zeros(2, 3, 6 * A6, A6))
    return Case(args, lambda a: R(out=PC.cube_pad_f32(a["x"], a["table"], out=a["out"])), None)


def _points():
    import sphere_points_cases as K
    import numpy as np
    return torch.from_numpy(np.array(K.pointset("ico2").points))


def _records(h=FH, w=FW):
    import sphere_points_cases as K
    from pseudocylindrical_convolution_amd import sphere_points
    return torch.from_numpy(sphere_points.records_numpy(K.pointset("ico2"), h, w))


@row("sphere_points_records", [X("points"), opd("out", offset=REFUSED)], inplace=["out"])
def _points_records(PC, dev):
    pts = _points()
    args = A(dev, points=pts, out=torch.zeros(pts.shape[0], 2, dtype=torch.int32))
    return Case(args, lambda a: R(out=PC.sphere_points_records(a["points"], FH, FW, out=a["out"])), None)


# (the number of points is the records': they define the call's shape together with x)
@row("sphere_points_sample_f32", [X(), opd("records", offset=REFUSED, short=DEFINES_SHAPE), opd("out")], inplace=["out"])
def _points_sample(PC, dev):
    rec = _records()
    args = A(dev, x=_frames(), records=rec, out=torch.zeros(2, 3, rec.shape[0]))
    return Case(args, lambda a: R(out=PC.sphere_points_sample_f32(a["x"], a["records"], out=a["out"])), None)


def _points_mse(fn):
    def make(PC, dev):
        args = A(dev, x=_frames(), rec_x=_records(), y=_frames(2, 3, 8, 16, seed=14), rec_y=_records(8, 16))
        return Case(args, lambda a: R(mse=getattr(PC, fn)(a["x"], a["rec_x"], a["y"], a["rec_y"])), None)
    return make


MSE_OPERANDS = [X(), opd("rec_x", offset=REFUSED, short=DEFINES_SHAPE), opd("y"), opd("rec_y", offset=REFUSED)]
row("sphere_points_mse_device", MSE_OPERANDS, op="sphere_points_mse")(_points_mse("sphere_points_mse_device"))
row("sphere_points_mse", MSE_OPERANDS)(_points_mse("sphere_points_mse"))


# ---- ring outputs, the ring-only pad, the weight pack, the optimiser step -----------------------------------------------------

RING = 2
RING_FILL = "B"      # every torch.empty of the call is filled with stale_memory's pattern B: the ring must still hold it


def _ring_of(y):
    """(the ring elements of the padded buffer behind a ring output, as one vector; the interior, dense)"""
    buf, ring = y._pconv_ring
    mask = torch.ones(buf.shape[2:], dtype=torch.bool, device=buf.device)
    mask[ring:-ring, ring:-ring] = False
    return buf[:, :, mask], y.contiguous()


def _filled_ring_call(fn):
    """fn() -> a ring output, made under the fill: the interior, and the ring, which nothing but the fill may have written"""
    import pytest
    import stale_memory as SM
    with SM.filled(pytest.MonkeyPatch(), RING_FILL):
        y = fn()
    ring, interior = _ring_of(y)
    assert y._pconv_ring[1] == RING and bool(SM.holds_pattern(ring, RING_FILL).all()), "wrote outside the view: the ring"
    assert not bool(SM.holds_pattern(interior, RING_FILL).any())
    return R(y=interior, ring=ring)


def _tile_conv_ring(PC, dev):
    shape, k = (2, 24, 6, 70, 64), 3
    tn, cin, h, w, cout = shape
    x, wt, b, sl, res, gt, limit = _conv_inputs(shape, k, 1)
    owner = _owner()

    def run(a):
        return _filled_ring_call(lambda: PC.tile_conv2d(owner, a["x"], a["weight"], a["bias"], 1, a["slope"], a["col_limit"], tn,
                                                        residual=a["residual"], trim=True, ring=RING))
    return Case(A(dev, x=x, weight=wt, bias=b, slope=sl, col_limit=limit, residual=res), run, None)


row("tile_conv2d", CONV_OPERANDS, route="direct-ring2", env={"PCONV_CONV3X3": "direct"})(_tile_conv_ring)


@row("tile_gdn", [X(strided=HONOURED), opd("gamma", strided=HONOURED), opd("beta", strided=HONOURED),
                  opd("col_limit"), opd("residual", **ROWS_VIEW)], route="ring2", env={"PCONV_CONV3X3": "direct"})
def _tile_gdn_ring(PC, dev):
    base = _tile_gdn(PC, dev)
    owner = _owner()

    def run(a):
        return _filled_ring_call(lambda: PC.tile_gdn(owner, a["x"], a["gamma"], a["beta"], False, a["col_limit"], 2,
                                                     a["residual"], RING))
    return Case(base.args, run, None)


# x is the tagged interior view itself: every deformed copy (which the harness tags with the same buffer) is no view of
# that buffer, and the ring-only pad would pad the buffer and never read the copy
@row("PseudoPadOp.forward_ring", [X(strided=REFUSED, offset=REFUSED)])
def _forward_ring(PC, dev):
    case, ins = _ins(PAD)
    ctx = _ctx(PC, "pseudo", case)
    op = _keep(PC.PseudoPadOp(case["pad"], C.NPART, ctx.addr(), 0, False), ctx)
    tn, c, h, w = ins["x"].shape
    buf = torch.full((tn, c, h + 2 * RING, w + 2 * RING), SENTINEL).to(dev)
    view = buf[:, :, RING:-RING, RING:-RING]
    view.copy_(ins["x"].to(dev))
    view._pconv_ring = (buf, RING)
    args = collections.OrderedDict(x=view)
    return Case(args, lambda a: R(y=op.forward_ring(a["x"])), None)


@row("packed_conv_weight", [X("weight", strided=HONOURED)])
def _packed_conv_weight(PC, dev):
    wt = _conv_inputs((2, 24, 6, 70, 64), 3, 1)[1]
    owner = _owner()
    def run(a):
        stream = PC._stream(torch.device("cuda", torch.cuda.current_device()))
        return R(packed=PC.packed_conv_weight(owner, a["weight"], stream))
    return Case(A(dev, weight=wt), run, None)


# records: one row of nine 8-byte words per tensor (addresses of parameter, gradient, accumulator, the two moments, the
# element count, six fp32 scalars); segments: the table of optim_segments.  The tensors the step writes through those
# addresses -- parameter and moments -- lie one element inside sentinel buffers, one spare element at either end
@row("optim_step", [opd("records"), opd("segments[0]")])
def _optim_step(PC, dev):
    import numpy as np
    from pseudocylindrical_convolution_amd import optim
    sizes = [3, 255, 4097]
    g = torch.Generator().manual_seed(21)
    bufs = [[torch.full((n + 2,), SENTINEL).to(dev) for _ in range(4)] for n in sizes]      # p, grad, m, v
    for row_bufs, n in zip(bufs, sizes):
        for k, t in enumerate(row_bufs):
            v = torch.randn(n, generator=g) * (1.0 if k == 0 else 0.1)
            t[1:n + 1] = (v.abs() if k == 3 else v).to(dev)
    inside = [[t[1:n + 1] for t in row_bufs] for row_bufs, n in zip(bufs, sizes)]
    ints = np.array([[p.data_ptr(), gr.data_ptr(), 0, m.data_ptr(), v.data_ptr(), p.numel()] for p, gr, m, v in inside],
                    dtype=np.int64)
    floats = np.array([optim._scalars(1e-3, 0.9, 0.999, 1e-8, 1.0)] * len(sizes), dtype=np.float32)
    records = torch.from_numpy(np.concatenate([ints, floats.view(np.int64)], axis=1)).to(dev)
    args = collections.OrderedDict(records=records, segments=PC.optim_segments(sizes, dev))

    def run(a):
        ws = PC.optim_step(a["records"], a["segments"], 0.1, torch.device(dev))
        # (total and norm; the clip coefficient is the low fp32 half of the third word, whose high half nothing writes)
        out = R(figures=ws[:2].clone(), coef=ws[2:3].view(torch.float32)[:1].clone())
        for i, (p, gr, m, v) in enumerate(inside):
            out["p%d" % i], out["m%d" % i], out["v%d" % i] = p, m, v
        ends = torch.stack([t[j] for row_bufs in bufs for t in row_bufs for j in (0, -1)])
        assert bool((ends == SENTINEL).all()), "wrote outside the tensors of the records"
        out["ends"] = ends
        return out
    return Case(args, run, None)


# ---- what has no row ---------------------------------------------------------------------------------------------------

# public entries that take a tensor and turn it into an address without a row: none (the completeness test holds it empty)
NOT_SWEPT = {}
# public entries that take no tensor, or read only its device / its values on the host
NO_ADDRESS = {
    "tile_widths": "a host list of weights", "conv_col_limit": "`like` gives the device of the table",
    "conv3x3_mode": "no operand", "conv_plan": "integers", "conv_kernel_name": "integers", "erp_coded_size": "integers",
    "optim_segments": "a host list of counts", "ws_msssim_levels": "views of the workspace, no call of the library",
    "PseudoQuantOp.update_weight": "torch arithmetic on the parameters, no address is taken",
    "EntropyCtxPadRun2Op.backward": "returns nothing, reads nothing",
}
# methods every op class shares that take no tensor (or only `like`, for its device)
SHARED_METHODS = ("to", "addr", "start_context", "widths_host", "widths", "produce_fill_param", "restart", "pad_tables",
                  "pad_reverse_tables", "causal_tables", "causal_reverse_tables", "schedule", "schedule_device",
                  "causal_halo")


def public_entries(PC):
    """every public function of PCONV.py and every public method of its public classes, as 'name' / 'Class.method'"""
    out = []
    for name, obj in vars(PC).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != PC.__name__:
            continue
        if inspect.isfunction(obj):
            out.append(name)
        elif inspect.isclass(obj) and name in PC.__all__:
            for m, f in inspect.getmembers(obj, inspect.isfunction):
                if not m.startswith("_") and m not in SHARED_METHODS:
                    out.append("%s.%s" % (name, m))
    return sorted(out)


def parameters(PC, entry):
    obj = PC
    for part in entry.split("."):
        obj = getattr(obj, part)
    return [p for p in inspect.signature(obj).parameters if p != "self"]


def tensor_arguments(args):
    """the names of the tensors among a recipe's arguments ('root[i]' for the members of a list)"""
    names = []
    for k, v in args.items():
        if isinstance(v, torch.Tensor):
            names.append(k)
        elif isinstance(v, (list, tuple)):
            names += ["%s[%d]" % (k, i) for i, t in enumerate(v) if isinstance(t, torch.Tensor)]
    return names


def incomplete(PC, rows=None, not_swept=None, no_address=None):
    """what is wrong with the table, one line each: a public entry with no row, a row for no entry, an argument that
    holds a tensor and is no named operand, an operand with a deformation that has neither outcome nor reason"""
    rows = ROWS if rows is None else rows
    not_swept = NOT_SWEPT if not_swept is None else not_swept
    no_address = NO_ADDRESS if no_address is None else no_address
    bad, public = [], public_entries(PC)
    listed = [r.entry for r in rows] + list(not_swept) + list(no_address)
    for entry in public:
        if entry not in listed:
            bad.append("%s: a public entry point with no row" % entry)
    for entry in sorted(set(listed)):
        if entry not in public:
            bad.append("%s: listed, but PCONV.py has no such public entry point" % entry)
    for entry in sorted(set(r.entry for r in rows) & (set(not_swept) | set(no_address))):
        bad.append("%s: has a row and is listed as having none" % entry)
    for r in rows:
        if r.entry not in public:
            continue
        case = r.make(PC, "cpu")
        params = parameters(PC, r.entry)
        named = [o.name for o in r.operands]
        for k in case.args:
            if k not in params:
                bad.append("%s: the recipe fills %r, which is no parameter" % (row_id(r), k))
        for name in tensor_arguments(case.args):
            if name not in named:
                bad.append("%s: %s holds a tensor and is no named operand" % (row_id(r), name))
        for o in r.operands:
            if re.sub(r"\[\d+\]$", "", o.name) not in case.args:
                bad.append("%s: operand %s is not among the recipe's arguments" % (row_id(r), o.name))
            for d in DEFORMATIONS:
                reason = o.na.get(d)
                if reason is not None and reason not in REASONS:
                    bad.append("%s: %s/%s: %r is none of the three reasons" % (row_id(r), o.name, d, reason))
                if reason is None and d in ("strided", "offset") and getattr(o, d) not in (HONOURED, REFUSED):
                    bad.append("%s: %s/%s has no pinned outcome" % (row_id(r), o.name, d))
                if reason is None and d == "short" and o.short is None:
                    bad.append("%s: %s/short has neither a form nor a reason" % (row_id(r), o.name))
        for name in r.inplace:
            if name not in named:
                bad.append("%s: in-place operand %s is not named" % (row_id(r), name))
    return bad


def cases(rows=None):
    """[(row, operand, deformation)] that run, and [(row, operand, deformation, reason)] that do not apply"""
    run, na = [], []
    for r in (ROWS if rows is None else rows):
        for o in r.operands:
            for d in DEFORMATIONS:
                if d in o.na:
                    na.append((r, o, d, o.na[d]))
                else:
                    run.append((r, o, d))
    return run, na


def case_id(c):
    return "%s-%s-%s" % (row_id(c[0]), c[1].name, c[2])


# ---- the harness -------------------------------------------------------------------------------------------------------

def _refusal_names(r, o, message):
    if not message.startswith(r.op):
        return "the refusal does not begin with the op's name %s: %r" % (r.op, message)
    if len(r.operands) > 1 and not re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(re.sub(r"\[\d+\]$", "", o.name)),
                                             message):
        return "the refusal does not name the operand %s: %r" % (o.name, message)
    return None


def _results(PC, patch, run, args):
    """the call's results as bits, and the entry points it called in the library, in order"""
    names, real = [], PC.call

    def traced(fn, *a):
        names.append(fn)
        return real(fn, *a)
    with patch.context() as m:
        m.setattr(PC, "call", traced)
        out = run(args)
    return collections.OrderedDict((k, (bits(v), v.dtype, tuple(v.shape))) for k, v in out.items()), names


def _same(got, ref, what):
    assert list(got) == list(ref), (what, list(got), list(ref))
    for k in ref:
        assert got[k][1:] == ref[k][1:], "%s: %s is %s %s, dense: %s %s" % ((what, k) + got[k][1:] + ref[k][1:])
        if not torch.equal(got[k][0], ref[k][0]):
            bad = got[k][0] != ref[k][0]
            raise AssertionError("%s: %s: %d of %d elements differ in their bits from the call with a dense operand"
                                 % (what, k, int(bad.sum()), bad.numel()))


def _gaps_hold(view, buf, form, what):
    """every element of the buffer behind `view` that the view does not cover still holds the sentinel"""
    s = _sentinel(buf.dtype)
    if form == "offset":
        gap = buf[:1]
    elif form == "wide":
        gap = buf[..., 1::2]
    else:
        return
    assert bool((gap == s).all()), "%s: wrote outside the view (%d gap elements changed)" % (what, int((gap != s).sum()))


def _tag_like(deformed, t):
    """a tensor tagged as the interior view of a ring buffer hands its tag to its deformed copy: what stands in its place
    claims the same buffer"""
    if hasattr(t, "_pconv_ring"):
        deformed._pconv_ring = t._pconv_ring


def check(PC, r, o, deformation, dev, elsewhere, patch):
    """the (row, operand, deformation) case against the contract; raises AssertionError (Reached for a refused operand
    that got to the library).  PC: the module under test (PconvError, call, _backward_call, _native.call); dev: where
    well-formed operands live; elsewhere: the device of the `device` deformation; patch: pytest's monkeypatch"""
    what = "%s, %s, %s" % (row_id(r), o.name, deformation)
    assert deformation not in o.na, what
    for k, v in r.env.items():
        patch.setenv(k, v)
    if deformation in ("strided", "offset"):
        expected = getattr(o, deformation)
        base = r.make(PC, dev)
        if base.prepare:
            base.prepare(base.args)
        ref, ref_calls = _results(PC, patch, base.run, base.args)
        probe = get(r.make(PC, "cpu").args, o.name)
        forms = [f[0] for f in strided_forms(probe)] if deformation == "strided" else ["offset"]
        for form in forms:
            case = r.make(PC, dev)
            t = get(case.args, o.name)
            if deformation == "strided":
                view, buf = [f[1:] for f in strided_forms(t) if f[0] == form][0]
                assert not view.is_contiguous(), what
            else:
                view, buf = offset_form(t)
                assert view.is_contiguous() and view.data_ptr() % (2 * view.element_size()) != 0, what
            assert dense_read_covered(view) and tuple(view.shape) == tuple(t.shape), what
            _tag_like(view, t)
            put(case.args, o.name, view)
            if case.prepare:
                case.prepare(case.args)
            try:
                got, calls = _results(PC, patch, case.run, case.args)
            except PC.PconvError as e:
                assert expected == REFUSED, "%s (%s): refused, the table says honoured: %s" % (what, form, e)
                if deformation == "strided":
                    wrong = _refusal_names(r, o, str(e))
                    assert wrong is None, "%s (%s): %s" % (what, form, wrong)
                continue
            assert expected == HONOURED, "%s (%s): ran, the table says refused" % (what, form)
            assert calls == ref_calls, "%s (%s): the library calls %s, with a dense operand %s" % (what, form, calls, ref_calls)
            _same(got, ref, "%s (%s)" % (what, form))
            if o.name in r.inplace:
                _gaps_hold(view, buf, form, "%s (%s)" % (what, form))
        return
    case = r.make(PC, dev)
    if case.prepare:
        case.prepare(case.args)
    t = get(case.args, o.name)
    if deformation == "dtype":
        bad = other_dtype(t)
        assert bad.dtype != t.dtype and tuple(bad.shape) == tuple(t.shape)
    elif deformation == "device":
        bad = other_device(t, elsewhere)
        assert bad.device != t.device
    else:
        bad = o.short(t)
        assert bad.numel() < t.numel() or o.short is one_more
    _tag_like(bad, t)
    put(case.args, o.name, bad)

    def recorder(fn, *args):
        raise Reached("reached the library with a refused operand: %s, %s, %s (%s)" % (row_id(r), o.name, deformation, fn))

    patch.setattr(PC, "call", recorder)
    patch.setattr(PC, "_backward_call", recorder)
    patch.setattr(PC._native, "call", recorder)
    try:
        case.run(case.args)
    except PC.PconvError as e:
        wrong = _refusal_names(r, o, str(e))
        assert wrong is None, "%s: %s" % (what, wrong)
        return
    except Reached:
        raise
    except Exception as e:
        raise AssertionError("%s: not refused by the wrapper: %s: %s" % (what, type(e).__name__, e))
    raise AssertionError("%s: not refused: the call returned" % what)
