"""Cases of the optimiser step shared by the CPU tests (the numpy twin of optim.Adam) and the GPU tests (csrc/optim.hip),
and the float64 reference: torch.optim.Adam on float64 copies with clip_grad_norm_.

A case is a list of tensor shapes in parameter groups; its parameters, and the gradient and the accumulator of every
step, are functions of (case, step) alone, so that every runner sees the same numbers."""
import collections

import numpy as np
import torch

Case = collections.namedtuple("Case", "name shapes lrs skipped edge")
#   shapes: one list of shapes per parameter group; lrs: one lr per group; skipped: index (over all parameters) of the
#   parameter whose gradient is None, or None; edge: None, "small", "inf" or "nan"

# short quads (1, 3, 255, 1023), short segments (4095, 4097), several segments, a 4-D tensor
SIZES = [(1,), (3,), (255,), (256 * 4 - 1,), (4095,), (4096,), (4097,), (3 * 4096 + 5,), (16, 16, 3, 3)]

CASES = [
    Case("sizes", [SIZES], [1e-3], None, None),
    Case("many", [[(4 * 4096 + 1,)] * 70], [1e-3], None, None),       # 350 segments: the closing launch strides
    Case("skipped", [SIZES], [1e-3], 2, None),                        # one gradient is None
    Case("groups", [SIZES[:5], SIZES[5:]], [1e-3, 1e-2], None, None),  # two learning rates
    Case("small", [[(4097,), (7,)]], [1e-3], None, "small"),          # subnormals, +-0, 2^-80-scaled values
    Case("inf", [[(4097,), (7,)]], [1e-3], None, "inf"),
    Case("nan", [[(4097,), (7,)]], [1e-3], None, "nan"),
]
BY_NAME = {c.name: c for c in CASES}

CLIP_BINDS, CLIP_LOOSE = 0.1, 1e6   # against gradient norms of 1 .. 100 (not the edge lists: whatever they give)


def _flat_shapes(case):
    return [s for group in case.shapes for s in group]


def _gen(case, what, step):
    return torch.Generator().manual_seed(1000 * CASES.index(case) + 10 * step + what)


def _small(x):
    """the values of x replaced, in a cycle of 5: a subnormal, its negative, +0, -0, x * 2^-80"""
    flat = x.reshape(-1).clone()
    k = torch.arange(flat.numel()) % 5
    sub = torch.tensor(1e-41, dtype=torch.float32)
    flat = torch.where(k == 0, sub, flat * 2.0 ** -80)
    flat = torch.where(k == 1, -sub, flat)
    flat = torch.where(k == 2, torch.tensor(0.0), flat)
    flat = torch.where(k == 3, torch.tensor(-0.0), flat)
    return flat.reshape(x.shape)


def parameters(case):
    """[[float32 CPU tensor]] per group, values of order 1"""
    g = _gen(case, 0, 0)
    return [[torch.randn(s, generator=g) for s in group] for group in case.shapes]


def gradients(case, step):
    """the float32 CPU gradients of `step` over all parameters (None for the skipped one)"""
    g = _gen(case, 1, step)
    out = [torch.randn(s, generator=g) * 0.1 for s in _flat_shapes(case)]
    if case.edge == "small":
        out = [_small(x) for x in out]
    if case.edge in ("inf", "nan"):
        out[0].view(-1)[5] = float(case.edge)
    if case.skipped is not None:
        out[case.skipped] = None
    return out


def accumulators(case, step):
    g = _gen(case, 2, step)
    out = [torch.randn(s, generator=g) * 0.1 for s in _flat_shapes(case)]
    return [_small(x) for x in out] if case.edge == "small" else out


def moments(case):
    """(exp_avg, exp_avg_sq) an edge list starts from, else None: small values of both signs / not below zero"""
    if case.edge != "small":
        return None
    g = _gen(case, 3, 0)
    m = [_small(torch.randn(s, generator=g)) for s in _flat_shapes(case)]
    return m, [x.abs() for x in m]


def build(case, make_optimizer, device="cpu", dtype=torch.float32):
    """(parameters as leaf tensors over all groups, the optimiser over them in the case's groups)"""
    groups = [[p.to(device=device, dtype=dtype).requires_grad_() for p in group] for group in parameters(case)]
    opt = make_optimizer([{"params": ps, "lr": lr} for ps, lr in zip(groups, case.lrs)])
    params = [p for ps in groups for p in ps]
    start = moments(case)
    if start is not None:
        for p, m, v in zip(params, *start):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m.to(device=device, dtype=dtype),
                            "exp_avg_sq": v.to(device=device, dtype=dtype)}
    return params, opt


def set_gradients(case, step, params):
    for p, g in zip(params, gradients(case, step)):
        p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype)


def torch_steps(case, steps, with_acc, clip, dtype):
    """what train.py's default path does, `steps` times, in `dtype` on the CPU: grad += acc, clip_grad_norm_ (clip > 0),
    torch.optim.Adam.step.  Returns (parameters, optimiser, the gradient norm of every step)"""
    params, opt = build(case, lambda groups: torch.optim.Adam(groups), dtype=dtype)
    norms = []
    for step in range(steps):
        set_gradients(case, step, params)
        live = [p for p in params if p.grad is not None]
        if with_acc:
            for p, a in zip(params, accumulators(case, step)):
                if p.grad is not None:
                    p.grad += a.to(dtype)
        norms.append(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in live])))
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(live, clip)
        opt.step()
    return params, opt, norms


def native_steps(case, steps, with_acc, clip, device="cpu"):
    """optim.Adam.step(acc, clip), `steps` times on `device`.  Returns (parameters, optimiser, the accumulators after
    the last step or None, [(total, norm, coef)] of every step as CPU tensors)"""
    from pseudocylindrical_convolution_amd import optim
    params, opt = build(case, lambda groups: optim.Adam(groups), device=device)
    accs, figures = None, []
    for step in range(steps):
        set_gradients(case, step, params)
        accs = [a.to(device) for a in accumulators(case, step)] if with_acc else None
        opt.step(acc=accs, clip=clip)
        figures.append(tuple(t.cpu().clone() for t in (opt.last_total, opt.last_grad_norm, opt.last_coef)))
    return params, opt, accs, figures


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    """a and b hold the same bit patterns; a NaN matches a NaN of any payload (which payload an operation hands on
    is the processor's choice, not the definition's)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = a.isnan()
    return bool(torch.equal(nan, b.isnan()) and torch.equal(bits(a)[~nan], bits(b)[~nan]))


def states(opt, params):
    return [opt.state.get(p, {}) for p in params]
