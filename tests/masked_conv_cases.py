"""Shared by tests/test_masked_conv_cpu.py and tests/test_gpu_masked_conv.py: the shapes the native masked 5x5
convolution (pconv_conv5*, PCONV.conv5x5 / conv5x5_backward) is held at, their inputs with the causal mask applied, and
its CPU twins.

The weight is masked by the unmodified oracle.pconv_cpu.MaskConstrainOp (constrain 5: the first layer, one input
channel per group; constrain 6: a hidden layer, three) -- the kernels take the masked weight as it is: every tap,
zero or not, is a step of the chain.

  forward          oracle.pconv_cpu.conv2d_chain(x, w_masked, bias, 1): one fmaf chain over (ci, kh, kw) ascending
  backward         twin_dgrad / twin_wgrad / twin_bgrad, f64_grads and bounds of tests/conv_backward_cases.py, which are
                   generic in k: the orders of the 1x1 / 3x3 backward taken at k = 5
"""
import collections

import torch

import conv_backward_cases as B

# (the fields conv_backward_cases.bounds / out_size read, then the mask's)
Case = collections.namedtuple("Case", "name k s cin cout h w tn need_x edges G constrain")


def _case(name, G, hidden, tn, h, w, need_x=True, edges=False):
    return Case(name, 5, 1, 3 * G if hidden else G, 3 * G, h, w, tn, need_x, edges, G, 6 if hidden else 5)


# each the smallest shape at which something can break
CASES = [
    _case("a", 14, True, 3, 8, 70),         # wo = 66 crosses a 64-pixel run; 42 couts are ragged against 32 / 96-cout blocks
    _case("b", 14, False, 2, 6, 37),        # the first layer: one channel per group, odd wo = 33 (the (-0, +0) step)
    _case("c", 28, True, 2, 6, 22),         # several K chunks
    _case("d", 48, True, 1, 5, 21),         # ho = 1; two cout blocks; the widest model
    _case("e", 14, True, 2, 36, 134),       # a 4160-step chain per weight-gradient partial (ho * wo = 32 * 130)
    _case("f", 14, False, 2, 6, 37, edges=True),    # as b at fp32's edges: subnormals, +-0, underflowing products
    _case("g", 14, True, 3, 8, 70, need_x=False),   # as a: the first layer's input is the symbols and needs no gradient
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

out_size = B.out_size
bits = B.bits
bounds = B.bounds
f64_grads = B.f64_grads


def masked(weight, case):
    """a copy of `weight` with the non-causal taps zeroed by the oracle's MaskConstrainOp"""
    from oracle import pconv_cpu
    w = weight.detach().clone().contiguous()
    pconv_cpu.MaskConstrainOp(case.constrain, case.G, 0, False).forward(w)
    return w


_inputs = {}


def inputs(case):
    """(x, masked weight, bias, gout) float32 on the CPU, seeded by the case's name; built once, never modified"""
    if case.name not in _inputs:
        g = torch.Generator().manual_seed(5000 + ord(case.name))
        ho, wo = out_size(case)
        x = torch.randn(case.tn, case.cin, case.h, case.w, generator=g)
        weight = torch.randn(case.cout, case.cin, 5, 5, generator=g) / float(case.cin * 25) ** 0.5
        bias = torch.randn(case.cout, generator=g)
        gout = torch.randn(case.tn, case.cout, ho, wo, generator=g)
        if case.edges:
            x, gout, weight = B._edges(x, g, 1.0), B._edges(gout, g, -1.0), B._edges(weight, g, 1.0)
            bias = torch.where(torch.rand(case.cout, generator=g) < 0.5, bias * 2.0 ** -140, -torch.zeros_like(bias))
        _inputs[case.name] = (x, masked(weight, case), bias, gout)
    return _inputs[case.name]


def kept_fraction(case):
    w = inputs(case)[1]
    return float((masked(torch.ones_like(w), case) != 0).double().mean())


_twins = {}


def twin(case):
    """(y, gin or None, gw, gb) of the case, computed once per process and never modified"""
    if case.name not in _twins:
        from oracle import pconv_cpu
        x, weight, bias, gout = inputs(case)
        y = pconv_cpu.conv2d_chain(x, weight, bias, 1)
        gin = B.twin_dgrad(weight, gout, case.h, case.w, 1) if case.need_x else None
        _twins[case.name] = (y, gin, B.twin_wgrad(x, gout, 5, 1), B.twin_bgrad(gout))
    return _twins[case.name]


def forward_bound(case, x, weight, bias):
    """per-element bound of |chain - f64| for the forward: cin * 25 fmaf steps and the bias add, as
    conv_backward_cases.bounds states it for a chain"""
    absum = torch.nn.functional.conv2d(x.abs().double(), weight.abs().double(), bias.abs().double())
    return (case.cin * 25 + 1) * (B.U * absum + B.TINY)


def same_bits(got, ref, what):
    got, ref = bits(got), bits(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got != ref
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d entries differ, first at %s: got 0x%08x, expected 0x%08x"
                             % (what, int(bad.sum()), bad.numel(), first, got[first].item() & 0xffffffff,
                                ref[first].item() & 0xffffffff))
