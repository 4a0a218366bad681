"""Shared by tests/test_conv_backward_cpu.py and tests/test_gpu_conv_backward.py: the shapes the native convolution
backward (csrc/conv_backward.hip) is held at, their inputs, the CPU twin that restates its three orders, and the
float64 reference with the chain's own error bound.

The twin is built from the unmodified oracle.pconv_cpu.conv2d_chain (C fmaf, one k-ascending chain per output):

  data gradient    conv2d_chain, stride 1, of the numpy-prepared gradient (zero-stuffed to the stride, padded by k - 1,
                   (h-k) % s / (w-k) % s further zero rows / columns) with wT[ci][co][a][b] = w[co][ci][k-1-a][k-1-b]
  weight partial   P_t[co][n] = the chain over the tile's pixels p = (y, x) ascending of gout[t,co,p] * patch[p][n],
                   patch[p][(ci*k + kh)*k + kw] = in[t, ci, s y + kh, s x + kw].  conv2d_chain takes square kernels only,
                   so the pixels are handed to it as the CHANNELS of a 1x1 convolution (its chain runs over the
                   channels ascending): x = patch as (1, P, 1, N), weight = gout[t] as (cout, P, 1, 1).  This is the
                   chain `conv2d_chain(in[t].reshape(cin,1,h,w), gout[t].reshape(cout,1,ho,wo))` would run if it took
                   an ho x wo kernel, for either stride.
  weight gradient  (((P_0 + P_1) + P_2) + ...) in float32
  bias gradient    the fp64 walk of the two-stage reduction (256 lanes per plane, the tree 128 .. 1, planes ascending)
"""
import collections

import numpy as np
import torch

Case = collections.namedtuple("Case", "name k s cin cout h w tn need_x edges")

# each the smallest shape at which something can break
CASES = [
    Case("a", 3, 1, 24, 40, 7, 70, 3, True, False),     # wo 68 crosses a 64-column run; ragged cout
    Case("b", 3, 2, 16, 32, 10, 21, 3, True, False),    # one untouched bottom row: gin row 9 must be +0
    Case("c", 1, 1, 5, 3, 4, 33, 2, True, False),       # ragged cin; odd wo (a pad step per run)
    Case("d", 1, 2, 48, 192, 5, 130, 3, True, False),
    Case("e", 3, 1, 3, 192, 6, 20, 2, False, False),    # the first layer: no data gradient requested
    Case("f", 3, 1, 192, 192, 6, 66, 2, True, False),   # several column blocks and cout blocks
    Case("g", 3, 1, 192, 768, 4, 18, 1, True, False),
    Case("h", 3, 1, 16, 16, 66, 130, 1, True, False),   # an 8192-step chain per partial
    Case("i", 3, 2, 16, 32, 10, 21, 3, True, True),     # as b at fp32's edges: subnormals, +-0, products that underflow
    # as c at fp32's edges: the pad step of an odd run meets accumulators that are -0.  Weight and bias gradient only
    # (the data gradient's arithmetic is pconv_conv2d's, pinned at these edges by tests/test_gpu_fp32_edges.py)
    Case("j", 1, 1, 5, 3, 4, 33, 2, False, True),
]
BY_NAME = {c.name: c for c in CASES}


def out_size(case):
    return (case.h - case.k) // case.s + 1, (case.w - case.k) // case.s + 1


def _edges(t, g, sign):
    """some entries subnormal, +0, -0 and small enough for products of two of them to underflow; channel 0 is small
    throughout (products of two such channels are subnormal) and channel 1 smaller still and of one sign, so that
    whole chains run on products below 2^-149 that round to the same signed zero"""
    r = torch.rand(t.shape, generator=g)
    t = torch.where(r < 0.10, t * 2.0 ** -130, t)
    t = torch.where((r >= 0.10) & (r < 0.15), torch.zeros_like(t), t)
    t = torch.where((r >= 0.15) & (r < 0.20), -torch.zeros_like(t), t)
    t = torch.where((r >= 0.20) & (r < 0.35), t * 2.0 ** -78, t)
    t[:, 0] = t[:, 0] * 2.0 ** -70
    t[:, 1] = t[:, 1].abs() * (sign * 2.0 ** -80)
    return t.contiguous()


def inputs(case):
    """(x, weight, gout) float32 on the CPU, seeded by the case's name"""
    g = torch.Generator().manual_seed(1000 + ord(case.name))
    ho, wo = out_size(case)
    x = torch.randn(case.tn, case.cin, case.h, case.w, generator=g)
    weight = torch.randn(case.cout, case.cin, case.k, case.k, generator=g) / float(case.cin * case.k * case.k) ** 0.5
    gout = torch.randn(case.tn, case.cout, ho, wo, generator=g)
    if case.edges:
        x, gout, weight = _edges(x, g, 1.0), _edges(gout, g, -1.0), _edges(weight, g, 1.0)
    return x, weight, gout


# ---- the twin -------------------------------------------------------------------------------------------------------

def prepared_gradient(gout, h, w, k, s):
    tn, cout, ho, wo = gout.shape
    p = np.zeros((tn, cout, h + k - 1, w + k - 1), dtype=np.float32)
    p[:, :, k - 1:k - 1 + s * ho:s, k - 1:k - 1 + s * wo:s] = gout.numpy()
    return torch.from_numpy(p)


def transposed_weight(weight):
    return weight.flip(2, 3).transpose(0, 1).contiguous()


def twin_dgrad(weight, gout, h, w, s):
    from oracle import pconv_cpu
    k = weight.shape[2]
    return pconv_cpu.conv2d_chain(prepared_gradient(gout, h, w, k, s), transposed_weight(weight), None, 1)


def patches(xt, k, s, ho, wo):
    """(P, N): patch[p = y*wo + x][(ci*k + kh)*k + kw] = xt[ci, s y + kh, s x + kw]"""
    cin = xt.shape[0]
    a = xt.numpy()
    out = np.empty((ho * wo, cin * k * k), dtype=np.float32)
    for ci in range(cin):
        for kh in range(k):
            for kw in range(k):
                out[:, (ci * k + kh) * k + kw] = a[ci, kh::s, kw::s][:ho, :wo].reshape(-1)
    return out


def twin_wgrad_partial(xt, gt, k, s):
    """P_t (cout, cin, k, k) of one tile"""
    from oracle import pconv_cpu
    cin, cout, (ho, wo) = xt.shape[0], gt.shape[0], gt.shape[1:]
    pt = patches(xt, k, s, ho, wo)
    xs = torch.from_numpy(pt).reshape(1, ho * wo, 1, cin * k * k)
    ws = gt.reshape(cout, ho * wo, 1, 1).contiguous()
    return pconv_cpu.conv2d_chain(xs, ws, None, 1).reshape(cout, cin, k, k)


def twin_wgrad(x, gout, k, s):
    acc = None
    for t in range(x.shape[0]):
        p = twin_wgrad_partial(x[t], gout[t], k, s).numpy()
        acc = p if acc is None else (acc + p).astype(np.float32)   # one float32 add per element
    return torch.from_numpy(acc)


def twin_bgrad(gout):
    tn, cout, ho, wo = gout.shape
    g = gout.numpy().astype(np.float64).reshape(tn, cout, ho * wo)
    rows = (ho * wo + 255) // 256
    padded = np.zeros((tn, cout, rows * 256), dtype=np.float64)   # (+0 terms: no-ops on sums that start at +0)
    padded[:, :, :ho * wo] = g
    lanes = np.zeros((tn, cout, 256), dtype=np.float64)
    for r in range(rows):
        lanes = lanes + padded[:, :, r * 256:(r + 1) * 256]
    s = 128
    while s > 0:
        lanes[:, :, :s] = lanes[:, :, :s] + lanes[:, :, s:2 * s]
        s //= 2
    acc = np.zeros(cout, dtype=np.float64)
    for t in range(tn):
        acc = acc + lanes[t, :, 0]
    return torch.from_numpy(acc.astype(np.float32))


_twins = {}


def twin(case):
    """(gin or None, gw, gb) of the case, computed once per process and never modified"""
    if case.name not in _twins:
        x, weight, gout = inputs(case)
        gin = twin_dgrad(weight, gout, case.h, case.w, case.s) if case.need_x else None
        _twins[case.name] = (gin, twin_wgrad(x, gout, case.k, case.s), twin_bgrad(gout))
    return _twins[case.name]


# ---- float64 reference and the chain's bound ------------------------------------------------------------------------

U = 2.0 ** -24       # unit roundoff of float32
TINY = 2.0 ** -150   # half an ulp in the subnormal range: the absolute error of a rounding that underflows


def f64_grads(x, weight, gout, s):
    """(gin, gw, gb) of conv2d in float64 by torch autograd"""
    xd = x.double().requires_grad_(True)
    wd = weight.double().requires_grad_(True)
    bd = torch.zeros(weight.shape[0], dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(xd, wd, bd, s)
    return torch.autograd.grad(y, (xd, wd, bd), gout.double())


def bounds(case, x, weight, gout):
    """per-element bound of |twin - f64| for (gin, gw, gb): a chain of n fmaf steps (and float32 adds) errs by at
    most n * 2^-24 * sum|a_i b_i| to first order, plus 2^-150 for every rounding that lands in the subnormal range;
    the sum of the absolute products is the same gradient of the absolute tensors, taken in float64.  The bias
    gradient is a float64 sum rounded once: 2^-24 * sum|g|, plus the float64 sums' own N * 2^-53 * sum|g| on either
    side."""
    ho, wo = out_size(case)
    ain, aw, ab = f64_grads(x.abs(), weight.abs(), gout.abs(), case.s)
    n_x = case.cout * case.k * case.k
    n_w = ho * wo + (case.tn - 1)
    n_b = case.tn * ho * wo
    return (n_x * (U * ain + TINY), n_w * (U * aw + TINY), (U + 2 * n_b * 2.0 ** -53) * ab + TINY)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)
