"""Squared error and SSIM weighted by a per-pixel weight plane (include/pconv_hip.h, pconv_weighted_mse_* and
pconv_weighted_ssim_f32; csrc/weighted_metrics.hip): WS-PSNR and WS-SSIM for any projection whose area weights are known,
and for masks.

WS-PSNR (Sun, Lu, Yu, IEEE SPL 2017) is defined for every projection by the area its pixels cover on the sphere.
sphere_metrics.py knows one such weight, the cosine of an ERP row; here the weights are data: a float64 (H, W) plane shared
by all frames and channels.  cube.area_weights (the solid angle of every pixel of a CMP / EAC picture) is the first user;
a mask of inactive regions, half-sphere content or a region of interest is the same call with another plane.

Definition, per plane (f, c) of two batches of one shape -- float32 (n, C, H, W), or uint8 (n, H, W, 3) read as
float(u8) / 255 -- with pixel p the row-major index in the plane and W the plane's total:
  d = x - y and e = d * d in fp32;  term_p = w_p * e, one fp64 product;  MSE[f][c] = (sum of the terms) / W
The sum runs in fp64 in the fixed order of the header (chunks of 1024 pixels, 256 lanes of four, a tree, a second stage
of the same shape: `ordered_sum`), which depends on H * W alone.  A figure is 10 log10(1 / mean over the channels).
Backward, of sum(gout * MSE) with respect to y:  k = ((2 gout[f][c]) w_p) / W in fp64, rounded once to fp32;
grad = k * (y - x) in fp32.  The gradient with respect to x is the same with x and y swapped.

SSIM, per plane (f, c) (`ssim`): map is sphere_metrics' SSIM map of the plane -- the 11-tap Gaussian of sigma 1.5 as g (x) g,
zero padding of 5 on the borders of the H x W plane, C1 = 0.01^2, C2 = 0.03^2 --
  SSIM[f][c] = (sum of w_p * map_p) / W
With erp_plane(h, w) the mean over the channels is sphere_metrics' WS-SSIM.  A window knows nothing of the projection: it
is the caller who lays the picture out so that a window's neighbourhood in the plane is its neighbourhood on the sphere
wherever the weight is not zero (cube.ws_ssim continues every face by the window's radius and weighs the ring zero).
The kernel computes the map in fp32 (the passes of pconv_ws_metrics_f32) and the sum in fp64 in the header's order; the
twin `ssim_torch` is the definition in float64: the two agree to about 1e-6, not to the bit.  `ssim` and its twins are forward
only (a tensor that requires grad is refused); the way in for training is `ssim_loss_terms`.
Backward, of sum(gout * SSIM) with respect to y (`ssim_backward`, pconv_weighted_ssim_backward_f32): sphere_metrics' gradient
with the per-row factor replaced by a per-pixel one, k_p = (gout[f][c] w_p) / W in fp64, rounded once to fp32 and zero
outside the plane;  grad = (blur(k a) + (2 y) blur(k b)) + x blur(k c), a, b, c those of sphere_metrics' head; no km term.
One kernel, the ERP backward's passes; `ssim_backward_torch` is the statement, and the kernel is held to it by a bound.

GPU tensors go to the HIP kernels (_metric_ops.weighted_mse_*, weighted_ssim_device); CPU tensors to the torch twins below;
for the squared error they follow the definition operation by operation: the bits are equal.  The twins are no fallback
for GPU tensors.

Limits.  W is supplied by the host (`WeightPlane.total`: math.fsum, the exactly rounded sum), never summed on the device.
A weight of zero is allowed (a mask); negative or non-finite weights and a plane that sums to zero are refused when the
plane is made.  The SSIM has no uint8 kernel (uint8 frames are converted first) and no multi-scale form; its gradient is
held to a bound, not to the bit.  No 4:2:0.
"""
import collections
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _metric_ops, sphere_metrics
from ._native import PconvError

CHUNK = 1024       # PCONV_SPHERE_POINTS_CHUNK
LANES = 256
KEPT_DEVICES = 4   # uploads a WeightPlane keeps


class WeightPlane(object):
    """a weight plane: `weights` (float64 (H, W) numpy, read-only), `total` = math.fsum of it, and the copies made of it on
    devices, the last KEPT_DEVICES.  Checked once, on the host: a negative or non-finite weight and a total of zero are
    refused"""

    def __init__(self, weights):
        if torch.is_tensor(weights):
            if weights.device.type != "cpu":
                raise PconvError("weight plane: a numpy array or a CPU tensor expected, got a tensor on %s" % weights.device)
            weights = weights.detach().numpy()
        w = np.asarray(weights)
        if w.dtype != np.float64 or w.ndim != 2 or w.size == 0:
            raise PconvError("weight plane: float64 (H, W) weights expected, got %s %s" % (w.dtype, w.shape))
        if not np.all(np.isfinite(w)):
            raise PconvError("weight plane: a weight is not finite (NaN or infinite)")
        if np.any(w < 0):
            raise PconvError("weight plane: a weight is negative")
        total = math.fsum(w.ravel().tolist())
        if not 0.0 < total < math.inf:
            raise PconvError("weight plane: the weights' total is %r: a plane that is all zero (or overflows) weighs nothing" % total)
        w = np.array(w, dtype=np.float64, order="C")
        w.setflags(write=False)
        self.weights, self.total = w, total
        self._on = collections.OrderedDict()

    @property
    def shape(self):
        return self.weights.shape

    def on(self, device=None):
        """the plane as a float64 (H, W) tensor on `device`, uploaded once; do not write to it"""
        device = torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = str(device)
        if key in self._on:
            self._on.move_to_end(key)
            return self._on[key]
        t = torch.from_numpy(np.array(self.weights)).to(device)
        self._on[key] = t
        while len(self._on) > KEPT_DEVICES:
            self._on.popitem(last=False)
        return t


def _plane(plane):
    return plane if isinstance(plane, WeightPlane) else WeightPlane(plane)


def _tree(v):
    """(.., 256) -> (..): lane l < s takes lane[l] + lane[l + s], s = 128 .. 1"""
    s = LANES // 2
    while s >= 1:
        v = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def ordered_sum(terms):
    """float64 (.., P) -> (..): the sum over the last axis in the header's order -- chunks of 1024, lane l of 256 adding the
    elements l, l + 256, l + 512, l + 768 of its chunk ascending, the tree, then the partials the same way.  A position that
    does not exist adds +0, which changes no sum that started at +0"""
    lead, count = terms.shape[:-1], terms.shape[-1]
    chunks = (count + CHUNK - 1) // CHUNK
    t = torch.zeros(lead + (chunks * CHUNK,), dtype=torch.float64, device=terms.device)
    t[..., :count] = terms
    t = t.reshape(lead + (chunks, CHUNK // LANES, LANES))
    lane = t[..., 0, :]
    for i in range(1, CHUNK // LANES):
        lane = lane + t[..., i, :]
    partials = _tree(lane)                                   # (.., chunks)
    rounds = (chunks + LANES - 1) // LANES
    p = torch.zeros(lead + (rounds * LANES,), dtype=torch.float64, device=terms.device)
    p[..., :chunks] = partials
    p = p.reshape(lead + (rounds, LANES))
    lane = p[..., 0, :]
    for i in range(1, rounds):
        lane = lane + p[..., i, :]
    return _tree(lane)


def _as_planes(t):
    """the batch as (n, C, H, W) of its float type: uint8 (n, H, W, 3) through float(u8) / 255 in float32"""
    if not torch.is_tensor(t) or t.dim() != 4:
        raise PconvError("weighted metrics: 4-D batches expected, got %s" % (tuple(t.shape) if torch.is_tensor(t) else type(t).__name__,))
    if t.dtype == torch.uint8 and t.shape[3] == 3:
        return (t.permute(0, 3, 1, 2).float() / 255.).contiguous()
    if t.dtype in (torch.float32, torch.float64):
        return t
    raise PconvError("weighted metrics: float32 (n, C, H, W) or uint8 (n, H, W, 3) expected, got %s %s" % (t.dtype, tuple(t.shape)))


def _check(x, y, plane, what="weighted metrics"):
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.dtype != y.dtype or x.shape != y.shape or x.device != y.device \
            or x.dim() != 4:
        raise PconvError("%s: two 4-D batches of one shape, type and device expected, got %s and %s"
                         % (what, *("%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__
                                    for t in (x, y))))
    hw = tuple(x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:])
    if hw != tuple(plane.shape):
        raise PconvError("%s: the weight plane is %dx%d, the pictures are %dx%d" % (what, plane.shape[1], plane.shape[0], hw[1], hw[0]))


def mse_torch(x, y, plane):
    """float64 (n, C) on the batches' device: the definition in torch, operation by operation (the CPU path of `mse` and
    the kernel's twin, bit for bit).  float64 batches are taken too: every fp32 step then runs in float64"""
    plane = _plane(plane)
    _check(x, y, plane)
    a, b = _as_planes(x), _as_planes(y)
    d = a - b
    e = (d * d).double()
    terms = plane.on(a.device).reshape(1, 1, -1) * e.reshape(e.shape[0], e.shape[1], -1)
    return ordered_sum(terms) / plane.total


def backward_torch(x, y, plane, gout):
    """the gradient of sum(gout * mse(x, y, plane)) with respect to y in torch, operation by operation: k = ((2 gout) w) / W
    in float64, rounded once to the batches' type; k * (y - x) in that type.  gout: float64 (n, C)"""
    plane = _plane(plane)
    _check(x, y, plane, "weighted loss")
    k = ((2.0 * gout.double())[:, :, None, None] * plane.on(x.device)[None, None]) / plane.total
    return k.to(x.dtype) * (y - x)


def mse_device(x, y, plane):
    """`mse` with the result left on the batches' device: nothing waits"""
    plane = _plane(plane)
    _check(x, y, plane)
    if x.is_cuda:
        return _metric_ops.weighted_mse_device(x.contiguous(), y.contiguous(), plane.on(x.device), plane.total)
    return mse_torch(x, y, plane)


def backward(x, y, plane, gout):
    """float32 (n, C, H, W): the gradient of sum(gout * mse_device(x, y, plane)) with respect to y; gout float64 (n, C) on
    the batches' device.  GPU tensors: the HIP kernel, one launch; CPU tensors: backward_torch; the same bits.  For the
    gradient with respect to x swap x and y"""
    plane = _plane(plane)
    _check(x, y, plane, "weighted loss")
    if x.is_cuda:
        return _metric_ops.weighted_mse_backward(x.contiguous(), y.contiguous(), plane.on(x.device), plane.total, gout.contiguous())
    return backward_torch(x, y, plane, gout)


def mse(x, y, plane):
    """float64 CPU tensor (n, C): per frame and channel (sum of w_p (x - y)^2) / W.  x, y: one shape, float32 (n, C, H, W)
    or uint8 (n, H, W, 3); plane: a WeightPlane (or float64 (H, W) weights) of the pictures' size.  GPU tensors: the HIP
    kernel; CPU tensors: mse_torch; the same bits"""
    return mse_device(x, y, plane).cpu()


def psnr(x, y, plane):
    """float64 (n,) dB of each frame: 10 log10(1 / mean over the channels of `mse`), +inf for identical frames"""
    return sphere_metrics.psnr(mse(x, y, plane).mean(dim=1))


class _Mse(torch.autograd.Function):
    """`mse_device` of float batches: the kernel (GPU) or the twin (CPU) forward, and the backward kernel / twin once per
    input that needs a gradient"""

    @staticmethod
    def forward(ctx, x, y, plane):
        ctx.save_for_backward(x, y)
        ctx.plane = plane
        return mse_device(x, y, plane)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        return (backward(y, x, ctx.plane, gout) if ctx.needs_input_grad[0] else None), \
            (backward(x, y, ctx.plane, gout) if ctx.needs_input_grad[1] else None), None


def channel_mean(values):
    """float64 (n, C) -> (n,): the channels added in ascending order, then one division by C as a tensor -- the same
    operations on every device (a division by a python number may become a multiplication by its inverse on a GPU)"""
    total = values[:, 0]
    for c in range(1, values.shape[1]):
        total = total + values[:, c]
    return total / torch.full((), float(values.shape[1]), dtype=values.dtype, device=values.device)


def loss_terms(x, y, plane):
    """float64 (n,) on the inputs' device, attached to autograd: per frame the mean over the channels of `mse`, as a loss.
    x, y: float32 (n, C, H, W) of one shape (CPU tensors may be float64; uint8 carries no gradient and is refused).  GPU
    tensors: the HIP kernels forward and backward, no host synchronisation; CPU tensors: the twins"""
    plane = _plane(plane)
    _check(x, y, plane, "weighted loss")
    if not x.is_floating_point() or (x.is_cuda and x.dtype != torch.float32):
        raise PconvError("weighted loss: float32 (n, C, H, W) batches expected (uint8 frames carry no gradient), got %s %s"
                         % (x.dtype, tuple(x.shape)))
    return channel_mean(_Mse.apply(x.contiguous(), y.contiguous(), plane))


def _ssim_operands(x, y, plane):
    plane = _plane(plane)
    _check(x, y, plane, "weighted ssim")
    if x.requires_grad or y.requires_grad:
        raise PconvError("weighted ssim: a tensor that requires grad: the weighted SSIM is forward only; detach the pictures")
    return _as_planes(x), _as_planes(y), plane


def ssim_torch(x, y, plane):
    """float64 (n, C) on the batches' device: the definition in float64 torch (the CPU path of `ssim` and the reference
    the GPU tests compare the kernel with): sphere_metrics' full SSIM map, weighed by the plane, over plane.total"""
    a, b, plane = _ssim_operands(x, y, plane)
    ssim_map = sphere_metrics._ssim_map(sphere_metrics._moments(a.double(), b.double(), sphere_metrics.gaussian()), True)
    return (ssim_map * plane.on(a.device)).sum(dim=(2, 3)) / plane.total


def ssim_device(x, y, plane):
    """`ssim` with the result left on the batches' device: nothing waits"""
    a, b, plane = _ssim_operands(x, y, plane)
    if a.is_cuda:
        if a.dtype != torch.float32:
            raise PconvError("weighted ssim: float32 (n, C, H, W) or uint8 (n, H, W, 3) expected on a GPU, got %s" % a.dtype)
        return _metric_ops.weighted_ssim_device(a.contiguous(), b.contiguous(), plane.on(a.device), plane.total)
    return ssim_torch(a, b, plane)


def ssim(x, y, plane):
    """float64 CPU tensor (n, C): per frame and channel (sum of w_p map_p) / W, map the SSIM map of the plane.  x, y: one
    shape, float32 (n, C, H, W) or uint8 (n, H, W, 3); plane: a WeightPlane (or float64 (H, W) weights) of the pictures'
    size.  GPU tensors: the HIP kernel (fp32 map); CPU tensors: ssim_torch (float64).  A tensor that requires grad is
    refused"""
    return ssim_device(x, y, plane).cpu()


def _check_gout(x, gout, what):
    if not torch.is_tensor(gout) or tuple(gout.shape) != tuple(x.shape[:2]):
        raise PconvError("%s: gout (n, C) = %s expected, got %s" % (what, tuple(x.shape[:2]), tuple(gout.shape)
                                                                    if torch.is_tensor(gout) else type(gout).__name__))


def ssim_backward_torch(x, y, plane, gout, dt=torch.float64):
    """the gradient of sum(gout * ssim(x, y, plane)) with respect to y by the explicit formula of include/pconv_hip.h
    (pconv_weighted_ssim_backward_f32), in torch: the statement the HIP kernel is held to.  x, y (n, C, H, W); gout (n, C).
    k = (gout w) / W is formed in float64 and rounded once to dt; everything else runs in dt, operation by operation in the
    kernel's order: sphere_metrics' moments, coefficients and (blur(k a) + (2 y) blur(k b)) + x blur(k c).  Returns dt
    (n, C, H, W)"""
    plane = _plane(plane)
    _check(x, y, plane, "weighted ssim loss")
    _check_gout(x, gout, "weighted ssim loss")
    k = ((gout.detach().double().to(x.device)[:, :, None, None] * plane.on(x.device)[None, None]) / plane.total).to(dt)
    x, y = x.detach().to(dt), y.detach().to(dt)
    g = sphere_metrics.gaussian()
    return sphere_metrics._own(x, y, k, sphere_metrics._coefficients(sphere_metrics._moments(x, y, g), True), g)


def ssim_backward(x, y, plane, gout):
    """float32 (n, C, H, W): the gradient of sum(gout * ssim_device(x, y, plane)) with respect to y; x, y float32 GPU
    tensors, gout float64 (n, C) on their device.  The HIP kernel, one launch (the passes of sphere_metrics' backward with a
    per-pixel factor); it agrees with ssim_backward_torch to a bound, not to the bit.  For the gradient with respect to x
    swap x and y.  CPU tensors are refused: ssim_backward_torch is the statement there"""
    plane = _plane(plane)
    _check(x, y, plane, "weighted ssim loss")
    _check_gout(x, gout, "weighted ssim loss")
    if not x.is_cuda or x.dtype != torch.float32:
        raise PconvError("weighted ssim loss: ssim_backward is the HIP kernel: float32 GPU tensors expected, got %s on %s "
                         "(ssim_backward_torch states the gradient on any device)" % (x.dtype, x.device))
    return _metric_ops.weighted_ssim_backward(x.contiguous(), y.contiguous(), plane.on(x.device), plane.total, gout.contiguous())


class _Ssim(torch.autograd.Function):
    """the weighted SSIM per plane of float32 GPU batches: the forward kernel, and the backward kernel once per input that
    needs a gradient"""

    @staticmethod
    def forward(ctx, x, y, plane):
        ctx.save_for_backward(x, y)
        ctx.plane = plane
        return _metric_ops.weighted_ssim_device(x, y, plane.on(x.device), plane.total)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        return (ssim_backward(y, x, ctx.plane, gout) if ctx.needs_input_grad[0] else None), \
            (ssim_backward(x, y, ctx.plane, gout) if ctx.needs_input_grad[1] else None), None


def ssim_loss_terms(x, y, plane):
    """float64 (n,) on the inputs' device, attached to autograd: per frame the mean over the channels of the weighted SSIM
    (`ssim`'s values), as a loss term.  x, y: float (n, C, H, W) of one shape; uint8 carries no gradient and is refused.
    GPU tensors (float32): the HIP kernels forward and backward, no host synchronisation.  CPU tensors: the float64 torch
    statement (ssim_torch's), differentiated by torch"""
    plane = _plane(plane)
    _check(x, y, plane, "weighted ssim loss")
    if not x.is_floating_point() or (x.is_cuda and x.dtype != torch.float32):
        raise PconvError("weighted ssim loss: float32 (n, C, H, W) batches expected (uint8 frames carry no gradient), got %s %s"
                         % (x.dtype, tuple(x.shape)))
    if x.is_cuda:
        return channel_mean(_Ssim.apply(x.contiguous(), y.contiguous(), plane))
    ssim_map = sphere_metrics._ssim_map(sphere_metrics._moments(x.double(), y.double(), sphere_metrics.gaussian()), True)
    return channel_mean((ssim_map * plane.on(x.device)).sum(dim=(2, 3)) / plane.total)


def ssim_figure(x, y, plane):
    """float64 (n,): the mean over the channels of `ssim`, one number per frame"""
    return channel_mean(ssim(x, y, plane))


def erp_plane(h, w):
    """the WeightPlane of an h x w ERP frame: sphere_metrics.weights(h), the cosine of each row, broadcast over the columns"""
    rows = sphere_metrics.weights(int(h)).numpy()
    return WeightPlane(np.repeat(rows[:, None], int(w), axis=1))
