"""Looking at a panorama: rectilinear viewports of ERP frames, of any size, field of view and orientation
(include/pconv_hip.h, pconv_viewport_map / pconv_viewport_render_f32).

float32 (n, C, h, w) -> (n, V, C, vh, vw): what a pinhole camera at the centre of the sphere sees in V orientations.  A
view is five int32 in units of 2^-16 degree (`view` makes it from degrees, rounding once): yaw, pitch, roll with the
meaning and ranges of erp_rotate.py, and the full horizontal and vertical field of view, each in [1, 170] degrees.

A view of vh x vw pixels with supersampling ss in 1 .. 4 has a grid of gh = vh * ss rows and gw = vw * ss columns of
samples.  Sample (r, q) looks along d = (1, a, b), a = (2 (q + 1/2) / gw - 1) tan(hfov / 2), b = (1 - 2 (r + 1/2) / gh)
tan(vfov / 2) (right is +y, up is +z, the centre of the picture is (1, 0, 0)) and reads the source at s = M d, M the
matrix of erp_rotate.py; `source_map_numpy` / the HIP map kernel turn s into erp_rotate's record, the source position
in 1/256 pixel (fp64).  `render_torch` / the HIP renderer read the source there with erp_rotate's 6 x 6 Lanczos-3 sampler
and average a pixel's ss x ss samples in a fixed order (p outer, t inner, fp32 additions, then one multiplication by
float32(1 / ss^2)), so the kernel of csrc/viewport.hip (PCONV.viewport_render_f32) and `render_torch` give the same bits
on the same map.

Anti-aliasing (`plan`).  The sampler interpolates; it does not average.  Where a view pixel covers more than one source
pixel the samples of the grid do: ss is the number of source pixels per view pixel at the centre of the view, where a
gnomonic view is coarsest, at most 4; beyond 4 the source is first reduced with erp_resample.resize until 4 samples
suffice.  The limits: the average is a box over the pixel, not a wider reconstruction filter; ss is chosen for the
centre of the view, so towards the edges of a wide view the samples are denser than they need to be; and a view here is
not, pixel for pixel, the view of the reference's ProjectsOp (MultiProject), whose grid, FoV convention and bilinear
sampler differ.

`Renderer` holds the maps of its views for one source size; `render` is the one-view convenience; `metrics` scores two
batches through a renderer (plain PSNR / SSIM of the rendered views, averaged over the views).  GPU tensors take the HIP
kernels, CPU tensors the twin (the oracle backend).

Training on the views.  `Renderer.render` (and erp_rotate.rotate) of a tensor that requires grad is attached to autograd
through one Function whose backward is the adjoint of "sampler over a map plus ss x ss average" in a defined order
(include/pconv_hip.h, pconv_remap_backward_f32): for every source pixel one fp32 accumulator starting at +0, to which the
terms ((g' wy[a]) wx[b]) -- g' = g[j][i] for ss = 1, else g[j][i] float32(1 / ss^2), one fp32 rounding per product and
per addition -- are added in the order a sequential walk of the forward reaches the pixel: grid sample s = r gw + q
ascending, then tap row a, then tap column b; the tap's pixel by the sampler's rule word for word; coinciding taps are
terms of their own; a pixel no term reaches gets +0.  `reverse_lists` builds that order once per map on the host (a CSR
list per source pixel from the very map the forward read), the kernel of csrc/remap_backward.hip
(PCONV.remap_backward_f32) gathers along it without atomics, and `render_backward_torch` is its twin: the same bits on the
same map and lists.  `loss_terms` is `metrics` as a loss (train.py --loss vp).  A view whose plan reads a reduced source
carries a gradient only through a Renderer made with prefilter_grad=True: the reduced source is then made by
erp_resample.resize under autograd, whose backward has a stated order as well (pconv_erp_resample_backward_f32), and
the gradient of x is the sum over the source sizes.  Limit: a list of at most 2^31 - 1 entries.
"""
import math

import numpy as np
import torch

from . import _native, erp_resample, erp_rotate, sphere_metrics
from ._native import PconvError
from .PCONV_operator import backend

PHASES, UNIT = erp_rotate.PHASES, erp_rotate.UNIT
MAX_SS = 4   # PCONV_VIEWPORT_MAX_SS
_NAMES = ("yaw", "pitch", "roll", "hfov", "vfov")
_RANGE = erp_rotate._RANGE + ((1 * UNIT, 170 * UNIT), (1 * UNIT, 170 * UNIT))


def check(view):
    """the integer quintuple (yaw, pitch, roll, hfov, vfov) of `view`; PconvError, naming the value, for anything that
    is not five integers in their ranges"""
    try:
        five = tuple(view)
        if len(five) != 5 or any(int(v) != v for v in five):
            raise TypeError
        five = tuple(int(v) for v in five)
    except (TypeError, ValueError):
        raise PconvError("viewport: a view is five integers in units of 2^-16 degree (viewport.view), got %r" % (view,))
    for name, v, (lo, hi) in zip(_NAMES, five, _RANGE):
        if not lo <= v <= hi:
            raise PconvError("viewport: %s %d is outside %d .. %d (units of 2^-16 degree)" % (name, v, lo, hi))
    return five


def _size(size, what="view"):
    try:
        vh, vw = (int(v) for v in size)
    except (TypeError, ValueError):
        raise PconvError("viewport: a %s size is (height, width), got %r" % (what, size))
    if not (2 <= vh <= 1 << 20 and 2 <= vw <= 1 << 20):
        raise PconvError("viewport: a %s side of %dx%d is outside 2 .. 2^20" % (what, vw, vh))
    return vh, vw


def view(yaw, pitch, roll, hfov, vfov=None, size=None):
    """degrees -> the integer quintuple in units of 2^-16 degree, each value rounded once.  vfov=None with size=(vh, vw):
    square pixels, vfov = 2 atan(tan(hfov / 2) vh / vw).  Values out of range are refused, not wrapped"""
    if vfov is None:
        if size is None:
            raise PconvError("viewport: a view needs vfov, or size=(vh, vw) for square pixels")
        vh, vw = _size(size)
        vfov = math.degrees(2.0 * math.atan(math.tan(math.radians(float(hfov)) / 2.0) * vh / vw))
    return check(tuple(int(round(float(v) * UNIT)) for v in (yaw, pitch, roll, hfov, vfov)))


def basis(view):
    """(M (3, 3), tan(hfov / 2), tan(vfov / 2)) in float64, from the host C function the map kernel takes them from"""
    out = np.empty(11, dtype=np.float64)
    _native.call("pconv_host_viewport_basis", *(check(view) + (out.ctypes.data,)))
    return out[:9].reshape(3, 3).copy(), float(out[9]), float(out[10])


def _check_source(h, w):
    try:
        return erp_rotate._check_size(h, w)
    except PconvError as exc:
        raise PconvError(str(exc).replace("erp rotate:", "viewport: the source:"))


def _check_grid(gh, gw):
    gh, gw = int(gh), int(gw)
    if not (2 <= gh <= MAX_SS << 20 and 2 <= gw <= MAX_SS << 20):
        raise PconvError("viewport: a grid side of %dx%d is outside 2 .. %d * 2^20" % (gw, gh, MAX_SS))
    if 8 * gh * gw >= 1 << 31:
        raise PconvError("viewport: a map of %dx%d records is 2^31 bytes or more" % (gw, gh))
    return gh, gw


def directions(gh, gw, view):
    """s = M d float64 (3, gh, gw): where each sample of the gh x gw grid of `view` looks, in the source's frame (not
    normalised)"""
    gh, gw = _check_grid(gh, gw)
    m, tx, ty = basis(view)
    a = ((2.0 * (np.arange(gw, dtype=np.float64) + 0.5) / gw - 1.0) * tx)[None, :]
    b = ((1.0 - 2.0 * (np.arange(gh, dtype=np.float64) + 0.5) / gh) * ty)[:, None]
    return np.stack([m[r, 0] + m[r, 1] * a + m[r, 2] * b for r in range(3)])


def source_coordinates(h, w, gh, gw, view):
    """(u, v) float64 (gh, gw): the column and row, in pixels of the h x w source, that grid sample (r, q) reads (the
    rule before its quantisation)"""
    h, w = _check_source(h, w)
    sx, sy, sz = directions(gh, gw, view)
    u = (np.arctan2(sy, sx) / (2.0 * np.pi) + 0.5) * w - 0.5
    v = (0.5 - np.arctan2(sz, np.hypot(sx, sy)) / np.pi) * h - 0.5
    return u, v


def source_map_numpy(h, w, gh, gw, view):
    """the map in float64 on the host: int32 (gh, gw, 2), [..., 0] = rint(u * PHASES) modulo w * PHASES, [..., 1] =
    rint(v * PHASES)"""
    u, v = source_coordinates(h, w, gh, gw, view)
    qu = np.mod(np.rint(u * PHASES).astype(np.int64), int(w) * PHASES)
    qv = np.rint(v * PHASES).astype(np.int64)
    return np.stack([qu, qv], axis=2).astype(np.int32)


def source_map(h, w, gh, gw, view, device=None):
    """int32 (gh, gw, 2) map on `device`: from the HIP kernel for a GPU device, from source_map_numpy on the CPU (the
    two agree except where a position lies within 1e-10 of a rounding boundary).  Nothing is cached: a map is 8 bytes
    per sample"""
    h, w = _check_source(h, w)
    gh, gw = _check_grid(gh, gw)
    view = check(view)
    device = torch.device("cpu" if device is None else device)
    if device.type == "cuda":
        ops = backend.ops()
        if not hasattr(ops, "viewport_map"):
            raise PconvError("viewport: the active backend has no viewport_map kernel for a GPU device")
        return ops.viewport_map(h, w, gh, gw, view, device)
    return torch.from_numpy(source_map_numpy(h, w, gh, gw, view))


def _check_ss(ss):
    if int(ss) != ss or not 1 <= int(ss) <= MAX_SS:
        raise PconvError("viewport: ss = %r supersampling is outside 1 .. %d" % (ss, MAX_SS))
    return int(ss)


def _check_frames(x, map, vh, vw, ss):
    if x.dim() != 4 or x.dtype != torch.float32:
        raise PconvError("viewport: float32 (n, C, h, w) expected, got %s %s" % (x.dtype, tuple(x.shape)))
    _check_source(*x.shape[2:])
    vh, vw = _size((vh, vw))
    ss = _check_ss(ss)
    if map.dtype != torch.int32 or tuple(map.shape) != (vh * ss, vw * ss, 2) or map.device != x.device:
        raise PconvError("viewport: the map must be int32 (%d, %d, 2) on the frames' device, got %s %s on %s"
                         % (vh * ss, vw * ss, map.dtype, tuple(map.shape), map.device))
    return vh, vw, ss


def render_torch(x, map, vh, vw, ss, clamp=False):
    """the renderer in torch, float32 operation by operation, on any device (the CPU path and the kernel's twin):
    float32 (n, C, h, w) and the int32 (vh * ss, vw * ss, 2) map of one view -> (n, C, vh, vw)"""
    vh, vw, ss = _check_frames(x, map, vh, vw, ss)
    out = None
    for p in range(ss):
        for t in range(ss):
            s = erp_rotate.sample_torch(x, map[p::ss, t::ss])
            out = s if out is None else out + s
    if ss > 1:
        out = out * torch.tensor(np.float32(1.0 / (ss * ss)), device=x.device)
    return out.clamp(0.0, 1.0) if clamp else out


def reverse_lists(map, h, w):
    """(start, entry): the transpose of the sampler over `map` (int32 (gh, gw, 2), the map the forward read) as one list
    per pixel of the h x w source, int32 tensors of h w + 1 and 36 gh gw elements on the map's device
    (pconv_host_remap_reverse: a stable counting sort of the forward walk; entry e = s 36 + a 6 + b).  A device map is
    copied to the host once, so that forward and backward agree on every record; 144 bytes per grid sample"""
    h, w = _check_source(h, w)
    if map.dtype != torch.int32 or map.dim() != 3 or map.shape[2] != 2:
        raise PconvError("viewport: a map is int32 (gh, gw, 2), got %s %s" % (map.dtype, tuple(map.shape)))
    gh, gw = _check_grid(*map.shape[:2])
    if 36 * gh * gw > np.iinfo(np.int32).max:
        raise PconvError("viewport: the %d list entries of a %dx%d grid are beyond int32: no gradient through this view"
                         % (36 * gh * gw, gw, gh))
    count = _native.call("pconv_host_remap_reverse_size", gh, gw)
    host = np.ascontiguousarray(map.detach().cpu().numpy())
    start, entry = np.empty(h * w + 1, dtype=np.int32), np.empty(count, dtype=np.int32)
    _native.call("pconv_host_remap_reverse", host.ctypes.data, gh, gw, h, w, start.ctypes.data, entry.ctypes.data)
    return torch.from_numpy(start).to(map.device), torch.from_numpy(entry).to(map.device)


def render_backward_torch(g, map, lists, h, w, vh, vw, ss, accumulate_into=None):
    """the gradient of render_torch (clamp=False) with respect to x, in the order of include/pconv_hip.h
    (pconv_remap_backward_f32), float32 operation by operation on any device (the CPU path and the kernel's twin):
    float32 (n, C, vh, vw), the map and its `reverse_lists` -> (n, C, h, w).  Every source pixel has one accumulator,
    starting at +0 (accumulate_into: at that tensor's values; a new tensor is returned either way), to which the terms
    ((g' wy[a]) wx[b]) of its list are added front to back, g' = g for ss = 1 and g float32(1 / ss^2) otherwise.
    Vectorised in rounds: round k adds the k-th entry of every list that has one"""
    h, w = _check_source(h, w)
    vh, vw = _size((vh, vw))
    ss = _check_ss(ss)
    gw = vw * ss
    if g.dim() != 4 or g.dtype != torch.float32 or tuple(g.shape[2:]) != (vh, vw):
        raise PconvError("viewport: a float32 (n, C, %d, %d) gradient expected, got %s %s" % (vh, vw, g.dtype, tuple(g.shape)))
    if map.dtype != torch.int32 or tuple(map.shape) != (vh * ss, gw, 2) or map.device != g.device:
        raise PconvError("viewport: the map must be int32 (%d, %d, 2) on the gradient's device, got %s %s on %s"
                         % (vh * ss, gw, map.dtype, tuple(map.shape), map.device))
    start, entry = (t.to(g.device).long() for t in lists)
    if start.numel() != h * w + 1 or entry.numel() != 36 * vh * ss * gw:
        raise PconvError("viewport: the lists are not those of this map and a %dx%d source" % (w, h))
    n, c = g.shape[:2]
    if accumulate_into is None:
        acc = torch.zeros((n, c, h * w), dtype=torch.float32, device=g.device)
    else:
        if tuple(accumulate_into.shape) != (n, c, h, w) or accumulate_into.dtype != torch.float32:
            raise PconvError("viewport: accumulate_into must be float32 (%d, %d, %d, %d)" % (n, c, h, w))
        acc = accumulate_into.to(g.device).reshape(n, c, h * w).clone()
    table = erp_rotate.phases().to(g.device)
    records = map.reshape(-1, 2).long()
    flat = g.reshape(n, c, vh * vw)
    if ss > 1:
        flat = flat * torch.tensor(np.float32(1.0 / (ss * ss)), device=g.device)
    length = start[1:] - start[:-1]
    alive = torch.nonzero(length > 0).flatten()      # the destinations that still have an entry in round k
    k = 0
    while alive.numel():
        e = entry[start[alive] + k]
        s, a, b = torch.div(e, 36, rounding_mode="floor"), torch.div(e, 6, rounding_mode="floor") % 6, e % 6
        rec = records[s]
        wy, wx = table[torch.remainder(rec[:, 1], PHASES), a], table[torch.remainder(rec[:, 0], PHASES), b]
        r, q = torch.div(s, gw, rounding_mode="floor"), s % gw
        pixel = torch.div(r, ss, rounding_mode="floor") * vw + torch.div(q, ss, rounding_mode="floor")
        acc[:, :, alive] = acc[:, :, alive] + (flat[:, :, pixel] * wy) * wx
        k += 1
        alive = alive[length[alive] > k]
    return acc.reshape(n, c, h, w)


class _Remap(torch.autograd.Function):
    """"sampler over maps plus ss x ss average" under autograd: (n, C, h, w) -> (n, V, C, vh, vw).  `forward` is the
    caller's unclamped forward; `views` holds per view (map, lists, ss), lists a callable that builds them at the first
    backward.  Backward: the views in ascending k into one gradient, accumulating from the second on -- the kernel for
    GPU tensors, render_backward_torch for CPU tensors: the same bits on the same maps.  clamp: torch.clamp's gradient,
    zero where the unclamped value lay outside [0, 1]"""

    @staticmethod
    def forward(ctx, x, forward, views, clamp):
        out = forward(x)
        ctx.views, ctx.source = views, tuple(x.shape[2:])
        if clamp:
            ctx.save_for_backward((out >= 0.0) & (out <= 1.0))
            out = out.clamp_(0.0, 1.0)
        ctx.clamp = clamp
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.clamp:
            g = torch.where(ctx.saved_tensors[0], g, torch.zeros((), dtype=g.dtype, device=g.device))
        g = g.contiguous()
        (h, w), (vh, vw) = ctx.source, g.shape[3:]
        ops = None
        if g.is_cuda:
            ops = backend.ops()
            if not hasattr(ops, "remap_backward_f32"):
                raise PconvError("viewport: the active backend has no remap_backward_f32 kernel for a GPU tensor")
        gin = None
        for k, (q, lists, ss) in enumerate(ctx.views):
            if ops is not None:
                gin = ops.remap_backward_f32(g, q, lists(), h, w, vh, vw, ss, gin, k, k > 0)
            else:
                gin = render_backward_torch(g[:, k], q, lists(), h, w, vh, vw, ss, gin)
        return gin, None, None, None


def ratio(h, w, view, vh, vw):
    """source pixels per view pixel at the centre of the view, the larger of the two axes (float64)"""
    h, w = _check_source(h, w)
    vh, vw = _size((vh, vw))
    _, tx, ty = basis(view)
    return max(w * tx / (math.pi * vw), 2.0 * h * ty / (math.pi * vh))


def plan(h, w, view, vh, vw):
    """(h2, w2, ss): the anti-aliasing rule.  With r = ratio(...): ss = min(4, max(1, ceil(r - 1e-9))); r <= 4 keeps the
    source, (h2, w2) = (h, w); r > 4 asks for the source reduced first (erp_resample.resize) to the smallest even w2 >=
    4 w / r (4 pi vw / tan(hfov / 2) where the horizontal axis is the coarser one) and h2 = round(h w2 / w), rendered with
    ss = 4.  A reduction beyond what resize takes (8 x per axis) is refused"""
    r = ratio(h, w, view, vh, vw)
    h, w, vh, vw = int(h), int(w), int(vh), int(vw)
    ss = min(MAX_SS, max(1, int(math.ceil(r - 1e-9))))
    if r <= MAX_SS:
        return h, w, ss
    _, tx, ty = basis(view)
    need = 4.0 * math.pi * vw / tx if w * tx / (math.pi * vw) >= 2.0 * h * ty / (math.pi * vh) else 4.0 * w / r
    w2 = int(math.ceil(need))
    w2 += w2 % 2
    h2 = max(2, int(round(h * w2 / float(w))))
    if w > erp_resample.MAX_SHRINK * w2 or h > erp_resample.MAX_SHRINK * h2:
        raise PconvError("viewport: a %dx%d view of a %dx%d source covers %.1f source pixels per pixel: more than %d x %d"
                         % (vw, vh, w, h, r, MAX_SS, erp_resample.MAX_SHRINK))
    return h2, w2, MAX_SS


def paper_views(size):
    """the 14 directions of the paper's evaluation (MultiProject.THETAS / PHIS) as views of `size` = (vh, vw): yaw =
    theta * 180 degrees (theta = 1 written -180), pitch = phi * 180 degrees, roll 0, hfov 90 degrees, square pixels.  Not,
    pixel for pixel, the views of ProjectsOp"""
    from .PCONV_operator.ops import MultiProject
    return [view(-180.0 if theta == 1 else theta * 180.0, phi * 180.0, 0.0, 90.0, size=size)
            for theta, phi in zip(MultiProject.THETAS, MultiProject.PHIS)]


class Renderer(object):
    """The views `views` (quintuples of `view`) of h x w sources at `size` = (vh, vw), their maps built once on `device`
    (the HIP map kernel on a GPU, numpy on the CPU; 8 ss^2 bytes per pixel and view, held by this object alone).
    ss=None: every view takes `plan`'s supersampling and, where plan asks for it, its reduced source (resized once per
    render call and size); ss=k: that supersampling on the source as it is.  prefilter_grad=True: under autograd a view
    on a reduced source carries its gradient through erp_resample.resize's ordered backward; by default such a view
    is refused then."""

    def __init__(self, h, w, views, size, ss=None, device=None, prefilter_grad=False):
        self.prefilter_grad = bool(prefilter_grad)
        self.h, self.w = _check_source(h, w)
        self.vh, self.vw = _size(size)
        self.views = [check(v) for v in views]
        if not self.views:
            raise PconvError("viewport: a renderer needs at least one view")
        self.device = torch.device("cpu" if device is None else device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if ss is None:
            self.plans = [plan(self.h, self.w, v, self.vh, self.vw) for v in self.views]
        else:
            self.plans = [(self.h, self.w, _check_ss(ss))] * len(self.views)
        self.maps = [source_map(h2, w2, self.vh * k, self.vw * k, v, self.device)
                     for v, (h2, w2, k) in zip(self.views, self.plans)]
        self._lists = [None] * len(self.views)   # the reverse lists of the backward, built when first asked for

    @property
    def ss(self):
        """the supersampling of the views: one integer when they agree, else the tuple"""
        ks = tuple(p[2] for p in self.plans)
        return ks[0] if len(set(ks)) == 1 else ks

    def render(self, x, clamp=False, out=None):
        """float32 (n, C, h, w) on the renderer's device -> (n, V, C, vh, vw): one render launch per view for GPU
        tensors, the twin for CPU tensors.  clamp=True bounds the result to [0, 1].  With grad mode on and x requiring a
        gradient the result is attached to autograd (one Function; `_Remap`): the values are the same, the backward is the
        ordered one of include/pconv_hip.h (pconv_remap_backward_f32), view after view in ascending k, its lists built at
        the first backward and held by the renderer (144 bytes per grid sample and view).  Refused then: out=, and,
        unless the renderer was made with prefilter_grad=True, a view whose plan reads a reduced source (the resize in
        front carries no gradient by default).  With prefilter_grad=True each reduced source is made once per size by
        erp_resample.resize under autograd (its ordered backward, pconv_erp_resample_backward_f32), the views of each
        source size go through one `_Remap`, the result holds the views in their order, and the gradient of x is the
        sum over the source sizes, made by autograd"""
        if torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad:
            if out is not None:
                raise PconvError("viewport: out= cannot be combined with a gradient: the result of an input that requires "
                                 "grad is a new tensor attached to autograd")
            sizes = []   # the source sizes of the plans, in the order the views first ask for them
            for k, (h2, w2, _) in enumerate(self.plans):
                if (h2, w2) != (self.h, self.w) and not self.prefilter_grad:
                    raise PconvError("viewport: view %d reads the source reduced to %dx%d (viewport.plan): the resize in "
                                     "front of the renderer carries no gradient" % (k, w2, h2))
                if (h2, w2) not in sizes:
                    sizes.append((h2, w2))
            self._check_frames(x)
            if sizes == [(self.h, self.w)]:
                views = [(q, (lambda k=k: self.lists(k)), p[2]) for k, (p, q) in enumerate(zip(self.plans, self.maps))]
                return _Remap.apply(x, self._render, views, bool(clamp))
            rendered = [None] * len(self.views)
            for h2, w2 in sizes:
                ks = [k for k, p in enumerate(self.plans) if p[:2] == (h2, w2)]
                src = x if (h2, w2) == (self.h, self.w) else erp_resample.resize(x, h2, w2)
                views = [(self.maps[k], (lambda k=k: self.lists(k)), self.plans[k][2]) for k in ks]
                group = _Remap.apply(src, (lambda s, ks=ks: self._render_views(s, ks)), views, bool(clamp))
                for slot, k in enumerate(ks):
                    rendered[k] = group[:, slot]
            return torch.stack(rendered, dim=1)
        return self._render(x, clamp, out)

    def _render_views(self, src, ks):
        """the views `ks`, unclamped, of `src`, a source of the size their plans name: (n, len(ks), C, vh, vw)"""
        n, c = src.shape[:2]
        out = torch.empty((n, len(ks), c, self.vh, self.vw), dtype=torch.float32, device=src.device)
        ops = backend.ops() if src.is_cuda else None
        if ops is not None and not hasattr(ops, "viewport_render_f32"):
            raise PconvError("viewport: the active backend has no viewport_render_f32 kernel for a GPU tensor")
        src = src.contiguous()
        for slot, k in enumerate(ks):
            self._render_slot(ops, src, k, out, slot)
        return out

    def _render_slot(self, ops, src, k, out, slot, clamp=False):
        """view k of `src` into out[:, slot]: one render launch (ops: the GPU backend) or the twin (ops=None)"""
        if ops is not None:
            ops.viewport_render_f32(src, self.maps[k], self.vh, self.vw, self.plans[k][2], clamp, out, slot)
        else:
            out[:, slot] = render_torch(src, self.maps[k], self.vh, self.vw, self.plans[k][2], clamp)

    def lists(self, k):
        """the reverse lists of view k (reverse_lists), built at the first call and kept"""
        if self._lists[k] is None:
            h2, w2, _ = self.plans[k]
            self._lists[k] = reverse_lists(self.maps[k], h2, w2)
        return self._lists[k]

    def _check_frames(self, x):
        if x.dim() != 4 or x.dtype != torch.float32 or tuple(x.shape[2:]) != (self.h, self.w) or x.device != self.device:
            raise PconvError("viewport: float32 (n, C, %d, %d) on %s expected, got %s %s on %s"
                             % (self.h, self.w, self.device, x.dtype, tuple(x.shape), x.device))

    def _render(self, x, clamp=False, out=None):
        if x.dim() != 4 or x.dtype != torch.float32 or tuple(x.shape[2:]) != (self.h, self.w) or x.device != self.device:
            raise PconvError("viewport: float32 (n, C, %d, %d) on %s expected, got %s %s on %s"
                             % (self.h, self.w, self.device, x.dtype, tuple(x.shape), x.device))
        n, c = x.shape[:2]
        shape = (n, len(self.views), c, self.vh, self.vw)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
            raise PconvError("viewport: out must be contiguous float32 %s on the frames' device" % (shape,))
        ops = None
        if x.is_cuda:
            ops = backend.ops()
            if not hasattr(ops, "viewport_render_f32"):
                raise PconvError("viewport: the active backend has no viewport_render_f32 kernel for a GPU tensor")
            x = x.contiguous()
        sources = {(self.h, self.w): x}
        for k, (h2, w2, _) in enumerate(self.plans):
            if (h2, w2) not in sources:
                sources[(h2, w2)] = erp_resample.resize(x, h2, w2)
            self._render_slot(ops, sources[(h2, w2)], k, out, k, clamp)
        return out


def render(x, view, size, ss=None, clamp=False):
    """one view of float32 (n, C, h, w): (n, C, vh, vw).  The maps are built for this call; hold a Renderer to reuse them"""
    if x.dim() != 4:
        raise PconvError("viewport: float32 (n, C, h, w) expected, got %s %s" % (x.dtype, tuple(x.shape)))
    return Renderer(x.shape[2], x.shape[3], [view], size, ss, x.device).render(x, clamp)[:, 0]


def metrics(renderer, x, y):
    """float64 CPU tensor (n, 2) of two batches seen through `renderer`: [:, 0] the MSE and [:, 1] the SSIM of the
    rendered views (sphere_metrics.metrics(., ., "uniform") per view), averaged over the views"""
    vx, vy = renderer.render(x), renderer.render(y)
    total = None
    for k in range(len(renderer.views)):
        m = sphere_metrics.metrics(vx[:, k].contiguous(), vy[:, k].contiguous(), "uniform")
        total = m if total is None else total + m
    return total / len(renderer.views)


def loss_terms(renderer, x, y):
    """float64 (n, 2) [MSE, SSIM] of two batches seen through `renderer`, on the inputs' device and attached to autograd:
    the values of `metrics`, as a loss.  Per view k, sphere_metrics.loss_terms(vx[:, k], vy[:, k], "uniform") of the
    rendered views; the views summed in ascending k in float64 and divided by V -- the sum `metrics` makes, so the two
    agree exactly.  The gradient reaches x and y through the renderer's ordered backward (Renderer.render)"""
    vx, vy = renderer.render(x), renderer.render(y)
    total = None
    for k in range(len(renderer.views)):
        m = sphere_metrics.loss_terms(vx[:, k].contiguous(), vy[:, k].contiguous(), "uniform")
        total = m if total is None else total + m
    return total / len(renderer.views)
