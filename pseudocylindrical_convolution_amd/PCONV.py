"""`PCONV` -- the native-module surface of the reference, on MI355X.

The reference binds 21 stateful C++ op classes with pybind11
(extension/main.cpp:4-137).  This module offers the same classes, constructor
signatures and methods; each one owns its output buffers, step counters and
table caches exactly like the reference's `base_opt` objects
(extension/base_opt.hpp:4-81) and launches the hand-written HIP kernels of
libpconv_hip.so through the C ABI in include/pconv_hip.h.

There is no CPU path here: every forward needs the HIP library and a GPU tensor.
"""
import collections
import ctypes
import functools
import os
import weakref

import numpy as np
import torch

from . import _native
from ._native import PconvError, call

__all__ = [
    "ProjectsOp", "DtowOp", "ContextReshapeOp", "EntropyGmmOp", "MaskConstrainOp",
    "SphereSliceOp", "SphereUsliceOp", "EntropyGmmTableOp", "EntropyContextOp",
    "EntropyCtxPadRun2Op", "DExtract2Op", "DInput2Op", "EntropyConv2Op", "PseudoContextOp",
    "PseudoPadOp", "PseudoFillOp", "PseudoEntropyContextOp", "PseudoEntropyPadOp",
    "PseudoQuantOp", "PseudoDQuantOp", "EntropyAddOp",
]

# addr() string -> context object (string2class.cc:2-22 parses a raw pointer;
# here the string is an opaque key and borrowers keep a strong reference)
_contexts = weakref.WeakValueDictionary()


def _lookup(addr):
    try:
        return _contexts[addr]
    except KeyError:
        raise PconvError("no live context object for address %r" % (addr,))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _np_ptr(a):
    return a.ctypes.data


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _require_gpu(x, what):
    if not x.is_cuda:
        raise PconvError("%s: expected a GPU tensor (this build has no CPU path), got %s" % (what, x.device))
    if x.dtype != torch.float32:
        raise PconvError("%s: only float32 is supported, got %s" % (what, x.dtype))
    if not x.is_contiguous():
        raise PconvError("%s: input must be contiguous" % what)


def _require_operand(t, what, name, shape, dtype, like, dense=True):
    """operand `name` of `what`, checked before its address goes to the library: a tensor of element type `dtype` on the
    device of `like` (the call's first operand).  shape: a tuple, the exact shape (None: any extent); an int, a length the
    tensor must at least have.  dense: contiguous (False: the wrapper makes its own dense copy).  Attribute comparisons
    only: nothing is copied and nothing waits"""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == like.device and (t.is_contiguous() or not dense)
    if ok and isinstance(shape, int):
        ok = t.numel() >= shape
    elif ok:
        ok = t.dim() == len(shape) and all(e is None or e == s for e, s in zip(shape, t.shape))
    if not ok:
        want = "at least %d elements" % shape if isinstance(shape, int) else \
            "(%s)" % ", ".join("*" if e is None else str(int(e)) for e in shape)
        got = "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__
        raise PconvError("%s: %s must be a %s%s tensor of %s on %s, got %s"
                         % (what, name, "contiguous " if dense else "", str(dtype).split(".")[1], want, like.device, got))
    return t


def tile_widths(weight, npart, height, width, rule="pconv_host_tile_widths"):
    """Valid width of each latitude tile (math_cuda.cu:223-253; `rule`: the slice's variant, :177-221)."""
    w = np.ascontiguousarray(weight, dtype=np.float32)
    out = np.zeros(npart, dtype=np.int32)
    call(rule, _np_ptr(w), npart, height, width, _np_ptr(out))
    return out


def _timed(method, label):
    """`timeit=True` of the reference's constructors (timer.h:5-47: events around the kernels of a
    call, then `<head> Elapsed time : <ms> ms` on stdout): here around the whole forward / backward
    call of the op, on the stream the op launches on"""

    @functools.wraps(method)
    def run(self, *args, **kwargs):
        if not self.timeit_:
            return method(self, *args, **kwargs)
        stream = torch.cuda.current_stream(self._dev())
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        try:
            return method(self, *args, **kwargs)
        finally:
            stop.record(stream)
            stop.synchronize()
            print("%s.%s Elapsed time : %f ms" % (type(self).__name__, label, start.elapsed_time(stop)))

    return run


# When set to an object with a `records` list (bench.py), every launch of the HBM-bound gather /
# permute kernels is bracketed by events on its stream: (kernel, class label, algorithmic bytes of
# SURVEY 8d for this call, start, end).  None in normal operation.
hbm_probe = None
_VALID_FRACTION = 836.0 / 1024.0  # valid columns / all columns of the tile stack


class _HbmTimed(object):
    __slots__ = ("probe", "kernel", "label", "nbytes", "stream", "e0")

    def __init__(self, kernel, label, nbytes, device):
        self.probe = hbm_probe
        if self.probe is not None:
            self.kernel, self.label, self.nbytes = kernel, label, float(nbytes)
            self.stream = torch.cuda.current_stream(device)

    def __enter__(self):
        if self.probe is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(self.stream)
        return self

    def __exit__(self, *exc):
        if self.probe is not None and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(self.stream)
            self.probe.records.append((self.kernel, self.label, self.nbytes, self.e0, e1))
        return False


class _PreviousSwitch(int):
    """what a call of a _Switch returns: the switch's previous value (an int that compares like the bool), and a
    context manager that puts that value back on leaving the block"""

    def __new__(cls, switch):
        self = int.__new__(cls, switch.on)
        self.switch = switch
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.switch.on = bool(self)
        return False


class _Switch(object):
    """A process-wide boolean, off by default, read where it matters at every call.  switch(on) sets it (None leaves
    it) and returns its previous value; `with switch(True): ...` restores the previous value at the end of the block,
    also after an exception.  switch.is_on() reads it."""

    def __init__(self):
        self.on = False

    def __call__(self, on=None):
        previous = _PreviousSwitch(self)
        if on is not None:
            self.on = bool(on)
        return previous

    def is_on(self):
        return self.on


# The backward calls of SphereSliceOp, SphereUsliceOp, ProjectsOp and PseudoQuantOp sum with float atomics by
# default; with this switch on they take the ordered (atomic-free) kernels of csrc/backward_ordered.hip, whose
# sums run in the order include/pconv_hip.h defines.  Read at every backward call.
ordered_backward = _Switch()
backward_is_ordered = ordered_backward.is_on
backward_launches = collections.Counter()   # entry point -> backward calls of those four ops that launched it


def _backward_call(fn, *args):
    backward_launches[fn] += 1
    call(fn, *args)


# The convolutions of a training step go to the vendor library's forward and backward by default (TileConv2d under
# autograd); with this switch on they stay on this project's kernels: tile_conv2d forward, tile_conv2d_backward
# (csrc/conv_backward.hip) for the three gradients.  Read at every TileConv2d call under autograd.
native_conv_grad = _Switch()
conv_grad_is_native = native_conv_grad.is_on

# The masked 5x5 convolutions of the entropy model (MaskConv2 / MaskConv3 with kernel size 5) call the vendor
# library's conv2d by default, also under native_conv_grad; with this switch on they go to conv5x5 /
# conv5x5_backward (csrc/conv.hip, csrc/conv_backward.hip).  A switch of its own: neither native_conv_grad nor
# ordered_backward changes it or is changed by it.  Read at every _MaskConv.forward.
native_masked_conv = _Switch()
masked_conv_is_native = native_masked_conv.is_on


class _Op(object):
    """State shared by all ops: target device and re-used output buffers
    (base_opt.hpp:12-72)."""

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        for name, attr in list(vars(cls).items()):
            if callable(attr) and (name.startswith("forward") or name.startswith("backward")):
                setattr(cls, name, _timed(attr, name))

    def __init__(self, device, timeit=False):
        self.device_ = int(device)
        self.timeit_ = bool(timeit)
        self._top = {}
        self._shape = None

    def to(self, device):
        device = int(device)
        if device != self.device_:
            self.device_ = device
            self._top = {}
            self._shape = None
            self._moved()

    def _moved(self):
        pass

    def _dev(self):
        return torch.device("cuda", self.device_)

    def _reshaped(self, shape):
        shape = tuple(int(s) for s in shape)
        if shape == self._shape:
            return False
        self._shape = shape
        return True

    def _out(self, slot, shape, like, zero=False):
        """Op-owned output buffer, reallocated only when its shape changes."""
        shape = tuple(int(s) for s in shape)
        t = self._top.get(slot)
        if t is None or tuple(t.shape) != shape or t.device != like.device:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=like.device)
            self._top[slot] = t
        return t

    def _upload(self, array, like):
        return torch.from_numpy(np.ascontiguousarray(array)).to(like.device)


# ---------------------------------------------------------------------------
# context objects
# ---------------------------------------------------------------------------
class _TileContext(_Op):
    """Shared geometry cache: tile widths per tensor width and gather tables per
    (height, width, pad).  Mirrors pseudo_context_opt / entropy_context
    (pseudo_context.hpp:8-45, entropy_context.hpp:10-53)."""

    def __init__(self, npart, rt, weight, device=0, timeit=False):
        super().__init__(device, timeit)
        self.npart_ = int(npart)
        self.rt_ = int(rt)
        self.weight_ = np.asarray(list(weight), dtype=np.float32)
        if self.weight_.shape[0] != self.npart_:
            raise PconvError("context: %d weights for %d tiles" % (self.weight_.shape[0], self.npart_))
        self.data_width_ = -1
        self._cache = {}
        self._addr = "pconv-ctx-%x" % id(self)
        _contexts[self._addr] = self

    def addr(self):
        return self._addr

    def start_context(self, width):
        if int(width) != self.data_width_:
            self._cache = {}
        self.data_width_ = int(width)

    def _moved(self):
        self._cache = {}

    def widths_host(self, height, width):
        key = ("wh", int(width))
        if key not in self._cache:
            self._cache[key] = tile_widths(self.weight_, self.npart_, int(height) * self.npart_, int(width))
        return self._cache[key]

    def widths(self, height, width, like):
        key = ("wd", int(width), like.device)
        if key not in self._cache:
            self._cache[key] = self._upload(self.widths_host(height, width), like)
        return self._cache[key]

    def produce_fill_param(self, height, width):
        dev = self._dev()
        key = ("wd", int(width), dev)
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(self.widths_host(height, width).copy()).to(dev)
        return self._cache[key]


class PseudoContextOp(_TileContext):
    """PCONV.PseudoContextOp (main.cpp:90-95, pseudo_context_cuda.cu:12-48,140-167)."""

    def pad_tables(self, height, width, pad, like):
        key = ("pad", int(height), int(width), int(pad), like.device)
        if key not in self._cache:
            wh = self.widths_host(height, width)
            n = self.npart_ * 2 * max(pad, 1)
            src_tile = np.zeros(n, np.int32)
            src_row = np.zeros(n, np.int32)
            col = np.zeros(n * width, np.int32)
            wgt = np.zeros(n * width, np.float32)
            if pad > 0:
                call("pconv_host_pad_table", _np_ptr(wh), self.npart_, height, width, pad,
                     _np_ptr(src_tile), _np_ptr(src_row), _np_ptr(col), _np_ptr(wgt))
            self._cache[key] = tuple(self._upload(a, like) for a in (src_tile, src_row, col, wgt))
        return self._cache[key]

    def pad_reverse_tables(self, height, width, pad, like):
        """reverse CSR of pad_tables for PseudoPadOp.backward (pconv_host_pad_reverse)"""
        key = ("padrev", int(height), int(width), int(pad), like.device)
        if key not in self._cache:
            wh = self.widths_host(height, width)
            start = np.zeros(self.npart_ * height * width + 1, np.int32)
            cap = max(4 * self.npart_ * pad * width, 1)   # (pad 0: no records, but no empty buffers either)
            dst = np.zeros(cap, np.int32)
            wgt = np.zeros(cap, np.float32)
            call("pconv_host_pad_reverse", _np_ptr(wh), self.npart_, height, width, pad, _np_ptr(start), _np_ptr(dst),
                 _np_ptr(wgt))
            self._cache[key] = tuple(self._upload(a, like) for a in (start, dst, wgt))
        return self._cache[key]


class PseudoEntropyContextOp(_TileContext):
    """PCONV.PseudoEntropyContextOp(npart, rt, context_version, weight, device, timeit)
    (main.cpp:109-113, pseudo_entropy_context_cuda.cu:51-240): tile widths for PseudoFill and
    the causal halo table (+ its reverse) of the training-time PseudoEntropyPad."""

    def __init__(self, npart, rt, context_version, weight, device=0, timeit=False):
        super().__init__(npart, rt, weight, device, timeit)
        self.context_version_ = int(context_version)
        if self.context_version_ not in (0, 1):
            raise ValueError("PseudoEntropyContextOp: undefined context version %r" % (context_version,))

    def causal_tables(self, height, width, pad, like):
        """(col, wgt): per (tile, side, halo row, column) first source column (-2 none, -1 second
        tap only) and its weight"""
        key = ("cpad", int(height), int(width), int(pad), like.device)
        if key not in self._cache:
            wh = self.widths_host(height, width)
            n = self.npart_ * 2 * pad * width
            col, wgt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
            if pad > 0:    # (pad 0: no halo rows, the kernel copies the valid columns and zeroes the rest)
                call("pconv_host_entropy_pad_table", _np_ptr(wh), self.npart_, height, width, pad,
                     self.context_version_, _np_ptr(col), _np_ptr(wgt))
            self._cache[key] = tuple(self._upload(a, like) for a in (col, wgt))
        return self._cache[key]

    def causal_reverse_tables(self, height, width, pad, like):
        """reverse CSR of causal_tables for PseudoEntropyPadOp.backward (pconv_host_causal_reverse)"""
        key = ("cpadrev", int(height), int(width), int(pad), like.device)
        if key not in self._cache:
            wh = self.widths_host(height, width)
            start = np.zeros(self.npart_ * height * width + 1, np.int32)
            cap = max(4 * self.npart_ * pad * width, 1)   # (pad 0: no records, but no empty buffers either)
            dst, wgt = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
            call("pconv_host_causal_reverse", _np_ptr(wh), self.npart_, height, width, pad,
                 self.context_version_, _np_ptr(start), _np_ptr(dst), _np_ptr(wgt))
            self._cache[key] = tuple(self._upload(a, like) for a in (start, dst, wgt))
        return self._cache[key]


class EntropyContextOp(_TileContext):
    """PCONV.EntropyContextOp (main.cpp:55-59, entropy_context_cuda.cu:13-222):
    wavefront schedule + causal halo lists."""

    def schedule(self, height, width, like):
        key = ("sched", int(height), int(width), like.device)
        if key not in self._cache:
            wh = self.widths_host(height, width)
            rows = height * self.npart_
            order = np.zeros(rows * width, np.int32)
            start = np.zeros(rows + width, np.int32)
            call("pconv_host_wavefront", _np_ptr(wh), self.npart_, height, width, _np_ptr(order),
                 _np_ptr(start))
            self._cache[key] = (self._upload(order, like), start)
            self._cache[("sched_dev",) + key[1:]] = (self._upload(start, like), int(np.diff(start).max()))
        return self._cache[key]

    def schedule_device(self, height, width, like):
        """(plane_start on the device, longest plane) of the same schedule"""
        self.schedule(height, width, like)
        return self._cache[("sched_dev", int(height), int(width), like.device)]

    def causal_halo(self, channel, height, width, pad, like):
        key = ("halo", int(channel), int(height), int(width), int(pad), like.device)
        if key not in self._cache:
            wh = self.widths_host(height, width)
            nplane = height * self.npart_ + width + pad - 1
            start = np.zeros(nplane + 1, np.int32)
            n = call("pconv_host_causal_halo", _np_ptr(wh), self.npart_, channel, height, width, pad,
                     None, None, None, None, None, _np_ptr(start))
            arrs = [np.zeros(max(n, 1), np.int32) for _ in range(3)]
            wgt = np.zeros(max(n, 1), np.float32)
            plane = np.zeros(max(n, 1), np.int32)
            call("pconv_host_causal_halo", _np_ptr(wh), self.npart_, channel, height, width, pad,
                 _np_ptr(arrs[0]), _np_ptr(arrs[1]), _np_ptr(arrs[2]), _np_ptr(wgt), _np_ptr(plane),
                 _np_ptr(start))
            dev = tuple(self._upload(a, like) for a in (arrs[0], arrs[1], arrs[2], wgt, plane))
            self._cache[key] = (dev, start)
        return self._cache[key]


# ---------------------------------------------------------------------------
# transform-path ops
# ---------------------------------------------------------------------------
class DtowOp(_Op):
    """PCONV.DtowOp(stride, d2w, device, timeit) (main.cpp:12-16, dtow_cuda.cu:11-103)."""

    def __init__(self, stride, d2w, device=0, timeit=False):
        super().__init__(device, timeit)
        self.stride_ = int(stride)
        self.d2w_ = bool(d2w)

    def forward(self, x):
        _require_gpu(x, "DtowOp")
        n, c, h, w = x.shape
        s = self.stride_
        shape = (n, c // (s * s), h * s, w * s) if self.d2w_ else (n, c * s * s, h // s, w // s)
        out = self._out(0, shape, x)
        with _HbmTimed("dtow2_kernel" if self.d2w_ else "wtod2_kernel", "Dtow c%d w%d" % (c, w), 8.0 * x.numel(), x.device):
            call("pconv_dtow", _ptr(x), _ptr(out), n, c, h, w, s, int(self.d2w_), _stream(x.device))
        return [out]

    def backward(self, grad):
        # the inverse permutation (dtow_cuda.cu:105-167)
        _require_gpu(grad, "DtowOp.backward")
        n, c, h, w = grad.shape
        s = self.stride_
        shape = (n, c * s * s, h // s, w // s) if self.d2w_ else (n, c // (s * s), h * s, w * s)
        out = self._out(1, shape, grad)
        call("pconv_dtow", _ptr(grad), _ptr(out), n, c, h, w, s, int(not self.d2w_), _stream(grad.device))
        return [out]


class ContextReshapeOp(_Op):
    """PCONV.ContextReshapeOp(ngroup, device, timeit) (main.cpp:18-22)."""

    def __init__(self, ngroup, device=0, timeit=False):
        super().__init__(device, timeit)
        self.ngroup_ = int(ngroup)

    def forward(self, x):
        _require_gpu(x, "ContextReshapeOp")
        n, c, h, w = x.shape
        out = self._out(0, (n * h * w * self.ngroup_, c // self.ngroup_), x)
        self._fwd_shape = (n, c, h, w)
        call("pconv_context_reshape", _ptr(x), _ptr(out), n, c, h, w, self.ngroup_, _stream(x.device))
        return [out]

    def backward(self, grad):
        """(n*g*h*w, cpg) -> (n, g*cpg, h, w): the inverse permutation (context_reshape_cuda.cu:63-95)"""
        _require_gpu(grad, "ContextReshapeOp.backward")
        n, c, h, w = self._fwd_shape
        if tuple(grad.shape) != (n * h * w * self.ngroup_, c // self.ngroup_):
            raise PconvError("ContextReshapeOp.backward: grad %s does not fit the forward's input %s" % (tuple(grad.shape), (n, c, h, w)))
        out = self._out(1, (n, c, h, w), grad)
        call("pconv_context_reshape_backward", _ptr(grad), _ptr(out), n, c, h, w, self.ngroup_, _stream(grad.device))
        return [out]


class EntropyGmmOp(_Op):
    """PCONV.EntropyGmmOp(num_gaussian, ignore_label, device, timeit) (main.cpp:24-28)."""

    def __init__(self, num_gaussian, ignore_label, device=0, timeit=False):
        super().__init__(device, timeit)
        self.num_gaussian_ = int(num_gaussian)
        self.ignore_label_ = int(ignore_label)

    def forward(self, weight, delta, mean, label):
        """weight, delta, mean (m, num_gaussian), label m values: contiguous float32 on one GPU"""
        for name, t in (("weight", weight), ("delta", delta), ("mean", mean), ("label", label)):
            _require_gpu(t, "EntropyGmmOp: " + name)
        if weight.dim() != 2 or weight.shape[1] != self.num_gaussian_:
            raise PconvError("EntropyGmmOp: weight %s: (m, num_gaussian = %d) expected" % (tuple(weight.shape), self.num_gaussian_))
        m, ng = weight.shape
        for name, t, count in (("delta", delta, m * ng), ("mean", mean, m * ng), ("label", label, m)):
            if t.numel() != count or t.device != weight.device:
                raise PconvError("EntropyGmmOp: %s %s on %s does not fit weight %s on %s"
                                 % (name, tuple(t.shape), t.device, tuple(weight.shape), weight.device))
        loss = self._out(0, (m,), weight)
        dw = self._out(1, (m, ng), weight)
        dd = self._out(2, (m, ng), weight)
        dm = self._out(3, (m, ng), weight)
        dl = self._out(4, (m, 1), weight)
        call("pconv_gmm_loss", _ptr(weight), _ptr(delta), _ptr(mean), _ptr(label), _ptr(loss), _ptr(dw),
             _ptr(dd), _ptr(dm), _ptr(dl), m, ng, _stream(weight.device))
        return [loss]

    def backward(self, grad):
        """the per-row derivatives the forward kernel left in the op's buffers, times the
        incoming gradient (entropy_gmm_cuda.cu:95-127): [d weight, d delta, d mean, d label]"""
        _require_gpu(grad, "EntropyGmmOp.backward")
        if 1 not in self._top or grad.numel() != self._top[1].shape[0] or grad.device != self._top[1].device:
            raise PconvError("EntropyGmmOp.backward: grad %s does not fit the forward's %d rows"
                             % (tuple(grad.shape), self._top[1].shape[0] if 1 in self._top else 0))
        g = grad.reshape(-1, 1)
        return [self._top[1] * g, self._top[2] * g, self._top[3] * g, self._top[4] * g]


class MaskConstrainOp(_Op):
    """PCONV.MaskConstrainOp(constrain, ngroup, device, timeit) (main.cpp:30-34)."""

    def __init__(self, constrain, ngroup, device=0, timeit=False):
        super().__init__(device, timeit)
        self.constrain_ = int(constrain)
        self.ngroup_ = int(ngroup)

    def forward(self, w):
        _require_gpu(w, "MaskConstrainOp")
        nout, cin, k, k2 = w.shape
        call("pconv_mask_constrain", _ptr(w), nout, cin, k, self.ngroup_, self.constrain_, _stream(w.device))

    def backward(self, grad):
        self.forward(grad)


class _SphereResample(_Op):
    def __init__(self, npart, interp_type, pad, weight, device=0, timeit=False):
        super().__init__(device, timeit)
        self.npart_ = int(npart)
        self.interp_type_ = int(interp_type)
        self.pad_ = int(pad)
        self.weight_ = np.asarray(list(weight), dtype=np.float32)
        self._tabs = {}

    def _moved(self):
        self._tabs = {}

    def _widths(self, height, width):
        return tile_widths(self.weight_, self.npart_, height, width)

    def _host_taps(self, builder, height, width):
        wh = self._widths(height, width)
        col = np.zeros(self.npart_ * width, np.int32)
        coef = np.zeros(self.npart_ * width * 4, np.float32)
        call(builder, _np_ptr(wh), self.npart_, width, _np_ptr(col), _np_ptr(coef))
        return wh, col, coef

    def _tables(self, builder, height, width, like):
        key = (int(height), int(width), like.device)
        if key not in self._tabs:
            self._tabs[key] = tuple(self._upload(a, like) for a in self._host_taps(builder, height, width))
        return self._tabs[key]

    def _reverse_tables(self, builder, uslice, height, width, like):
        """widths and the reverse CSR of _tables (pconv_host_tap_reverse) for the ordered backward, cached beside
        the forward tables"""
        key = ("reverse", int(height), int(width), like.device)
        if key not in self._tabs:
            wh, col, coef = self._host_taps(builder, height, width)
            count = call("pconv_host_tap_reverse_size", _np_ptr(wh), self.npart_, width, uslice)
            start = np.zeros(self.npart_ * width + 1, np.int32)
            src, rcoef = np.zeros(count, np.int32), np.zeros(count, np.float32)
            call("pconv_host_tap_reverse", _np_ptr(wh), self.npart_, width, _np_ptr(col), _np_ptr(coef), uslice,
                 _np_ptr(start), _np_ptr(src), _np_ptr(rcoef))
            self._tabs[key] = tuple(self._upload(a, like) for a in (wh, start, src, rcoef))
        return self._tabs[key]


class SphereSliceOp(_SphereResample):
    """PCONV.SphereSliceOp(npart, interp, pad, weight, device, timeit)
    (main.cpp:37-41, sphere_slice_cuda.cu:55-146)."""

    def _widths(self, height, width):
        """sphere_cal_npart_hw_v2's rule (math_cuda.cu:177-221), which differs from every other op's at a weight
        total of exactly 3 * npart"""
        return tile_widths(self.weight_, self.npart_, height, width, "pconv_host_slice_widths")

    def forward(self, x):
        _require_gpu(x, "SphereSliceOp")
        n, c, h, w = x.shape
        if h % self.npart_:
            raise PconvError("SphereSliceOp: height %d is not a multiple of npart %d" % (h, self.npart_))
        wd, col, coef = self._tables("pconv_host_slice_taps", h, w, x)
        p = self.pad_
        out = self._out(0, (n * self.npart_, c, h // self.npart_ + 2 * p, w + 2 * p), x, zero=p > 0)
        with _HbmTimed("slice_kernel", "SphereSlice w%d" % w, 8.0 * x.numel(), x.device):
            call("pconv_sphere_slice", _ptr(x), _ptr(out), _ptr(wd), _ptr(col), _ptr(coef), n, c, h, w,
                 self.npart_, p, _stream(x.device))
        return [out]

    def backward(self, grad):
        """grad of the tile stack -> grad of the ERP image: the transpose of the 4-tap resampling
        (sphere_slice_cuda.cu:191-244)"""
        _require_gpu(grad, "SphereSliceOp.backward")
        tn, c, hp, wp = grad.shape
        p = self.pad_
        n, h, w = tn // self.npart_, (hp - 2 * p) * self.npart_, wp - 2 * p
        out = self._out(1, (n, c, h, w), grad)
        if ordered_backward.on:
            wd, rs, rc, rw = self._reverse_tables("pconv_host_slice_taps", 0, h, w, grad)
            _backward_call("pconv_sphere_slice_backward_ordered", _ptr(grad), _ptr(out), _ptr(wd), _ptr(rs), _ptr(rc),
                           _ptr(rw), n, c, h, w, self.npart_, p, _stream(grad.device))
            return [out]
        wd, col, coef = self._tables("pconv_host_slice_taps", h, w, grad)
        _backward_call("pconv_sphere_slice_backward", _ptr(grad), _ptr(out), _ptr(wd), _ptr(col), _ptr(coef), n, c, h, w,
                       self.npart_, p, _stream(grad.device))
        return [out]


class SphereUsliceOp(_SphereResample):
    """PCONV.SphereUsliceOp (main.cpp:43-47, sphere_uslice_cuda.cu:32-126)."""

    def forward(self, x):
        _require_gpu(x, "SphereUsliceOp")
        p = self.pad_
        tn, c, hp, wp = x.shape
        h, w = hp - 2 * p, wp - 2 * p
        if tn % self.npart_:
            raise PconvError("SphereUsliceOp: batch %d is not a multiple of npart %d" % (tn, self.npart_))
        n = tn // self.npart_
        wd, col, coef = self._tables("pconv_host_uslice_taps", h * self.npart_, w, x)
        out = self._out(0, (n, c, h * self.npart_, w), x)
        with _HbmTimed("uslice_kernel", "SphereUslice w%d" % out.shape[3], 8.0 * out.numel(), x.device):
            call("pconv_sphere_uslice", _ptr(x), _ptr(out), _ptr(wd), _ptr(col), _ptr(coef), n, c, h, w,
                 self.npart_, p, _stream(x.device))
        return [out]

    def forward_into(self, x, out):
        """forward() with the caller's output tensor (n, c, h * npart, w), contiguous -- a frame of a batch the
        caller assembles: no op-owned buffer, no copy afterwards (engine.CodecEngine.reconstruct)"""
        _require_gpu(x, "SphereUsliceOp.forward_into: x")
        p = self.pad_
        tn, c, hp, wp = x.shape
        h, w = hp - 2 * p, wp - 2 * p
        n = tn // self.npart_
        if tn % self.npart_:
            raise PconvError("SphereUsliceOp.forward_into: x: batch %d is not a multiple of npart %d" % (tn, self.npart_))
        _require_operand(out, "SphereUsliceOp.forward_into", "out", (n, c, h * self.npart_, w), torch.float32, x)
        wd, col, coef = self._tables("pconv_host_uslice_taps", h * self.npart_, w, x)
        with _HbmTimed("uslice_kernel", "SphereUslice w%d" % out.shape[3], 8.0 * out.numel(), x.device):
            call("pconv_sphere_uslice", _ptr(x), _ptr(out), _ptr(wd), _ptr(col), _ptr(coef), n, c, h, w,
                 self.npart_, p, _stream(x.device))
        return out

    def backward(self, grad):
        """grad of the ERP image -> grad of the (padded) tile stack, zero outside the valid
        interior (sphere_uslice_cuda.cu:128-200)"""
        _require_gpu(grad, "SphereUsliceOp.backward")
        n, c, hh, w = grad.shape
        p = self.pad_
        h = hh // self.npart_
        out = self._out(1, (n * self.npart_, c, h + 2 * p, w + 2 * p), grad)
        if ordered_backward.on:
            wd, rs, rc, rw = self._reverse_tables("pconv_host_uslice_taps", 1, hh, w, grad)
            _backward_call("pconv_sphere_uslice_backward_ordered", _ptr(grad), _ptr(out), _ptr(wd), _ptr(rs), _ptr(rc),
                           _ptr(rw), n, c, h, w, self.npart_, p, _stream(grad.device))
            return [out]
        wd, col, coef = self._tables("pconv_host_uslice_taps", hh, w, grad)
        _backward_call("pconv_sphere_uslice_backward", _ptr(grad), _ptr(out), _ptr(wd), _ptr(col), _ptr(coef), n, c, h, w,
                       self.npart_, p, _stream(grad.device))
        return [out]


class PseudoPadOp(_Op):
    """PCONV.PseudoPadOp(pad, npart, ctx_addr, device, timeit)
    (main.cpp:97-101, pseudo_pad.cu:12-125); one fused launch."""

    def __init__(self, pad, npart, ctx_addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.pad_ = int(pad)
        self.npart_ = int(npart)
        self.ctx_ = _lookup(ctx_addr)

    def forward(self, x):
        _require_gpu(x, "PseudoPadOp")
        tn, c, h, w = x.shape
        p = self.pad_
        wd = self.ctx_.widths(h, w, x)
        st, sr, col, wgt = self.ctx_.pad_tables(h, w, p, x)
        out = self._out(0, (tn, c, h + 2 * p, w + 2 * p), x)
        with _HbmTimed("pseudo_pad_kernel", "PseudoPad c%d w%d p%d" % (c, w, p), 4.0 * (x.numel() + out.numel()), x.device):
            call("pconv_pseudo_pad", _ptr(x), _ptr(out), _ptr(wd), _ptr(st), _ptr(sr), _ptr(col), _ptr(wgt), tn,
                 c, h, w, p, self.npart_, _stream(x.device))
        return [out]

    def forward_ring(self, x):
        """x is the interior view of a padded buffer (`x._pconv_ring = (buffer, store)`, set by
        tile_conv2d / tile_gdn with ring > 0): fill the ring of this op's pad in place and
        return the padded view -- no copy of the tensor."""
        ring = getattr(x, "_pconv_ring", None)
        if ring is None or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            raise PconvError("PseudoPadOp.forward_ring: x must be the float32 interior view of a ring buffer on a GPU "
                             "(the result of tile_conv2d / tile_gdn with ring > 0)")
        buf, store = ring
        tn, c, h, w = x.shape
        if tuple(buf.shape) == (tn, c, h + 2 * store, w + 2 * store) and (
                buf.dtype != x.dtype or buf.device != x.device or x.stride() != buf.stride()
                or x.data_ptr() != buf.data_ptr() + 4 * store * (buf.stride(2) + 1)):
            # (a buffer of another shape: the copying pad below reads x alone)
            raise PconvError("PseudoPadOp.forward_ring: x %s %s on %s is not the interior view of its ring buffer %s %s on %s"
                             % (x.dtype, tuple(x.shape), x.device, buf.dtype, tuple(buf.shape), buf.device))
        p = self.pad_
        if p <= 0 or p > store or tuple(buf.shape) != (tn, c, h + 2 * store, w + 2 * store) or not buf.is_contiguous():
            return self.forward(x.contiguous())[0]
        wd = self.ctx_.widths(h, w, x)
        st, sr, col, wgt = self.ctx_.pad_tables(h, w, p, x)
        with _HbmTimed("pseudo_pad_ring_kernel", "PseudoPad ring c%d w%d p%d" % (c, w, p), 4.0 * tn * c * ((h + 2 * p) * (w + 2 * p) - h * w), x.device):
            call("pconv_pseudo_pad_ring", _ptr(buf), _ptr(wd), _ptr(st), _ptr(sr), _ptr(col), _ptr(wgt), tn, c, h, w, p,
                 store, self.npart_, _stream(x.device))
        d = store - p
        return buf if d == 0 else buf[:, :, d:-d, d:-d]

    def backward(self, grad):
        """grad (tn, c, h+2p, w+2p) -> (tn, c, h, w): interior + folded wrap columns + the halo
        entries interpolated from each element (pseudo_pad.cu:127-235)"""
        _require_gpu(grad, "PseudoPadOp.backward")
        tn, c, hp, wp = grad.shape
        p = self.pad_
        h, w = hp - 2 * p, wp - 2 * p
        wd = self.ctx_.widths(h, w, grad)
        rs, rd, rw = self.ctx_.pad_reverse_tables(h, w, p, grad)
        out = self._out(1, (tn, c, h, w), grad)
        call("pconv_pseudo_pad_backward", _ptr(grad), _ptr(out), _ptr(wd), _ptr(rs), _ptr(rd), _ptr(rw), tn, c, h, w,
             p, self.npart_, _stream(grad.device))
        return [out]


class PseudoFillOp(_Op):
    """PCONV.PseudoFillOp(pad, npart, fvalue, trim, addr, context_version, device, timeit)
    (main.cpp:103-107, pseudo_fill_cuda.cu:11-77); in place."""

    def __init__(self, pad, npart, fvalue, trim, addr, context_version, device=0, timeit=False):
        super().__init__(device, timeit)
        self.pad_, self.npart_ = int(pad), int(npart)
        self.fvalue_, self.trim_ = int(fvalue), int(trim)
        self.context_version_ = int(context_version)
        self.ctx_ = _lookup(addr)

    def _run(self, x, value):
        _require_gpu(x, "PseudoFillOp")
        tn, c, h, w = x.shape
        wd = self.ctx_.widths(h, w, x)
        with _HbmTimed("pseudo_fill_kernel", "PseudoFill c%d w%d" % (c, w), 4.0 * x.numel() * (1.0 - _VALID_FRACTION), x.device):
            call("pconv_pseudo_fill", _ptr(x), _ptr(wd), tn, c, h, w, self.npart_, self.pad_, self.trim_,
                 float(value), _stream(x.device))
        return [x]

    def forward(self, x):
        return self._run(x, self.fvalue_)

    def backward(self, grad):
        return self._run(grad, 0.0)


class PseudoEntropyPadOp(_Op):
    """PCONV.PseudoEntropyPadOp(pad, npart, addr, device, timeit) (main.cpp:115-119,
    pseudo_entropy_pad_cuda.cu:39-241): causal pad of the training-time EntropyNet."""

    def __init__(self, pad, npart, addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.pad_, self.npart_ = int(pad), int(npart)
        self.ctx_ = _lookup(addr)
        if not isinstance(self.ctx_, PseudoEntropyContextOp):
            raise TypeError("PseudoEntropyPadOp needs the address of a PseudoEntropyContextOp")

    def forward(self, x):
        _require_gpu(x, "PseudoEntropyPadOp.forward")
        tn, c, h, w = x.shape
        p = self.pad_
        wd = self.ctx_.widths(h, w, x)
        col, wgt = self.ctx_.causal_tables(h, w, p, x)
        out = self._out(0, (tn, c, h + 2 * p, w + 2 * p), x)
        call("pconv_entropy_pad", _ptr(x), _ptr(out), _ptr(wd), _ptr(col), _ptr(wgt), tn, c, h, w, p, self.npart_,
             _stream(x.device))
        return [out]

    def backward(self, grad):
        _require_gpu(grad, "PseudoEntropyPadOp.backward")
        tn, c, hp, wp = grad.shape
        p = self.pad_
        h, w = hp - 2 * p, wp - 2 * p
        wd = self.ctx_.widths(h, w, grad)
        rs, rd, rw = self.ctx_.causal_reverse_tables(h, w, p, grad)
        out = self._out(1, (tn, c, h, w), grad)
        call("pconv_entropy_pad_backward", _ptr(grad), _ptr(out), _ptr(wd), _ptr(rs), _ptr(rd), _ptr(rw), tn, c, h,
             w, p, self.npart_, _stream(grad.device))
        return [out]


class PseudoQuantOp(_Op):
    """PCONV.PseudoQuantOp(channel, bins, npart, decay, check_iters, ntop, top_alpha, addr,
    device, timeit) (main.cpp:121-125, pseudo_quant_cuda.cu:157-194); eval forward."""

    def __init__(self, channel, bin_num, npart, weight_decay, check_iters, ntop, top_alpha, addr,
                 device=0, timeit=False):
        super().__init__(device, timeit)
        self.channel_, self.bin_num_, self.npart_ = int(channel), int(bin_num), int(npart)
        self.ntop_ = int(ntop)
        self.top_alpha_ = float(top_alpha)
        self.weight_decay_, self.mod_ = float(weight_decay), int(check_iters)
        self.iter_ = 0
        self.count_data_ = None
        self.ctx_ = _lookup(addr)

    def update_weight(self, weight, ncount):
        """Every `check_iters` training-mode calls: merge quantiser levels that the
        running histogram `ncount` says are unused, then decay the histogram
        (pseudo_quant_cuda.cu:97-143).  The reference's codec driver never calls
        .eval(), so this path is live there too (pseudo_codec.py:241-246)."""
        if self.iter_ % self.mod_ != 0 or self.iter_ == 0:
            return
        levels = self.bin_num_
        w, cnt = weight.data, ncount.data
        used = cnt >= 1e-3
        idx = torch.arange(levels, device=w.device).expand_as(w)
        top = torch.where(used & (idx >= 2), idx, torch.ones_like(idx)).max(dim=1).values  # last used level, >= 1
        base = w.gather(1, top[:, None])[:, 0] - torch.log((levels - top).to(w.dtype))
        w.copy_(torch.where(idx >= top[:, None], base[:, None].expand_as(w), w))
        empty0 = cnt[:, 0] < 1e-3
        if bool(empty0.any()):
            w0 = w[:, 0] + torch.exp(w[:, 1])
            merged = torch.log((torch.exp(w[:, 1]) + torch.exp(w[:, 2])) / 2)
            w[:, 0] = torch.where(empty0, w0, w[:, 0])
            w[:, 1] = torch.where(empty0, merged, w[:, 1])
            w[:, 2] = torch.where(empty0, merged, w[:, 2])
        cnt.mul_(self.weight_decay_)

    def forward(self, x, weight, count, train):
        """x (tn, channel, h, w) and the level table weight (channel, bins): contiguous float32 on one GPU; count: the
        module's running histogram, read and written by torch arithmetic in training mode only"""
        _require_gpu(x, "PseudoQuantOp: x")
        tn, c, h, w = x.shape
        if c != self.channel_:
            raise PconvError("PseudoQuantOp: x has %d channels, built for %d" % (c, self.channel_))
        _require_operand(weight, "PseudoQuantOp", "weight", (c, self.bin_num_), torch.float32, x)
        if train:
            self.update_weight(weight, count)
        wd = self.ctx_.widths(h, w, x)
        tab = self._out("tab", (c, self.bin_num_), x)
        val = self._out(0, x.shape, x)
        idx = self._out(1, x.shape, x)  # kept for backward even when only the value is returned
        # per-call histogram of the levels hit, -1 per valid element: the op's own
        # count_data_ (pseudo_quant_cuda.cu:12,64,83,167), zeroed on every call; the
        # reference hands it to autograd as the "gradient" of the module's `count`
        self.count_data_ = self._out("count", (c, self.bin_num_), x)
        self.count_data_.zero_()
        # (r6) the histogram has one reader, the training graph (backward hands it to `count` as its "gradient"): an
        # eval-mode call under no_grad -- the codec -- leaves it zero and takes the kernel's 16-byte form
        hist = self.count_data_ if (train or torch.is_grad_enabled()) else None
        with _HbmTimed("quant_kernel", "PseudoQuant c%d w%d" % (x.shape[1], x.shape[3]), 12.0 * x.numel(), x.device):
            call("pconv_quant", _ptr(x), _ptr(weight.detach()), _ptr(tab), _ptr(val), _ptr(idx), _ptr(hist),
                 _ptr(wd), tn, c, h, w, self.bin_num_, self.npart_, _stream(x.device))
        if train:
            self.iter_ += 1
        return [val, idx] if self.ntop_ > 1 else [val]

    def backward(self, grads, x, out):
        """[g_val(, g_idx)], the forward's input and value output -> [g_x, g_weight, count_data_]
        (pseudo_quant_cuda.cu:197-311): straight-through for the value, the index gradient scaled
        by the local level width, the quantisation error summed into the levels at or below each
        element's level; the per-call histogram is what the reference hands back for `count`.  x and out: contiguous
        float32 of the forward's shape; the gradients: float32 of that shape on x's device, strided ones accepted (they
        are made contiguous)."""
        _require_gpu(x, "PseudoQuantOp.backward: x")
        tn, c, h, w = x.shape
        if self.count_data_ is None or 1 not in self._top or tuple(self._top[0].shape) != tuple(x.shape):
            raise PconvError("PseudoQuantOp.backward: no matching forward call for x %s" % (tuple(x.shape),))
        _require_operand(out, "PseudoQuantOp.backward", "out", x.shape, torch.float32, x)
        # (the gradients are made contiguous: strided ones are accepted)
        g_val = _require_operand(grads[0], "PseudoQuantOp.backward", "grads[0]", x.shape, torch.float32, x, dense=False).contiguous()
        g_idx = None
        if self.ntop_ > 1 and len(grads) > 1 and grads[1] is not None:
            g_idx = _require_operand(grads[1], "PseudoQuantOp.backward", "grads[1]", x.shape, torch.float32, x, dense=False).contiguous()
        wd = self.ctx_.widths(h, w, x)
        g_in = self._out("g_in", x.shape, x)
        g_w = self._out("g_w", (c, self.bin_num_), x)
        bins = self._out("bins", (c, self.bin_num_), x)
        if ordered_backward.on:
            nbytes = call("pconv_quant_backward_ordered_workspace_bytes", tn, c, self.bin_num_)
            ws = self._top.get("partials")
            if ws is None or ws.numel() != nbytes or ws.device != x.device:
                ws = self._top["partials"] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            _backward_call("pconv_quant_backward_ordered", _ptr(x), _ptr(out), _ptr(self._top[1]), _ptr(g_val), _ptr(g_idx),
                           _ptr(self._top["tab"]), _ptr(g_in), _ptr(g_w), _ptr(bins), _ptr(ws), _ptr(wd), self.top_alpha_,
                           tn, c, h, w, self.bin_num_, self.npart_, _stream(x.device))
            return [g_in, g_w, self.count_data_]
        _backward_call("pconv_quant_backward", _ptr(x), _ptr(out), _ptr(self._top[1]), _ptr(g_val), _ptr(g_idx),
             _ptr(self._top["tab"]), _ptr(g_in), _ptr(g_w), _ptr(bins), _ptr(wd), self.top_alpha_, tn, c, h, w,
             self.bin_num_, self.npart_, _stream(x.device))
        return [g_in, g_w, self.count_data_]


class PseudoDQuantOp(_Op):
    """PCONV.PseudoDQuantOp(npart, channel, bins, addr, device, timeit)
    (main.cpp:127-130, pseudo_dquant_cuda.cu:11-70)."""

    def __init__(self, npart, channel, bin_num, addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.npart_, self.nchannel_, self.bin_num_ = int(npart), int(channel), int(bin_num)
        self.ctx_ = _lookup(addr)

    def forward(self, x, weight):
        """x (tn, c, h, w) and the level table weight (channel, bins): contiguous float32 on one GPU"""
        _require_gpu(x, "PseudoDQuantOp: x")
        tn, c, h, w = x.shape
        _require_operand(weight, "PseudoDQuantOp", "weight", (self.nchannel_, self.bin_num_), torch.float32, x)
        wd = self.ctx_.widths(h, w, x)
        tab = self._out("tab", (self.nchannel_, self.bin_num_), x)
        out = self._out(0, x.shape, x)
        with _HbmTimed("dquant_kernel", "PseudoDQuant c%d w%d" % (c, w), 8.0 * x.numel(), x.device):
            call("pconv_dquant", _ptr(x), _ptr(weight.detach()), _ptr(tab), _ptr(out), _ptr(wd), tn, c, h, w,
                 self.nchannel_, self.bin_num_, self.npart_, _stream(x.device))
        return [out]


class ProjectsOp(_Op):
    """PCONV.ProjectsOp(h, w, thetas, phis, fov, near, device, timeit)
    (main.cpp:6-10, projects_cuda.cu:98-255)."""

    def __init__(self, h_out, w_out, thetas, phis, fov=0.33333, near=False, device=0, timeit=False):
        super().__init__(device, timeit)
        self.h_out_, self.w_out_ = int(h_out), int(w_out)
        self.theta_ = np.asarray(list(thetas), np.float32)
        self.phi_ = np.asarray(list(phis), np.float32)
        if self.theta_.shape != self.phi_.shape:
            raise PconvError("ProjectsOp: thetas and phis differ in length")
        self.nview_ = int(self.theta_.shape[0])
        self.fov_, self.near_ = float(fov), bool(near)
        self._tf = {}
        self._rev = {}

    def _moved(self):
        self._tf = {}
        self._rev = {}

    def _table(self, h, w, like):
        key = (h, w, like.device)
        if key not in self._tf:
            tf = np.zeros(self.nview_ * self.h_out_ * self.w_out_ * 2, np.float32)
            call("pconv_host_project_table", _np_ptr(self.theta_), _np_ptr(self.phi_), self.nview_, self.fov_,
                 self.h_out_, self.w_out_, h, w, _np_ptr(tf))
            self._tf[key] = self._upload(tf, like)
        return self._tf[key]

    def _reverse_tables(self, h, w, like):
        """reverse CSR of the sampling table (pconv_host_project_reverse) for the ordered backward, cached beside it"""
        key = (h, w, like.device)
        if key not in self._rev:
            tf = self._table(h, w, like).cpu().numpy()
            inner = self.h_out_ * self.w_out_
            count = call("pconv_host_project_reverse_size", self.nview_, inner, int(self.near_))
            start = np.zeros(h * w + 1, np.int32)
            sample, wgt = np.zeros(count, np.int32), np.zeros(count, np.float32)
            call("pconv_host_project_reverse", _np_ptr(tf), self.nview_, inner, h, w, int(self.near_), _np_ptr(start),
                 _np_ptr(sample), _np_ptr(wgt))
            self._rev[key] = tuple(self._upload(a, like) for a in (start, sample, wgt))
        return self._rev[key]

    def forward(self, x):
        _require_gpu(x, "ProjectsOp")
        n, c, h, w = x.shape
        tf = self._table(h, w, x)
        out = self._out(0, (n * self.nview_, c, self.h_out_, self.w_out_), x)
        self._fwd_shape = (n, c, h, w)
        call("pconv_project", _ptr(x), _ptr(tf), _ptr(out), n, c, h, w, self.nview_, self.h_out_,
             self.w_out_, int(self.near_), _stream(x.device))
        return [out]

    def backward(self, grad):
        """grad of the viewports -> [grad of the ERP image, sampling-weight count]
        (projects_cuda.cu:257-329)"""
        _require_gpu(grad, "ProjectsOp.backward")
        n, c, h, w = self._fwd_shape
        if tuple(grad.shape) != (n * self.nview_, c, self.h_out_, self.w_out_):
            raise PconvError("ProjectsOp.backward: grad %s does not fit the forward's %s"
                             % (tuple(grad.shape), (n * self.nview_, c, self.h_out_, self.w_out_)))
        gin = self._out(1, (n, c, h, w), grad)
        cnt = self._out(2, (n, c, h, w), grad)
        if ordered_backward.on:
            rs, rc, rw = self._reverse_tables(h, w, grad)
            _backward_call("pconv_project_backward_ordered", _ptr(grad), _ptr(rs), _ptr(rc), _ptr(rw), _ptr(gin), _ptr(cnt),
                           n, c, h, w, self.nview_, self.h_out_, self.w_out_, _stream(grad.device))
            return [gin, cnt]
        _backward_call("pconv_project_backward", _ptr(grad), _ptr(self._table(h, w, grad)), _ptr(gin), _ptr(cnt), n, c, h, w,
                       self.nview_, self.h_out_, self.w_out_, int(self.near_), _stream(grad.device))
        return [gin, cnt]


# ---------------------------------------------------------------------------
# entropy wavefront ops
# ---------------------------------------------------------------------------
class _WavefrontOp(_Op):
    """Step counter shared by the entropy ops: `pidx_` advances on every forward,
    is reset by restart() or a shape change (e.g. d_input_v2.hpp:21,
    d_input_cuda_v2.cu:16)."""

    def __init__(self, device, timeit):
        super().__init__(device, timeit)
        self.pidx_ = 0

    def restart(self):
        self.pidx_ = 0

    def _step(self):
        p = self.pidx_
        self.pidx_ += 1
        return p

    @staticmethod
    def _window(psum, ngroup, last_plane, start):
        """Schedule slice of a step: planes [psum-ngroup+1, psum] clipped to
        [0, last_plane]; returns (lo, len)."""
        st = max(psum - ngroup + 1, 0)
        end = psum + 1 if psum < last_plane else last_plane + 1
        if st >= len(start) or end >= len(start) or st > end:
            return 0, 0
        return int(start[st]), int(start[end] - start[st])


class DInput2Op(_WavefrontOp):
    """PCONV.DInput2Op(nchannel, npart, pad, bias, repeat, addr, device, timeit)
    (main.cpp:75-79, d_input_cuda_v2.cu:13-86)."""

    def __init__(self, nchannel, npart, pad, bias, repeat, addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.channel_, self.npart_, self.pad_ = int(nchannel), int(npart), int(pad)
        self.bias_, self.rep_ = float(bias), int(repeat)
        self.ctx_ = _lookup(addr)

    def forward(self, x):
        _require_gpu(x, "DInput2Op")
        nimg, h, w = x.shape[0], x.shape[2] // self.npart_, x.shape[3]
        if self._reshaped((nimg, h, w)):
            self.pidx_ = 0
        order, start = self.ctx_.schedule(h, w, x)
        p = self.pad_
        top = self._out(0, (self.rep_ * nimg * self.npart_, self.channel_, h + 2 * p, w + 2 * p), x)
        psum = self._step()
        rows = h * self.npart_
        if psum == 0:
            top.zero_()
        elif psum <= rows + w + self.channel_ - 2:
            psum -= 1
            lo, ln = self._window(psum, self.channel_, rows + w - 2, start)
            if ln > 0:
                call("pconv_dinput2", _ptr(x), _ptr(top), _ptr(order), lo, ln, nimg, self.channel_,
                     self.npart_, h, w, p, psum, self.bias_, self.rep_, _stream(x.device))
        return [top]


class EntropyCtxPadRun2Op(_WavefrontOp):
    """PCONV.EntropyCtxPadRun2Op(pad, npart, ngroup, input, ctx_addr, device, timeit)
    (main.cpp:61-66, entropy_ctx_pad_run2_cuda.cu:11-117); in place."""

    def __init__(self, pad, npart, ngroup, input, ctx_addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.pad_, self.npart_, self.ngroup_ = int(pad), int(npart), int(ngroup)
        self.input_ = bool(input)
        self.ctx_ = _lookup(ctx_addr)

    def forward(self, x):
        _require_gpu(x, "EntropyCtxPadRun2Op")
        p = self.pad_
        num, channel, h, w = x.shape[0], x.shape[1], x.shape[2] - 2 * p, x.shape[3] - 2 * p
        if self._reshaped((num, channel, h, w)):
            self.pidx_ = 0
        (dst, s0, s1, wgt, plane), start = self.ctx_.causal_halo(channel, h, w, p, x)
        psum = self._step()
        if self.input_:
            psum -= 1
        rows = h * self.npart_
        if 0 <= psum < rows + w + p + self.ngroup_ - 2:
            lo, ln = self._window(psum, self.ngroup_, rows + w + p - 2, start)
            if ln > 0:
                call("pconv_ctx_pad_run2", _ptr(x), _ptr(dst), _ptr(s0), _ptr(s1), _ptr(wgt), _ptr(plane), lo,
                     ln, num // self.npart_, channel // self.ngroup_, channel, self.npart_, h, w, p, psum,
                     _stream(x.device))
        return [x]

    def backward(self, grad):
        return []


class EntropyConv2Op(_WavefrontOp):
    """PCONV.EntropyConv2Op(npart, channel, ngroup, nout, k, constrain, pad_in, pad_out, addr,
    device, timeit) (main.cpp:81-88, entropy_conv_cuda_v2.cu:11-459)."""

    def __init__(self, npart, channel, ngroup, nout, kernel_size, constrain, pad_in, pad_out, addr,
                 device=0, timeit=False):
        super().__init__(device, timeit)
        self.npart_, self.channel_, self.ngroup_, self.nout_ = int(npart), int(channel), int(ngroup), int(nout)
        self.kernel_size_, self.constrain_ = int(kernel_size), int(constrain)
        self.pad_in_, self.pad_out_ = int(pad_in), int(pad_out)
        self.ctx_ = _lookup(addr)

    def _run(self, x, weight, bias, act, batch):
        """x, weight (nout, channel, k, k), bias and act (nout) -- the _batch entries: nset of each in front --:
        contiguous float32 on one GPU, all checked before the first call of the library"""
        _require_gpu(x, "EntropyConv2Op: x")
        pi, po = self.pad_in_, self.pad_out_
        num, channel, h, w = x.shape[0], x.shape[1], x.shape[2] - 2 * pi, x.shape[3] - 2 * pi
        if channel != self.channel_:
            raise PconvError("EntropyConv2Op: x has %d input channels, built for %d" % (channel, self.channel_))
        # one weight set (nout, channel, k, k) with (nout) bias and slopes, or -- the _batch entries -- nset of them
        _require_operand(weight, "EntropyConv2Op", "weight",
                         ((None,) if batch else ()) + (self.nout_, channel, self.kernel_size_, self.kernel_size_), torch.float32, x)
        nset = int(weight.shape[0]) if batch else 1
        sets = (nset,) if batch else ()
        _require_operand(bias, "EntropyConv2Op", "bias", sets + (self.nout_,), torch.float32, x)
        if act is not None:
            _require_operand(act, "EntropyConv2Op", "act", sets + (self.nout_,), torch.float32, x)
        if self._reshaped((num, channel, h, w)):
            self.pidx_ = 0
        order, start = self.ctx_.schedule(h, w, x)
        start_dev, longest = self.ctx_.schedule_device(h, w, x)
        top = self._out(0, (num, self.nout_, h + 2 * po, w + 2 * po), x)
        psum = self._step()
        rows = h * self.npart_
        nimg = num // self.npart_
        if psum < rows + w + self.ngroup_ - 2:
            lo, ln = self._window(psum, self.ngroup_, rows + w - 2, start)
            if ln > 0:
                if psum == 0:
                    top.zero_()
                first = max(psum - self.ngroup_ + 1, 0)
                end = psum + 1 if psum < rows + w - 2 else rows + w - 1
                call("pconv_entropy_conv", _ptr(x), _ptr(weight.detach()), _ptr(bias.detach()),
                     _ptr(act.detach()) if act is not None else None, _ptr(top), _ptr(order), _ptr(start_dev),
                     first, end - first, longest, nimg, max(nimg // nset, 1), channel, self.nout_, self.ngroup_,
                     self.kernel_size_, self.constrain_, self.npart_, h, w, pi, po, psum, None, None, None, None,
                     _stream(x.device))
        return [top]

    def forward(self, x, weight, bias):
        return self._run(x, weight, bias, None, False)

    def forward_act(self, x, weight, bias, act):
        return self._run(x, weight, bias, act, False)

    def forward_batch(self, x, weight, bias):
        return self._run(x, weight, bias, None, True)

    def forward_act_batch(self, x, weight, bias, act):
        return self._run(x, weight, bias, act, True)


class EntropyAddOp(_WavefrontOp):
    """PCONV.EntropyAddOp(npart, channel, ngroup, pad, addr, device, timeit)
    (main.cpp:132-136, entropy_add_cuda.cu:11-75); x += y in place."""

    def __init__(self, npart, channel, ngroup, pad, addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.npart_, self.channel_, self.ngroup_, self.pad_ = int(npart), int(channel), int(ngroup), int(pad)
        self.ctx_ = _lookup(addr)

    def forward(self, x, y):
        """x += y at the current wavefront: x and y contiguous float32 of one shape on one GPU"""
        _require_gpu(x, "EntropyAddOp: x")
        _require_operand(y, "EntropyAddOp", "y", x.shape, torch.float32, x)
        p = self.pad_
        num, channel, h, w = x.shape[0], x.shape[1], x.shape[2] - 2 * p, x.shape[3] - 2 * p
        if self._reshaped((num, channel, h, w)):
            self.pidx_ = 0
        order, start = self.ctx_.schedule(h, w, x)
        psum = self._step()
        rows = h * self.npart_
        if psum <= rows + w + self.ngroup_ - 2:
            lo, ln = self._window(psum, self.ngroup_, rows + w - 2, start)
            if ln > 0:
                call("pconv_entropy_add", _ptr(x), _ptr(y), _ptr(order), lo, ln, num // self.npart_,
                     self.channel_, self.ngroup_, self.npart_, h, w, p, psum, _stream(x.device))
        return [x]


class DExtract2Op(_WavefrontOp):
    """PCONV.DExtract2Op(npart, nchannel, label, addr, device, timeit)
    (main.cpp:68-73, d_extract_cuda_v2.cu:12-166)."""

    def __init__(self, npart, nchannel, label, addr, device=0, timeit=False):
        super().__init__(device, timeit)
        self.npart_, self.nchannel_, self.label_ = int(npart), int(nchannel), bool(label)
        self.ctx_ = _lookup(addr)
        self.top_num_ = torch.zeros(1, dtype=torch.int32)

    def _prepare(self, x):
        _require_gpu(x, "DExtract2Op")
        num, channel, h, w = x.shape
        if self._reshaped((num, channel, h, w)):
            self.pidx_ = 0
            self.top_num_ = torch.zeros(1, dtype=torch.int32)
        order, start = self.ctx_.schedule(h, w, x)
        cpn = channel // self.nchannel_
        top = self._out(0, (num // self.npart_, cpn, h * self.npart_, w), x)
        return num, channel, h, w, cpn, order, start, top

    def forward(self, x):
        num, channel, h, w, cpn, order, start, top = self._prepare(x)
        psum = self._step()
        rows = h * self.npart_
        mod = rows + w + self.nchannel_ - 2
        nimg = num // self.npart_
        run = False
        if self.label_:
            run = psum < mod
        elif psum == 0:
            top.zero_()
        elif psum <= mod:
            psum -= 1
            run = True
        if run:
            lo, ln = self._window(psum, self.nchannel_, rows + w - 2, start)
            self.top_num_[0] = ln * nimg
            if ln > 0:
                call("pconv_dextract2", _ptr(x), _ptr(top), _ptr(order), lo, ln, nimg, channel, cpn,
                     self.npart_, h, w, psum, _stream(x.device))
        return [top, self.top_num_]

    def forward_batch(self, x):
        num, channel, h, w, cpn, order, start, top = self._prepare(x)
        psum = self._step()
        rows = h * self.npart_
        nimg = num // self.npart_
        nout = nimg // 3
        if psum < rows + w + self.nchannel_ - 2:
            lo, ln = self._window(psum, self.nchannel_, rows + w - 2, start)
            self.top_num_[0] = nout * ln
            if ln > 0:
                call("pconv_dextract2_batch", _ptr(x), _ptr(top), _ptr(order), lo, ln, nimg, channel, cpn,
                     self.npart_, h, w, psum, nout, cpn * rows * w * nout, _stream(x.device))
        return [top, self.top_num_]


class EntropyGmmTableOp(_Op):
    """PCONV.EntropyGmmTableOp(nstep, bias, K, total, beta, device, timeit)
    (main.cpp:49-53, entropy_gmm_table_cuda.cu:11-185)."""

    def __init__(self, nstep, bias, num_gaussian, total_region, beta=1e-6, device=0, timeit=False):
        super().__init__(device, timeit)
        self.nstep_, self.bias_ = int(nstep), float(bias)
        self.num_gaussian_, self.total_region_, self.beta_ = int(num_gaussian), float(total_region), float(beta)
        if self.num_gaussian_ > 16:
            raise PconvError("EntropyGmmTableOp: at most 16 gaussians")

    def forward(self, weight, delta, mean, tnum):
        """weight, delta, mean: contiguous float32 of rows * num_gaussian elements each, read as [row][gaussian];
        tnum[0] <= rows: the rows to make"""
        for name, t in (("weight", weight), ("delta", delta), ("mean", mean)):
            _require_gpu(t, "EntropyGmmTableOp: " + name)
        rows = weight.numel() // self.num_gaussian_
        if weight.dim() == 4:
            rows = weight.shape[0] * weight.shape[2] * weight.shape[3]
        for name, t in (("delta", delta), ("mean", mean)):
            if t.numel() != weight.numel() or t.device != weight.device:
                raise PconvError("EntropyGmmTableOp: %s %s on %s does not fit weight %s on %s"
                                 % (name, tuple(t.shape), t.device, tuple(weight.shape), weight.device))
        tn = int(tnum[0])
        if not 0 <= tn <= rows or tn * self.num_gaussian_ > weight.numel():
            raise PconvError("EntropyGmmTableOp: tnum %d of the %d rows of weight %s" % (tn, rows, tuple(weight.shape)))
        table = self._out(0, (rows, self.nstep_ + 1), weight)
        call("pconv_gmm_table", _ptr(weight), _ptr(delta), _ptr(mean), _ptr(table), tn, self.num_gaussian_,
             self.nstep_, self.bias_, self.total_region_, self.beta_, 0, _stream(weight.device))
        return [table]

    def forward_batch(self, data, tnum):
        _require_gpu(data, "EntropyGmmTableOp: data")
        stride = data.numel() // 3
        rows = data.shape[0] * data.shape[2] * data.shape[3] // 3
        tn = int(tnum[0])
        if not 0 <= tn <= rows or tn * self.num_gaussian_ > stride:
            raise PconvError("EntropyGmmTableOp: tnum %d of the %d rows of data %s" % (tn, rows, tuple(data.shape)))
        table = self._out(0, (rows, self.nstep_ + 1), data)
        if tn > 0:
            base = data.data_ptr()
            call("pconv_gmm_table", base, base + 4 * stride, base + 8 * stride, _ptr(table), tn,
                 self.num_gaussian_, self.nstep_, self.bias_, self.total_region_, self.beta_, 1,
                 _stream(data.device))
        return [table]


# ---------------------------------------------------------------------------
# dense tile convolution (not a class of the reference's PCONV: it replaces the
# cuDNN calls behind nn.Conv2d in model_zoo_v2.py)
# ---------------------------------------------------------------------------
def conv_col_limit(ctx_op, h, base, extra, like):
    """(device int32[npart], npart): per latitude tile the first output column of a
    tile convolution that nothing downstream can read -- valid width at tile width
    `base` plus the `extra` halo columns the output still carries."""
    key = ("limit", int(base), int(extra), like.device)
    cache = ctx_op._cache
    if key not in cache:
        cache[key] = ctx_op._upload((ctx_op.widths_host(h, base) + int(extra)).astype(np.int32), like)
    return cache[key], ctx_op.npart_


CONV3X3_DEFAULT = "wino42"
WINO_ROW_SPLIT = os.environ.get("PCONV_WINO_SPLIT", "1") == "1"
WINO_FLAT_REMAINDER = os.environ.get("PCONV_WINO_FLAT", "1") == "1"   # 2-row launches on csrc/wino_flat.hip (0: the 4-row tile)

# the tile convolution kernels: C entry point, the two symbols of its weight packer, its shape predicate (the direct
# kernel takes every layer), the name its launches carry in conv_probe (direct: conv_kernel_name()), and the attribute
# of the layer that caches its packed weight (a layer may hold all three at once)
ConvKernel = collections.namedtuple("ConvKernel", "entry packed_size pack_weight supported probe_name slot")
CONV_KERNELS = {
    "direct": ConvKernel("pconv_conv2d", "pconv_conv_packed_size", "pconv_conv_pack_weight", None, None, "_pconv_packed"),
    # Winograd F(2x2, 3x3) (csrc/wino.hip), packed as U = G g Gt
    "wino": ConvKernel("pconv_conv3x3_wino", "pconv_wino_packed_size", "pconv_wino_pack_weight", "pconv_wino_supported",
                       "wino_conv3x3_kernel", "_pconv_packed_wino"),
    # ... its 2 x 128-pixel workgroup tile (csrc/wino_flat.hip): same layers, same weights
    "wino_flat": ConvKernel("pconv_conv3x3_wino_flat", "pconv_wino_packed_size", "pconv_wino_pack_weight",
                            "pconv_wino_supported", "wino_conv3x3_kernel", "_pconv_packed_wino"),
    # Winograd F(4x2, 3x3) (csrc/wino42.hip), packed as U = G6 g G4t
    "wino42": ConvKernel("pconv_conv3x3_wino42", "pconv_wino42_packed_size", "pconv_wino42_pack_weight",
                         "pconv_wino42_supported", "wino42_conv3x3_kernel", "_pconv_packed_wino42"),
}


def _cached_pack(owner, slot, weight, make, *args):
    """make(weight, *args): a pack of `weight`, kept in attribute `slot` of `owner` until the parameter is modified
    (in place -- an optimiser step bumps weight._version --, by load_state_dict, or -- for writes through `.data` --
    after backend.invalidate_derived()).  Every packed weight of the module goes through here."""
    from .PCONV_operator import backend
    key = (weight.data_ptr(), weight._version, weight.device, backend.param_epoch())
    cached = getattr(owner, slot, None)
    if cached is not None and cached[0] == key:
        return cached[1]
    packed = make(weight, *args)
    setattr(owner, slot, (key, packed))
    return packed


def _pack(weight, packed_size, size_dims, pack_weight, dims, stream):
    """a new buffer of packed_size(*size_dims) floats, filled by pack_weight(weight, buffer, *dims, stream)"""
    size = getattr(_native.hip_lib(), packed_size)(*size_dims)
    if size < 0:
        raise PconvError("%s: weight %s is too large to pack" % (pack_weight, tuple(weight.shape)))
    packed = torch.empty(int(size), dtype=torch.float32, device=weight.device)
    call(pack_weight, _ptr(weight.detach().contiguous()), _ptr(packed), *dims + (stream,))
    return packed


def _pack_forward(weight, kind, stream):
    kernel = CONV_KERNELS[kind]
    cout, cin, k = weight.shape[:3]
    if kind == "direct":   # 1x1 or 3x3; the size call could also report the padded extents
        return _pack(weight, kernel.packed_size, (cout, cin, k, None, None), kernel.pack_weight, (cout, cin, k), stream)
    return _pack(weight, kernel.packed_size, (cout, cin), kernel.pack_weight, (cout, cin), stream)   # Winograd: 3x3 by construction


def _packed_weight(owner, weight, kind, stream):
    """a conv weight in the layout of CONV_KERNELS[kind] (direct: the [k][cout] fp32 slab), cached on `owner`"""
    return _cached_pack(owner, CONV_KERNELS[kind].slot, weight, _pack_forward, kind, stream)


def packed_conv_weight(owner, weight, stream):
    """[k][cout] fp32 slab of a conv weight for pconv_conv2d / pconv_gdn (see _packed_weight).  weight: a 4-D float32
    GPU tensor of any strides (the pack reads a dense copy)"""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or weight.dtype != torch.float32 or not weight.is_cuda:
        raise PconvError("packed_conv_weight: weight must be a 4-D float32 GPU tensor, got %s"
                         % ("%s %s on %s" % (weight.dtype, tuple(weight.shape), weight.device)
                            if isinstance(weight, torch.Tensor) else type(weight).__name__))
    return _packed_weight(owner, weight, "direct", stream)


def conv3x3_mode():
    """which kernel takes the 3x3 stride-1 layers (PCONV_CONV3X3): 'wino42' = Winograd F(4x2, 3x3)
    (csrc/wino42.hip) where it takes the layer, F(2x2, 3x3) elsewhere; 'wino' = F(2x2, 3x3)
    (csrc/wino.hip); 'direct' = the fmaf-chain kernel the oracle restates bit for bit"""
    mode = os.environ.get("PCONV_CONV3X3", CONV3X3_DEFAULT)
    if mode[0] == "d":
        return "direct"
    return mode if mode in ("wino42", "wino42!") else "wino"   # "wino42!": every layer the kernel takes (tests / probes)


def conv_plan(cin, h, w, cout, k, stride, d2w=False, fused=False, aligned=True):
    """The launches of one tile_conv2d call, as pure arithmetic on the layer: ([(kernel, r0, rows)], fallback) with
    kernel a key of CONV_KERNELS and [r0, r0 + rows) its output rows.  fused: a sigmoid or a gate follows (direct kernel
    only); aligned: output and residual rows start on 8-byte boundaries.  fallback: Winograd was selected for the layer
    and nothing took it (counted in conv_fallbacks).
    3x3 stride-1 layers go to Winograd on the matrix cores unless PCONV_CONV3X3=direct asks for the fmaf-chain kernel
    (the bit-exact form the oracle restates); what a kernel takes is the library's pconv_*_supported alone."""
    ho = (h - k) // stride + 1
    direct = [("direct", 0, ho)]
    mode = conv3x3_mode()
    if k != 3 or stride != 1 or fused or mode == "direct":
        return direct, False
    if not aligned:
        return direct, True
    lib, d2 = _native.hip_lib(), 1 if d2w else 0
    wino42_takes = getattr(lib, CONV_KERNELS["wino42"].supported)
    wino_takes = getattr(lib, CONV_KERNELS["wino"].supported)     # (the flat build takes the same layers)
    # a launch of exactly two output rows (the split's remainder) takes the 2 x 128-pixel workgroup tile
    flat = "wino_flat" if WINO_FLAT_REMAINDER else "wino"
    # F(4x2, 3x3) works on 64-cout blocks: a 96-cout layer would run a third of them empty (and its 24 chunks are
    # head and tail of the unrolled loop, no steady state): measured 0.475 vs 0.374 ms, it stays with F(2x2, 3x3)
    # ... and on 8-row blocks.  Row counts that leave a remainder of up to four rows (66, 34, 18, 10: the "+1 halo"
    # layers of ResidualBlockV2) are SPLIT (r6): the whole 8-row blocks on F(4x2), the remainder as one 4-row block
    # row of F(2x2) in a second launch over row views of the same tensors -- before, 66 rows ran a ninth F(4x2) block
    # for two rows and 34 / 18 / 10 rows went to F(2x2) altogether.  PCONV_WINO_SPLIT=0: the round-5 rule (A/B).
    blocks = ho // 8 * 8
    if mode == "wino42" and cout % 64 == 0 and ho > 8 and 0 < ho % 8 <= 4 and WINO_ROW_SPLIT and \
            wino42_takes(cin, blocks + 2, w, cout, d2) == 1 and wino_takes(cin, ho - blocks + 2, w, cout, d2) == 1:
        return [("wino42", 0, blocks), (flat if ho - blocks == 2 else "wino", blocks, ho - blocks)], False
    # ... otherwise F(4x2) where the output rows fill its 8-row blocks to 8/9 at least
    if (mode == "wino42!" or (mode == "wino42" and cout % 64 == 0 and (ho + 7) // 8 * 8 * 8 <= 9 * ho)) and \
            wino42_takes(cin, h, w, cout, d2) == 1:
        return [("wino42", 0, ho)], False
    if wino_takes(cin, h, w, cout, d2) == 1:
        return [(flat if ho == 2 else "wino", 0, ho)], False
    return direct, True


def _aligned8(t):
    """rows of a (tile, channel, row, col) tensor start on 8-byte boundaries (float2 / float4 stores)"""
    return t.data_ptr() % 8 == 0 and t.stride(0) % 2 == 0 and t.stride(1) % 2 == 0 and t.stride(2) % 2 == 0


# 3x3 stride-1 calls that took the direct kernel although Winograd was selected, by (cin, h, w, cout, d2w)
# (on the codec path: the 3-channel input and 12-channel output layers only)
conv_fallbacks = {}

# when set to an object with a `records` list, every tile-conv / GDN launch is bracketed
# by events on its own stream: (kernel instantiation, class label, algorithmic flops,
# start, end).  Used by bench.py for the live roofline figures; None in normal operation.
conv_probe = None


class _ConvTimed(object):
    """conv_probe's bracket around one launch, like _HbmTimed.  describe() -> (kernel, label, flops, nbytes) is
    called only when a probe is set"""
    __slots__ = ("probe", "describe", "stream", "e0")

    def __init__(self, device, describe):
        self.probe = conv_probe
        if self.probe is not None:
            self.describe, self.stream = describe, torch.cuda.current_stream(device)

    def __enter__(self):
        if self.probe is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(self.stream)
        return self

    def __exit__(self, *exc):
        if self.probe is not None and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(self.stream)
            kernel, label, flops, nbytes = self.describe()
            self.probe.records.append((kernel, label, flops, self.e0, e1, nbytes))
        return False


def conv_kernel_name(cout, k, stride, squared=False, cin=0, pixels=0):
    """the kernel instantiation pconv_conv2d / pconv_gdn pick for a layer (csrc/conv.hip), as
    rocprofv3 prints it: conv_mfma_kernel<MT, NT, WM, WN, KS, S, KC, SQ>, or -- only when
    PCONV_CONV1X1=resident asks for it -- the weight-resident conv1x1_rb_kernel<WM, SQ> for 1x1
    stride-1 layers whose slab fits LDS (use_resident_1x1 in conv.hip)"""
    sq = "true" if squared else "false"
    mode = os.environ.get("PCONV_CONV1X1", "auto")[0]
    if k == 1 and stride == 1 and cin >= 32 and cin % 16 == 0 and cout > 32 and mode == "r" and \
            (cin + 15) // 16 * 16 * (192 if cout > 96 else 96) * 4 <= 150 * 1024:
        return "conv1x1_rb_kernel<%d, %s>" % (2 if cout > 96 else 1, sq)
    if k == 3 and stride == 1 and cout <= 16 and os.environ.get("PCONV_CONV_SMALL", "1") != "0":
        # (16-cout tiles on v_mfma_f32_16x16x4_f32: the 12-channel output layer)
        return "conv_small_kernel<3, 4>"
    mt, nt, wm, wn = (3, 1, 2, 4) if cout > 96 else ((3, 1, 1, 8) if cout > 32 else (1, 1, 1, 4))
    return "conv_mfma_kernel<%d, %d, %d, %d, %d, %d, %d, %s>" % (mt, nt, wm, wn, k, stride, 16 if k == 1 else 4, sq)


def _like_output(t, out, what):
    if t is None:
        return None
    if tuple(t.shape) != tuple(out.shape) or t.device != out.device or t.dtype != torch.float32:
        raise PconvError("%s: expected a float32 tensor shaped like the output %s, got %s"
                         % (what, tuple(out.shape), tuple(t.shape)))
    return t if t.stride(3) == 1 else t.contiguous()


# the size rules _host_query may ask: integer arithmetic on the host, no tensor, no device, no launch
HOST_QUERIES = ("pconv_erp_coded_size", "pconv_erp_resample_workspace_bytes", "pconv_erp_resample_backward_workspace_bytes",
                "pconv_ws_msssim_workspace_bytes")


def _host_query(fn, *args):
    """a size rule of the library (HOST_QUERIES only), asked where an operand's check needs its answer: before the
    wrapper's first call().  Everything else goes through call()"""
    if fn not in HOST_QUERIES:
        raise PconvError("%s is no host-only size rule: it goes through call()" % fn)
    return _native.check(getattr(_native.hip_lib(), fn)(*args), fn)


def _gpu_device(what, device):
    """`device` as a cuda device with its index; None: the current one"""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise PconvError("%s: expected a GPU device (this build has no CPU path), got %s" % (what, device))
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _require_frames(x, what):
    """the shape of a contiguous float32 (n, C, h, w) GPU tensor"""
    _require_gpu(x, what)
    if x.dim() != 4:
        raise PconvError("%s: float32 (n, C, h, w) expected" % what)
    return x.shape


def _require_sides(what, h, w):
    if not (2 <= h <= 1 << 20 and 2 <= w <= 1 << 20) or 4 * h * w >= 1 << 31:
        raise PconvError("%s: %dx%d: sides of 2 .. 2^20 and a plane below 2^31 bytes expected" % (what, w, h))


def _output(what, out, shape, dtype, device, where, name="out"):
    """`out` checked -- a contiguous tensor of this shape, dtype and device (`where` names the device in the refusal) --
    or, when it is None, a new one"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != device:
        raise PconvError("%s: %s must be contiguous %s (%s) on %s"
                         % (what, name, str(dtype).split(".")[1], ", ".join(str(int(s)) for s in shape), where))
    return out


def _require_view(what, vh, vw, ss):
    if not (2 <= vh <= 1 << 20 and 2 <= vw <= 1 << 20 and 1 <= ss <= 4):
        raise PconvError("%s: a view of %dx%d with ss = %d: sides of 2 .. 2^20 and ss of 1 .. 4 expected" % (what, vw, vh, ss))


def _require_map(what, map, gh, gw, device, where):
    if map.dtype != torch.int32 or tuple(map.shape) != (gh, gw, 2) or not map.is_contiguous() or map.device != device:
        raise PconvError("%s: the map must be contiguous int32 (%d, %d, 2) on %s" % (what, gh, gw, where))


def _require_rows(x, what):
    """GPU float32 4-D tensor whose columns are contiguous (dense, or the interior view
    of a padded buffer)"""
    if not x.is_cuda:
        raise PconvError("%s: expected a GPU tensor (this build has no CPU path), got %s" % (what, x.device))
    if x.dtype != torch.float32 or x.dim() != 4:
        raise PconvError("%s: only 4-D float32 is supported, got %s %s" % (what, x.dtype, tuple(x.shape)))
    return x if x.stride(3) == 1 else x.contiguous()


def _views(*tensors):
    """(tile, channel, row) element strides of each tensor for the C ABI; a missing tensor
    gets zeros (never dereferenced)"""
    flat = []
    for t in tensors:
        flat += [0, 0, 0] if t is None else [t.stride(0), t.stride(1), t.stride(2)]
    return (ctypes.c_longlong * len(flat))(*flat)


def _ring_output(shape, ring, like):
    """output tensor; with ring > 0 the interior view of a fresh padded buffer, tagged so
    that PseudoPadOp.forward_ring finds the buffer"""
    tn, c, h, w = shape
    if ring <= 0:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    buf = torch.empty((tn, c, h + 2 * ring, w + 2 * ring), dtype=torch.float32, device=like.device)
    out = buf[:, :, ring:-ring, ring:-ring]
    out._pconv_ring = (buf, ring)
    return out


def leaky_clip_(x):
    """ClipData.forward (model_zoo_v2.py:8-26) in place on a contiguous fp32 GPU tensor, one pass"""
    _require_gpu(x, "leaky_clip_")
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise PconvError("leaky_clip_: contiguous float32 tensor expected")
    with _HbmTimed("leaky_clip_kernel", "ClipData n%d" % x.numel(), 8.0 * x.numel(), x.device):
        call("pconv_leaky_clip", _ptr(x), x.numel(), _stream(x.device))
    return x


def frames_u8_to_f32(img, out=None):
    """device side of img2tensor (pseudo_codec.py:215-217): uint8 (n, H, W, 3) GPU tensor -> float32 (n, 3, H, W),
    float(u8) / 255 exactly as the reference's host division; the bus carried a quarter of the bytes"""
    if not img.is_cuda:
        raise PconvError("frames_u8_to_f32: img: expected a GPU tensor (this build has no CPU path), got %s" % img.device)
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3 or not img.is_contiguous():
        raise PconvError("frames_u8_to_f32: img: contiguous uint8 (n, H, W, 3) expected")
    n, h, w, _ = img.shape
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=img.device)
    elif tuple(out.shape) != (n, 3, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != img.device:
        raise PconvError("frames_u8_to_f32: out must be contiguous float32 (n, 3, H, W) on the image's device")
    with _HbmTimed("frames_u8_to_f32_kernel", "img2tensor n%d" % n, 5.0 * img.numel(), img.device):
        call("pconv_frames_u8_to_f32", _ptr(img), _ptr(out), n, h, w, _stream(img.device))
    return out


def frames_f32_to_u8(x, out=None):
    """device side of tensor2img (pseudo_codec.py:219-221): float32 (n, 3, H, W) -> uint8 (n, H, W, 3),
    (uint8)(int)(x * 255) as numpy's cast does it"""
    if not x.is_cuda:
        raise PconvError("frames_f32_to_u8: x: expected a GPU tensor (this build has no CPU path), got %s" % x.device)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise PconvError("frames_f32_to_u8: x: contiguous float32 (n, 3, H, W) expected")
    n, _, h, w = x.shape
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=x.device)
    elif tuple(out.shape) != (n, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device:
        raise PconvError("frames_f32_to_u8: out must be contiguous uint8 (n, H, W, 3) on the tensor's device")
    with _HbmTimed("frames_f32_to_u8_kernel", "tensor2img n%d" % n, 5.0 * x.numel(), x.device):
        call("pconv_frames_f32_to_u8", _ptr(x), _ptr(out), n, h, w, _stream(x.device))
    return out


def erp_coded_size(h, w):
    """(H, W, top) of an h x w ERP frame under the pole / seam padding rule (pconv_erp_coded_size)"""
    H, W, top = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _host_query("pconv_erp_coded_size", int(h), int(w), ctypes.byref(H), ctypes.byref(W), ctypes.byref(top))
    return H.value, W.value, top.value


def frames_u8_to_f32_erp(img, out=None):
    """frames_u8_to_f32 for any ERP size: uint8 (n, h, w, 3) GPU tensor (any width, any byte offset) -> float32
    (n, 3, H, W) padded by the pole / seam rule (erp_size.py), float(u8) / 255 as img2tensor"""
    if not img.is_cuda:
        raise PconvError("frames_u8_to_f32_erp: img: expected a GPU tensor (this build has no CPU path), got %s" % img.device)
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3 or not img.is_contiguous():
        raise PconvError("frames_u8_to_f32_erp: img: contiguous uint8 (n, h, w, 3) expected")
    n, h, w, _ = img.shape
    H, W, _top = erp_coded_size(h, w)
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=img.device)
    elif tuple(out.shape) != (n, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != img.device:
        raise PconvError("frames_u8_to_f32_erp: out must be contiguous float32 (n, 3, %d, %d) on the image's device" % (H, W))
    with _HbmTimed("frames_u8_to_f32_erp_pad_kernel", "img2tensor+pad n%d" % n, img.numel() + 4.0 * out.numel(), img.device):
        call("pconv_frames_u8_to_f32_erp", _ptr(img), _ptr(out), n, h, w, _stream(img.device))
    return out


def erp_pad_f32(x, out=None):
    """float32 (n, 3, h, w) GPU tensor -> (n, 3, H, W) padded by the pole / seam rule (erp_size.py)"""
    _require_gpu(x, "erp_pad_f32: x")
    if x.dim() != 4 or x.shape[1] != 3:
        raise PconvError("erp_pad_f32: x: float32 (n, 3, h, w) expected")
    n, _, h, w = x.shape
    H, W, _top = erp_coded_size(h, w)
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise PconvError("erp_pad_f32: out must be contiguous float32 (n, 3, %d, %d) on the input's device" % (H, W))
    with _HbmTimed("erp_pad_f32_kernel", "ErpPad n%d" % n, 4.0 * (x.numel() + out.numel()), x.device):
        call("pconv_erp_pad_f32", _ptr(x), _ptr(out), n, h, w, _stream(x.device))
    return out


def frames_f32_to_u8_crop(x, height, width, out=None):
    """frames_f32_to_u8 and the decoder's crop in one pass: float32 (n, 3, H, W) coded frames -> uint8
    (n, height, width, 3) of rows top..top+height-1, columns 0..width-1 (any width, any byte offset of out)"""
    _require_gpu(x, "frames_f32_to_u8_crop: x")
    H, W, _top = erp_coded_size(height, width)
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, H, W):
        raise PconvError("frames_f32_to_u8_crop: x: float32 (n, 3, %d, %d) expected for %dx%d, got %s"
                         % (H, W, width, height, tuple(x.shape)))
    n = x.shape[0]
    if out is None:
        out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=x.device)
    elif tuple(out.shape) != (n, height, width, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device:
        raise PconvError("frames_f32_to_u8_crop: out must be contiguous uint8 (n, %d, %d, 3) on the tensor's device"
                         % (height, width))
    with _HbmTimed("frames_f32_to_u8_crop_kernel", "tensor2img+crop n%d" % n, 5.0 * out.numel(), x.device):
        call("pconv_frames_f32_to_u8_crop", _ptr(x), _ptr(out), n, height, width, _stream(x.device))
    return out


# name -> (PCONV_YUV_* constant, dtype, bit depth) / PCONV_YUV_BT* / PCONV_YUV_LIMITED, _FULL (include/pconv_hip.h)
YUV_FORMATS = {"yuv420p": (0, torch.uint8, 8), "nv12": (1, torch.uint8, 8), "yuv420p10le": (2, torch.uint16, 10)}
YUV_MATRICES = {"bt709": 0, "bt601": 1}
YUV_RANGES = {"limited": 0, "full": 1}


def _yuv_args(what, h, w, fmt, matrix, range):
    if fmt not in YUV_FORMATS or matrix not in YUV_MATRICES or range not in YUV_RANGES:
        raise PconvError("%s: unknown pixel format, matrix or range: %r, %r, %r (formats %s; matrices %s; ranges %s)"
                         % (what, fmt, matrix, range, sorted(YUV_FORMATS), sorted(YUV_MATRICES), sorted(YUV_RANGES)))
    h, w = int(h), int(w)
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise PconvError("%s: a 4:2:0 frame needs even sides of at least 2, got %dx%d" % (what, w, h))
    code, dtype, depth = YUV_FORMATS[fmt]
    return h, w, code, dtype, (depth + 7) // 8, h * w * 3 // 2


def frames_yuv420_to_f32(buf, h, w, fmt, matrix="bt709", range="limited", out=None):
    """YUV 4:2:0 frames -> RGB at the coded size (yuv.py, pconv_frames_yuv420_to_f32): buf a GPU tensor (n, h*w*3/2)
    of the format's dtype (any offset its element size allows) -> float32 (n, 3, H, W), the colour conversion fused
    with the pole / seam pad"""
    if not buf.is_cuda:
        raise PconvError("frames_yuv420_to_f32: buf: expected a GPU tensor (this build has no CPU path), got %s" % buf.device)
    h, w, code, dtype, size, elems = _yuv_args("frames_yuv420_to_f32", h, w, fmt, matrix, range)
    if buf.dtype != dtype or buf.dim() != 2 or buf.shape[1] != elems or not buf.is_contiguous():
        raise PconvError("frames_yuv420_to_f32: buf: contiguous %s (n, %d) expected for %s frames of %dx%d, got %s %s"
                         % (dtype, elems, fmt, w, h, buf.dtype, tuple(buf.shape)))
    n = buf.shape[0]
    H, W, _top = erp_coded_size(h, w)
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=buf.device)
    elif tuple(out.shape) != (n, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != buf.device:
        raise PconvError("frames_yuv420_to_f32: out must be contiguous float32 (n, 3, %d, %d) on the frames' device" % (H, W))
    with _HbmTimed("frames_yuv420_to_f32_kernel", "yuv2tensor+pad %s n%d" % (fmt, n), size * buf.numel() + 4.0 * out.numel(),
                   buf.device):
        call("pconv_frames_yuv420_to_f32", _ptr(buf), _ptr(out), n, h, w, code, YUV_MATRICES[matrix], YUV_RANGES[range],
             _stream(buf.device))
    return out


def frames_f32_to_yuv420(x, h, w, fmt, matrix="bt709", range="limited", out=None):
    """RGB at the coded size -> YUV 4:2:0 frames (yuv.py, pconv_frames_f32_to_yuv420): float32 (n, 3, H, W) coded
    frames -> (n, h*w*3/2) of the format's dtype, rows top..top+h-1 and columns 0..w-1 converted, the chroma filtered
    down with the seam wrapped (any offset of out its element size allows)"""
    _require_gpu(x, "frames_f32_to_yuv420: x")
    h, w, code, dtype, size, elems = _yuv_args("frames_f32_to_yuv420", h, w, fmt, matrix, range)
    H, W, _top = erp_coded_size(h, w)
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, H, W):
        raise PconvError("frames_f32_to_yuv420: x: float32 (n, 3, %d, %d) expected for %dx%d, got %s"
                         % (H, W, w, h, tuple(x.shape)))
    n = x.shape[0]
    if out is None:
        out = torch.empty((n, elems), dtype=dtype, device=x.device)
    elif tuple(out.shape) != (n, elems) or out.dtype != dtype or not out.is_contiguous() or out.device != x.device:
        raise PconvError("frames_f32_to_yuv420: out must be contiguous %s (n, %d) on the tensor's device" % (dtype, elems))
    with _HbmTimed("frames_f32_to_yuv420_kernel", "tensor2yuv+crop %s n%d" % (fmt, n), 12.0 * n * h * w + size * out.numel(),
                   x.device):
        call("pconv_frames_f32_to_yuv420", _ptr(x), _ptr(out), n, h, w, code, YUV_MATRICES[matrix], YUV_RANGES[range],
             _stream(x.device))
    return out


_resample_tables = {}   # (device, h, w, h2, w2) -> (first_x, wx, first_y, wy) on the device


def erp_resample_f32(x, h2, w2, clamp=False, out=None, workspace=None):
    """float32 (n, C, h, w) GPU tensor -> (n, C, h2, w2): the sphere-aware Lanczos-3 resize (erp_resample.py,
    pconv_erp_resample_f32).  The tap tables live on the device, cached per (h, w, h2, w2); workspace: a uint8 GPU
    tensor of at least pconv_erp_resample_workspace_bytes bytes (allocated when None)"""
    n, c, h, w = _require_frames(x, "erp_resample_f32: x")
    h2, w2 = int(h2), int(w2)
    nbytes = _host_query("pconv_erp_resample_workspace_bytes", n, c, h, w, h2, w2)
    out = _output("erp_resample_f32", out, (n, c, h2, w2), torch.float32, x.device, "the input's device")
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.numel() < nbytes or not workspace.is_contiguous()
                                  or workspace.device != x.device):
        raise PconvError("erp_resample_f32: workspace must be a contiguous uint8 tensor of %d bytes on the input's device" % nbytes)
    key = (x.device, h, w, h2, w2)
    if key not in _resample_tables:
        from .erp_resample import taps
        fx, wx = taps(w, w2)
        fy, wy = taps(h, h2)
        _resample_tables[key] = tuple(t.to(x.device) for t in (fx, wx, fy, wy))
    fx, wx, fy, wy = _resample_tables[key]
    if workspace is None:
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    # input read + intermediate written and read + output written
    counted = 4.0 * (x.numel() + 2.0 * n * c * h * w2 + out.numel())
    with _HbmTimed("erp_resample_kernels", "ErpResample %dx%d->%dx%d n%d" % (w, h, w2, h2, n), counted, x.device):
        call("pconv_erp_resample_f32", _ptr(x), _ptr(out), _ptr(workspace), _ptr(fx), _ptr(wx), wx.shape[1], _ptr(fy),
             _ptr(wy), wy.shape[1], n, c, h, w, h2, w2, 1 if clamp else 0, _stream(x.device))
    return out


_resample_reverse = {}   # (device, h, w, h2, w2) -> (wx, start_x, entry_x, wy, start_y, entry_y, crossed_y) on the device


def erp_resample_backward_f32(g, h, w, gin=None, workspace=None):
    """the gradient of erp_resample_f32 (clamp=False) with respect to its input, in the order of include/pconv_hip.h
    (pconv_erp_resample_backward_f32): float32 (n, C, h2, w2) GPU gradient of the resize of h x w frames -> (n, C, h, w).
    The weight tables and the transposed lists (erp_resample.reverse_taps) live on the device, cached per (h, w, h2, w2);
    gin: a contiguous float32 (n, C, h, w) tensor to write (allocated when None; every element is written); workspace:
    a uint8 GPU tensor of at least pconv_erp_resample_backward_workspace_bytes bytes (allocated when None)"""
    _require_gpu(g, "erp_resample_backward_f32: g")
    if g.dim() != 4 or g.dtype != torch.float32 or not g.is_contiguous():
        raise PconvError("erp_resample_backward_f32: g: a contiguous float32 (n, C, h2, w2) gradient expected, got %s %s"
                         % (g.dtype, tuple(g.shape)))
    n, c, h2, w2 = g.shape
    h, w = int(h), int(w)
    nbytes = _host_query("pconv_erp_resample_backward_workspace_bytes", n, c, h, w, h2, w2)
    gin = _output("erp_resample_backward_f32", gin, (n, c, h, w), torch.float32, g.device, "the gradient's device", "gin")
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.numel() < nbytes or not workspace.is_contiguous()
                                  or workspace.device != g.device):
        raise PconvError("erp_resample_backward_f32: workspace must be a contiguous uint8 tensor of %d bytes on the gradient's "
                         "device" % nbytes)
    key = (g.device, h, w, h2, w2)
    if key not in _resample_reverse:
        from .erp_resample import reverse_taps, taps
        tables = (taps(w, w2)[1],) + reverse_taps(w, w2, 0)[:2] + (taps(h, h2)[1],) + reverse_taps(h, h2, 1)
        _resample_reverse[key] = tuple(t.to(g.device) for t in tables)
    wx, start_x, entry_x, wy, start_y, entry_y, crossed_y = _resample_reverse[key]
    if workspace is None:
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=g.device)
    # gradient read + intermediate written and read + input gradient written
    counted = 4.0 * (g.numel() + 2.0 * n * c * h * w2 + gin.numel())
    with _HbmTimed("erp_resample_backward_kernels", "ErpResampleBackward %dx%d<-%dx%d n%d" % (w, h, w2, h2, n), counted,
                   g.device):
        call("pconv_erp_resample_backward_f32", _ptr(g), _ptr(gin), _ptr(workspace), _ptr(wx), wx.shape[1], _ptr(start_x),
             _ptr(entry_x), _ptr(wy), wy.shape[1], _ptr(start_y), _ptr(entry_y), _ptr(crossed_y), n, c, h, w, h2, w2,
             _stream(g.device))
    return gin


_rotate_phases = {}   # device -> the phase table of erp_rotate.phases() on the device


def erp_rotation_map(h, w, rotation, inverse=False, device=None, out=None):
    """int32 (h, w, 2) GPU tensor: where on the source each pixel of the rotated h x w frame lies, in 1/256 pixel
    (erp_rotate.py, pconv_erp_rotation_map).  rotation: (yaw, pitch, roll) in units of 2^-16 degree; inverse: the map
    of the way back.  One launch; the trigonometry runs in fp64 on the device"""
    h, w = int(h), int(w)
    try:
        yaw, pitch, roll = (int(v) for v in rotation)
    except (TypeError, ValueError):
        raise PconvError("erp_rotation_map: a rotation is three integers in units of 2^-16 degree, got %r" % (rotation,))
    device = _gpu_device("erp_rotation_map", device)
    _require_sides("erp_rotation_map", h, w)
    out = _output("erp_rotation_map", out, (h, w, 2), torch.int32, device, device)
    with torch.cuda.device(device), _HbmTimed("erp_rotation_map_kernel", "ErpRotationMap %dx%d" % (w, h), 8.0 * h * w, device):
        call("pconv_erp_rotation_map", _ptr(out), h, w, yaw, pitch, roll, 1 if inverse else 0, _stream(device))
    return out


def erp_remap_f32(x, map, clamp=False, out=None):
    """float32 (n, C, h, w) GPU tensor -> (n, C, h, w) read through `map` (int32 (h, w, 2) on the same device, from
    erp_rotation_map) with the 6 x 6 Lanczos-3 footprint of erp_rotate.py (pconv_erp_remap_f32).  The phase table lives
    on the device, cached per device; out must not be x"""
    n, c, h, w = _require_frames(x, "erp_remap_f32: x")
    _require_map("erp_remap_f32", map, h, w, x.device, "the input's device")
    table = _phase_table(x.device)
    out = _output("erp_remap_f32", out, (n, c, h, w), torch.float32, x.device, "the input's device")
    # input read + output written + the map read once per frame
    counted = 4.0 * (x.numel() + out.numel()) + 8.0 * n * h * w
    with _HbmTimed("erp_remap_f32_kernel", "ErpRemap %dx%d n%d" % (w, h, n), counted, x.device):
        call("pconv_erp_remap_f32", _ptr(x), _ptr(out), _ptr(map), _ptr(table), n, c, h, w, 1 if clamp else 0,
             _stream(x.device))
    return out


def _phase_table(device):
    if device not in _rotate_phases:
        from .erp_rotate import phases
        _rotate_phases[device] = phases().to(device)
    return _rotate_phases[device]


SPHERE_POINTS_MODES = {"lanczos": 0, "nearest": 1}  # PCONV_SPHERE_POINTS_LANCZOS, PCONV_SPHERE_POINTS_NEAREST
SPHERE_POINTS_MAX = (1 << 28) - 1


def _sphere_points_mode(what, interp):
    if interp not in SPHERE_POINTS_MODES:
        raise PconvError("%s: interp must be one of %s, got %r" % (what, sorted(SPHERE_POINTS_MODES), interp))
    return SPHERE_POINTS_MODES[interp]


def _sphere_points_records_of(what, rec, x, name="records"):
    """the record count of `rec`, contiguous int32 (P, 2) on x's device"""
    if rec.dtype != torch.int32 or rec.dim() != 2 or rec.shape[1] != 2 or not rec.is_contiguous() or rec.device != x.device \
            or not 1 <= rec.shape[0] <= SPHERE_POINTS_MAX:
        raise PconvError("%s: the %s must be contiguous int32 (P, 2), 1 <= P < 2^28, on the input's device, got %s %s "
                         "on %s" % (what, name if name == "records" else "records " + name, rec.dtype, tuple(rec.shape), rec.device))
    return rec.shape[0]


def sphere_points_records(points, h, w, out=None):
    """int32 (P, 2) GPU tensor: the 1/256-pixel records of the points (float64 (P, 2) of (longitude, latitude) on the
    device) for a picture of h x w (sphere_points.py, pconv_sphere_points_records).  One launch, fp64, no trigonometry"""
    h, w = int(h), int(w)
    if not points.is_cuda or points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 2 \
            or not points.is_contiguous() or not 1 <= points.shape[0] <= SPHERE_POINTS_MAX:
        raise PconvError("sphere_points_records: contiguous float64 (P, 2) points, 1 <= P < 2^28, on a GPU expected, got %s "
                         "%s on %s" % (points.dtype, tuple(points.shape), points.device))
    _require_sides("sphere_points_records", h, w)
    count = points.shape[0]
    out = _output("sphere_points_records", out, (count, 2), torch.int32, points.device, "the points' device")
    with _HbmTimed("sphere_points_records_kernel", "SpherePointsRecords %dx%d P%d" % (w, h, count), 24.0 * count, points.device):
        call("pconv_sphere_points_records", _ptr(points), _ptr(out), count, h, w, _stream(points.device))
    return out


def sphere_points_sample_f32(x, records, interp="lanczos", out=None):
    """float32 (n, C, h, w) GPU tensor -> (n, C, P): every plane read at the records (int32 (P, 2) on the same device,
    from sphere_points_records for this h x w) with the 6 x 6 Lanczos-3 footprint of erp_rotate.py or, interp="nearest",
    the nearest pixel (pconv_sphere_points_sample_f32)"""
    n, c, h, w = _require_frames(x, "sphere_points_sample_f32: x")
    mode = _sphere_points_mode("sphere_points_sample_f32", interp)
    count = _sphere_points_records_of("sphere_points_sample_f32", records, x)
    out = _output("sphere_points_sample_f32", out, (n, c, count), torch.float32, x.device, "the input's device")
    # the algorithmic bytes of the gather: one pixel (nearest) or 36 (lanczos) per point and plane, the output, the records
    counted = 4.0 * n * c * count * ((36 if mode == 0 else 1) + 1) + 8.0 * n * count
    with _HbmTimed("sphere_points_sample_kernel", "SpherePointsSample %dx%d n%d P%d" % (w, h, n, count), counted, x.device):
        call("pconv_sphere_points_sample_f32", _ptr(x), _ptr(out), _ptr(records), _ptr(_phase_table(x.device)), n, c, h, w,
             count, mode, _stream(x.device))
    return out


def sphere_points_mse_device(x, rec_x, y, rec_y, interp="lanczos"):
    """float64 (n, C) on the inputs' device: the mean over the P points of (a - b)^2, a the sample of x (n, C, h1, w1) at
    rec_x and b the sample of y (n, C, h2, w2) at rec_y, the difference and its square in fp32, the sum in fp64 in the
    order of include/pconv_hip.h (pconv_sphere_points_mse_f32).  Two launches, no sample is written; nothing waits"""
    _require_gpu(x, "sphere_points_mse: x")
    _require_gpu(y, "sphere_points_mse: y")
    if x.dim() != 4 or y.dim() != 4 or x.shape[:2] != y.shape[:2] or x.device != y.device:
        raise PconvError("sphere_points_mse: x and y: two float32 (n, C, h, w) batches of equal n and C on one device expected, got "
                         "%s on %s and %s on %s" % (tuple(x.shape), x.device, tuple(y.shape), y.device))
    mode = _sphere_points_mode("sphere_points_mse", interp)
    count = _sphere_points_records_of("sphere_points_mse", rec_x, x, "rec_x")
    if _sphere_points_records_of("sphere_points_mse", rec_y, y, "rec_y") != count:
        raise PconvError("sphere_points_mse: the two record lists rec_x and rec_y differ in length: %d and %d" % (count, rec_y.shape[0]))
    n, c = x.shape[:2]
    nbytes = call("pconv_sphere_points_mse_workspace_bytes", n, c, count)
    workspace = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    out = torch.empty((n, c), dtype=torch.float64, device=x.device)
    counted = 4.0 * n * c * count * 2 * (36 if mode == 0 else 1) + 16.0 * n * c * count
    with _HbmTimed("sphere_points_mse_kernel", "SpherePointsMse n%d P%d" % (n, count), counted, x.device):
        call("pconv_sphere_points_mse_f32", _ptr(x), x.shape[2], x.shape[3], _ptr(rec_x), _ptr(y), y.shape[2], y.shape[3],
             _ptr(rec_y), _ptr(_phase_table(x.device)), n, c, count, mode, _ptr(workspace), _ptr(out), _stream(x.device))
    return out


def sphere_points_mse(x, rec_x, y, rec_y, interp="lanczos"):
    """sphere_points_mse_device with the float64 (n, C) result copied to the host"""
    return sphere_points_mse_device(x, rec_x, y, rec_y, interp).cpu()


def viewport_map(h, w, gh, gw, view, device=None, out=None):
    """int32 (gh, gw, 2) GPU tensor: where on the h x w source each sample of the gh x gw grid of a rectilinear view
    lies, in 1/256 pixel (viewport.py, pconv_viewport_map).  view: (yaw, pitch, roll, hfov, vfov) in units of 2^-16
    degree.  One launch; the trigonometry runs in fp64 on the device"""
    h, w, gh, gw = int(h), int(w), int(gh), int(gw)
    try:
        yaw, pitch, roll, hfov, vfov = (int(v) for v in view)
    except (TypeError, ValueError):
        raise PconvError("viewport_map: a view is five integers in units of 2^-16 degree, got %r" % (view,))
    device = _gpu_device("viewport_map", device)
    if not (2 <= gh <= 1 << 22 and 2 <= gw <= 1 << 22) or 8 * gh * gw >= 1 << 31:
        raise PconvError("viewport_map: a grid of %dx%d: sides of 2 .. 2^22 and a map below 2^31 bytes expected" % (gw, gh))
    out = _output("viewport_map", out, (gh, gw, 2), torch.int32, device, device)
    with torch.cuda.device(device), _HbmTimed("viewport_map_kernel", "ViewportMap %dx%d" % (gw, gh), 8.0 * gh * gw, device):
        call("pconv_viewport_map", _ptr(out), h, w, gh, gw, yaw, pitch, roll, hfov, vfov, _stream(device))
    return out


def viewport_render_f32(x, map, vh, vw, ss, clamp=False, out=None, slot=0):
    """float32 (n, C, h, w) GPU tensor -> one rectilinear view of vh x vw pixels, read through `map` (int32 (vh * ss,
    vw * ss, 2) on the same device, from viewport_map) and averaged over ss x ss samples per pixel (viewport.py,
    pconv_viewport_render_f32).  out: a contiguous float32 (n, V, C, vh, vw) tensor whose view `slot` is written, the
    others left alone; None: a new (n, 1, C, vh, vw)"""
    n, c, h, w = _require_frames(x, "viewport_render_f32: x")
    vh, vw, ss, slot = int(vh), int(vw), int(ss), int(slot)
    _require_view("viewport_render_f32", vh, vw, ss)
    _require_map("viewport_render_f32", map, vh * ss, vw * ss, x.device, "the input's device")
    table = _phase_table(x.device)
    if out is None:
        out = torch.empty((n, 1, c, vh, vw), dtype=torch.float32, device=x.device)
    elif out.dim() != 5 or out.shape[0] != n or tuple(out.shape[2:]) != (c, vh, vw) or out.dtype != torch.float32 \
            or not out.is_contiguous() or out.device != x.device:
        raise PconvError("viewport_render_f32: out must be contiguous float32 (%d, V, %d, %d, %d) on the input's device"
                         % (n, c, vh, vw))
    views = out.shape[1]
    if not 0 <= slot < views:
        raise PconvError("viewport_render_f32: slot %d of %d views" % (slot, views))
    frame = c * vh * vw
    # every sample's 36 source values (what the caches make of their overlap is not counted away) + its record per
    # plane + the output written
    counted = 4.0 * 36 * n * c * vh * vw * ss * ss + 8.0 * n * c * vh * vw * ss * ss + 4.0 * n * frame
    with _HbmTimed("viewport_render_f32_kernel", "ViewportRender %dx%d->%dx%d ss%d n%d" % (w, h, vw, vh, ss, n), counted,
                   x.device):
        call("pconv_viewport_render_f32", _ptr(x), out.data_ptr() + 4 * slot * frame, _ptr(map), _ptr(table), n, c, h, w,
             vh, vw, ss, views * frame, 1 if clamp else 0, _stream(x.device))
    return out


def remap_backward_f32(gout, map, lists, h, w, vh, vw, ss, gin=None, slot=0, accumulate=False):
    """the gradient of viewport_render_f32 (and, with ss = 1 and vh x vw = h x w, of erp_remap_f32) with respect to its
    input, in the order of include/pconv_hip.h (pconv_remap_backward_f32): float32 (n, C, h, w).  gout: the contiguous
    float32 gradient of the views, (n, V, C, vh, vw), of which view `slot` is read in place, or (n, C, vh, vw); map: the
    int32 (vh * ss, vw * ss, 2) map the forward read; lists: (start, entry) of viewport.reverse_lists on the same
    device.  gin: the contiguous tensor to write (None: a new one); accumulate=True adds to what gin holds, leaving
    the pixels no sample reads untouched"""
    _require_gpu(gout, "remap_backward_f32: gout")
    h, w, vh, vw, ss, slot = int(h), int(w), int(vh), int(vw), int(ss), int(slot)
    if gout.dim() == 4:
        gout = gout.unsqueeze(1)
    if gout.dim() != 5 or tuple(gout.shape[3:]) != (vh, vw) or not gout.is_contiguous():
        raise PconvError("remap_backward_f32: gout: a contiguous float32 (n, V, C, %d, %d) or (n, C, %d, %d) gradient expected, got %s"
                         % (vh, vw, vh, vw, tuple(gout.shape)))
    n, views, c = gout.shape[:3]
    if not 0 <= slot < views:
        raise PconvError("remap_backward_f32: slot %d of %d views" % (slot, views))
    _require_view("remap_backward_f32", vh, vw, ss)
    _require_map("remap_backward_f32", map, vh * ss, vw * ss, gout.device, "the gradient's device")
    entries = 36 * vh * ss * vw * ss
    try:
        start, entry = lists
        good = all(t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == gout.device
                   for t in (start, entry)) and start.numel() == h * w + 1 and entry.numel() == entries
    except (TypeError, ValueError, AttributeError):
        good = False
    if not good:
        raise PconvError("remap_backward_f32: lists must be (start, entry) of viewport.reverse_lists for this map and a %dx%d "
                         "source: contiguous int32 of %d and %d elements on the gradient's device" % (w, h, h * w + 1, entries))
    if gin is None and accumulate:
        raise PconvError("remap_backward_f32: accumulate needs the gin to add to")
    gin = _output("remap_backward_f32", gin, (n, c, h, w), torch.float32, gout.device, "the gradient's device", "gin")
    table = _phase_table(gout.device)
    frame = c * vh * vw
    # per plane: every entry (4 bytes), its record and its gradient value (what the caches make of their reuse is not
    # counted away), the starts, and gin written (and read, when accumulating)
    counted = n * ((c + 3) // 4) * (4.0 * entries + 8.0 * entries + 4.0 * (h * w + 1)) + 4.0 * n * c * entries \
        + 4.0 * gin.numel() * (2 if accumulate else 1)
    with _HbmTimed("remap_backward_f32_kernel", "RemapBackward %dx%d<-%dx%d ss%d n%d" % (w, h, vw, vh, ss, n), counted,
                   gout.device):
        call("pconv_remap_backward_f32", gout.data_ptr() + 4 * slot * frame, _ptr(gin), _ptr(map), _ptr(table), _ptr(start),
             _ptr(entry), n, c, h, w, vh, vw, ss, views * frame, 1 if accumulate else 0, _stream(gout.device))
    return gin


CUBE_KINDS = {"cmp": 1, "eac": 2}   # PCONV_CUBE_CMP, PCONV_CUBE_EAC
CUBE_PAD = 3                        # PCONV_CUBE_PAD
CUBE_MAX_FACE = 9453                # PCONV_CUBE_MAX_FACE


def _cube_args(what, kind, a, ss):
    if kind not in CUBE_KINDS:
        raise PconvError("%s: kind must be one of %s, got %r" % (what, sorted(CUBE_KINDS), kind))
    a, ss = int(a), int(ss)
    if not (2 <= a <= CUBE_MAX_FACE and 1 <= ss <= 4):
        raise PconvError("%s: a face size of %d with ss = %d: a of 2 .. %d and ss of 1 .. 4 expected" % (what, a, ss, CUBE_MAX_FACE))
    return CUBE_KINDS[kind], a, ss


def cube_from_erp_map(kind, a, ss, h, w, device=None, out=None):
    """int32 (6 a ss, a ss, 2) GPU tensor: where on the h x w ERP source each sample of the face stack of a "cmp" / "eac"
    cube of face size a lies, in 1/256 pixel (cube.py, pconv_cube_from_erp_map).  One launch; the trigonometry runs in
    fp64 on the device"""
    code, a, ss = _cube_args("cube_from_erp_map", kind, a, ss)
    h, w = int(h), int(w)
    device = _gpu_device("cube_from_erp_map", device)
    _require_sides("cube_from_erp_map", h, w)
    gs = a * ss
    if 8 * 6 * gs * gs >= 1 << 31:
        raise PconvError("cube_from_erp_map: a map of %dx%d records is 2^31 bytes or more" % (gs, 6 * gs))
    out = _output("cube_from_erp_map", out, (6 * gs, gs, 2), torch.int32, device, device)
    with torch.cuda.device(device), _HbmTimed("cube_from_erp_map_kernel", "CubeFromErpMap a%d ss%d" % (a, ss), 48.0 * gs * gs,
                                              device):
        call("pconv_cube_from_erp_map", _ptr(out), code, a, ss, h, w, _stream(device))
    return out


def cube_to_erp_map(kind, a, h, w, ss, device=None, out=None):
    """int32 (h ss, w ss, 2) GPU tensor: where on the padded face stack (one plane of 6 (a + 6) x (a + 6)) each sample of
    an h x w ERP frame lies, in 1/256 pixel (cube.py, pconv_cube_to_erp_map).  One launch, fp64 on the device"""
    code, a, ss = _cube_args("cube_to_erp_map", kind, a, ss)
    h, w = int(h), int(w)
    device = _gpu_device("cube_to_erp_map", device)
    _require_sides("cube_to_erp_map", h, w)
    if 8 * h * ss * w * ss >= 1 << 31:
        raise PconvError("cube_to_erp_map: a map of %dx%d records is 2^31 bytes or more" % (w * ss, h * ss))
    out = _output("cube_to_erp_map", out, (h * ss, w * ss, 2), torch.int32, device, device)
    with torch.cuda.device(device), _HbmTimed("cube_to_erp_map_kernel", "CubeToErpMap %dx%d ss%d" % (w, h, ss),
                                              8.0 * h * w * ss * ss, device):
        call("pconv_cube_to_erp_map", _ptr(out), code, a, h, w, ss, _stream(device))
    return out


def cube_pad_f32(x, table, out=None):
    """float32 (n, C, 6 a, a) GPU face stack -> (n, C, 6 A, A), A = a + 6: every face continued by 3 pixels across its
    edges, the ring read bilinearly from the neighbouring faces through `table` (int32 (6 (A^2 - a^2), 3) on the same
    device, from cube.pad_table) (cube.py, pconv_cube_pad_f32).  One launch; out must not be x"""
    n, c, h6, a = _require_frames(x, "cube_pad_f32: x")
    if h6 != 6 * a or not 2 <= a <= CUBE_MAX_FACE:
        raise PconvError("cube_pad_f32: a face stack (n, C, 6 a, a), a of 2 .. %d, expected, got %s" % (CUBE_MAX_FACE, tuple(x.shape)))
    A = a + 2 * CUBE_PAD
    ring = 6 * (A * A - a * a)
    if table.dtype != torch.int32 or tuple(table.shape) != (ring, 3) or not table.is_contiguous() or table.device != x.device:
        raise PconvError("cube_pad_f32: the table must be contiguous int32 (%d, 3) on the input's device" % ring)
    out = _output("cube_pad_f32", out, (n, c, 6 * A, A), torch.float32, x.device, "the input's device")
    # the faces read + the padded stack written + the ring's records and four reads per ring pixel
    counted = 4.0 * (x.numel() + out.numel()) + n * c * ring * (12.0 + 16.0)
    with _HbmTimed("cube_pad_f32_kernel", "CubePad a%d n%d" % (a, n), counted, x.device):
        call("pconv_cube_pad_f32", _ptr(x), _ptr(out), _ptr(table), n, c, a, _stream(x.device))
    return out


WS_WEIGHTINGS = {"ws": 0, "uniform": 1}  # PCONV_WS_WEIGHT_SPHERE, PCONV_WS_WEIGHT_UNIFORM


def ws_metrics(x, y, weighting="ws"):
    """WS-MSE and WS-SSIM of each frame (pconv_ws_metrics_f32 / _u8, sphere_metrics.py): x, y GPU tensors of the
    same shape, both contiguous float32 (n, C, h, w) or both uint8 (n, h, w, 3) (read as float(u8) / 255).
    Returns a float64 CPU tensor (n, 2): [:, 0] the weighted MSE, [:, 1] the weighted SSIM"""
    return ws_metrics_device(x, y, weighting).cpu()


def _ws_frames(what, x, y, weighting, float_only, min_side, entry):
    """the checks shared by the sphere-metric entries; returns (n, c, h, w) and the forward entry's name, entry + "_f32"
    or "_u8" """
    if weighting not in WS_WEIGHTINGS:
        raise PconvError("%s: weighting must be one of %s, got %r" % (what, sorted(WS_WEIGHTINGS), weighting))
    if not (x.is_cuda and y.is_cuda):
        raise PconvError("%s: x and y: expected GPU tensors (this build has no CPU path), got %s and %s" % (what, x.device, y.device))
    if x.device != y.device or x.dtype != y.dtype or x.shape != y.shape:
        raise PconvError("%s: the two batches x and y differ: %s %s %s vs %s %s %s"
                         % (what, x.device, x.dtype, tuple(x.shape), y.device, y.dtype, tuple(y.shape)))
    if not (x.is_contiguous() and y.is_contiguous()) or x.dim() != 4:
        raise PconvError("%s: x and y: contiguous 4-D tensors expected" % what)
    if x.dtype == torch.float32:
        n, c, h, w = x.shape
        fn = entry + "_f32"
    elif x.dtype == torch.uint8 and x.shape[3] == 3 and not float_only:
        n, h, w, c = x.shape
        fn = entry + "_u8"
    else:
        raise PconvError("%s: float32 (n, C, h, w)%s expected, got %s %s"
                         % (what, "" if float_only else " or uint8 (n, h, w, 3)", x.dtype, tuple(x.shape)))
    if h < min_side or w < min_side:
        raise PconvError("%s: h and w must be at least %d, got %dx%d" % (what, min_side, w, h))
    return (n, c, h, w), fn


def _ws_gout(what, gout, x):
    """the upstream gradients of a sphere-metric backward entry: contiguous float64 (n, 2) next to the frames"""
    n = x.shape[0]
    if not gout.is_cuda or gout.device != x.device or gout.dtype != torch.float64 or tuple(gout.shape) != (n, 2) \
            or not gout.is_contiguous():
        raise PconvError("%s: gout must be contiguous float64 (%d, 2) on the inputs' device, got %s %s %s"
                         % (what, n, gout.device, gout.dtype, tuple(gout.shape)))


def ws_metrics_device(x, y, weighting="ws"):
    """ws_metrics with the float64 (n, 2) result left on the inputs' device: nothing waits for the kernel"""
    (n, c, h, w), fn = _ws_frames("ws_metrics", x, y, weighting, False, 1, "pconv_ws_metrics")
    nbytes = call("pconv_ws_metrics_workspace_bytes", n, h, w)
    workspace = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    out = torch.empty((n, 2), dtype=torch.float64, device=x.device)
    with _HbmTimed("ms_forward_kernel", "WsMetrics n%d" % n, 2.0 * x.numel() * x.element_size(), x.device):
        call(fn, _ptr(x), _ptr(y), n, c, h, w, WS_WEIGHTINGS[weighting], _ptr(workspace), _ptr(out), _stream(x.device))
    return out


def ws_metrics_backward(x, y, gout, weighting="ws"):
    """Gradient of Σ_f gout[f, 0]·WS-MSE_f + gout[f, 1]·WS-SSIM_f with respect to y (pconv_ws_metrics_backward_f32):
    x, y contiguous float32 (n, C, h, w) GPU tensors of the same shape, gout contiguous float64 (n, 2) on the same
    device (read by the kernel: no host copy).  Returns float32 (n, C, h, w).  For the gradient with respect to x
    swap x and y"""
    (n, c, h, w), _ = _ws_frames("ws_metrics_backward", x, y, weighting, True, 1, "pconv_ws_metrics")
    _ws_gout("ws_metrics_backward", gout, x)
    out = torch.empty_like(x)
    with _HbmTimed("ms_backward_kernel", "WsMetricsBackward n%d" % n, 12.0 * x.numel(), x.device):
        call("pconv_ws_metrics_backward_f32", _ptr(x), _ptr(y), _ptr(gout), n, c, h, w, WS_WEIGHTINGS[weighting],
             _ptr(out), _stream(x.device))
    return out


WS_MS_SCALES, WS_MS_MIN_SIDE = 5, 16


def ws_msssim_device(x, y, weighting="ws"):
    """WS-MS-SSIM of each frame (pconv_ws_msssim_f32 / _u8, include/pconv_hip.h states the definition): x, y GPU
    tensors of the same shape, both contiguous float32 (n, C, h, w) or both uint8 (n, h, w, 3), h, w >= 16.  Returns
    (values, workspace): values float64 (n, 7) on the device, columns 0-4 the per-scale v_0..v_4, column 5 WS-MSE,
    column 6 WS-MS-SSIM; workspace the uint8 tensor that holds the pyramid x_1, y_1, ..., x_4, y_4 (ws_msssim_levels)
    and that ws_msssim_backward reads.  Nothing waits for the kernels"""
    (n, c, h, w), fn = _ws_frames("ws_msssim", x, y, weighting, False, WS_MS_MIN_SIDE, "pconv_ws_msssim")
    nbytes = call("pconv_ws_msssim_workspace_bytes", n, c, h, w)
    workspace = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    out = torch.empty((n, 7), dtype=torch.float64, device=x.device)
    # the frames read once, the pyramid (one third of them as float32) written once and read once
    counted = 2.0 * x.numel() * x.element_size() + 2.0 * (2.0 * n * c * h * w * 4 / 3)
    with _HbmTimed("ms_forward_kernel", "WsMsSsim n%d" % n, counted, x.device):
        call(fn, _ptr(x), _ptr(y), n, c, h, w, WS_WEIGHTINGS[weighting], _ptr(workspace), _ptr(out), _stream(x.device))
    return out, workspace


def ws_msssim(x, y, weighting="ws"):
    """ws_msssim_device with the float64 (n, 7) values copied to the host; also returns the workspace"""
    out, workspace = ws_msssim_device(x, y, weighting)
    return out.cpu(), workspace


def ws_msssim_levels(workspace, n, c, h, w):
    """the pyramid inside a workspace of ws_msssim_device: [(x_1, y_1), ..., (x_4, y_4)] as float32 (n, c, h >> s,
    w >> s) views"""
    levels, at = [], 0
    for s in range(1, WS_MS_SCALES):
        hs, ws = h >> s, w >> s
        size = n * c * hs * ws
        pair = workspace[4 * at:4 * (at + 2 * size)].view(torch.float32)
        levels.append((pair[:size].view(n, c, hs, ws), pair[size:].view(n, c, hs, ws)))
        at += 2 * size
    return levels


def ws_msssim_backward(x, y, workspace, values, gout, weighting="ws", swapped=False):
    """Gradient of Σ_f gout[f, 0]·WS-MSE_f + gout[f, 1]·WS-MS-SSIM_f with respect to y (pconv_ws_msssim_backward_f32):
    x, y contiguous float32 (n, C, h, w) GPU tensors, (values, workspace) what ws_msssim_device returned for them,
    gout contiguous float64 (n, 2) on the same device (read by the kernels: no host copy).  Returns float32
    (n, C, h, w).  For the gradient with respect to x exchange x and y and pass swapped=True: the workspace then is
    that of the forward of (y, x)"""
    (n, c, h, w), _ = _ws_frames("ws_msssim_backward", x, y, weighting, True, WS_MS_MIN_SIDE, "pconv_ws_msssim")
    _ws_gout("ws_msssim_backward", gout, x)
    if values.device != x.device or values.dtype != torch.float64 or tuple(values.shape) != (n, 7) \
            or not values.is_contiguous():
        raise PconvError("ws_msssim_backward: values must be contiguous float64 (%d, 7) on the inputs' device, got %s %s %s"
                         % (n, values.device, values.dtype, tuple(values.shape)))
    nbytes = _host_query("pconv_ws_msssim_workspace_bytes", n, c, h, w)
    if workspace.device != x.device or workspace.dtype != torch.uint8 or workspace.numel() != nbytes \
            or not workspace.is_contiguous():
        raise PconvError("ws_msssim_backward: the workspace must be the %d bytes ws_msssim_device returned, got %s %s %s"
                         % (nbytes, workspace.device, workspace.dtype, tuple(workspace.shape)))
    coarse = torch.empty((call("pconv_ws_msssim_backward_workspace_bytes", n, c, h, w),), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    with _HbmTimed("ms_backward_kernel", "WsMsSsimBackward n%d" % n, 16.0 * x.numel(), x.device):
        call("pconv_ws_msssim_backward_f32", _ptr(x), _ptr(y), _ptr(workspace), _ptr(values), _ptr(gout), n, c, h, w,
             WS_WEIGHTINGS[weighting], 1 if swapped else 0, _ptr(coarse), _ptr(out), _stream(x.device))
    return out


def tile_gdn(owner, x, gamma, beta, inverse, col_limit=None, npart=0, residual=None, ring=0):
    """PseudoGDNV2.forward in one launch: x / sqrt(beta + gamma x^2) (inverse: x * sqrt)
    (+ residual), zeros from each tile's col_limit on.  gamma (ch, ch), beta (ch):
    effective values.  ring: see tile_conv2d.  x and residual: row-strided views accepted (any other view is
    copied); gamma and beta: any strides (packed / copied dense); col_limit: contiguous int32, at least npart long."""
    x = _require_rows(x, "tile_gdn: x")
    tn, ch, h, w = x.shape
    _require_operand(gamma, "tile_gdn", "gamma", (ch, ch), torch.float32, x, dense=False)
    _require_operand(beta, "tile_gdn", "beta", (ch,), torch.float32, x, dense=False)
    if col_limit is not None:
        _require_operand(col_limit, "tile_gdn", "col_limit", int(npart), torch.int32, x)
    stream = _stream(x.device)
    out = _ring_output((tn, ch, h, w), ring, x)
    residual = _like_output(residual, out, "tile_gdn: residual")
    packed = packed_conv_weight(owner, gamma.view(ch, ch, 1, 1), stream)      # (the first call of the library)
    views = _views(x, out, residual)

    def describe():
        # (+ algorithmic HBM bytes: x in, y out, the residual: each once)
        return (conv_kernel_name(ch, 1, 1, True, cin=ch, pixels=tn * h * w), "GDN %d w%d" % (ch, w),
                2.0 * ch * ch * tn * h * w * _VALID_FRACTION,
                4.0 * ch * tn * h * w * _VALID_FRACTION * (3 if residual is not None else 2))

    beta = beta.detach().contiguous()      # (kept for the duration of the call)
    with _ConvTimed(x.device, describe):
        call("pconv_gdn", _ptr(x), _ptr(packed), _ptr(beta), _ptr(out), tn, ch, h, w,
             1 if inverse else 0, _ptr(col_limit), int(npart), _ptr(residual), ctypes.addressof(views), stream)
    return out


FUSED_EPILOGUE = True  # tile_conv2d takes sigmoid / gate / residual / trim


def tile_conv2d(owner, x, weight, bias, stride, slope=None, col_limit=None, npart=0, sigmoid=False, gate=None,
                residual=None, trim=False, ring=0, d2w=False):
    """y = conv2d(x, weight, bias, stride), no padding, on the fp32 matrix cores, then in
    the same launch PReLU(slope) or sigmoid, * gate, + residual, and (trim) zeros from
    each tile's col_limit on.  x (tn, cin, h, w) -> (tn, cout, ho, wo).  x, gate and
    residual may be interior views of padded buffers.  ring > 0: the result is written
    into the interior of a buffer padded by `ring` (returned as that view), so that a
    following PseudoPad only has to fill the ring.  d2w: DtowOp(2, True) applied by the
    store, the result is (tn, cout/4, 2*ho, 2*wo).  x, gate and residual: row-strided views accepted (any other
    view is copied); weight: any strides (it is packed); bias and slope: contiguous float32 (cout); col_limit:
    contiguous int32, at least npart long.  Every operand is checked before the first call of the library."""
    x = _require_rows(x, "tile_conv2d: x")
    tn, cin, h, w = x.shape
    _require_operand(weight, "tile_conv2d", "weight", (None, cin, None, None), torch.float32, x, dense=False)
    cout, cin_w, k, k2 = weight.shape
    if k != k2:
        raise PconvError("tile_conv2d: weight %s does not fit input %s" % (tuple(weight.shape), tuple(x.shape)))
    if bias is not None:
        _require_operand(bias, "tile_conv2d", "bias", (cout,), torch.float32, x)
    if slope is not None:
        _require_operand(slope, "tile_conv2d", "slope", (cout,), torch.float32, x)
    if col_limit is not None:
        _require_operand(col_limit, "tile_conv2d", "col_limit", int(npart), torch.int32, x)
    stream = _stream(x.device)
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    out = _ring_output((tn, cout // 4, 2 * ho, 2 * wo) if d2w else (tn, cout, ho, wo), ring, x)
    if sigmoid and slope is not None:
        raise PconvError("tile_conv2d: PReLU and sigmoid are exclusive")
    if d2w and (gate is not None or residual is not None or trim or sigmoid or cout % 4):
        raise PconvError("tile_conv2d: d2w takes no sigmoid / gate / residual / trim and needs cout % 4 == 0")
    gate = _like_output(gate, out, "tile_conv2d: gate")
    residual = _like_output(residual, out, "tile_conv2d: residual")
    # (only a 3x3 layer can go to the kernels that ask for it)
    fused = sigmoid or gate is not None
    aligned = k == 3 and _aligned8(out) and (residual is None or _aligned8(residual))
    launches, fallback = conv_plan(cin, h, w, cout, k, stride, d2w, fused, aligned)
    if fallback and not aligned and _aligned8(out) and residual.data_ptr() % 8 and \
            residual.stride(0) % 2 == 0 and residual.stride(1) % 2 == 0 and residual.stride(2) % 2 == 0:
        # the residual's start alone keeps the layer off its kernel: where a dense copy has 8-byte aligned rows, the
        # layer takes the kernel -- and gives the bits -- of the same call with an aligned residual
        wanted = conv_plan(cin, h, w, cout, k, stride, d2w, fused, True)
        if not wanted[1] and wo % 2 == 0 and (ho * wo) % 2 == 0:      # (a kernel takes the layer; the copy's strides are even)
            residual, aligned = residual.clone(memory_format=torch.contiguous_format), True
            launches, fallback = wanted
    if fallback:
        # a plain 3x3 stride-1 layer that Winograd was selected for went to the direct kernel (shape not
        # taken, or output / residual rows not 8-byte aligned): counted, so that the choice is never silent
        key = (cin, h, w, cout, bool(d2w))
        conv_fallbacks[key] = conv_fallbacks.get(key, 0) + 1
    act = 4 if sigmoid else (1 if slope is not None else 0)
    bias_p, slope_p = _ptr(bias.detach()) if bias is not None else None, _ptr(slope.detach()) if slope is not None else None

    def winograd(kind, r0, rows):
        """output rows [r0, r0 + rows) by one Winograd launch over row views (whole tensors: r0 = 0, rows = ho)"""
        kernel = CONV_KERNELS[kind]
        whole = r0 == 0 and rows == ho
        rs = 2 if d2w else 1
        xv = x if whole else x[:, :, r0:r0 + rows + 2]
        ov = out if whole else out[:, :, rs * r0:rs * (r0 + rows)]
        rv = residual if (whole or residual is None) else residual[:, :, r0:r0 + rows]

        def describe():
            return (kernel.probe_name, "3x3 s1 %d->%d w%d" % (cin, cout, wo) + ("" if whole else (" rows %d of %d" % (rows, ho))),
                    2.0 * cin * 9 * cout * tn * rows * wo * _VALID_FRACTION,
                    4.0 * tn * _VALID_FRACTION * (cin * (rows + 2) * w + cout * rows * wo * (1 + (residual is not None))))

        with _ConvTimed(x.device, describe):
            views = _views(xv, ov, rv)
            call(kernel.entry, _ptr(xv), _ptr(_packed_weight(owner, weight, kind, stream)), bias_p, _ptr(ov), tn, cin,
                 rows + 2, w, cout, act, slope_p, _ptr(col_limit), int(npart), _ptr(rv), 1 if trim else 0,
                 1 if d2w else 0, ctypes.addressof(views), stream)

    def direct():
        def describe():
            # algorithmic HBM bytes: the input once, the output once, residual / gate once each
            return (conv_kernel_name(cout, k, stride, cin=cin, pixels=tn * h * w),
                    "%dx%d s%d %d->%d w%d" % (k, k, stride, cin, cout, wo), 2.0 * cin * k * k * cout * tn * ho * wo * _VALID_FRACTION,
                    4.0 * tn * _VALID_FRACTION * (cin * h * w + cout * ho * wo * (1 + (residual is not None) + (gate is not None))))

        with _ConvTimed(x.device, describe):
            views = _views(x, out, residual, gate)
            call("pconv_conv2d", _ptr(x), _ptr(_packed_weight(owner, weight, "direct", stream)), bias_p, _ptr(out),
                 tn, cin, h, w, cout, k, int(stride), act, slope_p, _ptr(col_limit), int(npart),
                 _ptr(residual), _ptr(gate), 1 if trim else 0, 1 if d2w else 0, ctypes.addressof(views), stream)

    for kind, r0, rows in launches:
        if kind == "direct":   # always the whole layer
            direct()
        else:
            winograd(kind, r0, rows)
    return out


def _conv_tensors(where, tensors):
    """every tensor of a call is checked, whether the call reads it or not: the entry points take raw addresses"""
    first = tensors[0][1]
    for name, t, dims in tensors:
        if not isinstance(t, torch.Tensor) or t.dim() != dims:
            raise PconvError("%s: %s must be a %d-D tensor" % (where, name, dims))
        _require_gpu(t.detach(), "%s: %s" % (where, name))
        if t.device != first.device:
            raise PconvError("%s: %s is on %s, %s on %s" % (where, name, t.device, tensors[0][0], first.device))


# The two families of convolutions with a native backward: the kernel sizes and strides their entry points accept,
# whether those entry points take (k, stride) as arguments (those of one size and one stride do not), the slot of the
# transposed pack on its owner, and the entry points.
ConvFamily = collections.namedtuple(
    "ConvFamily", "ksizes strides sized slot_t packed_size pack_weight_transposed dgrad_workspace dgrad wgrad_workspace wgrad")
_TILE_CONV = ConvFamily((1, 3), (1, 2), True, "_pconv_packed_t", "pconv_conv_packed_size", "pconv_conv_pack_weight_transposed",
                        "pconv_conv2d_dgrad_workspace_bytes", "pconv_conv2d_dgrad", "pconv_conv2d_wgrad_workspace_bytes",
                        "pconv_conv2d_wgrad")
_CONV5 = ConvFamily((5,), (1,), False, "_pconv_packed5_t", "pconv_conv5_packed_size", "pconv_conv5_pack_weight_transposed",
                    "pconv_conv5_dgrad_workspace_bytes", "pconv_conv5_dgrad", "pconv_conv5_wgrad_workspace_bytes",
                    "pconv_conv5_wgrad")


def _pack_transposed(weight, family, stream):
    """the flipped, transposed weights of the data gradient in the slab layout of the family's forward (the
    transposed layer has cin output and cout input channels)"""
    cout, cin, k = weight.shape[:3]
    ks = (k,) if family.sized else ()
    return _pack(weight, family.packed_size, (cin, cout) + ks + (None, None), family.pack_weight_transposed, (cout, cin) + ks,
                 stream)


def _conv_backward(where, family, x, weight, gout, stride, need, owner):
    """(gin, gw, gb) of y = conv2d(x, weight, bias, stride), no padding, for a convolution of `family`, from
    gout = dL/dy; a gradient `need` does not ask for is neither computed nor returned (None)"""
    need_x, need_w, need_b = (bool(n) for n in need)
    _conv_tensors(where, [("gout", gout, 4), ("x", x, 4), ("weight", weight, 4)])
    tn, cout, ho, wo = gout.shape
    cout_w, cin, k, k2 = weight.shape
    stride = int(stride)
    tn_x, cin_x, h, w = x.shape
    if (tn_x, cin_x, cout_w, k2) != (tn, cin, cout, k) or k not in family.ksizes or stride not in family.strides or \
            ((h - k) // stride + 1, (w - k) // stride + 1) != (ho, wo) or ho < 1 or wo < 1:
        raise PconvError("%s: x %s, weight %s, gout %s, stride %d do not fit"
                         % (where, tuple(x.shape), tuple(weight.shape), tuple(gout.shape), stride))
    stream = _stream(gout.device)
    lib = _native.hip_lib()
    ks, kst = ((k,), (k, stride)) if family.sized else ((), ())

    def workspace(nbytes):
        if nbytes < 0:
            raise PconvError("%s: workspace query failed: %s" % (where, (lib.pconv_last_error() or b"").decode()))
        return torch.empty(int(nbytes), dtype=torch.uint8, device=gout.device) if nbytes else None

    gin = gw = gb = None
    if need_x:
        packed = _cached_pack(weight if owner is None else owner, family.slot_t, weight, _pack_transposed, family, stream)
        gin = torch.empty((tn, cin, h, w), dtype=torch.float32, device=gout.device)
        ws = workspace(getattr(lib, family.dgrad_workspace)(tn, cout, h, w, *kst))
        call(family.dgrad, _ptr(gout), _ptr(packed), _ptr(gin), _ptr(ws), tn, cin, h, w, cout, *kst + (stream,))
    if need_w or need_b:
        if need_w:
            gw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=gout.device)
        if need_b:
            gb = torch.empty((cout,), dtype=torch.float32, device=gout.device)
        # (a bias-only call needs the fp64 planes alone, not the partials in front of them)
        ws = workspace(getattr(lib, family.wgrad_workspace)(tn, cin, cout, *ks) if need_w else tn * cout * 8)
        call(family.wgrad, _ptr(x) if need_w else None, _ptr(gout), _ptr(gw), _ptr(gb), _ptr(ws), tn, cin, h, w, cout,
             *kst + (stream,))
    return gin, gw, gb


def tile_conv2d_backward(x, weight, gout, stride, need=(True, True, True), owner=None):
    """(gin, gw, gb) of y = conv2d(x, weight, bias, stride), no padding, from gout = dL/dy, in the orders
    include/pconv_hip.h defines; a gradient `need` does not ask for is neither computed nor returned (None).
    x (tn, cin, h, w), weight (cout, cin, k, k), gout (tn, cout, ho, wo): dense fp32 on the GPU.  owner: the object
    that caches the transposed pack (default: the weight tensor itself)."""
    return _conv_backward("tile_conv2d_backward", _TILE_CONV, x, weight, gout, stride, need, owner)


# ---- the optimiser step (optim.Adam on GPU tensors) ----------------------------------------------------------------

OptimSegments = collections.namedtuple("OptimSegments", "table counts ntensor nsegment")


def optim_segments(counts, device):
    """the segment table (pconv_host_optim_segments) of tensors of `counts` elements, on `device`; depends on the
    sizes alone"""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.ndim != 1 or counts.size < 1:
        raise PconvError("optim_segments: a non-empty list of element counts expected")
    nsegment = call("pconv_host_optim_segments", _np_ptr(counts), counts.size, None)
    table = np.empty((nsegment, 2), dtype=np.int32)
    call("pconv_host_optim_segments", _np_ptr(counts), counts.size, _np_ptr(table))
    return OptimSegments(torch.from_numpy(table).to(device), counts, int(counts.size), int(nsegment))


def optim_step(records, segments, clip, device):
    """pconv_optim_sqnorm + pconv_optim_adam over the device table `records` ((ntensor, 9) int64: pconv_optim_tensor)
    in THE ORDER of include/pconv_hip.h: two launches and the closing launch of the norm.  Returns the workspace as
    float64: [0] total, [1] norm, the low half of [2] the fp32 clip coefficient, then the segment partials.  records and
    segments.table: contiguous, on `device`; the tensors behind the records' addresses are the caller's to check
    (optim.Adam does)."""
    table = segments.table
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (segments.nsegment, 2) or \
            not table.is_cuda or not table.is_contiguous() or table.device != torch.device(device):
        raise PconvError("optim_step: the table of segments must be a contiguous (%d, 2) int32 tensor on %s (optim_segments)"
                         % (segments.nsegment, device))
    if not isinstance(records, torch.Tensor) or records.dtype != torch.int64 or tuple(records.shape) != (segments.ntensor, 9) or \
            not records.is_cuda or not records.is_contiguous() or records.device != table.device:
        raise PconvError("optim_step: records must be a contiguous (%d, 9) int64 tensor on %s" % (segments.ntensor, device))
    stream = _stream(records.device)
    nbytes = call("pconv_optim_workspace_bytes", segments.ntensor, segments.nsegment)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=records.device)
    args = (_ptr(records), _ptr(table), _np_ptr(segments.counts), segments.ntensor, segments.nsegment)
    call("pconv_optim_sqnorm", *args + (float(clip), _ptr(ws), stream))
    call("pconv_optim_adam", *args + (_ptr(ws), stream))
    return ws


# ---- the masked 5x5 convolutions of the entropy model under training (native_masked_conv) ------------------------

def _pack5(weight, stream):
    """a (cout, cin, 5, 5) weight in pconv_conv5's slab layout.  The causal mask is written through weight.data (no
    version bump) -- but always to the same values at the same places, and _MaskConv.forward writes it before it
    comes here, so a pack made under a key of _cached_pack is the pack of the masked weight under that key (its
    transposed pack likewise)."""
    cout, cin = weight.shape[:2]
    return _pack(weight, "pconv_conv5_packed_size", (cout, cin, None, None), "pconv_conv5_pack_weight", (cout, cin), stream)


def conv5x5(owner, x, weight, bias):
    """y = conv2d(x, weight, bias) for a 5x5 weight, stride 1, no padding, on the fp32 matrix cores: x (tn, cin, h, w)
    -> (tn, cout, h - 4, w - 4), every output one fmaf chain over (ci, kh, kw) ascending, then + bias
    (include/pconv_hip.h).  The weight is taken as it is -- the caller has masked it.  owner: the object the pack is
    cached on."""
    _conv_tensors("conv5x5", [("x", x, 4), ("weight", weight, 4)] + ([("bias", bias, 1)] if bias is not None else []))
    tn, cin, h, w = x.shape
    cout, cin_w, k, k2 = weight.shape
    if cin != cin_w or (k, k2) != (5, 5) or h < 5 or w < 5:
        raise PconvError("conv5x5: weight %s does not fit input %s" % (tuple(weight.shape), tuple(x.shape)))
    if bias is not None and bias.shape[0] != cout:
        raise PconvError("conv5x5: bias %s does not fit weight %s" % (tuple(bias.shape), tuple(weight.shape)))
    stream = _stream(x.device)
    out = torch.empty((tn, cout, h - 4, w - 4), dtype=torch.float32, device=x.device)
    call("pconv_conv5", _ptr(x), _ptr(_cached_pack(owner, "_pconv_packed5", weight, _pack5, stream)),
         _ptr(bias.detach()) if bias is not None else None, _ptr(out), tn, cin, h, w, cout, stream)
    return out


def conv5x5_backward(x, weight, gout, need=(True, True, True), owner=None):
    """(gin, gw, gb) of y = conv5x5(x, weight, bias) from gout = dL/dy, in the orders include/pconv_hip.h defines; a
    gradient `need` does not ask for is neither computed nor returned (None).  gw is the dense gradient, masked taps
    included (what the vendor path returns too: the weights are masked again at every forward).  owner: the object
    that caches the transposed pack (default: the weight tensor itself)."""
    return _conv_backward("conv5x5_backward", _CONV5, x, weight, gout, 1, need, owner)
