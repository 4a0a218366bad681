"""Shared by tests/test_stale_memory_cpu.py (CPU) and tests/test_gpu_stale_memory.py (GPU): a result must not depend on
what freshly allocated memory held.

`filled(monkeypatch, kind)` replaces torch.empty, torch.empty_like and Tensor.new_empty for the duration of a block:
the replacements return the real allocation overwritten with a byte pattern.  torch.zeros stays as it is.

    tensor kind                                              fill "A"                     fill "B"
    float32 / float64 (and every other floating type)        every byte 0xFF: a NaN       every byte 0x3F: 0.7470588 as
                                                             in both widths               float32, finite, of unit scale
    uint8 workspaces that hold floating-point values only    as above                     as above
    integer tensors (maps, records, indices, counters,       every byte 0x00              every byte 0x01
      uint8 pictures) and workspaces that hold indices

Fill A fails every comparison of floating values; fill B stands for what a NaN cannot reach (clamps, max, PReLU selects
and `x < 0 ? ... : ...` swallow a NaN).  The integer patterns are both in range for every consumer: a hole in a map has
to show as a difference, not as a wild address.

A one-dimensional uint8 tensor allocated inside the package is a workspace; which kind it is, is said per allocating
function in WORKSPACES -- by file and qualified name (Class.method, outer.inner), so that no other function of the same
bare name is classified unseen -- with the sentence of include/pconv_hip.h that says what it holds.  A workspace
allocated by a function the table does not name is refused: the table stays complete.

`refill(op, kind)` overwrites every tensor an op owns (`_top`) with the pattern: the second use of an op-owned buffer.
The stepped ops (PCONV._WavefrontOp) carry their result from step to step by design and zero it at step 0: they are
refilled only before step 0 of a pass, after restart() -- refill() refuses any other moment.

UNWRITTEN lists the regions that may legitimately keep the fill, each with the sentence that declares it undefined."""
import contextlib
import os
import sys

import torch

KINDS = ("A", "B")
FLOAT_BYTE = {"A": 0xFF, "B": 0x3F}
INT_BYTE = {"A": 0x00, "B": 0x01}
B_FLOAT32 = 0.7470588088035583      # 0x3F3F3F3F

PACKAGE = os.sep + "pseudocylindrical_convolution_amd" + os.sep
TESTS = os.path.dirname(os.path.abspath(__file__))

# allocating function, "file:qualified name" -> (what the workspace holds, the header's words).
# Every one holds floating-point values only; none holds an index.
WORKSPACES = {
    "PCONV.py:ws_metrics_device": ("float", "pconv_ws_metrics_workspace_bytes(n, h, w) bytes (one fp64 pair per tile and frame)"),
    "PCONV.py:ws_msssim_device": ("float", "pconv_ws_msssim_workspace_bytes(n, c, h, w) bytes of device memory, 8-byte aligned: x_1, "
                                  "y_1, ..., x_4, y_4 as float32"),
    "PCONV.py:ws_msssim_backward": ("float", "pconv_ws_msssim_backward_workspace_bytes(n, c, h, w) bytes, 4-byte aligned: g_1..g_4 "
                                    "(one third of one input)"),
    "PCONV.py:erp_resample_f32": ("float", "workspace is device memory of pconv_erp_resample_workspace_bytes(...) bytes (mid)"),
    "PCONV.py:erp_resample_backward_f32": ("float", "device memory of pconv_erp_resample_backward_workspace_bytes(...) bytes (gmid)"),
    "PCONV.py:sphere_points_mse_device": ("float", "the chunk's partial, stored in the workspace (one double per plane and chunk)"),
    # PseudoQuantOp.backward under ordered_backward(True): the op's "partials" slot
    "PCONV.py:PseudoQuantOp.backward": ("float", "pconv_quant_backward_ordered_workspace_bytes(tn, c, levels) bytes (one fp64 per plane and level)"),
    # _conv_backward's local helper: the prepared gradient (float32), the weight partials (float32) and the bias
    # gradient's fp64 planes
    "PCONV.py:_conv_backward.workspace": ("float", "pconv_conv2d_dgrad_workspace_bytes(...) bytes / pconv_conv2d_wgrad_workspace_bytes(tn, cin, cout, "
                           "k) bytes; pconv_conv5_wgrad_workspace_bytes(tn, cin, cout) = tn * cout * cin * 25 * 4 rounded up to "
                           "16, + tn * cout * 8"),
}
OP_WORKSPACE_SLOTS = {"partials": "float"}     # uint8 tensors in an op's _top, by slot

# region -> the sentence that already declares it undefined (include/pconv_hip.h, or the docstring named)
UNWRITTEN = {
    "slice_pad_ring": "pconv_sphere_slice: only the interior is written when pad > 0, as in the reference.",
    "ring_output_before_forward_ring": "pconv_conv2d: Lets a convolution write the interior of a padded buffer (whose ring "
                                       "pconv_pseudo_pad_ring then fills) -- PCONV.tile_conv2d: ring > 0: the result is written "
                                       "into the interior of a buffer padded by `ring` (returned as that view), so that a "
                                       "following PseudoPad only has to fill the ring.",
    "engine_stream_beyond_length": "pconv_ee_stream: whatever the engine's buffer holds beyond them is undefined and must not "
                                   "be read.",
}


def _is_float(dtype):
    return dtype.is_floating_point or dtype.is_complex


def byte_for(dtype, kind, workspace=None):
    """the byte a tensor of `dtype` is filled with; workspace: "float" / "index" for a uint8 workspace"""
    assert kind in KINDS, kind
    if _is_float(dtype) or workspace == "float":
        return FLOAT_BYTE[kind]
    return INT_BYTE[kind]


def pattern(dtype, kind):
    """one element of the pattern as a tensor of `dtype`"""
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((size,), byte_for(dtype, kind), dtype=torch.uint8).view(dtype)[0]


def fill_(t, kind, workspace=None):
    """overwrite every byte of the dense tensor `t`"""
    if t.numel() == 0 or t.device.type == "meta" or t.layout != torch.strided:
        return t
    with torch.no_grad():      # (a leaf that asks for a gradient is filled too)
        flat = t.detach()
        # a fresh allocation is dense in some memory format: its numel() elements from the first on are all of it
        torch.as_strided(flat, (flat.numel(),), (1,)).view(torch.uint8).fill_(byte_for(t.dtype, kind, workspace))
    return t


CO_NESTED = 0x10


def allocation_site(frame):
    """"file:qualified name" of the function a frame runs: Class.method for a method (by its `self`), outer.inner for a
    function defined inside another (by the caller's frame), the bare name otherwise"""
    code = frame.f_code
    name = code.co_name
    if "self" in frame.f_locals and code.co_varnames[:1] == ("self",):
        owner = next((k for k in type(frame.f_locals["self"]).__mro__ if name in vars(k)), type(frame.f_locals["self"]))
        name = "%s.%s" % (owner.__name__, name)
    elif code.co_flags & CO_NESTED and frame.f_back is not None:
        name = "%s.%s" % (frame.f_back.f_code.co_name, name)
    return "%s:%s" % (os.path.basename(code.co_filename), name)


def _workspace_kind(t, depth):
    """None, or what the table says of a 1-D uint8 allocation made by a function of the package"""
    if t.dtype != torch.uint8 or t.dim() != 1:
        return None
    frame = sys._getframe(depth)
    while frame is not None and os.path.dirname(frame.f_code.co_filename) == TESTS:
        frame = frame.f_back      # (a test that wraps torch.empty itself, as tests/test_gpu_conv_backward.py does)
    if frame is None or PACKAGE not in frame.f_code.co_filename:
        return None
    name = allocation_site(frame)
    assert name in WORKSPACES, "stale_memory.WORKSPACES does not say what the uint8 workspace of %s holds" % name
    return WORKSPACES[name][0]


@contextlib.contextmanager
def filled(monkeypatch, kind):
    assert kind in KINDS, kind
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty
    made = []

    def empty(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        made.append("empty")
        return fill_(t, kind, _workspace_kind(t, 2))

    def empty_like(*args, **kwargs):
        made.append("empty_like")
        return fill_(real_like(*args, **kwargs), kind)

    def new_empty(self, *args, **kwargs):
        made.append("new_empty")
        return fill_(real_new(self, *args, **kwargs), kind)

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        m.setattr(torch, "empty_like", empty_like)
        m.setattr(torch.Tensor, "new_empty", new_empty)
        yield made
    assert torch.empty is real_empty and torch.empty_like is real_like and torch.Tensor.new_empty is real_new


def regimes(monkeypatch):
    """[(name, context manager factory)]: unpatched, fill A, fill B"""
    return [("plain", contextlib.nullcontext)] + [(k, (lambda k=k: filled(monkeypatch, k))) for k in KINDS]


def refill(op, kind):
    """overwrite every tensor the op owns with the pattern; a stepped op only before step 0 of a pass"""
    assert getattr(op, "pidx_", 0) == 0, "%s is refilled only before step 0 (after restart())" % type(op).__name__
    n = 0
    for slot, t in op._top.items():
        if isinstance(t, torch.Tensor):
            fill_(t, kind, OP_WORKSPACE_SLOTS.get(slot) if t.dtype == torch.uint8 else None)
            n += 1
    return n


def bits(t):
    """the tensor's bits as integers of its element size (float32 -> int32, float64 -> int64)"""
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b))


def holds_pattern(t, kind):
    """bool tensor: the elements of `t` that are the fill pattern of `kind`"""
    return bits(t) == bits(pattern(t.dtype, kind).to(t.device).reshape(1))
