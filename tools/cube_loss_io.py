"""Training on cube pictures (cube.ws_ssim_loss_terms, cube.ws_loss_terms: cube_pad_backward_f32_kernel of csrc/cube.hip and
the weight-plane form of ms_backward_kernel, csrc/sphere_metrics.hip) on one GPU: eight 3-channel cube pictures of
a = 1024 as face stacks of 6144x1024; the stacks continued by 5 are 6204x1034.

Times, with device events (warm-up, which also builds and caches the table, the reverse lists and the weight planes; then
rounds that alternate the cases; the median of the rounds):
  pad backward                cube.pad_backward of a gradient of the padded stacks (one launch)
  ... torch                   the same adjoint composed from torch on the device: the interior slice plus four index_add_
                              of the ring gradients times their coefficients (float atomics: no defined order)
  weighted ssim backward      weighted_metrics.ssim_backward on two padded stacks and the plane (one launch)
  ... torch, fp32 conv2d      the same gradient from torch autograd of the SSIM written with one grouped 11 x 11 conv2d per
                              moment in float32, forward and backward
  erp ws_metrics backward     sphere_metrics' kernel (pconv_ws_metrics_backward_f32) on the same padded stacks read as ERP
                              frames: the same passes with a per-row factor -- what the per-pixel factor costs
  composite loss, fwd + bwd   mean of cube.ws_loss_terms + 0.1 (1 - mean of cube.ws_ssim_loss_terms) of two face stacks, and
                              its gradient with respect to one of them
  ... torch                   the same expression from torch on the device: index continuation, conv2d SSIM, autograd
Counted bytes: the pad backward reads a padded gradient and writes a stack; the SSIM backward reads both padded stacks and
writes one gradient, the plane once (it stays in cache); against 8 TB/s.  The figures are measured against nothing:
reported, not gated.

    python tools/cube_loss_io.py [--rounds 10] [--out FILE]      (--out profiles/cube_loss.txt records the table)
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, cube, sphere_metrics  # noqa: E402
from pseudocylindrical_convolution_amd import weighted_metrics as WM  # noqa: E402

PEAK = 8e12   # bytes / s of HBM


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


class TorchPad(object):
    """the continuation and its adjoint from torch indexing on the device (differentiable; the adjoint by index_add_)"""

    def __init__(self, kind, a, depth, dev):
        rec = torch.from_numpy(np.array(cube.pad_table(kind, a, depth))).long().to(dev)
        A = a + 2 * depth
        ring = A * A - a * a
        g = rec[:, 0].clamp(0, 5)
        x0, y0 = (rec[:, 1] >> 8).clamp(0, a - 1), (rec[:, 2] >> 8).clamp(0, a - 1)
        x1, y1 = (x0 + 1).clamp(max=a - 1), (y0 + 1).clamp(max=a - 1)
        fx, fy = (rec[:, 1] & 255).float() / 256.0, (rec[:, 2] & 255).float() / 256.0
        self.at = [(g * a + yy) * a + xx for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
        self.coef = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
        R, Q = (torch.from_numpy(v).to(dev) for v in cube.ring_pixels(a, depth))
        face = torch.arange(6, device=dev).repeat_interleave(ring)
        self.ring_at = (face * A + R.repeat(6)) * A + Q.repeat(6)
        self.a, self.A, self.depth = a, A, depth

    def forward(self, y):
        n, c = y.shape[:2]
        flat = y.reshape(n, c, -1)
        value = sum(flat[:, :, at] * coef for at, coef in zip(self.at, self.coef))
        out = F.pad(y.reshape(n, c, 6, self.a, self.a), (self.depth,) * 4).reshape(n, c, -1)
        return out.index_copy(2, self.ring_at, value).reshape(n, c, 6 * self.A, self.A)

    def backward(self, g):
        n, c = g.shape[:2]
        d, a = self.depth, self.a
        gin = g.reshape(n, c, 6, self.A, self.A)[:, :, :, d:d + a, d:d + a].reshape(n, c, -1).clone()
        ring = g.reshape(n, c, -1)[:, :, self.ring_at]
        for at, coef in zip(self.at, self.coef):
            gin.index_add_(2, at, ring * coef)
        return gin.reshape(n, c, 6 * a, a)


def conv2d_ssim(px, py, w, total):
    """the weighted SSIM per plane of two padded stacks in float32 torch: the window g (x) g as one grouped conv2d per moment"""
    g = torch.tensor(sphere_metrics.gaussian(), dtype=torch.float32, device=px.device)
    c = px.shape[1]
    window = (g[:, None] * g[None, :])[None, None].repeat(c, 1, 1, 1)
    blur = lambda t: F.conv2d(t, window, padding=5, groups=c)
    mx, my = blur(px), blur(py)
    sxx, syy, sxy = blur(px * px) - mx * mx, blur(py * py) - my * my, blur(px * py) - mx * my
    ssim_map = ((2 * mx * my + sphere_metrics.C1) * (2 * sxy + sphere_metrics.C2)) / \
        ((mx * mx + my * my + sphere_metrics.C1) * (sxx + syy + sphere_metrics.C2))
    return (ssim_map.double() * w).sum(dim=(2, 3)) / total


def make_cases(dev, n, a, kind):
    """[(name, callable, counted bytes or None, the name of the case it is compared with or None)]"""
    sp = cube.spec(kind, "faces")
    depth = cube.SSIM_PAD
    A = a + 2 * depth
    gen = torch.Generator().manual_seed(1)
    x = torch.rand((n, 3, 6 * a, a), generator=gen).to(dev)
    y = (x + 0.02 * torch.rand((n, 3, 6 * a, a), generator=gen).to(dev)).contiguous()
    plane, area = cube.ssim_plane(kind, a), cube.weight_plane(sp, a)
    w, total = plane.on(dev), plane.total
    wa, area_total = area.on(dev), area.total
    px, py = cube.pad(x, kind, depth), cube.pad(y, kind, depth)
    g_pad = torch.randn((n, 3, 6 * A, A), generator=gen).to(dev)
    gout = (torch.randn((n, 3), generator=gen, dtype=torch.float64) + 2.0).to(dev)
    pairs = torch.stack([torch.zeros(n, dtype=torch.float64, device=dev), gout[:, 0]], dim=1).contiguous()
    tpad = TorchPad(kind, a, depth, dev)
    planes, pixels, padded = 3 * n, 6 * a * a, 6 * A * A

    def ssim_backward_torch():
        leaf = py.detach().requires_grad_(True)
        (grad,) = torch.autograd.grad(conv2d_ssim(px, leaf, w, total), leaf, gout)
        return grad

    def loss_ours():
        leaf = y.detach().requires_grad_(True)
        loss = cube.ws_loss_terms(x, leaf, sp).mean() + 0.1 * (1 - cube.ws_ssim_loss_terms(x, leaf, sp).mean())
        (grad,) = torch.autograd.grad(loss, leaf)
        return loss.detach(), grad

    def loss_torch():
        leaf = y.detach().requires_grad_(True)
        d = x - leaf
        mse = ((d * d).double() * wa).sum(dim=(2, 3)) / area_total
        ssim = conv2d_ssim(tpad.forward(x), tpad.forward(leaf), w, total)
        loss = mse.mean(dim=1).mean() + 0.1 * (1 - ssim.mean(dim=1).mean())
        (grad,) = torch.autograd.grad(loss, leaf)
        return loss.detach(), grad

    cases = [("pad backward", lambda: cube.pad_backward(g_pad, kind, a, depth), 4 * planes * (pixels + padded), None),
             ("pad backward, torch", lambda: tpad.backward(g_pad), None, "pad backward"),
             ("weighted ssim backward", lambda: WM.ssim_backward(px, py, plane, gout), 12 * planes * padded + 8 * padded, None),
             ("weighted ssim backward, torch, fp32 conv2d", ssim_backward_torch, None, "weighted ssim backward"),
             ("erp ws_metrics backward, same pixels", lambda: PCONV.ws_metrics_backward(px, py, pairs, "ws"), 12 * planes * padded,
              "weighted ssim backward"),
             ("composite loss, fwd + bwd", loss_ours, None, None),
             ("composite loss, fwd + bwd, torch", loss_torch, None, "composite loss, fwd + bwd")]
    ours, theirs = loss_ours(), loss_torch()
    scale = lambda t: t.abs().max().item()
    check = [("pad backward / torch", (cube.pad_backward(g_pad, kind, a, depth) - tpad.backward(g_pad)).abs().max().item() / scale(g_pad)),
             ("ssim backward / conv2d", scale(WM.ssim_backward(px, py, plane, gout) - ssim_backward_torch()) / scale(ssim_backward_torch())),
             ("loss", abs(ours[0].item() - theirs[0].item())), ("loss gradient / torch", scale(ours[1] - theirs[1]) / scale(theirs[1]))]
    return cases, check, ours[0].item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--face", type=int, default=1024)
    ap.add_argument("--kind", default="cmp", choices=sorted(cube.KINDS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cube_loss_io: needs a GPU")
    dev = torch.device("cuda:0")
    cases, check, figure = make_cases(dev, args.frames, args.face, args.kind)
    for c in cases:   # warm-up: code objects loaded, tables, lists and planes built and cached, clocks up
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    text = table(args, cases, check, figure, times, torch.cuda.get_device_name(dev))
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def table(args, cases, check, figure, times, device):
    med = {k: statistics.median(v) for k, v in times.items()}
    A = args.face + 2 * cube.SSIM_PAD
    lines = ["# cube loss: %d cube pictures of 3 channels, %s, a = %d, face stacks of %dx%d, float32; continued by %d to %dx%d; "
             "weight planes float64" % (args.frames, args.kind, args.face, 6 * args.face, args.face, cube.SSIM_PAD, 6 * A, A),
             "# 'torch': the same expression composed from torch on the device (index_add_ adjoint, one grouped 11 x 11 conv2d per "
             "moment in float32, autograd)",
             "# 'erp ws_metrics backward': pconv_ws_metrics_backward_f32 on the same padded stacks read as ERP frames: a per-row factor",
             "# counted bytes: gradients and stacks read and written once, the plane once; %% of %.0f TB/s" % (PEAK / 1e12),
             "# median of %d rounds of %d calls, rounds alternate the cases; composite loss %.6f" % (args.rounds, args.reps, figure),
             "# device: %s" % device,
             "%-44s %10s %10s %8s %7s %15s %9s" % ("case", "MB", "us", "TB/s", "% peak", "min-max us", "x ours")]
    for name, _, nbytes, against in cases:
        t = med[name]
        rate = "%10.1f %10.1f %8.2f %7.1f" % (nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK) if nbytes else \
            "%10s %10.1f %8s %7s" % ("-", t * 1e6, "-", "-")
        ratio = "%9.2f" % (t / med[against]) if against else "%9s" % ""
        lines.append("%-44s %s %7.0f-%7.0f %s" % (name, rate, min(times[name]) * 1e6, max(times[name]) * 1e6, ratio))
    lines.append("# the kernels against the torch forms (relative to the largest value; the loss absolute): "
                 + ", ".join("%s %.2g" % c for c in check))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
