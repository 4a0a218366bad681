"""WS-SSIM of cube pictures (cube.ws_ssim: csrc/cube.hip at depth 5, weighted_ssim_kernel of csrc/weighted_metrics.hip) on one
GPU: eight 3-channel cube pictures of a = 1024, as face stacks of 6144x1024; the padded stacks are 6204x1034.

Times, with device events (warm-up, which also builds and caches the pad table and the weight plane; then rounds that
alternate the cases; the median of the rounds):
  continue x / continue y     cube.pad(.., depth=5) of each picture (one launch each)
  weighted ssim               weighted_metrics.ssim_device on the two padded stacks and the plane (two launches)
  ws_ssim, whole              cube.ws_ssim_planes: the three above and the copy of the (n, C) result to the host
  ... torch, float64          the same definition composed from torch on the device: cube.pad_torch of both pictures and
                              weighted_metrics.ssim_torch (the tests' reference)
  ... torch, fp32 conv2d      the padded stacks through one grouped 11 x 11 conv2d per moment in float32, the map and the
                              weighted sum in torch
  erp ws_metrics              sphere_metrics' kernel (pconv_ws_metrics_f32) on the same two padded stacks read as ERP frames
                              of 6204x1034: the same pixels through the same tile passes, weighted by a row cosine instead
                              of a float64 plane -- what the per-pixel weights cost
Counted bytes: the continuation reads a stack and writes a padded one; the metric kernels read both padded stacks once,
the weighted one also the plane once per picture plane (it stays in cache: counted once); against 8 TB/s.  The figures
are measured against nothing: reported, not gated.

    python tools/cube_ssim_io.py [--rounds 10] [--out FILE]      (--out profiles/cube_ssim.txt records the table)
"""
import argparse
import os
import statistics
import sys

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


def conv2d_ssim(px, py, w, total):
    """the weighted SSIM of two padded stacks in float32 torch: the window g (x) g as one grouped conv2d per moment"""
    g = torch.tensor(sphere_metrics.gaussian(), dtype=torch.float32, device=px.device)
    n, c, h, wd = px.shape
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
    g = torch.Generator().manual_seed(1)
    x = torch.rand((n, 3, 6 * a, a), generator=g).to(dev)
    y = (x + 0.02 * torch.rand((n, 3, 6 * a, a), generator=g).to(dev)).contiguous()
    plane = cube.ssim_plane(kind, a)
    w, total = plane.on(dev), plane.total
    table = cube.pad_table_on(kind, a, dev, depth)
    px, py = cube.pad(x, kind, depth), cube.pad(y, kind, depth)
    planes, pixels, padded = 3 * n, 6 * a * a, 6 * A * A
    pad_bytes = 4 * planes * (pixels + padded)

    def torch64():
        return WM.ssim_torch(cube.pad_torch(x, table, depth), cube.pad_torch(y, table, depth), plane)
    cases = [("continue x", lambda: cube.pad(x, kind, depth), pad_bytes, None),
             ("continue y", lambda: cube.pad(y, kind, depth), pad_bytes, None),
             ("weighted ssim", lambda: WM.ssim_device(px, py, plane), 8 * planes * padded + 8 * padded, None),
             ("ws_ssim, whole", lambda: cube.ws_ssim_planes(x, y, sp), 2 * pad_bytes + 8 * planes * padded + 8 * padded, None),
             ("ws_ssim, torch, float64", torch64, None, "ws_ssim, whole"),
             ("weighted ssim, torch, fp32 conv2d", lambda: conv2d_ssim(px, py, w, total), None, "weighted ssim"),
             ("erp ws_metrics, same pixels", lambda: PCONV.ws_metrics_device(px, py, "ws"), 8 * planes * padded, "weighted ssim")]
    ours = cube.ws_ssim_planes(x, y, sp)
    check = [("torch float64", (ours - torch64().cpu()).abs().max().item()),
             ("fp32 conv2d", (WM.ssim_device(px, py, plane) - conv2d_ssim(px, py, w, total)).abs().max().item())]
    return cases, check, float(ours.mean())


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
        raise SystemExit("cube_ssim_io: needs a GPU")
    dev = torch.device("cuda:0")
    cases, check, figure = make_cases(dev, args.frames, args.face, args.kind)
    for c in cases:   # warm-up: code objects loaded, tables and planes built and cached, clocks up
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
    lines = ["# cube ws_ssim: %d cube pictures of 3 channels, %s, a = %d, face stacks of %dx%d, float32; continued by %d to %dx%d; "
             "weight plane float64 (solid angles, zero on the ring)" % (args.frames, args.kind, args.face, 6 * args.face, args.face,
                                                                         cube.SSIM_PAD, 6 * A, A),
             "# 'torch, float64': cube.pad_torch + weighted_metrics.ssim_torch on the device; 'fp32 conv2d': one grouped 11 x 11 conv2d "
             "per moment on the padded stacks",
             "# 'erp ws_metrics': pconv_ws_metrics_f32 on the same padded stacks read as ERP frames: row weights instead of a float64 plane",
             "# counted bytes: stacks read and written once, the plane once; %% of %.0f TB/s" % (PEAK / 1e12),
             "# median of %d rounds of %d calls, rounds alternate the cases; mean figure %.6f" % (args.rounds, args.reps, figure),
             "# device: %s" % device,
             "%-36s %10s %10s %8s %7s %13s %9s" % ("case", "MB", "us", "TB/s", "% peak", "min-max us", "x ours")]
    for name, _, nbytes, against in cases:
        t = med[name]
        rate = "%10.1f %10.1f %8.2f %7.1f" % (nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK) if nbytes else \
            "%10s %10.1f %8s %7s" % ("-", t * 1e6, "-", "-")
        ratio = "%9.2f" % (t / med[against]) if against else "%9s" % ""
        lines.append("%-36s %s %6.0f-%6.0f %s" % (name, rate, min(times[name]) * 1e6, max(times[name]) * 1e6, ratio))
    lines.append("# the kernels against the torch forms (absolute, per plane): " + ", ".join("%s %.2g" % c for c in check))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
