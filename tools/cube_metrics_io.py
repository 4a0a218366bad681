"""Scoring cube pictures on the sphere (csrc/weighted_metrics.hip, cube.points_mse) on one GPU: eight 3-channel cube
pictures of a = 1024, as face stacks of 6144x1024.

Times, with device events (warm-up, which also builds and caches the weight plane, the records, the maps and the pad
table; then rounds that alternate the cases; the median of the rounds):
  weighted mse / backward     weighted_metrics.mse_device and .backward on the cube's solid-angle plane (two launches / one)
  ... composed from torch     (w * (x - y) ** 2).sum((2, 3)) / W on the device, and autograd's gradient of it (the backward
                              pass alone, on a graph built before the window)
  points nearest / lanczos / cpp   cube.points_mse with both operands cube pictures: the face continuation of both, then the
                              fused sphere-points kernel on the cube's own records (icosphere of level 8; the CPP grid of 2048x4096)
  ... through ERP             the path there was before: cube.to_erp of both pictures to 2048x4096, then sphere_points.mse
Counted bytes of the weighted kernels: x and y read once, the weight plane read once (forward: 8 HW + 8 n C HW; backward: the
same plus the gradient written, 12 n C HW + 8 HW), against 8 TB/s.  The point metrics are gathers: their time is reported,
not a rate.  The figures are measured against nothing: reported, not gated.

    python tools/cube_metrics_io.py [--rounds 10] [--out FILE]      (profiles/cube_metrics.txt holds the table as its last block)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import cube, sphere_points  # noqa: E402
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


def make_cases(dev, n, a, level):
    """[(name, callable, counted bytes or None, the name of the case it is compared with or None)]"""
    sp = cube.spec("cmp", "faces")
    g = torch.Generator().manual_seed(1)
    x = torch.rand((n, 3, 6 * a, a), generator=g).to(dev)
    y = (x + 0.02 * torch.rand((n, 3, 6 * a, a), generator=g).to(dev)).contiguous()
    plane = cube.weight_plane(sp, a)
    w, total = plane.on(dev), plane.total
    gout = torch.full((n, 3), 1.0 / 3.0, dtype=torch.float64, device=dev)
    pixels, planes = 6 * a * a, 3 * n
    # the torch composition and its graph (built once: the window holds the backward pass alone)
    yg = y.detach().clone().requires_grad_(True)
    composed = lambda t: (w * (x - t) ** 2).sum((2, 3)) / total
    loss = (composed(yg) * gout).sum()
    ico, cpp = sphere_points.icosphere_set(level), sphere_points.cpp_set(*cube.erp_size(a))
    erp = cube.erp_size(a)

    def through_erp(ps, interp):
        return sphere_points.mse(cube.to_erp(x, erp, sp), cube.to_erp(y, erp, sp), ps, interp)
    cases = [("weighted mse", lambda: WM.mse_device(x, y, plane), 8 * pixels + 8 * planes * pixels, None),
             ("weighted mse, torch", lambda: composed(y), None, "weighted mse"),
             ("weighted mse backward", lambda: WM.backward(x, y, plane, gout), 8 * pixels + 12 * planes * pixels, None),
             ("weighted mse backward, torch", lambda: torch.autograd.grad(loss, yg, retain_graph=True), None, "weighted mse backward")]
    for name, ps, interp in (("points nearest", ico, "nearest"), ("points lanczos", ico, "lanczos"), ("points cpp", cpp, "lanczos")):
        cases.append((name, lambda ps=ps, interp=interp: cube.points_mse(x, y, ps, interp, sp, sp), None, None))
        cases.append((name + ", through ERP", lambda ps=ps, interp=interp: through_erp(ps, interp), None, name))
    # the two forms of each pair compute the same quantity
    check = [("weighted mse", (WM.mse_device(x, y, plane) - composed(y)).abs().max().item() / composed(y).abs().max().item()),
             ("weighted mse backward", (WM.backward(x, y, plane, gout).double() - torch.autograd.grad(loss, yg, retain_graph=True)[0].double())
              .abs().max().item() / WM.backward(x, y, plane, gout).abs().max().item())]
    for name, ps, interp in (("points nearest", ico, "nearest"), ("points lanczos", ico, "lanczos")):
        ours, theirs = cube.points_mse(x, y, ps, interp, sp, sp), through_erp(ps, interp)
        check.append((name, ((ours - theirs).abs() / theirs).max().item()))
    return cases, check, (len(ico), len(cpp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--face", type=int, default=1024)
    ap.add_argument("--level", type=int, default=sphere_points.LEVEL)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cube_metrics_io: needs a GPU")
    dev = torch.device("cuda:0")
    cases, check, (n_ico, n_cpp) = make_cases(dev, args.frames, args.face, args.level)
    for c in cases:   # warm-up: code objects loaded, records, maps and tables built and cached, clocks up
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    text = table(args, cases, check, (n_ico, n_cpp), times, torch.cuda.get_device_name(dev))
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def table(args, cases, check, sizes, times, device):
    (n_ico, n_cpp), med = sizes, {k: statistics.median(v) for k, v in times.items()}
    lines = ["# cube metrics: %d cube pictures of 3 channels, a = %d, face stacks of %dx%d, float32; weight plane float64 (solid angles, cmp)"
             % (args.frames, args.face, 6 * args.face, args.face),
             "# points: icosphere of level %d (%d points), CPP grid of %dx%d (%d points); both operands cube pictures"
             % ((args.level, n_ico) + cube.erp_size(args.face)[::-1] + (n_cpp,)),
             "# 'torch': (w * (x - y) ** 2).sum((2, 3)) / W and autograd's backward of it; 'through ERP': cube.to_erp of both, then sphere_points.mse",
             "# counted bytes (weighted kernels only): inputs and the weight plane read once, the gradient written once; %% of "
             "%.0f TB/s" % (PEAK / 1e12),
             "# median of %d rounds of %d calls, rounds alternate the cases" % (args.rounds, args.reps),
             "# device: %s" % device,
             "%-36s %10s %10s %8s %7s %13s %9s" % ("case", "MB", "us", "TB/s", "% peak", "min-max us", "x ours")]
    for name, _, nbytes, against in cases:
        t = med[name]
        rate = "%10.1f %10.1f %8.2f %7.1f" % (nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK) if nbytes else \
            "%10s %10.1f %8s %7s" % ("-", t * 1e6, "-", "-")
        ratio = "%9.2f" % (t / med[against]) if against else "%9s" % ""
        lines.append("%-36s %s %6.0f-%6.0f %s" % (name, rate, min(times[name]) * 1e6, max(times[name]) * 1e6, ratio))
    lines.append("# the two forms of a pair agree within (relative): " + ", ".join("%s %.2g" % c for c in check))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
