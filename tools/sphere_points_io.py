"""The sphere-sampled metrics (csrc/sphere_points.hip) on one GPU: the kernel rows of profiles/sphere_points.txt.

Times the fused PCONV.sphere_points_mse_device for S-PSNR-NN and S-PSNR-I (icosphere level 8) and for CPP-PSNR (the CPP
grid of the picture's size), and PCONV.sphere_points_sample_f32 (both modes, icosphere level 8), on float32 frames of three
planes at 4096x2048 with n = 8 and at 8192x4096 with n = 1, with device events (warm-up, then rounds that alternate the
cases; the median of the rounds).  x and y have the same size, y = x + noise; the records of both are made once.
Algorithmic bytes: per plane and point (36 taps lanczos | 1 nearest) x 4 bytes per picture read, the records, and for the
sampler its output: a rate of requests, most of them served by L1 / L2, NOT an HBM rate.

    python tools/sphere_points_io.py [--rounds 10] [--out profiles/sphere_points_io.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, sphere_points  # noqa: E402

SHAPES = [(8, 2048, 4096), (1, 4096, 8192)]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sphere_points_io: needs a GPU")
    dev = torch.device("cuda:0")
    ico = sphere_points.icosphere_set()
    cases = []
    for n, h, w in SHAPES:
        x = torch.rand((n, 3, h, w), device=dev)
        y = (x + 0.05 * torch.randn_like(x)).clamp_(0, 1)
        size = "%dx%d n%d" % (w, h, n)
        rec = ico.records(h, w, dev)
        grid = sphere_points.cpp_set(h, w).records(h, w, dev)
        planes = n * 3
        for name, r, interp in (("S-PSNR-NN ico8", rec, "nearest"), ("S-PSNR-I ico8", rec, "lanczos"), ("CPP-PSNR", grid, "lanczos")):
            taps = 36 if interp == "lanczos" else 1
            cases.append(("mse %s %s" % (name, size), lambda x=x, y=y, r=r, i=interp: PCONV.sphere_points_mse_device(x, r, y, r, i),
                          planes * r.shape[0] * (2 * 4 * taps + 16)))
        for interp in ("nearest", "lanczos"):
            taps = 36 if interp == "lanczos" else 1
            out = torch.empty((n, 3, rec.shape[0]), device=dev)
            cases.append(("sample %s ico8 %s" % (interp, size),
                          lambda x=x, r=rec, i=interp, out=out: PCONV.sphere_points_sample_f32(x, r, i, out),
                          planes * rec.shape[0] * 4 * (taps + 1) + 8 * n * rec.shape[0]))
    for c in cases:   # warm-up: code objects loaded, the phase table on the device, clocks up
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    lines = ["# sphere_points: the fused mean squared error over the points (two launches) and the sampler (one launch), float32, "
             "three planes per frame",
             "# icosphere level 8 = %d points; the CPP grid has two thirds of the picture's pixels" % len(ico),
             "# algorithmic bytes = what the gather asks for (a rate of requests, not an HBM rate)",
             "# median of %d rounds of %d calls" % (args.rounds, args.reps),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "%-40s %10s %10s %8s %13s" % ("case", "MB", "us", "GB/s", "min-max us")]
    for name, _, nbytes in cases:
        t = statistics.median(times[name])
        lines.append("%-40s %10.1f %10.1f %8.0f %6.1f-%6.1f"
                     % (name, nbytes / 1e6, t * 1e6, nbytes / t / 1e9, min(times[name]) * 1e6, max(times[name]) * 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
