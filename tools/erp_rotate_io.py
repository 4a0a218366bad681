"""The sphere rotation of ERP frames (csrc/erp_rotate.hip) on one GPU, beside the sphere-aware resize at the same sizes.

Times the map build (PCONV.erp_rotation_map) and the sampler (PCONV.erp_remap_f32, three planes per frame, clamp on) at
4096x2048 with n = 8 and at 8192x4096 with n = 1, and erp_resample.resize (identity size: the same bytes in and out) at
the same two shapes, with device events (warm-up, then rounds that alternate the cases; the median of the rounds).
Counted bytes: the map build writes the map (8 bytes per pixel); the sampler reads the input, writes the output and reads
the map once per frame; the resize reads the input, writes and reads its intermediate picture and writes the output.
Against 8 TB/s.

    python tools/erp_rotate_io.py [--rounds 10] [--out profiles/erp_rotate.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, erp_rotate  # noqa: E402

PEAK = 8e12   # bytes / s of HBM
SHAPES = [(8, 2048, 4096), (1, 4096, 8192)]
ANGLES = (30, 20, 10)


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
        raise SystemExit("erp_rotate_io: needs a GPU")
    dev = torch.device("cuda:0")
    rot = erp_rotate.units(*ANGLES)
    cases = []
    for n, h, w in SHAPES:
        x = torch.rand((n, 3, h, w), device=dev)
        out = torch.empty_like(x)
        q = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
        ws = torch.empty((4 * n * 3 * h * w,), dtype=torch.uint8, device=dev)
        size = "%dx%d n%d" % (w, h, n)
        cases.append(("map " + size, lambda h=h, w=w, q=q: PCONV.erp_rotation_map(h, w, rot, False, dev, q), 8 * h * w))
        cases.append(("remap " + size, lambda x=x, q=q, out=out: PCONV.erp_remap_f32(x, q, True, out),
                      4 * 2 * x.numel() + 8 * n * h * w))
        cases.append(("resize " + size, lambda x=x, out=out, ws=ws, h=h, w=w: PCONV.erp_resample_f32(x, h, w, True, out, ws),
                      4 * 4 * x.numel()))
    for c in cases:   # warm-up: code objects loaded, tables on the device, clocks up (and the maps written)
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    lines = ["# erp_rotate: map build (fp64, one launch per size, rotation and direction) and sampler (float32, three planes "
             "per frame, clamp on),",
             "# beside erp_resample.resize at the same size in and out; rotation (%g, %g, %g) degrees" % ANGLES,
             "# counted bytes: map = map written; remap = input read + output written + map read once per frame; "
             "resize = input + 2 x intermediate + output",
             "# median of %d rounds of %d calls; %% of %.0f TB/s" % (args.rounds, args.reps, PEAK / 1e12),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "%-28s %10s %10s %8s %7s %11s" % ("case", "MB", "us", "TB/s", "% peak", "min-max TB/s")]
    for name, _, nbytes in cases:
        t = statistics.median(times[name])
        lo, hi = nbytes / max(times[name]) / 1e12, nbytes / min(times[name]) / 1e12
        lines.append("%-28s %10.1f %10.1f %8.2f %7.1f %5.2f-%5.2f"
                     % (name, nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK, lo, hi))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
