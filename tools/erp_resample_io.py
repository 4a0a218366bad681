"""The sphere-aware Lanczos-3 resize (csrc/erp_resample.hip) on one GPU, beside the PIL bicubic resize of check_img.

Times erp_resample.resize at 8192x4096 -> 4096x2048, 4096x2048 -> 8192x4096 and 5760x2880 -> 4096x2048 with n = 1 (three
planes each), and 8192x4096 -> 4096x2048 again with n = 8, with device events (warm-up, then rounds that alternate the
shapes; the median of the rounds).  Counted bytes = input read + intermediate picture written and read + output written,
against 8 TB/s.  check_img's PIL call (uint8, on the host: what --height/--width does) is timed at the same three
single-frame shapes.

    python tools/erp_resample_io.py [--rounds 10] [--out profiles/erp_resample.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, erp_resample, pseudo_codec  # noqa: E402

PEAK = 8e12   # bytes / s of HBM
SHAPES = [(1, 4096, 8192, 2048, 4096), (1, 2048, 4096, 4096, 8192), (1, 2880, 5760, 2048, 4096),
          (8, 4096, 8192, 2048, 4096)]


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
    ap.add_argument("--pil-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("erp_resample_io: needs a GPU")
    dev = torch.device("cuda:0")
    cases = []
    for n, h, w, h2, w2 in SHAPES:
        x = torch.rand((n, 3, h, w), device=dev)
        out = torch.empty((n, 3, h2, w2), device=dev)
        ws = torch.empty((4 * n * 3 * h * w2,), dtype=torch.uint8, device=dev)
        counted = 4 * (x.numel() + 2 * n * 3 * h * w2 + out.numel())
        name = "%dx%d -> %dx%d n%d" % (w, h, w2, h2, n)
        cases.append((name, lambda x=x, out=out, ws=ws, h2=h2, w2=w2: PCONV.erp_resample_f32(x, h2, w2, True, out, ws),
                      counted, erp_resample.taps(w, w2)[1].shape[1], erp_resample.taps(h, h2)[1].shape[1]))
    for c in cases:   # warm-up: code objects loaded, tables on the device, clocks up
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    lines = ["# erp_resample.resize, float32, three planes per frame, clamp on; counted bytes = input read + intermediate "
             "written and read + output written",
             "# median of %d rounds of %d calls (two kernels per call); %% of %.0f TB/s" % (args.rounds, args.reps, PEAK / 1e12),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "%-32s %4s %4s %10s %10s %8s %7s %11s" % ("shape", "Tx", "Ty", "MB", "us", "TB/s", "% peak", "min-max TB/s")]
    for name, _, nbytes, tx, ty in cases:
        t = statistics.median(times[name])
        lo, hi = nbytes / max(times[name]) / 1e12, nbytes / min(times[name]) / 1e12
        lines.append("%-32s %4d %4d %10.1f %10.1f %8.2f %7.1f %5.2f-%5.2f"
                     % (name, tx, ty, nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK, lo, hi))
    lines.append("# check_img (PIL bicubic, uint8 (h, w, 3), on this host's CPU; median of %d calls):" % args.pil_reps)
    g = np.random.default_rng(0)
    for n, h, w, h2, w2 in SHAPES[:3]:
        img = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ts = []
        for _ in range(args.pil_reps):
            t0 = time.perf_counter()
            pseudo_codec.check_img(img, h2, w2)
            ts.append(time.perf_counter() - t0)
        lines.append("#   %-30s %10.1f ms" % ("%dx%d -> %dx%d" % (w, h, w2, h2), statistics.median(ts) * 1e3))
        print("pil", w, h, flush=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
