"""Cubemap panoramas (csrc/cube.hip, cube.py) on one GPU: eight frames 4096x2048 <-> cube pictures of a = 1024.

Times cube.from_erp (one render launch over the cached map) and cube.to_erp (the face continuation plus one render
launch over the cached map), both kinds, three planes per frame, clamp on, layout "faces", with device events (warm-up,
which also builds and caches the maps and the pad table; then rounds that alternate the cases; the median of the rounds).
The maps and the pad kernel get rows of their own.  Counted bytes: a conversion reads its input and writes its output
once (what the renderer's 36 taps make of the caches is not counted); the pad reads the faces and writes the padded
stack; a map build writes the map.  Against 8 TB/s.  The figures are measured against nothing: reported, not gated.

    python tools/cube_io.py [--rounds 10] [--out FILE]      (profiles/cube.txt holds the table as its last block)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, cube  # noqa: E402

PEAK = 8e12   # bytes / s of HBM
N, H, W, A = 8, 2048, 4096, 1024


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
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cube_io: needs a GPU")
    dev = torch.device("cuda:0")
    x = torch.rand((N, 3, H, W), device=dev)
    y = torch.rand((N, 3, 6 * A, A), device=dev)
    padded = 4 * N * 3 * 6 * (A + 6) ** 2
    cases = []
    for kind in ("cmp", "eac"):
        size = "%s %dx%d a%d n%d" % (kind, W, H, A, N)
        cases.append(("from_erp " + size, lambda kind=kind: cube.from_erp(x, A, kind, clamp=True, layout="faces"),
                      4 * (x.numel() + y.numel())))
        cases.append(("to_erp " + size, lambda kind=kind: cube.to_erp(y, (H, W), kind, clamp=True, layout="faces"),
                      4 * (x.numel() + y.numel()) + 2 * padded))
        cases.append(("pad " + size, lambda kind=kind: cube.pad(y, kind), 4 * y.numel() + padded))
        q1 = torch.empty((6 * A, A, 2), dtype=torch.int32, device=dev)
        q2 = torch.empty((H, W, 2), dtype=torch.int32, device=dev)
        cases.append(("from_erp map " + size, lambda kind=kind, q=q1: PCONV.cube_from_erp_map(kind, A, 1, H, W, dev, q), 8 * 6 * A * A))
        cases.append(("to_erp map " + size, lambda kind=kind, q=q2: PCONV.cube_to_erp_map(kind, A, H, W, 1, dev, q), 8 * H * W))
    for c in cases:   # warm-up: code objects loaded, maps and tables built and cached, clocks up
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    lines = ["# cube: from_erp (one render launch) and to_erp (face continuation + one render launch), float32, three planes per "
             "frame, clamp on, ss = 1,",
             "# maps and pad table cached; the pad kernel and the two map kernels (fp64) on rows of their own",
             "# counted bytes: input read + output written (to_erp: + the padded stack written and read); pad = faces + "
             "padded stack; map = map written",
             "# median of %d rounds of %d calls; %% of %.0f TB/s" % (args.rounds, args.reps, PEAK / 1e12),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "%-36s %10s %10s %8s %7s %11s" % ("case", "MB", "us", "TB/s", "% peak", "min-max TB/s")]
    for name, _, nbytes in cases:
        t = statistics.median(times[name])
        lo, hi = nbytes / max(times[name]) / 1e12, nbytes / min(times[name]) / 1e12
        lines.append("%-36s %10.1f %10.1f %8.2f %7.1f %5.2f-%5.2f"
                     % (name, nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK, lo, hi))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
