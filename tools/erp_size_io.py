"""Frame I/O kernels of any-size panoramas (csrc/erp_size.hip) against today's frame kernels, on one GPU.

Times frames_u8_to_f32_erp, erp_pad_f32 and frames_f32_to_u8_crop at 5760x2880 (coded 5760x3072), n = 8, and
frames_u8_to_f32 / frames_f32_to_u8 at 4096x2048, n = 8, with device events (warm-up, then rounds that alternate the
kernels; the median of the rounds).  Counted bytes = bytes of the input tensor read + bytes of the output written.

    python tools/erp_size_io.py [--rounds 20] [--out profiles/erp_size_io.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, erp_size  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("erp_size_io: needs a GPU")
    dev = torch.device("cuda:0")
    n, (h, w) = 8, (2880, 5760)
    H, W, _ = erp_size.coded_size(h, w)
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    f32 = torch.rand(n, 3, h, w, generator=g).to(dev)
    coded = torch.empty((n, 3, H, W), device=dev)
    back = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    rec = torch.rand(n, 3, H, W, generator=g).to(dev)
    hb, wb = 2048, 4096
    u8b = torch.randint(0, 256, (n, hb, wb, 3), generator=g, dtype=torch.uint8).to(dev)
    f32b = torch.empty((n, 3, hb, wb), device=dev)
    backb = torch.empty_like(u8b)
    recb = torch.rand(n, 3, hb, wb, generator=g).to(dev)
    cases = [
        ("frames_u8_to_f32_erp_pad_kernel", "%dx%d -> %dx%d" % (w, h, W, H),
         lambda: PCONV.frames_u8_to_f32_erp(u8, coded), u8.numel() + 4 * coded.numel()),
        ("erp_pad_f32_kernel", "%dx%d -> %dx%d" % (w, h, W, H),
         lambda: PCONV.erp_pad_f32(f32, coded), 4 * f32.numel() + 4 * coded.numel()),
        ("frames_f32_to_u8_crop_kernel", "%dx%d -> %dx%d" % (W, H, w, h),
         lambda: PCONV.frames_f32_to_u8_crop(rec, h, w, back), 4 * 3 * n * h * w + back.numel()),
        ("frames_u8_to_f32_kernel", "%dx%d" % (wb, hb), lambda: PCONV.frames_u8_to_f32(u8b, f32b),
         u8b.numel() + 4 * f32b.numel()),
        ("frames_f32_to_u8_kernel", "%dx%d" % (wb, hb), lambda: PCONV.frames_f32_to_u8(recb, backb),
         4 * recb.numel() + backb.numel()),
    ]
    for _, _, fn, _ in cases:   # warm-up: code objects loaded, clocks up
        timed(fn, 3)
    times = {c[0]: [] for c in cases}
    for _ in range(args.rounds):
        for name, _, fn, _ in cases:
            times[name].append(timed(fn, args.reps))
    lines = ["# n = %d frames per launch; counted bytes = input read + output written; median of %d rounds of %d launches"
             % (n, args.rounds, args.reps), "# device: %s" % torch.cuda.get_device_name(dev),
             "%-34s %-24s %10s %10s %8s %8s" % ("kernel", "size", "MB", "us", "TB/s", "min-max")]
    rate = {}
    for name, size, _, nbytes in cases:
        t = statistics.median(times[name])
        lo, hi = nbytes / max(times[name]) / 1e12, nbytes / min(times[name]) / 1e12
        rate[name] = nbytes / t / 1e12
        lines.append("%-34s %-24s %10.1f %10.1f %8.2f %4.2f-%4.2f" % (name, size, nbytes / 1e6, t * 1e6, rate[name], lo, hi))
    ref = {"frames_u8_to_f32_erp_pad_kernel": "frames_u8_to_f32_kernel", "erp_pad_f32_kernel": "frames_u8_to_f32_kernel",
           "frames_f32_to_u8_crop_kernel": "frames_f32_to_u8_kernel"}
    lines.append("# time per counted byte relative to the existing frame kernel of the same direction:")
    for name, base in ref.items():
        lines.append("#   %-32s %.2fx %s  (target: >= 3.5 TB/s and <= 1.3x)" % (name, rate[base] / rate[name], base))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
