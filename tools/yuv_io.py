"""The YUV 4:2:0 frame kernels (csrc/yuv.hip) against the uint8 RGB frame kernels of the same direction, on one GPU.

Times frames_yuv420_to_f32 and frames_f32_to_yuv420 for yuv420p, nv12 and yuv420p10le, and frames_u8_to_f32_erp /
frames_f32_to_u8_crop, at 4096x2048 (codable) and 5760x2880 (coded 5760x3072), n = 8, with device events (warm-up,
then rounds that alternate the kernels; the median of the rounds).  Counted bytes = bytes of the input read + bytes of
the output written; the input tensors of one size exceed the 256 MiB of the last-level cache together.

    python tools/yuv_io.py [--rounds 20] [--out profiles/yuv_io.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, erp_size, yuv  # noqa: E402

FORMATS = ["yuv420p", "nv12", "yuv420p10le"]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def cases_of(n, h, w, dev):
    """[(kernel, label, fn, counted bytes, direction)] of one frame size"""
    H, W, _ = erp_size.coded_size(h, w)
    g = torch.Generator().manual_seed(h)
    coded = torch.empty((n, 3, H, W), device=dev)
    rec = torch.rand(n, 3, H, W, generator=g).to(dev)
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    back = torch.empty_like(u8)
    size = "%dx%d" % (w, h)
    cases = [("frames_u8_to_f32_erp", size, lambda: PCONV.frames_u8_to_f32_erp(u8, coded), u8.numel() + 4 * coded.numel(), "in"),
             ("frames_f32_to_u8_crop", size, lambda: PCONV.frames_f32_to_u8_crop(rec, h, w, back),
              4 * 3 * n * h * w + back.numel(), "out")]
    for fmt in FORMATS:
        elems, sample = yuv.frame_elems(h, w), yuv.frame_bytes(h, w, fmt) // yuv.frame_elems(h, w)
        src = torch.randint(0, 1 << yuv.depth(fmt), (n, elems), generator=g, dtype=torch.int32).to(yuv.dtype(fmt)).to(dev)
        dst = torch.empty_like(src)
        cases.append(("frames_yuv420_to_f32 " + fmt, size, lambda src=src, fmt=fmt: PCONV.frames_yuv420_to_f32(src, h, w, fmt, out=coded),
                      sample * src.numel() + 4 * coded.numel(), "in"))
        cases.append(("frames_f32_to_yuv420 " + fmt, size, lambda dst=dst, fmt=fmt: PCONV.frames_f32_to_yuv420(rec, h, w, fmt, out=dst),
                      4 * 3 * n * h * w + sample * dst.numel(), "out"))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_io: needs a GPU")
    dev = torch.device("cuda:0")
    n = 8
    lines = ["# n = %d frames per launch; counted bytes = input read + output written; median of %d rounds of %d launches"
             % (n, args.rounds, args.reps), "# device: %s" % torch.cuda.get_device_name(dev),
             "%-36s %-12s %9s %9s %7s %10s %s" % ("kernel", "size", "MB", "us", "TB/s", "min-max", "time / u8 kernel")]
    for h, w in ((2048, 4096), (2880, 5760)):
        cases = cases_of(n, h, w, dev)
        for _, _, fn, _, _ in cases:   # warm-up: code objects loaded, clocks up
            timed(fn, 3)
        times = {c[0]: [] for c in cases}
        for _ in range(args.rounds):
            for name, _, fn, _, _ in cases:
                times[name].append(timed(fn, args.reps))
        med = {name: statistics.median(t) for name, t in times.items()}
        base = {"in": med["frames_u8_to_f32_erp"], "out": med["frames_f32_to_u8_crop"]}
        for name, size, _, nbytes, way in cases:
            lo, hi = nbytes / max(times[name]) / 1e12, nbytes / min(times[name]) / 1e12
            lines.append("%-36s %-12s %9.1f %9.1f %7.2f  %4.2f-%4.2f %.2fx" % (name, size, nbytes / 1e6, med[name] * 1e6,
                                                                             nbytes / med[name] / 1e12, lo, hi, med[name] / base[way]))
        del cases
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
