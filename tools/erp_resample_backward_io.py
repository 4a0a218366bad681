"""The ordered backward of the sphere-aware resize (csrc/erp_resample_backward.hip) on one GPU, beside the forward on the
same shapes and the gradient torch's autograd makes of erp_resample.resize_torch on the device.

Times PCONV.erp_resample_backward_f32 (two launches, three planes per frame), PCONV.erp_resample_f32 (two launches) and
the backward pass of resize_torch (index_select and its scatter-add backward, tap by tap) at 4096x2048 -> 2048x1024 and
2048x1024 -> 4096x2048 with n = 8, and on the (2, 3, 512, 1024) training batch down to 256x512 and up to 1024x2048, with
device events (warm-up, then rounds that alternate the cases; the median of the rounds).  Counted bytes, forward and
backward alike: the tensor read, the intermediate picture written and read, the tensor written; against 8 TB/s.  The
torch gradient is timed as retain_graph backward calls on one graph, so its forward is not in the figure.

    python tools/erp_resample_backward_io.py [--rounds 10] [--out profiles/erp_resample_backward.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, erp_resample  # noqa: E402

PEAK = 8e12   # bytes / s of HBM
# (n, h, w, h2, w2)
SHAPES = [(8, 2048, 4096, 1024, 2048), (8, 1024, 2048, 2048, 4096), (2, 512, 1024, 256, 512), (2, 512, 1024, 1024, 2048)]


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
        raise SystemExit("erp_resample_backward_io: needs a GPU")
    dev = torch.device("cuda:0")
    cases = []
    for n, h, w, h2, w2 in SHAPES:
        x = torch.rand((n, 3, h, w), device=dev)
        g = torch.rand((n, 3, h2, w2), device=dev)
        out, gin = torch.empty_like(g), torch.empty_like(x)
        ws = torch.empty((4 * n * 3 * h * w2,), dtype=torch.uint8, device=dev)
        nbytes = 4 * (x.numel() + 2 * n * 3 * h * w2 + g.numel())
        size = "%dx%d->%dx%d n%d" % (w, h, w2, h2, n)
        cases.append(("backward " + size, lambda g=g, gin=gin, ws=ws, h=h, w=w: PCONV.erp_resample_backward_f32(g, h, w, gin, ws),
                      nbytes))
        cases.append(("forward  " + size, lambda x=x, out=out, ws=ws, h2=h2, w2=w2: PCONV.erp_resample_f32(x, h2, w2, False, out, ws),
                      nbytes))
        leaf = x.clone().requires_grad_()
        graph = erp_resample.resize_torch(leaf, h2, w2)

        def torch_grad(graph=graph, leaf=leaf, g=g):
            leaf.grad = None
            graph.backward(g, retain_graph=True)

        cases.append(("torch    " + size, torch_grad, nbytes))
        torch_grad()
        twin = erp_resample.resize_backward_torch(g[:1], h, w)
        same = torch.equal(PCONV.erp_resample_backward_f32(g[:1].contiguous(), h, w), twin)
        print("%s: kernels == twin on frame 0: %s; max |kernels - torch autograd| = %.3e"
              % (size, same, (PCONV.erp_resample_backward_f32(g, h, w) - leaf.grad).abs().max().item()), flush=True)
    for c in cases:   # warm-up: code objects loaded, tables and lists on the device, clocks up
        timed(c[1], 2)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], args.reps))
        print("round", r, flush=True)
    lines = ["# erp_resample backward: the two gather launches of pconv_erp_resample_backward_f32 (float32, three planes per "
             "frame),",
             "# beside the forward on the same shape and the backward pass torch's autograd makes of resize_torch on the device",
             "# counted bytes (all three rows): tensor read + 2 x intermediate + tensor written",
             "# median of %d rounds of %d calls; %% of %.0f TB/s" % (args.rounds, args.reps, PEAK / 1e12),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "%-40s %10s %10s %8s %7s %11s" % ("case", "MB", "us", "TB/s", "% peak", "min-max TB/s")]
    for name, _, nbytes in cases:
        t = statistics.median(times[name])
        lo, hi = nbytes / max(times[name]) / 1e12, nbytes / min(times[name]) / 1e12
        lines.append("%-40s %10.1f %10.1f %8.2f %7.1f %5.2f-%5.2f"
                     % (name, nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100.0 * nbytes / t / PEAK, lo, hi))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
