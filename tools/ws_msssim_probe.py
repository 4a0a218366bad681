"""WS-MS-SSIM on one GPU: the kernels of csrc/sphere_metrics.hip over five scales against the same kernels over one scale
and a torch composition.

  forward   PCONV.ws_msssim_device (five ms_forward_kernel launches that also write the pyramid, one closing launch)
            against PCONV.ws_metrics_device (ms_forward_kernel<T, 1, 1>, one launch, and its closing launch) on the
            same frames, at n = 8 and n = 1 frames of 4096 x 2048 x 3, and against the definition composed from torch on the device
            (sphere_metrics.ms_scales_torch in float32: pooling by strided adds, the window as shifted sums)
  backward  PCONV.ws_msssim_backward (five gather launches, coarse to fine) against PCONV.ws_metrics_backward
  loss      sphere_metrics.ms_loss_terms forward + .backward() against sphere_metrics.loss_terms, (2, 3, 512, 1024)

Timed with device events on the launch stream: warm-up of every shape, then rounds that alternate the candidates,
median of the rounds.  Outputs are allocated inside the timed calls, as a user's call does.

    python tools/ws_msssim_probe.py [--rounds 10] [--out profiles/ws_msssim.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, sphere_metrics  # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def alternate(fns, rounds, reps):
    """median, min and max seconds per call of each candidate, the candidates alternating round by round"""
    for fn in fns:
        timed(fn, 2)
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(timed(fn, reps))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def table(title, names, stats):
    lines = [title, "%-22s %12s %12s %12s %8s" % ("call", "median us", "min us", "max us", "ratio")]
    for name, (med, lo, hi) in zip(names, stats):
        lines.append("%-22s %12.1f %12.1f %12.1f %8.2f" % (name, med * 1e6, lo * 1e6, hi * 1e6, med / stats[0][0]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--torch-rounds", type=int, default=3, help="rounds of the torch composition (one call each)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ws_msssim_probe: needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    lines = ["# WS-MS-SSIM: median of %d rounds of %d calls, candidates alternating; ratio = over the first row"
             % (args.rounds, args.reps), "# device: %s" % torch.cuda.get_device_name(dev)]
    c, h, w = 3, 2048, 4096
    for n in (8, 1):
        x = torch.rand(n, c, h, w, generator=g).to(dev)
        y = x + 0.05 * torch.randn(n, c, h, w, device=dev)
        single = lambda: PCONV.ws_metrics_device(x, y)
        multi = lambda: PCONV.ws_msssim_device(x, y)
        got = PCONV.ws_msssim(x, y)[0]
        lines += table("# forward, n = %d frames of %d x %d x %d float32" % (n, w, h, c),
                       ["ws_metrics (1 scale)", "ws_msssim (5 scales)"], alternate([single, multi], args.rounds, args.reps))

        def composed():
            with torch.no_grad():
                return sphere_metrics.ms_product(sphere_metrics.ms_scales_torch(x, y, "ws", torch.float32).double())

        want = composed().cpu()
        st = alternate([multi, composed], args.torch_rounds, 1)
        lines += table("# the same frames: the kernels against the definition composed from torch (float32, %d rounds of 1 call)"
                       % args.torch_rounds, ["ws_msssim (5 scales)", "torch composition"], st)
        lines.append("# largest |WS-MS-SSIM kernels - torch composition| = %.3g" % (got[:, 6] - want).abs().max().item())
        gout = torch.ones((n, 2), dtype=torch.float64, device=dev)
        values, workspace = PCONV.ws_msssim_device(x, y)
        back1 = lambda: PCONV.ws_metrics_backward(x, y, gout)
        back5 = lambda: PCONV.ws_msssim_backward(x, y, workspace, values, gout)
        lines += table("# backward, n = %d frames of %d x %d x %d float32" % (n, w, h, c),
                       ["ws_metrics_backward", "ws_msssim_backward"], alternate([back1, back5], args.rounds, args.reps))
        del x, y, values, workspace
    x = torch.rand(2, 3, 512, 1024, generator=g).to(dev)
    y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).requires_grad_()

    def loss(entry):
        def run():
            y.grad = None
            terms = entry(x, y)
            (terms[:, 0].mean() + 0.1 * (1 - terms[:, 1].mean())).backward()
        return run

    lines += table("# loss forward + backward, reconstruction -> its gradient, (2, 3, 512, 1024)",
                   ["loss_terms", "ms_loss_terms"],
                   alternate([loss(sphere_metrics.loss_terms), loss(sphere_metrics.ms_loss_terms)], args.rounds, 5))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
