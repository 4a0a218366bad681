"""The two training losses on one GPU: forward + backward from the reconstruction to its gradient.

  ws        sphere_metrics.loss_terms (the forward kernel of csrc/sphere_metrics.hip), the batch means of WS-MSE and
            WS-SSIM, .backward() (ms_backward_kernel<1, 1, 0>: one gather launch, no atomics)
  viewport  the paper's loss as train.py builds it: two MultiProject(171, 256, 0.5) ops (14 views each), the MSE over
            the views, SSIM(11, 3) (pytorch_ssim: five MIOpen 11 x 11 convolutions a call), .backward() (the
            convolutions' backward and ProjectsOp.backward, a scatter with float atomics)

Both on a (2, 3, 512, 1024) batch, timed with device events on the launch stream: warm-up, then rounds that alternate
the two, median of the rounds.  The loss is mse + 0.1·(1 - ssim) in both.  The backward kernel alone is also timed at
n = 8 frames of 4096 x 2048 (bytes = x and y read, the gradient written).

    python tools/ws_loss_probe.py [--rounds 10] [--out profiles/ws_loss.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, sphere_metrics  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator import MultiProject, SSIM  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ws_loss_probe: needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 512, 1024, generator=g).to(dev)
    y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).requires_grad_()
    pr1, pr2 = MultiProject(171, 256, 0.5, False, 0).to(dev), MultiProject(171, 256, 0.5, False, 0).to(dev)
    sim = SSIM(11, 3).to(dev)

    def ws():
        y.grad = None
        terms = sphere_metrics.loss_terms(x, y)
        (terms[:, 0].mean() + 0.1 * (1 - terms[:, 1].mean())).backward()

    def viewport():
        y.grad = None
        py, px = pr1(y), pr2(x)
        (torch.mean((px - py) * (px - py)) + 0.1 * (1 - sim(px, py))).backward()

    for fn in (ws, viewport):
        timed(fn, 3)
    tw, tv = [], []
    for _ in range(args.rounds):
        tw.append(timed(ws, args.reps))
        tv.append(timed(viewport, args.reps))
    a, b = statistics.median(tw), statistics.median(tv)
    lines = ["# loss forward + backward, reconstruction -> its gradient, (2, 3, 512, 1024); median of %d rounds of %d calls"
             % (args.rounds, args.reps), "# device: %s" % torch.cuda.get_device_name(dev),
             "%-10s %10s %10s %10s" % ("loss", "median us", "min us", "max us"),
             "%-10s %10.1f %10.1f %10.1f" % ("ws", a * 1e6, min(tw) * 1e6, max(tw) * 1e6),
             "%-10s %10.1f %10.1f %10.1f" % ("viewport", b * 1e6, min(tv) * 1e6, max(tv) * 1e6),
             "viewport / ws = %.2f" % (b / a)]
    del pr1, pr2, sim
    # the kernels alone at n = 8, 4096 x 2048
    n, c, h, w = 8, 3, 2048, 4096
    xb = torch.rand(n, c, h, w, generator=g).to(dev)
    yb = xb + 0.05 * torch.randn(n, c, h, w, device=dev)
    gout = torch.ones((n, 2), dtype=torch.float64, device=dev)
    fwd = lambda: PCONV.ws_metrics_device(xb, yb)
    bwd = lambda: PCONV.ws_metrics_backward(xb, yb, gout)
    for fn in (fwd, bwd):
        timed(fn, 2)
    tf, tb = [], []
    for _ in range(args.rounds):
        tf.append(timed(fwd, 3))
        tb.append(timed(bwd, 3))
    fbytes, bbytes = 8.0 * xb.numel(), 12.0 * xb.numel()
    a, b = statistics.median(tf), statistics.median(tb)
    lines += ["# the kernels alone, n = 8 frames of 4096 x 2048 x 3 float32 (the output allocated inside the timed call)",
              "%-10s %10s %10s %8s" % ("kernel", "median us", "MB moved", "TB/s"),
              "%-10s %10.1f %10.1f %8.2f" % ("forward", a * 1e6, fbytes / 1e6, fbytes / a / 1e12),
              "%-10s %10.1f %10.1f %8.2f" % ("backward", b * 1e6, bbytes / 1e6, bbytes / b / 1e12)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
