"""The ordered (atomic-free) backward kernels (csrc/backward_ordered.hip) beside the default float-atomic forms, on
one GPU, and whether a whole model then trains to the same bits twice.

1. Times SphereSliceOp / SphereUsliceOp / ProjectsOp / PseudoQuantOp .backward in both forms at the training shapes
   (batch 2, 512x1024; slice and uslice at 3 and 192 channels; 14 views of 171x256; the quantiser at 192 channels)
   with device events: warm-up, then rounds that alternate the two forms; the median of the rounds.
2. Runs CMPNetV2MF(56, 192, 192) for 5 Adam steps twice from one seed under what `train.py --deterministic` sets
   (train.deterministic_mode) and reports whether the parameter checksums and every parameter are bit-identical; if
   not, the first tensor that differs.  The convolution backward is the vendor library's: this part is an
   observation, not a guarantee of this project.

    python tools/backward_ordered_io.py [--rounds 10] [--out profiles/backward_ordered.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, model_zoo_v2, train  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator import MultiProject  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator.base import set_weight  # noqa: E402

NPART, N, H, W = 16, 2, 512, 1024


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def cases(dev):
    """(label, backward call) per op and shape; the forward calls that size the ops are made here"""
    weight = set_weight(NPART, True)
    g = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    out = []
    for c in (3, 192):
        sl = PCONV.SphereSliceOp(NPART, 0, 0, weight, 0, False)
        grad = torch.randn_like(sl.forward(rnd(N, c, H, W))[0])
        out.append(("slice c%d" % c, lambda sl=sl, grad=grad: sl.backward(grad)))
        us = PCONV.SphereUsliceOp(NPART, 0, 0, weight, 0, False)
        grad = torch.randn_like(us.forward(rnd(N * NPART, c, H // NPART, W))[0])
        out.append(("uslice c%d" % c, lambda us=us, grad=grad: us.backward(grad)))
    pr = PCONV.ProjectsOp(171, 256, MultiProject.THETAS, MultiProject.PHIS, 0.5, False, 0, False)
    grad = torch.randn_like(pr.forward(rnd(N, 3, H, W))[0])
    out.append(("projects 14 x 171x256", lambda pr=pr, grad=grad: pr.backward(grad)))
    ctx = PCONV.PseudoContextOp(NPART, 20, weight, 0, False)
    qt = PCONV.PseudoQuantOp(192, 8, NPART, 0.9, 100, 2, 0.1, ctx.addr(), 0, False)
    x = (torch.rand(N * NPART, 192, H // 256, W // 16, generator=g) * 1.2 - 0.1).to(dev)
    qw = torch.zeros(192, 8)
    qw[:, 0], qw[:, 1:] = 1. / 9, -2.1972246
    val = qt.forward(x, qw.to(dev), torch.zeros(192, 8, device=dev), False)[0]
    grads = [torch.randn_like(x), torch.randn_like(x)]
    out.append(("quant c192", lambda qt=qt, grads=grads, x=x, val=val: qt.backward(grads, x, val)))
    return out


def model_run(dev, steps):
    """parameters of CMPNetV2MF(56, 192, 192) after `steps` Adam steps on one seeded batch"""
    torch.manual_seed(3)
    model = model_zoo_v2.CMPNetV2MF(56, 192, 192, NPART, opt=True, init=False, device_id=0).to(dev).train()
    pr1, pr2 = MultiProject(171, 256, 0.5, False, 0).to(dev), MultiProject(171, 256, 0.5, False, 0).to(dev)
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
    opt = torch.optim.Adam([p for k, p in model.named_parameters() if k != 'quant.count'], lr=1e-4)
    for _ in range(steps):
        opt.zero_grad()
        y, ent_vec, mask = model(x)
        py, px = pr1(y), pr2(x)
        loss = torch.mean((px - py) * (px - py)) + torch.sum(ent_vec) / torch.sum(mask).item()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return [(k, p.detach().clone()) for k, p in model.named_parameters()], loss.item()


def checksum(params):
    return sum(p.double().abs().sum().item() for _, p in params)   # the figure train.py logs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=5, help="Adam steps of the whole-model runs (0: skip them)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("backward_ordered_io: needs a GPU")
    dev = torch.device("cuda:0")
    lines = ["ordered against atomic backward, batch %d, %dx%d; median of %d rounds of %d launches, the forms alternating"
             % (N, H, W, args.rounds, args.reps), "%-24s %12s %12s %8s" % ("op", "atomic us", "ordered us", "ratio")]
    todo = cases(dev)
    for _, fn in todo:   # warm-up of both forms: code objects loaded, reverse tables built and on the device
        for on in (False, True):
            with PCONV.ordered_backward(on):
                timed(fn, 2)
    for label, fn in todo:
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                with PCONV.ordered_backward(on):
                    t[on].append(timed(fn, args.reps))
        a, o = statistics.median(t[False]), statistics.median(t[True])
        lines.append("%-24s %12.1f %12.1f %8.2f" % (label, a * 1e6, o * 1e6, o / a))
    if args.steps:
        lines.append("")
        for name, mode in (("--deterministic", train.deterministic_mode), ("default (atomic)", PCONV.ordered_backward)):
            with mode():
                (pa, la), (pb, lb) = model_run(dev, args.steps), model_run(dev, args.steps)
            differ = [k for (k, a), (_, b) in zip(pa, pb) if not torch.equal(a, b)]
            lines.append("CMPNetV2MF(56, 192, 192), %d Adam steps, twice from one seed, %s: checksums %.17g / %.17g, "
                         "last losses %.9g / %.9g, %d of %d parameter tensors differ%s"
                         % (args.steps, name, checksum(pa), checksum(pb), la, lb, len(differ), len(pa),
                            "" if not differ else " (first: %s)" % differ[0]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
