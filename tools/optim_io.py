"""The native optimiser step (csrc/optim.hip, optim.Adam, `train.py --optim native`) beside torch's, on one GPU.

1. On the parameter list of CMPNetV2MF(56, 192, 192) (all parameters but the quantiser's histogram), with gradients
   and gradient accumulators of seeded noise: the native step -- optim.Adam.step(acc, clip 0.1): table upload, squared
   norm, closing launch, update -- against AccGrad.copy_back + clip_grad_norm_ + torch.optim.Adam.step.  Device events
   around one step, warm-up, then rounds in which the two forms alternate; the median of the rounds.  The native
   path's achieved TB/s stands against its algorithmic 44 bytes per element: 8 read by the norm pass (grad, acc), 20
   read (p, grad, acc, m, v) and 16 written (p, m, v, acc) by the update.  The three launches are also timed alone,
   on a table built once: the whole step carries the host's part (checks, bias corrections, table and upload).
2. Training steps per second of the full model's step (batch 2 of 512x1024, MSE + rate, an optimiser step on every
   batch) with each optimiser, the forms alternating.

    python tools/optim_io.py [--rounds 10] [--out profiles/optim_step.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, model_zoo_v2, optim  # noqa: E402

NPART, N, H, W = 16, 2, 512, 1024
CLIP = 0.1
BYTES_PER_ELEMENT = 44


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


class Form(object):
    """one optimiser over its own copy of the model, and what a step of it is"""

    def __init__(self, native, dev):
        torch.manual_seed(3)
        self.model = model_zoo_v2.CMPNetV2MF(56, 192, 192, NPART, opt=True, init=False, device_id=0).to(dev).train()
        self.params = [p for k, p in self.model.named_parameters() if k != "quant.count"]
        self.native = native
        self.opt = (optim.Adam if native else torch.optim.Adam)(self.params, lr=1e-5)
        self.acc = model_zoo_v2.AccGrad(self.params)
        self.x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)

    def fill(self):
        """fresh gradients and accumulators (outside the timed window; new tensors, as after zero_grad())"""
        g = torch.Generator(device=self.x.device).manual_seed(5)
        for p, a in zip(self.params, self.acc.acc_grad):
            p.grad = torch.randn(p.shape, generator=g, device=p.device) * 1e-3
            a.copy_(torch.randn(p.shape, generator=g, device=p.device) * 1e-3)

    def step(self):
        if self.native:
            self.opt.step(acc=self.acc.acc_grad, clip=CLIP)
        else:
            self.acc.copy_back(self.params)
            torch.nn.utils.clip_grad_norm_(self.params, CLIP)
            self.opt.step()

    def train_rate(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.opt.zero_grad()
            y, ent_vec, mask = self.model(self.x)
            (torch.mean((self.x - y) ** 2) + torch.sum(ent_vec) / torch.sum(mask).item()).backward()
            self.step()
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3, help="training steps per timed window (0: skip the step rate)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_io: needs a GPU")
    dev = torch.device("cuda:0")
    forms = {"native": Form(True, dev), "torch": Form(False, dev)}
    elements = sum(p.numel() for p in forms["native"].params)
    t = {k: [] for k in forms}
    for rnd in range(2 + args.rounds):   # two warm-up rounds
        for k, f in forms.items():
            f.fill()
            torch.cuda.synchronize()
            dt = timed(f.step)
            if rnd >= 2:
                t[k].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    # the three launches alone, on a table built once: what the kernels do with the bytes, without the host's part
    # (the checks of 410 tensors, the bias corrections, the table and its upload)
    f = forms["native"]
    f.fill()
    items = [(p, p.grad, a, f.opt.state[p]["exp_avg"], f.opt.state[p]["exp_avg_sq"],
              optim._scalars(1e-5, 0.9, 0.999, 1e-8, 10.0)) for p, a in zip(f.params, f.acc.acc_grad)]
    records, segments = f.opt._tables(PCONV, items, dev)
    launches = lambda: PCONV.optim_step(records, segments, CLIP, dev)
    timed(launches)
    med["launches"] = statistics.median(timed(launches) for _ in range(args.rounds))
    lines = ["optimiser step over the %d tensors (%d elements) of CMPNetV2MF(56, 192, 192): accumulated gradient, global norm, "
             "clip %.1f, Adam; median of %d rounds of one step, the forms alternating"
             % (len(forms["native"].params), elements, CLIP, args.rounds),
             "native (optim.Adam.step(acc, clip): table upload + 3 launches)   %8.1f us   %.3f TB/s of the algorithmic %d B/element"
             % (med["native"] * 1e6, BYTES_PER_ELEMENT * elements / med["native"] * 1e-12, BYTES_PER_ELEMENT),
             "torch  (AccGrad.copy_back + clip_grad_norm_ + Adam.step)         %8.1f us   (native / torch %.2f)"
             % (med["torch"] * 1e6, med["native"] / med["torch"]),
             "the native step's 3 launches alone (%d segments, table built once) %8.1f us   %.3f TB/s"
             % (segments.nsegment, med["launches"] * 1e6, BYTES_PER_ELEMENT * elements / med["launches"] * 1e-12)]
    if args.steps:
        for f in forms.values():
            f.train_rate(1)
        r = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                r[k].append(f.train_rate(args.steps))
        rn, rt = statistics.median(r["native"]), statistics.median(r["torch"])
        lines += ["", "full-model training step (CMPNetV2MF, batch %d of %dx%d, MSE + rate, an optimiser step per batch), median of "
                  "%d rounds of %d steps: --optim torch %.2f steps/s, --optim native %.2f steps/s (native / torch %.3f)"
                  % (N, H, W, args.rounds, args.steps, rt, rn, rn / rt)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
