"""The ordered backward of the viewport renderer (csrc/remap_backward.hip) and train.py's --loss vp on one GPU.

For (2, 3, h, w) batches at 512 x 1024 and at 1024 x 2048, the 14 paper views at a quarter of the width (256 x 171, 512 x
341):
  backward ss1 / plan   the 14 pconv_remap_backward_f32 launches alone (gradient of the view stack -> gradient of the
                        frames, accumulating from the second view on), lists built beforehand; with ss = 1, and with
                        the supersampling viewport.plan gives (what --loss vp trains with)
  render+backward       Renderer.render under autograd and .backward(g), ss = 1
  torch autograd        the same composed from torch: autograd through erp_rotate.sample_torch on the GPU, ss = 1
  loss vp               viewport.loss_terms forward + backward, reconstruction -> its gradient, as train.py builds it
  loss viewport, ws     the two losses of tools/ws_loss_probe.py on the same batch, in the same session
  step rate             training steps per second of the full-model step (CMPNetV2MF(56, 192, 192), batch 2 of 512 x
                        1024, the loss through train.forward_losses, Adam, --conv vendor) under --loss viewport, vp
                        and ws, alternating in one process
  lists                 the one-off build of a renderer's reverse lists: host milliseconds (map copied to the host,
                        counting sort, upload) and bytes
Device events on the launch stream, a warm-up, then rounds that alternate the cases; the median of the rounds.

    python tools/viewport_backward_probe.py [--rounds 7] [--out profiles/viewport_backward.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, model_zoo_v2, sphere_metrics, train, viewport  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator import MultiProject, SSIM  # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def step_rates(dev, rounds, steps):
    """{loss: median steps per second} of the full-model training step, the losses alternating"""
    torch.manual_seed(3)
    model = model_zoo_v2.CMPNetV2MF(56, 192, 192, 16, opt=True, init=False, device_id=0).to(dev).train()
    x = torch.rand(2, 3, 512, 1024, generator=torch.Generator().manual_seed(4)).to(dev)
    opt = torch.optim.Adam([p for k, p in model.named_parameters() if k != "quant.count"], lr=1e-5)
    pr = [MultiProject(171, 256, 0.5, False, 0).to(dev) for _ in range(2)]
    losses = {name: train.build_parser().parse_args(["--loss", name]) for name in ("viewport", "vp", "ws")}
    sims = {name: train.make_sim_func(a, dev) for name, a in losses.items()}
    rates = {name: [] for name in losses}
    for rnd in range(rounds + 1):   # round 0 warms up
        for name, a in losses.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                opt.zero_grad()
                mse, ssim, rate = train.forward_losses(a, model, x, pr[0], pr[1], sims[name])
                (mse + 0.01 * (1 - ssim) + rate).backward()
                opt.step()
            torch.cuda.synchronize()
            if rnd:
                rates[name].append(steps / (time.perf_counter() - t0))
    return {name: statistics.median(v) for name, v in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window (torch autograd: one)")
    ap.add_argument("--steps", type=int, default=3, help="training steps per timed window (0: skip the step rate)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("viewport_backward_probe: needs a GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    lines = ["# device: %s; median of %d rounds of %d calls (torch autograd: 1), min and max of the rounds beside it"
             % (torch.cuda.get_device_name(dev), args.rounds, args.reps)]
    for h, w in ((512, 1024), (1024, 2048)):
        vw = w // 4
        vh = (2 * vw + 1) // 3
        x = torch.rand(2, 3, h, w, generator=gen).to(dev)
        y = (x + 0.05 * torch.randn(x.shape, generator=gen).to(dev)).requires_grad_()
        views = viewport.paper_views((vh, vw))
        r1 = viewport.Renderer(h, w, views, (vh, vw), ss=1, device=dev)
        rp = viewport.Renderer(h, w, views, (vh, vw), device=dev)
        build = {}
        for name, r in (("ss1", r1), ("plan", rp)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(len(views)):
                r.lists(k)
            torch.cuda.synchronize()
            build[name] = (time.perf_counter() - t0, sum(4 * (a.numel() + b.numel()) for a, b in r._lists))
        g = torch.randn(2, len(views), 3, vh, vw, generator=gen).to(dev)
        gin = torch.empty_like(x)

        def launches(r):
            for k, (p, q) in enumerate(zip(r.plans, r.maps)):
                PCONV.remap_backward_f32(g, q, r.lists(k), h, w, vh, vw, p[2], gin, k, k > 0)

        def render_backward():
            y.grad = None
            r1.render(y).backward(g)

        def torch_autograd():
            y.grad = None
            torch.stack([viewport.render_torch(y, q, vh, vw, 1) for q in r1.maps], 1).backward(g)

        def loss_vp():
            y.grad = None
            terms = viewport.loss_terms(rp, x, y)
            (terms[:, 0].mean() + 0.1 * (1 - terms[:, 1].mean())).backward()

        pr1, pr2 = MultiProject(171, 256, 0.5, False, 0).to(dev), MultiProject(171, 256, 0.5, False, 0).to(dev)
        sim = SSIM(11, 3).to(dev)

        def loss_viewport():
            y.grad = None
            py, px = pr1(y), pr2(x)
            (torch.mean((px - py) * (px - py)) + 0.1 * (1 - sim(px, py))).backward()

        def loss_ws():
            y.grad = None
            terms = sphere_metrics.loss_terms(x, y)
            (terms[:, 0].mean() + 0.1 * (1 - terms[:, 1].mean())).backward()

        cases = [("backward ss1 (14 launches)", 1, lambda: launches(r1)),
                 ("backward plan ss%s (14 launches)" % (rp.ss,), 1, lambda: launches(rp)),
                 ("render+backward ss1 (Renderer)", 1, render_backward),
                 ("torch autograd ss1 (sample_torch)", 0, torch_autograd),
                 ("loss vp (ss%s) fwd+bwd" % (rp.ss,), 1, loss_vp),
                 ("loss viewport (MultiProject 256x171)", 1, loss_viewport),
                 ("loss ws fwd+bwd", 1, loss_ws)]
        for c in cases:
            timed(c[2], 1)
        times = {c[0]: [] for c in cases}
        for rnd in range(args.rounds):
            for c in cases:
                times[c[0]].append(timed(c[2], args.reps if c[1] else 1))
        print("measured", h, w, flush=True)
        lists = r1.lists(0)[0]
        empty = float((lists[1:] == lists[:-1]).double().mean())
        lines += ["# (2, 3, %d, %d), 14 views of %dx%d; plan: ss = %s; view 0 at ss 1: %.1f%% of the source pixels have an empty "
                  "list, the longest list has %d entries" % (h, w, vw, vh, rp.ss, 100 * empty, int((lists[1:] - lists[:-1]).max())),
                  "%-40s %10s %10s %10s" % ("case", "median us", "min us", "max us")]
        for name, _, _ in cases:
            t = times[name]
            lines.append("%-40s %10.1f %10.1f %10.1f" % (name, statistics.median(t) * 1e6, min(t) * 1e6, max(t) * 1e6))
        for name in ("ss1", "plan"):
            lines.append("lists %-4s: 14 views built in %.1f ms on the host (copy, sort, upload), %.1f MB held"
                         % (name, build[name][0] * 1e3, build[name][1] / 1e6))
    if args.steps:
        torch.cuda.empty_cache()
        m = step_rates(dev, 5, args.steps)
        lines.append("full-model training step (CMPNetV2MF(56, 192, 192), batch 2 of 512x1024, mse + 0.01 (1 - ssim) + rate, Adam, "
                     "--conv vendor), median of 5 rounds of %d steps: --loss viewport %.2f steps/s, vp %.2f steps/s, ws %.2f steps/s "
                     "(vp / viewport %.3f)" % (args.steps, m["viewport"], m["vp"], m["ws"], m["vp"] / m["viewport"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
