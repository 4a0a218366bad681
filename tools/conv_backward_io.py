"""The native convolution backward (csrc/conv_backward.hip, `train.py --conv native`) beside the vendor library's, on
one GPU.

1. Records the convolutions one training step of CMPNetV2MF(56, 192, 192) at batch 2 of 512x1024 sends to
   PCONV.tile_conv2d_backward (every TileConv2d layer and the GDN's 1x1 contraction) and groups them into layer
   classes (k, stride, cin -> cout, tile size, whether the data gradient is asked for).
2. Per class, times the data gradient, the weight gradient and the bias gradient of both forms with device events:
   native = PCONV.tile_conv2d_backward with one `need` flag set (workspace allocation, prepare / pack, the sum of the
   partials included), vendor = aten.convolution_backward with the matching output mask.  Warm-up, then rounds in
   which the forms alternate; the median of the rounds.  The weight-gradient call's executed TFLOP/s (the 96 x 128
   blocks and even-length runs the kernel really multiplies) stands against the 157.3 TFLOP/s fp32-MFMA peak.
3. Training steps per second of the --base stage's step (CMPNetV2M, batch 2, viewport MSE + 0.01 (1 - SSIM), Adam)
   with the switch off and on, the forms alternating.

    python tools/conv_backward_io.py [--rounds 10] [--out profiles/conv_backward.txt]
"""
import argparse
import collections
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, model_zoo_v2  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator import SSIM, MultiProject  # noqa: E402

NPART, N, H, W = 16, 2, 512, 1024
PEAK = 157.3

Layer = collections.namedtuple("Layer", "k s cin cout tn h w need_x")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def layer_classes(dev):
    """{Layer: calls per step} of one native training step of the whole model"""
    seen = collections.Counter()
    real = PCONV.tile_conv2d_backward

    def record(x, weight, gout, stride, need=(True, True, True), owner=None):
        cout, cin, k, _ = weight.shape
        seen[Layer(k, int(stride), cin, cout, x.shape[0], x.shape[2], x.shape[3], bool(need[0]))] += 1
        return real(x, weight, gout, stride, need, owner=owner)

    torch.manual_seed(3)
    model = model_zoo_v2.CMPNetV2MF(56, 192, 192, NPART, opt=True, init=False, device_id=0).to(dev).train()
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
    PCONV.tile_conv2d_backward = record
    try:
        with PCONV.native_conv_grad(True):
            y, ent_vec, mask = model(x)
            (torch.mean((x - y) ** 2) + torch.sum(ent_vec) / torch.sum(mask).item()).backward()
    finally:
        PCONV.tile_conv2d_backward = real
    torch.cuda.synchronize()
    return seen


def executed_flops(L):
    """multiply-adds x 2 the weight-gradient kernel really issues: whole 96 x 128 blocks, runs of even length"""
    ho, wo = (L.h - L.k) // L.s + 1, (L.w - L.k) // L.s + 1
    steps = sum(2 * ((min(64, wo - c0) + 1) // 2) for c0 in range(0, wo, 64)) * ho
    blocks = ((L.cout + 95) // 96) * ((L.cin * L.k * L.k + 127) // 128)
    return 2.0 * 96 * 128 * blocks * steps * L.tn


def forms(L, dev):
    """{(gradient, form): call} on seeded data of the layer's shape"""
    g = torch.Generator().manual_seed(5)
    ho, wo = (L.h - L.k) // L.s + 1, (L.w - L.k) // L.s + 1
    x = torch.randn(L.tn, L.cin, L.h, L.w, generator=g).to(dev)
    w = (torch.randn(L.cout, L.cin, L.k, L.k, generator=g) / (L.cin * L.k * L.k) ** 0.5).to(dev)
    gout = torch.randn(L.tn, L.cout, ho, wo, generator=g).to(dev)
    vendor = lambda mask: torch.ops.aten.convolution_backward(gout, x, w, [L.cout], [L.s, L.s], [0, 0], [1, 1], False,
                                                              [0, 0], 1, mask)
    native = lambda need: PCONV.tile_conv2d_backward(x, w, gout, L.s, need)
    out = {}
    for i, name in enumerate(("data", "weight", "bias")):
        if name == "data" and not L.need_x:
            continue
        mask = [j == i for j in range(3)]
        out[(name, "native")] = lambda mask=mask: native(tuple(mask))
        out[(name, "vendor")] = lambda mask=mask: vendor(mask)
    return out


def step_rate(dev, native, steps, state={}):
    """steps per second of the --base stage's training step"""
    if "model" not in state:
        torch.manual_seed(3)
        state["model"] = model_zoo_v2.CMPNetV2M(56, 192, 192, NPART, opt=True, init=False, device_id=0).to(dev).train()
        state["pr"] = (MultiProject(171, 256, 0.5, False, 0).to(dev), MultiProject(171, 256, 0.5, False, 0).to(dev))
        state["ssim"] = SSIM(11, 3).to(dev)
        state["x"] = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
        state["opt"] = torch.optim.Adam([p for k, p in state["model"].named_parameters() if k != "quant.count"], lr=1e-5)
    model, (pr1, pr2), ssim, x, opt = state["model"], state["pr"], state["ssim"], state["x"], state["opt"]
    with PCONV.native_conv_grad(native):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.zero_grad()
            py, px = pr1(model(x)), pr2(x)
            (torch.mean((px - py) * (px - py)) + 0.01 * (1 - ssim(px, py))).backward()
            opt.step()
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed window (0: skip the step rate)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_backward_io: needs a GPU")
    dev = torch.device("cuda:0")
    classes = layer_classes(dev)
    lines = ["native against vendor convolution backward, CMPNetV2MF(56, 192, 192), batch %d of %dx%d (%d tiles); "
             "median of %d rounds of %d calls, the forms alternating; us per call"
             % (N, H, W, N * NPART, args.rounds, args.reps),
             "%-34s %3s | %9s %9s | %9s %9s %7s %5s | %9s %9s"
             % ("layer class (tile h x w)", "n", "data nat", "vendor", "wgt nat", "vendor", "TF/s ex", "peak", "bias nat", "vendor")]
    total = collections.Counter()
    order = sorted(classes, key=lambda L: (-L.k, L.s, L.cin * L.cout, L.h * L.w))
    for L in order:
        todo = forms(L, dev)
        for fn in todo.values():
            timed(fn, 2)   # code objects loaded, the library's algorithm chosen
        t = {key: [] for key in todo}
        for _ in range(args.rounds):
            for key, fn in todo.items():
                t[key].append(timed(fn, args.reps))
        med = {key: statistics.median(v) for key, v in t.items()}
        for (name, form), v in med.items():
            total[(name, form, L.s)] += v * classes[L]
        tf = executed_flops(L) / med[("weight", "native")] * 1e-12
        us = lambda name, form: "%9.1f" % (med[(name, form)] * 1e6) if (name, form) in med else "%9s" % "-"
        lines.append("%-34s %3d | %s %s | %s %s %7.1f %4.0f%% | %s %s"
                     % ("%dx%d s%d %4d->%-4d %3dx%-4d" % (L.k, L.k, L.s, L.cin, L.cout, L.h, L.w), classes[L],
                        us("data", "native"), us("data", "vendor"), us("weight", "native"), us("weight", "vendor"), tf,
                        100 * tf / PEAK, us("bias", "native"), us("bias", "vendor")))
    lines.append("")
    for s in (1, 2):
        lines.append("per step, stride-%d layers: data gradient native %.2f ms / vendor %.2f ms%s; weight gradient %.2f / %.2f ms; "
                     "bias gradient %.2f / %.2f ms"
                     % (s, total[("data", "native", s)] * 1e3, total[("data", "vendor", s)] * 1e3,
                        " (carries the 4x of the zero-stuffed gradient)" if s == 2 else "",
                        total[("weight", "native", s)] * 1e3, total[("weight", "vendor", s)] * 1e3,
                        total[("bias", "native", s)] * 1e3, total[("bias", "vendor", s)] * 1e3))
    if args.steps:
        for native in (False, True):
            step_rate(dev, native, 2)   # warm-up of both forms
        r = {False: [], True: []}
        for _ in range(args.rounds):
            for native in (False, True):
                r[native].append(step_rate(dev, native, args.steps))
        v, n = statistics.median(r[False]), statistics.median(r[True])
        lines += ["", "--base stage training step (CMPNetV2M, batch %d of %dx%d, viewport MSE + 0.01 (1 - SSIM), Adam), "
                  "median of %d rounds of %d steps: --conv vendor %.2f steps/s, --conv native %.2f steps/s (native / vendor %.2f)"
                  % (N, H, W, args.rounds, args.steps, v, n, n / v)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
