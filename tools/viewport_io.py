"""Rectilinear viewports of ERP frames (csrc/viewport.hip) on one GPU, beside the reference's 14 bilinear views and the torch twin.

Times eight 4096x2048 frames (three planes) rendered to the 14 paper views at 256x171 (viewport.plan: the source reduced
first, then ss = 4) and at 1024x683 (ss = 2, no prefilter): the map build, the prefilter, the 14 render launches alone and
Renderer.render as a whole; beside them MultiProject (ProjectsOp: one bilinear sample per pixel) on the same frames at
the same two view sizes, and viewport.render_torch on the GPU on the same maps.  Device events, a warm-up, then rounds
that alternate the cases; the median of the rounds.  Counted bytes of the render kernel: its loads as issued (36
four-byte source values per sample and plane, the 8-byte record per sample and plane) and its stores; what the caches
make of the overlap of neighbouring footprints is the point of the figure.  Against 8 TB/s.

    python tools/viewport_io.py [--rounds 5] [--out profiles/viewport.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, erp_resample, viewport  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator.ops import MultiProject  # noqa: E402

PEAK = 8e12   # bytes / s of HBM
N, C, H, W = 8, 3, 2048, 4096
SIZES = [(171, 256), (683, 1024)]


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2, help="calls per timed window (the twin: one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("viewport_io: needs a GPU")
    dev = torch.device("cuda:0")
    x = torch.rand((N, C, H, W), device=dev)
    cases, notes = [], []
    for vh, vw in SIZES:
        size = "%dx%d" % (vw, vh)
        views = viewport.paper_views((vh, vw))
        r = viewport.Renderer(H, W, views, (vh, vw), device=dev)
        h2, w2, ss = r.plans[0]
        assert all(p == r.plans[0] for p in r.plans)
        notes.append("# %s: plan = source %dx%d, ss = %d; a map is %.1f MB" % (size, w2, h2, ss, 8e-6 * vh * vw * ss * ss))
        out = torch.empty((N, len(views), C, vh, vw), device=dev)
        src = x if (h2, w2) == (H, W) else erp_resample.resize(x, h2, w2)
        samples = N * C * vh * vw * ss * ss * len(views)
        loads = samples * (36 * 4 + 8) + 4 * out.numel()
        q = torch.empty((vh * ss, vw * ss, 2), dtype=torch.int32, device=dev)
        cases.append(("maps %s (14 launches)" % size, 1,
                      lambda views=views, h2=h2, w2=w2, q=q: [PCONV.viewport_map(h2, w2, q.shape[0], q.shape[1], v, dev, q)
                                                               for v in views], 8 * q.numel() // 2 * len(views)))
        if (h2, w2) != (H, W):
            cases.append(("prefilter %dx%d->%dx%d" % (W, H, w2, h2), 1, lambda h2=h2, w2=w2: erp_resample.resize(x, h2, w2),
                          4 * (x.numel() + 2 * N * C * H * w2 + N * C * h2 * w2)))
        cases.append(("render %s ss%d (14 launches)" % (size, ss), 1,
                      lambda r=r, src=src, out=out, vh=vh, vw=vw: [PCONV.viewport_render_f32(src, q_, vh, vw, p[2], True, out, k)
                                                                    for k, (p, q_) in enumerate(zip(r.plans, r.maps))], loads))
        cases.append(("Renderer.render %s" % size, 1, lambda r=r, out=out: r.render(x, True, out), loads))
        mp = MultiProject(vh, vw, 0.5, False, 0).to(dev)
        cases.append(("MultiProject %s (bilinear)" % size, 1, lambda mp=mp: mp(x), 4 * (4 + 1) * N * C * vh * vw * len(views)))
        cases.append(("render_torch %s (GPU twin)" % size, 0,
                      lambda r=r, src=src, vh=vh, vw=vw: [viewport.render_torch(src, q_, vh, vw, p[2], True)
                                                          for p, q_ in zip(r.plans, r.maps)], loads))
    for c in cases:   # warm-up: code objects loaded, tables on the device, clocks up
        timed(c[2], 1)
    print("warm", flush=True)
    times = {c[0]: [] for c in cases}
    for rnd in range(args.rounds):
        for c in cases:
            times[c[0]].append(timed(c[2], args.reps if c[1] else 1))
        print("round", rnd, flush=True)
    lines = ["# viewport: %d frames of %dx%d, %d planes, to the 14 paper views (hfov 90 degrees, square pixels), clamp on" % (N, W, H, C),
             "# counted bytes: maps = maps written; prefilter = input + 2 x intermediate + output; render, Renderer.render and "
             "render_torch = the render kernel's",
             "#   loads as issued (36 x 4 B per sample and plane + the 8 B record) + the views written; MultiProject = 4 "
             "source values read + 1 written per pixel",
             "# Renderer.render = prefilter (where the plan has one) + the 14 render launches, the maps held by the renderer"]
    lines += notes
    lines += ["# median of %d rounds of %d calls (render_torch: 1); %% of %.0f TB/s" % (args.rounds, args.reps, PEAK / 1e12),
              "# device: %s" % torch.cuda.get_device_name(dev),
              "%-40s %10s %10s %8s %7s %11s" % ("case", "MB", "us", "TB/s", "% peak", "min-max TB/s")]
    for name, _, _, nbytes in cases:
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
