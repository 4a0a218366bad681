"""GPU probe: the wide entropy nets (valid_dim 112 / 192: 28 / 48 groups) beside the 56-channel one, vector kernel
(PCONV_EE_BULK=valu) against the matrix-core encoder.  Output for profiles/wide_models.txt.

  python tools/wide_models_probe.py layers [reps]
      one 4096 x 2048 frame (symbol planes 16 x 512, 3 weight sets per launch) encoded in ONE step range per call at
      14 / 28 / 48 groups in both modes -- run it under `rocprofv3 --kernel-trace --stats` for the time per launch of
      each bulk kernel; the streams of the two modes are compared here
  python tools/wide_models_probe.py summarise DIR
      per-launch table of the bulk kernels from the *kernel_stats.csv that rocprofv3 wrote under DIR
  python tools/wide_models_probe.py codec [steps] [H W]
      encode + decode host to host, 8 frames per call (CodecEngine + FramePipe: the step of bench.py), for
      valid_dim 56 / 112 / 192 in both modes: MPix/s and the phase split (analysis, exposed entropy encode, entropy
      decode, synthesis)"""
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

MODES = ("valu", "mfma")


def _ent(vd):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    torch.manual_seed(1234)
    enc = PC.PseudoEncoder(vd, 0).eval()
    g = torch.Generator().manual_seed(7)
    enc.ent.load_state_dict({k: torch.randn(v.shape, generator=g) * 0.05 for k, v in enc.ent.state_dict().items()})
    return enc.ent


def layers(reps):
    from pseudocylindrical_convolution_amd.engine import EntropyEngine
    h, w = 16, 512
    for vd in (56, 112, 192):
        ent = _ent(vd)
        sym = torch.randint(0, 8, (16, ent.ngroup, h, w), generator=torch.Generator().manual_seed(3)).float().cuda()
        sym = ent.fill(sym).contiguous()
        out = {}
        for mode in MODES:
            os.environ["PCONV_EE_BULK"] = mode
            eng = EntropyEngine(ent, h, w, 1, "cuda:0")
            best = 1e9
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.encode_begin(sym, 1)
                streams = eng.encode_end()
                best = min(best, time.perf_counter() - t0)
            out[mode] = streams
            print("groups %2d  %-4s  forms %s  encode (one range, GPU + coder) %.1f ms  %d bytes" % (
                ent.ngroup, mode, "".join(str(f) for f in eng.encoder_forms), best * 1e3, len(streams[0])), flush=True)
            del eng
        print("groups %2d  streams identical: %s" % (ent.ngroup, out["valu"] == out["mfma"]), flush=True)
    os.environ.pop("PCONV_EE_BULK", None)


def summarise(root):
    files = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_stats.csv under %s" % root)
    rows = []
    for path in files:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if "ee_conv_bulk" not in name:
                    continue
                avg = next((float(v) for k, v in r.items() if k and "Average" in k), None)
                rows.append((name, int(r.get("Calls", 0) or 0), avg))
    print("%-70s %6s %12s" % ("kernel", "calls", "us / launch"))
    for name, calls, avg in sorted(rows, key=lambda t: t[0]):
        short = name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]
        print("%-70s %6d %12.1f" % (short[:70], calls, (avg or 0.0) / 1e3))


def codec(steps, H, W):
    import bench
    from pseudocylindrical_convolution_amd.engine import CodecEngine, FramePipe
    n = 8
    host = torch.stack([bench.frame_u8(H, W, 100 + i) for i in range(n)], 0).pin_memory()
    for vd in (56, 112, 192):
        for mode in MODES:
            os.environ["PCONV_EE_BULK"] = mode
            enc, dec = bench.make_codec(0, vd=vd)
            eng = CodecEngine(vd, 0, enc, dec)
            pipe = FramePipe(n, H, W, torch.device("cuda", 0))
            fill = use = 0

            def step():
                nonlocal fill, use
                slot, use = use, use ^ 1
                frames = pipe.take(slot)
                pipe.prefetch(host, fill)
                fill ^= 1
                streams = eng.encode(frames)
                rec = eng.decode(streams, H, W)
                pipe.give(rec, slot)
                return slot, streams

            pipe.prefetch(host, fill)
            fill ^= 1
            slot, streams = step()           # warm-up: engines, kernels, first use of every buffer
            pipe.wait(slot)
            torch.cuda.synchronize()
            eng.phase_probe = []
            t0 = time.perf_counter()
            for _ in range(steps):
                slot, streams = step()
            pipe.wait(slot)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            per = {}
            for name, e0, e1 in eng.phase_probe:
                per[name] = per.get(name, 0.0) + e0.elapsed_time(e1) / steps
            eng.phase_probe = None
            print("vd %3d  %-4s  %7.2f MPix/s  step %7.1f ms  analysis %6.1f  entropy_encode %6.1f  entropy_decode %7.1f"
                  "  synthesis %6.1f ms  %d bytes" % (
                      vd, mode, n * H * W / dt / 1e6, dt * 1e3, per.get("analysis", 0), per.get("entropy_encode", 0),
                      per.get("entropy_decode", 0), per.get("synthesis", 0), sum(len(s) for s in streams)), flush=True)
            del eng, pipe, enc, dec
            torch.cuda.empty_cache()
    os.environ.pop("PCONV_EE_BULK", None)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "layers"
    if what == "layers":
        layers(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    elif what == "summarise":
        summarise(sys.argv[2])
    elif what == "codec":
        codec(int(sys.argv[2]) if len(sys.argv) > 2 else 2, int(sys.argv[3]) if len(sys.argv) > 3 else 2048,
              int(sys.argv[4]) if len(sys.argv) > 4 else 4096)
    else:
        sys.exit(__doc__)
