"""Rate without coding on one GPU: CodecEngine.rate() against encode(), evaluate() against encode() + decode().

Eight 4096x2048 frames, seeded random weights (the entropy state of tests/test_gpu_engine.py), valid_dim 56.  Every
call is timed with device events recorded in the caller's stream around it (they include the host-side waits of
encode / decode: the end event is recorded when the call returns) after a warm-up that creates every engine and
workspace, and each timed call follows an untimed call of the same kind; the median of the rounds.  The phases of
encode() / decode() come from CodecEngine.phase_probe (the events bench.py uses), the two parts of rate() from an
event between its analysis transform and its engine calls.

    python tools/rate_probe.py [--frames 8] [--rounds 5] [--out profiles/rate_estimate.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import pseudo_codec as PC, rate  # noqa: E402
from pseudocylindrical_convolution_amd.engine import CodecEngine  # noqa: E402


def codec(vd):
    torch.manual_seed(1234)
    enc, dec = PC.PseudoEncoder(vd, 0).eval(), PC.PseudoDecoder(vd, 0).eval()
    g = torch.Generator().manual_seed(7)
    sd = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in enc.ent.state_dict().items()}
    enc.ent.load_state_dict(sd)
    dec.ent.load_state_dict(sd)
    dec.quant.weight.data.copy_(enc.quant.weight.data)
    return CodecEngine(vd, 0, enc, dec)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--valid-dim", type=int, default=56)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_probe: needs a GPU")
    n, H, W = args.frames, args.height, args.width
    eng = codec(args.valid_dim)
    x = torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()

    def rate_in_two_parts():
        """rate() with an event between its two halves: (analysis ms, entropy ms)"""
        t_sym, sym = timed(lambda: eng.symbols(x).contiguous())
        return t_sym, timed(lambda: eng._rate_of_symbols(sym, n, False))[0]

    def coded():
        streams = eng.encode(x)
        return streams, eng.decode(streams, H, W)

    cases = [("rate()", lambda: eng.rate(x)), ("encode()", lambda: eng.encode(x)),
             ("evaluate()", lambda: eng.evaluate(x)), ("encode() + decode()", coded)]
    for _ in range(2):   # warm-up: engines, workspaces, code objects, clocks
        for _, fn in cases:
            fn()
        rate_in_two_parts()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    phases = {"analysis": [], "entropy_encode": [], "entropy_decode": [], "synthesis": []}
    rate_only, rate_analysis = [], []
    streams = bits = None
    for _ in range(args.rounds):
        for name, fn in cases:
            eng.phase_probe = [] if name == "encode() + decode()" else None
            fn()   # (the same call just before the timed one: the allocator holds this call's blocks)
            t, out = timed(fn)
            times[name].append(t)
            if name == "rate()":
                bits = out
            if name == "encode()":
                streams = out
            if eng.phase_probe is not None:
                torch.cuda.synchronize()
                for phase, e0, e1 in eng.phase_probe:
                    phases[phase].append(e0.elapsed_time(e1))
                eng.phase_probe = None
        rate_in_two_parts()
        t_sym, t_rate = rate_in_two_parts()
        rate_analysis.append(t_sym)
        rate_only.append(t_rate)
    med = lambda v: statistics.median(v) if v else float("nan")
    est = rate.bpp(bits, H, W).cpu().numpy()
    real = [len(s) * 8.0 / (H * W) for s in streams]
    lines = ["# %d frames of %dx%d, valid_dim %d, seeded random weights; device events around each call, median of %d "
             "rounds after 2 warm-up rounds, each timed call after an untimed one of its kind (ms)" % (n, W, H, args.valid_dim, args.rounds),
             "# device: %s" % torch.cuda.get_device_name(0),
             "%-34s %10s %10s %10s" % ("call", "median", "min", "max")]
    for name, _ in cases:
        lines.append("%-34s %10.1f %10.1f %10.1f" % (name, med(times[name]), min(times[name]), max(times[name])))
    lines.append("%-34s %10.1f %10.1f %10.1f" % ("  rate(): analysis part", med(rate_analysis), min(rate_analysis), max(rate_analysis)))
    lines.append("%-34s %10.1f %10.1f %10.1f" % ("  rate(): entropy part", med(rate_only), min(rate_only), max(rate_only)))
    for phase in ("analysis", "entropy_encode", "entropy_decode", "synthesis"):
        v = phases[phase]
        if v:
            lines.append("%-34s %10.1f %10.1f %10.1f" % ("  phase: " + phase, med(v), min(v), max(v)))
    lines.append("# rate() / encode(): %.2f;  evaluate() / (encode() + decode()): %.2f;  entropy part of rate() / "
                 "entropy_encode phase: %.2f" % (med(times["rate()"]) / med(times["encode()"]),
                                                 med(times["evaluate()"]) / med(times["encode() + decode()"]),
                                                 med(rate_only) / med(phases["entropy_encode"])))
    lines.append("# bpp from the rows / bpp of the streams, per frame: " +
                 ", ".join("%.5f / %.5f" % (a, b) for a, b in zip(est, real)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
