"""WS-PSNR / WS-SSIM on one GPU: the HIP kernels of csrc/sphere_metrics.hip (ms_forward_kernel<T, 1, 1>,
ms_close_kernel<1>) against the torch composition.

The torch composition is what a user would write without the kernel: pytorch_ssim's five depthwise 11x11
convolutions (F.conv2d, MIOpen) for the SSIM map, then the row-weighted means of the map and of (x - y)^2, with
uint8 frames converted to float32 first.  Both are timed with device events at n = 1 and 8 frames of 4096x2048 and
5760x2880, float32 (n, 3, h, w) and uint8 (n, h, w, 3): warm-up, then rounds that alternate the two, median of the
rounds.  The HIP figure is the C entry point with its workspace allocated beforehand (both launches); effective
TB/s = the bytes of the two input batches / time.  The two results are checked against each other.

    python tools/sphere_metrics_probe.py [--rounds 10] [--out profiles/sphere_metrics.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudocylindrical_convolution_amd import PCONV, sphere_metrics  # noqa: E402
from pseudocylindrical_convolution_amd._native import call  # noqa: E402
from pseudocylindrical_convolution_amd.PCONV_operator import pytorch_ssim  # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def torch_composition(x, y, wr):
    """(n, 2) WS-MSE, WS-SSIM: pytorch_ssim's map and weighted means in torch (float32, MIOpen convolutions)"""
    if x.dtype == torch.uint8:
        x, y = (t.permute(0, 3, 1, 2).float() / 255. for t in (x, y))
    c = x.shape[1]
    win = pytorch_ssim.create_window(11, c).to(x.device)
    blur = lambda t: F.conv2d(t, win, padding=5, groups=c)
    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(x * x) - mu1_sq, blur(y * y) - mu2_sq, blur(x * y) - mu1_mu2
    smap = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    norm = c * x.shape[3] * wr.sum()
    wmse = (((x - y) ** 2).double() * wr).sum(dim=(1, 2, 3)) / norm
    wssim = (smap.double() * wr).sum(dim=(1, 2, 3)) / norm
    return torch.stack([wmse, wssim], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sphere_metrics_probe: needs a GPU")
    dev = torch.device("cuda:0")
    lines = ["# WS-PSNR + WS-SSIM of n frame pairs; median of %d rounds of %d calls; TB/s = input bytes / time"
             % (args.rounds, args.reps), "# device: %s" % torch.cuda.get_device_name(dev),
             "%-6s %-10s %2s %10s %10s %8s %11s %8s %9s %9s" % ("dtype", "size", "n", "MB in", "hip us", "TB/s",
                                                                 "torch us", "TB/s", "speed-up", "max diff")]
    for (h, w) in ((2048, 4096), (2880, 5760)):
        wr = sphere_metrics.weights(h).to(dev).view(1, 1, h, 1)
        for dtype in ("float32", "uint8"):
            for n in (1, 8):
                g = torch.Generator().manual_seed(n * h)
                if dtype == "float32":
                    x = torch.rand(n, 3, h, w, generator=g)
                    y = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(0, 1)
                    fn, c = "pconv_ws_metrics_f32", x.shape[1]
                else:
                    x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
                    y = (x.int() + torch.randint(-6, 7, x.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
                    fn, c = "pconv_ws_metrics_u8", 3
                x, y = x.to(dev), y.to(dev)
                ws = torch.empty(call("pconv_ws_metrics_workspace_bytes", n, h, w), dtype=torch.uint8, device=dev)
                out = torch.empty((n, 2), dtype=torch.float64, device=dev)
                stream = torch.cuda.current_stream(dev).cuda_stream
                hip = lambda: call(fn, x.data_ptr(), y.data_ptr(), n, c, h, w, 0, ws.data_ptr(), out.data_ptr(), stream)
                ref = lambda: torch_composition(x, y, wr)
                got, want = PCONV.ws_metrics(x, y), ref().cpu()
                diff = (got - want).abs().max().item()
                for fnc in (hip, ref):
                    timed(fnc, 2)
                th, tt = [], []
                for _ in range(args.rounds):
                    th.append(timed(hip, args.reps))
                    tt.append(timed(ref, args.reps))
                nbytes = 2.0 * x.numel() * x.element_size()
                a, b = statistics.median(th), statistics.median(tt)
                lines.append("%-6s %-10s %2d %10.1f %10.1f %8.2f %11.1f %8.2f %8.1fx %9.1e"
                             % (dtype[:5], "%dx%d" % (w, h), n, nbytes / 1e6, a * 1e6, nbytes / a / 1e12, b * 1e6,
                                nbytes / b / 1e12, b / a, diff))
                sys.stdout.write(lines[-1] + "\n")
                sys.stdout.flush()
                del x, y, ws, out
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
