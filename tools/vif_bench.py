"""Time the pixel-domain visual information fidelity (csrc/vif.hip) against the same score composed from torch ops.

    python tools/vif_bench.py [--out profiles/vif_bench.txt]

Defaults (sigma_n_sq 2, value_range (-1, 1)), shapes (8,1,256,256), (64,1,256,256), (8,1,512,512); forward + backward of the score with
gradients to both images.  ``ops.vif`` runs five launches forward (four ``vif_scale_fwd``, ``vif_final``) and four backward; the baseline
is the composition a user would otherwise write, the definition on the device in fp32: per scale five grouped ``F.conv2d`` with the
outer product of the window (up to 17 x 17 taps), two more for the decimation, the ``where``s of the four branches, the logarithms and
sums, the gradient left to autograd.
A row: median [min, max] ms of the HIP op and of the composition, the ratio of the medians, the spread (max - min) / median of the
seven batches of either, the peak device memory either allocates above the inputs in one forward + backward, and the traffic floor --
x and r read once per direction, both gradients written once -- over the HIP op's median time as a share of 8 TB/s.
Method (tools/dwt_bench.py's): 5 warm-up runs of each, then 7 batches of 20 runs each, the two candidates' batches alternating,
timed with device events around the batch; outputs are not read back between runs.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faoctasr                          # noqa: E402
from dwt_bench import timed_pair         # noqa: E402

SHAPES = ((8, 1, 256, 256), (64, 1, 256, 256), (8, 1, 512, 512))
SIGMA_N_SQ, EPS = 2.0, 1e-8
HBM_BYTES_PER_S = 8e12


def windows(ch):
    """Per scale the 2-D window stacked per channel."""
    out = []
    for s in range(4):
        w = torch.tensor(faoctasr.ops.vif_window(s), dtype=torch.float64)
        out.append(torch.outer(w, w)[None, None].repeat(ch, 1, 1, 1).float().cuda())
    return out


def composed(x, r, ks):
    ch = x.shape[1]
    x, r = (x + 1) * 127.5, (r + 1) * 127.5
    num = den = 0
    for s, k in enumerate(ks):
        f = lambda t: F.conv2d(t, k, groups=ch)
        if s > 0:
            x, r = f(x)[..., ::2, ::2], f(r)[..., ::2, ::2]
        mx, mr = f(x), f(r)
        sxx, srr, sxr = torch.relu(f(x * x) - mx * mx), torch.relu(f(r * r) - mr * mr), f(x * r) - mx * mr
        g = sxr / (srr + EPS)
        sv = sxx - g * sxr
        zero = torch.zeros_like(g)
        m = srr < EPS
        g, sv, srr = torch.where(m, zero, g), torch.where(m, sxx, sv), torch.where(m, zero, srr)
        m = sxx < EPS
        g, sv = torch.where(m, zero, g), torch.where(m, zero, sv)
        m = g < 0
        sv, g = torch.where(m, sxx, sv), torch.where(m, zero, g)
        sv = torch.where(sv <= EPS, torch.full_like(sv, EPS), sv)
        num = num + torch.log10(1 + g * g * srr / (sv + SIGMA_N_SQ)).sum(dim=(1, 2, 3))
        den = den + torch.log10(1 + srr / SIGMA_N_SQ).sum(dim=(1, 2, 3))
    return ((num + EPS) / (den + EPS)).mean()


def peak_above_inputs(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vif_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    lines = ["VIFp, sigma_n_sq 2, value_range (-1, 1), forward + backward of the score to both images:",
             "csrc/vif.hip against five grouped F.conv2d per scale + two for the decimation + the branches' wheres + autograd in fp32, on the same card; device: %s;"
             % torch.cuda.get_device_name(0),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "peak = device memory allocated above the inputs during one forward + backward, hip / composed;",
             "floor = the traffic floor (x, r read once per direction, both gradients written once) over the hip median as a share of 8 TB/s", ""]
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        ch = shape[1]
        box5 = torch.ones(ch, 1, 5, 5, device="cuda") / 25.0
        rg = 2.0 * F.conv2d(F.pad(torch.randn(*shape, device="cuda", generator=g), (2, 2, 2, 2), mode="replicate"), box5, groups=ch)
        xg = (rg + 0.1 * torch.randn(*shape, device="cuda", generator=g)).requires_grad_(True)
        rg.requires_grad_(True)
        ks = windows(ch)

        def fused():
            return faoctasr.ops.vif(xg, rg)
        with torch.no_grad():
            sf, sc = float(fused()), float(composed(xg, rg, ks))
        assert abs(sf - sc) <= 1e-4 * abs(sc), (sf, sc)                     # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = rg.grad = None
                fn().backward()
            return run

        hip, ref = step(fused), step(lambda: composed(xg, rg, ks))
        (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
        xg.grad = rg.grad = None
        pk_hip = peak_above_inputs(hip)
        xg.grad = rg.grad = None
        pk_ref = peak_above_inputs(ref)
        xg.grad = rg.grad = None
        floor = 4 * 6 * xg.numel() / HBM_BYTES_PER_S * 1e3
        lines.append("%-5s %-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx%s  spread %4.1f%% / %4.1f%%  peak %.1f / %.1f MiB  floor %.4f ms = %4.1f%%"
                     % ("vif", "x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m,
                        "" if m + (hi - lo) + (thi - tlo) < tm else "  ** not faster by more than both spreads **",
                        100 * (hi - lo) / m, 100 * (thi - tlo) / tm, pk_hip / 2 ** 20, pk_ref / 2 ** 20, floor, 100 * floor / m))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
