"""Time the vessel Dice index (csrc/vessel.hip) against the same score composed from torch ops.

    python tools/vessel_bench.py [--out profiles/vessel_bench.txt]

Defaults (sigmas (1, 2, 3), equal weights, beta 0.5, c 0.1, eps 1e-6, value_range (-1, 1), bright), shapes (8,1,256,256),
(64,1,256,256), (8,1,512,512); forward + backward of the score with gradients to both images.  ``ops.vessel_dice`` runs two entry points
forward (three launches: ``vessel_index``, ``vessel_final`` and its one-block mean) and one backward; the baseline is the composition a
user would otherwise write, the restatement of tests/test_vessel_cpu.py on the device in fp32: per image and scale three grouped
``F.conv2d`` with the outer products of the sampled Gaussian-derivative kernels, the pointwise ops of the measure, the three means of the
Dice coefficient, the gradient left to autograd.
A row: median [min, max] ms of the HIP op and of the composition, the ratio of the medians, the spread (max - min) / median of the
seven batches of either, the peak device memory either allocates above the inputs in one forward + backward, and the traffic floor --
x and y read once per direction, both gradients written once -- over the HIP op's median time as a share of 8 TB/s.
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
SIGMAS, BETA, C, EPS = (1.0, 2.0, 3.0), 0.5, 0.1, 1e-6
HBM_BYTES_PER_S = 8e12


def kernels(ch):
    """Per scale (R, sigma^2, the three 2-D kernels of a, b, d stacked per channel), flipped: conv2d correlates."""
    out = []
    for sigma in SIGMAS:
        R = int(3 * sigma + 0.5)
        t = torch.arange(-R, R + 1, dtype=torch.float64)
        g = torch.exp(-t * t / (2 * sigma * sigma))
        g = g / g.sum()
        g1, g2 = -t / sigma ** 2 * g, (t * t / sigma ** 4 - 1 / sigma ** 2) * g
        k = torch.stack([torch.outer(kh.flip(0), kw.flip(0)) for kw, kh in ((g2, g), (g1, g1), (g, g2))])[:, None]
        out.append((R, sigma * sigma, k.repeat(ch, 1, 1, 1).float().cuda()))
    return out


def response(x, ks):
    u = (x + 1) / 2
    ch = x.shape[1]
    acc = 0
    for R, s2, k in ks:
        H = s2 * F.conv2d(u, k, padding=R, groups=ch)
        a, b, d = H[:, 0::3], H[:, 1::3], H[:, 2::3]
        m, h = (a + d) / 2, (a - d) / 2
        q = h * h + b * b
        pos = q > 0
        r = torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))
        kappa, mu = r - m, m + r
        ks_ = torch.where(kappa > 0, kappa, torch.ones_like(kappa))
        E1 = mu * mu / (2 * BETA * BETA * ks_ * ks_)
        valid = (kappa > 0) & (E1 < 87.0)
        E1 = torch.where(valid, E1, torch.zeros_like(E1))
        E2 = (mu * mu + kappa * kappa) / (2 * C * C)
        acc = acc + torch.where(valid, torch.exp(-E1) * -torch.expm1(-E2), torch.zeros_like(E1)) / len(ks)
    return acc


def composed(x, y, ks):
    A, B = response(x, ks), response(y, ks)
    D = (A * A).mean(dim=(1, 2, 3)) + (B * B).mean(dim=(1, 2, 3)) + EPS
    return ((2 * (A * B).mean(dim=(1, 2, 3)) + EPS) / D).mean()


def peak_above_inputs(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vessel_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    lines = ["The vessel Dice index, sigmas %s, beta 0.5, c 0.1, eps 1e-6, value_range (-1, 1), forward + backward of the score to both images:" % (SIGMAS,),
             "csrc/vessel.hip against three grouped F.conv2d per image and scale + pointwise ops + three means + autograd in fp32, on the same card; device: %s;"
             % torch.cuda.get_device_name(0),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "peak = device memory allocated above the inputs during one forward + backward, hip / composed;",
             "floor = the traffic floor (x, y read once per direction, both gradients written once) over the hip median as a share of 8 TB/s", ""]
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        ch = shape[1]
        box5 = torch.ones(ch, 1, 5, 5, device="cuda") / 25.0
        xg = 2.0 * F.conv2d(F.pad(torch.randn(*shape, device="cuda", generator=g), (2, 2, 2, 2), mode="replicate"), box5, groups=ch)
        yg = (xg + 0.1 * torch.randn(*shape, device="cuda", generator=g)).requires_grad_(True)
        xg.requires_grad_(True)
        ks = kernels(ch)

        def fused():
            return faoctasr.ops.vessel_dice(xg, yg)
        with torch.no_grad():
            sf, sc = float(fused()), float(composed(xg, yg, ks))
        assert abs(sf - sc) <= 1e-4 * abs(sc), (sf, sc)                     # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = yg.grad = None
                fn().backward()
            return run

        hip, ref = step(fused), step(lambda: composed(xg, yg, ks))
        (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
        xg.grad = yg.grad = None
        pk_hip = peak_above_inputs(hip)
        xg.grad = yg.grad = None
        pk_ref = peak_above_inputs(ref)
        xg.grad = yg.grad = None
        floor = 4 * 6 * xg.numel() / HBM_BYTES_PER_S * 1e3
        lines.append("%-12s %-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx%s  spread %4.1f%% / %4.1f%%  peak %.1f / %.1f MiB  floor %.4f ms = %4.1f%%"
                     % ("vessel_dice", "x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m,
                        "" if m + (hi - lo) + (thi - tlo) < tm else "  ** not faster by more than both spreads **",
                        100 * (hi - lo) / m, 100 * (thi - tlo) / tm, pk_hip / 2 ** 20, pk_ref / 2 ** 20, floor, 100 * floor / m))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
