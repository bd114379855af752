"""Time the local normalised cross-correlation (csrc/lncc.hip) against the same score composed from torch ops.

    python tools/lncc_bench.py [--out profiles/lncc_bench.txt] [--win 9]

Defaults (win = 9, eps = 1e-5), shapes (8,1,256,256), (64,1,256,256), (8,1,512,512); forward + backward of the loss 1 - LNCC with
gradients to both images.  ``ops.lncc`` runs two launches forward and one backward; the baseline is the composition the op replaces,
the restatement of tests/test_lncc_cpu.py on the device in fp32: five grouped ``F.conv2d`` with a win x win kernel of ones and padding
win // 2, the pointwise ops and the mean, the gradient left to autograd.
A row: median [min, max] ms of the HIP op and of the composition, the ratio of the medians, the spread (max - min) / median of the
seven batches of either, the peak device memory either allocates above the inputs in one forward + backward, and the traffic floor --
a and b read once per direction, both gradients written once -- over the HIP op's median time as a share of 8 TB/s.
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
EPS = 1e-5
HBM_BYTES_PER_S = 8e12


def composed(x, y, ones, win):
    ch, n = x.shape[1], float(win * win)

    def box(t):
        return F.conv2d(t, ones, padding=win // 2, groups=ch)
    Sa, Sb, Saa, Sbb, Sab = box(x), box(y), box(x * x), box(y * y), box(x * y)
    u, va, vb = Sab - Sa * Sb / n, Saa - Sa * Sa / n, Sbb - Sb * Sb / n
    return (u * u / (va * vb + EPS)).mean(dim=(1, 2, 3)).mean()


def peak_above_inputs(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lncc_bench.txt"))
    ap.add_argument("--win", type=int, default=9)
    args = ap.parse_args()
    win = args.win
    faoctasr._lib.load()
    lines = ["LNCC, win = %d, eps = 1e-5, forward + backward of 1 - LNCC to both images:" % win,
             "csrc/lncc.hip against five grouped F.conv2d (%d x %d ones, padding %d) + pointwise ops + autograd in fp32, on the same card; device: %s;"
             % (win, win, win // 2, torch.cuda.get_device_name(0)),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "peak = device memory allocated above the inputs during one forward + backward, hip / composed;",
             "floor = the traffic floor (a, b read once per direction, both gradients written once) over the hip median as a share of 8 TB/s", ""]
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        box5 = torch.ones(shape[1], 1, 5, 5, device="cuda") / 25.0

        def smooth(t):
            return F.conv2d(F.pad(t, (2, 2, 2, 2), mode="replicate"), box5, groups=shape[1])
        xg = 2.0 * smooth(torch.randn(*shape, device="cuda", generator=g))
        yg = (-0.6 * xg + 0.2 + 0.6 * smooth(torch.randn(*shape, device="cuda", generator=g))
              + 0.05 * torch.randn(*shape, device="cuda", generator=g)).requires_grad_(True)
        xg.requires_grad_(True)
        ones = torch.ones(shape[1], 1, win, win, device="cuda")
        with torch.no_grad():
            sf, sc = float(faoctasr.ops.lncc(xg, yg, win, EPS)), float(composed(xg, yg, ones, win))
        assert abs(sf - sc) <= 1e-4 * abs(sc), (sf, sc)                 # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = yg.grad = None
                (1 - fn()).backward()
            return run

        hip, ref = step(lambda: faoctasr.ops.lncc(xg, yg, win, EPS)), step(lambda: composed(xg, yg, ones, win))
        (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
        xg.grad = yg.grad = None
        pk_hip = peak_above_inputs(hip)
        xg.grad = yg.grad = None
        pk_ref = peak_above_inputs(ref)
        xg.grad = yg.grad = None
        floor = 4 * 6 * xg.numel() / HBM_BYTES_PER_S * 1e3
        lines.append("%-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx%s  spread %4.1f%% / %4.1f%%  peak %.1f / %.1f MiB  floor %.4f ms = %4.1f%%"
                     % ("x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m, "" if m <= tm else "  ** the fused path loses here **",
                        100 * (hi - lo) / m, 100 * (thi - tlo) / tm, pk_hip / 2 ** 20, pk_ref / 2 ** 20, floor, 100 * floor / m))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
