"""Time HaarPSI (csrc/haarpsi.hip) against the same score composed from torch ops.

    python tools/haarpsi_bench.py [--out profiles/haarpsi_bench.txt]

Defaults (c = 30, alpha = 4.2, value_range (-1, 1)), shapes (8,1,256,256), (64,1,256,256), (8,1,512,512); forward + backward of the
loss 1 - HaarPSI with gradients to both images.  ``ops.haarpsi`` runs two launches forward and one backward; the baseline is the
composition the op replaces, the restatement of tests/test_haarpsi_cpu.py on the device in fp32: ``F.avg_pool2d`` of the mapped pair,
per scale ``F.pad`` and two grouped ``F.conv2d`` with the +-2^-k kernels, ``abs``, the similarity, ``sigmoid``, ``where``, the sums and
the logit, the gradient left to autograd.
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
C, ALPHA, LO, HI = 30.0, 4.2, -1.0, 1.0
HBM_BYTES_PER_S = 8e12


def composed(x, y, kernels):
    def half_map(t):
        u = (t - LO) * 255 / (HI - LO)
        return F.avg_pool2d(F.pad(u, (0, t.shape[-1] % 2, 0, t.shape[-2] % 2)), 2)

    def haar(u2, k):
        K, ch = 2 ** k, u2.shape[1]
        p = F.pad(u2, (K // 2 - 1, K // 2, K // 2 - 1, K // 2))
        kv = kernels[k]
        return F.conv2d(p, kv.expand(ch, 1, K, K), groups=ch), F.conv2d(p, kv.t().expand(ch, 1, K, K), groups=ch)
    u2, v2 = half_map(x), half_map(y)
    gx, gy = [haar(u2, k) for k in (1, 2, 3)], [haar(v2, k) for k in (1, 2, 3)]
    num = den = 0
    for o in (0, 1):
        S = 0
        for k in (0, 1):
            a, b = gx[k][o].abs(), gy[k][o].abs()
            S = S + (2 * a * b + C) / (a * a + b * b + C)
        a3, b3 = gx[2][o].abs(), gy[2][o].abs()
        Wt = torch.where(a3 >= b3, a3, b3)
        num = num + (torch.sigmoid(ALPHA * (S / 2)) * Wt).sum(dim=(1, 2, 3))
        den = den + Wt.sum(dim=(1, 2, 3))
    r = num / den
    return ((torch.log(r / (1 - r)) / ALPHA) ** 2).mean()


def peak_above_inputs(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haarpsi_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    kernels = {}
    for k in (1, 2, 3):
        kv = torch.full((2 ** k, 2 ** k), 2.0 ** -k, device="cuda")
        kv[2 ** k // 2:] *= -1
        kernels[k] = kv
    lines = ["HaarPSI, c = 30, alpha = 4.2, value_range (-1, 1), forward + backward of 1 - HaarPSI to both images:",
             "csrc/haarpsi.hip against F.avg_pool2d + F.pad + grouped F.conv2d (2, 4, 8) + pointwise ops + autograd in fp32, on the same card; device: %s;"
             % torch.cuda.get_device_name(0),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "peak = device memory allocated above the inputs during one forward + backward, hip / composed;",
             "floor = the traffic floor (x, y read once per direction, both gradients written once) over the hip median as a share of 8 TB/s", ""]
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        n = torch.randn(*shape, device="cuda", generator=g)
        xg = 2.0 * F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(shape[1], 1, 5, 5, device="cuda") / 25.0, groups=shape[1])
        yg = (xg + 0.1 * torch.randn(*shape, device="cuda", generator=g)).requires_grad_(True)
        xg.requires_grad_(True)
        with torch.no_grad():
            sf, sc = float(faoctasr.ops.haarpsi(xg, yg)), float(composed(xg, yg, kernels))
        assert abs(sf - sc) <= 1e-4 * abs(sc), (sf, sc)                 # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = yg.grad = None
                (1 - fn()).backward()
            return run

        hip, ref = step(lambda: faoctasr.ops.haarpsi(xg, yg)), step(lambda: composed(xg, yg, kernels))
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
