"""Time GMSD and MS-GMSD (csrc/gmsd.hip) against the same scores composed from torch ops.

    python tools/gmsd_bench.py [--out profiles/gmsd_bench.txt]

Defaults (c = 0.0026, value_range (-1, 1), the four MS-GMSD weights), shapes (8,1,256,256), (64,1,256,256), (8,1,512,512); forward +
backward of the score with gradients to both images.  ``ops.gmsd`` runs two launches forward and one backward, ``ops.ms_gmsd`` five and
four; the baseline is the composition the op replaces, the restatement of tests/test_gmsd_cpu.py on the device in fp32: ``F.avg_pool2d``,
``F.pad``, a grouped ``F.conv2d`` with the two Prewitt kernels, the pointwise ops and the two reductions of the variance, the gradient
left to autograd.
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
C = 0.0026
HBM_BYTES_PER_S = 8e12


def variance(a, b, k):
    ch = a.shape[1]
    ga, gb = F.conv2d(F.pad(a, (1, 1, 1, 1)), k, groups=ch), F.conv2d(F.pad(b, (1, 1, 1, 1)), k, groups=ch)
    ma, mb = torch.sqrt(ga[:, 0::2] ** 2 + ga[:, 1::2] ** 2), torch.sqrt(gb[:, 0::2] ** 2 + gb[:, 1::2] ** 2)
    g = (2 * ma * mb + C) / (ma * ma + mb * mb + C)
    return ((g - g.mean(dim=(1, 2, 3), keepdim=True)) ** 2).mean(dim=(1, 2, 3))


def composed(x, y, k, weights):
    a, b = (x + 1) / 2, (y + 1) / 2
    if weights is None:
        return torch.sqrt(variance(F.avg_pool2d(a, 2), F.avg_pool2d(b, 2), k)).mean()
    acc = 0
    for j, w in enumerate(weights):
        if j:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
        acc = acc + w * variance(a, b, k)
    return torch.sqrt(acc).mean()


def peak_above_inputs(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmsd_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    lines = ["GMSD and MS-GMSD (weights %s), c = 0.0026, value_range (-1, 1), forward + backward of the score to both images:" % (faoctasr.ops.MSGMSD_WEIGHTS,),
             "csrc/gmsd.hip against F.avg_pool2d + F.pad + grouped F.conv2d (Prewitt) + pointwise ops + two reductions + autograd in fp32, on the same card; device: %s;"
             % torch.cuda.get_device_name(0),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "peak = device memory allocated above the inputs during one forward + backward, hip / composed;",
             "floor = the traffic floor (a, b read once per direction, both gradients written once) over the hip median as a share of 8 TB/s", ""]
    for name, weights in (("gmsd", None), ("ms_gmsd", faoctasr.ops.MSGMSD_WEIGHTS)):
        for shape in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(1)
            ch = shape[1]
            box5 = torch.ones(ch, 1, 5, 5, device="cuda") / 25.0
            xg = 2.0 * F.conv2d(F.pad(torch.randn(*shape, device="cuda", generator=g), (2, 2, 2, 2), mode="replicate"), box5, groups=ch)
            yg = (xg + 0.1 * torch.randn(*shape, device="cuda", generator=g)).requires_grad_(True)
            xg.requires_grad_(True)
            kx = torch.tensor([[1.0, 0.0, -1.0]] * 3, device="cuda") / 3.0
            k = torch.stack((kx, kx.t()))[:, None].repeat(ch, 1, 1, 1)

            def fused():
                return faoctasr.ops.gmsd(xg, yg) if weights is None else faoctasr.ops.ms_gmsd(xg, yg, weights)
            with torch.no_grad():
                sf, sc = float(fused()), float(composed(xg, yg, k, weights))
            assert abs(sf - sc) <= 1e-4 * abs(sc), (sf, sc)                 # the two candidates compute the same thing

            def step(fn):
                def run():
                    xg.grad = yg.grad = None
                    fn().backward()
                return run

            hip, ref = step(fused), step(lambda: composed(xg, yg, k, weights))
            (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
            xg.grad = yg.grad = None
            pk_hip = peak_above_inputs(hip)
            xg.grad = yg.grad = None
            pk_ref = peak_above_inputs(ref)
            xg.grad = yg.grad = None
            floor = 4 * 6 * xg.numel() / HBM_BYTES_PER_S * 1e3
            lines.append("%-8s %-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx%s  spread %4.1f%% / %4.1f%%  peak %.1f / %.1f MiB  floor %.4f ms = %4.1f%%"
                         % (name, "x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m,
                            "" if m + (hi - lo) + (thi - tlo) < tm else "  ** not faster by more than both spreads **",
                            100 * (hi - lo) / m, 100 * (thi - tlo) / tm, pk_hip / 2 ** 20, pk_ref / 2 ** 20, floor, 100 * floor / m))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
