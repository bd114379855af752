"""Time soft-clDice (csrc/cldice.hip) against the same index composed from torch ops.

    python tools/cldice_bench.py [--out profiles/cldice_bench.txt]

smooth 1, value_range (-1, 1), bright vessels; shapes (8,1,256,256), (64,1,256,256), (8,1,512,512) at iters 3 and 10; forward + backward of
the index with gradients to both images.  ``ops.cldice`` runs two entry points forward (``cldice_index``, ``cldice_final``) and one backward
(``cldice_grad``); the baseline is the composition a user would otherwise write, the definition on the device in fp32: per level and image
two one-dimensional ``max_pool2d`` of the negated plane and a ``torch.min`` (the erosion), one 3 x 3 ``max_pool2d`` (the dilation), and the
pointwise recurrence, the gradient left to autograd (every ``max_pool2d`` keeps an int64 index map for it).
A row: median [min, max] ms of the HIP op and of the composition, the ratio of the medians, the spread (max - min) / median of the
seven batches of either, the peak device memory either allocates above the inputs in one forward + backward, and the traffic floor --
x and y read once per direction, both gradients written once -- over the HIP op's median time as a share of 8 TB/s (the records the
forward stores and the backward reads, 2 * 2 * 5 (iters + 1) bytes per sample, are this design's own traffic and not part of the floor).
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
ITERS = (3, 10)
SMOOTH = 1.0
HBM_BYTES_PER_S = 8e12


def erode(I):
    return torch.min(-F.max_pool2d(-I, (3, 1), 1, (1, 0)), -F.max_pool2d(-I, (1, 3), 1, (0, 1)))


def skeleton(u, iters):
    I, s = u, None
    for _ in range(iters + 1):
        nxt = erode(I)
        delta = torch.relu(I - F.max_pool2d(nxt, 3, 1, 1))
        s = delta if s is None else s + torch.relu(delta - s * delta)
        I = nxt
    return s


def composed(x, y, iters):
    ux, uy = (x + 1) / 2, (y + 1) / 2
    sx, sy = skeleton(ux, iters), skeleton(uy, iters)
    tprec = ((sx * uy).sum(dim=(1, 2, 3)) + SMOOTH) / (sx.sum(dim=(1, 2, 3)) + SMOOTH)
    tsens = ((sy * ux).sum(dim=(1, 2, 3)) + SMOOTH) / (sy.sum(dim=(1, 2, 3)) + SMOOTH)
    return (2 * tprec * tsens / (tprec + tsens)).mean()


def peak_above_inputs(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cldice_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    lines = ["soft-clDice, smooth 1, value_range (-1, 1), forward + backward of the index to both images:",
             "csrc/cldice.hip against three max_pool2d + a min per level and image + the pointwise recurrence + autograd in fp32, on the same card; device: %s;"
             % torch.cuda.get_device_name(0),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "peak = device memory allocated above the inputs during one forward + backward, hip / composed;",
             "floor = the traffic floor (x, y read once per direction, both gradients written once) over the hip median as a share of 8 TB/s", ""]
    for iters in ITERS:
        for shape in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(1)
            ch = shape[1]
            box5 = torch.ones(ch, 1, 5, 5, device="cuda") / 25.0
            b = F.conv2d(F.pad(torch.rand(*shape, device="cuda", generator=g), (2, 2, 2, 2), mode="replicate"), box5, groups=ch)
            base = (b - b.min()) / (b.max() - b.min())
            xg = (2 * base - 1).requires_grad_(True)
            yg = (2 * (0.8 * base + 0.2 * torch.rand(*shape, device="cuda", generator=g)) - 1).requires_grad_(True)

            def fused():
                return faoctasr.ops.cldice(xg, yg, iters, SMOOTH)
            with torch.no_grad():
                sf, sc = float(fused()), float(composed(xg, yg, iters))
            assert abs(sf - sc) <= 1e-5 * abs(sc), (sf, sc)                 # the two candidates compute the same thing

            def step(fn):
                def run():
                    xg.grad = yg.grad = None
                    fn().backward()
                return run

            hip, ref = step(fused), step(lambda: composed(xg, yg, iters))
            (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
            xg.grad = yg.grad = None
            pk_hip = peak_above_inputs(hip)
            xg.grad = yg.grad = None
            pk_ref = peak_above_inputs(ref)
            xg.grad = yg.grad = None
            floor = 4 * 6 * xg.numel() / HBM_BYTES_PER_S * 1e3
            lines.append("%-9s %-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx%s  spread %4.1f%% / %4.1f%%  peak %.1f / %.1f MiB  floor %.4f ms = %4.1f%%"
                         % ("iters %d" % iters, "x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m,
                            "" if m + (hi - lo) + (thi - tlo) < tm else "  ** not faster by more than both spreads **",
                            100 * (hi - lo) / m, 100 * (thi - tlo) / tm, pk_hip / 2 ** 20, pk_ref / 2 ** 20, floor, 100 * floor / m))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
