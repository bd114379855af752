"""Time multi-scale SSIM (csrc/msssim.hip) against the same score composed from torch ops.

    python tools/msssim_bench.py [--out profiles/msssim_bench.txt]

M = 5, default weights, data_range 1, shapes (8,1,256,256), (64,1,256,256), (8,1,512,512); forward + backward of the loss 1 - MS
with gradients to both images.  ``ops.ms_ssim`` runs M + 1 launches forward and M backward; the baseline is the composition the
op replaces: five grouped ``F.conv2d`` with the 11 x 11 window per scale, ``F.avg_pool2d`` between the scales, ``pow`` and ``prod``,
the gradient left to autograd.
A row: median [min, max] ms of the HIP op and of the composition, the ratio of the medians, the spread (max - min) / median of the
seven batches of either, and the traffic floor -- each scale's pair read once forward and once backward, the pooled pairs and both
gradients of every scale written once -- over the HIP op's median time as a share of 8 TB/s.
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
M = 5
HBM_BYTES_PER_S = 8e12


def composed(x, y, window):
    w = faoctasr.ops.MSSSIM_WEIGHTS
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ch = x.shape[1]
    a, b, factors = x, y, []
    for j in range(M):
        mu1, mu2 = F.conv2d(a, window, padding=5, groups=ch), F.conv2d(b, window, padding=5, groups=ch)
        s11 = F.conv2d(a * a, window, padding=5, groups=ch) - mu1 * mu1
        s22 = F.conv2d(b * b, window, padding=5, groups=ch) - mu2 * mu2
        s12 = F.conv2d(a * b, window, padding=5, groups=ch) - mu1 * mu2
        cs = (2 * s12 + C2) / (s11 + s22 + C2)
        if j == M - 1:
            cs = cs * (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)
        factors.append(cs.mean(dim=(1, 2, 3)))
        if j < M - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    f = torch.stack(factors, dim=1).clamp(min=0)
    return f.pow(torch.tensor(w, device=x.device)).prod(dim=1).mean()


def traffic_floor_bytes(shape):
    """fp32 bytes that must move: forward reads the pair of every scale and writes the pooled pairs; backward reads the pair of
    every scale and the coarser gradients and writes both gradients of every scale."""
    n, c, h, w = shape
    px = [n * c * (h >> j) * (w >> j) for j in range(M)]
    fwd = 2 * sum(px) + 2 * sum(px[1:])
    bwd = 2 * sum(px) + 2 * sum(px[1:]) + 2 * sum(px)
    return 4 * (fwd + bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    lines = ["MS-SSIM, M = 5, default weights, forward + backward of 1 - MS to both images:",
             "csrc/msssim.hip against grouped F.conv2d (11 x 11) + F.avg_pool2d + pow + prod + autograd, on the same card; device: %s;"
             % torch.cuda.get_device_name(0),
             "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed;",
             "floor = the traffic floor over the hip median as a share of 8 TB/s", ""]
    for shape in SHAPES:
        window = faoctasr.ssim.create_window(11, shape[1]).cuda()
        xg = torch.rand(*shape, device="cuda")
        yg = (xg + 0.05 * torch.randn(*shape, device="cuda")).clamp(0, 1).requires_grad_(True)
        xg.requires_grad_(True)
        with torch.no_grad():
            sf, sc = float(faoctasr.ops.ms_ssim(xg, yg, M)), float(composed(xg, yg, window))
        assert abs(sf - sc) <= 1e-5 * abs(sc), (sf, sc)                 # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = yg.grad = None
                (1 - fn()).backward()
            return run

        (m, lo, hi), (tm, tlo, thi) = timed_pair(step(lambda: faoctasr.ops.ms_ssim(xg, yg, M)), step(lambda: composed(xg, yg, window)))
        floor = traffic_floor_bytes(shape) / HBM_BYTES_PER_S * 1e3
        lines.append("%-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx  spread %4.1f%% / %4.1f%%  floor %.4f ms = %4.1f%%"
                     % ("x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m, 100 * (hi - lo) / m, 100 * (thi - tlo) / tm, floor, 100 * floor / m))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
