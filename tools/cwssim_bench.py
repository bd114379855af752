"""Time the complex-wavelet structural similarity (csrc/cwssim.hip) against the same index composed from torch ops.

    python tools/cwssim_bench.py [--out profiles/cwssim_bench.txt]

near_sym_a + qshift_a (taps from the test fixtures), 'symmetric', J = 3, win 7, K 1e-2, shapes (8,1,256,256), (64,1,256,256),
(8,1,512,512); forward + backward of the loss 1 - S with gradients to both images.  Both candidates run the same transform ops
(two ``DTCWTForward``; their backward passes are ``dtcwt_inv_j2`` / ``dtcwt_inv_j1``); they differ in the index alone: ``CWSSIM``
runs ``cwssim_index`` / ``cwssim_final`` / ``cwssim_grad`` per level, the baseline forms the products with torch ops, box-sums them
with ``F.avg_pool2d`` and leaves the gradient to autograd.
A row: median [min, max] ms of the HIP op and of the composition, the ratio of the medians and the spread (max - min) / median
of the seven batches of either.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import faoctasr                          # noqa: E402
from dwt_bench import timed_pair         # noqa: E402
import test_cwssim_cpu as R              # noqa: E402

SHAPES = ((8, 1, 256, 256), (64, 1, 256, 256), (8, 1, 512, 512))
K, J, WIN = 1e-2, 3, 7


def box(t):
    n, c, o, h, w = t.shape
    return F.avg_pool2d(t.reshape(n, c * o, h, w), WIN, stride=1) * float(WIN * WIN)


def composed(fwd, x, y):
    acc = None
    for a, b in zip(fwd(x)[1], fwd(y)[1]):
        ar, ai, br, bi = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
        zr, zi = box(ar * br + ai * bi), box(ai * br - ar * bi)
        E = box(ar * ar + ai * ai) + box(br * br + bi * bi)
        t = ((2 * torch.sqrt(zr * zr + zi * zi) + K) / (E + K)).mean()
        acc = t if acc is None else acc + t
    return acc / J


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cwssim_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    fb, fq = R.tuples("a")
    mod = faoctasr.CWSSIM(biort=fb, qshift=fq, J=J, win=WIN, K=K).cuda()
    fwd = faoctasr.DTCWTForward(biort=fb, qshift=fq, J=J).cuda()
    lines = ["CW-SSIM, near_sym_a (5, 7 taps) + qshift_a (10 taps), 'symmetric', J = 3, win 7, forward + backward of 1 - S to both images:",
             "csrc/cwssim.hip against the same transform ops + torch products + F.avg_pool2d + autograd, on the same card; device: %s;"
             % torch.cuda.get_device_name(0), "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, hip / composed", ""]
    for shape in SHAPES:
        xg = torch.randn(*shape, device="cuda")
        yg = (xg + 0.5 * torch.randn(*shape, device="cuda")).requires_grad_(True)
        xg.requires_grad_(True)
        with torch.no_grad():
            sf, sc = float(mod(xg, yg)), float(composed(fwd, xg, yg))
        assert abs(sf - sc) <= 1e-5 * abs(sc), (sf, sc)                 # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = yg.grad = None
                (1 - fn()).backward()
            return run

        (m, lo, hi), (tm, tlo, thi) = timed_pair(step(lambda: mod(xg, yg)), step(lambda: composed(fwd, xg, yg)))
        lines.append("%-16s hip %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx  spread %4.1f%% / %4.1f%%"
                     % ("x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m, 100 * (hi - lo) / m, 100 * (thi - tlo) / tm))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
