"""Time the DTCWT magnitude loss (csrc/dtcwt_loss.hip) against the composition it replaces.

    python tools/dtcwt_loss_bench.py [--out profiles/dtcwt_loss_bench.txt]

near_sym_a + qshift_a (taps from the test fixtures), 'symmetric', magbias 1e-2, J = 3, shapes (8,1,256,256), (64,1,256,256),
(8,1,512,512); forward + backward with gradients to both images, ``DTCWTMagnitudeLoss`` against the composition the package offered
before: two ``DTCWTForward`` (J launches each, the band pyramids written to memory; their backward passes are ``dtcwt_inv_j2`` /
``dtcwt_inv_j1``), torch ops for the magnitudes and ``ops.l1_loss`` per level.
A row: median [min, max] ms of the fused op and of the composition, the ratio of the medians, the spread (max - min) / median of
the seven batches of either, and the traffic floor over the fused time in GB/s and as a share of the HBM rate given by
``--hbm-tbs`` (8.0 TB/s, the MI355X's specification).  Floor: x and y in and the cotangent bands out for the forward; the
cotangent bands in and dx, dy out for the backward -- with P the bytes of one image a level-j band tensor holds 12 P / 4^j, so
the op moves 2 (2 + 2 * 12 (1/4 + 1/16 + 1/64)) P = 19.75 P (the lowpass planes between the launches are not counted).
Method (tools/dwt_bench.py's): 5 warm-up runs of each, then 7 batches of 20 runs each, the two candidates' batches alternating,
timed with device events around the batch; outputs are not read back between runs.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import faoctasr                          # noqa: E402
from dwt_bench import timed_pair         # noqa: E402
import test_dtcwt_loss_cpu as R          # noqa: E402

SHAPES = ((8, 1, 256, 256), (64, 1, 256, 256), (8, 1, 512, 512))
BIAS, J = 1e-2, 3


def composed(ops, fwd, x, y):
    hx, hy = fwd(x)[1], fwd(y)[1]
    acc = None
    for a, b in zip(hx, hy):
        ra = torch.sqrt(a[..., 0] ** 2 + a[..., 1] ** 2 + BIAS * BIAS)
        rb = torch.sqrt(b[..., 0] ** 2 + b[..., 1] ** 2 + BIAS * BIAS)
        t = ops.l1_loss(ra, rb)
        acc = t if acc is None else acc + t
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtcwt_loss_bench.txt"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    faoctasr._lib.load()
    ops = faoctasr.ops
    fb, fq = R.tuples("a")
    crit = faoctasr.DTCWTMagnitudeLoss(biort=fb, qshift=fq, J=J).cuda()
    fwd = faoctasr.DTCWTForward(biort=fb, qshift=fq, J=J).cuda()
    lines = ["DTCWT magnitude loss, near_sym_a (5, 7 taps) + qshift_a (10 taps), 'symmetric', J = 3, forward + backward to both images: csrc/dtcwt_loss.hip",
             "against two DTCWTForward + torch magnitudes + ops.l1_loss, on the same card; device: %s; median [min, max] ms of 7 batches of 20 runs;"
             % torch.cuda.get_device_name(0), "spread = (max - min) / median of the batches, fused / composed", ""]
    for shape in SHAPES:
        xg = torch.randn(*shape, device="cuda").requires_grad_(True)
        yg = torch.randn(*shape, device="cuda").requires_grad_(True)
        mb = 19.75 * xg.numel() * 4 / 1e6
        with torch.no_grad():
            lf, lc = float(crit(xg, yg)), float(composed(ops, fwd, xg, yg))
        assert abs(lf - lc) <= 1e-5 * abs(lc), (lf, lc)                 # the two candidates compute the same thing

        def step(fn):
            def run():
                xg.grad = yg.grad = None
                fn().backward()
            return run

        (m, lo, hi), (tm, tlo, thi) = timed_pair(step(lambda: crit(xg, yg)), step(lambda: composed(ops, fwd, xg, yg)))
        gbs = mb / 1e3 / (m / 1e3)
        lines.append("%-16s fused %.4f [%.4f, %.4f]  composed %.4f [%.4f, %.4f]  ratio %5.2fx  spread %4.1f%% / %4.1f%%  %6.1f MB  %7.1f GB/s = %4.1f%% of HBM rate"
                     % ("x".join(map(str, shape)), m, lo, hi, tm, tlo, thi, tm / m, 100 * (hi - lo) / m, 100 * (thi - tlo) / tm, mb, gbs,
                        100 * gbs / (args.hbm_tbs * 1e3)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
