"""Time the DTCWT scattering layers (csrc/scat.hip) against what they replace.

    python tools/scat_bench.py [--out profiles/scat_bench.txt]

near_sym_a + qshift_a (taps from the test fixtures), 'symmetric', magbias 1e-2, shapes (8,1,256,256), (64,1,256,256), (8,1,512,512);
``ScatLayer`` and ``ScatLayerj2`` forward + backward (a cotangent on Z), against two candidates:
  (a) the composition the package offered before the fused kernels: ``ops.dtcwt_fwd_j1`` / ``dtcwt_fwd_j2`` (their backward passes
      are ``dtcwt_inv_j1`` / ``dtcwt_inv_j2``) with torch ops for the magnitude -- an autograd function that keeps the unit phasors,
      as the reference's does --, the pooling, its upsampling adjoint and the concatenation;
  (b) the plain-torch restatement of tests/test_scat_cpu.py run on the GPU in fp32.
A row: median [min, max] ms of the fused layer and of the candidate, the ratio of the medians, the spread (max - min) / median of
the seven batches of either, and the traffic floor over the fused time in GB/s and as a share of the HBM rate given by
``--hbm-tbs`` (8.0 TB/s, the MI355X's specification).  Floor: x in, Z and the phasors out for the forward; dZ and the phasors in,
dX out for the backward -- with P the bytes of x, ``ScatLayer`` moves 2 (1 + 7/4 + 12/4) P and ``ScatLayerj2``
2 (1 + 49/16 + 12/4 + 12/16 + 72/16) P (its temporaries between the three launches are not counted).
Method (tools/dwt_bench.py's): 5 warm-up runs of each, then 7 batches of 20 runs each, the two candidates' batches alternating,
timed with device events around the batch; outputs are not read back between runs.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F
from torch.autograd import Function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import faoctasr                          # noqa: E402
from dwt_bench import timed_pair         # noqa: E402
import test_scat_cpu as R                # noqa: E402

SHAPES = ((8, 1, 256, 256), (64, 1, 256, 256), (8, 1, 512, 512))
BIAS = 1e-2


class SmoothMag(Function):
    """h (.., 2) -> sqrt(re^2 + im^2 + b^2) - b, the unit phasors kept for the backward."""

    @staticmethod
    def forward(ctx, h, b):
        r = torch.sqrt(h[..., 0] ** 2 + h[..., 1] ** 2 + b * b)
        ctx.save_for_backward(h / r.unsqueeze(-1))
        return r - b

    @staticmethod
    def backward(ctx, dr):
        return dr.unsqueeze(-1) * ctx.saved_tensors[0], None


def composed1(ops, m, x):
    N, C = x.shape[:2]
    ll, h = ops.dtcwt_fwd_j1(x, m.h0o, m.h1o, False, 1, -1, 1)                   # h (N, 6, C, h, w, 2)
    Z = torch.cat((F.avg_pool2d(ll, 2)[:, None], SmoothMag.apply(h, BIAS)), 1)
    return Z.view(N, 7 * C, Z.shape[3], Z.shape[4])


def composed2(ops, m, x):
    N, C = x.shape[:2]
    s0, h = ops.dtcwt_fwd_j1(x, m.h0o, m.h1o, False, 1, -1, 1)
    m1 = SmoothMag.apply(h, BIAS)                                                # (N, 6, C, h2, w2)
    ll2, h = ops.dtcwt_fwd_j2(s0, m.h0a, m.h0b, m.h1a, m.h1b, False, 1, -1)
    m2 = SmoothMag.apply(h, BIAS)                                                # (N, 6, C, h4, w4)
    l1, h = ops.dtcwt_fwd_j1(m1.view(N, 6 * C, m1.shape[3], m1.shape[4]), m.h0o, m.h1o, False, 1, -1, 1)
    hw = tuple(m2.shape[3:])
    m21 = SmoothMag.apply(h, BIAS).view((N, 36, C) + hw)
    Z = torch.cat((F.avg_pool2d(ll2, 2)[:, None], F.avg_pool2d(l1, 2).view((N, 6, C) + hw), m2, m21), 1)
    return Z.view((N, 49 * C) + hw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scat_bench.txt"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    faoctasr._lib.load()
    ops = faoctasr.ops
    fb, fq = R.tuples("a")
    b = {k: v.float().cuda() for k, v in R.bufs("a").items()}
    one, two = faoctasr.ScatLayer(biort=fb).cuda(), faoctasr.ScatLayerj2(biort=fb, qshift=fq).cuda()
    lines = ["Scattering layers, near_sym_a (5, 7 taps) + qshift_a (10 taps), 'symmetric', forward + backward: csrc/scat.hip against (a) the dtcwt kernels",
             "composed with torch ops and (b) the plain-torch restatement, on the same card; device: %s; median [min, max] ms of 7 batches of 20 runs;"
             % torch.cuda.get_device_name(0), "spread = (max - min) / median of the batches, fused / candidate", ""]

    def row(shape, what, cand, hip, ref, mb):
        (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
        gbs = mb / 1e3 / (m / 1e3)
        lines.append("%-16s %-12s fused %.4f [%.4f, %.4f]  %-12s %.4f [%.4f, %.4f]  ratio %5.2fx  spread %4.1f%% / %4.1f%%  %6.1f MB  %7.1f GB/s = %4.1f%% of HBM rate"
                     % ("x".join(map(str, shape)), what, m, lo, hi, cand, tm, tlo, thi, tm / m, 100 * (hi - lo) / m, 100 * (thi - tlo) / tm, mb, gbs,
                        100 * gbs / (args.hbm_tbs * 1e3)))
        print(lines[-1], flush=True)

    for shape in SHAPES:
        xg = torch.randn(*shape, device="cuda").requires_grad_(True)
        plane = xg.numel() * 4 / 1e6
        for what, fused, comp, plain, mb in (
                ("ScatLayer", one, lambda t: composed1(ops, one, t), lambda t: R.layer1(t, b, "symmetric"), 2 * (1 + 7 / 4 + 3) * plane),
                ("ScatLayerj2", two, lambda t: composed2(ops, two, t), lambda t: R.layer2(t, b), 2 * (1 + 49 / 16 + 3 + 12 / 16 + 72 / 16) * plane)):
            cot = torch.randn_like(fused(xg))

            def step(fn, cot=cot):
                def run():
                    xg.grad = None
                    fn(xg).backward(cot)
                return run

            row(shape, what, "(a) composed", step(fused), step(comp), mb)
            row(shape, what, "(b) torch", step(fused), step(plain), mb)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
