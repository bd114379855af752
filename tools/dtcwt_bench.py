"""Time the dual-tree complex wavelet transform (csrc/dtcwt.hip) against the torch composition it replaces.

    python tools/dtcwt_bench.py [--out profiles/dtcwt_bench.txt]

near_sym_a + qshift_a (the defaults; taps from the test fixtures), 'symmetric', shapes (8,1,256,256), (64,1,256,256), (8,1,512,512):
  * each of the four kernels alone: level-1 forward and inverse on the image, level-2 forward and inverse on its lowpass;
  * ``DTCWTForward(J=3)`` forward + backward (a cotangent on every output);
  * the same through the plain-torch restatement of tests/test_dtcwt_cpu.py (index-gather extension, one multiply-add pass per
    tap, stack / slice interleaves and q2c, its backward the restated inverse) run on the GPU in fp32;
  * the traffic floor over the time, in GB/s and as a share of the HBM rate given by ``--hbm-tbs`` (8.0 TB/s, the MI355X's
    specification).  Floor: a level-1 kernel moves 1 plane one way and 4 planes' worth the other (ll + 12 real planes at a
    quarter of the resolution), a level >= 2 kernel 1 plane in and 1 plane out, counted on that level's input plane.
Method (tools/dwt_bench.py's): 5 warm-up runs of each, then the median of 7 batches of 20 runs each, the two candidates' batches
alternating, timed with device events around the batch; outputs are not read back between runs.
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
import test_dtcwt_cpu as R               # noqa: E402

SHAPES = ((8, 1, 256, 256), (64, 1, 256, 256), (8, 1, 512, 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtcwt_bench.txt"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    faoctasr._lib.load()
    ops = faoctasr.ops
    (fb, fq), (ib, iq) = R.tuples("a")
    b = {k: v.float().cuda() for k, v in R.bufs("a").items()}
    lines = ["DTCWT, near_sym_a (5, 7 taps) + qshift_a (10 taps), 'symmetric': csrc/dtcwt.hip against the plain-torch restatement on the same card,",
             "device: %s; median [min, max] ms of 7 batches of 20 runs; floor: level 1 = 1 plane + 4 planes, level 2 = 1 plane + 1 plane" % torch.cuda.get_device_name(0), ""]

    def row(shape, what, hip, ref, mb):
        (m, lo, hi), (tm, tlo, thi) = timed_pair(hip, ref)
        gbs = mb / 1e3 / (m / 1e3)
        lines.append("%-16s %-22s %.4f [%.4f, %.4f]  torch %.4f [%.4f, %.4f]  %6.1f MB  %7.1f GB/s = %4.1f%% of HBM rate  %5.1fx"
                     % ("x".join(map(str, shape)), what, m, lo, hi, tm, tlo, thi, mb, gbs, 100 * gbs / (args.hbm_tbs * 1e3), tm / m))
        print(lines[-1], flush=True)

    for shape in SHAPES:
        x = torch.randn(*shape, device="cuda")
        plane = x.numel() * 4 / 1e6
        fwd = faoctasr.DTCWTForward(biort=fb, qshift=fq, J=3).cuda()
        inv = faoctasr.DTCWTInverse(biort=ib, qshift=iq).cuda()
        with torch.no_grad():
            ll1, h1 = ops.dtcwt_fwd_j1(x, fwd.h0o, fwd.h1o)
            ll2, h2 = ops.dtcwt_fwd_j2(ll1, fwd.h0a, fwd.h0b, fwd.h1a, fwd.h1b)
            row(shape, "fwd_j1", lambda: ops.dtcwt_fwd_j1(x, fwd.h0o, fwd.h1o), lambda: R.fwd_j1(x, b["h0o"], b["h1o"], True), 5 * plane)
            row(shape, "inv_j1", lambda: ops.dtcwt_inv_j1(ll1, h1, inv.g0o, inv.g1o), lambda: R.inv_j1(ll1, h1, b["g0o"], b["g1o"], True), 5 * plane)
            row(shape, "fwd_j2", lambda: ops.dtcwt_fwd_j2(ll1, fwd.h0a, fwd.h0b, fwd.h1a, fwd.h1b),
                lambda: R.fwd_j2(ll1, b["h0a"], b["h0b"], b["h1a"], b["h1b"]), 2 * plane)
            row(shape, "inv_j2", lambda: ops.dtcwt_inv_j2(ll2, h2, inv.g0a, inv.g0b, inv.g1a, inv.g1b),
                lambda: R.inv_j2(ll2, h2, b["g0a"], b["g0b"], b["g1a"], b["g1b"]), 2 * plane)
        xg = x.clone().requires_grad_(True)
        yl, yh = fwd(xg)
        cots = [torch.randn_like(t) for t in [yl] + yh]

        def hip_step():
            xg.grad = None
            yl, yh = fwd(xg)
            torch.autograd.backward([yl] + yh, cots)

        def torch_step():
            xg.grad = None
            yl, yh = R.forward_levels(xg, b, "symmetric", 3)
            torch.autograd.backward([yl] + yh, cots)

        row(shape, "J=3 fwd + bwd", hip_step, torch_step, 2 * (5 + 2 / 4 + 2 / 16) * plane)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
