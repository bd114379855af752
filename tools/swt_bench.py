"""Time the fused stationary wavelet transform (csrc/swt.hip) against the torch composition it replaces, on the GPU.

    python tools/swt_bench.py [--out profiles/swt_bench.txt]

Per shape (8x1x256x256, 64x1x256x256, 8x64x128x128), db4, 'periodic', J = 1 and J = 3:
  * ``SWTForward(J)`` forward alone, and forward + backward (a cotangent on every level), fused;
  * the same through the reference's composition written here: an index-gather pad of (L d / 2 - d, L d / 2) and a grouped
    dilated ``F.conv2d`` per axis, levels chained on band 0, autograd for the backward;
  * the fused path's traffic floor -- per level one plane read and four written, 5 planes, the same again backward -- over its
    time, in GB/s and as a fraction of the HBM rate given by ``--hbm-tbs`` (8.0 TB/s, the MI355X's specification).
Method: 5 warm-up runs of each, then the median of 7 batches of 20 runs each, fused and composition batches alternating, timed
with device events around the batch; outputs are not read back between runs.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faoctasr                          # noqa: E402
from dwt_bench import timed_pair         # noqa: E402


def torch_level(x, h0, h1, d):
    """One periodic a-trous level on x[N,C,H,W] with the reversed (correlation) taps: wrap-pad W, grouped dilated conv; then H."""
    N, C, H, W = x.shape
    L = h0.numel()
    lo, hi = L * d // 2 - d, L * d // 2
    iw = torch.from_numpy(np.mod(np.arange(-lo, W + hi), W)).long().to(x.device)
    ih = torch.from_numpy(np.mod(np.arange(-lo, H + hi), H)).long().to(x.device)
    w = torch.stack((h0, h1)).reshape(2, 1, 1, L).repeat(C, 1, 1, 1)
    lohi = F.conv2d(x.index_select(3, iw), w, groups=C, dilation=d)
    w2 = torch.stack((h0, h1)).reshape(2, 1, L, 1).repeat(2 * C, 1, 1, 1)
    return F.conv2d(lohi.index_select(2, ih), w2, groups=2 * C, dilation=d).reshape(N, C, 4, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swt_bench.txt"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    faoctasr._lib.load()
    w = faoctasr.daubechies(4)
    lines = ["stationary wavelet transform, db4 (8 taps), 'periodic': fused HIP kernels against a torch composition (gather pad + grouped dilated conv)",
             "device: %s; median [min, max] ms of 7 batches of 20 runs; floor = 5 planes per level and direction" % torch.cuda.get_device_name(0), ""]
    for shape in ((8, 1, 256, 256), (64, 1, 256, 256), (8, 64, 128, 128)):
        for J in (1, 3):
            fwd = faoctasr.SWTForward(J=J, wave=w, mode="periodic").cuda()
            x = torch.randn(shape, device="cuda").requires_grad_(True)
            ys = fwd(x)
            cots = [torch.randn_like(y) for y in ys]
            h0, h1 = fwd.h0_col.reshape(-1), fwd.h1_col.reshape(-1)

            def torch_levels(v):
                out = []
                for j in range(J):
                    y = torch_level(v, h0, h1, 1 << j)
                    out.append(y)
                    v = y[:, :, 0]
                return out

            def fused_f():
                with torch.no_grad():
                    return fwd(x)

            def torch_f():
                with torch.no_grad():
                    return torch_levels(x)

            def fused_fb():
                x.grad = None
                torch.autograd.backward(fwd(x), cots)

            def torch_fb():
                x.grad = None
                torch.autograd.backward(torch_levels(x), cots)

            for a, b in zip(ys, torch_f()):                 # the composition computes what the fused path computes
                assert float((a - b).abs().max()) < 1e-4
            fused_fb()
            g = x.grad.clone()
            torch_fb()
            assert float((g - x.grad).abs().max()) < 1e-3
            floor = 4 * 5 * x.numel() * J
            for name, f, t, nbytes in (("forward", fused_f, torch_f, floor), ("forward+backward", fused_fb, torch_fb, 2 * floor)):
                mf, mt = timed_pair(f, t)
                gbs = nbytes / (mf[0] * 1e-3) / 1e9
                verdict = "fused %.2fx the composition's speed" % (mt[0] / mf[0]) + ("" if mf[0] <= mt[0] else "  ** the fused path loses here **")
                lines.append("%-14s J=%d %-17s fused %.4f [%.4f, %.4f]  torch %.4f [%.4f, %.4f]  %6.1f MB  %7.1f GB/s = %4.1f%% of HBM rate  %s"
                             % ("x".join(map(str, shape)), J, name, mf[0], mf[1], mf[2], mt[0], mt[1], mt[2], nbytes / 1e6, gbs,
                                100 * gbs / (args.hbm_tbs * 1e3), verdict))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
