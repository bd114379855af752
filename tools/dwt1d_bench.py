"""Time the 1-D DWT (csrc/dwt1d.hip) against the torch composition it replaces and its two launch shapes against each other.

    python tools/dwt1d_bench.py [--out profiles/dwt1d_bench.txt]

db4, 'symmetric', J = 1 and 3, row sets 64 x 256, 8*64*256 x 256, 64 x 16384 and 8 x 262144 (rows x samples):
  * ``DWT1DForward(J)`` forward alone, and forward + backward (a cotangent on every output), with the launch ``fused=None`` picks;
  * the same through the reference's scheme restated on the GPU: per level an index-gather pad and a stride-2 ``F.conv1d`` on the
    (lo, hi) pair, the backward a ``F.conv_transpose1d`` on the same taps and a crop (the reference's definition), levels
    chained as the reference chains them;
  * where a row fits the fused launch, the forced tiled launch (``fused=False``, a launch per level) against the fused one;
  * the traffic floor -- x read once and every coefficient written once, the same again backward -- over the time, in GB/s and
    as a fraction of the HBM rate given by ``--hbm-tbs`` (8.0 TB/s, the MI355X's specification).
Method (tools/dwt_bench.py's): 5 warm-up runs of each, then the median of 7 batches of 20 runs each, the two candidates'
batches alternating, timed with device events around the batch; outputs are not read back between runs.
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


class TorchLevel(torch.autograd.Function):
    """One 'symmetric' analysis level of rows x[R, 1, n] with the reversed (correlation) taps w[2, 1, L] -> [R, 2, O]."""

    @staticmethod
    def forward(ctx, x, w):
        n, L = x.shape[-1], w.shape[-1]
        O = (n + L - 1) // 2
        base = (2 * (O - 1) - n + L) // 2
        m = np.mod(np.arange(2 * (O - 1) + L) - base, 2 * n)
        idx = torch.from_numpy(np.where(m < n, m, 2 * n - 1 - m)).long().to(x.device)
        ctx.save_for_backward(w)
        ctx.n = n
        return F.conv1d(x.index_select(2, idx), w, stride=2)

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        L = w.shape[-1]
        return F.conv_transpose1d(dy, w, stride=2)[..., L - 2:L - 2 + ctx.n].contiguous(), None


def torch_levels(x, w, J):
    """(lo, [hi_j]) of rows x[R, 1, n], the strided band slices made contiguous as the reference makes them."""
    his, lo = [], x
    for _ in range(J):
        lohi = TorchLevel.apply(lo, w)
        lo, hi = lohi[:, 0:1].contiguous(), lohi[:, 1:2].contiguous()
        his.append(hi)
    return lo, his


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwt1d_bench.txt"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    faoctasr._lib.load()
    wave = faoctasr.daubechies(4)
    ops = faoctasr.ops
    lines = ["1-D DWT, db4 (8 taps), 'symmetric': csrc/dwt1d.hip against a torch composition (gather pad + stride-2 conv1d, conv_transpose1d backward),",
             "and its fused launch (all levels of a row in LDS, rows up to %d samples) against its tiled one (a launch per level)" % faoctasr.DWT1D_FUSED_MAX,
             "device: %s; median [min, max] ms of 7 batches of 20 runs; floor = x read once, every coefficient written once, per direction" % torch.cuda.get_device_name(0), ""]
    for rows, n in ((64, 256), (8 * 64 * 256, 256), (64, 16384), (8, 262144)):
        for J in (1, 3):
            fwd = faoctasr.DWT1DForward(J=J, wave=wave, mode="symmetric").cuda()
            x = torch.randn(1, rows, n, device="cuda").requires_grad_(True)
            xt = x.detach().reshape(rows, 1, n).requires_grad_(True)
            w = torch.cat((fwd.h0, fwd.h1), dim=0)
            yl, yh = fwd(x)
            outs = [yl] + list(yh)
            cots = [torch.randn_like(t) for t in outs]
            cots_t = [c.reshape(rows, 1, -1) for c in cots]
            fits = n <= faoctasr.DWT1D_FUSED_MAX

            def run(fused):
                lo, his = ops.dwt1d_analysis(x, fwd.h0, fwd.h1, 1, J, fused=fused)
                return [lo] + his

            def hip_f(fused=None):
                with torch.no_grad():
                    return run(fused)

            def torch_f():
                with torch.no_grad():
                    lo, his = torch_levels(xt, w, J)
                    return [lo] + his

            def hip_fb(fused=None):
                x.grad = None
                torch.autograd.backward(run(fused), cots)

            def torch_fb():
                xt.grad = None
                lo, his = torch_levels(xt, w, J)
                torch.autograd.backward([lo] + his, cots_t)

            for a, b in zip(hip_f(), torch_f()):            # the composition computes what the kernels compute
                assert float((a.reshape(-1) - b.reshape(-1)).abs().max()) < 1e-4
            hip_fb()
            torch_fb()
            assert float((x.grad.reshape(-1) - xt.grad.reshape(-1)).abs().max()) < 1e-3
            floor = 4 * (x.numel() + sum(t.numel() for t in outs))
            tag = "%dx%d" % (rows, n)
            for name, f, t, nbytes in (("forward", hip_f, torch_f, floor), ("forward+backward", hip_fb, torch_fb, 2 * floor)):
                mf, mt = timed_pair(f, t)
                gbs = nbytes / (mf[0] * 1e-3) / 1e9
                verdict = "%.2fx the composition's speed" % (mt[0] / mf[0]) + ("" if mf[0] <= mt[0] else "  ** the kernels lose here **")
                lines.append("%-14s J=%d %-17s %-5s %.4f [%.4f, %.4f]  torch %.4f [%.4f, %.4f]  %6.1f MB  %7.1f GB/s = %4.1f%% of HBM rate  %s"
                             % (tag, J, name, "fused" if fits else "tiled", mf[0], mf[1], mf[2], mt[0], mt[1], mt[2], nbytes / 1e6, gbs,
                                100 * gbs / (args.hbm_tbs * 1e3), verdict))
                print(lines[-1], flush=True)
                if fits:
                    mf, mt = timed_pair(lambda: f(True), lambda: f(False))
                    verdict = "fused %.2fx the tiled launch's speed" % (mt[0] / mf[0]) + ("" if mf[0] <= mt[0] else "  ** the fused launch loses here **")
                    lines.append("%-14s J=%d %-17s fused %.4f [%.4f, %.4f]  tiled %.4f [%.4f, %.4f]  %s"
                                 % (tag, J, name, mf[0], mf[1], mf[2], mt[0], mt[1], mt[2], verdict))
                    print(lines[-1], flush=True)
            del x, xt, yl, yh, outs, cots, cots_t
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
