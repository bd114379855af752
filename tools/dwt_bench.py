"""Time the fused general DWT (csrc/dwt.hip) against the stock-op composition it replaces, on the GPU.

    python tools/dwt_bench.py [--out profiles/dwt_bench.txt]

Per shape (8x1x256x256, 8x64x128x128), db4, modes 'symmetric' and 'periodization':
  * ``DWTForward(J=3)`` forward + backward (cotangents on yl and every yh) and ``DWTInverse`` forward, fused;
  * the same through a torch composition written here: index-gather padding, grouped strided ``F.conv2d`` for the analysis,
    grouped ``F.conv_transpose2d`` for the synthesis, autograd for the backward (its backward is the true adjoint, the fused
    one the reference's definition: the same amount of work);
  * the fused path's compulsory traffic (every level reads its input once and writes its four bands once, forward and backward)
    over its time, as a fraction of the HBM rate given by ``--hbm-tbs`` (8.0 TB/s, the MI355X's specification).
Method: 5 warm-up runs of each, then the median of 7 batches of 20 runs each, fused and composition batches alternating,
timed with device events around the batch; outputs are not read back between runs.  The composition pads with even-sized 'periodization' only (both shapes are even at every level).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import faoctasr                          # noqa: E402


def timed_pair(fa, fb, warm=5, batches=7, runs=20):
    """(median, min, max) ms per run of ``fa`` and of ``fb``, their batches alternating in one loop: a drift of the clocks or a
    neighbour on the machine meets both alike."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(batches):
        for which, fn in enumerate((fa, fb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(runs):
                fn()
            e.record()
            e.synchronize()
            ms[which].append(s.elapsed_time(e) / runs)
    return tuple((float(np.median(m)), float(min(m)), float(max(m))) for m in ms)


def gather_index(N, L, mode, device):
    O = (N + L - 1) // 2
    base = (2 * (O - 1) - N + L) // 2
    j = np.arange(2 * (O - 1) + L) - base
    if mode == "symmetric":
        m = np.mod(j, 2 * N)
        idx = np.where(m < N, m, 2 * N - 1 - m)
    else:                               # periodization at an even N: a rotation by L/2 - 1 and a wrap
        idx = np.mod(np.arange(N + L - 2) - (L - 1) + L // 2, N)
    return torch.from_numpy(idx).long().to(device)


def torch_analysis(x, h0, h1, mode):
    """One level on x[N,C,H,W]: gather-pad W, grouped conv stride (1,2); gather-pad H, grouped conv stride (2,1)."""
    C, L = x.shape[1], h0.numel()
    w = torch.stack((h0, h1)).reshape(2, 1, 1, L).repeat(C, 1, 1, 1)
    lohi = F.conv2d(x.index_select(3, gather_index(x.shape[3], L, mode, x.device)), w, stride=(1, 2), groups=C)
    w2 = torch.stack((h0, h1)).reshape(2, 1, L, 1).repeat(2 * C, 1, 1, 1)
    y = F.conv2d(lohi.index_select(2, gather_index(x.shape[2], L, mode, x.device)), w2, stride=(2, 1), groups=2 * C)
    y = y.reshape(x.shape[0], C, 4, y.shape[-2], y.shape[-1])
    return y[:, :, 0].contiguous(), y[:, :, 1:].contiguous()


def torch_synthesis(ll, hi, g0, g1, mode):
    C, L = ll.shape[1], g0.numel()

    def one(lo, hh, dim):
        shape = (C, 1, L, 1) if dim == 2 else (C, 1, 1, L)
        s = (2, 1) if dim == 2 else (1, 2)
        a, b = g0.reshape(1, 1, -1).expand(C, 1, L).reshape(shape), g1.reshape(1, 1, -1).expand(C, 1, L).reshape(shape)
        if mode == "periodization":
            y = F.conv_transpose2d(lo, a, stride=s, groups=C) + F.conv_transpose2d(hh, b, stride=s, groups=C)
            n = 2 * lo.shape[dim]
            head = y.narrow(dim, 0, L - 2) + y.narrow(dim, n, L - 2)
            y = torch.cat((head, y.narrow(dim, L - 2, n - (L - 2))), dim=dim)
            return torch.roll(y, shifts=-(L // 2 - 1), dims=dim)
        pad = (L - 2, 0) if dim == 2 else (0, L - 2)
        return F.conv_transpose2d(lo, a, stride=s, padding=pad, groups=C) + F.conv_transpose2d(hh, b, stride=s, padding=pad, groups=C)
    lh, hl, hh = torch.unbind(hi, dim=2)
    return one(one(ll, lh, 2), one(hl, hh, 2), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwt_bench.txt"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    faoctasr._lib.load()
    w = faoctasr.daubechies(4)
    J = 3
    lines = ["general DWT, db4 (8 taps), J = %d: fused HIP kernels against a torch composition (gather pad + grouped strided conv)" % J,
             "device: %s; median [min, max] ms of 7 batches of 20 runs; HBM fraction = compulsory bytes / time / %.1f TB/s" % (torch.cuda.get_device_name(0), args.hbm_tbs), ""]
    for shape in ((8, 1, 256, 256), (8, 64, 128, 128)):
        for mode in ("symmetric", "periodization"):
            fwd, inv = faoctasr.DWTForward(J=J, wave=w, mode=mode).cuda(), faoctasr.DWTInverse(wave=w, mode=mode).cuda()
            x = torch.randn(shape, device="cuda").requires_grad_(True)
            yl, yh = fwd(x)
            cots = [torch.randn_like(t) for t in [yl] + list(yh)]
            h0, h1 = fwd.h0_col.reshape(-1), fwd.h1_col.reshape(-1)
            g0, g1 = inv.g0_col.reshape(-1), inv.g1_col.reshape(-1)

            def fused_fb():
                x.grad = None
                a, b = fwd(x)
                torch.autograd.backward([a] + list(b), cots)

            def torch_fb():
                x.grad = None
                ll, hs = x, []
                for _ in range(J):
                    ll, h = torch_analysis(ll, h0, h1, mode)
                    hs.append(h)
                torch.autograd.backward([ll] + hs, cots)

            cl, ch = yl.detach(), [h.detach() for h in yh]

            def fused_inv():
                return inv((cl, ch))

            def torch_inv():
                ll = cl
                for h in ch[::-1]:
                    if ll.shape[-2] > h.shape[-2]:
                        ll = ll[..., :-1, :]
                    if ll.shape[-1] > h.shape[-1]:
                        ll = ll[..., :-1]
                    ll = torch_synthesis(ll, h, g0, g1, mode)
                return ll
            # the composition computes what the fused path computes
            ll = x.detach()
            for h_fused in yh:
                ll, h = torch_analysis(ll, h0, h1, mode)
                assert float((h - h_fused).abs().max()) < 1e-4
            assert float((ll - yl).abs().max()) < 1e-4
            assert float((fused_inv() - torch_inv()).abs().max()) < 1e-4
            # compulsory traffic: per level, input once + four bands once, forward; the same again backward
            level_bytes = 0
            ll = x
            for h in yh:
                level_bytes += 4 * (ll.numel() + 4 * h.numel() // 3)
                ll = h[:, :, 0]
            for name, f, t, nbytes in (("forward+backward", fused_fb, torch_fb, 2 * level_bytes), ("inverse", fused_inv, torch_inv, level_bytes)):
                mf, mt = timed_pair(f, t)
                frac = nbytes / (mf[0] * 1e-3) / (args.hbm_tbs * 1e12)
                verdict = "fused %.2fx the composition's speed" % (mt[0] / mf[0]) + ("" if mf[0] <= mt[0] else "  ** the fused path loses here **")
                lines.append("%-16s %-14s %-17s fused %.4f [%.4f, %.4f]  torch %.4f [%.4f, %.4f]  %5.1f MB  %.1f%% of HBM rate  %s"
                             % ("x".join(map(str, shape)), mode, name, mf[0], mf[1], mf[2], mt[0], mt[1], mt[2], nbytes / 1e6, 100 * frac, verdict))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
