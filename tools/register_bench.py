"""Time ``ops.phase_correlation`` (upsample 10) alone, and followed by ``ops.fourier_shift`` of the second image by the shift it found,
against the fp32 torch composition of the same definition on the same GPU (``torch.fft.rfft2`` / ``irfft2``, device-side arg-max, a
``matmul`` refinement with tables built on the device from the peak, a phase ramp for the shift).  Neither side reads anything back.

One child process per shape under a time limit (a fault in one ends the run, nothing is started after it).  Inside it the
measurements alternate: ``--rounds`` (7) batches of ``--reps`` (20) repetitions each, HIP events around each batch, warm-up first;
the figure of a batch is its mean per repetition, the reported figure the median over the batches, with their spread.  Peak memory
is ``torch.cuda.max_memory_allocated`` above what is allocated once the inputs exist (tables included, they are built in the warm-up).

    python tools/register_bench.py [--shapes 8x1x256x256,64x1x256x256,8x1x512x512] [--out profiles/register_bench.txt]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("hip_pc", "torch_pc", "hip_pc_shift", "torch_pc_shift")
EPS, U, MAX_SHIFT, D = 1e-16, 10, 8, (-2.3, 1.7)


def smooth(t, r):
    import torch
    return sum(torch.roll(t, (dy, dx), (-2, -1)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / (2 * r + 1) ** 2


def child(shape, reps, rounds):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    N, C, H, W = shape
    Wh, T = W // 2 + 1, -(-3 * U // 2)
    g = torch.Generator().manual_seed(0)
    rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64)
    a = (2 * smooth(rn(), 2) + 0.25 * rn()).float().cuda()
    b0 = faoctasr.fourier_shift(a, D).double().cpu() + 0.3 * rn()
    b = (0.7 * smooth(b0, 1) + 0.3 * b0).float().cuda()
    signed = lambda n: ((torch.arange(n) + n // 2) % n - n // 2).cuda()
    pos = lambda n: torch.where(torch.arange(n) > n // 2, torch.arange(n) - n, torch.arange(n)).cuda()
    wy, wx, py, px = signed(H), signed(W)[:Wh], pos(H), pos(W)
    window = torch.where((py.abs()[:, None] <= MAX_SHIFT) & (px.abs()[None, :] <= MAX_SHIFT), 0.0, -math.inf).cuda()
    mv = torch.full((Wh,), 2.0, device="cuda")
    mv[0] = 1
    if W % 2 == 0:
        mv[W // 2] = 1
    j = (torch.arange(T) - T // 2).cuda()

    def torch_pc():
        F, G = torch.fft.rfft2(a), torch.fft.rfft2(b)
        R = G * F.conj() / (H * W)
        Rn = (R / torch.sqrt(R.real ** 2 + R.imag ** 2 + EPS)).sum(1)
        surf = torch.fft.irfft2(Rn, s=(H, W)) + window
        idx = surf.flatten(1).argmax(1)
        sy, sx = py[idx // W], px[idx % W]
        ey = torch.polar(torch.ones((), device="cuda"), (2 * math.pi / (U * H)) * ((wy[None, None, :] * (sy[:, None, None] * U + j[None, :, None])) % (U * H)).float())
        ex = torch.polar(torch.ones((), device="cuda"), (2 * math.pi / (U * W)) * ((wx[None, :, None] * (sx[:, None, None] * U + j[None, None, :])) % (U * W)).float())
        up = (ey @ (Rn * mv) @ ex).real / (H * W * C)
        k = up.flatten(1).argmax(1)
        shift = torch.stack(((sy * U + j[k // T]).float() / U, (sx * U + j[k % T]).float() / U), 1)
        return shift, up.flatten(1).gather(1, k[:, None])[:, 0]

    def torch_shift(x, d):
        ph = wy[None, :, None] * d[:, 0, None, None] / H + wx[None, None, :] * d[:, 1, None, None] / W
        ramp = torch.polar(torch.ones((), device="cuda"), -2 * math.pi * ph)[:, None]
        return torch.fft.irfft2(torch.fft.rfft2(x) * ramp, s=(H, W))

    def hip_both():
        d, _ = faoctasr.phase_correlation(a, b, U, MAX_SHIFT)
        return faoctasr.fourier_shift(b, -d)

    runs = {"hip_pc": lambda: faoctasr.phase_correlation(a, b, U, MAX_SHIFT), "torch_pc": torch_pc, "hip_pc_shift": hip_both,
            "torch_pc_shift": lambda: torch_shift(b, -torch_pc()[0])}
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        for k in KINDS:                                                # warm-up: tables, caches, the allocator's pools
            for _ in range(5):
                runs[k]()
            torch.cuda.synchronize()
        found = {"hip": runs["hip_pc"]()[0][0].tolist(), "torch": runs["torch_pc"]()[0][0].tolist()}
        peak = {}
        for k in KINDS:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            runs[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - before
        ms = {k: [] for k in KINDS}
        for _ in range(rounds):
            for k in KINDS:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(reps):
                    runs[k]()
                e.record()
                e.synchronize()
                ms[k].append(s.elapsed_time(e) / reps)
    out = {"shape": list(shape), "reps": reps, "rounds": rounds, "upsample": U, "max_shift": MAX_SHIFT, "displacement": list(D),
           "shift_found": found, "inputs_bytes": base}
    for k in KINDS:
        out[k] = {"median_ms": statistics.median(ms[k]), "spread_ms": [min(ms[k]), max(ms[k])], "peak_bytes_above_inputs": peak[k]}
    for what in ("pc", "pc_shift"):
        out["hip_faster_%s_by_more_than_the_spread" % what] = max(ms["hip_" + what]) < min(ms["torch_" + what])
        out["torch_faster_%s_by_more_than_the_spread" % what] = max(ms["torch_" + what]) < min(ms["hip_" + what])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x1x256x256,64x1x256x256,8x1x512x512")
    ap.add_argument("--shape", default=None, help="the one shape of a --child run")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    a = ap.parse_args()
    if a.child:
        child(tuple(int(s) for s in a.shape.split("x")), a.reps, a.rounds)
        return
    for text in a.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", text, "--reps", str(a.reps), "--rounds", str(a.rounds)],
                           timeout=a.limit, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit("the measurement of %s ended with status %d: stopping" % (text, r.returncode))
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
