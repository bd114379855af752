"""Time forward + backward of the spectral phase-consistency loss (ops.phase_loss) at the benchmark's image size against the
fp32 ``torch.fft`` composition of the same formula on the same GPU (mask built once, outside the timed region).

Each measurement runs in a child process of its own under a time limit (a fault in one ends the run, nothing is started after
it); HIP events around each repetition, warm-up first, median reported.  ``--step`` additionally times a whole train step
with and without the opt-in term.

    python tools/phase_loss_bench.py [--batch 8] [--size 256] [--reps 50] [--rounds 2] [--step]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/phase_loss_bench.py --child hip      # the kernels' shares
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(B, H):
    import torch
    g = torch.Generator().manual_seed(0)
    x = torch.tanh(torch.randn(B, 1, H, H, generator=g))
    y = torch.tanh(x + 0.3 * torch.randn(B, 1, H, H, generator=g))
    return x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)


def timed(fn, reps, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def child(kind, B, H, reps):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    if kind == "step":
        import random
        random.seed(1234)
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        a = (torch.rand(B, 1, H, H, generator=g) * 2 - 1).cuda()
        b = (torch.rand(B, 1, H, H, generator=g) * 2 - 1).cuda()
        out = {}
        for w in (0.0, 0.5):
            ts = faoctasr.TrainStep(device="cuda", precision="f16x2", phase_weight=w)
            out["phase_weight_%g" % w] = timed(lambda: ts.step(a, b), max(reps // 3, 10), warmup=4)
            del ts
        print(json.dumps({"kind": kind, "batch": B, "size": H, **out}))
        return
    x, y = inputs(B, H)
    if kind == "hip":
        def run():
            x.grad = y.grad = None
            faoctasr.ops.phase_loss(x, y, 5.0).backward()
    else:
        i = torch.arange(H, dtype=torch.float64)[:, None] - H // 2
        m = (1 - torch.exp(-0.5 * (i * i + i.T * i.T) / 25.0)).float().cuda()

        def run():
            x.grad = y.grad = None
            ax = (m * torch.log(torch.abs(torch.fft.fftshift(torch.fft.fft2(x), dim=(-2, -1))))).flatten(1)
            ay = (m * torch.log(torch.abs(torch.fft.fftshift(torch.fft.fft2(y), dim=(-2, -1))))).flatten(1)
            (-torch.cosine_similarity(ax, ay, dim=1)).mean().backward()
    print(json.dumps({"kind": kind, "batch": B, "size": H, **timed(run, reps)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="the two measurements alternate this many times")
    ap.add_argument("--step", action="store_true", help="also the train step with phase_weight 0 and 0.5 (information only)")
    ap.add_argument("--child", choices=["hip", "fft", "step"], default=None)
    ap.add_argument("--limit", type=int, default=180, help="seconds per child process")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        child(a.child, a.batch, a.size, a.reps)
        return
    kinds = ["hip", "fft"] * a.rounds + (["step"] if a.step else [])
    for kind in kinds:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--batch", str(a.batch), "--size", str(a.size),
                            "--reps", str(a.reps)], timeout=a.limit, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit("the %s measurement ended with status %d: stopping" % (kind, r.returncode))
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
