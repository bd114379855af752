"""Time forward + backward of the total-variation loss (ops.tv_loss) against the torch composition that ``TVLoss.forward`` was
before the fused op existed (restated below, so the comparison survives the change), on the same GPU.

Each measurement runs in a child process of its own under a time limit (a fault in one ends the run, nothing is started after
it); HIP events around each repetition, warm-up first, median reported.  ``--step`` additionally times a whole train step at
256x256, batch 8, with ``tv_weight`` 0 and 0.5.

    python tools/tv_loss_bench.py [--reps 50] [--rounds 2] [--step]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/tv_loss_bench.py --child hip --shape 8,1,256,256     # the kernels' shares
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 1, 256, 256), (8, 1, 256, 256), (8, 1, 512, 512))


def composition(x, weight=1):
    """``TVLoss.forward`` as it stood before ``ops.tv_loss``: ~8 ATen launches forward, ~10 backward, four strided temporaries."""
    b, c, h, w = x.shape
    count_h, count_w = c * (h - 1) * w, c * h * (w - 1)
    h_tv = ((x[:, :, 1:, :] - x[:, :, :h - 1, :]) ** 2).sum()
    w_tv = ((x[:, :, :, 1:] - x[:, :, :, :w - 1]) ** 2).sum()
    return weight * 2 * (h_tv / count_h + w_tv / count_w) / b


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


def child(kind, shape, reps):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    if kind == "step":
        import random
        B, H = 8, 256
        g = torch.Generator().manual_seed(7)
        a = (torch.rand(B, 1, H, H, generator=g) * 2 - 1).cuda()
        b = (torch.rand(B, 1, H, H, generator=g) * 2 - 1).cuda()
        out = {}
        for w in (0.0, 0.5):
            random.seed(1234)
            torch.manual_seed(0)
            ts = faoctasr.TrainStep(device="cuda", precision="f16x2", tv_weight=w)
            out["tv_weight_%g" % w] = timed(lambda: ts.step(a, b), max(reps // 3, 10), warmup=4)
            del ts
        print(json.dumps({"kind": kind, "batch": B, "size": H, **out}))
        return
    x = torch.tanh(torch.randn(*shape, generator=torch.Generator().manual_seed(0))).cuda().requires_grad_(True)
    fn = faoctasr.ops.tv_loss if kind == "hip" else composition

    def run():
        x.grad = None
        fn(x).backward()
    print(json.dumps({"kind": kind, "shape": list(shape), "bytes_min": 3 * 4 * x.numel(), **timed(run, reps)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="the two measurements of a shape alternate this many times")
    ap.add_argument("--step", action="store_true", help="also the train step at 256x256, batch 8, with tv_weight 0 and 0.5")
    ap.add_argument("--child", choices=["hip", "torch", "step"], default=None)
    ap.add_argument("--shape", default="8,1,256,256", help="B,C,H,W of a --child run")
    ap.add_argument("--limit", type=int, default=180, help="seconds per child process")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        child(a.child, tuple(int(v) for v in a.shape.split(",")), a.reps)
        return
    jobs = [(kind, shape) for shape in SHAPES for _ in range(a.rounds) for kind in ("hip", "torch")] + ([("step", SHAPES[1])] if a.step else [])
    for kind, shape in jobs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--shape", ",".join(map(str, shape)), "--reps", str(a.reps)],
                           timeout=a.limit, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit("the %s measurement ended with status %d: stopping" % (kind, r.returncode))
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
