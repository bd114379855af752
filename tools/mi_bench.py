"""Time forward + backward (gradients to both images) of the differentiable mutual information (ops.mutual_information,
csrc/mi.hip) against the torch composition of its definition on the same GPU (Gaussian Parzen windows by softmax, the joint
histogram by bmm, autograd), and record the peak device memory of both.

One child process per (shape, bins) under a time limit (a fault in one ends the run, nothing is started after it).  In it the two
paths alternate: ``--rounds`` batches of ``--reps`` repetitions each, HIP events around every repetition, warm-up first; a
batch's figure is its median and the summary gives the median of the batches' medians with their spread.
``torch.cuda.max_memory_allocated`` is read per path after its first batch, on top of the inputs, which both paths share.  The
traffic floor is what any implementation must move: x and y read once per direction, both gradients written once -- 24 bytes a
pixel -- as a share of 8 TB/s.

    python tools/mi_bench.py [--shapes 8x1x256x256,64x1x256x256,8x1x512x512] [--bins 32,64] [--out profiles/mi_bench.txt]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/mi_bench.py --child --shape 8x1x256x256 --bins 32      # the kernels' shares
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def inputs(shape):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    x = torch.clamp(2 * F.avg_pool2d(torch.randn(*shape, generator=g), 5, stride=1, padding=2), -1, 1)
    y = torch.clamp(0.8 * x ** 3 - 0.1 + 0.15 * torch.randn(*shape, generator=g), -1, 1)
    return x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)


def torch_mi(x, y, bins, sigma_ratio=1.0, eps=1e-6):
    import torch
    N, C, H, W = x.shape
    d = 2.0 / bins
    c = -1.0 + (torch.arange(bins, dtype=x.dtype, device=x.device) + 0.5) * d
    sigma = sigma_ratio * d

    def weights(v):
        return torch.softmax(-(v.reshape(N * C, H * W, 1) - c) ** 2 / (2 * sigma ** 2), dim=-1)

    P = torch.bmm(weights(x).transpose(1, 2), weights(y)) / (H * W)
    pa, pb = P.sum(2), P.sum(1)
    Ha, Hb = -(pa * torch.log(pa + eps)).sum(1), -(pb * torch.log(pb + eps)).sum(1)
    Hab = -(P * torch.log(P + eps)).sum((1, 2))
    return (Ha + Hb - Hab).mean()


def batch(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def child(shape, bins, reps, rounds):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    x, y = inputs(shape)

    def hip():
        x.grad = y.grad = None
        faoctasr.ops.mutual_information(x, y, bins).backward()

    def composed():
        x.grad = y.grad = None
        torch_mi(x, y, bins).backward()

    paths = {"hip": hip, "torch": composed}
    med = {k: [] for k in paths}
    peak = {}
    for k, fn in paths.items():                     # warm-up and the memory figure, one path at a time
        x.grad = y.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    for _ in range(rounds):
        for k, fn in paths.items():
            med[k].append(batch(fn, reps))
    n = 1
    for s in shape:
        n *= s
    floor = 24 * n
    out = {"shape": list(shape), "bins": bins, "reps": reps, "rounds": rounds, "floor_bytes": floor}
    for k in paths:
        m = statistics.median(med[k])
        out[k] = {"median_ms": m, "spread_ms": [min(med[k]), max(med[k])], "peak_bytes_above_inputs": peak[k],
                  "floor_share_of_8TBps": floor / HBM_BYTES_PER_S / (m * 1e-3)}
    out["faster_by_more_than_the_spread"] = max(med["hip"]) < min(med["torch"])
    out["slower_by_more_than_the_spread"] = min(med["hip"]) > max(med["torch"])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x1x256x256,64x1x256x256,8x1x512x512")
    ap.add_argument("--shape", default="8x1x256x256", help="the one shape of a --child run")
    ap.add_argument("--bins", default="32,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7, help="the two paths alternate this many batches per shape")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi_bench.txt"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        child(tuple(int(s) for s in a.shape.split("x")), int(a.bins), a.reps, a.rounds)
        return
    lines = ["Mutual information (Gaussian Parzen windows, sigma_ratio 1, range (-1, 1)), forward + backward to both images: csrc/mi.hip",
             "against softmax + bmm + autograd in torch on the same card; medians of %d alternating batches of %d repetitions, [spread];"
             % (a.rounds, a.reps),
             "peak = torch.cuda.max_memory_allocated above the inputs; floor = 24 bytes a pixel (x, y read per direction, dx, dy written) at 8 TB/s",
             ""]
    for text in a.shapes.split(","):
        for bins in a.bins.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", text, "--bins", bins, "--reps", str(a.reps),
                                "--rounds", str(a.rounds)], timeout=a.limit, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit("the measurement of %s, %s bins ended with status %d: stopping" % (text, bins, r.returncode))
            d = json.loads(r.stdout.strip().splitlines()[-1])
            h, t = d["hip"], d["torch"]
            verdict = "FASTER" if d["faster_by_more_than_the_spread"] else ("SLOWER" if d["slower_by_more_than_the_spread"] else "within the spread")
            line = ("%-14s K=%-2s  hip %.3f ms [%.3f, %.3f] peak %8.2f MiB floor share %5.2f%%  |  torch %.3f ms [%.3f, %.3f] peak %9.2f MiB  |  "
                    "%.2fx  %s" % (text, bins, h["median_ms"], h["spread_ms"][0], h["spread_ms"][1], h["peak_bytes_above_inputs"] / 2 ** 20,
                                   100 * h["floor_share_of_8TBps"], t["median_ms"], t["spread_ms"][0], t["spread_ms"][1],
                                   t["peak_bytes_above_inputs"] / 2 ** 20, t["median_ms"] / h["median_ms"], verdict))
            print(line, flush=True)
            lines.append(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
