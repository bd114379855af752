"""Time forward + backward (gradients to both images) of the focal frequency loss (ops.focal_frequency_loss) against the fp32
``torch.fft`` composition of its definition on the same GPU (autograd, weight detached).

Each measurement runs in a child process of its own under a time limit (a fault in one ends the run, nothing is started after
it); HIP events around each repetition, warm-up first, median reported; the two measurements alternate ``--rounds`` times per
shape, and the summary line gives the medians' spread over the rounds.  The traffic floor is computed from the shapes: what the
op's launches must read and write once each (row pass, column pass, their two backward counterparts, the negation), and the
compulsory part of it (read x and y, write dx and dy).

    python tools/ffl_bench.py [--shapes 8x1x256x256,64x1x256x256,8x1x512x512] [--reps 50] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ffl_bench.py --child hip --shape 8x1x256x256      # the kernels' shares
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
    g = torch.Generator().manual_seed(0)
    x = torch.tanh(torch.randn(*shape, generator=g))
    y = torch.tanh(x + 0.3 * torch.randn(*shape, generator=g))
    return x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)


def traffic_floor_bytes(shape):
    """(launch floor, compulsory) bytes of one forward + backward.  Per pixel of a plane: row pass reads x, y (8) and writes
    [P | Q] of both (16); the column pass reads them (16) and writes Re, J of the difference (8); the backward column pass reads
    those (8) and writes [T1 | T2] (8); the last row pass reads that (8) and writes dx (4); the negation reads dx and writes
    dy (8).  Tables and partial sums are left out (they stay in cache / are a few KiB)."""
    n = 1
    for s in shape:
        n *= s
    return 84 * n, 16 * n


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


def child(kind, shape, reps, alpha):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    x, y = inputs(shape)
    if kind == "hip":
        def run():
            x.grad = y.grad = None
            faoctasr.ops.focal_frequency_loss(x, y, alpha).backward()
    else:
        def run():
            x.grad = y.grad = None
            D = torch.fft.fft2(x, norm="ortho") - torch.fft.fft2(y, norm="ortho")
            q = D.real ** 2 + D.imag ** 2
            with torch.no_grad():
                w = torch.sqrt(q) ** alpha
                w = w / w.amax(dim=(-2, -1), keepdim=True)
                w[torch.isnan(w)] = 0
                w = torch.clamp(w, 0, 1)
            (w * q).mean().backward()
    print(json.dumps({"kind": kind, "shape": list(shape), "alpha": alpha, **timed(run, reps)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x1x256x256,64x1x256x256,8x1x512x512")
    ap.add_argument("--shape", default="8x1x256x256", help="the one shape of a --child run")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3, help="the two measurements alternate this many times per shape")
    ap.add_argument("--child", choices=["hip", "fft"], default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child process")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        child(a.child, tuple(int(s) for s in a.shape.split("x")), a.reps, a.alpha)
        return
    for text in a.shapes.split(","):
        shape = tuple(int(s) for s in text.split("x"))
        med = {"hip": [], "fft": []}
        for kind in ["hip", "fft"] * a.rounds:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--shape", text, "--reps", str(a.reps),
                                "--alpha", str(a.alpha)], timeout=a.limit, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit("the %s measurement of %s ended with status %d: stopping" % (kind, text, r.returncode))
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            med[kind].append(json.loads(line)["median_ms"])
        floor, compulsory = traffic_floor_bytes(shape)
        hip_ms = statistics.median(med["hip"])
        print(json.dumps({"summary": text, "hip_median_ms": hip_ms, "hip_spread_ms": [min(med["hip"]), max(med["hip"])],
                          "fft_median_ms": statistics.median(med["fft"]), "fft_spread_ms": [min(med["fft"]), max(med["fft"])],
                          "faster_by_more_than_the_spread": max(med["hip"]) < min(med["fft"]),
                          "launch_floor_bytes": floor, "launch_floor_share_of_8TBps": floor / HBM_BYTES_PER_S / (hip_ms * 1e-3),
                          "compulsory_bytes": compulsory, "compulsory_share_of_8TBps": compulsory / HBM_BYTES_PER_S / (hip_ms * 1e-3)}),
              flush=True)


if __name__ == "__main__":
    main()
