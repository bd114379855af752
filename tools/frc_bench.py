"""Time forward + backward (gradients to both images) of the Fourier ring correlation loss ``1 - ops.frc(x, y)`` against the fp32
torch composition of its definition on the same GPU (``torch.fft.rfft2``, three ``index_add_``, autograd).

One child process per shape under a time limit (a fault in one ends the run, nothing is started after it).  Inside it the two
measurements alternate: ``--rounds`` (7) batches of ``--reps`` (20) repetitions each, HIP events around each batch, warm-up first;
the figure of a batch is its mean per repetition, the reported figure the median over the batches, with their spread.  Peak memory
is ``torch.cuda.max_memory_allocated`` above what is allocated once the inputs exist (tables included, they are built in the
warm-up).  The traffic floor is computed from the shapes: what the op's launches must read and write once each, and the compulsory
part of it (read x and y, write dx and dy).

    python tools/frc_bench.py [--shapes 8x1x256x256,64x1x256x256,8x1x512x512] [--out profiles/frc_bench.txt]
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
KINDS = ("hip", "torch")
EPS = 1e-16


def smooth(t, r):
    import torch
    return sum(torch.roll(t, (dy, dx), (-2, -1)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / (2 * r + 1) ** 2


def inputs(shape):
    import torch
    g = torch.Generator().manual_seed(0)
    rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64)
    x = 2 * smooth(rn(), 2) + 0.25 * rn()
    y0 = x + 0.3 * rn()
    y = 0.7 * smooth(y0, 1) + 0.3 * y0
    return x.float().cuda().requires_grad_(True), y.float().cuda().requires_grad_(True)


def traffic_floor_bytes(shape):
    """(launch floor, compulsory) bytes of one forward + backward to both images.  Per pixel: the row pass reads x and y (8), the
    last row pass writes dx and dy (8).  Per half-plane position: the row pass writes [P | Q] of both images (16); the column pass
    reads them (16), writes the three weighted planes (12) and Re, J of both images (16); the ring sums read the three planes (12);
    the backward column pass reads Re, J of both (16) and the int16 ring map (2) and writes [T1 | T2] of both (16); the last row pass
    reads that (16).  Tables, ring means and coefficient tables are left out (cache / a few KiB)."""
    N, C, H, W = shape
    Wh = W // 2 + 1
    return N * C * H * (16 * W + 122 * Wh), 16 * N * C * H * W


def child(shape, reps, rounds):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    x, y = inputs(shape)
    N, C, H, W = shape
    bins, cnt = faoctasr.radial_bins(H, W)
    Wh, k_max = W // 2 + 1, min(H, W) // 2
    idx = bins[:, :Wh].flatten().cuda()
    m = torch.full((Wh,), 2.0)
    m[0] = 1
    if W % 2 == 0:
        m[W // 2] = 1
    m, cntf, K = (m / (H * W)).cuda(), cnt.float().cuda(), cnt.numel()

    def ring(q):
        return torch.zeros(N, C, K, device=q.device).index_add_(2, idx, (q * m).reshape(N, C, H * Wh)) / cntf

    def torch_index():
        F, G = torch.fft.rfft2(x), torch.fft.rfft2(y)
        r = ring(F.real * G.real + F.imag * G.imag) / torch.sqrt(ring(F.real ** 2 + F.imag ** 2) * ring(G.real ** 2 + G.imag ** 2) + EPS)
        return r[..., 1:k_max + 1].mean()

    def make(kind):
        def run():
            x.grad = y.grad = None
            (1 - (torch_index() if kind == "torch" else faoctasr.ops.frc(x, y))).backward()
        return run
    runs = {k: make(k) for k in KINDS}
    base = torch.cuda.memory_allocated()
    peak, vals = {}, {}
    for k in KINDS:                                                    # warm-up: tables, caches, the allocator's pools
        for _ in range(5):
            runs[k]()
        torch.cuda.synchronize()
        with torch.no_grad():
            vals[k] = float(torch_index() if k == "torch" else faoctasr.ops.frc(x, y))
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
    out = {"shape": list(shape), "reps": reps, "rounds": rounds, "inputs_bytes": base}
    for k in KINDS:
        out[k] = {"median_ms": statistics.median(ms[k]), "spread_ms": [min(ms[k]), max(ms[k])], "peak_bytes_above_inputs": peak[k], "index": vals[k]}
    floor, compulsory = traffic_floor_bytes(shape)
    hip_s = out["hip"]["median_ms"] * 1e-3
    out["hip_faster_than_torch_by_more_than_the_spread"] = max(ms["hip"]) < min(ms["torch"])
    out["torch_faster_than_hip_by_more_than_the_spread"] = max(ms["torch"]) < min(ms["hip"])
    out["launch_floor_bytes"], out["compulsory_bytes"] = floor, compulsory
    out["launch_floor_share_of_8TBps"] = floor / HBM_BYTES_PER_S / hip_s
    out["compulsory_share_of_8TBps"] = compulsory / HBM_BYTES_PER_S / hip_s
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
