"""Time forward + backward (gradients to both images) of the spectral-profile loss (ops.spectral_profile_loss) against the fp32
torch composition of its definition on the same GPU (``torch.fft.rfft2``, ``index_add_``, log, mse, autograd), and against the
same kernels forced to full-spectrum tables (``_full_spectrum``, a switch of this tool only): what the half-spectrum form buys.

One child process per shape under a time limit (a fault in one ends the run, nothing is started after it).  Inside it the three
measurements alternate: ``--rounds`` (7) batches of ``--reps`` (20) repetitions each, HIP events around each batch, warm-up first;
the figure of a batch is its mean per repetition, the reported figure the median over the batches, with their spread.  Peak memory
is ``torch.cuda.max_memory_allocated`` above what is allocated once the inputs exist (tables included, they are built in the
warm-up).  The traffic floor is computed from the shapes: what the op's launches must read and write once each, and the compulsory
part of it (read x and y, write dx and dy).

    python tools/sprof_bench.py [--shapes 8x1x256x256,64x1x256x256,8x1x512x512] [--batch-profile 1] [--out profiles/sprof_bench.txt]
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
KINDS = ("hip", "hip_full", "torch")


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


def traffic_floor_bytes(shape, full=False):
    """(launch floor, compulsory) bytes of one forward + backward to both images.  Per image: the row pass reads x (4 per pixel);
    per half-plane position it writes [P | Q] (8); the column pass reads them (8), writes the power (4) and Re, J (8); the binning
    reads the power (4); the backward column pass reads Re, J (8) and the int16 ring map (2) and writes [T1 | T2] (8); the last row
    pass reads that (8) and writes dx (4 per pixel).  Tables, profiles and coefficient tables are left out (cache / a few KiB)."""
    N, C, H, W = shape
    Wh = W if full else W // 2 + 1
    return 2 * N * C * H * (8 * W + 58 * Wh), 16 * N * C * H * W


def child(shape, reps, rounds, batch):
    import torch
    import faoctasr
    assert torch.cuda.is_available(), "needs a GPU"
    x, y = inputs(shape)
    N, C, H, W = shape
    bins, cnt = faoctasr.radial_bins(H, W)
    Wh = W // 2 + 1
    idx = bins[:, :Wh].flatten().cuda()
    m = torch.full((Wh,), 2.0)
    m[0] = 1
    if W % 2 == 0:
        m[W // 2] = 1
    m, cntf, K = (m / (H * W)).cuda(), cnt.float().cuda(), cnt.numel()

    def composition(t):
        Fq = torch.fft.rfft2(t)
        q = ((Fq.real ** 2 + Fq.imag ** 2) * m).reshape(N, C, H * Wh)
        return torch.log(torch.zeros(N, C, K, device=t.device).index_add_(2, idx, q) / cntf + 1e-8)

    def torch_loss():
        ax, ay = composition(x), composition(y)
        d = (ax.mean((0, 1)) - ay.mean((0, 1))) if batch else (ax - ay)
        return (d[..., 1:] ** 2).mean()

    def make(kind):
        def run():
            x.grad = y.grad = None
            if kind == "torch":
                torch_loss().backward()
            else:
                faoctasr.ops.spectral_profile_loss(x, y, batch_profile=batch, _full_spectrum=kind == "hip_full").backward()
        return run
    runs = {k: make(k) for k in KINDS}
    base = torch.cuda.memory_allocated()
    peak, vals = {}, {}
    for k in KINDS:                                                    # warm-up: tables, caches, the allocator's pools
        for _ in range(5):
            runs[k]()
        torch.cuda.synchronize()
        with torch.no_grad():
            vals[k] = float(torch_loss() if k == "torch" else faoctasr.ops.spectral_profile_loss(x, y, batch_profile=batch, _full_spectrum=k == "hip_full"))
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
    out = {"shape": list(shape), "batch_profile": bool(batch), "reps": reps, "rounds": rounds, "inputs_bytes": base}
    for k in KINDS:
        out[k] = {"median_ms": statistics.median(ms[k]), "spread_ms": [min(ms[k]), max(ms[k])], "peak_bytes_above_inputs": peak[k], "loss": vals[k]}
    floor, compulsory = traffic_floor_bytes(shape)
    floor_full, _ = traffic_floor_bytes(shape, full=True)
    hip_s = out["hip"]["median_ms"] * 1e-3
    out["hip_faster_than_torch_by_more_than_the_spread"] = max(ms["hip"]) < min(ms["torch"])
    out["half_spectrum_gain"] = out["hip_full"]["median_ms"] / out["hip"]["median_ms"]
    out["launch_floor_bytes"], out["launch_floor_bytes_full_spectrum"], out["compulsory_bytes"] = floor, floor_full, compulsory
    out["launch_floor_share_of_8TBps"] = floor / HBM_BYTES_PER_S / hip_s
    out["compulsory_share_of_8TBps"] = compulsory / HBM_BYTES_PER_S / hip_s
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x1x256x256,64x1x256x256,8x1x512x512")
    ap.add_argument("--shape", default=None, help="the one shape of a --child run")
    ap.add_argument("--batch-profile", type=int, default=1, help="1: the unpaired domain form the train step uses; 0: the paired form")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    a = ap.parse_args()
    if a.child:
        child(tuple(int(s) for s in a.shape.split("x")), a.reps, a.rounds, a.batch_profile)
        return
    for text in a.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", text, "--reps", str(a.reps), "--rounds", str(a.rounds),
                            "--batch-profile", str(a.batch_profile)], timeout=a.limit, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit("the measurement of %s ended with status %d: stopping" % (text, r.returncode))
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
