"""Write tests/golden/golden_frc.npz: the Fourier ring correlation by its literal definition, independent of the package.

The reference tree does not contain this index, so the fixture is the definition itself on the CPU, with nothing shared with the
kernels or the tests: the ring of every frequency comes from Python integers, both spectra from explicit full-plane DFT matrices
(four matmuls each), the three ring means from a Python loop over the rings, and the gradients from autograd through those matmuls.

    F = fft2(x), G = fft2(y) unnormalised                                       per (n, c) plane
    bin(u, v) = the largest k with k^2 H^2 W^2 <= M^2 (u_c^2 W^2 + v_c^2 H^2), M = min(H, W), u_c = ((u + H//2) mod H) - H//2
    Nk = mean_ring Re(F conj G) / (HW),  Xk = mean_ring |F|^2 / (HW),  Yk = mean_ring |G|^2 / (HW)
    r_k = Nk / sqrt(Xk Yk + eps);  index = mean over n, c and k_min <= k <= k_max of r_k;  curve = r_k at every ring

It runs in float64 (the truth) and in float32 (the same matmuls; its index is kept as ``index32dft``).  The yardstick of the GPU
tests is the error of the fp32 ``torch.fft`` + ``index_add_`` run of the same definition against float64; that run is made here too
(``*err32``, ``index32``), and its float64 twin is held to the matrices' result at 1e-12.

Asserted here before anything is written: the guards the gradient comparisons rely on (min_{k>=1} Xk / mean(x^2) >= 2^-8 for both
images, |index| >= 0.25), the gradients against central differences (small cases), |r_k| <= 1, and the error bars themselves on the
float32 matrix run (each array's relative L2 error <= 8 x the torch.fft run's, the index within 8 r |I| + 1 ulp).

Settings (k_min, k_max): (1, None -> M//2), (0, K-1), (2, max(M//4, 2)), each clipped into [0, K-1] (the 2 x 3 plane has two rings).
Per case the file holds the fp32 inputs (seed 0, the recipe of ``inputs``), the float64 curve and, per setting, the float64 index
and per-image values and the fp32 figures; the float64 gradients for the cases and settings of ``GRADIENTS``.

    python tools/gen_golden_frc.py
"""
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
GRADIENTS = {(1, 1, 2, 3): (0, 1, 2), (2, 1, 8, 8): (0, 1, 2), (1, 2, 37, 53): (0,)}          # setting numbers
EPS = 1e-16
GUARD = 2.0 ** -8
MIN_INDEX = 0.25


def smooth(t, r):
    acc = torch.zeros_like(t)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            acc = acc + torch.roll(t, (dy, dx), (-2, -1))
    return acc / (2 * r + 1) ** 2


def inputs(shape):
    g = torch.Generator().manual_seed(0)
    rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64)
    x = 2 * smooth(rn(), 2) + 0.25 * rn()
    y0 = x + 0.3 * rn()
    y = 0.7 * smooth(y0, 1) + 0.3 * y0
    return x.float(), y.float()


def rings(H, W):
    """(bin as a list of rows, counts) in Python integers."""
    M = min(H, W)
    rows, cnt = [], {}
    for u in range(H):
        uc = (u + H // 2) % H - H // 2
        row = []
        for v in range(W):
            vc = (v + W // 2) % W - W // 2
            num, den = M * M * (uc * uc * W * W + vc * vc * H * H), H * H * W * W
            k = math.isqrt(num // den)
            assert k * k * den <= num < (k + 1) * (k + 1) * den
            row.append(k)
            cnt[k] = cnt.get(k, 0) + 1
        rows.append(row)
    K = max(cnt) + 1
    assert sorted(cnt) == list(range(K)) and sum(cnt.values()) == H * W
    return rows, [cnt[k] for k in range(K)]


def settings(H, W, K):
    M = min(H, W)
    raw = ((1, M // 2), (0, K - 1), (2, max(M // 4, 2)))
    out = []
    for a, b in raw:
        a = min(a, K - 1)
        out.append((a, max(a, min(b, K - 1))))
    return out


def dft(n, dtype):
    ph = (torch.arange(n)[:, None] * torch.arange(n)[None, :]) % n
    t = 2 * math.pi * ph.double() / n
    return torch.cos(t).to(dtype), torch.sin(t).to(dtype)


def means_dft(x, y, rows, cnt):
    """(Nk, Xk, Yk), each (N, C, K), through explicit DFT matrices and a loop over the rings, in x's dtype."""
    H, W = x.shape[-2:]
    (CH, SH), (CW, SW) = dft(H, x.dtype), dft(W, x.dtype)
    fr, fi = CH @ x @ CW - SH @ x @ SW, SH @ x @ CW + CH @ x @ SW
    gr, gi = CH @ y @ CW - SH @ y @ SW, SH @ y @ CW + CH @ y @ SW
    bins = torch.tensor(rows)
    planes = ((fr * gr + fi * gi) / (H * W), (fr * fr + fi * fi) / (H * W), (gr * gr + gi * gi) / (H * W))
    return tuple(torch.stack([(q * (bins == k)).sum((-2, -1)) / cnt[k] for k in range(len(cnt))], -1) for q in planes)


def means_fft(x, y, rows, cnt):
    """The same through torch.fft.fft2 and index_add_, in x's dtype."""
    N, C, H, W = x.shape
    F, G = torch.fft.fft2(x), torch.fft.fft2(y)
    flat = torch.tensor(rows).flatten()
    c = torch.tensor(cnt, dtype=x.dtype)
    planes = ((F.real * G.real + F.imag * G.imag) / (H * W), (F.real ** 2 + F.imag ** 2) / (H * W), (G.real ** 2 + G.imag ** 2) / (H * W))
    return tuple(torch.zeros(N, C, len(cnt), dtype=x.dtype).index_add_(2, flat, q.reshape(N, C, -1)) / c for q in planes)


def run(x, y, rows, cnt, band, means, dtype):
    x = x.detach().to(dtype).clone().requires_grad_(True)
    y = y.detach().to(dtype).clone().requires_grad_(True)
    Nk, Xk, Yk = means(x, y, rows, cnt)
    curve = Nk / torch.sqrt(Xk * Yk + EPS)
    per = curve[..., band[0]:band[1] + 1].mean((1, 2))
    index = per.mean()
    gx, gy = torch.autograd.grad(index, (x, y))
    return dict(index=float(index.detach()), per=per.detach().double(), gx=gx.double(), gy=gy.double(), curve=curve.detach().double(),
                Xk=Xk.detach().double(), Yk=Yk.detach().double())


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def central_differences(x, y, rows, cnt, band, gx, gy):
    g = torch.Generator().manual_seed(7)

    def f(a, b):
        Nk, Xk, Yk = means_dft(a, b, rows, cnt)
        return float((Nk / torch.sqrt(Xk * Yk + EPS))[..., band[0]:band[1] + 1].mean())
    x, y, h = x.double(), y.double(), 1e-6
    for _ in range(3):
        dx, dy = torch.randn(x.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64)
        num = (f(x + h * dx, y + h * dy) - f(x - h * dx, y - h * dy)) / (2 * h)
        ana = float((gx * dx).sum() + (gy * dy).sum())
        assert abs(num - ana) <= 1e-6 * max(abs(ana), 1e-12) + 1e-9, (num, ana)


def main():
    out, runs = {}, []
    smallest, r32 = float("inf"), 0.0
    for shape in SHAPES:
        x, y = inputs(shape)
        H, W = shape[-2:]
        rows, cnt = rings(H, W)
        case = "x".join(str(s) for s in shape)
        out["x_" + case], out["y_" + case] = x.numpy(), y.numpy()
        out["cnt_" + case] = np.array(cnt, dtype=np.int64)
        bands = settings(H, W, len(cnt))
        out["bands_" + case] = np.array(bands, dtype=np.int64)
        for s, band in enumerate(bands):
            r64 = run(x, y, rows, cnt, band, means_dft, torch.float64)
            d32 = run(x, y, rows, cnt, band, means_dft, torch.float32)
            f32 = run(x, y, rows, cnt, band, means_fft, torch.float32)
            f64 = run(x, y, rows, cnt, band, means_fft, torch.float64)
            assert abs(f64["index"] - r64["index"]) <= 1e-12 * abs(r64["index"]) and rel(f64["gx"], r64["gx"]) <= 1e-11
            assert rel(f64["gy"], r64["gy"]) <= 1e-11 and rel(f64["curve"], r64["curve"]) <= 1e-12
            assert float(r64["curve"].abs().max()) <= 1 + 1e-12
            for img, A in ((x, r64["Xk"]), (y, r64["Yk"])):
                if A.shape[-1] > 1:
                    ratio = float((A[..., 1:] / (img.double() ** 2).mean((-2, -1))[..., None]).min())
                    smallest = min(smallest, ratio)
                    assert ratio >= GUARD, (shape, ratio)
            assert abs(r64["index"]) >= MIN_INDEX, (shape, band, r64["index"])
            if x.numel() <= 4096:
                central_differences(x, y, rows, cnt, band, r64["gx"], r64["gy"])
            t = "%s_s%d" % (case, s)
            out["index64_" + t], out["index32_" + t], out["index32dft_" + t] = np.float64(r64["index"]), np.float32(f32["index"]), np.float32(d32["index"])
            out["per64_" + t] = r64["per"].numpy()
            out["gxerr32_" + t], out["gyerr32_" + t] = np.float64(rel(f32["gx"], r64["gx"])), np.float64(rel(f32["gy"], r64["gy"]))
            if s in GRADIENTS.get(shape, ()):
                out["gx64_" + t], out["gy64_" + t] = r64["gx"].numpy(), r64["gy"].numpy()
            r32 = max(r32, abs(f32["index"] - r64["index"]) / abs(r64["index"]))
            runs.append((t, r64, d32, f32))
            print("%-20s band %-9s index64 %.12f  index32 rel err %.2e  gx32 rel err %.2e  gy32 rel err %.2e  curve32 rel err %.2e"
                  % (t, band, r64["index"], abs(f32["index"] - r64["index"]) / abs(r64["index"]), out["gxerr32_" + t], out["gyerr32_" + t],
                     rel(f32["curve"], r64["curve"])))
        out["curve64_" + case] = r64["curve"].numpy()
        out["curveerr32_" + case] = np.float64(rel(f32["curve"], r64["curve"]))
    # the error bars of the GPU tests, on the float32 run through the matrices (another fp32 evaluation of the same definition)
    for t, r64, d32, f32 in runs:
        bar = 8 * r32 * abs(r64["index"]) + float(np.spacing(np.float32(abs(r64["index"]))))
        assert abs(d32["index"] - r64["index"]) <= bar, (t, d32["index"], r64["index"], bar)
        for k in ("gx", "gy", "curve"):
            assert rel(d32[k], r64[k]) <= 8 * rel(f32[k], r64[k]), (t, k, rel(d32[k], r64[k]), rel(f32[k], r64[k]))
    print("smallest Xk[k >= 1] / mean(x^2) over the cases: %.4f (guard %.4f); largest fp32 relative index error %.2e" % (smallest, GUARD, r32))
    out["shapes"] = np.array(SHAPES, dtype=np.int64)
    out["eps"] = np.float64(EPS)
    path = os.path.join(ROOT, "tests", "golden", "golden_frc.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
