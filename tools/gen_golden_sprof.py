"""Write tests/golden/golden_sprof.npz: the spectral-profile loss by its literal definition, independent of the package.

The reference tree does not contain this loss, so the fixture is the definition itself in float64 on the CPU, with nothing shared
with the kernels or the tests: the ring of every frequency comes from Python integers, the spectrum from explicit full-plane DFT
matrices (four matmuls), the profile from a loop over the rings, and the gradients from autograd through those matmuls.

    F = fft2(x) unnormalised, q = |F|^2 / (HW)                              per (n, c) plane
    bin(u, v) = the largest k with k^2 H^2 W^2 <= M^2 (u_c^2 W^2 + v_c^2 H^2), M = min(H, W), u_c = ((u + H//2) mod H) - H//2
    A[k] = mean of q over bin k,  a = log(A + eps)
    paired:  L = mean_{n,c,k>=k_min} (a_x - a_y)^2        batch:  L = mean_{k>=k_min} (mean_{n,c} a_x - mean_{n,c} a_y)^2

Asserted here before anything is written: Parseval (sum_k cnt_k A[k] = sum x^2), the gradients against central differences, and
the conditioning guard the gradient tests rely on (min_{k>=1} A[k] / mean(x^2) >= 2^-8 for both images).

Per case the file holds the fp32 inputs (seed 0, the recipe of ``inputs``), both float64 profiles, and per setting (batch_profile,
k_min) the float64 loss and per-image values, the fp32 ``torch.fft`` run's loss and its relative L2 errors (profiles, gradients)
against float64; the float64 gradients themselves for the cases and settings of ``GRADIENTS``.

    python tools/gen_golden_sprof.py
"""
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
SETTINGS = ((False, 0), (False, 1), (True, 0), (True, 1))               # (batch_profile, k_min)
GRADIENTS = {(2, 1, 8, 8): SETTINGS, (1, 2, 37, 53): ((False, 1), (True, 1))}
EPS = 1e-8
GUARD = 2.0 ** -8


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


def dft(n):
    ph = (torch.arange(n)[:, None] * torch.arange(n)[None, :]) % n
    t = 2 * math.pi * ph.double() / n
    return torch.cos(t), torch.sin(t)


def profile64(x, rows, cnt):
    """A (N, C, K) of x (N, C, H, W) float64 through explicit DFT matrices and a loop over the rings."""
    H, W = x.shape[-2:]
    (CH, SH), (CW, SW) = dft(H), dft(W)
    re = CH @ x @ CW - SH @ x @ SW
    im = SH @ x @ CW + CH @ x @ SW
    q = (re * re + im * im) / (H * W)
    bins = torch.tensor(rows)
    return torch.stack([(q * (bins == k)).sum((-2, -1)) / cnt[k] for k in range(len(cnt))], -1)


def profile_fft(x, rows, cnt):
    """The same through torch.fft and index_add_, in x's dtype."""
    F = torch.fft.fft2(x)
    q = (F.real ** 2 + F.imag ** 2) / (x.shape[-2] * x.shape[-1])
    flat = q.reshape(x.shape[0], x.shape[1], -1)
    A = torch.zeros(x.shape[0], x.shape[1], len(cnt), dtype=x.dtype).index_add_(2, torch.tensor(rows).flatten(), flat)
    return A / torch.tensor(cnt, dtype=x.dtype)


def loss_of(Ax, Ay, batch, k_min, eps=EPS):
    ax, ay = torch.log(Ax + eps), torch.log(Ay + eps)
    if batch:
        return ((ax.mean((0, 1)) - ay.mean((0, 1)))[k_min:] ** 2).mean(), None
    per = ((ax - ay)[..., k_min:] ** 2).mean((1, 2))
    return per.mean(), per


def run(x, y, rows, cnt, batch, k_min, profile, dtype):
    x = x.detach().to(dtype).clone().requires_grad_(True)
    y = y.detach().to(dtype).clone().requires_grad_(True)
    Ax, Ay = profile(x, rows, cnt), profile(y, rows, cnt)
    loss, per = loss_of(Ax, Ay, batch, k_min)
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach(), per.detach() if per is not None else None, gx, gy, Ax.detach(), Ay.detach()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def central_differences(x, y, rows, cnt, batch, k_min, gx, gy):
    g = torch.Generator().manual_seed(7)
    f = lambda a, b: float(loss_of(profile64(a, rows, cnt), profile64(b, rows, cnt), batch, k_min)[0])
    x, y, h = x.double(), y.double(), 1e-6
    for _ in range(3):
        dx, dy = torch.randn(x.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64)
        num = (f(x + h * dx, y + h * dy) - f(x - h * dx, y - h * dy)) / (2 * h)
        ana = float((gx * dx).sum() + (gy * dy).sum())
        assert abs(num - ana) <= 1e-6 * max(abs(ana), 1e-12) + 1e-9, (num, ana)


def tag_of(shape, setting):
    return "%s_b%d_k%d" % ("x".join(str(s) for s in shape), setting[0], setting[1])


def main():
    out = {}
    smallest = float("inf")
    for shape in SHAPES:
        x, y = inputs(shape)
        H, W = shape[-2:]
        rows, cnt = rings(H, W)
        case = "x".join(str(s) for s in shape)
        out["x_" + case], out["y_" + case] = x.numpy(), y.numpy()
        out["cnt_" + case] = np.array(cnt, dtype=np.int64)
        for st in SETTINGS:
            l64, per64, gx64, gy64, Ax, Ay = run(x, y, rows, cnt, *st, profile64, torch.float64)
            l32, _, gx32, gy32, Ax32, Ay32 = run(x, y, rows, cnt, *st, profile_fft, torch.float32)
            lf, _, gxf, gyf, Axf, _ = run(x, y, rows, cnt, *st, profile_fft, torch.float64)
            assert abs(float(lf) - float(l64)) <= 1e-12 * abs(float(l64)) and rel(gxf, gx64) <= 1e-11 and rel(Axf, Ax) <= 1e-12
            for img, A in ((x, Ax), (y, Ay)):
                e = (img.double() ** 2).sum((-2, -1))
                assert float(((A * torch.tensor(cnt)).sum(-1) - e).abs().max()) <= 1e-12 * float(e.max())            # Parseval
                if A.shape[-1] > 1:
                    ratio = float((A[..., 1:] / (img.double() ** 2).mean((-2, -1))[..., None]).min())
                    smallest = min(smallest, ratio)
                    assert ratio >= GUARD, (shape, ratio)
            if x.numel() <= 4096:
                central_differences(x, y, rows, cnt, *st, gx64, gy64)
            t = tag_of(shape, st)
            out["loss64_" + t], out["loss32_" + t] = np.float64(float(l64)), np.float32(float(l32))
            if per64 is not None:
                out["per64_" + t] = per64.numpy()
            out["gxerr32_" + t], out["gyerr32_" + t] = np.float64(rel(gx32, gx64)), np.float64(rel(gy32, gy64))
            if st in GRADIENTS.get(shape, ()):
                out["gx64_" + t], out["gy64_" + t] = gx64.numpy(), gy64.numpy()
            print("%-22s loss64 %.12e  loss32 rel err %.2e  gx32 rel err %.2e  gy32 rel err %.2e"
                  % (t, float(l64), abs(float(l32) - float(l64)) / abs(float(l64)), out["gxerr32_" + t], out["gyerr32_" + t]))
        out["Ax_" + case], out["Ay_" + case] = Ax.numpy(), Ay.numpy()
        out["Axerr32_" + case], out["Ayerr32_" + case] = np.float64(rel(Ax32, Ax)), np.float64(rel(Ay32, Ay))
    print("smallest A[k >= 1] / mean(x^2) over the cases: %.4f (guard %.4f)" % (smallest, GUARD))
    out["shapes"] = np.array(SHAPES, dtype=np.int64)
    out["settings"] = np.array([[int(b), k] for b, k in SETTINGS], dtype=np.int64)
    out["eps"] = np.float64(EPS)
    path = os.path.join(ROOT, "tests", "golden", "golden_sprof.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
