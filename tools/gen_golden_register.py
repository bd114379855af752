"""Write tests/golden/golden_register.npz: phase-correlation registration and the Fourier shift by their literal definitions, in numpy
float64 with explicit DFT matrices, independent of the package and the tests.

    F = fft2(a), G = fft2(b) unnormalised;  R = G conj(F) / (HW);  Rn = R / sqrt(|R|^2 + eps), zero in every ring above k_max
    surface = sum_c Re ifft2(Rn);  coarse peak: the first maximum in row-major order with |d_y| <= max_shift, |d_x| <= max_shift
    up[j,i] = (1/HW) sum_c sum_u sum_{v<Wh} m_v Re(Rn[c,u,v] exp(2 pi i (f_u (s_y + o_j) + f_v (s_x + o_i)))),  o_j = (j - T//2) / U,
    T = ceil(1.5 U), f of numpy.fft.fftfreq (Nyquist at -1/2), m_v = 2 except for the self-mirrored columns;  the first maximum wins
    shift = (s_y + o_j*, s_x + o_i*),  peak = the winning value over C
    fourier_shift(x, d) = Re ifft2(fft2(x) exp(-2 pi i (f_u d_y + f_v d_x)))

Inputs, per case (shape, displacement d): seed s, rn() standard normal float64 from ``torch.Generator().manual_seed(s)`` (the one use of
torch besides the fp32 yardstick below): a = 2 smooth(rn(), 2) + 0.25 rn();  b0 = fourier_shift(a, d) + 0.3 rn();
b = 0.7 smooth(b0, 1) + 0.3 b0;  both rounded to fp32.  The tests rebuild them from the seed kept in the file.

The arg-max is discontinuous, so before anything is written this asserts on float64, for every case and setting, that the coarse
maximum and the refined maximum each exceed their runner-up by at least 2^-12 of their value.  A case that fails is not dropped: the
first seed of range(2000) that passes for all its settings is taken and recorded.  Settings: U in 1, 4, 10 with every ring, and
U = 10 with the ring cut k_max = K // 2; max_shift = min(8, H // 2, W // 2), which is also what ``Registered`` searches.  For the
seam case displaced by (-2.3, 1.7) it also asserts that the FRC index of the registered, cropped pair exceeds the unregistered one.

The yardstick of the GPU tests is the error of the fp32 ``torch.fft`` run of the same definition; its peaks are kept (``peak32_*``)
and its float64 twin is held to the matrices' result here.

    python tools/gen_golden_register.py
"""
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
DISPLACEMENTS = ((0, 0), (1, -1), (3, -2), (-2.3, 1.7), (0.4, -0.6), (2.5, -0.5))
UPSAMPLE = (1, 4, 10)
SURFACES = (((2, 1, 8, 8), (1, -1)), ((1, 2, 37, 53), (-2.3, 1.7)), ((2, 1, 72, 136), (2.5, -0.5)))
SEAMS, SEAMS_D = (2, 1, 72, 136), (-2.3, 1.7)
EPS = 1e-16
GAP = 2.0 ** -12


def smooth(t, r):
    acc = np.zeros_like(t)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            acc = acc + np.roll(t, (dy, dx), (-2, -1))
    return acc / (2 * r + 1) ** 2


def dft(n):
    ph = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    return np.exp(-2j * math.pi * ph / n)


def fft2(x):
    return dft(x.shape[-2]) @ x @ dft(x.shape[-1])


def ifft2(z):
    H, W = z.shape[-2:]
    return np.conj(dft(H)) @ z @ np.conj(dft(W)) / (H * W)


def signed(n):
    return np.array([(u + n // 2) % n - n // 2 for u in range(n)])


def position(n):
    """The signed position of every index of a correlation surface: positions > n//2 wrap negative."""
    return np.array([p - n if p > n // 2 else p for p in range(n)])


def fourier_shift(x, d):
    H, W = x.shape[-2:]
    ramp = np.exp(-2j * math.pi * (signed(H)[:, None] * d[0] / H + signed(W)[None, :] * d[1] / W))
    return ifft2(fft2(x) * ramp).real


def inputs(shape, d, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64).numpy()
    a = 2 * smooth(rn(), 2) + 0.25 * rn()
    b0 = fourier_shift(a, d) + 0.3 * rn()
    b = 0.7 * smooth(b0, 1) + 0.3 * b0
    return a.astype(np.float32), b.astype(np.float32)


def rings(H, W):
    """The ring of every frequency and the number of rings, in Python integers."""
    M = min(H, W)
    out = np.zeros((H, W), dtype=np.int64)
    for u in range(H):
        uc = (u + H // 2) % H - H // 2
        for v in range(W):
            vc = (v + W // 2) % W - W // 2
            num, den = M * M * (uc * uc * W * W + vc * vc * H * H), H * H * W * W
            k = math.isqrt(num // den)
            assert k * k * den <= num < (k + 1) * (k + 1) * den
            out[u, v] = k
    return out, int(out.max()) + 1


def cross_power(a, b, k_max, eps=EPS):
    H, W = a.shape[-2:]
    F, G = fft2(a.astype(np.float64)), fft2(b.astype(np.float64))
    R = G * np.conj(F) / (H * W)
    Rn = R / np.sqrt(R.real ** 2 + R.imag ** 2 + eps)
    if k_max is not None:
        Rn = np.where(rings(H, W)[0] > k_max, 0.0, Rn)
    return Rn


def first_max(plane, allowed=None):
    """(flat index of the first maximum, its value, the gap to the runner-up over the value) among the allowed positions."""
    flat = plane.reshape(-1).copy()
    if allowed is not None:
        flat[~allowed.reshape(-1)] = -np.inf
    i = int(np.argmax(flat))
    top = float(flat[i])
    flat[i] = -np.inf
    return i, top, (top - float(flat.max())) / top if flat.size > 1 else 1.0


def register(a, b, U, max_shift, k_max=None):
    """(shift (N, 2), peak (N,), surface (N, H, W), smallest coarse gap, smallest refined gap), float64."""
    N, C, H, W = a.shape
    Wh = W // 2 + 1
    Rn = cross_power(a, b, k_max)
    surf = ifft2(Rn).real.sum(1)
    wy, wx, py, px = signed(H), signed(W), position(H), position(W)
    allowed = (np.abs(py)[:, None] <= max_shift) & (np.abs(px)[None, :] <= max_shift)
    mv = np.array([1.0 if v == 0 or 2 * v == W else 2.0 for v in range(Wh)])
    T = -(-3 * U // 2)
    shift, peak, gc, gr = np.zeros((N, 2)), np.zeros(N), 1.0, 1.0
    for n in range(N):
        i, top, gap = first_max(surf[n], allowed)
        gc = min(gc, gap)
        sy, sx = int(py[i // W]), int(px[i % W])
        shift[n], peak[n] = (sy, sx), top / C
        if U == 1:
            continue
        j = np.arange(T) - T // 2
        ey = np.exp(2j * math.pi * ((wy[None, :] * (sy * U + j)[:, None]) % (U * H)) / (U * H))               # (T, H)
        ex = np.exp(2j * math.pi * ((wx[:Wh, None] * (sx * U + j)[None, :]) % (U * W)) / (U * W))             # (Wh, T)
        up = sum((ey @ (Rn[n, c][:, :Wh] * mv[None, :]) @ ex).real for c in range(C)) / (H * W)
        i, top, gap = first_max(up)
        gr = min(gr, gap)
        shift[n], peak[n] = ((sy * U + j[i // T]) / U, (sx * U + j[i % T]) / U), top / C
    return shift, peak, surf, gc, gr


def torch_run(a, b, U, max_shift, k_max, dtype):
    """The same definition through ``torch.fft`` in ``dtype`` (the yardstick of the GPU tests): (shift, peak, surface) as float64."""
    N, C, H, W = a.shape
    Wh = W // 2 + 1
    cdt = torch.complex64 if dtype == torch.float32 else torch.complex128
    ta, tb = torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype)
    F, G = torch.fft.fft2(ta), torch.fft.fft2(tb)
    R = G * F.conj() / (H * W)
    Rn = R / torch.sqrt(R.real ** 2 + R.imag ** 2 + EPS)
    if k_max is not None:
        Rn = torch.where(torch.from_numpy(rings(H, W)[0] > k_max), torch.zeros((), dtype=cdt), Rn)
    surf = torch.fft.ifft2(Rn).real.sum(1)
    wy, wx, py, px = signed(H), signed(W), position(H), position(W)
    allowed = (np.abs(py)[:, None] <= max_shift) & (np.abs(px)[None, :] <= max_shift)
    mv = torch.tensor([1.0 if v == 0 or 2 * v == W else 2.0 for v in range(Wh)], dtype=dtype)
    T = -(-3 * U // 2)
    shift, peak = np.zeros((N, 2)), np.zeros(N)
    for n in range(N):
        i, top, _ = first_max(surf[n].double().numpy(), allowed)
        sy, sx = int(py[i // W]), int(px[i % W])
        shift[n], peak[n] = (sy, sx), top / C
        if U == 1:
            continue
        j = np.arange(T) - T // 2
        ey = torch.from_numpy(np.exp(2j * math.pi * ((wy[None, :] * (sy * U + j)[:, None]) % (U * H)) / (U * H))).to(cdt)
        ex = torch.from_numpy(np.exp(2j * math.pi * ((wx[:Wh, None] * (sx * U + j)[None, :]) % (U * W)) / (U * W))).to(cdt)
        up = sum((ey @ (Rn[n, c][:, :Wh] * mv[None, :]) @ ex).real for c in range(C)) / (H * W)
        i, top, _ = first_max(up.double().numpy())
        shift[n], peak[n] = ((sy * U + j[i // T]) / U, (sx * U + j[i % T]) / U), top / C
    return shift, peak, surf.double().numpy()


def frc_index(x, y, eps=1e-16):
    """The FRC index of ``ops.frc`` (k_min = 1, k_max = min(H, W) // 2) per sample, from the matrices."""
    N, C, H, W = x.shape
    bins, K = rings(H, W)
    F, G = fft2(x), fft2(y)
    out = np.zeros(N)
    for n in range(N):
        r = []
        for c in range(C):
            for k in range(1, min(H, W) // 2 + 1):
                m = bins == k
                nk = (F[n, c] * np.conj(G[n, c])).real[m].mean() / (H * W)
                xk, yk = (np.abs(F[n, c]) ** 2)[m].mean() / (H * W), (np.abs(G[n, c]) ** 2)[m].mean() / (H * W)
                r.append(nk / math.sqrt(xk * yk + eps))
        out[n] = np.mean(r)
    return out


def settings(H, W):
    K = rings(H, W)[1]
    return [(U, None) for U in UPSAMPLE] + [(10, K // 2)]


def case_name(shape, d):
    return "x".join(str(s) for s in shape) + "_" + "_".join(("%g" % v).replace("-", "m").replace(".", "p") for v in d)


def cases():
    for shape in SHAPES:
        for d in DISPLACEMENTS:
            if abs(d[0]) < shape[2] / 2 and abs(d[1]) < shape[3] / 2:
                yield shape, d


def solve(shape, d):
    """The first seed whose every setting passes the gap guards, with its results."""
    H, W = shape[2:]
    ms = min(8, H // 2, W // 2)
    for seed in range(2000):
        a, b = inputs(shape, d, seed)
        res, ok = {}, True
        for U, k_max in settings(H, W):
            shift, peak, surf, gc, gr = register(a, b, U, ms, k_max)
            if gc < GAP or gr < GAP:
                ok = False
                break
            res[(U, k_max)] = (shift, peak, surf, gc, gr)
        if ok:
            return seed, a, b, res
    raise AssertionError("no seed in range(2000) passes the guards for %s %s" % (shape, d))


def main():
    out, r_peak, gaps = {}, 0.0, {}
    for shape, d in cases():
        H, W = shape[2:]
        ms = min(8, H // 2, W // 2)
        seed, a, b, res = solve(shape, d)
        name = case_name(shape, d)
        out["seed_" + name] = np.int64(seed)
        for (U, k_max), (shift, peak, surf, gc, gr) in res.items():
            key = "%s_U%d%s" % (name, U, "" if k_max is None else "_cut")
            out["shift_" + key], out["peak_" + key] = shift, peak
            s64, p64, f64 = torch_run(a, b, U, ms, k_max, torch.float64)
            assert np.array_equal(s64, shift) and np.allclose(p64, peak, rtol=1e-11, atol=0) and np.allclose(f64, surf, rtol=0, atol=1e-12)
            s32, p32, _ = torch_run(a, b, U, ms, k_max, torch.float32)
            assert np.array_equal(s32, shift), (key, s32, shift)
            out["peak32_" + key] = p32
            r_peak = max(r_peak, float(np.max(np.abs(p32 - peak) / np.abs(peak))))
            tag = "U%d%s" % (U, "" if k_max is None else "_cut")
            gaps[tag] = (min(gaps.get(tag, (1, 1))[0], gc), min(gaps.get(tag, (1, 1))[1], gr))
            if k_max is not None:
                out["kmax_" + key] = np.int64(k_max)
        if (shape, d) in SURFACES:
            out["surface_" + name] = res[(1, None)][2]
        if shape == SEAMS and d == SEAMS_D:
            m = ms + 1
            est = res[(10, None)][0]
            moved = np.stack([fourier_shift(b[n].astype(np.float64), -est[n]) for n in range(shape[0])])
            crop = lambda t: t[..., m:-m, m:-m]
            reg, raw = frc_index(crop(a.astype(np.float64)), crop(moved)), frc_index(crop(a.astype(np.float64)), crop(b.astype(np.float64)))
            assert (reg > raw).all(), (reg, raw)
            out["frc_registered"], out["frc_unregistered"] = reg, raw
        print("%-34s seed %d  %s" % (name, seed, "  ".join("U%d%s %s" % (U, "" if k is None else "cut", np.round(v[0], 3).tolist())
                                                             for (U, k), v in res.items())))
    for tag, (gc, gr) in sorted(gaps.items()):
        print("smallest gaps %-8s coarse %.3e refined %.3e" % (tag, gc, gr))
    print("largest relative peak error of the fp32 torch.fft run: %.3e" % r_peak)
    path = os.path.join(ROOT, "tests", "golden", "golden_register.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
