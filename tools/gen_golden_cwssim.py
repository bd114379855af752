"""Write tests/golden/golden_cwssim.npz: the complex-wavelet structural similarity

    S(x, y) = sum_j w_j S_j / sum_j w_j,   S_j = mean over (n, c, orientation, position p) of (2 |z_p| + K) / (E_p + K),
    z_p = sum_{W(p)} cx conj(cy),   E_p = sum_{W(p)} |cx|^2 + sum_{W(p)} |cy|^2,   K = 1e-2,

over the win x win box windows W(p) at every valid position of the bands cx = yh_j(x), cy = yh_j(y) of the reference's own
``DTCWTForward``, composed with torch ops (products, ``avg_pool2d`` as the box sum) on the CPU, once in float64 and once in
float32; the loss is 1 - S and its gradients with respect to x and y come from autograd.  Runs where the reference checkout
exists only (oracle/ref_shim.py).  Banks a, b, c as tools/gen_golden_dtcwt.py names them, taps passed as tuples.

Inputs: x ~ N(0, 1) and y = x + 0.5 n, n ~ N(0, 1), float32 values, one pair per shape.  u = z / |z| amplifies rounding by
kappa_p = sum_W |cx| |cy| / |z_p|; the largest kappa_p over every window of the float64 run is recorded per bank and case.

Per shape ``in/<shape>/x``, ``in/<shape>/y``; per bank and case ``<bank>/<case>/loss`` (1 - S), ``scores`` (S per image), ``dx``, ``dy``
(float64), ``<bank>/<case>/f32/...`` (float32) and ``<bank>/<case>/kappa``; per bank the six buffers the reference registers
(``<bank>/buf_<name>``, float64).  The file stays below 1 MiB.

    python tools/gen_golden_cwssim.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_shim              # noqa: E402
from gen_golden_dtcwt import BANKS, FWD_BUFS, tables      # noqa: E402

K = 1e-2
#: (case, shape, J, win, mode, level weights or None, y needs a gradient)
CASES = (("j1_w3_symmetric", (2, 3, 16, 24), 1, 3, "symmetric", None, True),
         ("j1_w3_zero", (1, 3, 16, 24), 1, 3, "zero", None, True),
         ("j2_w3_symmetric", (2, 3, 16, 24), 2, 3, "symmetric", None, True),
         ("j3_w7_56x56", (1, 1, 56, 56), 3, 7, "symmetric", None, True),
         ("j2_w5_weights", (1, 2, 24, 40), 2, 5, "symmetric", (0.5, 2.0), True),
         ("j1_w1", (2, 1, 16, 16), 1, 1, "symmetric", None, True),
         ("j2_w3_xonly", (1, 3, 16, 24), 2, 3, "symmetric", None, False))


def shape_key(shape):
    return "%dx%dx%dx%d" % tuple(shape)


def box(t, win):
    """The win x win box sums of a (N, C, 6, h, w) tensor at the valid positions."""
    n, c, o, h, w = t.shape
    return (F.avg_pool2d(t.reshape(n, c * o, h, w), win, stride=1) * float(win * win)).reshape(n, c, o, h - win + 1, w - win + 1)


def level_index(cx, cy, win):
    """(S per image, the largest kappa) of one level's bands."""
    xr, xi, yr, yi = cx[..., 0], cx[..., 1], cy[..., 0], cy[..., 1]
    zr, zi = box(xr * yr + xi * yi, win), box(xi * yr - xr * yi, win)
    E = box(xr * xr + xi * xi, win) + box(yr * yr + yi * yi, win)
    m = torch.sqrt(zr * zr + zi * zi)
    S = (2 * m + K) / (E + K)
    kappa = box(torch.sqrt(xr * xr + xi * xi) * torch.sqrt(yr * yr + yi * yi), win) / m
    return S.mean(dim=(1, 2, 3, 4)), float(kappa.detach().max())


def run(fwd_cls, taps, J, win, mode, weights, x, y, y_grad, dtype):
    """(loss, scores per image, dx, dy or None, largest kappa) of one run in ``dtype``."""
    torch.set_default_dtype(dtype)
    try:
        fwd = fwd_cls(biort=taps[0], qshift=taps[1], J=J, mode=mode)
        x = x.to(dtype).clone().requires_grad_(True)
        y = y.to(dtype).clone().requires_grad_(y_grad)
        hx, hy = fwd(x)[1], fwd(y)[1]
        w = weights or (1.0,) * J
        scores, kappa = 0.0, 0.0
        for j in range(J):
            s, k = level_index(hx[j], hy[j], win)
            scores = scores + w[j] * s
            kappa = max(kappa, k)
        scores = scores / sum(w)
        loss = 1 - scores.mean()
        loss.backward()
        return loss.detach().numpy(), scores.detach().numpy(), x.grad.numpy(), (y.grad.numpy() if y_grad else None), kappa
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref_shim.load()
    from pytorch_wavelets import DTCWTForward
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    out = {}
    taps = {bank: tables(bank)[0] for bank in BANKS}
    for k, shape in enumerate(sorted(set(c[1] for c in CASES))):
        g = torch.Generator().manual_seed(9700 + k)
        x = torch.randn(*shape, generator=g, dtype=torch.float32)
        y = x + 0.5 * torch.randn(*shape, generator=g, dtype=torch.float32)
        out["in/%s/x" % shape_key(shape)], out["in/%s/y" % shape_key(shape)] = x.numpy(), y.numpy()
    for case, shape, J, win, mode, weights, y_grad in CASES:
        x, y = (torch.from_numpy(out["in/%s/%s" % (shape_key(shape), n)]) for n in "xy")
        for bank in BANKS:
            r64 = run(DTCWTForward, taps[bank], J, win, mode, weights, x, y, y_grad, torch.float64)
            r32 = run(DTCWTForward, taps[bank], J, win, mode, weights, x, y, y_grad, torch.float32)
            for prefix, r in (("%s/%s/" % (bank, case), r64), ("%s/%s/f32/" % (bank, case), r32)):
                out[prefix + "loss"], out[prefix + "scores"], out[prefix + "dx"] = r[0], r[1], r[2]
                if y_grad:
                    out[prefix + "dy"] = r[3]
            out["%s/%s/kappa" % (bank, case)] = np.float64(r64[4])
            print("%s %-16s largest kappa %.3f loss %.12f (fp32 %.9f)" % (bank, case, r64[4], r64[0], r32[0]))
    torch.set_default_dtype(torch.float64)
    for bank in BANKS:
        fwd = DTCWTForward(biort=taps[bank][0], qshift=taps[bank][1])
        for name in FWD_BUFS:
            out["%s/buf_%s" % (bank, name)] = getattr(fwd, name).numpy()
    torch.set_default_dtype(torch.float32)
    path = os.path.join(ROOT, "tests", "golden", "golden_cwssim.npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size >= 1 << 20:
        raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
