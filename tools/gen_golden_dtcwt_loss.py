"""Write tests/golden/golden_cwt_loss.npz: the DTCWT magnitude loss

    L(x, y) = sum_j w_j * l1_loss(r(yh_j(x)), r(yh_j(y))),     r(h) = sqrt(re^2 + im^2 + b^2),  b = 1e-2

composed from the reference's own ``DTCWTForward`` and torch ops on the CPU, once in float64 and once in float32, with its
gradients with respect to x and y by autograd.  Runs where the reference checkout exists only (oracle/ref_shim.py).  Banks a, b,
c as tools/gen_golden_dtcwt.py names them (near_sym_a + qshift_a, near_sym_b + qshift_c, legall + qshift_d), taps passed as tuples.

Cases (shared by the banks): J = 1, 2, 3 on (2,3,16,24) in 'symmetric', J = 1 in 'zero', (1,1,8,8) at J = 3 (1 x 1 bands at the
last level), (1,2,8,16) at J = 3 with the level weights (0.5, 1.25, 2.0), and (1,2,8,16) at J = 2 in 'zero' where only x needs a
gradient (no dy).

The tie condition.  sign(r_x - r_y) is discontinuous, so a case's inputs are N(0,1) images from the first seed for which, for all
three banks, (1) the smallest |r_x - r_y| / max(r_x, r_y) over every coefficient of the float64 run is at least 2^-16 and (2) the
float32 and float64 runs agree on every sign.  Both are asserted; the seed and each bank's smallest gap are recorded.

Per case ``in/<case>/x``, ``in/<case>/y`` (float32 values) and ``in/<case>/seed``; per bank and case ``<bank>/<case>/loss``, ``dx``,
``dy`` (float64), ``<bank>/<case>/f32/...`` (float32) and ``<bank>/<case>/gap``; per bank the six buffers the reference registers
(``<bank>/buf_<name>``, float64).  The file stays below 1 MiB.

    python tools/gen_golden_dtcwt_loss.py
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

MAGBIAS = 1e-2
MIN_GAP = 2.0 ** -16
#: (case, shape, J, mode, level weights or None, y needs a gradient)
CASES = (("j1_symmetric", (2, 3, 16, 24), 1, "symmetric", None, True),
         ("j1_zero", (2, 3, 16, 24), 1, "zero", None, True),
         ("j2_symmetric", (2, 3, 16, 24), 2, "symmetric", None, True),
         ("j3_symmetric", (2, 3, 16, 24), 3, "symmetric", None, True),
         ("j3_8x8", (1, 1, 8, 8), 3, "symmetric", None, True),
         ("j3_weights", (1, 2, 8, 16), 3, "symmetric", (0.5, 1.25, 2.0), True),
         ("j2_zero_xonly", (1, 2, 8, 16), 2, "zero", None, False))


def magnitudes(fwd, t):
    return [torch.sqrt(h[..., 0] ** 2 + h[..., 1] ** 2 + MAGBIAS * MAGBIAS) for h in fwd(t)[1]]


def run(fwd_cls, taps, J, mode, weights, x, y, y_grad, dtype):
    """(loss, dx, dy or None, per-coefficient r_x - r_y, smallest relative gap) of one run in ``dtype``."""
    torch.set_default_dtype(dtype)
    try:
        fwd = fwd_cls(biort=taps[0], qshift=taps[1], J=J, mode=mode)
        x = x.to(dtype).clone().requires_grad_(True)
        y = y.to(dtype).clone().requires_grad_(y_grad)
        rx, ry = magnitudes(fwd, x), magnitudes(fwd, y)
        w = weights or (1.0,) * J
        loss = sum(w[j] * F.l1_loss(rx[j], ry[j]) for j in range(J))
        loss.backward()
        diff = torch.cat([(a - b).detach().reshape(-1) for a, b in zip(rx, ry)])
        big = torch.cat([torch.maximum(a, b).detach().reshape(-1) for a, b in zip(rx, ry)])
        return loss.detach().numpy(), x.grad.numpy(), (y.grad.numpy() if y_grad else None), diff, float((diff.abs() / big).min())
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
    for k, (case, shape, J, mode, weights, y_grad) in enumerate(CASES):
        for seed in range(9100 + 100 * k, 9200 + 100 * k):
            g = torch.Generator().manual_seed(seed)
            x, y = torch.randn(*shape, generator=g, dtype=torch.float32), torch.randn(*shape, generator=g, dtype=torch.float32)
            runs, ok = {}, True
            for bank in BANKS:
                r64 = run(DTCWTForward, taps[bank], J, mode, weights, x, y, y_grad, torch.float64)
                r32 = run(DTCWTForward, taps[bank], J, mode, weights, x, y, y_grad, torch.float32)
                ok = ok and r64[4] >= MIN_GAP and bool((torch.sign(r64[3]) == torch.sign(r32[3].double())).all())
                runs[bank] = (r64, r32)
            if ok:
                break
        else:
            raise SystemExit("%s: no seed meets the tie condition" % case)
        out["in/%s/x" % case], out["in/%s/y" % case], out["in/%s/seed" % case] = x.numpy(), y.numpy(), np.int64(seed)
        for bank in BANKS:
            r64, r32 = runs[bank]
            assert r64[4] >= MIN_GAP and bool((torch.sign(r64[3]) == torch.sign(r32[3].double())).all())      # the tie condition
            for prefix, r in (("%s/%s/" % (bank, case), r64), ("%s/%s/f32/" % (bank, case), r32)):
                out[prefix + "loss"], out[prefix + "dx"] = r[0], r[1]
                if y_grad:
                    out[prefix + "dy"] = r[2]
            out["%s/%s/gap" % (bank, case)] = np.float64(r64[4])
            print("%s %-14s seed %d coefficients %6d smallest gap %.3e loss %.9f (fp32 %.9f)" % (bank, case, seed, r64[3].numel(), r64[4], r64[0], r32[0]))
    torch.set_default_dtype(torch.float64)
    for bank in BANKS:
        fwd = DTCWTForward(biort=taps[bank][0], qshift=taps[bank][1])
        for name in FWD_BUFS:
            out["%s/buf_%s" % (bank, name)] = getattr(fwd, name).numpy()
    torch.set_default_dtype(torch.float32)
    path = os.path.join(ROOT, "tests", "golden", "golden_cwt_loss.npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size >= 1 << 20:
        raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
