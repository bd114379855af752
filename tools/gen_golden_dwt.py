"""Write tests/golden/golden_dwt*.npz: the reference's own ``DWTForward`` / ``DWTInverse`` on the CPU, with the taps passed as tuples.

Runs where the reference checkout exists only (oracle/ref_shim.py imports its modules; its PyWavelets stand-in knows no tables,
so every bank goes in as tap arrays computed by ``faoctasr.daubechies``).  Cases:

  a  single level, banks db2, db4 and the 4-tuple (db2 first pair, db4 second pair), the five modes, sizes 16x16, 13x18 and the
     small case (5x7 for db2, 9x6 otherwise), N x C = 2 x 2               -> golden_dwt.npz, golden_dwt_a_mixed.npz (4-tuple)
  b  1x3x70x150, db4, 'symmetric' and 'periodization' (more than one tile per axis)             -> golden_dwt_b_<mode>.npz
  c  J = 3, db4, 2x1x64x48 and 2x1x45x52, 'symmetric', 'reflect', 'periodization'              -> golden_dwt_c_<mode>.npz

Per case: the seeded N(0,1) input (shared by the cases of one size), yl and every yh[j], the reference's x.grad for coded
cotangents, the inverse of the coefficients, its gradients with respect to yl and yh[0], and one inverse with a level set to
None (the last level of yh, i.e. the coarsest; for J = 1 the only one).  Where the reference itself raises -- 'reflect' goes
through F.pad, which wants the pad (L - 2 resp. L - 1 a side) below the image side: db4 at 9x6 -- the case holds the key
``reference_refuses`` only, and the tests compare that case with their float64 restatement alone.  Cotangents are stored as
uint16 codes k, standing for the exactly representable k / 65536 - 0.5.  Per bank: the eight buffers the reference registers.  The float arrays are full
fp32 results, which is why the cases are spread over several files: each stays below 1 MiB.  The fixtures are data; the tests
read them and never the reference.

    python tools/gen_golden_dwt.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim              # noqa: E402
import faoctasr                          # noqa: E402

MODES = ("zero", "symmetric", "reflect", "periodic", "periodization")


def banks():
    d2, d4 = faoctasr.daubechies(2), faoctasr.daubechies(4)
    return {
        "db2": ((d2.dec_lo, d2.dec_hi), (d2.rec_lo, d2.rec_hi)),
        "db4": ((d4.dec_lo, d4.dec_hi), (d4.rec_lo, d4.rec_hi)),
        "db2db4": ((d2.dec_lo, d2.dec_hi, d4.dec_lo, d4.dec_hi), (d2.rec_lo, d2.rec_hi, d4.rec_lo, d4.rec_hi)),
    }


def cases():
    """(file tag, bank, mode, J, shape)"""
    out = []
    for bank in ("db2", "db4", "db2db4"):
        for mode in MODES:
            for hw in ((16, 16), (13, 18), (5, 7) if bank == "db2" else (9, 6)):
                out.append(("_a_mixed" if bank == "db2db4" else "", bank, mode, 1, (2, 2) + hw))
    for mode in ("symmetric", "periodization"):
        out.append(("_b_" + mode, "db4", mode, 1, (1, 3, 70, 150)))
    for mode in ("symmetric", "reflect", "periodization"):
        for shape in ((2, 1, 64, 48), (2, 1, 45, 52)):
            out.append(("_c_" + mode, "db4", mode, 3, shape))
    return out


def case_id(bank, mode, J, shape):
    return "%s_%s_J%d_%dx%dx%dx%d" % ((bank, mode, J) + tuple(shape))


def cot_codes(shape, seed):
    n = int(np.prod(shape))
    k = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 7919 + 12345)) * np.uint64(2654435761)
    return ((k >> np.uint64(7)) % np.uint64(65536)).astype(np.uint16).reshape(shape)


def decode(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5))


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    R = ref_shim.load()
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    files = {}
    B = banks()
    for n, (tag, bank, mode, J, shape) in enumerate(cases()):
        out = files.setdefault(tag, {})
        fwd, inv = R.DWTForward(J=J, wave=B[bank][0], mode=mode), R.DWTInverse(wave=B[bank][1], mode=mode)
        for name in ("h0_col", "h1_col", "h0_row", "h1_row"):
            out["buf_%s_%s" % (bank, name)] = getattr(fwd, name).numpy()
        for name in ("g0_col", "g1_col", "g0_row", "g1_row"):
            out["buf_%s_%s" % (bank, name)] = getattr(inv, name).numpy()
        xkey = "x_%dx%dx%dx%d" % shape
        if xkey not in out:
            g = torch.Generator().manual_seed(4000 + 131 * shape[2] + shape[3])
            out[xkey] = torch.randn(*shape, generator=g).numpy()
        cid = case_id(bank, mode, J, shape)
        x = torch.from_numpy(out[xkey]).clone().requires_grad_(True)
        try:
            yl, yh = fwd(x)
        except RuntimeError as e:           # F.pad refuses a reflect pad that is not below the side (db4 at 9x6 pads W = 6 by 6)
            out[cid + "/reference_refuses"] = np.array(str(e).split(",")[0])
            print(cid, "the reference raises:", e)
            continue
        out[cid + "/yl"] = yl.detach().numpy()
        cots = [cot_codes(tuple(yl.shape), n)]
        for j, h in enumerate(yh):
            out[cid + "/yh%d" % j] = h.detach().numpy()
            cots.append(cot_codes(tuple(h.shape), n + 100 * (j + 1)))
        out[cid + "/cot_yl"] = cots[0]
        for j in range(J):
            out[cid + "/cot_yh%d" % j] = cots[j + 1]
        torch.autograd.backward([yl] + list(yh), [decode(c) for c in cots])
        out[cid + "/xgrad"] = x.grad.numpy()
        cl = yl.detach().clone().requires_grad_(True)
        ch = [h.detach().clone() for h in yh]
        ch[0].requires_grad_(True)
        y = inv((cl, ch))
        out[cid + "/inv"] = y.detach().numpy()
        cy = cot_codes(tuple(y.shape), n + 5000)
        out[cid + "/cot_inv"] = cy
        y.backward(decode(cy))
        out[cid + "/inv_gyl"] = cl.grad.numpy()
        out[cid + "/inv_gyh0"] = ch[0].grad.numpy()
        with torch.no_grad():
            out[cid + "/inv_none"] = inv((yl.detach(), [h.detach() for h in yh[:-1]] + [None])).numpy()
        print(cid, "yl", tuple(yl.shape), "inv", tuple(y.shape))
    for tag, out in files.items():
        path = os.path.join(ROOT, "tests", "golden", "golden_dwt%s.npz" % tag)
        np.savez(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        if size >= 1 << 20:
            raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
