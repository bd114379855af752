"""Write tests/golden/golden_swt*.npz: the reference's own ``afb2d_atrous`` on the CPU, level by level.

Runs where the reference checkout exists only (oracle/ref_shim.py puts its modules on the path).  The reference's ``SWTForward``
does not run past its constructor (its default mode is refused by its own pad, a second level indexes the wrong axis), so the
levels are chained here by hand: level j is ``afb2d_atrous(ll, filts, mode, 2**j)`` with the four filters prepared by
``prep_filt_afb2d``, its (N, 4C, H, W) result viewed as the documented (N, C, 4, H, W), and ``ll`` of the next level its band 0.
Cases:

  a  J = 1, banks db2, db4 and the 4-tuple (db2 on col, db4 on row), the modes zero, symmetric, reflect, periodic, 2x2x13x18;
     db4 at its J = 2 minimum 1x1x9x9, the four modes                                                 -> golden_swt.npz
  b  db4, J = 2, 1x1x70x150 (several tiles per axis, odd tile remainders), the four modes             -> golden_swt_b_<mode>.npz

Per case: the seeded N(0,1) input (shared by the cases of one size), every level's output ``y<j>``, and the reference's x.grad
(autograd through its pad and its dilated convolutions) for coded cotangents ``cot_y<j>`` on every level -- uint16 codes k
standing for the exactly representable k / 65536 - 0.5, as in tools/gen_golden_dwt.py.  Per bank: the four buffers
``prep_filt_afb2d`` makes.  Each file stays below 1 MiB.  The fixtures are data; the tests read them and never the reference.

    python tools/gen_golden_swt.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim              # noqa: E402
import faoctasr                          # noqa: E402
from gen_golden_dwt import cot_codes, decode   # noqa: E402

MODES = ("zero", "symmetric", "reflect", "periodic")
NAMES = ("h0_col", "h1_col", "h0_row", "h1_row")


def banks():
    d2, d4 = faoctasr.daubechies(2), faoctasr.daubechies(4)
    return {
        "db2": (d2.dec_lo, d2.dec_hi, d2.dec_lo, d2.dec_hi),
        "db4": (d4.dec_lo, d4.dec_hi, d4.dec_lo, d4.dec_hi),
        "db2db4": (d2.dec_lo, d2.dec_hi, d4.dec_lo, d4.dec_hi),
    }


def cases():
    """(file tag, bank, mode, J, shape)"""
    out = []
    for bank in ("db2", "db4", "db2db4"):
        for mode in MODES:
            out.append(("", bank, mode, 1, (2, 2, 13, 18)))
    for mode in MODES:
        out.append(("", "db4", mode, 2, (1, 1, 9, 9)))
    for mode in MODES:
        out.append(("_b_" + mode, "db4", mode, 2, (1, 1, 70, 150)))
    return out


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref_shim.load()
    from pytorch_wavelets.dwt import lowlevel
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    files = {}
    B = banks()
    for n, (tag, bank, mode, J, shape) in enumerate(cases()):
        out = files.setdefault(tag, {})
        filts = lowlevel.prep_filt_afb2d(*B[bank])
        for name, f in zip(NAMES, filts):
            out["buf_%s_%s" % (bank, name)] = f.numpy()
        xkey = "x_%dx%dx%dx%d" % shape
        if xkey not in out:
            g = torch.Generator().manual_seed(7000 + 131 * shape[2] + shape[3])
            out[xkey] = torch.randn(*shape, generator=g).numpy()
        cid = "%s_%s_J%d_%dx%dx%dx%d" % ((bank, mode, J) + shape)
        x = torch.from_numpy(out[xkey]).clone().requires_grad_(True)
        N, C, H, W = shape
        ys, ll = [], x
        for j in range(J):
            y = lowlevel.afb2d_atrous(ll, filts, mode, 2 ** j)
            assert tuple(y.shape) == (N, 4 * C, H, W), tuple(y.shape)
            y = y.reshape(N, C, 4, H, W)
            ys.append(y)
            ll = y[:, :, 0]
        cots = [cot_codes(tuple(y.shape), n + 100 * j) for j, y in enumerate(ys)]
        for j, y in enumerate(ys):
            out[cid + "/y%d" % j] = y.detach().numpy()
            out[cid + "/cot_y%d" % j] = cots[j]
        torch.autograd.backward(ys, [decode(c) for c in cots])
        out[cid + "/xgrad"] = x.grad.numpy()
        print(cid, [tuple(y.shape) for y in ys])
    for tag, out in files.items():
        path = os.path.join(ROOT, "tests", "golden", "golden_swt%s.npz" % tag)
        np.savez(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        if size >= 1 << 20:
            raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
