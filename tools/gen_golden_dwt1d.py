"""Write tests/golden/golden_dwt1d*.npz: the reference's own ``DWT1DForward`` / ``DWT1DInverse`` on the CPU, with the taps passed as
(lo, hi) tuples computed by ``faoctasr.daubechies`` (the reference's PyWavelets stand-in knows no tables).

Runs where the reference checkout exists only (oracle/ref_shim.py puts its modules on the path).  Cases, N x C = 2 x 3, banks db2
and db4, the five modes:

  J = 1 at lengths 16, 13 and the minimum L/2 + 1 (3 for db2, 5 for db4)                -> golden_dwt1d.npz
  J = 3 at lengths 64 and 301                                                           -> golden_dwt1d_j3_<bank>.npz

Per case: the seeded N(0,1) input (shared by the cases of one length), yl and every yh[j], the reference's x.grad for coded
cotangents, the inverse of the coefficients, its gradients with respect to yl and yh[0], and one inverse with the coarsest
level set to None.  Cotangents are stored as uint16 codes k, standing for the exactly representable k / 65536 - 0.5 (the coding
of tools/gen_golden_dwt.py).  Where the reference itself raises -- 'reflect' goes through F.pad, which wants the pad below the
signal's length: the two minimum-length 'reflect' cases, and only those (asserted) -- the case holds the key
``reference_refuses`` only.  Per bank: the four buffers the reference registers.  Every file stays below 1 MiB.

    python tools/gen_golden_dwt1d.py
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
BANKS = {"db2": 2, "db4": 4}


def cases():
    """(file tag, bank, mode, J, shape)"""
    out = []
    for bank, N in BANKS.items():
        for mode in MODES:
            for n in (16, 13, N + 1):
                out.append(("", bank, mode, 1, (2, 3, n)))
            for n in (64, 301):
                out.append(("_j3_" + bank, bank, mode, 3, (2, 3, n)))
    return out


def case_id(bank, mode, J, shape):
    return "%s_%s_J%d_%dx%dx%d" % ((bank, mode, J) + tuple(shape))


def cot_codes(shape, seed):
    n = int(np.prod(shape))
    k = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 7919 + 12345)) * np.uint64(2654435761)
    return ((k >> np.uint64(7)) % np.uint64(65536)).astype(np.uint16).reshape(shape)


def decode(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5))


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref_shim.load()
    from pytorch_wavelets import DWT1DForward, DWT1DInverse
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    files = {}
    for n, (tag, bank, mode, J, shape) in enumerate(cases()):
        out = files.setdefault(tag, {})
        w = faoctasr.daubechies(BANKS[bank])
        fwd, inv = DWT1DForward(J=J, wave=(w.dec_lo, w.dec_hi), mode=mode), DWT1DInverse(wave=(w.rec_lo, w.rec_hi), mode=mode)
        for mod, names in ((fwd, ("h0", "h1")), (inv, ("g0", "g1"))):
            for name in names:
                out["buf_%s_%s" % (bank, name)] = getattr(mod, name).numpy()
        xkey = "x_%dx%dx%d" % shape
        if xkey not in out:
            g = torch.Generator().manual_seed(7000 + shape[2])
            out[xkey] = torch.randn(*shape, generator=g).numpy()
        cid = case_id(bank, mode, J, shape)
        x = torch.from_numpy(out[xkey]).clone().requires_grad_(True)
        try:
            yl, yh = fwd(x)
        except RuntimeError as e:           # F.pad refuses a reflect pad that is not below the length
            assert mode == "reflect" and J == 1 and shape[2] == BANKS[bank] + 1, (cid, e)
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
        path = os.path.join(ROOT, "tests", "golden", "golden_dwt1d%s.npz" % tag)
        np.savez(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        if size >= 1 << 20:
            raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
