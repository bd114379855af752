"""Write tests/golden/golden_dtcwt_<bank>_<mode>.npz: the reference's own ``DTCWTForward`` / ``DTCWTInverse`` on the CPU, once in
float64 and once in float32, with the taps passed as tuples (read from the reference's tap tables, which are data files).

Runs where the reference checkout exists only (oracle/ref_shim.py puts its modules on the path).  Bank pairs:

  a  near_sym_a (5, 7 taps) + qshift_a (10 taps, m/2 odd): the defaults
  b  near_sym_b (13, 19 taps) + qshift_c (16 taps, m/2 even)
  c  legall (5, 3 taps) + qshift_d (18 taps, m/2 odd)

modes 'symmetric' and 'zero', shapes (2,3,16,24) J = 3, (1,2,13,18) J = 3 (odd: the last row is repeated, every later level needs
the pad to a multiple of 4 and the inverse its crop), (1,1,4,4) J = 3 (many folds, 1 x 1 bands) and (1,2,40,36) J = 2.

Per case: the seeded N(0,1) input (shared by the cases of one shape), yl and every yh[j], the reference's x.grad for coded
cotangents, the inverse of the coefficients, its gradients with respect to yl and yh[0], one inverse with the coarsest bandpass
set to None, and one forward with ``skip_hps = [False, True, False ...]`` (yl and the computed levels but the first, which
repeats yh0).  Cotangents are stored as uint16 codes k, standing for the exactly representable k / 65536 - 0.5 (the coding of
tools/gen_golden_dwt.py).  Every array twice: ``<case>/<name>`` from the float64 run, ``<case>/f32/<name>`` from the float32 one
(the input holds float32 values, and both inverses run on the float64 coefficients rounded to float32).  Per bank: the twelve buffers the reference registers,
in float64.  Every file stays below 1 MiB.

    python tools/gen_golden_dtcwt.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim              # noqa: E402

BANKS = {"a": ("near_sym_a", "qshift_a"), "b": ("near_sym_b", "qshift_c"), "c": ("legall", "qshift_d")}
MODES = ("symmetric", "zero")
SHAPES = (((2, 3, 16, 24), 3), ((1, 2, 13, 18), 3), ((1, 1, 4, 4), 3), ((1, 2, 40, 36), 2))
FWD_BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")
INV_BUFS = ("g0o", "g1o", "g0a", "g0b", "g1a", "g1b")


def case_id(bank, mode, J, shape):
    return "%s_%s_J%d_%dx%dx%dx%d" % ((bank, mode, J) + tuple(shape))


def cot_codes(shape, seed):
    n = int(np.prod(shape))
    k = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 7919 + 12345)) * np.uint64(2654435761)
    return ((k >> np.uint64(7)) % np.uint64(65536)).astype(np.uint16).reshape(shape)


def decode(codes, dtype):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5)).to(dtype)


def tables(bank):
    """The (biort, qshift) tap tuples of a bank pair for the forward and for the inverse, from the reference's data files."""
    from pytorch_wavelets.dtcwt.coeffs import biort, qshift
    h0o, g0o, h1o, g1o = biort(BANKS[bank][0])
    h0a, h0b, g0a, g0b, h1a, h1b, g1a, g1b = qshift(BANKS[bank][1])
    return ((h0o, h1o), (h0a, h0b, h1a, h1b)), ((g0o, g1o), (g0a, g0b, g1a, g1b))


def run_case(out, prefix, fwd_cls, inv_cls, taps, mode, J, x, cots, coeffs64, cot_inv, dtype):
    torch.set_default_dtype(dtype)
    (fb, fq), (ib, iq) = taps
    fwd, inv = fwd_cls(biort=fb, qshift=fq, J=J, mode=mode), inv_cls(biort=ib, qshift=iq, mode=mode)
    x = x.to(dtype).clone().requires_grad_(True)
    yl, yh = fwd(x)
    out[prefix + "yl"] = yl.detach().numpy()
    for j, h in enumerate(yh):
        out[prefix + "yh%d" % j] = h.detach().numpy()
    torch.autograd.backward([yl] + list(yh), [decode(c, dtype) for c in cots(yl, yh)])
    out[prefix + "xgrad"] = x.grad.numpy()
    if coeffs64 is None:                    # the inverse's input: the float64 coefficients rounded to float32, in both runs
        coeffs64 = (yl.detach().float(), [h.detach().float() for h in yh])
    cl = coeffs64[0].to(dtype).clone().requires_grad_(True)
    ch = [h.to(dtype).clone() for h in coeffs64[1]]
    ch[0].requires_grad_(True)
    y = inv((cl, ch))
    out[prefix + "inv"] = y.detach().numpy()
    y.backward(decode(cot_inv(y), dtype))
    out[prefix + "inv_gyl"], out[prefix + "inv_gyh0"] = cl.grad.numpy(), ch[0].grad.numpy()
    with torch.no_grad():
        out[prefix + "inv_none"] = inv((cl.detach(), [h.detach() for h in ch[:-1]] + [None])).numpy()
        skip = [False, True] + [False] * (J - 2)
        sl, sh = fwd_cls(biort=fb, qshift=fq, J=J, mode=mode, skip_hps=skip)(x.detach())
        out[prefix + "skip_yl"] = sl.numpy()
        for j in range(2, J):
            out[prefix + "skip_yh%d" % j] = sh[j].numpy()
        assert sh[1].shape == torch.Size([]) and torch.equal(sh[0], yh[0])
    torch.set_default_dtype(torch.float32)
    return coeffs64, fwd, inv


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref_shim.load()
    from pytorch_wavelets import DTCWTForward, DTCWTInverse
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    n = 0
    for bank in BANKS:
        taps = tables(bank)
        for mode in MODES:
            out = {}
            for shape, J in SHAPES:
                n += 1
                cid = case_id(bank, mode, J, shape)
                g = torch.Generator().manual_seed(8000 + shape[2] * 100 + shape[3])
                x = torch.randn(*shape, generator=g, dtype=torch.float32).double()     # float32 values: both runs read the same input
                out["x_%dx%dx%dx%d" % shape] = x.numpy()

                def cots(yl, yh, n=n, cid=cid):
                    c = [cot_codes(tuple(yl.shape), n)] + [cot_codes(tuple(h.shape), n + 100 * (j + 1)) for j, h in enumerate(yh)]
                    out[cid + "/cot_yl"] = c[0]
                    for j in range(len(yh)):
                        out[cid + "/cot_yh%d" % j] = c[j + 1]
                    return c

                def cot_inv(y, n=n, cid=cid):
                    out[cid + "/cot_inv"] = cot_codes(tuple(y.shape), n + 5000)
                    return out[cid + "/cot_inv"]

                coeffs, fwd, inv = run_case(out, cid + "/", DTCWTForward, DTCWTInverse, taps, mode, J, x, cots, None, cot_inv, torch.float64)
                run_case(out, cid + "/f32/", DTCWTForward, DTCWTInverse, taps, mode, J, x, cots, coeffs, cot_inv, torch.float32)
                print(cid, "yl", out[cid + "/yl"].shape, "inv", out[cid + "/inv"].shape)
            torch.set_default_dtype(torch.float64)
            (fb, fq), (ib, iq) = taps
            fwd, inv = DTCWTForward(biort=fb, qshift=fq), DTCWTInverse(biort=ib, qshift=iq)
            torch.set_default_dtype(torch.float32)
            for mod, names in ((fwd, FWD_BUFS), (inv, INV_BUFS)):
                for name in names:
                    out["buf_%s" % name] = getattr(mod, name).numpy()
            path = os.path.join(ROOT, "tests", "golden", "golden_dtcwt_%s_%s.npz" % (bank, mode))
            np.savez(path, **out)
            size = os.path.getsize(path)
            print("wrote", path, size, "bytes")
            if size >= 1 << 20:
                raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
