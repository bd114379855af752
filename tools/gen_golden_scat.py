"""Write tests/golden/golden_scat_<bank>.npz: the reference's own ``ScatLayer`` / ``ScatLayerj2`` (scatternet/layers.py) on the CPU,
once in float64 and once in float32.

Runs where the reference checkout exists only (oracle/ref_shim.py puts its modules on the path).  Bank pairs, as
tools/gen_golden_dtcwt.py names them:

  a  near_sym_a (5, 7 taps) + qshift_a (10 taps, m/2 odd): the defaults
  b  near_sym_b (13, 19 taps) + qshift_c (16 taps, m/2 even)
  c  legall (5, 3 taps) + qshift_d (18 taps, m/2 odd)

``ScatLayer`` in the modes 'symmetric' and 'zero' on (2,3,16,24) with and without ``combine_colour``, (1,2,13,19) (odd both ways:
the last row and column are repeated) and (1,1,2,2) (a 1 x 1 output: every tap folds); ``ScatLayerj2`` in 'symmetric' on
(2,3,16,24) with and without ``combine_colour``, (1,2,13,19) (padded to 16 x 24 by its own leading and trailing rows) and (1,1,8,8).
magbias is the default, 1e-2.

Per case: the seeded N(0,1) input (shared by the cases of one shape; it holds float32 values, so both runs read the same
numbers), Z, the cotangent as uint16 codes k standing for the exactly representable k / 65536 - 0.5 (the coding of
tools/gen_golden_dtcwt.py) and x.grad.  Every result twice: ``<case>/<name>`` from the float64 run, ``<case>/f32/<name>`` from the
float32 one.  Per bank: the six tap parameters the reference registers, in float64 (``buf_<name>``).  Every file stays below
1 MiB.

    python tools/gen_golden_scat.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_shim                          # noqa: E402
from gen_golden_dtcwt import BANKS, cot_codes, decode   # noqa: E402

J1_MODES = ("symmetric", "zero")
J1_SHAPES = (((2, 3, 16, 24), False), ((2, 3, 16, 24), True), ((1, 2, 13, 19), False), ((1, 1, 2, 2), False))
J2_SHAPES = (((2, 3, 16, 24), False), ((2, 3, 16, 24), True), ((1, 2, 13, 19), False), ((1, 1, 8, 8), False))
BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")


def case_id(order, mode, shape, colour):
    return "j%d_%s_%dx%dx%dx%d%s" % ((order, mode) + tuple(shape) + ("_cc" if colour else "",))


def cases():
    """(case id, order, mode, shape, combine_colour) of every case, in the order the seeds count them."""
    out = [(case_id(1, m, s, cc), 1, m, s, cc) for m in J1_MODES for s, cc in J1_SHAPES]
    return out + [(case_id(2, "symmetric", s, cc), 2, "symmetric", s, cc) for s, cc in J2_SHAPES]


def run(layer_cls, kw, x, codes, dtype):
    torch.set_default_dtype(dtype)
    try:
        layer = layer_cls(**kw)
        x = x.to(dtype).clone().requires_grad_(True)
        Z = layer(x)
        if codes is None:
            return tuple(Z.shape)
        Z.backward(decode(codes, dtype))
        return Z.detach().numpy(), x.grad.numpy()
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref_shim.load()
    from pytorch_wavelets.scatternet import ScatLayer, ScatLayerj2
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    for bank, (biort, qshift) in BANKS.items():
        out = {}
        for n, (cid, order, mode, shape, cc) in enumerate(cases(), 1):
            g = torch.Generator().manual_seed(9000 + shape[2] * 100 + shape[3])
            x = torch.randn(*shape, generator=g, dtype=torch.float32).double()
            out["x_%dx%dx%dx%d" % shape] = x.numpy()
            kw = dict(biort=biort, mode=mode, combine_colour=cc)
            if order == 2:
                kw["qshift"] = qshift
            cls = ScatLayer if order == 1 else ScatLayerj2
            codes = cot_codes(run(cls, kw, x, None, torch.float64), n)
            out[cid + "/cot"] = codes
            out[cid + "/Z"], out[cid + "/xgrad"] = run(cls, kw, x, codes, torch.float64)
            out[cid + "/f32/Z"], out[cid + "/f32/xgrad"] = run(cls, kw, x, codes, torch.float32)
            print(bank, cid, "Z", out[cid + "/Z"].shape)
        torch.set_default_dtype(torch.float64)
        layer = ScatLayerj2(biort=biort, qshift=qshift)
        torch.set_default_dtype(torch.float32)
        for name in BUFS:
            out["buf_%s" % name] = getattr(layer, name).detach().numpy()
        path = os.path.join(ROOT, "tests", "golden", "golden_scat_%s.npz" % bank)
        np.savez(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        if size >= 1 << 20:
            raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
