"""Write tests/golden/golden_tv.npz: the reference's own ``TVLoss`` (model.py:17-33) on the CPU.

Runs where the reference checkout exists only (oracle/ref_shim.py imports its modules).  For four small shapes -- batch and
channel counts above 1, odd sizes, a 2x2 image -- the file holds the seeded input ``tanh(randn)`` and, for the weights 1 and 0.5,
the reference's fp32 loss and its autograd gradient.  The fixture is data; the tests read it and never the reference.

    python tools/gen_golden_tv.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim              # noqa: E402

SHAPES = ((1, 1, 64, 64), (2, 1, 48, 80), (2, 3, 31, 50), (1, 1, 2, 2))
WEIGHTS = (1.0, 0.5)


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    R = ref_shim.load()
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    out = {}
    for i, shape in enumerate(SHAPES):
        g = torch.Generator().manual_seed(2000 + i)
        x = torch.tanh(torch.randn(*shape, generator=g))
        tag = "%dx%dx%dx%d" % shape
        out["x_" + tag] = x.numpy()
        for w in WEIGHTS:
            xr = x.clone().requires_grad_(True)
            loss = R.model.TVLoss(TVLoss_weight=w)(xr)
            loss.backward()
            out["loss_w%g_%s" % (w, tag)] = loss.detach().numpy().astype(np.float32)
            out["g_w%g_%s" % (w, tag)] = xr.grad.numpy()
            print(tag, "weight", w, "loss", float(loss.detach()), "|g|", float(xr.grad.norm()))
    out["shapes"] = np.array(SHAPES, dtype=np.int64)
    out["weights"] = np.array(WEIGHTS, dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "golden_tv.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
