"""Write tests/golden/golden_phase.npz: the reference's own ``phase_consistency_loss`` (model.py:36-58) on the CPU.

Runs where the reference checkout exists only (oracle/ref_shim.py imports its modules and turns the mask's ``.cuda()`` into a
no-op on a machine without a GPU).  For three batch-1 shapes the file holds the seeded inputs, the reference's fp32 loss and its
autograd gradients with respect to both inputs.  The fixture is data; the tests read it and never the reference.

    python tools/gen_golden_phase.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim              # noqa: E402

SHAPES = ((64, 64), (48, 80), (31, 50))


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    R = ref_shim.load()
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    crit = R.model.phase_consistency_loss()
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(1000 + i)
        x = torch.tanh(torch.randn(1, 1, H, W, generator=g))
        y = torch.tanh(x + 0.3 * torch.randn(1, 1, H, W, generator=g))
        x.requires_grad_(True)
        y.requires_grad_(True)
        loss = crit(x, y)
        loss.backward()
        tag = "%dx%d" % (H, W)
        out["x_" + tag], out["y_" + tag] = x.detach().numpy(), y.detach().numpy()
        out["loss_" + tag] = loss.detach().numpy().astype(np.float32)
        out["gx_" + tag], out["gy_" + tag] = x.grad.numpy(), y.grad.numpy()
        print(tag, "loss", float(loss.detach()), "|gx|", float(x.grad.norm()), "|gy|", float(y.grad.norm()))
    out["shapes"] = np.array(SHAPES, dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "golden_phase.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
