"""Write tests/golden/golden_ffl.npz: the focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021) by its literal definition.

The reference tree does not contain this loss, so the fixture is the definition itself, run with ``torch.fft`` on the CPU in
float64 and in float32 with gradients by autograd:

    D = fft2(x, norm="ortho") - fft2(y, norm="ortho")        per (n, c) plane
    q = Re(D)^2 + Im(D)^2
    w = sqrt(q)^alpha;  log_matrix: w = log(w + 1);  w = w / max(w) over the plane (batch_matrix: over the batch)
    w[isnan(w)] = 0;  w = clamp(w, 0, 1), detached
    L = mean(w * q)

Per case the file holds the seeded fp32 inputs and, per setting (alpha, log_matrix, batch_matrix), the float64 and float32
losses, the float32 run's relative L2 gradient error against float64 and the float64 gradient's norm.  The float64 gradient
itself (with respect to x; the one with respect to y is checked here to be its exact negation) is stored for the cases of at
most 10000 elements, which keeps the file below 1 MiB.  The fixture is data; the tests read it.

    python tools/gen_golden_ffl.py
"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = ((1.0, False, False), (0.5, True, False), (2.0, False, True), (0.0, False, False))
SHAPES = ((1, 1, 2, 2), (1, 1, 2, 3), (3, 1, 63, 50), (2, 1, 65, 70), (2, 2, 96, 64))
SAME = (3, 1, 16, 16)                # one more case: its middle sample has y == x (the NaN -> 0 rule)
FULL_GRADIENT_MAX = 10000


def definition(x, y, alpha, log_matrix, batch_matrix, dtype):
    """(loss, dL/dx, dL/dy) of the literal definition in ``dtype`` on the CPU."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    D = torch.fft.fft2(x, norm="ortho") - torch.fft.fft2(y, norm="ortho")
    q = D.real ** 2 + D.imag ** 2
    with torch.no_grad():
        w = torch.sqrt(q) ** alpha
        if log_matrix:
            w = torch.log(w + 1)
        w = w / (w.max() if batch_matrix else w.amax(dim=(-2, -1), keepdim=True))
        w[torch.isnan(w)] = 0
        w = torch.clamp(w, 0, 1)
    loss = (w * q).mean()
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach(), gx, gy


def tag_of(shape, setting):
    return "%s_a%g_l%d_b%d" % ("x".join(str(s) for s in shape), setting[0], setting[1], setting[2])


def main():
    out = {}
    cases = list(SHAPES) + [SAME]
    for i, shape in enumerate(cases):
        g = torch.Generator().manual_seed(2000 + i)
        x = torch.tanh(torch.randn(*shape, generator=g))
        y = torch.tanh(x + 0.3 * torch.randn(*shape, generator=g))
        if shape == SAME:
            y[1] = x[1]
        case = "x".join(str(s) for s in shape)
        out["x_" + case], out["y_" + case] = x.numpy(), y.numpy()
        for st in SETTINGS:
            l64, gx64, gy64 = definition(x, y, *st, torch.float64)
            l32, gx32, gy32 = definition(x, y, *st, torch.float32)
            assert torch.equal(gy64, -gx64) and torch.equal(gy32, -gx32)
            t = tag_of(shape, st)
            out["loss64_" + t] = np.float64(l64.item())
            out["loss32_" + t] = np.float32(l32.item())
            out["gnorm64_" + t] = np.float64(gx64.norm().item())
            out["gerr32_" + t] = np.float64(((gx32.double() - gx64).norm() / gx64.norm()).item())
            if x.numel() <= FULL_GRADIENT_MAX:
                out["gx64_" + t] = gx64.numpy()
            print("%-28s loss64 %.12e  loss32 rel err %.2e  |gx| %.4e  gx32 rel err %.2e"
                  % (t, l64.item(), abs(l32.item() - l64.item()) / abs(l64.item()), out["gnorm64_" + t], out["gerr32_" + t]))
    out["shapes"] = np.array(cases, dtype=np.int64)
    out["settings"] = np.array([[a, float(l), float(b)] for a, l, b in SETTINGS], dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "golden_ffl.npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
