"""Write tests/golden/golden_mi.npz: the differentiable mutual information by its literal definition.

The reference tree scores results with a hard-histogram NMI (utils.py:209-212), which has no gradient; the soft version is not in
it, so the fixture is the definition itself, run with torch on the CPU in float64 and in float32 with gradients by autograd:

    d = (hi - lo) / K,  c_k = lo + (k + 1/2) d,  sigma = sigma_ratio d                     (hi, lo) = (1, -1)
    Wa[p, k] = softmax_k(-(x_p - c_k)^2 / (2 sigma^2)),  Wb likewise from y                  per (n, c) plane
    P = Wa^T Wb / n_pix  (bmm),  pa = P.sum(cols),  pb = P.sum(rows)
    H(q) = -sum q log(q + eps),  MI = Ha + Hb - Hab,  normalized: NMI = (Ha + Hb) / Hab      eps = 1e-6
    score = mean over the planes

Inputs: x = clip(2 box5x5(randn), -1, 1), y = clip(0.8 x^3 - 0.1 + 0.15 randn, -1, 1) -- a nonlinear intensity map plus noise,
the relation mutual information sees and a pixelwise distance does not.

Per case the file holds the seeded fp32 inputs and, per setting (K, sigma_ratio, normalized), the float64 and float32 scores,
the float32 run's relative L2 error of either gradient against float64 (e_ref), the float64 gradients' norms and the smallest
float64 MI of a plane (the conditioning guard: MI is a difference of entropies, and a comparison against a score of 1e-4 nats
would measure nothing).  The float64 gradients themselves are stored for the cases of at most 1100 elements.  The fixture is
data; the tests read it.

    python tools/gen_golden_mi.py
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = ((32, 1.0), (64, 0.5), (24, 1.0), (40, 0.75))
SHAPES = ((2, 1, 7, 9), (1, 1, 33, 31), (3, 1, 63, 50), (2, 2, 96, 64))
FULL_GRADIENT_MAX = 1100
GUARD = 0.03


def make_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(*shape, generator=g)
    x = torch.clamp(2 * F.avg_pool2d(n, 5, stride=1, padding=2), -1, 1)
    y = torch.clamp(0.8 * x ** 3 - 0.1 + 0.15 * torch.randn(*shape, generator=g), -1, 1)
    return x, y


def definition(x, y, bins, sigma_ratio, normalized, dtype, value_range=(-1.0, 1.0), eps=1e-6):
    """(score, dS/dx, dS/dy, per-plane MI) of the literal definition in ``dtype`` on the CPU."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    N, C, H, W = x.shape
    lo, hi = value_range
    d = (hi - lo) / bins
    c = lo + (torch.arange(bins, dtype=dtype) + 0.5) * d
    sigma = sigma_ratio * d

    def weights(v):
        return torch.softmax(-(v.reshape(N * C, H * W, 1) - c) ** 2 / (2 * sigma ** 2), dim=-1)

    P = torch.bmm(weights(x).transpose(1, 2), weights(y)) / (H * W)
    pa, pb = P.sum(2), P.sum(1)
    Ha = -(pa * torch.log(pa + eps)).sum(1)
    Hb = -(pb * torch.log(pb + eps)).sum(1)
    Hab = -(P * torch.log(P + eps)).sum((1, 2))
    mi = Ha + Hb - Hab
    score = ((Ha + Hb) / Hab if normalized else mi).mean()
    gx, gy = torch.autograd.grad(score, (x, y))
    return score.detach(), gx, gy, mi.detach()


def tag_of(shape, bins, sigma_ratio, normalized):
    return "%s_k%d_s%g_n%d" % ("x".join(str(s) for s in shape), bins, sigma_ratio, int(normalized))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    out = {}
    for i, shape in enumerate(SHAPES):
        x, y = make_pair(shape, 3000 + i)
        case = "x".join(str(s) for s in shape)
        out["x_" + case], out["y_" + case] = x.numpy(), y.numpy()
        for bins, sr in SETTINGS:
            for normalized in (False, True):
                s64, gx64, gy64, mi64 = definition(x, y, bins, sr, normalized, torch.float64)
                s32, gx32, gy32, _ = definition(x, y, bins, sr, normalized, torch.float32)
                t = tag_of(shape, bins, sr, normalized)
                assert float(mi64.min()) >= GUARD, (t, mi64)
                out["score64_" + t] = np.float64(s64.item())
                out["score32_" + t] = np.float32(s32.item())
                out["mi_min_" + t] = np.float64(mi64.min().item())
                out["gxnorm64_" + t], out["gynorm64_" + t] = np.float64(gx64.norm().item()), np.float64(gy64.norm().item())
                out["gxerr32_" + t], out["gyerr32_" + t] = np.float64(rel_l2(gx32, gx64)), np.float64(rel_l2(gy32, gy64))
                if x.numel() <= FULL_GRADIENT_MAX:
                    out["gx64_" + t], out["gy64_" + t] = gx64.numpy(), gy64.numpy()
                print("%-26s score64 %.12e  score32 rel err %.2e  min plane MI %.4f  e_ref gx %.2e gy %.2e"
                      % (t, s64.item(), abs(s32.item() - s64.item()) / abs(s64.item()), mi64.min().item(), out["gxerr32_" + t],
                         out["gyerr32_" + t]))
    out["shapes"] = np.array(SHAPES, dtype=np.int64)
    out["settings"] = np.array(SETTINGS, dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "golden_mi.npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
