"""Write tests/golden/golden_msssim.npz: multi-scale SSIM (Wang, Simoncelli & Bovik 2003)

    MS[n] = prod_j max(F_j[n], 0)^w_j,   F_j[n] = mean_{c,h,w} cs_p at scale j < M,   F_M[n] = mean l_p cs_p at scale M,

scale 1 the input and scale j + 1 = ``F.avg_pool2d(scale j, 2)``.  Every scale is the reference's own ``ssim.create_window`` and the
``F.conv2d`` lines of ssim.py:17-32 with the cs factor split out, run on the CPU once in float64 and once in float32; the gradients
of the result (the mean over n, or the sum of the per-image scores) come from autograd.  Runs where the reference checkout exists
only (oracle/ref_shim.py).

Inputs: x = 5x5-box-smoothed N(0, 1) noise times 2, clipped to [-1, 1]; y = clip(x + 0.15 n); float32 values, one pair per shape.
``w_j MS / F_j`` amplifies rounding where a factor is small: the script asserts that every F_j[n] of the float64 run is at least
0.25, and that its levels = 1 case equals the reference's ``ssim.ssim`` on the same inputs.

Per shape ``in/<shape>/x``, ``in/<shape>/y``; per case ``<case>/score`` (0-d, or (N,)), ``factors`` (M, N), ``dx``, ``dy`` (float64;
no ``dy`` where only x needs a gradient) and ``<case>/f32/...`` (float32).  The file stays below 1 MiB.

    python tools/gen_golden_msssim.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim              # noqa: E402

DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
FACTOR_CAP = 0.25
#: (case, shape, levels, weights or None, data_range, per image, y needs a gradient)
CASES = (("m5_mean", (2, 2, 32, 48), 5, None, 1.0, False, True),
         ("m5_per_image", (2, 2, 32, 48), 5, None, 1.0, True, True),
         ("m3_weights_range2", (2, 2, 32, 48), 3, (0.2, 0.5, 0.3), 2.0, False, True),
         ("m5_odd", (1, 1, 37, 53), 5, None, 1.0, False, True),
         ("m1", (1, 3, 16, 24), 1, (1.0,), 1.0, False, True),
         ("m5_xonly", (2, 2, 32, 48), 5, None, 1.0, False, False))


def shape_key(shape):
    return "%dx%dx%dx%d" % tuple(shape)


def make_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(*shape, generator=g, dtype=torch.float32)
    box = torch.ones(shape[1], 1, 5, 5) / 25.0
    x = (2.0 * F.conv2d(n, box, padding=2, groups=shape[1])).clamp(-1.0, 1.0)
    y = (x + 0.15 * torch.randn(*shape, generator=g, dtype=torch.float32)).clamp(-1.0, 1.0)
    return x, y


def scale_factors(ref_ssim, a, b, C1, C2):
    """(mean cs, mean l cs) per image of one scale: ssim.py:17-32 with the cs factor split out."""
    channel = a.shape[1]
    window = ref_ssim.create_window(11, channel).type_as(a)
    mu1 = F.conv2d(a, window, padding=5, groups=channel)
    mu2 = F.conv2d(b, window, padding=5, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(a * a, window, padding=5, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(b * b, window, padding=5, groups=channel) - mu2_sq
    sigma12 = F.conv2d(a * b, window, padding=5, groups=channel) - mu1_mu2
    cs = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    lum = (2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)
    return cs.mean(dim=(1, 2, 3)), (lum * cs).mean(dim=(1, 2, 3))


def run(ref_ssim, x, y, levels, weights, data_range, per_image, y_grad, dtype):
    """(score, factors (M, N), dx, dy or None) of one run in ``dtype``."""
    x = x.to(dtype).clone().requires_grad_(True)
    y = y.to(dtype).clone().requires_grad_(y_grad)
    w = weights or DEFAULT_WEIGHTS[:levels]
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a, b, factors = x, y, []
    for j in range(levels):
        cs, lcs = scale_factors(ref_ssim, a, b, C1, C2)
        factors.append(lcs if j == levels - 1 else cs)
        if j < levels - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    ms = torch.ones_like(factors[0])
    for f, wj in zip(factors, w):
        ms = ms * f.clamp(min=0) ** wj
    score = ms if per_image else ms.mean()
    score.sum().backward()
    return (score.detach().numpy(), torch.stack(factors).detach().numpy(), x.grad.numpy(), y.grad.numpy() if y_grad else None)


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref = ref_shim.load()
    if torch.cuda.is_available():
        raise SystemExit("the fixture is the reference's CPU result: run this on a machine without a GPU")
    out = {}
    for k, shape in enumerate(sorted(set(c[1] for c in CASES))):
        x, y = make_pair(shape, 9800 + k)
        out["in/%s/x" % shape_key(shape)], out["in/%s/y" % shape_key(shape)] = x.numpy(), y.numpy()
    for case, shape, levels, weights, data_range, per_image, y_grad in CASES:
        x, y = (torch.from_numpy(out["in/%s/%s" % (shape_key(shape), n)]) for n in "xy")
        r64 = run(ref.ssim, x, y, levels, weights, data_range, per_image, y_grad, torch.float64)
        r32 = run(ref.ssim, x, y, levels, weights, data_range, per_image, y_grad, torch.float32)
        assert r64[1].min() >= FACTOR_CAP, "%s: smallest factor %.3f is below the conditioning cap %.2f" % (case, r64[1].min(), FACTOR_CAP)
        if levels == 1:
            for dtype, r in ((torch.float64, r64), (torch.float32, r32)):
                ref_score = ref.ssim.ssim(x.to(dtype), y.to(dtype)).numpy()
                assert abs(float(ref_score) - float(r[0])) <= 4 * np.finfo(r[0].dtype).eps, (case, ref_score, r[0])
        for prefix, r in ((case + "/", r64), (case + "/f32/", r32)):
            out[prefix + "score"], out[prefix + "factors"], out[prefix + "dx"] = r[0], r[1], r[2]
            if y_grad:
                out[prefix + "dy"] = r[3]
        print("%-18s smallest factor %.3f score %s (fp32 %s)" % (case, r64[1].min(), np.array2string(r64[0], precision=12),
                                                                 np.array2string(r32[0], precision=9)))
    path = os.path.join(ROOT, "tests", "golden", "golden_msssim.npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size >= 1 << 20:
        raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


if __name__ == "__main__":
    main()
