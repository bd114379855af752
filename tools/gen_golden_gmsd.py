"""Write tests/golden/golden_gmsd.npz: GMSD (Xue, Zhang, Mou & Bovik 2014) and MS-GMSD (Zhang, Shen, Wang & Li 2017) of two images
(N, C, H, W), channels independent grey planes pooled inside an image:

    u = (x - lo) / (hi - lo), value_range = (lo, hi);  pool(t) = the 2 x 2 mean at every second pixel, an odd last row or column dropped
    Prewitt gradients, zero padding 1: gx_p = (1/3) sum_{dy = -1..1} (t[y + dy][x - 1] - t[y + dy][x + 1]), gy_p the same on the other axis
    m_p = sqrt(gx_p^2 + gy_p^2) (no epsilon),  g_p = (2 ma_p mb_p + c) / (ma_p^2 + mb_p^2 + c)
    V[n] = the population variance of g_p over c, y, x, as mean((g - mean(g))^2)
    GMSD[n] = sqrt(V[n]) on pool(u_a), pool(u_b);  MS-GMSD[n] = sqrt(sum_j w_j V_j[n]), scale 1 the mapped input, scale j + 1 = pool(scale j)

on the CPU, once in float64 and once in float32.  Gradients and pooling are explicit sums of shifted slices -- no convolution or pooling
call, so that the values do not depend on the ``F.conv2d`` / ``avg_pool2d`` restatement of tests/test_gmsd_cpu.py -- written with torch
slices, so that autograd differentiates the same code; the gradients of the result (the mean over n, or the sum of the per-image
scores) come from autograd.

Checks made before anything is written, per case:
  * central differences in float64 on five entries of x and of y (the largest gradient entry and four random ones);
  * the conditioning caps of the float64 run: over both images and every scale of positive weight min_p m_p >= 2^-10 (sqrt is not
    differentiable at 0), per image and scale mean(d^2) / V <= 8 with d = 1 - g (the variance is a difference of two means), and
    every score > 0.

Inputs: x = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = x + 0.1 noise, rounded to values that float16 holds
exactly, so that the file can keep them in two bytes; they enter every computation as float32.  Per case the first seed of range(2000)
that meets the caps is taken; the script fails if none does.

Per case ``<case>/x``, ``<case>/y`` (float16, exact; a case that names another's inputs stores none), ``<case>/score`` (0-d, or (N,)),
``dx``, ``dy`` (float64; no ``dy`` where only x needs a gradient), ``min_m``, ``ratio``, ``seed``, ``<case>/f32/score`` (float32) and
``<case>/f32/dx_delta``, ``dy_delta`` (float32): the float32 run's gradient minus the float64 gradient rounded to float32, an exact
difference of two neighbouring float32 values that compresses where the gradient itself does not; ``float32(dx) + dx_delta`` is the
float32 run's gradient bit for bit (asserted here).  The gradient of plain GMSD is constant on every 2 x 2 cell of the pooling and zero
on a dropped row or column (asserted here), so its arrays hold one value per cell, ``[..., 0:2h:2, 0:2w:2]``.

    python tools/gen_golden_gmsd.py
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_M, MAX_RATIO = 2.0 ** -10, 8.0
MS_WEIGHTS = (0.096, 0.596, 0.289, 0.019)
#: (case, shape, weights (None: plain GMSD), c, value range, per image, y needs a gradient, the case whose inputs it shares or None)
CASES = (("g8", (1, 1, 8, 8), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("mean", (2, 1, 16, 16), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("xonly", (2, 1, 16, 16), None, 0.0026, (-1.0, 1.0), False, False, "mean"),
         ("per_image_cfg", (2, 2, 32, 48), None, 0.01, (0.0, 2.0), True, True, None),
         ("channels", (1, 3, 16, 24), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("odd", (1, 1, 37, 53), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("seam", (2, 1, 40, 136), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("ms", (2, 1, 32, 48), MS_WEIGHTS, 0.0026, (-1.0, 1.0), False, True, None),
         ("ms_odd", (1, 1, 37, 53), MS_WEIGHTS, 0.0026, (-1.0, 1.0), False, True, "odd"),
         ("ms_seam", (2, 1, 40, 136), MS_WEIGHTS, 0.0026, (-1.0, 1.0), False, True, "seam"),
         ("ms2", (1, 1, 16, 16), (0.3, 0.7), 0.0026, (-1.0, 1.0), False, True, None))


def smooth(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.randn(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    x = 2.0 * smooth(n1)
    y = x + 0.1 * n2
    return x.half().float(), y.half().float()


def pool(t):
    h, w = t.shape[-2] // 2, t.shape[-1] // 2
    return (t[..., 0:2 * h:2, 0:2 * w:2] + t[..., 0:2 * h:2, 1:2 * w:2] + t[..., 1:2 * h:2, 0:2 * w:2] + t[..., 1:2 * h:2, 1:2 * w:2]) / 4.0


def magnitude(t):
    H, W = t.shape[-2:]
    p = t.new_zeros(t.shape[:-2] + (H + 2, W + 2))
    p[..., 1:1 + H, 1:1 + W] = t
    gx = gy = 0
    for d in range(3):
        gx = gx + (p[..., d:d + H, 0:W] - p[..., d:d + H, 2:2 + W])
        gy = gy + (p[..., 0:H, d:d + W] - p[..., 2:2 + H, d:d + W])
    return torch.sqrt((gx / 3.0) ** 2 + (gy / 3.0) ** 2)


def scale_variance(a, b, c):
    """(V (N,), the smallest magnitude of either image, the largest mean(d^2) / V over the images)."""
    ma, mb = magnitude(a), magnitude(b)
    g = (2 * ma * mb + c) / (ma * ma + mb * mb + c)
    V = ((g - g.mean(dim=(1, 2, 3), keepdim=True)) ** 2).mean(dim=(1, 2, 3))
    d = (1 - g).detach()
    ratio = float(((d * d).mean(dim=(1, 2, 3)) / V.detach()).max()) if float(V.detach().min()) > 0 else float("inf")
    return V, min(float(ma.detach().min()), float(mb.detach().min())), ratio


def index(x, y, weights, c, value_range):
    """(per-image scores (N,), min m, max ratio)."""
    lo, hi = value_range
    a, b = (x - lo) / (hi - lo), (y - lo) / (hi - lo)
    if weights is None:
        V, m, r = scale_variance(pool(a), pool(b), c)
        return torch.sqrt(V), m, r
    acc, ms, rs = 0, [], []
    for j, w in enumerate(weights):
        if j:
            a, b = pool(a), pool(b)
        if w > 0:
            V, m, r = scale_variance(a, b, c)
            acc = acc + w * V
            ms.append(m)
            rs.append(r)
    return torch.sqrt(acc), min(ms), max(rs)


def run(x, y, weights, c, value_range, per_image, y_grad, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    y = y.to(dtype).clone().requires_grad_(y_grad)
    rows, m, r = index(x, y, weights, c, value_range)
    score = rows if per_image else rows.mean()
    score.sum().backward()
    return {"score": score.detach().numpy(), "rows": rows.detach().numpy(), "dx": x.grad.numpy(), "dy": y.grad.numpy() if y_grad else None,
            "min_m": m, "ratio": r}


def total(x, y, weights, c, value_range, per_image):
    rows = index(x, y, weights, c, value_range)[0]
    return float(rows.sum() if per_image else rows.mean())


def check_central_differences(case, x, y, r64, weights, c, value_range, per_image, y_grad, seed):
    rng = np.random.RandomState(seed)
    h = 1e-6
    for which, g in ((0, r64["dx"]), (1, r64["dy"])) if y_grad else ((0, r64["dx"]),):
        flat = np.abs(g).reshape(-1)
        for at in [int(flat.argmax())] + [int(v) for v in rng.randint(0, flat.size, 4)]:
            d = torch.zeros(x.numel(), dtype=torch.float64)
            d[at] = h
            d = d.reshape(x.shape)
            xd, yd = x.double(), y.double()
            up = total(xd + d, yd, weights, c, value_range, per_image) if which == 0 else total(xd, yd + d, weights, c, value_range, per_image)
            dn = total(xd - d, yd, weights, c, value_range, per_image) if which == 0 else total(xd, yd - d, weights, c, value_range, per_image)
            num, ana = (up - dn) / (2 * h), float(g.reshape(-1)[at])
            # the score is a float64 value below 1: 1e-15 of rounding over 2 h is 5e-10; the third-order term is h^2 |f'''|
            assert abs(num - ana) <= 1e-5 * abs(ana) + 2e-9, (case, "dxy"[1 + which], at, num, ana)


def qualifies(x, y, weights, c, value_range):
    with torch.no_grad():
        rows, m, r = index(x.double(), y.double(), weights, c, value_range)
    return m >= MIN_M and r <= MAX_RATIO and float(rows.min()) > 0


def find_seed(shape, configs):
    """The first seed whose pair meets the caps under every configuration that uses it."""
    for seed in range(2000):
        x, y = make_pair(shape, seed)
        if all(qualifies(x, y, *cfg) for cfg in configs):
            return seed, x, y
    raise SystemExit("no seed of range(2000) meets the conditioning caps for %s" % (shape,))


def cells(g, case):
    """One value per 2 x 2 cell of a plain-GMSD gradient, after asserting that nothing else is in it."""
    H, W = g.shape[-2:]
    h, w = H // 2, W // 2
    q = g[..., 0:2 * h:2, 0:2 * w:2]
    full = np.zeros_like(g)
    full[..., :2 * h, :2 * w] = np.repeat(np.repeat(q, 2, axis=-2), 2, axis=-1)
    assert np.array_equal(full, g), case
    return np.ascontiguousarray(q)


def main():
    out, inputs = {}, {}
    for case, shape, weights, c, vr, per_image, y_grad, shared in CASES:
        if shared is None:
            users = [(k[2], k[3], k[4]) for k in CASES if k[0] == case or k[7] == case]
            seed, x, y = find_seed(shape, users)
            inputs[case] = (seed, x, y)
            out[case + "/x"], out[case + "/y"] = x.numpy().astype(np.float16), y.numpy().astype(np.float16)
            assert np.array_equal(out[case + "/x"].astype(np.float32), x.numpy()) and np.array_equal(out[case + "/y"].astype(np.float32), y.numpy())
        seed, x, y = inputs[shared or case]
        r64 = run(x, y, weights, c, vr, per_image, y_grad, torch.float64)
        r32 = run(x, y, weights, c, vr, per_image, y_grad, torch.float32)
        assert r64["min_m"] >= MIN_M and r64["ratio"] <= MAX_RATIO and r64["rows"].min() > 0, (case, r64["min_m"], r64["ratio"], r64["rows"])
        check_central_differences(case, x, y, r64, weights, c, vr, per_image, y_grad, seed)
        out[case + "/seed"], out[case + "/min_m"], out[case + "/ratio"] = np.int64(seed), np.float64(r64["min_m"]), np.float64(r64["ratio"])
        out[case + "/score"], out[case + "/f32/score"] = r64["score"], r32["score"]
        for k in ("dx", "dy") if y_grad else ("dx",):
            g64, g32 = (r64[k], r32[k]) if weights is not None else (cells(r64[k], case), cells(r32[k], case))
            out["%s/%s" % (case, k)] = g64
            near = g64.astype(np.float32)
            delta = g32 - near
            assert delta.dtype == np.float32 and np.array_equal(near + delta, g32), (case, k)
            out["%s/f32/%s_delta" % (case, k)] = delta
        e = np.abs(r32["score"].astype(np.float64) - r64["score"]).max() / np.abs(r64["score"]).max()
        print("%-14s seed %4d  min m %.2e  ratio %.3f  score %s  fp32 score error %.1e  fp32 dx error %.1e" % (
            case, seed, r64["min_m"], r64["ratio"], np.array2string(r64["score"], precision=12), e,
            np.linalg.norm(r32["dx"].astype(np.float64) - r64["dx"]) / np.linalg.norm(r64["dx"])))
    path = os.path.join(ROOT, "tests", "golden", "golden_gmsd.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_haarpsi.npz"))
    print("wrote", path, size, "bytes; golden_haarpsi.npz has", limit)


if __name__ == "__main__":
    main()
