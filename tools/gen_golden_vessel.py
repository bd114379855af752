"""Write tests/golden/golden_vessel.npz: the Hessian vesselness in Frangi's form, made continuous, and the vessel Dice index of two
images (N, C, H, W), channels independent grey planes pooled inside an image:

    u = (x - lo) / (hi - lo), value_range = (lo, hi)
    per scale sigma: R = int(3 sigma + 0.5), t = -R..R, g = exp(-t^2 / (2 sigma^2)) / sum, g1 = -t / sigma^2 g, g2 = (t^2 / sigma^4 - 1 / sigma^2) g
    a = sigma^2 (g2 along W, g along H) * u, b = sigma^2 (g1, g1) * u, d = sigma^2 (g along W, g2 along H) * u: true convolutions, zero padding;
    bright False negates a, b, d
    m = (a + d) / 2, h = (a - d) / 2, r = sqrt(h^2 + b^2), kappa = r - m, mu = m + r
    E1 = mu^2 / (2 beta^2 kappa^2), E2 = (mu^2 + kappa^2) / (2 c^2), V = exp(-E1) (1 - exp(-E2)) where kappa > 0 and E1 < 87, else 0
    Rsp = sum_s w_s V_s (weights normalised to sum 1);  S[n] = (2 mean(A B) + eps) / (mean(A^2) + mean(B^2) + eps), A = Rsp(x), B = Rsp(y)

on the CPU, once in float64 and once in float32.  The convolutions are explicit sums of shifted slices -- no convolution call, so that
the values do not depend on the ``F.conv2d`` restatement of tests/test_vessel_cpu.py -- written with torch slices, so that autograd
differentiates the same code.  Index cases differentiate the mean over n, or the sum of the per-image scores; map cases differentiate
sum(Rsp * cot) for a stored random cotangent.

Checks made before anything is written, per case:
  * the float64 Hessians against scipy.ndimage.gaussian_filter(order=(0, 2) / (1, 1) / (2, 0), mode='constant', truncate=3.0) at 1e-13;
  * central differences in float64 on five entries of x and of y (the largest gradient entry and four random ones);
  * the conditioning caps of the float64 run: min r >= 2^-14 over both images and every scale of positive weight (sqrt is not
    differentiable at 0), every image's denominator D >= 2^-6, every score > 0.

Inputs: x = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = x + 0.1 noise, rounded to values that float16 holds
exactly; they enter every computation as float32.  Per set of inputs the first seed of range(2000) that meets the caps under every
case that uses it is taken; the script fails if none does.

Per case ``<case>/x``, ``<case>/y`` (float16, exact; a case that names another's inputs stores none), ``<case>/score`` (0-d, or (N,)) or
``<case>/map`` and ``<case>/cot``, ``dx``, ``dy`` (float64, rounded to 41 significant bits: ``trim``; none where a case shares its inputs with an index case, whose ``dx`` is the
same computation, asserted here), ``min_r``, ``min_D``, ``seed``,
``<case>/f32/score`` or ``<case>/f32/map_delta`` and ``<case>/f32/dx_delta``, ``dy_delta`` (int32): the float32 run's array as the distance
of its bit pattern (as int32) from that of the float64 array rounded to float32, a few units in the last place that compress where the
values do not; ``(float32(dx).view(int32) + dx_delta).view(float32)`` is the float32 run's gradient bit for bit (asserted here).

    python tools/gen_golden_vessel.py
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_R, MIN_D = 2.0 ** -14, 2.0 ** -6
E1_MAX = 87.0
DEFAULT = dict(sigmas=(1.0, 2.0, 3.0), weights=None, beta=0.5, c=0.1, eps=1e-6, value_range=(-1.0, 1.0), bright=True)
OTHER = dict(DEFAULT, sigmas=(1.5,), beta=0.7, c=0.05, value_range=(0.0, 2.0))
HALO = dict(DEFAULT, sigmas=(0.5, 3.0), weights=(1.0, 3.0))
DARK = dict(DEFAULT, bright=False)
#: (case, shape, settings, per image, y needs a gradient, the case whose inputs it shares or None, the filter alone (a map case))
CASES = (("v8", (1, 1, 8, 8), DEFAULT, False, True, None, False),
         ("mean", (2, 1, 16, 16), DEFAULT, False, True, None, False),
         ("xonly", (2, 1, 16, 16), DEFAULT, False, False, "mean", False),
         ("per_image_cfg", (2, 2, 32, 48), OTHER, True, True, None, False),
         ("channels", (1, 3, 16, 24), DEFAULT, False, True, None, False),
         ("odd", (1, 1, 37, 53), DEFAULT, False, True, None, False),
         ("seam", (2, 1, 40, 136), DEFAULT, False, True, None, False),
         ("halo", (1, 1, 5, 7), HALO, False, True, None, False),
         ("map_odd", (1, 1, 37, 53), DEFAULT, False, False, "odd", True),
         ("map_wide_dark", (1, 2, 18, 70), DARK, False, False, None, True))


def smooth(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.randn(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    x = 2.0 * smooth(n1)
    y = x + 0.1 * n2
    return x.half().float(), y.half().float()


def make_cot(shape, seed):
    g = torch.Generator().manual_seed(10000 + seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32).half().float()


def taps(sigma):
    """(R, g, g1, g2) as float64 arrays over t = -R..R."""
    R = int(3 * sigma + 0.5)
    t = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-t * t / (2 * sigma * sigma))
    g = g / g.sum()
    return R, g, -t / sigma ** 2 * g, (t * t / sigma ** 4 - 1 / sigma ** 2) * g


def conv_axis(u, k, axis):
    """The true convolution of u with the kernel k over t = -R..R along `axis` (-1 or -2), zero padding: out[i] = sum_t k[t] u[i - t]."""
    R = (len(k) - 1) // 2
    n = u.shape[axis]
    pad = (R, R, 0, 0) if axis == -1 else (0, 0, R, R)
    p = F.pad(u, pad)
    acc = 0
    for i, kv in enumerate(k):                       # t = i - R; the padded index of u[j - t] is j - t + R = j + 2 R - i
        s = 2 * R - i
        acc = acc + float(kv) * (p[..., s:s + n] if axis == -1 else p[..., s:s + n, :])
    return acc


def hessian(u, sigma, dtype):
    R, g, g1, g2 = taps(sigma)
    cast = lambda k: np.asarray(k, dtype=np.float64 if dtype == torch.float64 else np.float32)
    s2 = sigma * sigma
    a = s2 * conv_axis(conv_axis(u, cast(g2), -1), cast(g), -2)
    b = s2 * conv_axis(conv_axis(u, cast(g1), -1), cast(g1), -2)
    d = s2 * conv_axis(conv_axis(u, cast(g), -1), cast(g2), -2)
    return a, b, d


def measure(a, b, d, beta, c):
    """(V, r) of one scale."""
    m, h = (a + d) / 2, (a - d) / 2
    q = h * h + b * b
    pos = q > 0
    r = torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))
    kappa, mu = r - m, m + r
    ks = torch.where(kappa > 0, kappa, torch.ones_like(kappa))
    E1 = mu * mu / (2 * beta * beta * ks * ks)
    valid = (kappa > 0) & (E1 < E1_MAX)
    E1 = torch.where(valid, E1, torch.zeros_like(E1))
    E2 = (mu * mu + kappa * kappa) / (2 * c * c)
    return torch.where(valid, torch.exp(-E1) * -torch.expm1(-E2), torch.zeros_like(E1)), r


def response(x, cfg):
    """(Rsp, the smallest r over the scales of positive weight)."""
    lo, hi = cfg["value_range"]
    u = (x - lo) / (hi - lo)
    w = cfg["weights"] or (1.0,) * len(cfg["sigmas"])
    tot = sum(w)
    acc, rs = 0, []
    for sigma, wt in zip(cfg["sigmas"], w):
        if wt > 0:
            a, b, d = hessian(u, sigma, x.dtype)
            if not cfg["bright"]:
                a, b, d = -a, -b, -d
            V, r = measure(a, b, d, cfg["beta"], cfg["c"])
            acc = acc + (wt / tot) * V
            rs.append(float(r.detach().min()))
    return acc, min(rs)


def index(x, y, cfg):
    """(per-image scores (N,), min r, min D)."""
    A, ra = response(x, cfg)
    B, rb = response(y, cfg)
    D = (A * A).mean(dim=(1, 2, 3)) + (B * B).mean(dim=(1, 2, 3)) + cfg["eps"]
    S = (2 * (A * B).mean(dim=(1, 2, 3)) + cfg["eps"]) / D
    return S, min(ra, rb), float(D.detach().min())


def objective(x, y, cot, cfg, per_image, is_map):
    """(the differentiated scalar, what is stored as the result, min r, min D)."""
    if is_map:
        A, r = response(x, cfg)
        return (A * cot.to(x.dtype)).sum(), A, r, float("inf")
    rows, r, D = index(x, y, cfg)
    score = rows if per_image else rows.mean()
    return score.sum(), score, r, D


def run(x, y, cot, cfg, per_image, y_grad, is_map, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    y = y.to(dtype).clone().requires_grad_(y_grad)
    f, res, r, D = objective(x, y, cot, cfg, per_image, is_map)
    f.backward()
    return {"res": res.detach().numpy(), "dx": x.grad.numpy(), "dy": y.grad.numpy() if y_grad else None, "min_r": r, "min_D": D,
            "min_score": float("inf") if is_map else float(res.detach().min())}


def check_scipy(case, x, cfg):
    from scipy.ndimage import gaussian_filter
    lo, hi = cfg["value_range"]
    u = ((x.double() - lo) / (hi - lo))
    for sigma in cfg["sigmas"]:
        a, b, d = hessian(u, sigma, torch.float64)
        for got, order in ((a, (0, 2)), (b, (1, 1)), (d, (2, 0))):
            for n in range(u.shape[0]):
                for ch in range(u.shape[1]):
                    want = sigma * sigma * gaussian_filter(u[n, ch].numpy(), sigma, order=order, mode="constant", truncate=3.0)
                    assert np.abs(got[n, ch].numpy() - want).max() <= 1e-13, (case, sigma, order, np.abs(got[n, ch].numpy() - want).max())


def check_central_differences(case, x, y, cot, r64, cfg, per_image, y_grad, is_map, seed):
    rng = np.random.RandomState(seed)
    h = 1e-6
    value = lambda xx, yy: float(objective(xx, yy, cot, cfg, per_image, is_map)[0])
    for which, g in ((0, r64["dx"]), (1, r64["dy"])) if y_grad else ((0, r64["dx"]),):
        flat = np.abs(g).reshape(-1)
        for at in [int(flat.argmax())] + [int(v) for v in rng.randint(0, flat.size, 4)]:
            d = torch.zeros(x.numel(), dtype=torch.float64)
            d[at] = h
            d = d.reshape(x.shape)
            xd, yd = x.double(), y.double()
            with torch.no_grad():
                up = value(xd + d, yd) if which == 0 else value(xd, yd + d)
                dn = value(xd - d, yd) if which == 0 else value(xd, yd - d)
            num, ana = (up - dn) / (2 * h), float(g.reshape(-1)[at])
            # the value is a float64 of order 1 (a map case: of order sqrt(P)): 1e-15 of rounding over 2 h; the third-order term is h^2 |f'''|
            assert abs(num - ana) <= 1e-5 * abs(ana) + 2e-8, (case, "dxy"[1 + which], at, num, ana)


def qualifies(x, y, cfg, is_map):
    with torch.no_grad():
        if is_map:
            return response(x.double(), cfg)[1] >= MIN_R
        rows, r, D = index(x.double(), y.double(), cfg)
    return r >= MIN_R and D >= MIN_D and float(rows.min()) > 0


def find_seed(shape, users):
    for seed in range(2000):
        x, y = make_pair(shape, seed)
        if all(qualifies(x, y, cfg, is_map) for cfg, is_map in users):
            return seed, x, y
    raise SystemExit("no seed of range(2000) meets the conditioning caps for %s" % (shape,))


def trim(a64):
    """A float64 array rounded to 41 significant bits (the low 12 bits of every mantissa zero), which the file's compression then drops:
    half a unit of 2^-40 is 4.5e-13 relative at the worst and 2.3e-13 in the mean square, below the 1e-12 at which the restatement is
    compared with these arrays and seven orders below the float32 errors they measure."""
    bits = np.ascontiguousarray(a64).view(np.int64)
    return ((bits + 0x800) & ~np.int64(0xFFF)).view(np.float64)


def delta(a64, a32, what):
    """The float32 run's array as the distance of its bit pattern from that of the float64 array rounded to float32: small integers."""
    near = np.ascontiguousarray(a64.astype(np.float32))
    dl = np.ascontiguousarray(a32).view(np.int32) - near.view(np.int32)
    assert a32.dtype == np.float32 and np.array_equal((near.view(np.int32) + dl).view(np.float32), a32), what
    return dl


def main():
    out, inputs = {}, {}
    for case, shape, cfg, per_image, y_grad, shared, is_map in CASES:
        if shared is None:
            users = [(k[2], k[6]) for k in CASES if k[0] == case or k[5] == case]
            seed, x, y = find_seed(shape, users)
            inputs[case] = (seed, x, y)
            out[case + "/x"] = x.numpy().astype(np.float16)
            assert np.array_equal(out[case + "/x"].astype(np.float32), x.numpy())
            if not all(m for _, m in users):
                out[case + "/y"] = y.numpy().astype(np.float16)
                assert np.array_equal(out[case + "/y"].astype(np.float32), y.numpy())
        seed, x, y = inputs[shared or case]
        cot = make_cot(shape, seed) if is_map else None
        r64 = run(x, y, cot, cfg, per_image, y_grad, is_map, torch.float64)
        r32 = run(x, y, cot, cfg, per_image, y_grad, is_map, torch.float32)
        assert r64["min_r"] >= MIN_R and r64["min_D"] >= MIN_D and r64["min_score"] > 0, (case, r64["min_r"], r64["min_D"], r64["min_score"])
        check_scipy(case, x, cfg)
        check_central_differences(case, x, y, cot, r64, cfg, per_image, y_grad, is_map, seed)
        out[case + "/seed"], out[case + "/min_r"], out[case + "/min_D"] = np.int64(seed), np.float64(r64["min_r"]), np.float64(r64["min_D"])
        if is_map:
            out[case + "/cot"] = cot.numpy().astype(np.float16)
            assert np.array_equal(out[case + "/cot"].astype(np.float32), cot.numpy())
            out[case + "/map"] = trim(r64["res"])
            out[case + "/f32/map_delta"] = delta(out[case + "/map"], r32["res"], (case, "map"))
        else:
            out[case + "/score"], out[case + "/f32/score"] = r64["res"], r32["res"]
        for k in ("dx", "dy") if y_grad else ("dx",):
            if shared is not None and not is_map:    # the same float64 computation as the case it shares its inputs with: stored once
                assert np.array_equal(trim(r64[k]), out["%s/%s" % (shared, k)]), (case, k)
                assert np.array_equal(delta(trim(r64[k]), r32[k], (case, k)), out["%s/f32/%s_delta" % (shared, k)]), (case, k)
                continue
            out["%s/%s" % (case, k)] = trim(r64[k])
            out["%s/f32/%s_delta" % (case, k)] = delta(out["%s/%s" % (case, k)], r32[k], (case, k))
        e = np.abs(r32["res"].astype(np.float64) - r64["res"]).max() / np.abs(r64["res"]).max()
        print("%-14s seed %4d  min r %.2e  min D %.3f  result %s  fp32 result error %.1e  fp32 dx error %.1e" % (
            case, seed, r64["min_r"], r64["min_D"], "map" if is_map else np.array2string(r64["res"], precision=12), e,
            np.linalg.norm(r32["dx"].astype(np.float64) - r64["dx"]) / np.linalg.norm(r64["dx"])))
    path = os.path.join(ROOT, "tests", "golden", "golden_vessel.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; golden_gmsd.npz has", os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_gmsd.npz")))


if __name__ == "__main__":
    main()
