"""Write tests/golden/golden_cldice.npz: soft-clDice (Shit et al., CVPR 2021) of two images x, y of (N, C, H, W), channels independent grey
planes pooled inside an image:

    u = (x - lo) / (hi - lo), value_range = (lo, hi); bright = False uses (hi - x) / (hi - lo)
    E(I)[q] = min of I over the 5-point cross {q, up, down, left, right}, D(I)[q] = max of I over the 3 x 3 square around q, positions
      outside the image left out
    I_0 = u, I_{k+1} = E(I_k), O_k = D(I_{k+1}), delta_k = relu(I_k - O_k), k = 0..K, K = iters
    s_0 = delta_0, s_k = s_{k-1} + relu(delta_k - s_{k-1} delta_k), skel(u) = s_K
    Tprec = (sum skel(x) u_y + smooth) / (sum skel(x) + smooth), Tsens = (sum skel(y) u_x + smooth) / (sum skel(y) + smooth) per image n
    S[n] = 2 Tprec Tsens / (Tprec + Tsens), 0 where the denominator is 0

on the CPU, once in float64 and once in float32.  The float64 run takes every minimum and maximum over explicit shifted slices of the
plane padded with +inf or -inf (``torch.minimum`` / ``torch.maximum``: no pooling call, so that the values do not depend on the
``max_pool2d`` restatement of tests/test_cldice_cpu.py) and autograd differentiates those slices.  The float32 run is the torch
composition the kernels are measured against: ``max_pool2d`` as the definition's identities state it.  A case differentiates the mean
over n, or the sum of the per-image scores.

Checks made before anything is written, per case:
  * central differences in float64 on five entries of x and of y (the largest gradient entry and four random ones);
  * the conditioning caps of the float64 run: the gradient of the pair flipped on both axes, flipped back, equals the gradient to 1e-12
    in relative L2 (no tie between different pixels decides anything), and 1 - max skel >= 2^-6 (no mask of the recurrence on its edge).

Inputs: ``noise`` is uniform noise in [0, 1], ``smooth`` its 5 x 5 box blur (replicate-padded) rescaled to [0, 1]; the partner is
0.8 * that + 0.2 * other noise; both rounded to multiples of 2^-23, so that the image ``lo + u (hi - lo)`` (or ``hi - u (hi - lo)``) and the
map back to u are exact in float32 for the ranges used and a tie in float32 is a tie in float64.

Per case ``<case>/x``, ``<case>/y`` (float32; a case that names another's inputs stores none), ``<case>/score`` (0-d, or (N,)), ``dx``, ``dy``
(float64, rounded to 41 significant bits: ``trim``; none where a case shares its inputs with another, whose ``dx`` is the same
computation, asserted here), ``max_skel``, ``tie`` (the measured flip distance), and ``<case>/f32/score``, ``<case>/f32/dx_delta``, ``dy_delta``
(int32): the float32 run's array as the distance of its bit pattern from that of the float64 array rounded to float32.  Every 4-d
array is stored as its byte planes, uint8 of shape (itemsize,) + shape under ``<key>#<dtype>`` (``planes``), the packing of golden_vif.npz.

    python tools/gen_golden_cldice.py
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ITERS = 10
TIE_CAP, SKEL_CAP = 1e-12, 2.0 ** -6
GRID = 2.0 ** 23
SEED = 0
DEFAULT = dict(iters=3, smooth=1.0, value_range=(-1.0, 1.0), bright=True)
DARK = dict(iters=5, smooth=1.0, value_range=(0.0, 2.0), bright=False)
#: (case, shape, settings, per image, y needs a gradient, the kind of input, the case whose inputs it shares or None)
CASES = (("mean", (2, 1, 41, 53), DEFAULT, False, True, "smooth", None),
         ("xonly", (2, 1, 41, 53), DEFAULT, False, False, "smooth", "mean"),
         ("per_image_dark", (1, 2, 70, 140), DARK, True, True, "noise", None),
         ("limit", (1, 1, 96, 96), dict(DEFAULT, iters=MAX_ITERS), False, True, "smooth", None),
         ("small", (1, 1, 5, 7), DEFAULT, False, True, "noise", None),
         ("row", (1, 1, 1, 40), dict(DEFAULT, iters=1), False, True, "noise", None))


def box(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed, kind, cfg):
    """(x, y) as float32 images in the value range."""
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.rand(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    base = n1
    if kind == "smooth":
        b = box(n1)
        base = (b - b.min()) / (b.max() - b.min())
    lo, hi = cfg["value_range"]

    def image(u):
        u = torch.round(u.double() * GRID) / GRID
        v = lo + u * (hi - lo) if cfg["bright"] else hi - u * (hi - lo)
        assert torch.equal(v.float().double(), v)
        return v.float()
    return image(base), image(0.8 * base + 0.2 * n2)


def to_unit(x, cfg):
    lo, hi = cfg["value_range"]
    return (x - lo) / (hi - lo) if cfg["bright"] else (hi - x) / (hi - lo)


# ------------------------------------------------------------------------------------------------------------------------
# float64: explicit shifted slices
# ------------------------------------------------------------------------------------------------------------------------
def shifted(I, fill, offsets):
    H, W = I.shape[-2:]
    P = F.pad(I, (1, 1, 1, 1), value=fill)
    return [P[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in offsets]


def erode(I):
    up, left, centre, right, down = shifted(I, float("inf"), ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)))
    return torch.minimum(torch.minimum(torch.minimum(up, left), torch.minimum(centre, right)), down)


def dilate(I):
    s = shifted(I, -float("inf"), [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    out = s[0]
    for t in s[1:]:
        out = torch.maximum(out, t)
    return out


def skeleton(u, iters, erode=erode, dilate=dilate):
    I = u
    s = None
    for k in range(iters + 1):
        nxt = erode(I)
        delta = torch.relu(I - dilate(nxt))
        s = delta if s is None else s + torch.relu(delta - s * delta)
        I = nxt
    return s


def rows(x, y, cfg, erode=erode, dilate=dilate):
    """((N,) scores, the largest skeleton value)."""
    ux, uy = to_unit(x, cfg), to_unit(y, cfg)
    sx, sy = skeleton(ux, cfg["iters"], erode, dilate), skeleton(uy, cfg["iters"], erode, dilate)
    sm = cfg["smooth"]
    tprec = ((sx * uy).sum(dim=(1, 2, 3)) + sm) / (sx.sum(dim=(1, 2, 3)) + sm)
    tsens = ((sy * ux).sum(dim=(1, 2, 3)) + sm) / (sy.sum(dim=(1, 2, 3)) + sm)
    den = tprec + tsens
    S = torch.where(den != 0, 2 * tprec * tsens / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den))
    return S, max(float(sx.detach().max()), float(sy.detach().max()))


# ------------------------------------------------------------------------------------------------------------------------
# float32: the torch composition
# ------------------------------------------------------------------------------------------------------------------------
def pool_erode(I):
    return torch.min(-F.max_pool2d(-I, (3, 1), 1, (1, 0)), -F.max_pool2d(-I, (1, 3), 1, (0, 1)))


def pool_dilate(I):
    return F.max_pool2d(I, 3, 1, 1)


def objective(x, y, cfg, per_image, pooled=False):
    S, top = rows(x, y, cfg, *((pool_erode, pool_dilate) if pooled else ()))
    score = S if per_image else S.mean()
    return score.sum(), score, top


def run(x, y, cfg, per_image, y_grad, dtype, pooled=False):
    x = x.to(dtype).clone().requires_grad_(True)
    y = y.to(dtype).clone().requires_grad_(y_grad)
    f, res, top = objective(x, y, cfg, per_image, pooled)
    f.backward()
    return dict(max_skel=top, res=res.detach().numpy(), dx=x.grad.numpy(), dy=y.grad.numpy() if y_grad else None)


def flip_distance(x, y, cfg, per_image, y_grad, r64):
    """The conditioning cap on ties: the relative L2 distance of the flipped pair's gradient, flipped back, from the gradient."""
    f = run(torch.flip(x, (2, 3)), torch.flip(y, (2, 3)), cfg, per_image, y_grad, torch.float64)
    worst = 0.0
    for k in ("dx", "dy") if y_grad else ("dx",):
        back = np.flip(f[k], (2, 3))
        worst = max(worst, float(np.linalg.norm(back - r64[k]) / np.linalg.norm(r64[k])))
    return worst


def check_central_differences(case, x, y, r64, cfg, per_image, y_grad):
    rng = np.random.RandomState(SEED)
    h = 1e-7
    value = lambda xx, yy: float(objective(xx, yy, cfg, per_image)[0])
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
            # the value is a float64 of order 1: 1e-16 of rounding over 2 h = 1e-9; between two changes of an ordering the function is a
            # polynomial of low degree in one pixel, and the nearest other grid value is 2.4e-7 (a step of 2^-22 of the range 2) away
            assert abs(num - ana) <= 1e-4 * abs(ana) + 2e-9, (case, "dx" if which == 0 else "dy", at, num, ana)


def trim(a64):
    """A float64 array rounded to 41 significant bits (the low 12 bits of every mantissa zero), which the file's compression then drops:
    half a unit of 2^-40 is 4.5e-13 relative at the worst, below the 1e-12 at which the restatement is compared with these arrays."""
    bits = np.ascontiguousarray(a64).view(np.int64)
    return ((bits + 0x800) & ~np.int64(0xFFF)).view(np.float64)


def delta(a64, a32, what):
    """The float32 run's array as the distance of its bit pattern from that of the float64 array rounded to float32: small integers."""
    near = np.ascontiguousarray(a64.astype(np.float32))
    dl = np.ascontiguousarray(a32).view(np.int32) - near.view(np.int32)
    assert a32.dtype == np.float32 and np.array_equal((near.view(np.int32) + dl).view(np.float32), a32), what
    return dl


def planes(a):
    """An array as its bytes, one plane per byte of the item: uint8 of shape (itemsize,) + a.shape, little-endian; ``unplanes`` of
    tests/test_cldice_cpu.py is the inverse."""
    a = np.ascontiguousarray(a)
    return np.ascontiguousarray(np.moveaxis(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)), -1, 0))


def main():
    out, inputs = {}, {}
    for case, shape, cfg, per_image, y_grad, kind, shared in CASES:
        if shared is None:
            x, y = make_pair(shape, SEED, kind, cfg)
            inputs[case] = (x, y)
            out[case + "/x"], out[case + "/y"] = x.numpy(), y.numpy()
        x, y = inputs[shared or case]
        r64 = run(x, y, cfg, per_image, y_grad, torch.float64)
        r32 = run(x, y, cfg, per_image, y_grad, torch.float32, pooled=True)
        tie = flip_distance(x, y, cfg, per_image, y_grad, r64)
        assert tie <= TIE_CAP, (case, "tie", tie)
        assert 1 - r64["max_skel"] >= SKEL_CAP, (case, "max skel", r64["max_skel"])
        out[case + "/tie"], out[case + "/max_skel"] = np.float64(tie), np.float64(r64["max_skel"])
        check_central_differences(case, x, y, r64, cfg, per_image, y_grad)
        out[case + "/score"], out[case + "/f32/score"] = r64["res"], r32["res"]
        for k in ("dx", "dy") if y_grad else ("dx",):
            if shared is not None:                   # the same float64 computation as the case it shares its inputs with: stored once
                assert np.array_equal(trim(r64[k]), out["%s/%s" % (shared, k)]), (case, k)
                assert np.array_equal(delta(trim(r64[k]), r32[k], (case, k)), out["%s/f32/%s_delta" % (shared, k)]), (case, k)
                continue
            out["%s/%s" % (case, k)] = trim(r64[k])
            out["%s/f32/%s_delta" % (case, k)] = delta(out["%s/%s" % (case, k)], r32[k], (case, k))
        e = np.abs(r32["res"].astype(np.float64) - r64["res"]).max() / np.abs(r64["res"]).max()
        print("%-15s tie %.1e  1 - max skel %.3f  score %s  fp32 score error %.1e  fp32 dx error %.1e" % (
            case, tie, 1 - r64["max_skel"], np.array2string(r64["res"], precision=12), e,
            np.linalg.norm(r32["dx"].astype(np.float64) - r64["dx"]) / np.linalg.norm(r64["dx"])))
    for k in [k for k in out if out[k].ndim == 4]:
        a = out.pop(k)
        back = np.moveaxis(planes(a), 0, -1).copy().view(a.dtype).reshape(a.shape)
        assert np.array_equal(back.view(np.uint8), a.view(np.uint8)), k
        out["%s#%s" % (k, a.dtype.str)] = planes(a)
    path = os.path.join(ROOT, "tests", "golden", "golden_cldice.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_vif.npz"))


if __name__ == "__main__":
    main()
