"""Write tests/golden/golden_vif.npz: the visual information fidelity in the pixel domain (VIFp; Sheikh & Bovik 2006) of an image under
test x against a reference r, both (N, C, H, W), channels independent grey planes pooled inside an image:

    u = (t - lo) * 255 / (hi - lo), value_range = (lo, hi); EPS = 1e-8
    scale s = 0..3: K_s = 2^(4-s) + 1, w_s[k] = exp(-(k - (K_s-1)/2)^2 / (2 (K_s/5)^2)) / sum, W_s * t the separable VALID convolution
      s > 0: x_s = (W_s * x_{s-1})[::2, ::2], r_s likewise
      mx = W_s*x_s, mr = W_s*r_s, sxx = relu(W_s*(x_s x_s) - mx^2), srr = relu(W_s*(r_s r_s) - mr^2), sxr = W_s*(x_s r_s) - mx mr
      g = sxr / (srr + EPS), sv = sxx - g sxr, then in this order
        srr < EPS: g = 0, sv = sxx, srr = 0;   sxx < EPS: g = 0, sv = 0;   g < 0: sv = sxx, g = 0;   sv <= EPS: sv = EPS
      num_s[n] = sum log10(1 + g^2 srr / (sv + sigma_n_sq)), den_s[n] = sum log10(1 + srr / sigma_n_sq)
    V[n] = (sum_s num_s + EPS) / (sum_s den_s + EPS)

on the CPU, once in float64 and once in float32.  The convolutions are explicit sums of shifted slices -- no convolution call, so that
the values do not depend on the ``F.conv2d`` restatement of tests/test_vif_cpu.py -- written with torch slices, so that autograd
differentiates the same code: a ``where`` passes the gradient of the branch it took, relu'(0) = 0.  A case differentiates the mean
over n, or the sum of the per-image scores.

Checks made before anything is written, per case:
  * central differences in float64 on five entries of x and of r (the largest gradient entry and four random ones);
  * the conditioning caps of the float64 run over all scales and positions: min sxx >= 1, min srr >= 1, min g >= 0.5, min sv >= 2^-8,
    so that no clamp is anywhere near.

Inputs, as in the family: r = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, x = r + 0.1 noise, seed 0, rounded to values
that float16 holds exactly; they enter every computation as float32.

Per case ``<case>/x``, ``<case>/r`` (float16, exact; a case that names another's inputs stores none), ``<case>/score`` (0-d, or (N,)),
``dx``, ``dr`` (float64, rounded to 41 significant bits: ``trim``; none where a case shares its inputs with another, whose ``dx`` is the
same computation, asserted here), ``min_sxx``, ``min_srr``, ``min_g``, ``min_sv``, and ``<case>/f32/score``, ``<case>/f32/dx_delta``,
``dr_delta`` (int32): the float32 run's array as the distance of its bit pattern (as int32) from that of the float64 array rounded to
float32; ``(float32(dx).view(int32) + dx_delta).view(float32)`` is the float32 run's gradient bit for bit (asserted here).  Every
4-d array is stored as its byte planes, uint8 of shape (itemsize,) + shape under ``<key>#<dtype>`` (``planes``): 95,528 float64 gradient
entries at 41 bits do not fit 1 MiB next to the inputs otherwise.

    python tools/gen_golden_vif.py
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-8
CAPS = dict(min_sxx=1.0, min_srr=1.0, min_g=0.5, min_sv=2.0 ** -8)
DEFAULT = dict(sigma_n_sq=2.0, value_range=(-1.0, 1.0))
OTHER = dict(sigma_n_sq=0.4, value_range=(0.0, 2.0))
SEED = 0
#: (case, shape, settings, per image, r needs a gradient, the case whose inputs it shares or None)
CASES = (("min41", (1, 1, 41, 41), DEFAULT, False, True, None),
         ("mean", (2, 1, 48, 56), DEFAULT, False, True, None),
         ("xonly", (2, 1, 48, 56), DEFAULT, False, False, "mean"),
         ("per_image_cfg", (2, 2, 48, 72), OTHER, True, True, None),
         ("channels", (1, 3, 57, 73), DEFAULT, False, True, None),
         ("seam", (1, 1, 72, 200), DEFAULT, False, True, None))


def smooth(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed):
    """(x, r): the image under test and the reference."""
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.randn(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    r = 2.0 * smooth(n1)
    x = r + 0.1 * n2
    return x.half().float(), r.half().float()


def window(s):
    K = 2 ** (4 - s) + 1
    v = [math.exp(-((k - (K - 1) / 2.0) ** 2) / (2.0 * (K / 5.0) ** 2)) for k in range(K)]
    total = math.fsum(v)
    return [t / total for t in v]


def valid_axis(u, w, axis):
    """The valid correlation of u with the (even) window w along `axis` (-1 or -2): out[i] = sum_k w[k] u[i + k]."""
    n = u.shape[axis] - len(w) + 1
    acc = 0
    for k, wk in enumerate(w):
        acc = acc + wk * (u[..., k:k + n] if axis == -1 else u[..., k:k + n, :])
    return acc


def filt(u, w):
    return valid_axis(valid_axis(u, w, -1), w, -2)


def vif_rows(x, r, cfg):
    """((N,) scores, the minima the caps speak of)."""
    lo, hi = cfg["value_range"]
    sn = cfg["sigma_n_sq"]
    x, r = (x - lo) * 255.0 / (hi - lo), (r - lo) * 255.0 / (hi - lo)
    num = den = 0
    mins = dict(min_sxx=float("inf"), min_srr=float("inf"), min_g=float("inf"), min_sv=float("inf"))
    for s in range(4):
        w = window(s)
        if s > 0:
            x, r = filt(x, w)[..., ::2, ::2], filt(r, w)[..., ::2, ::2]
        mx, mr = filt(x, w), filt(r, w)
        sxx = torch.relu(filt(x * x, w) - mx * mx)
        srr = torch.relu(filt(r * r, w) - mr * mr)
        sxr = filt(x * r, w) - mx * mr
        g = sxr / (srr + EPS)
        sv = sxx - g * sxr
        for k, v in (("min_sxx", sxx), ("min_srr", srr), ("min_g", g), ("min_sv", sv)):
            mins[k] = min(mins[k], float(v.detach().min()))
        zero = torch.zeros_like(g)
        m = srr < EPS
        g, sv, srr = torch.where(m, zero, g), torch.where(m, sxx, sv), torch.where(m, zero, srr)
        m = sxx < EPS
        g, sv = torch.where(m, zero, g), torch.where(m, zero, sv)
        m = g < 0
        sv, g = torch.where(m, sxx, sv), torch.where(m, zero, g)
        sv = torch.where(sv <= EPS, torch.full_like(sv, EPS), sv)
        num = num + torch.log10(1 + g * g * srr / (sv + sn)).sum(dim=(1, 2, 3))
        den = den + torch.log10(1 + srr / sn).sum(dim=(1, 2, 3))
    return (num + EPS) / (den + EPS), mins


def objective(x, r, cfg, per_image):
    rows, mins = vif_rows(x, r, cfg)
    score = rows if per_image else rows.mean()
    return score.sum(), score, mins


def run(x, r, cfg, per_image, r_grad, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    r = r.to(dtype).clone().requires_grad_(r_grad)
    f, res, mins = objective(x, r, cfg, per_image)
    f.backward()
    return dict(mins, res=res.detach().numpy(), dx=x.grad.numpy(), dr=r.grad.numpy() if r_grad else None)


def check_central_differences(case, x, r, r64, cfg, per_image, r_grad):
    rng = np.random.RandomState(SEED)
    h = 1e-6
    value = lambda xx, rr: float(objective(xx, rr, cfg, per_image)[0])
    for which, g in ((0, r64["dx"]), (1, r64["dr"])) if r_grad else ((0, r64["dx"]),):
        flat = np.abs(g).reshape(-1)
        for at in [int(flat.argmax())] + [int(v) for v in rng.randint(0, flat.size, 4)]:
            d = torch.zeros(x.numel(), dtype=torch.float64)
            d[at] = h
            d = d.reshape(x.shape)
            xd, rd = x.double(), r.double()
            with torch.no_grad():
                up = value(xd + d, rd) if which == 0 else value(xd, rd + d)
                dn = value(xd - d, rd) if which == 0 else value(xd, rd - d)
            num, ana = (up - dn) / (2 * h), float(g.reshape(-1)[at])
            # the value is a float64 of order 1: 1e-16 of rounding over 2 h; the third-order term is h^2 |f'''|
            assert abs(num - ana) <= 1e-5 * abs(ana) + 1e-9, (case, "dx" if which == 0 else "dr", at, num, ana)


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


def planes(a):
    """An array as its bytes, one plane per byte of the item: uint8 of shape (itemsize,) + a.shape, little-endian.  The planes of the
    sign and exponent and of the trimmed bits are nearly constant, which the file's compression sees only when they lie together;
    ``unplanes`` of tests/test_vif_cpu.py is the inverse."""
    a = np.ascontiguousarray(a)
    return np.ascontiguousarray(np.moveaxis(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)), -1, 0))


def main():
    out, inputs = {}, {}
    for case, shape, cfg, per_image, r_grad, shared in CASES:
        if shared is None:
            x, r = make_pair(shape, SEED)
            inputs[case] = (x, r)
            for k, t in (("x", x), ("r", r)):
                out["%s/%s" % (case, k)] = t.numpy().astype(np.float16)
                assert np.array_equal(out["%s/%s" % (case, k)].astype(np.float32), t.numpy())
        x, r = inputs[shared or case]
        r64 = run(x, r, cfg, per_image, r_grad, torch.float64)
        r32 = run(x, r, cfg, per_image, r_grad, torch.float32)
        for k, cap in CAPS.items():
            assert r64[k] >= cap, (case, k, r64[k], cap)
            out["%s/%s" % (case, k)] = np.float64(r64[k])
        check_central_differences(case, x, r, r64, cfg, per_image, r_grad)
        out[case + "/score"], out[case + "/f32/score"] = r64["res"], r32["res"]
        for k in ("dx", "dr") if r_grad else ("dx",):
            if shared is not None:                   # the same float64 computation as the case it shares its inputs with: stored once
                assert np.array_equal(trim(r64[k]), out["%s/%s" % (shared, k)]), (case, k)
                assert np.array_equal(delta(trim(r64[k]), r32[k], (case, k)), out["%s/f32/%s_delta" % (shared, k)]), (case, k)
                continue
            out["%s/%s" % (case, k)] = trim(r64[k])
            out["%s/f32/%s_delta" % (case, k)] = delta(out["%s/%s" % (case, k)], r32[k], (case, k))
        e = np.abs(r32["res"].astype(np.float64) - r64["res"]).max() / np.abs(r64["res"]).max()
        print("%-14s sxx >= %.1f srr >= %.1f g >= %.3f sv >= %.4f  score %s  fp32 score error %.1e  fp32 dx error %.1e" % (
            case, r64["min_sxx"], r64["min_srr"], r64["min_g"], r64["min_sv"], np.array2string(r64["res"], precision=12), e,
            np.linalg.norm(r32["dx"].astype(np.float64) - r64["dx"]) / np.linalg.norm(r64["dx"])))
    # every array of more than one item goes in as byte planes under "<key>#<dtype>"
    for k in [k for k in out if out[k].ndim == 4]:
        a = out.pop(k)
        back = np.moveaxis(planes(a), 0, -1).copy().view(a.dtype).reshape(a.shape)
        assert np.array_equal(back.view(np.uint8), a.view(np.uint8)), k
        out["%s#%s" % (k, a.dtype.str)] = planes(a)
    path = os.path.join(ROOT, "tests", "golden", "golden_vif.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
