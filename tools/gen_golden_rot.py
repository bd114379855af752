"""Write tests/golden/golden_rot_scat.npz and tests/golden/golden_rot_dtcwt.npz: the reference's rotationally symmetric
three-filter banks (near_sym_b_bp: 13, 19 and 19 taps; qshift_b_bp: 14 taps, m/2 odd) on the CPU, once in float64 and once in
float32.

Runs where the reference checkout exists only (oracle/ref_shim.py puts its modules on the path).

golden_rot_scat.npz -- the reference's own ``ScatLayer(biort='near_sym_b_bp')`` and ``ScatLayerj2(biort='near_sym_b_bp',
qshift='qshift_b_bp')`` on the cases of tools/gen_golden_scat.py (same shapes, modes, seeds and coding): per case ``x``, ``Z``,
the uint16-coded cotangent and ``x.grad``; per file the nine tap parameters the reference registers, in float64 (``buf_<name>``).

golden_rot_dtcwt.npz -- the reference's ``DTCWTForward`` cannot take these banks, so the transform is the composition of its four
functions: ``fwd_j1_rot`` then ``fwd_j2plus_rot`` twice (J = 3), and ``inv_j2plus_rot`` twice then ``inv_j1_rot`` on the synthesis
taps, level 1 in the modes 'symmetric' and 'zero', on (2,2,16,24) and (1,1,8,8) (no level needs a pad).  Per case: ``x``, ``yl``,
``yh0..2`` (N, C, 6, h, w, 2), the forward's ``x.grad`` for coded cotangents of all four outputs, the inverse of the float64
coefficients rounded to float32 (``inv``) and its gradients to ``yl`` and every ``yh``.  The forward's gradient is autograd through
the reference's functions; the inverse's is the reference's own rule (INV_J1.backward / INV_J2PLUS.backward with the ``_rot``
forwards: the matching forward on the synthesis taps, trees swapped at levels >= 2), because its c2q writes in place and autograd
cannot pass through it -- the float64 run asserts that the rule is the exact adjoint, <A c, dy> = <c, A* dy> to 1e-12.
Per file: the nine analysis and nine synthesis taps as the modules register them (prep_filt: reversed), ``buf_h*`` / ``buf_g*``.

Every array twice: ``<case>/<name>`` from the float64 run, ``<case>/f32/<name>`` from the float32 one.  Both files stay below 1 MiB.

    python tools/gen_golden_rot.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_shim                              # noqa: E402
from gen_golden_dtcwt import cot_codes, decode           # noqa: E402
from gen_golden_scat import cases, run                   # noqa: E402

BIORT, QSHIFT = "near_sym_b_bp", "qshift_b_bp"
SCAT_BUFS = ("h0o", "h1o", "h2o", "h0a", "h0b", "h1a", "h1b", "h2a", "h2b")
DT_MODES = ("symmetric", "zero")
DT_SHAPES = ((2, 2, 16, 24), (1, 1, 8, 8))
DT_J = 3


def dt_case_id(mode, shape):
    return "dt_%s_J%d_%dx%dx%dx%d" % ((mode, DT_J) + tuple(shape))


def save(name, out):
    path = os.path.join(ROOT, "tests", "golden", name)
    np.savez(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size >= 1 << 20:
        raise SystemExit("%s is %d bytes: a committed file stays below 1 MiB" % (path, size))


def scat_file():
    from pytorch_wavelets.scatternet import ScatLayer, ScatLayerj2
    out = {}
    for n, (cid, order, mode, shape, cc) in enumerate(cases(), 1):
        g = torch.Generator().manual_seed(9000 + shape[2] * 100 + shape[3])
        x = torch.randn(*shape, generator=g, dtype=torch.float32).double()
        out["x_%dx%dx%dx%d" % shape] = x.numpy()
        kw = dict(biort=BIORT, mode=mode, combine_colour=cc)
        if order == 2:
            kw["qshift"] = QSHIFT
        cls = ScatLayer if order == 1 else ScatLayerj2
        codes = cot_codes(run(cls, kw, x, None, torch.float64), n)
        out[cid + "/cot"] = codes
        out[cid + "/Z"], out[cid + "/xgrad"] = run(cls, kw, x, codes, torch.float64)
        out[cid + "/f32/Z"], out[cid + "/f32/xgrad"] = run(cls, kw, x, codes, torch.float32)
        print(cid, "Z", out[cid + "/Z"].shape)
    torch.set_default_dtype(torch.float64)
    layer = ScatLayerj2(biort=BIORT, qshift=QSHIFT)
    torch.set_default_dtype(torch.float32)
    assert list(layer.state_dict()) == list(SCAT_BUFS) and layer.bandpass_diag
    for name in SCAT_BUFS:
        out["buf_%s" % name] = getattr(layer, name).detach().numpy()
    save("golden_rot_scat.npz", out)


def dt_taps(dtype):
    """({name: prep_filt tensor} of the nine analysis taps, likewise the nine synthesis taps)."""
    from pytorch_wavelets.dtcwt.coeffs import biort, qshift
    from pytorch_wavelets.dtcwt.lowlevel import prep_filt
    h0o, g0o, h1o, g1o, h2o, g2o = biort(BIORT)
    h0a, h0b, g0a, g0b, h1a, h1b, g1a, g1b, h2a, h2b, g2a, g2b = qshift(QSHIFT)
    torch.set_default_dtype(dtype)
    try:
        h = {k: prep_filt(v, 1) for k, v in dict(h0o=h0o, h1o=h1o, h2o=h2o, h0a=h0a, h0b=h0b, h1a=h1a, h1b=h1b, h2a=h2a, h2b=h2b).items()}
        g = {k: prep_filt(v, 1) for k, v in dict(g0o=g0o, g1o=g1o, g2o=g2o, g0a=g0a, g0b=g0b, g1a=g1a, g1b=g1b, g2a=g2a, g2b=g2b).items()}
    finally:
        torch.set_default_dtype(torch.float32)
    return h, g


def dt_run(out, prefix, mode, x, cots, coeffs64, cot_inv, dtype):
    from pytorch_wavelets.dtcwt import transform_funcs as tf
    h, g = dt_taps(dtype)
    o_dim, ri_dim, h_dim, w_dim = tf.get_dimensions5(2, -1)
    x = x.to(dtype).clone().requires_grad_(True)
    low, hr, hi = tf.fwd_j1_rot(x, h["h0o"], h["h1o"], h["h2o"], False, o_dim, mode)
    yh = [torch.stack((hr, hi), dim=ri_dim)]
    for _ in range(1, DT_J):
        low, hr, hi = tf.fwd_j2plus_rot(low, h["h0a"], h["h1a"], h["h0b"], h["h1b"], h["h2a"], h["h2b"], False, o_dim, "symmetric")
        yh.append(torch.stack((hr, hi), dim=ri_dim))
    out[prefix + "yl"] = low.detach().numpy()
    for j, b in enumerate(yh):
        out[prefix + "yh%d" % j] = b.detach().numpy()
    torch.autograd.backward([low] + yh, [decode(c, dtype) for c in cots(low, yh)])
    out[prefix + "xgrad"] = x.grad.numpy()
    if coeffs64 is None:                    # the inverse's input: the float64 coefficients rounded to float32, in both runs
        coeffs64 = (low.detach().float(), [b.detach().float() for b in yh])
    cl, ch = coeffs64[0].to(dtype), [b.to(dtype) for b in coeffs64[1]]
    with torch.no_grad():
        y = cl
        for b in ch[:0:-1]:
            br, bi = torch.unbind(b, dim=ri_dim)
            y = tf.inv_j2plus_rot(y, br, bi, g["g0a"], g["g1a"], g["g0b"], g["g1b"], g["g2a"], g["g2b"], o_dim, h_dim, w_dim, "symmetric")
        br, bi = torch.unbind(ch[0], dim=ri_dim)
        y = tf.inv_j1_rot(y, br, bi, g["g0o"], g["g1o"], g["g2o"], o_dim, h_dim, w_dim, mode)
        out[prefix + "inv"] = y.numpy()
        # the inverse's gradients by the reference's own rule (INV_J1.backward, INV_J2PLUS.backward): the matching forward on the
        # synthesis taps, trees a and b swapped at levels >= 2
        dy = decode(cot_inv(y), dtype)
        dl, dr, di = tf.fwd_j1_rot(dy, g["g0o"], g["g1o"], g["g2o"], False, o_dim, mode)
        grads = [torch.stack((dr, di), dim=ri_dim)]
        for _ in range(1, DT_J):
            dl, dr, di = tf.fwd_j2plus_rot(dl, g["g0b"], g["g1b"], g["g0a"], g["g1a"], g["g2b"], g["g2a"], False, o_dim, "symmetric")
            grads.append(torch.stack((dr, di), dim=ri_dim))
        if dtype == torch.float64:          # <A c, dy> == <c, A* dy>: the rule is the exact adjoint
            lhs, rhs = (y * dy).sum(), (cl * dl).sum() + sum((b * gb).sum() for b, gb in zip(ch, grads))
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (float(lhs), float(rhs))
    out[prefix + "inv_gyl"] = dl.numpy()
    for j, gb in enumerate(grads):
        out[prefix + "inv_gyh%d" % j] = gb.numpy()
    return coeffs64


def dtcwt_file():
    out, n = {}, 0
    for mode in DT_MODES:
        for shape in DT_SHAPES:
            n += 1
            cid = dt_case_id(mode, shape)
            g = torch.Generator().manual_seed(8000 + shape[2] * 100 + shape[3])
            x = torch.randn(*shape, generator=g, dtype=torch.float32).double()     # float32 values: both runs read the same input
            out["x_%dx%dx%dx%d" % shape] = x.numpy()

            def cots(yl, yh, n=n, cid=cid):
                c = [cot_codes(tuple(yl.shape), n)] + [cot_codes(tuple(b.shape), n + 100 * (j + 1)) for j, b in enumerate(yh)]
                out[cid + "/cot_yl"] = c[0]
                for j in range(len(yh)):
                    out[cid + "/cot_yh%d" % j] = c[j + 1]
                return c

            def cot_inv(y, n=n, cid=cid):
                out[cid + "/cot_inv"] = cot_codes(tuple(y.shape), n + 5000)
                return out[cid + "/cot_inv"]

            coeffs = dt_run(out, cid + "/", mode, x, cots, None, cot_inv, torch.float64)
            dt_run(out, cid + "/f32/", mode, x, cots, coeffs, cot_inv, torch.float32)
            print(cid, "yl", out[cid + "/yl"].shape, "inv", out[cid + "/inv"].shape)
    h, g = dt_taps(torch.float64)
    for name, t in list(h.items()) + list(g.items()):
        out["buf_%s" % name] = t.numpy()
    save("golden_rot_dtcwt.npz", out)


def main():
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not on this machine")
    ref_shim.load()
    if torch.cuda.is_available():
        raise SystemExit("the fixtures are the reference's CPU results: run this on a machine without a GPU")
    scat_file()
    dtcwt_file()


if __name__ == "__main__":
    main()
