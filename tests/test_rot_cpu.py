"""The rotationally symmetric three-filter DTCWT banks (near_sym_b_bp / qshift_b_bp) without a GPU: a plain-torch float64
restatement of the four three-filter levels (transform_funcs.py fwd_j1_rot, fwd_j2plus_rot, inv_j1_rot, inv_j2plus_rot) and of
the two scattering layers over them (scatternet/lowlevel.py ScatLayerj1_rot_f, ScatLayerj2_rot_f), pinned to the reference's own
results in tests/golden/golden_rot_scat.npz and golden_rot_dtcwt.npz (tools/gen_golden_rot.py), and the host logic of the
3-tuple / 6-tuple tap forms.  The restatement is built on the helpers of test_dtcwt_cpu.py and test_scat_cpu.py; the GPU test
(test_gpu_rot.py) imports it from here."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch.autograd import Function

from test_dtcwt_cpu import decode, dfilt, from_orientations, ifilt, rel_l2, same_filter, to_orientations
from test_scat_cpu import J1_MODES, J1_SHAPES, J2_SHAPES, MAGBIAS, pool, smooth_mag, unpool

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCAT_BUFS = ("h0o", "h1o", "h2o", "h0a", "h0b", "h1a", "h1b", "h2a", "h2b")             # the reference's state-dict order
FWD_BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b", "h2o", "h2a", "h2b")              # the third filters after the existing six
INV_BUFS = ("g0o", "g1o", "g0a", "g0b", "g1a", "g1b", "g2o", "g2a", "g2b")
DT_MODES = ("symmetric", "zero")
DT_SHAPES = ((2, 2, 16, 24), (1, 1, 8, 8))
DT_J = 3
# position of the third filter in the entry points' arguments: (pointer, length) at level 1, the pair (a2, b2) at levels >= 2
THIRD_ARG = {"dtcwt_fwd_j1": 21, "dtcwt_fwd_j2": 21, "dtcwt_inv_j1": 20, "dtcwt_inv_j2": 20,
             "scat_fwd_j1": 24, "scat_fwd_j2": 23, "scat_bwd_j1": 18, "scat_bwd_j2": 17}
_gold = {}


def third_filter(name, args):
    """Whether a recorded call of entry ``name`` passes a third filter; a half-given one is an error."""
    p, q = args[THIRD_ARG[name]:THIRD_ARG[name] + 2]
    if name.endswith("j1"):
        assert (bool(p) and q >= 3) or (p is None and q == 0), (name, p, q)
    else:
        assert bool(p) == bool(q) and (p is None) == (q is None), (name, p, q)
    return bool(p)


def gold(which):
    """The arrays of golden_rot_<which>.npz, ``which`` 'scat' or 'dtcwt' (read once; do not modify them)."""
    if which not in _gold:
        with np.load(os.path.join(GOLDEN, "golden_rot_%s.npz" % which)) as z:
            _gold[which] = {k: z[k] for k in z.files}
    return _gold[which]


def bufs(dtype=torch.float64):
    """The eighteen registered taps of the fixture bank as flat tensors (taps reversed, as prep_filt stores them)."""
    g = gold("dtcwt")
    return {n: torch.from_numpy(g["buf_" + n]).reshape(-1).to(dtype) for n in FWD_BUFS + INV_BUFS}


def synthetic_bufs(dtype=torch.float64):
    """A seeded bank for what the only real one cannot exercise: a level-1 third filter of 3 taps, shorter than both others (its
    own centring offset), and q-shift filters of 16 taps (m/2 even: the other branch of the interpolation table), all six.  The
    taps have no symmetry, so a swapped tree or a reversed filter shows; the backward passes stay the reference's rule (the
    matching level on the same taps), which for such taps is a fixed linear map but not the adjoint."""
    g = torch.Generator().manual_seed(77)
    lens = dict(h0o=7, h1o=5, h2o=3, g0o=5, g1o=7, g2o=3)
    b = {n: torch.randn(L, generator=g, dtype=torch.float64) * 0.4 for n, L in lens.items()}
    for n in ("h0a", "h0b", "h1a", "h1b", "h2a", "h2b", "g0a", "g0b", "g1a", "g1b", "g2a", "g2b"):
        b[n] = torch.randn(16, generator=g, dtype=torch.float64) * 0.3
    return {n: v.float().to(dtype) for n, v in b.items()}                                # float32 values: every run reads the same taps


def tuples(b, analysis=True):
    """(biort 3-tuple, qshift 6-tuple) in the order the constructors take them (taps un-reversed)."""
    p = "h" if analysis else "g"
    w = {k: v.flip(0).tolist() for k, v in b.items()}
    return tuple(w[p + s] for s in ("0o", "1o", "2o")), tuple(w[p + s] for s in ("0a", "0b", "1a", "1b", "2a", "2b"))


def scat_cases():
    """(case id, order, mode, shape, combine_colour) of golden_rot_scat.npz"""
    out = [("j1_%s_%dx%dx%dx%d%s" % ((m,) + s + ("_cc" if cc else "",)), 1, m, s, cc) for m in J1_MODES for s, cc in J1_SHAPES]
    return out + [("j2_symmetric_%dx%dx%dx%d%s" % (s + ("_cc" if cc else "",)), 2, "symmetric", s, cc) for s, cc in J2_SHAPES]


def dt_cases():
    """(case id, mode, shape) of golden_rot_dtcwt.npz"""
    return [("dt_%s_J%d_%dx%dx%dx%d" % ((m, DT_J) + s), m, s) for m in DT_MODES for s in DT_SHAPES]


# ------------------------------------------------------------------------------------------------------------------------
# the restatement: the four three-filter levels
# ------------------------------------------------------------------------------------------------------------------------
def fwd_j1_rot(x, h0, h1, h2, sym):
    lo, hi, ba = same_filter(x, h0, 3, sym), same_filter(x, h1, 3, sym), same_filter(x, h2, 3, sym)
    return same_filter(lo, h0, 2, sym), to_orientations(same_filter(lo, h1, 2, sym), same_filter(hi, h0, 2, sym), same_filter(ba, h2, 2, sym))


def inv_j1_rot(ll, h, g0, g1, g2, sym):
    """ll or h may be None (zeros)."""
    lo = hi = ba = None
    if h is not None:
        lh, hl, hh = from_orientations(h)
        lo, hi, ba = same_filter(lh, g1, 2, sym), same_filter(hl, g0, 2, sym), same_filter(hh, g2, 2, sym)
    if ll is not None:
        t = same_filter(ll, g0, 2, sym)
        lo = t if lo is None else lo + t
    y = same_filter(lo, g0, 3, sym)
    return y if hi is None else same_filter(hi, g1, 3, sym) + y + same_filter(ba, g2, 3, sym)


def fwd_j2_rot(x, h0a, h0b, h1a, h1b, h2a, h2b):
    lo, hi, ba = dfilt(x, h0b, h0a, 3, False), dfilt(x, h1b, h1a, 3, True), dfilt(x, h2b, h2a, 3, True)
    return dfilt(lo, h0b, h0a, 2, False), to_orientations(dfilt(lo, h1b, h1a, 2, True), dfilt(hi, h0b, h0a, 2, False),
                                                          dfilt(ba, h2b, h2a, 2, True))


def inv_j2_rot(ll, h, g0a, g0b, g1a, g1b, g2a, g2b):
    lo = hi = ba = None
    if h is not None:
        lh, hl, hh = from_orientations(h)
        lo, hi, ba = ifilt(lh, g1b, g1a, 2, True), ifilt(hl, g0b, g0a, 2, False), ifilt(hh, g2b, g2a, 2, True)
    if ll is not None:
        t = ifilt(ll, g0b, g0a, 2, False)
        lo = t if lo is None else lo + t
    y = ifilt(lo, g0b, g0a, 3, False)
    return y if hi is None else ifilt(hi, g1b, g1a, 3, True) + y + ifilt(ba, g2b, g2a, 3, True)


def _q(b, p="h", swap=False):
    a, c = ("b", "a") if swap else ("a", "b")
    return tuple(b[p + s] for s in ("0" + a, "0" + c, "1" + a, "1" + c, "2" + a, "2" + c))


class RFwd1(Function):
    """Level 1 with the reference's backward: the inverse on the same taps."""

    @staticmethod
    def forward(ctx, x, h0, h1, h2, sym):
        ctx.cfg = (h0, h1, h2, sym)
        return fwd_j1_rot(x, h0, h1, h2, sym)

    @staticmethod
    def backward(ctx, dl, dh):
        return (inv_j1_rot(dl, dh, *ctx.cfg),) + (None,) * 4


class RFwd2(Function):
    """A level >= 2; the backward is the inverse on the trees swapped, the third pair included."""

    @staticmethod
    def forward(ctx, x, *q):
        ctx.q = q
        return fwd_j2_rot(x, *q)

    @staticmethod
    def backward(ctx, dl, dh):
        q = ctx.q
        return (inv_j2_rot(dl, dh, q[1], q[0], q[3], q[2], q[5], q[4]),) + (None,) * 6


class RInv1(Function):
    @staticmethod
    def forward(ctx, ll, h, g0, g1, g2, sym):
        ctx.cfg = (g0, g1, g2, sym)
        return inv_j1_rot(ll, h, g0, g1, g2, sym)

    @staticmethod
    def backward(ctx, dy):
        return fwd_j1_rot(dy, *ctx.cfg) + (None,) * 4


class RInv2(Function):
    @staticmethod
    def forward(ctx, ll, h, *q):
        ctx.q = q
        return inv_j2_rot(ll, h, *q)

    @staticmethod
    def backward(ctx, dy):
        q = ctx.q
        return fwd_j2_rot(dy, q[1], q[0], q[3], q[2], q[5], q[4]) + (None,) * 6


def forward_levels(x, b, mode, J):
    """``DTCWTForward``: (yl, [yh_0 .. yh_{J-1}]); a lowpass side that is no multiple of 4 repeats its first and last row / column."""
    low, h = RFwd1.apply(x, b["h0o"], b["h1o"], b["h2o"], mode == "symmetric")
    yh = [h]
    for _ in range(1, J):
        if low.shape[2] % 4:
            low = torch.cat((low[:, :, :1], low, low[:, :, -1:]), 2)
        if low.shape[3] % 4:
            low = torch.cat((low[:, :, :, :1], low, low[:, :, :, -1:]), 3)
        low, h = RFwd2.apply(low, *_q(b))
        yh.append(h)
    return low, yh


def _fit(low, h):
    if low.shape[2] != 2 * h.shape[3]:
        low = low[:, :, 1:-1]
    if low.shape[3] != 2 * h.shape[4]:
        low = low[:, :, :, 1:-1]
    return low


def inverse_levels(yl, yh, b, mode):
    """``DTCWTInverse``: a lowpass that is not twice its level's bandpass loses its first and last row / column."""
    for h in yh[:0:-1]:
        yl = RInv2.apply(_fit(yl, h), h, *_q(b, "g"))
    return RInv1.apply(_fit(yl, yh[0]), yh[0], b["g0o"], b["g1o"], b["g2o"], mode == "symmetric")


def restate_dt(x, b, mode, J, cots, coeffs, cot_inv, dtype):
    """The arrays of one golden_rot_dtcwt.npz case from the restatement in ``dtype``; ``coeffs``: the inverse's float32-valued
    input (yl, yh), None to take it from this run."""
    b = {k: v.to(dtype) for k, v in b.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    yl, yh = forward_levels(x, b, mode, J)
    out = {"yl": yl.detach()}
    out.update({"yh%d" % j: h.detach() for j, h in enumerate(yh)})
    torch.autograd.backward([yl] + yh, [c.to(dtype) for c in cots])
    out["xgrad"] = x.grad
    if coeffs is None:
        coeffs = (yl.detach().float(), [h.detach().float() for h in yh])
    cl = coeffs[0].to(dtype).clone().requires_grad_(True)
    ch = [h.to(dtype).clone().requires_grad_(True) for h in coeffs[1]]
    y = inverse_levels(cl, ch, b, mode)
    out["inv"] = y.detach()
    y.backward(cot_inv.to(dtype))
    out["inv_gyl"] = cl.grad
    out.update({"inv_gyh%d" % j: h.grad for j, h in enumerate(ch)})
    return out, coeffs


# ------------------------------------------------------------------------------------------------------------------------
# the restatement: the two layers
# ------------------------------------------------------------------------------------------------------------------------
class RScat1(Function):
    """ScatLayerj1_rot_f on an even-sided x: Z (N, 7, C, h, w), or (N, 9, h, w) for the colour form."""

    @staticmethod
    def forward(ctx, x, b, sym, bias, colour):
        ll, h = fwd_j1_rot(x, b["h0o"], b["h1o"], b["h2o"], sym)
        mag, phase = smooth_mag(h, bias, colour)
        ctx.cfg = (b, sym, colour)
        ctx.save_for_backward(phase)
        if colour:
            return torch.cat((pool(ll), mag[:, 0]), 1)
        return torch.cat((pool(ll)[:, None], mag.transpose(1, 2)), 1)

    @staticmethod
    def backward(ctx, dZ):
        b, sym, colour = ctx.cfg
        phase, = ctx.saved_tensors
        dlow, dmag = (dZ[:, :3], dZ[:, 3:][:, None]) if colour else (dZ[:, 0], dZ[:, 1:].transpose(1, 2))
        return inv_j1_rot(unpool(dlow), dmag.unsqueeze(-1) * phase, b["h0o"], b["h1o"], b["h2o"], sym), None, None, None, None


class RScat2(Function):
    """ScatLayerj2_rot_f on an x whose sides are multiples of 8: Z (N, 49, C, h, w) or (N, 51, h, w)."""

    @staticmethod
    def forward(ctx, x, b, bias, colour):
        N, C = x.shape[:2]
        o = (b["h0o"], b["h1o"], b["h2o"])
        s0, h = fwd_j1_rot(x, *o, True)
        m1, p1 = smooth_mag(h, bias, colour)                                     # (N, C1, 6, h2, w2)
        C1 = m1.shape[1]
        ll2, h = fwd_j2_rot(s0, *_q(b))
        m2, p2 = smooth_mag(h, bias, colour)                                     # (N, C1, 6, h4, w4)
        u = m1.transpose(1, 2).reshape(N, 6 * C1, m1.shape[3], m1.shape[4])      # channel o1 C1 + c
        l1, h = fwd_j1_rot(u, *o, True)
        m21, p21 = smooth_mag(h, bias, False)                                    # (N, 6 C1, 6 (o2), h4, w4)
        hw = m21.shape[3:]
        s2 = m21.reshape((N, 6, C1, 6) + hw).permute(0, 3, 1, 2, 4, 5).reshape((N, 36, C1) + hw)      # index 6 o2 + o1
        ctx.cfg = (b, colour, C1)
        ctx.save_for_backward(p1, p2, p21)
        if colour:
            return torch.cat((pool(ll2), pool(l1), m2[:, 0], s2[:, :, 0]), 1)
        return torch.cat((pool(ll2)[:, None], pool(l1).reshape((N, 6, C) + hw), m2.transpose(1, 2), s2), 1)

    @staticmethod
    def backward(ctx, dZ):
        b, colour, C1 = ctx.cfg
        p1, p2, p21 = ctx.saved_tensors
        o = (b["h0o"], b["h1o"], b["h2o"])
        N, hw = dZ.shape[0], tuple(dZ.shape[-2:])
        if colour:
            d_s0, d_s1, d_m2, d_s2 = dZ[:, :3], dZ[:, 3:9], dZ[:, 9:15][:, None], dZ[:, 15:][:, :, None]
        else:
            d_s0, d_s1, d_m2, d_s2 = dZ[:, 0], dZ[:, 1:7].reshape((N, 6 * C1) + hw), dZ[:, 7:13].transpose(1, 2), dZ[:, 13:]
        d_m21 = d_s2.reshape((N, 6, 6, C1) + hw).permute(0, 2, 3, 1, 4, 5).reshape((N, 6 * C1, 6) + hw)
        du = inv_j1_rot(unpool(d_s1), d_m21.unsqueeze(-1) * p21, *o, True)
        d_m1 = du.reshape((N, 6, C1) + tuple(du.shape[-2:])).transpose(1, 2)
        ds0 = inv_j2_rot(unpool(d_s0), d_m2.unsqueeze(-1) * p2, *_q(b, swap=True))          # the trees swapped
        return inv_j1_rot(ds0, d_m1.unsqueeze(-1) * p1, *o, True), None, None, None


def layer1(x, b, mode, colour=False, bias=MAGBIAS):
    """``ScatLayer`` on a three-filter bank: (N, 7C, h, w) or (N, 9, h, w); an odd side repeats its last row / column."""
    if x.shape[2] % 2:
        x = torch.cat((x, x[:, :, -1:]), 2)
    if x.shape[3] % 2:
        x = torch.cat((x, x[:, :, :, -1:]), 3)
    Z = RScat1.apply(x, b, mode == "symmetric", bias, colour)
    return Z if colour else Z.reshape(Z.shape[0], -1, Z.shape[3], Z.shape[4])


def layer2(x, b, colour=False, bias=MAGBIAS):
    """``ScatLayerj2`` on a three-filter bank; a side is brought to a multiple of 8 by its own first and last rows."""
    for dim in (2, 3):
        rem = x.shape[dim] % 8
        if rem:
            n, before, after = x.shape[dim], (8 - rem) // 2, (9 - rem) // 2
            x = torch.cat((x.narrow(dim, 0, before), x, x.narrow(dim, n - after, after)), dim)
    Z = RScat2.apply(x, b, bias, colour)
    return Z if colour else Z.reshape(Z.shape[0], -1, Z.shape[3], Z.shape[4])


def restate_scat(x, b, order, mode, colour, cot, dtype):
    """{"Z", "xgrad"} of a layer from the restatement in ``dtype``."""
    b = {k: v.to(dtype) for k, v in b.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    Z = layer1(x, b, mode, colour) if order == 1 else layer2(x, b, colour)
    Z.backward(cot.to(dtype))
    return {"Z": Z.detach(), "xgrad": x.grad}


def dt_inputs(case):
    """(x, forward cotangents [yl, yh0 ..], inverse input (yl, yh) of float32 values, inverse cotangent) of a dtcwt case."""
    cid, mode, shape = case
    g = gold("dtcwt")
    cots = [decode(g[cid + "/cot_yl"])] + [decode(g[cid + "/cot_yh%d" % j]) for j in range(DT_J)]
    coeffs = (torch.from_numpy(g[cid + "/yl"]).float(), [torch.from_numpy(g[cid + "/yh%d" % j]).float() for j in range(DT_J)])
    return torch.from_numpy(g["x_%dx%dx%dx%d" % shape]), cots, coeffs, decode(g[cid + "/cot_inv"])


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_fixture_files_are_small():
    for which in ("scat", "dtcwt"):
        assert os.path.getsize(os.path.join(GOLDEN, "golden_rot_%s.npz" % which)) < 1 << 20


def test_fixture_bank_is_the_one_the_issue_names():
    """13, 19 and 19 level-1 taps, 14 q-shift taps (m/2 odd); the scattering file's nine parameters are the transform file's."""
    b, g = bufs(), gold("scat")
    assert [len(b[n]) for n in ("h0o", "h1o", "h2o")] == [13, 19, 19] and all(len(b[n]) == 14 for n in FWD_BUFS[2:6] + FWD_BUFS[7:])
    for n in SCAT_BUFS:
        assert np.array_equal(g["buf_" + n].reshape(-1), b[n].numpy())


@pytest.mark.parametrize("case", scat_cases(), ids=lambda c: c[0])
def test_scat_restatement_matches_reference(case):
    cid, order, mode, shape, colour = case
    g = gold("scat")
    ref = restate_scat(torch.from_numpy(g["x_%dx%dx%dx%d" % shape]), bufs(), order, mode, colour, decode(g[cid + "/cot"]), torch.float64)
    for k, v in ref.items():
        want = g[cid + "/" + k]
        assert tuple(v.shape) == want.shape, (k, tuple(v.shape), want.shape)
        assert rel_l2(v, want) <= 1e-12, (k, rel_l2(v, want))


@pytest.mark.parametrize("case", dt_cases(), ids=lambda c: c[0])
def test_dtcwt_restatement_matches_reference(case):
    cid, mode, shape = case
    g = gold("dtcwt")
    x, cots, coeffs, cot_inv = dt_inputs(case)
    ref, _ = restate_dt(x, bufs(), mode, DT_J, cots, coeffs, cot_inv, torch.float64)
    assert len(ref) == 10
    for k, v in ref.items():
        want = g[cid + "/" + k]
        assert tuple(v.shape) == want.shape, (k, tuple(v.shape), want.shape)
        assert rel_l2(v, want) <= 1e-12, (k, rel_l2(v, want))


def test_fp32_reference_error_is_meaningful():
    """The fp32 reference sits 1e-9 .. 2e-6 from the fp64 one on every array: e_ref of the GPU test's bar is neither zero nor large."""
    for which, cases, keys in (("scat", scat_cases(), ("Z", "xgrad")),
                               ("dtcwt", dt_cases(), ("yl", "yh0", "yh1", "yh2", "xgrad", "inv", "inv_gyl", "inv_gyh0", "inv_gyh1", "inv_gyh2"))):
        g = gold(which)
        for case in cases:
            for k in keys:
                e = rel_l2(g[case[0] + "/f32/" + k], g[case[0] + "/" + k])
                assert 1e-9 < e < 2e-6, (case[0], k, e)


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_entry_points_are_declared(fa):
    """One entry point per launch, none with a ``_bp`` twin, each binding the argument list with the optional third filter: the
    pointers and lengths of three level-1 filters, or six q-shift pointers and their one length, then mode or nothing and the stream."""
    assert len(THIRD_ARG) == 8
    assert not [s for s in fa._lib.declared_symbols() if s.endswith("_bp")]
    for n, at in THIRD_ARG.items():
        assert "faoctasr_" + n in fa._lib.declared_symbols()
        codes = fa._lib._SIG[n][1].replace(" ", "")
        assert codes[at - 8:] == ("liii" + "pipipi" + "ip" if n.endswith("j1") else "liii" + "pppppp" + "ip"), (n, codes)


def entry_args(fa, name, taps, third_len=None, m=None, **data):
    """The arguments of entry ``name`` on one 1 x 1 x 8 x 8 plane with NULL data pointers and zero strides, bar ``data`` (position:
    pointer); ``taps`` are the three (pointer, length) pairs or the six pointers, None for a NULL."""
    at = THIRD_ARG[name]
    a = [{"p": None, "i": 0, "l": 0, "f": 0.0}[c] for c in fa._lib._SIG[name][1].replace(" ", "")]
    a[at - 8:at - 4] = [1, 1, 8, 8]
    if name.endswith("j1"):
        a[at - 4:at + 3] = [v for t in taps for v in ((fa.ops._tap_array(t), len(t)) if t is not None else (None, 0))] + [1]
        if third_len is not None:
            a[at + 1] = third_len
    else:
        a[at - 4:at + 3] = [fa.ops._tap_array(t) if t is not None else None for t in taps] + [len(taps[1]) if m is None else m]
    for k, v in data.items():
        a[int(k[1:])] = v
    return a


def test_tap_arguments_choose_the_form_before_any_launch(fa):
    """The third filter of the eight entry points is optional, and the tap arguments alone decide the form.  No GPU: every call
    here fails validation.  dt_with_taps1 / dt_with_taps2 / dt_with_tapsi (csrc/dtcwt_dev.h) check and pack the taps without a HIP
    call and hand them to run_* of the chosen form, whose first statement (sc_common in run_fwd_* of scat.hip) returns "null
    pointer" for the NULL data pointers passed here; the lowpass-alone refusal of dtcwt_fwd_j* follows only shape and block-count
    checks and precedes its launch.  So "null pointer" means: taps accepted, form chosen, data check reached."""
    lib = fa._lib.load()
    b = {k: tuple(v.float().tolist()) for k, v in bufs().items()}
    three1, three2 = (b["h0o"], b["h1o"], b["h2o"]), (b["h0a"], b["h0b"], b["h1a"], b["h1b"], b["h2a"], b["h2b"])
    host = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)            # a non-null x / ll for the checks that follow the first

    def refused(name, words, *a, **kw):
        rc, msg = getattr(lib, "faoctasr_" + name)(*entry_args(fa, name, *a, **kw)), lib.faoctasr_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and all(w in msg for w in words), (name, a, kw, rc, msg)

    for name in THIRD_ARG:
        if name.endswith("j1"):
            refused(name, ["null pointer"], three1[:2] + (None,))
            refused(name, ["null pointer"], three1)
            for L2 in (4, 1, 21):
                refused(name, ["third-filter tap count %d " % L2], three1, third_len=L2)
            refused(name, ["NULL third filter", "got 5"], three1[:2] + (None,), third_len=5)
            refused(name, ["null tap pointer"], (None,) + three1[1:])
        else:
            refused(name, ["null pointer"], three2[:4] + (None, None))
            refused(name, ["null pointer"], three2)
            refused(name, ["third filter pair (a2, b2)"], three2[:5] + (None,))
            refused(name, ["third filter pair (a2, b2)"], three2[:4] + (None, three2[5]))
            refused(name, ["null tap pointer"], (None,) + three2[1:])
            refused(name, ["q-shift tap count 13"], three2, m=13)
    for name, taps, two in (("dtcwt_fwd_j1", three1, three1[:2] + (None,)), ("dtcwt_fwd_j2", three2, three2[:4] + (None, None))):
        refused(name, ["null pointer"], taps, a0=host)                       # x alone: neither output
        refused(name, ["no third filter", "pass a NULL third filter"], taps, a0=host, a4=host)     # x and ll, no hi: the lowpass alone
        refused(name, ["H 7 W 8"], two, a0=host, a4=host, **{"a%d" % (THIRD_ARG[name] - 6): 7})     # two filters pass that check: the shape is next


def test_modules_register_the_reference_parameters(fa):
    b = bufs()
    fb, fq = tuples(b)
    gb, gq = tuples(b, analysis=False)
    one, two = fa.ScatLayer(biort=fb), fa.ScatLayerj2(biort=fb, qshift=fq)
    fwd, inv = fa.DTCWTForward(biort=fb, qshift=fq), fa.DTCWTInverse(biort=gb, qshift=gq)
    assert list(one.state_dict()) == ["h0o", "h1o", "h2o"] and list(two.state_dict()) == list(SCAT_BUFS)
    assert [n for n, _ in two.named_parameters()] == list(SCAT_BUFS) and not list(two.buffers())
    assert list(fwd.state_dict()) == list(FWD_BUFS) and list(inv.state_dict()) == list(INV_BUFS)
    assert not list(fwd.parameters()) and not list(inv.parameters())
    for mod in (one, two, fwd, inv):
        assert mod.bandpass_diag is True
        for n, p in mod.state_dict().items():
            assert p.dtype == torch.float32 and tuple(p.shape) == (1, 1, len(b[n]), 1) and not p.requires_grad
            assert torch.equal(p.reshape(-1), b[n].float()), n
    for n, p in two.named_parameters():
        assert isinstance(p, torch.nn.Parameter) and not p.requires_grad
    assert one.extra_repr().endswith("mode='symmetric', magbias=0.01") and two.extra_repr().endswith("mode='symmetric', magbias=0.01")


def test_two_filter_modules_are_unchanged(fa):
    b = bufs()
    fb, fq = tuples(b)
    one, two = fa.ScatLayer(biort=fb[:2]), fa.ScatLayerj2(biort=fb[:2], qshift=fq[:4])
    fwd = fa.DTCWTForward(biort=fb[:2], qshift=fq[:4])
    assert list(one.state_dict()) == ["h0o", "h1o"] and list(two.state_dict()) == list(SCAT_BUFS[:2] + SCAT_BUFS[3:7])
    assert list(fwd.state_dict()) == list(FWD_BUFS[:6])
    assert one.bandpass_diag is False and two.bandpass_diag is False and fwd.bandpass_diag is False


def test_reference_shaped_state_dict_loads(fa):
    b = bufs()
    fb, fq = tuples(b)
    dst = fa.ScatLayerj2(biort=([0.0] * 13, [0.0] * 19, [0.0] * 19), qshift=[[0.0] * 14] * 6)
    sd = {n: b[n].float().reshape(1, 1, -1, 1) for n in SCAT_BUFS}                       # as the reference's layer lists them
    dst.load_state_dict(sd)
    src = fa.ScatLayerj2(biort=fb, qshift=fq)
    assert all(torch.equal(getattr(dst, n), getattr(src, n)) for n in SCAT_BUFS)
    assert dst._taps == src._taps                                                        # the host record follows the load
    with pytest.raises(RuntimeError, match="h2o"):
        fa.ScatLayerj2(biort=fb[:2], qshift=fq[:4]).load_state_dict(sd)                  # a two-filter layer has no such key


def test_pairing_and_tuple_lengths(fa):
    b = bufs()
    fb, fq = tuples(b)
    for cls in (fa.ScatLayerj2, fa.DTCWTForward, fa.DTCWTInverse):
        with pytest.raises(ValueError, match="three-filter biort.*three-filter qshift"):
            cls(biort=fb, qshift=fq[:4])
        with pytest.raises(ValueError, match="three-filter biort.*three-filter qshift"):
            cls(biort=fb[:2], qshift=fq)
        with pytest.raises(ValueError, match="2-tuple"):
            cls(biort=fb + fb[:1], qshift=fq)
        with pytest.raises(ValueError, match="4-tuple"):
            cls(biort=fb, qshift=fq[:3])
        with pytest.raises(ValueError, match="4-tuple"):
            cls(biort=fb, qshift=fq[:5])
    with pytest.raises(ValueError, match="2-tuple"):
        fa.ScatLayer(biort=fb + fb[:1])
    with pytest.raises(ValueError, match="2-tuple"):                                     # the magnitude loss stays two-filter only
        fa.DTCWTMagnitudeLoss(biort=fb, qshift=fq, J=2)
    with pytest.raises(ValueError, match="4-tuple"):
        fa.DTCWTMagnitudeLoss(biort=fb[:2], qshift=fq, J=2)


def test_third_filter_length_checks(fa):
    b = bufs()
    fb, fq = tuples(b)
    ops, x = fa.ops, torch.zeros(1, 3, 8, 8)
    o3, o5, e10 = [0.25, 0.5, 0.25], [0.1] * 5, [0.1] * 10
    hi = torch.zeros(1, 3, 6, 4, 4, 2)
    for bad in ([0.1] * 4, [0.1] * 21, [0.1]):
        for call in (lambda: ops.scat_layer_j1(x, o5, o3, h2o=bad), lambda: ops.dtcwt_fwd_j1(x, o5, o3, h2o=bad),
                     lambda: ops.dtcwt_inv_j1(x, hi, o5, o3, g2o=bad), lambda: fa.ScatLayer(biort=(o5, o3, bad)),
                     lambda: ops.scat_layer_j2(x, o5, o3, e10, e10, e10, e10, h2o=bad, h2a=e10, h2b=e10)):
            with pytest.raises(ValueError, match="third level-1 filter.*odd"):
                call()
    for call in (lambda: ops.dtcwt_fwd_j2(x, e10, e10, e10, e10, h2a=e10, h2b=[0.1] * 8),
                 lambda: ops.dtcwt_inv_j2(x, None, e10, e10, e10, e10, g2a=[0.1] * 12, g2b=e10),
                 lambda: ops.scat_layer_j2(x, o5, o3, e10, e10, e10, e10, h2o=o3, h2a=e10, h2b=[0.1] * 12),
                 lambda: fa.ScatLayerj2(biort=fb, qshift=fq[:5] + ([0.1] * 16,))):
        with pytest.raises(ValueError, match="third q-shift filters must have the length of the other four"):
            call()
    with pytest.raises(ValueError, match="come as a pair"):
        ops.dtcwt_fwd_j2(x, e10, e10, e10, e10, h2a=e10)
    for kw in (dict(h2o=o3), dict(h2a=e10, h2b=e10), dict(h2o=o3, h2a=e10)):
        with pytest.raises(ValueError, match="all of h2o, h2a and h2b"):
            ops.scat_layer_j2(x, o5, o3, e10, e10, e10, e10, **kw)


def test_bp_names_stay_refused(fa):
    with pytest.raises(NotImplementedError, match="near_sym_b_bp.*third filter"):
        fa.ScatLayer(biort="near_sym_b_bp")
    with pytest.raises(NotImplementedError, match="near_sym_b_bp.*third filter"):
        fa.ScatLayerj2(biort="near_sym_b_bp", qshift="qshift_b_bp")
    with pytest.raises(NotImplementedError, match="qshift_b_bp.*third filter"):
        fa.ScatLayerj2(biort=tuples(bufs())[0], qshift="qshift_b_bp")
    with pytest.raises(NotImplementedError, match="three-filter"):
        fa.DTCWTMagnitudeLoss(biort="near_sym_b_bp")
    with pytest.raises(NotImplementedError, match="3-tuple.*6-tuple"):                  # the message says what to pass instead
        fa.ScatLayer(biort="near_sym_b_bp")


def test_bp_tables_through_a_provider(fa, monkeypatch):
    b = bufs()
    w = {k: v.flip(0).numpy() for k, v in b.items()}
    mod = types.ModuleType("rot_provider_for_test")
    mod.coeffs = types.ModuleType("rot_provider_for_test.coeffs")
    order_b = ("h0o", "g0o", "h1o", "g1o", "h2o", "g2o")
    order_q = ("h0a", "h0b", "g0a", "g0b", "h1a", "h1b", "g1a", "g1b", "h2a", "h2b", "g2a", "g2b")

    def biort(name):
        assert name in ("near_sym_b_bp", "near_sym_b")
        return tuple(w[n].reshape(-1, 1) for n in (order_b if name.endswith("_bp") else order_b[:4]))

    def qshift(name):
        assert name in ("qshift_b_bp", "qshift_b")
        return tuple(w[n].reshape(-1, 1) for n in (order_q if name.endswith("_bp") else order_q[:8]))
    mod.coeffs.biort, mod.coeffs.qshift = biort, qshift
    monkeypatch.setitem(sys.modules, "rot_provider_for_test", mod)
    monkeypatch.setitem(sys.modules, "rot_provider_for_test.coeffs", mod.coeffs)
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("rot_provider_for_test.coeffs",))
    tb, tq = fa.wavelets.dtcwt_biort_bp("near_sym_b_bp"), fa.wavelets.dtcwt_qshift_bp("qshift_b_bp")
    assert len(tb) == 6 and len(tq) == 12
    for got, n in zip(tb + tq, order_b + order_q):
        assert got.dtype == np.float64 and got.ndim == 1 and np.array_equal(got, w[n]), n
    layer = fa.ScatLayerj2(biort=(tb[0], tb[2], tb[4]), qshift=(tq[0], tq[1], tq[4], tq[5], tq[8], tq[9]))       # the one-liner
    assert all(torch.equal(getattr(layer, n).reshape(-1), b[n].float()) for n in SCAT_BUFS)
    with pytest.raises(ValueError, match="no three-filter"):
        fa.wavelets.dtcwt_biort_bp("near_sym_b")
    with pytest.raises(ValueError, match="no three-filter"):
        fa.wavelets.dtcwt_qshift_bp("qshift_b")
    with pytest.raises(NotImplementedError, match="third filter"):                       # a provider does not un-refuse the names
        fa.ScatLayer(biort="near_sym_b_bp")
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("no_such_module_for_dtcwt.coeffs",))
    with pytest.raises(NotImplementedError, match="near_sym_b_bp"):
        fa.wavelets.dtcwt_biort_bp("near_sym_b_bp")


def test_every_refusal_is_raised_on_the_host(fa, monkeypatch):
    """CPU tensors throughout and an ``ops.call`` that fails the test if reached: each named check fires before any launch."""
    def no_call(name, *a):
        raise AssertionError("entry point %s reached" % name)
    monkeypatch.setattr(fa.ops, "call", no_call)
    b = bufs()
    fb, fq = tuples(b)
    gb, gq = tuples(b, analysis=False)
    ops, x = fa.ops, torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="4 dimensions"):
        fa.ScatLayer(biort=fb)(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="3 channels"):
        fa.ScatLayerj2(biort=fb, qshift=fq, combine_colour=True)(torch.zeros(1, 1, 8, 8))
    with pytest.raises(NotImplementedError, match="symmetric"):
        fa.ScatLayerj2(biort=fb, qshift=fq, mode="zero")(x)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.scat_layer_j2(torch.zeros(1, 1, 8, 12), *fb[:2], *fq[:4], h2o=fb[2], h2a=fq[4], h2b=fq[5])
    with pytest.raises(ValueError, match="float32"):
        fa.ScatLayer(biort=fb)(x.double())
    with pytest.raises(ValueError, match="device"):
        fa.ScatLayer(biort=fb)(x)
    with pytest.raises(ValueError, match="device"):
        fa.ScatLayerj2(biort=fb, qshift=fq)(x)
    with pytest.raises(ValueError, match="device"):
        fa.DTCWTForward(biort=fb, qshift=fq, J=2)(x)
    with pytest.raises(ValueError, match="device"):
        fa.DTCWTInverse(biort=gb, qshift=gq)((torch.zeros(1, 3, 4, 4), [torch.zeros(1, 3, 6, 4, 4, 2), torch.zeros(1, 3, 6, 2, 2, 2)]))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.dtcwt_fwd_j2(torch.zeros(1, 1, 6, 8), *fq[:4], h2a=fq[4], h2b=fq[5])
