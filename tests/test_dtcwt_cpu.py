"""The dual-tree complex wavelet transform without a GPU: a float64 restatement in plain torch, written from the index maps of
DESIGN.md (not from the reference's text), pinned to the reference's own float64 results (tests/golden/golden_dtcwt_*.npz,
tools/gen_golden_dtcwt.py), the dot-product identity of its forward / backward pairs, and the host logic of ``ops`` and
``wavelets`` (everything that raises before an entry point is reached).

Bounds.  Restatement against the fixtures' float64 arrays: relative L2 <= 1e-12 -- both sides are float64 sums of at most a few
hundred terms, about 1e-14 of rounding, so 1e-12 leaves 100x.  Dot-product identity <F x, c> = <x, F' c>: <= 1e-10 relative (the
reference itself shows <= 8e-13).  Closed-form banks against the fixture's registered buffers: 1e-15 absolute."""
import glob
import math
import os

import numpy as np
import pytest
import torch
from torch.autograd import Function

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BANKS = ("a", "b", "c")
MODES = ("symmetric", "zero")
SHAPES = (((2, 3, 16, 24), 3), ((1, 2, 13, 18), 3), ((1, 1, 4, 4), 3), ((1, 2, 40, 36), 2))
FWD_BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")
INV_BUFS = ("g0o", "g1o", "g0a", "g0b", "g1a", "g1b")
_S = 1.0 / math.sqrt(2.0)
_gold = {}


def gold(bank, mode):
    if (bank, mode) not in _gold:
        with np.load(os.path.join(GOLDEN, "golden_dtcwt_%s_%s.npz" % (bank, mode))) as z:
            _gold[bank, mode] = {k: z[k] for k in z.files}
    return _gold[bank, mode]


def fixture_cases():
    return [("%s_%s_J%d_%dx%dx%dx%d" % ((b, m, J) + s), b, m, J, s) for b in BANKS for m in MODES for s, J in SHAPES]


def bufs(bank, dtype=torch.float64):
    """The twelve registered buffers of a bank pair as flat tensors: {name: taps reversed, as prep_filt stores them}."""
    g = gold(bank, "symmetric")
    return {n: torch.from_numpy(g["buf_" + n]).reshape(-1).to(dtype) for n in FWD_BUFS + INV_BUFS}


def decode(codes, dtype=torch.float32):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5)).to(dtype)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    d = float((a - b).norm())
    n = float(b.norm())
    return d / n if n else d


# ------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------
def take(x, pos, dim, sym):
    """x along ``dim`` at the positions ``pos`` of its extension: the half-sample symmetric fold of period 2N, or zeros."""
    N = x.shape[dim]
    pos = np.asarray(pos, dtype=np.int64)
    if sym:
        m = np.mod(pos, 2 * N)
        return x.index_select(dim, torch.from_numpy(np.where(m < N, m, 2 * N - 1 - m)).to(x.device))
    ok = (pos >= 0) & (pos < N)
    shape = [1] * x.dim()
    shape[dim] = len(pos)
    return x.index_select(dim, torch.from_numpy(np.clip(pos, 0, N - 1)).to(x.device)) * torch.from_numpy(ok).to(x).reshape(shape)


def same_filter(x, buf, dim, sym):
    """out[i] = sum_t buf[t] xs[i + t - L // 2], L odd."""
    L, i = len(buf), np.arange(x.shape[dim])
    return sum(buf[t] * take(x, i + t - L // 2, dim, sym) for t in range(L))


def interleave(parts, dim):
    """out[k i + q] = parts[q][i] along ``dim``."""
    dim = dim % parts[0].dim()
    s = list(parts[0].shape)
    s[dim] *= len(parts)
    return torch.stack(parts, dim=dim + 1).reshape(s)


def dfilt(x, fa, fb, dim, highpass):
    """The two-tree decimation by 2: A[i] = sum_t fa[t] xs[4i + 2t + 2 - m], B[i] = sum_t fb[t] xs[4i + 2t + 3 - m]; out = A, B
    interleaved, B first for a highpass call."""
    r, m = x.shape[dim], len(fa)
    assert r % 4 == 0 and len(fb) == m
    i = np.arange(r // 4)
    A = sum(fa[t] * take(x, 4 * i + 2 * t + 2 - m, dim, True) for t in range(m))
    B = sum(fb[t] * take(x, 4 * i + 2 * t + 3 - m, dim, True) for t in range(m))
    return interleave([B, A] if highpass else [A, B], dim)


def ifilt_table(m2, highpass):
    """Per output phase q of the 2x interpolation: (filter: 0 first argument / 1 second, polyphase half: 0 even / 1 odd taps,
    offset d), for out[4i + q] = sum_t half[t] xs[2 (i + t) + d - m2]."""
    if m2 % 2 == 0:
        return ((0, 0, 1), (1, 0, 0), (0, 1, 3), (1, 1, 2)) if highpass else ((0, 0, 0), (1, 0, 1), (0, 1, 2), (1, 1, 3))
    return ((0, 1, 2), (1, 1, 1), (0, 0, 2), (1, 0, 1)) if highpass else ((0, 1, 1), (1, 1, 2), (0, 0, 1), (1, 0, 2))


def ifilt(x, fa, fb, dim, highpass):
    r, m2 = x.shape[dim], len(fa) // 2
    assert r % 2 == 0
    i = np.arange(r // 2)
    parts = []
    for which, odd, d in ifilt_table(m2, highpass):
        half = (fb if which else fa)[odd::2]
        parts.append(sum(half[t] * take(x, 2 * (i + t) + d - m2, dim, True) for t in range(m2)))
    return interleave(parts, dim)


def q2c(y):
    y = y * _S
    a, b, c, d = y[..., 0::2, 0::2], y[..., 0::2, 1::2], y[..., 1::2, 0::2], y[..., 1::2, 1::2]
    return torch.stack((a - d, b + c), -1), torch.stack((a + d, b - c), -1)


def c2q(w1, w2):
    y = w1.new_zeros(w1.shape[:-3] + (2 * w1.shape[-3], 2 * w1.shape[-2]))
    y[..., 0::2, 0::2] = w1[..., 0] + w2[..., 0]
    y[..., 0::2, 1::2] = w1[..., 1] + w2[..., 1]
    y[..., 1::2, 0::2] = w1[..., 1] - w2[..., 1]
    y[..., 1::2, 1::2] = w2[..., 0] - w1[..., 0]
    return y * _S


def to_orientations(lh, hl, hh):
    """(N, C, 6, H', W', 2): 15, 45, 75, 105, 135, 165 degrees."""
    (d15, d165), (d45, d135), (d75, d105) = q2c(lh), q2c(hh), q2c(hl)
    return torch.stack((d15, d45, d75, d105, d135, d165), 2)


def from_orientations(h):
    return c2q(h[:, :, 0], h[:, :, 5]), c2q(h[:, :, 2], h[:, :, 3]), c2q(h[:, :, 1], h[:, :, 4])      # lh, hl, hh


def fwd_j1(x, h0, h1, sym, highs=True):
    lo = same_filter(x, h0, 3, sym)
    ll = same_filter(lo, h0, 2, sym)
    if not highs:
        return ll, None
    hi = same_filter(x, h1, 3, sym)
    return ll, to_orientations(same_filter(lo, h1, 2, sym), same_filter(hi, h0, 2, sym), same_filter(hi, h1, 2, sym))


def inv_j1(ll, h, g0, g1, sym):
    """ll or h may be None (zeros)."""
    lo = hi = None
    if h is not None:
        lh, hl, hh = from_orientations(h)
        hi = same_filter(hh, g1, 2, sym) + same_filter(hl, g0, 2, sym)
        lo = same_filter(lh, g1, 2, sym)
    if ll is not None:
        t = same_filter(ll, g0, 2, sym)
        lo = t if lo is None else lo + t
    y = same_filter(lo, g0, 3, sym)
    return y if hi is None else same_filter(hi, g1, 3, sym) + y


def fwd_j2(x, h0a, h0b, h1a, h1b, highs=True):
    lo = dfilt(x, h0b, h0a, 3, False)
    ll = dfilt(lo, h0b, h0a, 2, False)
    if not highs:
        return ll, None
    hi = dfilt(x, h1b, h1a, 3, True)
    return ll, to_orientations(dfilt(lo, h1b, h1a, 2, True), dfilt(hi, h0b, h0a, 2, False), dfilt(hi, h1b, h1a, 2, True))


def inv_j2(ll, h, g0a, g0b, g1a, g1b):
    lo = hi = None
    if h is not None:
        lh, hl, hh = from_orientations(h)
        hi = ifilt(hh, g1b, g1a, 2, True) + ifilt(hl, g0b, g0a, 2, False)
        lo = ifilt(lh, g1b, g1a, 2, True)
    if ll is not None:
        t = ifilt(ll, g0b, g0a, 2, False)
        lo = t if lo is None else lo + t
    y = ifilt(lo, g0b, g0a, 3, False)
    return y if hi is None else ifilt(hi, g1b, g1a, 3, True) + y


class RFwdJ1(Function):
    """The backward is the level-1 inverse on the analysis buffers."""

    @staticmethod
    def forward(ctx, x, h0, h1, sym, highs):
        ctx.cfg = (h0, h1, sym)
        ctx.set_materialize_grads(False)
        ll, h = fwd_j1(x, h0, h1, sym, highs)
        return (ll, h) if highs else ll

    @staticmethod
    def backward(ctx, dl, dh=None):
        return inv_j1(dl, dh, *ctx.cfg), None, None, None, None


class RFwdJ2(Function):
    """The backward is the level >= 2 inverse on the analysis buffers with a and b swapped."""

    @staticmethod
    def forward(ctx, x, h0a, h0b, h1a, h1b, highs):
        ctx.cfg = (h0b, h0a, h1b, h1a)
        ctx.set_materialize_grads(False)
        ll, h = fwd_j2(x, h0a, h0b, h1a, h1b, highs)
        return (ll, h) if highs else ll

    @staticmethod
    def backward(ctx, dl, dh=None):
        return inv_j2(dl, dh, *ctx.cfg), None, None, None, None, None


class RInvJ1(Function):
    """The backward is the level-1 forward on the synthesis buffers."""

    @staticmethod
    def forward(ctx, ll, h, g0, g1, sym):
        ctx.cfg = (g0, g1, sym)
        return inv_j1(ll, h, g0, g1, sym)

    @staticmethod
    def backward(ctx, dy):
        dl, dh = fwd_j1(dy, *ctx.cfg, highs=ctx.needs_input_grad[1])
        return dl if ctx.needs_input_grad[0] else None, dh, None, None, None


class RInvJ2(Function):
    """The backward is the level >= 2 forward on the synthesis buffers with a and b swapped."""

    @staticmethod
    def forward(ctx, ll, h, g0a, g0b, g1a, g1b):
        ctx.cfg = (g0b, g0a, g1b, g1a)
        return inv_j2(ll, h, g0a, g0b, g1a, g1b)

    @staticmethod
    def backward(ctx, dy):
        dl, dh = fwd_j2(dy, *ctx.cfg, highs=ctx.needs_input_grad[1])
        return dl if ctx.needs_input_grad[0] else None, dh, None, None, None, None


def forward_levels(x, b, mode, J, skip=None):
    """The module-level forward: (yl, [yh_j or None])."""
    skip = skip or [False] * J
    if x.shape[2] % 2:
        x = torch.cat((x, x[:, :, -1:]), 2)
    if x.shape[3] % 2:
        x = torch.cat((x, x[:, :, :, -1:]), 3)
    out = RFwdJ1.apply(x, b["h0o"], b["h1o"], mode == "symmetric", not skip[0])
    low, yh = (out[0], [out[1]]) if not skip[0] else (out, [None])
    for j in range(1, J):
        if low.shape[2] % 4:
            low = torch.cat((low[:, :, :1], low, low[:, :, -1:]), 2)
        if low.shape[3] % 4:
            low = torch.cat((low[:, :, :, :1], low, low[:, :, :, -1:]), 3)
        out = RFwdJ2.apply(low, b["h0a"], b["h0b"], b["h1a"], b["h1b"], not skip[j])
        low = out if skip[j] else out[0]
        yh.append(None if skip[j] else out[1])
    return low, yh


def inverse_levels(yl, yh, b, mode):
    low = yl
    for h in yh[:0:-1]:
        if h is not None:
            if low.shape[2] != 2 * h.shape[3]:
                low = low[:, :, 1:-1]
            if low.shape[3] != 2 * h.shape[4]:
                low = low[:, :, :, 1:-1]
        low = RInvJ2.apply(low, h, b["g0a"], b["g0b"], b["g1a"], b["g1b"])
    h = yh[0]
    if h is not None:
        if low.shape[2] != 2 * h.shape[3]:
            low = low[:, :, 1:-1]
        if low.shape[3] != 2 * h.shape[4]:
            low = low[:, :, :, 1:-1]
    return RInvJ1.apply(low, h, b["g0o"], b["g1o"], mode == "symmetric")


def restate(x, b, mode, J, cots, coeffs, cot_inv, dtype):
    """Every array a fixture case holds, from the restatement in ``dtype``."""
    b = {k: v.to(dtype) for k, v in b.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    yl, yh = forward_levels(x, b, mode, J)
    out = {"yl": yl.detach()}
    for j, h in enumerate(yh):
        out["yh%d" % j] = h.detach()
    torch.autograd.backward([yl] + yh, [c.to(dtype) for c in cots])
    out["xgrad"] = x.grad
    cl = coeffs[0].to(dtype).clone().requires_grad_(True)
    ch = [h.to(dtype).clone() for h in coeffs[1]]
    ch[0].requires_grad_(True)
    y = inverse_levels(cl, ch, b, mode)
    out["inv"] = y.detach()
    y.backward(cot_inv.to(dtype))
    out["inv_gyl"], out["inv_gyh0"] = cl.grad, ch[0].grad
    with torch.no_grad():
        out["inv_none"] = inverse_levels(cl.detach(), [h.detach() for h in ch[:-1]] + [None], b, mode)
        sl, sh = forward_levels(x.detach(), b, mode, J, skip=[False, True] + [False] * (J - 2))
        out["skip_yl"] = sl
        for j in range(2, J):
            out["skip_yh%d" % j] = sh[j]
    return out


def fixture_inputs(case):
    cid, bank, mode, J, shape = case
    g = gold(bank, mode)
    x = torch.from_numpy(g["x_%dx%dx%dx%d" % shape])
    cots = [decode(g[cid + "/cot_yl"])] + [decode(g[cid + "/cot_yh%d" % j]) for j in range(J)]
    coeffs = (torch.from_numpy(g[cid + "/yl"]).float(), [torch.from_numpy(g[cid + "/yh%d" % j]).float() for j in range(J)])
    return x, cots, coeffs, decode(g[cid + "/cot_inv"])


_restated = {}


def restate_case(case):
    """The float64 restatement of a fixture case, computed once and shared (do not modify the arrays)."""
    if case[0] not in _restated:
        x, cots, coeffs, cot_inv = fixture_inputs(case)
        _restated[case[0]] = restate(x, bufs(case[1]), case[2], case[3], cots, coeffs, cot_inv, torch.float64)
    return _restated[case[0]]


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_fixture_files_are_small():
    files = glob.glob(os.path.join(GOLDEN, "golden_dtcwt_*.npz"))
    assert len(files) == 6 and all(os.path.getsize(f) < 1 << 20 for f in files)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_restatement_matches_reference(case):
    g, ref = gold(case[1], case[2]), restate_case(case)
    assert len(ref) == 5 + 2 * case[3]
    for k, v in ref.items():
        want = g[case[0] + "/" + k]
        assert tuple(v.shape) == want.shape, (k, tuple(v.shape), want.shape)
        assert rel_l2(v, want) <= 1e-12, (k, rel_l2(v, want))


def test_fp32_reference_error_is_meaningful():
    """The fp32 reference sits 1e-8 .. 1e-6 from the fp64 one: e_ref of the GPU test's bar is neither zero nor large."""
    for case in fixture_cases():
        g = gold(case[1], case[2])
        for k in restate_case(case):
            e = rel_l2(g[case[0] + "/f32/" + k], g[case[0] + "/" + k])
            assert 1e-9 < e < 2e-6, (case[0], k, e)


@pytest.mark.parametrize("bank", BANKS)
@pytest.mark.parametrize("mode", MODES)
def test_dot_product_identity(bank, mode):
    """<F x, c> = <x, F' c> for the four forward / backward pairs as restated (each backward is written out above, not derived
    by autograd), on sides that fold more than once (4) and that do not."""
    b, sym = bufs(bank), mode == "symmetric"
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    dot = lambda a, c: float((a * c).sum())

    def check(name, lhs, rhs):
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs), 1e-30), (name, lhs, rhs)

    for H, W in ((4, 8), (12, 20)):
        x, cl, ch = rnd(2, 2, H, W), rnd(2, 2, H, W), rnd(2, 2, 6, H // 2, W // 2, 2)
        ll, h = fwd_j1(x, b["h0o"], b["h1o"], sym)
        check("fwd_j1", dot(ll, cl) + dot(h, ch), dot(x, inv_j1(cl, ch, b["h0o"], b["h1o"], sym)))
        y = rnd(2, 2, H, W)
        dl, dh = fwd_j1(y, b["g0o"], b["g1o"], sym)
        check("inv_j1", dot(inv_j1(cl, ch, b["g0o"], b["g1o"], sym), y), dot(cl, dl) + dot(ch, dh))
        cl, ch = rnd(2, 2, H // 2, W // 2), rnd(2, 2, 6, H // 4, W // 4, 2)
        ll, h = fwd_j2(x, b["h0a"], b["h0b"], b["h1a"], b["h1b"])
        check("fwd_j2", dot(ll, cl) + dot(h, ch), dot(x, inv_j2(cl, ch, b["h0b"], b["h0a"], b["h1b"], b["h1a"])))
        y = rnd(2, 2, H, W)
        dl, dh = fwd_j2(y, b["g0b"], b["g0a"], b["g1b"], b["g1a"])
        check("inv_j2", dot(inv_j2(cl, ch, b["g0a"], b["g0b"], b["g1a"], b["g1b"]), y), dot(cl, dl) + dot(ch, dh))


def test_restated_reconstruction():
    for bank in BANKS:
        b = bufs(bank)
        x = torch.randn(1, 2, 13, 22, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        yl, yh = forward_levels(x, b, "symmetric", 3)
        y = inverse_levels(yl, yh, b, "symmetric")
        assert float((y[:, :, :13] - x).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def tuples(bank):
    b = bufs(bank)
    w = {k: v.flip(0).tolist() for k, v in b.items()}              # back to the order the constructor takes
    return ((w["h0o"], w["h1o"]), (w["h0a"], w["h0b"], w["h1a"], w["h1b"])), ((w["g0o"], w["g1o"]), (w["g0a"], w["g0b"], w["g1a"], w["g1b"]))


def test_exports(fa):
    assert fa.DTCWT is fa.DTCWTForward and fa.IDTCWT is fa.DTCWTInverse
    assert fa.ops.DTCWT_MAX_TAPS == 20
    for n in ("dtcwt_fwd_j1", "dtcwt_fwd_j2", "dtcwt_inv_j1", "dtcwt_inv_j2"):
        assert "faoctasr_" + n in fa._lib.declared_symbols()


@pytest.mark.parametrize("bank", BANKS)
def test_modules_register_the_reference_buffers(fa, bank):
    (fb, fq), (ib, iq) = tuples(bank)
    fwd, inv = fa.DTCWTForward(biort=fb, qshift=fq), fa.DTCWTInverse(biort=ib, qshift=iq)
    b = bufs(bank)
    assert list(fwd.state_dict()) == list(FWD_BUFS) and list(inv.state_dict()) == list(INV_BUFS)
    for mod, names in ((fwd, FWD_BUFS), (inv, INV_BUFS)):
        for n in names:
            t = getattr(mod, n)
            assert t.dtype == torch.float32 and tuple(t.shape) == (1, 1, len(b[n]), 1)
            assert torch.equal(t.reshape(-1), b[n].float())
    assert (fwd.J, fwd.o_dim, fwd.ri_dim, fwd.mode, fwd.skip_hps, fwd.include_scale) == (3, 2, -1, "symmetric", [False] * 3, [False] * 3)
    assert (inv.o_dim, inv.ri_dim, inv.mode) == (2, -1, "symmetric")


def test_closed_form_banks(fa):
    """'near_sym_a' and 'legall' are built from their published rational forms and match the reference's registered buffers."""
    for name, bank in (("near_sym_a", "a"), ("legall", "c")):
        h0o, g0o, h1o, g1o = fa.wavelets.dtcwt_biort(name)
        b = bufs(bank)
        for got, n in ((h0o, "h0o"), (h1o, "h1o"), (g0o, "g0o"), (g1o, "g1o")):
            want = b[n].flip(0).numpy()
            assert len(got) == len(want) and np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-15, (name, n)
    q = tuples("a")
    fwd = fa.DTCWTForward(biort="near_sym_a", qshift=q[0][1])
    assert torch.equal(fwd.h1o.reshape(-1), bufs("a")["h1o"].float())
    inv = fa.DTCWTInverse(biort="legall", qshift=q[1][1])
    assert torch.equal(inv.g0o.reshape(-1), bufs("c")["g0o"].float())


def test_names_without_a_provider(fa, monkeypatch):
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("no_such_module_for_dtcwt.coeffs",))
    q = tuples("a")[0][1]
    with pytest.raises(NotImplementedError, match="qshift_a.*4-tuple"):
        fa.DTCWTForward()
    with pytest.raises(NotImplementedError, match="antonini.*2-tuple"):
        fa.DTCWTForward(biort="antonini", qshift=q)
    with pytest.raises(NotImplementedError, match="qshift_b"):
        fa.DTCWTInverse(qshift="qshift_b")


def test_names_through_a_provider(fa, monkeypatch):
    import sys
    import types
    (fb, fq), (ib, iq) = tuples("b")
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    mod = types.ModuleType("fake_dtcwt_coeffs")
    mod.biort = lambda name: tuple(col(v) for v in (fb[0], ib[0], fb[1], ib[1]))
    mod.qshift = lambda name: tuple(col(v) for v in (fq[0], fq[1], iq[0], iq[1], fq[2], fq[3], iq[2], iq[3]))
    monkeypatch.setitem(sys.modules, "fake_dtcwt_coeffs", mod)
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("fake_dtcwt_coeffs",))
    fwd, inv = fa.DTCWTForward(biort="near_sym_b", qshift="qshift_c"), fa.DTCWTInverse(biort="near_sym_b", qshift="qshift_c")
    b = bufs("b")
    for m_, names in ((fwd, FWD_BUFS), (inv, INV_BUFS)):
        for n in names:
            assert torch.equal(getattr(m_, n).reshape(-1), b[n].float()), n


def ref_layout(o_dim, ri_dim):
    """The shape the reference's two ``torch.stack`` calls give an (N, C, H', W') band, by doing them (its module refuses
    o_dim == ri_dim beforehand)."""
    if o_dim == ri_dim:
        raise IndexError("refused")
    o, r = o_dim % 6, ri_dim % 6
    if r < o:
        o -= 1
    t = torch.zeros(3, 5, 7, 11)
    return tuple(torch.stack([torch.stack([t] * 6, o)] * 2, r).shape)


def test_layout_bookkeeping(fa):
    sizes = {"n": 3, "c": 5, "h": 7, "w": 11, "o": 6, "r": 2}
    seen = 0
    for o in range(-6, 6):
        for r in range(-6, 6):
            try:
                want = ref_layout(o, r)
            except (IndexError, RuntimeError):
                with pytest.raises(ValueError):
                    fa.ops.dtcwt_layout(o, r)
                continue
            names = fa.ops.dtcwt_layout(o, r)
            assert sorted(names) == sorted("nchwor") and tuple(sizes[k] for k in names) == want, (o, r, names, want)
            seen += 1
    assert seen > 100
    assert fa.ops.dtcwt_layout(2, -1) == ("n", "c", "o", "h", "w", "r")
    with pytest.raises(ValueError, match="different dimensions"):
        fa.DTCWTForward(biort="legall", qshift=tuples("a")[0][1], o_dim=3, ri_dim=3)
    with pytest.raises(ValueError, match="different dimensions"):
        fa.ops.dtcwt_fwd_j1(torch.zeros(1, 1, 4, 4), [1.0], [1.0], False, 2, 2, 1)


def test_list_forms(fa):
    q = tuples("a")[0][1]
    m_ = fa.DTCWTForward(biort="legall", qshift=q, J=3, skip_hps=[False, True, False], include_scale=(True, False, True))
    assert m_.skip_hps == [False, True, False] and list(m_.include_scale) == [True, False, True]
    m_ = fa.DTCWTForward(biort="legall", qshift=q, J=2, skip_hps=True, include_scale=True)
    assert m_.skip_hps == [True, True] and m_.include_scale == [True, True]
    with pytest.raises(ValueError, match="skip_hps"):
        fa.DTCWTForward(biort="legall", qshift=q, J=3, skip_hps=[False, True])
    with pytest.raises(ValueError, match="include_scale"):
        fa.DTCWTForward(biort="legall", qshift=q, J=3, include_scale=[False])
    x = torch.zeros(1, 1, 8, 8)
    assert fa.DTCWTForward(biort="legall", qshift=q, J=0)(x)[0] is x and fa.DTCWTForward(biort="legall", qshift=q, J=0)(x)[1] is None


def test_size_table(fa):
    """ops.dtcwt_sizes: per level the (padded input, lowpass, bandpass) sides, against the restatement's shapes."""
    b = bufs("a")
    for H, W, J in ((16, 24, 3), (13, 18, 3), (4, 4, 3), (40, 36, 2), (30, 7, 4)):
        yl, yh = forward_levels(torch.zeros(1, 1, H, W, dtype=torch.float64), b, "symmetric", J)
        t = fa.ops.dtcwt_sizes(H, W, J)
        assert len(t) == J and t[-1][1] == tuple(yl.shape[2:])
        assert [s[2] for s in t] == [tuple(h.shape[3:5]) for h in yh]
        assert t[0][0] == (H + H % 2, W + W % 2) and all(s[0][0] % 4 == 0 and s[0][1] % 4 == 0 for s in t[1:])


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    (fb, fq), (ib, iq) = tuples("a")
    x = torch.zeros(1, 1, 8, 8)
    ops = fa.ops
    o3, o5, e4, e10 = [0.25, 0.5, 0.25], [0.1] * 5, [0.25] * 4, [0.1] * 10
    with pytest.raises(ValueError, match="odd"):
        ops.dtcwt_fwd_j1(x, e4, o3, False, 2, -1, 1)
    with pytest.raises(ValueError, match="odd"):
        ops.dtcwt_fwd_j1(x, o3, [0.1] * 21, False, 2, -1, 1)
    with pytest.raises(ValueError, match="odd"):
        ops.dtcwt_inv_j1(x, None, [1.0], o3, 2, -1, 1)
    with pytest.raises(ValueError, match="even"):
        ops.dtcwt_fwd_j2(x, *([[0.1] * 22] * 4), False, 2, -1)
    with pytest.raises(ValueError, match="even"):
        ops.dtcwt_fwd_j2(x, *([o5] * 4), False, 2, -1)
    with pytest.raises(ValueError, match="same length"):
        ops.dtcwt_fwd_j2(x, e10, e10, e10, e4, False, 2, -1)
    with pytest.raises(ValueError, match="same length"):
        ops.dtcwt_inv_j2(x, None, e10, e4, e10, e10, 2, -1)
    with pytest.raises(ValueError, match="even"):
        fa.DTCWTForward(biort=fb, qshift=[[0.1] * 32] * 4)
    with pytest.raises(ValueError, match="odd"):
        fa.DTCWTInverse(biort=(e4, o3), qshift=iq)
    with pytest.raises(ValueError, match="4-tuple"):
        fa.DTCWTForward(biort=fb, qshift=fq[:3])
    with pytest.raises(ValueError, match="2-tuple"):
        fa.DTCWTForward(biort=fb + fb, qshift=fq)
    with pytest.raises(ValueError, match="float32"):
        ops.dtcwt_fwd_j1(x.double(), o5, o3, False, 2, -1, 1)
    with pytest.raises(ValueError, match="device"):
        ops.dtcwt_fwd_j1(x, o5, o3, False, 2, -1, 1)
    with pytest.raises(ValueError, match="multiple of 2"):
        ops.dtcwt_fwd_j1(torch.zeros(1, 1, 7, 8), o5, o3, False, 2, -1, 1)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.dtcwt_fwd_j2(torch.zeros(1, 1, 8, 6), e10, e10, e10, e10, False, 2, -1)
    with pytest.raises(ValueError, match="multiple of 2"):
        ops.dtcwt_inv_j2(torch.zeros(1, 1, 3, 4), None, e10, e10, e10, e10, 2, -1)
    with pytest.raises(ValueError, match="6 orientations"):
        ops.dtcwt_inv_j1(x, torch.zeros(1, 1, 5, 4, 4, 2), o5, o3, 2, -1, 1)
    with pytest.raises(ValueError, match="real and imaginary"):
        ops.dtcwt_inv_j1(x, torch.zeros(1, 1, 6, 4, 4, 3), o5, o3, 2, -1, 1)
    with pytest.raises(ValueError, match="6 dimensions"):
        ops.dtcwt_inv_j1(x, torch.zeros(1, 6, 4, 4, 2), o5, o3, 2, -1, 1)
    with pytest.raises(ValueError, match="twice"):
        ops.dtcwt_inv_j1(x, torch.zeros(1, 1, 6, 3, 4, 2), o5, o3, 2, -1, 1)
    with pytest.raises(ValueError, match="twice"):
        ops.dtcwt_inv_j2(x, torch.zeros(1, 1, 6, 4, 3, 2), e10, e10, e10, e10, 2, -1)
    with pytest.raises(ValueError, match="both"):
        ops.dtcwt_inv_j1(None, None, o5, o3, 2, -1, 1)
    with pytest.raises(ValueError, match="4 dimensions"):
        fa.DTCWTForward(biort=fb, qshift=fq)(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="Unkown pad type"):
        fa.DTCWTForward(biort=fb, qshift=fq, mode="nope")(x)
