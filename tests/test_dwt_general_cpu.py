"""The general filter-bank DWT without a GPU: the computed Daubechies taps, the buffers the modules register, the errors they
raise, and a float64 restatement of the five padding modes' analysis and synthesis banks -- written here with stock torch ops
(index gathers, ``unfold``, strided adds), pinned to every array of the reference's fixtures (tests/golden/golden_dwt*.npz,
tools/gen_golden_dwt.py) at relative L2 <= 1e-6, a few fp32 ulp of the reference.  tests/test_gpu_dwt_general.py measures the
kernels against this restatement.

One fixture case, db4 / 'reflect' / 9x6, holds no arrays: the reference itself raises there (its reflect padding goes through
``F.pad``, which wants the pad of L - 2 a side below the image side), so nothing pins the restatement for it; the restatement
keeps folding about 0 and N - 1 (numpy's 'reflect'), and so do the kernels.

``daubechies(1)`` is the symmetric Haar pair, whose first tap carries exactly half the energy; "more than half" is asserted
from N = 2 on."""
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("golden_dwt.npz", "golden_dwt_a_mixed.npz", "golden_dwt_b_symmetric.npz", "golden_dwt_b_periodization.npz",
         "golden_dwt_c_symmetric.npz", "golden_dwt_c_reflect.npz", "golden_dwt_c_periodization.npz")
MODES = ("zero", "symmetric", "reflect", "periodic", "periodization")
A_BUFS = ("h0_col", "h1_col", "h0_row", "h1_row")
S_BUFS = ("g0_col", "g1_col", "g0_row", "g1_row")


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def _source_index(j, N, L, mode):
    """Where position j of the extended signal reads from (numpy int array; -1 = a zero)."""
    j = np.asarray(j)
    if mode == "zero":
        return np.where((j >= 0) & (j < N), j, -1)
    if mode == "symmetric":                     # ... x1 x0 | x0 x1 ... xN-1 | xN-1 ...
        m = np.mod(j, 2 * N)
        return np.where(m < N, m, 2 * N - 1 - m)
    if mode == "reflect":                       # ... x2 x1 | x0 x1 ... xN-1 | xN-2 ...
        m = np.mod(j, 2 * N - 2)
        return np.where(m < N, m, 2 * N - 2 - m)
    if mode == "periodic":
        return np.mod(j, N)
    if mode == "periodization":                 # extend an odd side by its last sample, shift by L/2, one period either side, zeros beyond
        Ne = N + (N & 1)
        m = np.minimum(np.mod(np.mod(j, Ne) + L // 2, Ne), N - 1)
        return np.where((j >= -Ne) & (j < Ne), m, -1)
    raise ValueError(mode)


def out_size(N, L, mode):
    return (N + 1) // 2 if mode == "periodization" else (N + L - 1) // 2


def analysis_1d(x, lo, hi, mode, dim):
    """out[i] = sum_k h[k] xe[2 i + k - base] along ``dim``; lo / hi are the registered (correlation) taps.  -> (low, high)"""
    N, L = x.shape[dim], lo.numel()
    O = out_size(N, L, mode)
    base = L - 1 if mode == "periodization" else (2 * (O - 1) - N + L) // 2
    src = _source_index(np.arange(2 * (O - 1) + L) - base, N, L, mode)
    xe = x.index_select(dim, torch.from_numpy(np.maximum(src, 0)).long())
    shape = [1] * x.dim()
    shape[dim] = -1
    xe = xe * torch.from_numpy((src >= 0)).to(x.dtype).reshape(shape)
    win = xe.unfold(dim, L, 2)                                  # (..., O, ..., L)
    return (win * lo.reshape(-1).to(x.dtype)).sum(-1), (win * hi.reshape(-1).to(x.dtype)).sum(-1)


def analysis_2d(x, bufs, mode):
    """One level.  bufs = (w lo, w hi, h lo, h hi): the first pair filters along W -- the modules hand their *_col buffers there."""
    lo, hi = analysis_1d(x, bufs[0], bufs[1], mode, 3)
    ll, lh = analysis_1d(lo, bufs[2], bufs[3], mode, 2)
    hl, hh = analysis_1d(hi, bufs[2], bufs[3], mode, 2)
    return ll, torch.stack((lh, hl, hh), dim=2)


def synthesis_1d(lo, hi, g0, g1, mode, dim):
    """The transposed stride-2 bank: full[2 i + k] += lo[i] g0[k] + hi[i] g1[k]; trimmed by L - 2 at the front, or, for
    periodization, wrapped once onto its first L - 2 samples and rolled by L/2 - 1."""
    lo, hi = lo.movedim(dim, -1), hi.movedim(dim, -1)
    n, L = lo.shape[-1], g0.numel()
    g0, g1 = g0.reshape(-1).to(lo.dtype), g1.reshape(-1).to(lo.dtype)
    full = lo.new_zeros(lo.shape[:-1] + (2 * n + L - 2,))
    for k in range(L):
        full[..., k:k + 2 * n:2] += lo * g0[k] + hi * g1[k]
    if mode == "periodization":
        head = full[..., :L - 2] + full[..., 2 * n:2 * n + L - 2]
        full = torch.cat((head, full[..., L - 2:]), dim=-1)[..., :2 * n]
        y = torch.roll(full, shifts=-(L // 2 - 1), dims=-1)
    else:
        y = full[..., L - 2:2 * n]
    return y.movedim(-1, dim)


def synthesis_2d(ll, highs, bufs, mode):
    lh, hl, hh = (torch.zeros_like(ll),) * 3 if highs is None else torch.unbind(highs, dim=2)
    if ll is None:
        ll = torch.zeros_like(lh)
    lo = synthesis_1d(ll, lh, bufs[2], bufs[3], mode, 2)
    hi = synthesis_1d(hl, hh, bufs[2], bufs[3], mode, 2)
    return synthesis_1d(lo, hi, bufs[0], bufs[1], mode, 3)


def forward_levels(x, bufs, mode, J):
    yh, ll = [], x
    for _ in range(J):
        ll, h = analysis_2d(ll, bufs, mode)
        yh.append(h)
    return ll, yh


def forward_grad(shapes, cot_yl, cot_yh, bufs, mode):
    """The reference's DWTForward backward: per level the synthesis bank on the ANALYSIS buffers, cropped to the level's input
    size; ``shapes[j]`` is the (H, W) that level j transformed."""
    g = cot_yl
    for j in reversed(range(len(cot_yh))):
        g = synthesis_2d(g, cot_yh[j], bufs, mode)[..., :shapes[j][0], :shapes[j][1]]
    return g


def inverse_levels(yl, yh, bufs, mode, trims=None):
    ll = yl
    for h in yh[::-1]:
        trim = [0, 0]
        if h is not None:
            if ll.shape[-2] > h.shape[-2]:
                ll, trim[0] = ll[..., :-1, :], 1
            if ll.shape[-1] > h.shape[-1]:
                ll, trim[1] = ll[..., :-1], 1
        if trims is not None:
            trims.append(trim)
        ll = synthesis_2d(ll, h, bufs, mode)
    return ll


def inverse_grads(cot, trims, bufs, mode):
    """The reference's DWTInverse backward: per level the analysis bank on the SYNTHESIS buffers with the mode's padding; a row
    or column dropped on the way up comes back as zeros.  -> (d yl, d yh[0])"""
    g, first_high = cot, None
    for j, trim in enumerate(reversed(trims)):
        g, h = analysis_2d(g, bufs, mode)
        if j == 0:
            first_high = h
        g = torch.nn.functional.pad(g, (0, trim[1], 0, trim[0]))
    return g, first_high


# ----------------------------------------------------------------------------------------
# the fixtures
# ----------------------------------------------------------------------------------------
_gold = {}


def gold():
    if not _gold:
        for f in FILES:
            with np.load(os.path.join(GOLDEN, f)) as z:
                for k in z.files:
                    _gold[k] = z[k]
    return _gold


def fixture_cases():
    """[(case id, bank, mode, J, shape)] of every case, the one the reference refuses included."""
    out = []
    for k in sorted(gold()):
        if k.endswith("/yl") or k.endswith("/reference_refuses"):
            cid = k.rsplit("/", 1)[0]
            bank, mode, J, shape = cid.split("_")
            out.append((cid, bank, mode, int(J[1:]), tuple(int(v) for v in shape.split("x"))))
    return out


def decode(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5))


def buffers(bank, names, dtype=torch.float64):
    return tuple(torch.from_numpy(gold()["buf_%s_%s" % (bank, n)]).to(dtype) for n in names)


def restate_case(cid, bank, mode, J, shape, dtype=torch.float64, banks=None):
    """Every array a fixture case holds, from the restatement in ``dtype`` (as float64).  ``banks`` overrides the fixture's
    buffers (off-fixture shapes): (analysis buffers, synthesis buffers)."""
    g = gold()
    ab, sb = banks if banks is not None else (buffers(bank, A_BUFS), buffers(bank, S_BUFS))
    ab, sb = [b.to(dtype) for b in ab], [b.to(dtype) for b in sb]
    x = torch.from_numpy(g["x_%dx%dx%dx%d" % shape]).to(dtype)
    out = {}
    shapes, ll = [], x
    for _ in range(J):
        shapes.append(ll.shape[-2:])
        ll = analysis_2d(ll, ab, mode)[0]
    yl, yh = forward_levels(x, ab, mode, J)
    out["yl"] = yl
    for j, h in enumerate(yh):
        out["yh%d" % j] = h
    if cid + "/cot_yl" in g:
        out["xgrad"] = forward_grad(shapes, decode(g[cid + "/cot_yl"]).to(dtype), [decode(g[cid + "/cot_yh%d" % j]).to(dtype) for j in range(J)], ab, mode)
        # the inverse runs on the FIXTURE's coefficients (fp32 values), as the reference's and the kernels' do
        cl = torch.from_numpy(g[cid + "/yl"]).to(dtype)
        ch = [torch.from_numpy(g[cid + "/yh%d" % j]).to(dtype) for j in range(J)]
        trims = []
        out["inv"] = inverse_levels(cl, ch, sb, mode, trims)
        out["inv_gyl"], out["inv_gyh0"] = inverse_grads(decode(g[cid + "/cot_inv"]).to(dtype), trims, sb, mode)
        out["inv_none"] = inverse_levels(cl, ch[:-1] + [None], sb, mode)
    return {k: v.double() for k, v in out.items()}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ----------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


@pytest.mark.parametrize("N", range(1, 9))
def test_daubechies_taps(fa, N):
    w = fa.daubechies(N)
    L = 2 * N
    dec_lo, dec_hi, rec_lo, rec_hi = (np.array(t, dtype=np.float64) for t in (w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi))
    assert len(dec_lo) == len(dec_hi) == len(rec_lo) == len(rec_hi) == L
    assert abs(dec_lo.sum() - math.sqrt(2.0)) <= 1e-12
    for m in range(N):
        assert abs(np.dot(dec_lo[2 * m:], dec_lo[:L - 2 * m]) - (1.0 if m == 0 else 0.0)) <= 1e-12, m
        assert abs(np.dot(dec_hi[2 * m:], dec_lo[:L - 2 * m])) <= 1e-12, m
    for p in range(N):
        assert abs(np.sum(dec_hi * np.arange(L, dtype=np.float64) ** p)) <= 1e-8 * L ** N, p
    assert np.array_equal(dec_lo, rec_lo[::-1]) and np.array_equal(rec_hi, dec_hi[::-1])
    assert np.array_equal(dec_hi, np.array([(-1.0) ** (k + 1) * dec_lo[L - 1 - k] for k in range(L)]))
    energy, front = float((rec_lo ** 2).sum()), float((rec_lo[:N] ** 2).sum())
    if N == 1:
        assert abs(front - 0.5 * energy) <= 1e-15          # Haar: symmetric
    else:
        assert front > 0.5 * energy                        # minimum phase
    if N == 2:
        s3 = math.sqrt(3.0)
        assert np.abs(dec_lo - np.array([1 - s3, 3 - s3, 3 + s3, 1 + s3]) / (4 * math.sqrt(2.0))).max() <= 1e-15
    with pytest.raises(ValueError):
        fa.daubechies(9)


def test_modules_register_the_reference_buffers(fa):
    d2, d4 = fa.daubechies(2), fa.daubechies(4)
    forms = {
        "db4": (d4, d4),
        "db2": ((d2.dec_lo, d2.dec_hi), (d2.rec_lo, d2.rec_hi)),
        "db2db4": ((d2.dec_lo, d2.dec_hi, d4.dec_lo, d4.dec_hi), (np.array(d2.rec_lo), torch.tensor(d2.rec_hi), d4.rec_lo, d4.rec_hi)),
    }
    for bank, (wf, wi) in forms.items():
        fwd, inv = fa.DWTForward(J=2, wave=wf, mode="symmetric"), fa.DWTInverse(wave=wi, mode="symmetric")
        assert sorted(n for n, _ in fwd.named_buffers()) == sorted(A_BUFS) and sorted(n for n, _ in inv.named_buffers()) == sorted(S_BUFS)
        for mod, names in ((fwd, A_BUFS), (inv, S_BUFS)):
            for n in names:
                want = gold()["buf_%s_%s" % (bank, n)]
                got = getattr(mod, n)
                assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, (bank, n)
                np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=0)
    L = len(d4.dec_lo)
    assert tuple(fwd.h0_col.shape) == (1, 1, 4, 1) and tuple(fwd.h0_row.shape) == (1, 1, 1, L)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_restatement_matches_the_fixture(case):
    cid, bank, mode, J, shape = case
    g = gold()
    if cid + "/reference_refuses" in g:
        assert (bank, mode, shape[2:]) == ("db4", "reflect", (9, 6))
        return
    got = restate_case(*case)
    assert len(got) == J + 6
    for k, v in got.items():
        want = torch.from_numpy(g[cid + "/" + k])
        assert tuple(v.shape) == tuple(want.shape), (cid, k, tuple(v.shape), tuple(want.shape))
        assert rel_l2(want, v) <= 1e-6, (cid, k, rel_l2(want, v))


def test_fixture_holds_the_cases_of_the_issue():
    cases = fixture_cases()
    a = [(c[1], c[2], c[4][2:]) for c in cases if c[3] == 1 and c[4][:2] == (2, 2)]
    for bank in ("db2", "db4", "db2db4"):
        for mode in MODES:
            for hw in ((16, 16), (13, 18), (5, 7) if bank == "db2" else (9, 6)):
                assert (bank, mode, hw) in a
    for mode in ("symmetric", "periodization"):
        assert any(c[1:] == ("db4", mode, 1, (1, 3, 70, 150)) for c in cases)
    for mode in ("symmetric", "reflect", "periodization"):
        for shape in ((2, 1, 64, 48), (2, 1, 45, 52)):
            assert any(c[1:] == ("db4", mode, 3, shape) for c in cases)
    assert len(cases) == 45 + 2 + 6 and sum(1 for c in cases if c[0] + "/reference_refuses" in gold()) == 1


def test_names_other_than_haar_stay_unresolved(fa):
    for name in ("db4", "db2", "sym4"):
        with pytest.raises(NotImplementedError, match="tuple"):
            fa.DWTForward(J=1, wave=name)
        with pytest.raises(NotImplementedError):
            fa.DWTInverse(wave=name)
    assert fa.DWTForward(J=1, wave="haar")._haar and fa.DWTForward(J=1, wave=fa.daubechies(1))._haar


def test_bad_banks_and_small_sides_raise_value_error(fa):
    d4 = fa.daubechies(4)
    with pytest.raises(ValueError):
        fa.DWTForward(wave=(d4.dec_lo[:7], d4.dec_hi[:7]))                   # odd L
    with pytest.raises(ValueError):
        fa.DWTInverse(wave=(d4.rec_lo[:5], d4.rec_hi[:5]))
    with pytest.raises(ValueError):
        fa.DWTForward(wave=([0.1] * 18, [0.1] * 18))                         # L = 18
    with pytest.raises(ValueError):
        fa.DWTForward(wave=(d4.dec_lo, d4.dec_hi, d4.dec_lo))                # three sequences
    for mode in MODES:
        fwd = fa.DWTForward(J=1, wave=d4, mode=mode)
        for shape in ((1, 1, 4, 16), (1, 1, 16, 4)):                         # a side of L/2: checked before anything is launched
            with pytest.raises(ValueError, match="minimum side"):
                fwd(torch.zeros(shape))
    for mode in ("constant", "replicate"):
        with pytest.raises(NotImplementedError):
            fa.DWTForward(J=1, wave=d4, mode=mode)(torch.zeros(1, 1, 16, 16))
