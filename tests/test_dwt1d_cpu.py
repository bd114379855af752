"""The 1-D filter-bank DWT without a GPU: the buffers ``DWT1DForward`` / ``DWT1DInverse`` register, the errors they raise before
any kernel entry point, the length tables, and a float64 restatement of one analysis and one synthesis level -- the formulas of
csrc/dwt1d.hip's header written with stock torch ops (index gathers, ``unfold``, strided adds), chained over the levels with the
reference's backward definitions and pinned to every array of the reference's fixtures (tests/golden/golden_dwt1d*.npz,
tools/gen_golden_dwt1d.py) at relative L2 <= 1e-6, a few fp32 ulp of the reference, the bar at which the 2-D restatement is
pinned to its fixtures.  tests/test_gpu_dwt1d.py measures the kernels against this restatement.

Two fixture cases, 'reflect' at the minimum length L/2 + 1 (db2 at 3, db4 at 5), hold no arrays: the reference itself raises
there (its reflect padding goes through ``F.pad``, which wants the pad below the length), so nothing pins the restatement for
them; it keeps folding about 0 and n - 1 as often as the position asks, and so do the kernels."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("golden_dwt1d.npz", "golden_dwt1d_j3_db2.npz", "golden_dwt1d_j3_db4.npz")
MODES = ("zero", "symmetric", "reflect", "periodic", "periodization")
BANK_ORDER = {"db2": 2, "db4": 4, "db8": 8}


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def source_index(j, n, L, mode):
    """Where position j of the extended signal reads from (numpy int array; -1 = a zero)."""
    j = np.asarray(j)
    if mode == "zero":
        return np.where((j >= 0) & (j < n), j, -1)
    if mode == "symmetric":                     # ... x1 x0 | x0 x1 ... xn-1 | xn-1 ...
        m = np.mod(j, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if mode == "reflect":                       # ... x2 x1 | x0 x1 ... xn-1 | xn-2 ...
        m = np.mod(j, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    if mode == "periodic":
        return np.mod(j, n)
    if mode == "periodization":                 # extend an odd length by its last sample, shift by L/2, one period either side
        ne = n + (n & 1)
        m = np.minimum(np.mod(np.mod(j, ne) + L // 2, ne), n - 1)
        return np.where((j >= -ne) & (j < ne), m, -1)
    raise ValueError(mode)


def out_size(n, L, mode):
    return (n + 1) // 2 if mode == "periodization" else (n + L - 1) // 2


def analysis(x, h0, h1, mode):
    """One level along the last dimension: out[i] = sum_k h[k] xe[2 i + k - base]; h0 / h1 are the registered (correlation) taps."""
    n, L = x.shape[-1], h0.numel()
    O = out_size(n, L, mode)
    base = L - 1 if mode == "periodization" else (2 * (O - 1) - n + L) // 2
    src = source_index(np.arange(2 * (O - 1) + L) - base, n, L, mode)
    xe = x.index_select(-1, torch.from_numpy(np.maximum(src, 0)).long()) * torch.from_numpy(src >= 0).to(x.dtype)
    win = xe.unfold(-1, L, 2)
    return (win * h0.reshape(-1).to(x.dtype)).sum(-1), (win * h1.reshape(-1).to(x.dtype)).sum(-1)


def synthesis(lo, hi, g0, g1, mode):
    """One level: full[2 i + k] += lo[i] g0[k] + hi[i] g1[k]; trimmed by L - 2 at the front, or, for periodization, wrapped once
    onto its first L - 2 samples and rolled by L/2 - 1.  ``hi`` None = zeros."""
    if hi is None:
        hi = torch.zeros_like(lo)
    n, L = lo.shape[-1], g0.numel()
    g0, g1 = g0.reshape(-1).to(lo.dtype), g1.reshape(-1).to(lo.dtype)
    full = lo.new_zeros(lo.shape[:-1] + (2 * n + L - 2,))
    for k in range(L):
        full[..., k:k + 2 * n:2] += lo * g0[k] + hi * g1[k]
    if mode == "periodization":
        head = full[..., :L - 2] + full[..., 2 * n:2 * n + L - 2]
        full = torch.cat((head, full[..., L - 2:]), dim=-1)[..., :2 * n]
        return torch.roll(full, shifts=-(L // 2 - 1), dims=-1)
    return full[..., L - 2:2 * n]


def forward_levels(x, h0, h1, mode, J):
    yh, lo = [], x
    for _ in range(J):
        lo, h = analysis(lo, h0, h1, mode)
        yh.append(h)
    return lo, yh


def forward_grad(lengths, cot_yl, cot_yh, h0, h1, mode):
    """The reference's DWT1DForward backward: per level the synthesis bank on the ANALYSIS buffers, cropped to the level's input
    length ``lengths[j]``."""
    g = cot_yl
    for j in reversed(range(len(cot_yh))):
        g = synthesis(g, cot_yh[j], h0, h1, mode)[..., :lengths[j]]
    return g


def inverse_levels(yl, yh, g0, g1, mode, trims=None):
    lo = yl
    for h in yh[::-1]:
        trim = 0
        if h is not None and lo.shape[-1] > h.shape[-1]:
            lo, trim = lo[..., :-1], 1
        if trims is not None:
            trims.append(trim)
        lo = synthesis(lo, h, g0, g1, mode)
    return lo


def inverse_grads(cot, trims, g0, g1, mode):
    """The reference's DWT1DInverse backward: per level the analysis bank on the SYNTHESIS buffers with the mode's padding; a
    sample dropped on the way up comes back as a zero.  -> (d yl, d yh[0])"""
    g, first_high = cot, None
    for j, trim in enumerate(reversed(trims)):
        g, h = analysis(g, g0, g1, mode)
        if j == 0:
            first_high = h
        g = torch.nn.functional.pad(g, (0, trim))
    return g, first_high


def restate(x, bufs, mode, J, cots, coeffs, cot_inv, dtype, none_level=True):
    """Every array of a case from the restatement in ``dtype``, returned as float64.  bufs = (h0, h1, g0, g1); cots = [cot_yl,
    cot_yh0 ..] or None (outputs only); coeffs = (yl, [yh]) the inverse runs on; ``none_level``: also the inverse with the coarsest
    level set to None."""
    h0, h1, g0, g1 = (b.to(dtype) for b in bufs)
    J = int(J)
    lengths, n = [], x.shape[-1]
    for _ in range(J):
        lengths.append(n)
        n = out_size(n, h0.numel(), mode)
    yl, yh = forward_levels(x.to(dtype), h0, h1, mode, J)
    out = {"yl": yl}
    for j, h in enumerate(yh):
        out["yh%d" % j] = h
    if cots is not None:
        out["xgrad"] = forward_grad(lengths, cots[0].to(dtype), [c.to(dtype) for c in cots[1:]], h0, h1, mode)
        cl, ch = coeffs[0].to(dtype), [h.to(dtype) for h in coeffs[1]]
        trims = []
        out["inv"] = inverse_levels(cl, ch, g0, g1, mode, trims)
        out["inv_gyl"], out["inv_gyh0"] = inverse_grads(cot_inv.to(dtype), trims, g0, g1, mode)
        if none_level:
            out["inv_none"] = inverse_levels(cl, ch[:-1] + [None], g0, g1, mode)
    return {k: v.double() for k, v in out.items()}


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
    """[(case id, bank, mode, J, shape)] of every case, those the reference refuses included."""
    out = []
    for k in sorted(gold()):
        if k.endswith("/yl") or k.endswith("/reference_refuses"):
            cid = k.rsplit("/", 1)[0]
            bank, mode, J, shape = cid.split("_")
            out.append((cid, bank, mode, int(J[1:]), tuple(int(v) for v in shape.split("x"))))
    return out


def decode(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5))


def buffers(bank):
    return tuple(torch.from_numpy(gold()["buf_%s_%s" % (bank, n)]).double() for n in ("h0", "h1", "g0", "g1"))


def refused(cid):
    return cid + "/reference_refuses" in gold()


def fixture_inputs(case):
    """(x, cots, coeffs, cot_inv) of a fixture case; the inverse runs on the FIXTURE's coefficients (fp32 values), as the
    reference's and the kernels' do.  A refused case has the input only."""
    cid, bank, mode, J, shape = case
    g = gold()
    x = torch.from_numpy(g["x_%dx%dx%d" % shape])
    if refused(cid):
        return x, None, None, None
    cots = [decode(g[cid + "/cot_yl"])] + [decode(g[cid + "/cot_yh%d" % j]) for j in range(J)]
    coeffs = (torch.from_numpy(g[cid + "/yl"]), [torch.from_numpy(g[cid + "/yh%d" % j]) for j in range(J)])
    return x, cots, coeffs, decode(g[cid + "/cot_inv"])


def restate_case(case, dtype=torch.float64):
    x, cots, coeffs, cot_inv = fixture_inputs(case)
    return restate(x, buffers(case[1]), case[2], case[3], cots, coeffs, cot_inv, dtype)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ----------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_restatement_matches_the_fixture(case):
    cid, bank, mode, J, shape = case
    g = gold()
    if refused(cid):
        assert mode == "reflect" and J == 1 and shape[2] == BANK_ORDER[bank] + 1, cid
        assert not any(k.startswith(cid + "/") and not k.endswith("/reference_refuses") for k in g)
        return
    got = restate_case(case)
    assert len(got) == J + 6
    for k, v in got.items():
        want = torch.from_numpy(g[cid + "/" + k])
        assert tuple(v.shape) == tuple(want.shape), (cid, k, tuple(v.shape), tuple(want.shape))
        assert rel_l2(want, v) <= 1e-6, (cid, k, rel_l2(want, v))


def test_fixture_holds_the_cases_of_the_issue():
    cases = fixture_cases()
    have = {c[1:] for c in cases}
    for bank in ("db2", "db4"):
        for mode in MODES:
            for n in (16, 13, BANK_ORDER[bank] + 1):
                assert (bank, mode, 1, (2, 3, n)) in have
            for n in (64, 301):
                assert (bank, mode, 3, (2, 3, n)) in have
    assert len(cases) == 50
    assert sorted(c[0] for c in cases if refused(c[0])) == ["db2_reflect_J1_2x3x3", "db4_reflect_J1_2x3x5"]
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20


def test_modules_register_the_reference_buffers(fa):
    d2, d4 = fa.daubechies(2), fa.daubechies(4)
    forms = {"db4": (d4, d4), "db2": ((d2.dec_lo, d2.dec_hi), (np.array(d2.rec_lo), torch.tensor(d2.rec_hi)))}
    for bank, (wf, wi) in forms.items():
        fwd, inv = fa.DWT1DForward(J=2, wave=wf, mode="symmetric"), fa.DWT1DInverse(wave=wi, mode="symmetric")
        assert isinstance(fwd, fa.wavelets._TapModule) and isinstance(inv, fa.wavelets._TapModule)
        assert [n for n, _ in fwd.named_buffers()] == ["h0", "h1"] and [n for n, _ in inv.named_buffers()] == ["g0", "g1"]
        w = fa.daubechies(BANK_ORDER[bank])
        L = 2 * BANK_ORDER[bank]
        for mod, name, taps in ((fwd, "h0", w.dec_lo[::-1]), (fwd, "h1", w.dec_hi[::-1]), (inv, "g0", w.rec_lo), (inv, "g1", w.rec_hi)):
            got, want = getattr(mod, name), gold()["buf_%s_%s" % (bank, name)]
            assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, L) == want.shape, (bank, name)
            np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=0)
            np.testing.assert_allclose(got.numpy().ravel(), np.array(taps, dtype=np.float32), rtol=1e-6, atol=0)
            assert mod._taps[name] == tuple(got.reshape(-1).tolist())


def test_state_dict_round_trip(fa):
    d2, d4 = fa.daubechies(2), fa.daubechies(4)
    src, inv_src = fa.DWT1DForward(J=2, wave=d4), fa.DWT1DInverse(wave=d4)
    dst, inv_dst = fa.DWT1DForward(J=2, wave=(d4.dec_hi, d4.dec_lo)), fa.DWT1DInverse(wave=(d4.rec_hi, d4.rec_lo))
    assert sorted(src.state_dict()) == ["h0", "h1"] and sorted(inv_src.state_dict()) == ["g0", "g1"]
    dst.load_state_dict(src.state_dict(), strict=True)
    inv_dst.load_state_dict(inv_src.state_dict(), strict=True)
    for a, b, names in ((src, dst, ("h0", "h1")), (inv_src, inv_dst, ("g0", "g1"))):
        for n in names:
            assert torch.equal(getattr(a, n), getattr(b, n))
            assert b._taps[n] == a._taps[n]                         # the loaded taps are the host record
    with pytest.raises(RuntimeError):
        fa.DWT1DForward(wave=d2).load_state_dict(src.state_dict())  # 4 taps against 8


def test_haar_is_daubechies_1_and_other_names_stay_unresolved(fa):
    for a, b in ((fa.DWT1DForward(wave="haar"), fa.DWT1DForward(wave=fa.daubechies(1))), (fa.DWT1DForward(wave="db1"), fa.DWT1DForward()),
                 (fa.DWT1DInverse(wave="haar"), fa.DWT1DInverse(wave=fa.daubechies(1)))):
        assert a._taps == b._taps and all(len(v) == 2 for v in a._taps.values())
    s = 2.0 ** -0.5
    np.testing.assert_allclose(fa.DWT1DForward().h1.numpy().ravel(), [s, -s], rtol=1e-6)       # dec_hi [-s, s] reversed
    np.testing.assert_allclose(fa.DWT1DInverse().g1.numpy().ravel(), [s, -s], rtol=1e-6)
    for name in ("db4", "sym4"):
        with pytest.raises(NotImplementedError, match="tuple"):
            fa.DWT1DForward(wave=name)
        with pytest.raises(NotImplementedError):
            fa.DWT1DInverse(wave=name)


def test_length_tables(fa):
    """Odd and even lengths in both length rules: (n + L - 1) // 2, and (n + 1) // 2 for periodization."""
    ops = fa.ops
    assert ops.dwt1d_lengths(301, 8, 1, 3) == [301, 154, 80, 43]
    assert ops.dwt1d_lengths(64, 8, 0, 3) == [64, 35, 21, 14]
    assert ops.dwt1d_lengths(301, 8, 2, 3) == [301, 151, 76, 38]
    assert ops.dwt1d_lengths(64, 4, 2, 3) == [64, 32, 16, 8]
    assert ops.dwt1d_lengths(9, 16, 4, 2) == [9, 12, 13]            # below L - 1 a level grows
    for mode_name, mode in (("symmetric", 1), ("periodization", 2)):
        for n in (301, 64, 13):
            lens = ops.dwt1d_lengths(n, 8, mode, 3)
            assert lens[1:] == [out_size(m, 8, mode_name) for m in lens[:-1]]
    # the inverse: a result is 2 c - L + 2 long (2 c for periodization); one surplus sample of the running lowpass is dropped
    assert ops.dwt1d_inverse_lengths(43, [154, 80, 43], 8, 1) == ([154, 80, 43], [302, 154, 80])
    assert ops.dwt1d_inverse_lengths(38, [151, 76, 38], 8, 2) == ([151, 76, 38], [302, 152, 76])
    assert ops.dwt1d_inverse_lengths(44, [154, 80, 43], 8, 1) == ([154, 80, 43], [302, 154, 80])       # the coarsest lowpass one too long
    assert ops.dwt1d_inverse_lengths(43, [154, None, 43], 8, 1) == ([154, 80, 43], [302, 154, 80])
    assert ops.dwt1d_inverse_lengths(14, [35, 21, 14], 8, 0) == ([35, 21, 14], [64, 36, 22])           # 22 -> 21 and 36 -> 35 dropped
    with pytest.raises(ValueError, match="does not belong"):
        ops.dwt1d_inverse_lengths(45, [154, 80, 43], 8, 1)
    with pytest.raises(ValueError, match="does not belong"):
        ops.dwt1d_inverse_lengths(43, [155, 80, 43], 8, 1)
    with pytest.raises(ValueError, match="minimum"):
        ops.dwt1d_inverse_lengths(3, [3], 8, 1)


def test_fused_limit_is_the_library_s(fa):
    assert fa.DWT1D_FUSED_MAX == fa.ops.DWT1D_FUSED_MAX == fa._lib.load().faoctasr_dwt1d_fused_max() == 8192


def test_every_value_error_is_raised_before_any_entry_point(fa, monkeypatch):
    calls = []
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: calls.append(name))
    d4 = fa.daubechies(4)
    with pytest.raises(ValueError):
        fa.DWT1DForward(wave=(d4.dec_lo[:7], d4.dec_hi[:7]))                 # odd tap count
    with pytest.raises(ValueError):
        fa.DWT1DInverse(wave=(d4.rec_lo[:5], d4.rec_hi[:5]))
    with pytest.raises(ValueError):
        fa.DWT1DForward(wave=([0.1] * 18, [0.1] * 18))                       # 18 taps
    with pytest.raises(ValueError):
        fa.DWT1DForward(wave=(d4.dec_lo, d4.dec_hi[:6]))                     # unequal pair
    with pytest.raises(ValueError):
        fa.DWT1DForward(wave=(d4.dec_lo, d4.dec_hi, d4.dec_lo, d4.dec_hi))   # the 2-D four-sequence form
    for mode in MODES:
        fwd, inv = fa.DWT1DForward(J=1, wave=d4, mode=mode), fa.DWT1DInverse(wave=d4, mode=mode)
        with pytest.raises(ValueError, match="minimum length"):
            fwd(torch.zeros(1, 1, 4))                                        # L/2 samples
        with pytest.raises(ValueError, match="minimum length"):              # 9 -> 8 (5 for periodization) -> .. a later level too short
            fa.DWT1DForward(J=8, wave=d4, mode="periodization")(torch.zeros(1, 1, 9))
        for bad in (torch.zeros(1, 16), torch.zeros(1, 1, 1, 16)):
            with pytest.raises(ValueError, match="3d"):
                fwd(bad)
            with pytest.raises(ValueError, match="3d"):
                inv((bad, [bad]))
        with pytest.raises(ValueError, match="does not belong"):
            inv((torch.zeros(1, 1, 12), [torch.zeros(1, 1, 10)]))            # two samples too long
        with pytest.raises(ValueError, match="do not belong"):
            inv((torch.zeros(1, 2, 10), [torch.zeros(1, 1, 10)]))
        with pytest.raises(ValueError, match="minimum"):
            inv((torch.zeros(1, 1, 1), [torch.zeros(1, 1, 1)]))
    with pytest.raises(ValueError, match="levels"):
        fa.DWT1DForward(J=9, wave=d4)(torch.zeros(1, 1, 4096))
    with pytest.raises(ValueError, match="levels"):
        fa.ops.dwt1d_analysis(torch.zeros(1, 1, 64), d4.dec_lo, d4.dec_hi, 0, J=0)
    with pytest.raises(ValueError, match="DWT1D_FUSED_MAX"):
        fa.ops.dwt1d_analysis(torch.zeros(1, 1, fa.DWT1D_FUSED_MAX + 1), d4.dec_lo, d4.dec_hi, 0, J=1, fused=True)
    with pytest.raises(ValueError):
        fa.ops.afb1d(torch.zeros(1, 1, 64), d4.dec_lo[:7], d4.dec_hi[:7], 0)
    with pytest.raises(ValueError):
        fa.AFB1D.apply(torch.zeros(1, 1, 4), fa.DWT1DForward(wave=d4).h0, fa.DWT1DForward(wave=d4).h1, 0)
    with pytest.raises(ValueError):
        fa.SFB1D.apply(torch.zeros(1, 1, 12), torch.zeros(1, 1, 10), fa.DWT1DInverse(wave=d4).g0, fa.DWT1DInverse(wave=d4).g1, 0)
    with pytest.raises(ValueError, match="Unkown pad type"):
        fa.DWT1DForward(wave=d4, mode="mirror")(torch.zeros(1, 1, 16))
    for mode in ("constant", "replicate"):
        with pytest.raises(NotImplementedError):
            fa.DWT1DForward(wave=d4, mode=mode)(torch.zeros(1, 1, 16))
    assert calls == []
    with pytest.raises(fa.KernelError):                                      # and a host tensor is refused, not computed
        fa.DWT1DForward(wave=d4)(torch.zeros(1, 1, 16))
    assert calls == []
