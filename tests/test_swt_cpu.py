"""The stationary wavelet transform without a GPU: a float64 restatement of the a-trous analysis, of its adjoint and of the periodic
inverse, written from their definitions with stock torch ops (index gathers for the analysis and the inverse, ``index_add_`` over
the extended domain for the adjoint), pinned to every array of the reference's fixtures (tests/golden/golden_swt*.npz,
tools/gen_golden_swt.py: ``afb2d_atrous`` level by level and autograd through it); the modules' buffers, aliases and errors; and
the two C entry points' declarations.  tests/test_gpu_swt.py measures the kernels against this restatement.

Per axis, with h the taps in wavelet order, L their count, d = 2^level and xe the mode's extension of x:
    analysis   out[i] = sum_k h[k] xe[i - k d + L d / 2]                                   (W pass first, then H)
    adjoint    dx[j]  = sum_{p : map(p) = j} sum_k h[k] dy0[p + k d - L d / 2]             p in [-(L d / 2 - d), N + L d / 2)
    inverse    y[m]   = 1/2 sum_k g0[k] lo[(m - k d + (L/2 - 1) d) mod N] + g1[k] hi[same]  (H first, then W; coarse to fine)

The pin: relative L2 <= 4 * 2^-23 between the fixture (fp32 results of fp32 convolutions) and the restatement in float64 on
the fixture's own fp32 tap buffers."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = ("zero", "symmetric", "reflect", "periodic")
FILES = ("golden_swt.npz",) + tuple("golden_swt_b_%s.npz" % m for m in MODES)
A_BUFS = ("h0_col", "h1_col", "h0_row", "h1_row")
S_BUFS = ("g0_col", "g1_col", "g0_row", "g1_row")
PIN = 4.0 * 2.0 ** -23


# ----------------------------------------------------------------------------------------
# the restatement.  A bank is (lo_h, hi_h, lo_w, hi_w): 1-D tensors in wavelet order, the pair that filters along H first.
# ----------------------------------------------------------------------------------------
def ext_index(p, N, mode):
    """Where position p of the extended signal reads from (numpy int array; -1 = a zero)."""
    p = np.asarray(p)
    if mode == "zero":
        return np.where((p >= 0) & (p < N), p, -1)
    if mode == "symmetric":
        m = np.mod(p, 2 * N)
        return np.where(m < N, m, 2 * N - 1 - m)
    if mode == "reflect":
        m = np.mod(p, 2 * N - 2)
        return np.where(m < N, m, 2 * N - 2 - m)
    if mode in ("periodic", "periodization", "per"):
        return np.mod(p, N)
    raise ValueError(mode)


def _take(x, dim, src):
    """x gathered along ``dim`` at ``src`` (numpy ints), zeros where src < 0."""
    shape = [1] * x.dim()
    shape[dim] = -1
    return x.index_select(dim, torch.from_numpy(np.maximum(src, 0)).long()) * torch.from_numpy(src >= 0).to(x.dtype).reshape(shape)


def analysis_1d(x, lo, hi, mode, d, dim):
    N, L = x.shape[dim], lo.numel()
    i = np.arange(N)
    a, b = torch.zeros_like(x), torch.zeros_like(x)
    for k in range(L):
        xe = _take(x, dim, ext_index(i - k * d + L * d // 2, N, mode))
        a, b = a + lo[k] * xe, b + hi[k] * xe
    return a, b


def analysis_2d(x, bank, mode, d):
    """(N, C, H, W) -> (N, C, 4, H, W): bands (W lo, H lo), (W lo, H hi), (W hi, H lo), (W hi, H hi)."""
    lo_h, hi_h, lo_w, hi_w = bank
    lo, hi = analysis_1d(x, lo_w, hi_w, mode, d, 3)
    ll, lh = analysis_1d(lo, lo_h, hi_h, mode, d, 2)
    hl, hh = analysis_1d(hi, lo_h, hi_h, mode, d, 2)
    return torch.stack((ll, lh, hl, hh), dim=2)


def adjoint_1d(c_lo, c_hi, lo, hi, mode, d, dim):
    N, L = c_lo.shape[dim], lo.numel()
    p = np.arange(-(L * d // 2 - d), N + L * d // 2)
    z = 0
    for k in range(L):
        e = p + k * d - L * d // 2
        src = np.where((e >= 0) & (e < N), e, -1)
        z = z + lo[k] * _take(c_lo, dim, src) + hi[k] * _take(c_hi, dim, src)
    dst = ext_index(p, N, mode)
    keep = np.nonzero(dst >= 0)[0]
    out = torch.zeros_like(c_lo)
    return out.index_add_(dim, torch.from_numpy(dst[keep]).long(), z.index_select(dim, torch.from_numpy(keep).long()))


def adjoint_2d(c, bank, mode, d):
    lo_h, hi_h, lo_w, hi_w = bank
    lo = adjoint_1d(c[:, :, 0], c[:, :, 1], lo_h, hi_h, mode, d, 2)
    hi = adjoint_1d(c[:, :, 2], c[:, :, 3], lo_h, hi_h, mode, d, 2)
    return adjoint_1d(lo, hi, lo_w, hi_w, mode, d, 3)


def inverse_1d(lo, hi, g0, g1, d, dim):
    N, L = lo.shape[dim], g0.numel()
    m = np.arange(N)
    y = torch.zeros_like(lo)
    for k in range(L):
        src = np.mod(m - k * d + (L // 2 - 1) * d, N)
        y = y + g0[k] * _take(lo, dim, src) + g1[k] * _take(hi, dim, src)
    return 0.5 * y


def inverse_2d(c, bank, d):
    g0_h, g1_h, g0_w, g1_w = bank
    lo = inverse_1d(c[:, :, 0], c[:, :, 1], g0_h, g1_h, d, 2)
    hi = inverse_1d(c[:, :, 2], c[:, :, 3], g0_h, g1_h, d, 2)
    return inverse_1d(lo, hi, g0_w, g1_w, d, 3)


def forward_levels(x, bank, mode, J):
    out, ll = [], x
    for j in range(J):
        y = analysis_2d(ll, bank, mode, 1 << j)
        out.append(y)
        ll = y[:, :, 0]
    return out


def forward_grad(cots, bank, mode):
    """x.grad for one cotangent per level: coarse to fine, a level's gradient joins band 0 of the next finer cotangent."""
    g = None
    for j in reversed(range(len(cots))):
        c = cots[j]
        if g is not None:
            c = c.clone()
            c[:, :, 0] += g
        g = adjoint_2d(c, bank, mode, 1 << j)
    return g


def inverse_levels(coeffs, bank):
    ll = coeffs[-1][:, :, 0]
    for j in reversed(range(len(coeffs))):
        ll = inverse_2d(torch.cat((ll.unsqueeze(2), coeffs[j][:, :, 1:]), dim=2), bank, 1 << j)
    return ll


def analysis_bank(bufs, dtype=torch.float64):
    """(h0_col, h1_col, h0_row, h1_row) buffers in the prep_filt_afb2d form -> (lo_h, hi_h, lo_w, hi_w) in wavelet order."""
    return tuple(torch.as_tensor(b).reshape(-1).flip(0).to(dtype) for b in bufs)


def synthesis_bank(bufs, dtype=torch.float64):
    return tuple(torch.as_tensor(b).reshape(-1).to(dtype) for b in bufs)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def decode(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65536.0) - np.float32(0.5))


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
    """[(case id, bank, mode, J, shape)]"""
    out = []
    for k in sorted(gold()):
        if k.endswith("/xgrad"):
            cid = k.rsplit("/", 1)[0]
            bank, mode, J, shape = cid.split("_")
            out.append((cid, bank, mode, int(J[1:]), tuple(int(v) for v in shape.split("x"))))
    return out


def fixture_bank(bank, dtype=torch.float64):
    return analysis_bank([gold()["buf_%s_%s" % (bank, n)] for n in A_BUFS], dtype)


_restated = {}


def restate_case(cid, bank, mode, J, shape, dtype=torch.float64):
    """Every array of a fixture case from the restatement in ``dtype``, as float64; computed once per (case, dtype), read-only."""
    key = (cid, dtype)
    if key not in _restated:
        g = gold()
        b = fixture_bank(bank, dtype)
        x = torch.from_numpy(g["x_%dx%dx%dx%d" % shape]).to(dtype)
        out = {"y%d" % j: y for j, y in enumerate(forward_levels(x, b, mode, J))}
        out["xgrad"] = forward_grad([decode(g[cid + "/cot_y%d" % j]).to(dtype) for j in range(J)], b, mode)
        _restated[key] = {k: v.double() for k, v in out.items()}
    return _restated[key]


# ----------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def waves(fa, bank):
    """(analysis wave, synthesis wave) of a bank name; 'db2db4' is the 4-tuple with db2 on col (H) and db4 on row (W)."""
    if bank == "db2db4":
        a, b = fa.daubechies(2), fa.daubechies(4)
        return (a.dec_lo, a.dec_hi, b.dec_lo, b.dec_hi), (a.rec_lo, a.rec_hi, b.rec_lo, b.rec_hi)
    w = fa.daubechies(int(bank[2:]))
    return w, w


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_restatement_matches_the_fixture(case):
    cid, bank, mode, J, shape = case
    got = restate_case(*case)
    assert sorted(got) == sorted(["y%d" % j for j in range(J)] + ["xgrad"])
    for k, v in got.items():
        want = torch.from_numpy(gold()[cid + "/" + k])
        assert tuple(v.shape) == tuple(want.shape), (cid, k, tuple(v.shape), tuple(want.shape))
        e = rel_l2(want, v)
        print("SWT_PIN %-36s %-6s %.3e" % (cid, k, e))
        assert e <= PIN, (cid, k, e)


def test_fixture_holds_the_cases_of_the_issue():
    cases = [c[1:] for c in fixture_cases()]
    for mode in MODES:
        for bank in ("db2", "db4", "db2db4"):
            assert (bank, mode, 1, (2, 2, 13, 18)) in cases
        assert ("db4", mode, 2, (1, 1, 9, 9)) in cases
        assert ("db4", mode, 2, (1, 1, 70, 150)) in cases
    assert len(cases) == 20
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20


def test_the_mixed_bank_pins_the_axis_naming():
    """db2 on col, db4 on row: with the pairs swapped the restatement is far from the fixture, so the fixture tells them apart."""
    cid, bank, mode, J, shape = next(c for c in fixture_cases() if c[1] == "db2db4" and c[2] == "symmetric")
    b = fixture_bank(bank)
    assert b[0].numel() == 4 and b[2].numel() == 8                  # the col pair (4 taps) filters along H
    x = torch.from_numpy(gold()["x_%dx%dx%dx%d" % shape]).double()
    want = torch.from_numpy(gold()[cid + "/y0"])
    assert rel_l2(want, analysis_2d(x, b, mode, 1)) <= PIN
    assert rel_l2(want, analysis_2d(x, (b[2], b[3], b[0], b[1]), mode, 1)) > 0.1


@pytest.mark.parametrize("mode", MODES)
def test_restated_adjoint_is_the_transpose(mode):
    """<A x, c> == <x, A^T c> in float64, at d = 1 and at d = 4 on the minimum side of db4 (17)."""
    g = torch.Generator().manual_seed(11)
    import faoctasr
    w = faoctasr.daubechies(4)
    b = tuple(torch.tensor(t, dtype=torch.float64) for t in (w.dec_lo, w.dec_hi, w.dec_lo, w.dec_hi))
    for d, shape in ((1, (1, 2, 7, 10)), (4, (1, 1, 17, 23))):
        x = torch.randn(shape, generator=g, dtype=torch.float64)
        y = analysis_2d(x, b, mode, d)
        c = torch.randn(y.shape, generator=g, dtype=torch.float64)
        lhs, rhs = float((y * c).sum()), float((x * adjoint_2d(c, b, mode, d)).sum())
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (mode, d, lhs, rhs)


@pytest.mark.parametrize("bank", ("db1", "db4", "db8", "db2db4"))
def test_fp64_reconstruction(fa, bank):
    """inverse(forward(x)) == x to 1e-10, J = 3 at 33x40, from the modules' own construction (float64 taps)."""
    wf, wi = waves(fa, bank)
    af = tuple(torch.tensor(np.asarray(t, dtype=np.float64)) for t in fa.wavelets._swt_taps(wf, True))
    sy = tuple(torch.tensor(np.asarray(t, dtype=np.float64)) for t in fa.wavelets._swt_taps(wi, False))
    x = torch.randn(2, 1, 33, 40, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    y = inverse_levels(forward_levels(x, af, "periodic", 3), sy)
    err = float((y - x).abs().max())
    print("SWT_PIN reconstruction %s max-abs %.3e" % (bank, err))
    assert err <= 1e-10


def test_inverse_is_a_quarter_of_the_adjoint_for_an_orthonormal_bank(fa):
    w = fa.daubechies(4)
    a = tuple(torch.tensor(t, dtype=torch.float64) for t in (w.dec_lo, w.dec_hi, w.dec_lo, w.dec_hi))
    s = tuple(torch.tensor(t, dtype=torch.float64) for t in (w.rec_lo, w.rec_hi, w.rec_lo, w.rec_hi))
    c = torch.randn(1, 2, 4, 19, 21, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    for d in (1, 2):
        assert float((inverse_2d(c, s, d) - 0.25 * adjoint_2d(c, a, "periodic", d)).abs().max()) <= 1e-12


def test_modules_register_the_reference_buffers(fa):
    d2, d4 = fa.daubechies(2), fa.daubechies(4)
    forms = {"db4": d4, "db2": (d2.dec_lo, d2.dec_hi), "db2db4": (np.array(d2.dec_lo), torch.tensor(d2.dec_hi), d4.dec_lo, d4.dec_hi)}
    for bank, wf in forms.items():
        fwd = fa.SWTForward(J=2, wave=wf, mode="symmetric")
        assert sorted(n for n, _ in fwd.named_buffers()) == sorted(A_BUFS)
        for n in A_BUFS:
            want, got = gold()["buf_%s_%s" % (bank, n)], getattr(fwd, n)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, (bank, n)
            np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=0)
    assert tuple(fwd.h0_col.shape) == (1, 1, 4, 1) and tuple(fwd.h0_row.shape) == (1, 1, 1, 8)
    inv = fa.SWTInverse(wave=(d2.rec_lo, d2.rec_hi, d4.rec_lo, d4.rec_hi))
    assert sorted(n for n, _ in inv.named_buffers()) == sorted(S_BUFS)
    assert tuple(inv.g0_col.shape) == (1, 1, 4, 1) and tuple(inv.g1_row.shape) == (1, 1, 1, 8)
    np.testing.assert_allclose(inv.g1_row.reshape(-1).numpy(), np.asarray(d4.rec_hi, dtype=np.float32), rtol=1e-6)
    np.testing.assert_allclose(inv.g0_col.reshape(-1).numpy(), np.asarray(d2.rec_lo, dtype=np.float32), rtol=1e-6)
    s = 2.0 ** -0.5
    haar = fa.SWTForward()                                          # defaults: one level, db1, 'periodization'
    assert haar.J == 1 and haar.mode == "periodization"
    np.testing.assert_allclose(haar.h1_col.reshape(-1).numpy(), [s, -s], rtol=1e-6)      # dec_hi = [-s, s], reversed
    np.testing.assert_allclose(fa.SWTInverse().g1_row.reshape(-1).numpy(), [s, -s], rtol=1e-6)


def test_state_dict_round_trip(fa):
    src, dst = fa.SWTForward(J=2, wave=fa.daubechies(4), mode="reflect"), fa.SWTForward(J=2, wave=([0.0] * 8, [0.0] * 8), mode="reflect")
    sd = src.state_dict()
    assert sorted(sd) == sorted(A_BUFS)
    dst.load_state_dict(sd, strict=True)
    for n in A_BUFS:
        assert torch.equal(getattr(dst, n), getattr(src, n))
        assert dst._taps[n] == src._taps[n]                         # the host record follows the loaded buffers
    inv, inv2 = fa.SWTInverse(wave=fa.daubechies(2)), fa.SWTInverse(wave=([0.0] * 4, [0.0] * 4))
    inv2.load_state_dict(inv.state_dict(), strict=True)
    assert all(torch.equal(getattr(inv2, n), getattr(inv, n)) and inv2._taps[n] == inv._taps[n] for n in S_BUFS)


def test_mode_aliases_and_errors(fa):
    from faoctasr.wavelets import swt_mode_to_int
    assert swt_mode_to_int("periodization") == swt_mode_to_int("per") == swt_mode_to_int("periodic") == 6
    assert [swt_mode_to_int(m) for m in MODES] == [0, 1, 4, 6]
    d4 = fa.daubechies(4)
    for mode in ("periodic", "periodization", "per"):
        fa.SWTInverse(wave=d4, mode=mode)
    for mode in ("zero", "symmetric", "reflect"):
        with pytest.raises(ValueError, match="periodic"):
            fa.SWTInverse(wave=d4, mode=mode)
    for mode in ("constant", "replicate", "nonsense"):
        with pytest.raises(ValueError):
            fa.SWTForward(wave=d4, mode=mode)
    with pytest.raises(ValueError):
        fa.SWTForward(J=5, wave=d4)                                 # dilation 16
    with pytest.raises(ValueError):
        fa.SWTForward(wave=(d4.dec_lo[:7], d4.dec_hi[:7]))          # odd L
    with pytest.raises(NotImplementedError):
        fa.SWTForward(wave="db4")                                   # names other than haar / db1 stay unresolved
    # minimum side L 2^(J-1) / 2 + 1: db4, J = 2 -> 9; checked before anything is launched (a host tensor gets that far)
    for mode in MODES + ("periodization",):
        fwd = fa.SWTForward(J=2, wave=d4, mode=mode)
        for shape in ((1, 1, 8, 16), (1, 1, 16, 8)):
            with pytest.raises(ValueError, match="minimum side"):
                fwd(torch.zeros(shape))
    with pytest.raises(ValueError, match="minimum side"):
        fa.SWTInverse(wave=d4)([torch.zeros(1, 1, 4, 8, 16), torch.zeros(1, 1, 4, 8, 16)])
    with pytest.raises(fa.KernelError):                             # a host tensor of a legal size is refused, not computed
        fa.SWTForward(J=2, wave=d4, mode="zero")(torch.zeros(1, 1, 9, 9))


def test_entry_points_are_declared(fa):
    header = open(os.path.join(ROOT, "include", "faoctasr.h")).read()
    for name in ("faoctasr_swt2d_analysis", "faoctasr_swt2d_adjoint"):
        assert "int %s(" % name in header
        assert name in fa._lib.declared_symbols()
