"""The complex-wavelet structural similarity without a GPU: a plain-torch restatement of

    S(x, y) = sum_j w_j S_j / sum_j w_j,   S_j = mean over (n, c, orientation, position p) of S_p = (2 |z_p| + K) / (E_p + K),
    z_p = sum_{q in W(p)} cx_q conj(cy_q),   E_p = sum_W |cx_q|^2 + sum_W |cy_q|^2

on the dual-tree levels of tests/test_dtcwt_cpu.py (win x win box windows at the valid positions), with its backward written
out -- with u_p = z_p / |z_p|, a_p = 2 / (E_p + K), b_p = 2 S_p / (E_p + K), A_q = sum_{p: q in W(p)} a_p u_p and B_q likewise of b_p,
the cotangent bands are dS_j/dcx_q = (cy_q A_q - cx_q B_q) / count_j and dS_j/dcy_q = (cx_q conj(A_q) - cy_q B_q) / count_j, carried to the
images by the levels' adjoints --, pinned to the reference's own float64 results (tests/golden/golden_cwssim.npz,
tools/gen_golden_cwssim.py), and the host logic of ``ops.cw_ssim``, ``ops.cw_ssim_bands``, ``CWSSIM``, ``image_metrics(cw_ssim=...)``
and ``TrainStep(cwssim_weight=...)`` (everything that raises before an entry point is reached).  The fixture and every test
here speak of the loss 1 - S and of the per-image scores S.

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (the loss: absolute difference over |loss|; arrays:
relative L2).  Both sides are float64 sums of at most a few thousand terms; the only ill-conditioned step is u = z / |z|, which
amplifies rounding by kappa_p = sum_W |cx| |cy| / |z_p|, and every case's largest kappa_p is at most 8 (asserted on the
restatement, window by window, none excluded): about 1e-14 of rounding."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_dtcwt_cpu import forward_levels, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_cwssim.npz")
BANKS = ("a", "b", "c")
BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")
KC = 1e-2
MAX_KAPPA = 8.0
#: (case, shape, J, win, mode, level weights or None, y needs a gradient): the table of tools/gen_golden_cwssim.py
CASES = (("j1_w3_symmetric", (2, 3, 16, 24), 1, 3, "symmetric", None, True),
         ("j1_w3_zero", (1, 3, 16, 24), 1, 3, "zero", None, True),
         ("j2_w3_symmetric", (2, 3, 16, 24), 2, 3, "symmetric", None, True),
         ("j3_w7_56x56", (1, 1, 56, 56), 3, 7, "symmetric", None, True),
         ("j2_w5_weights", (1, 2, 24, 40), 2, 5, "symmetric", (0.5, 2.0), True),
         ("j1_w1", (2, 1, 16, 16), 1, 1, "symmetric", None, True),
         ("j2_w3_xonly", (1, 3, 16, 24), 2, 3, "symmetric", None, False))
NEW_SYMBOLS = ("faoctasr_cwssim_workspace_floats", "faoctasr_cwssim_index", "faoctasr_cwssim_grad", "faoctasr_cwssim_final")
_gold = {}
_restated = {}


def gold():
    if not _gold:
        with np.load(GOLDEN) as z:
            _gold.update({k: z[k] for k in z.files})
    return _gold


def bufs(bank, dtype=torch.float64):
    """The six registered buffers of a bank pair as flat tensors (taps reversed, as prep_filt stores them)."""
    return {n: torch.from_numpy(gold()["%s/buf_%s" % (bank, n)]).reshape(-1).to(dtype) for n in BUFS}


def tuples(bank):
    """(biort, qshift) in the order the constructors take them."""
    w = {k: v.flip(0).tolist() for k, v in bufs(bank).items()}
    return (w["h0o"], w["h1o"]), (w["h0a"], w["h0b"], w["h1a"], w["h1b"])


def fixture_cases():
    return [(bank,) + c for bank in BANKS for c in CASES]


def case_name(case):
    return "%s_%s" % (case[0], case[1])


def fixture_inputs(case):
    g = gold()
    key = "%dx%dx%dx%d" % tuple(case[2])
    return torch.from_numpy(g["in/%s/x" % key]), torch.from_numpy(g["in/%s/y" % key])


# ------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------
def box(t, win):
    """out[..., i, j] = sum_{s, r < win} t[..., i + s, j + r] at the valid positions, as a sum of shifted slices."""
    ph, pw = t.shape[-2] - win + 1, t.shape[-1] - win + 1
    out = torch.zeros(t.shape[:-2] + (ph, pw), dtype=t.dtype)
    for s in range(win):
        for r in range(win):
            out = out + t[..., s:s + ph, r:r + pw]
    return out


def box_t(t, win):
    """The transpose of ``box``: out[..., q] = the sum of t over the windows that contain q."""
    ph, pw = t.shape[-2:]
    out = torch.zeros(t.shape[:-2] + (ph + win - 1, pw + win - 1), dtype=t.dtype)
    for s in range(win):
        for r in range(win):
            out[..., s:s + ph, r:r + pw] += t
    return out


def level_terms(cx, cy, win, K=KC):
    """(S_p, dS/dcx summed over p, dS/dcy likewise, largest kappa_p) of one level's detached bands (N, C, 6, h, w, 2)."""
    xr, xi, yr, yi = cx[..., 0], cx[..., 1], cy[..., 0], cy[..., 1]
    zr, zi = box(xr * yr + xi * yi, win), box(xi * yr - xr * yi, win)
    E = box(xr * xr + xi * xi, win) + box(yr * yr + yi * yi, win)
    m = torch.sqrt(zr * zr + zi * zi)
    S = (2 * m + K) / (E + K)
    safe = torch.where(m > 0, m, torch.ones_like(m))
    ur, ui = torch.where(m > 0, zr / safe, torch.zeros_like(m)), torch.where(m > 0, zi / safe, torch.zeros_like(m))
    a, b = 2 / (E + K), 2 * S / (E + K)
    Ar, Ai, B = box_t(a * ur, win), box_t(a * ui, win), box_t(b, win)
    gx = torch.stack((yr * Ar - yi * Ai - xr * B, yr * Ai + yi * Ar - xi * B), -1)           # cy A - cx B
    gy = torch.stack((xr * Ar + xi * Ai - yr * B, -xr * Ai + xi * Ar - yi * B), -1)          # cx conj(A) - cy B
    kappa = float((box(torch.sqrt(xr * xr + xi * xi) * torch.sqrt(yr * yr + yi * yi), win) / m).max())
    return S, gx, gy, kappa


def restate(x, y, b, mode, J, win, weights=None, K=KC, dtype=torch.float64, x_grad=True, y_grad=True, levels=forward_levels):
    """{"loss", "scores", "dx", "dy", "kappa"} in ``dtype``: the loss is 1 - mean_n S_n, ``scores`` the S_n.  The levels (with the
    modules' padding) come from ``levels``, whose backward is the levels' adjoints written out in test_dtcwt_cpu; the cotangent
    bands handed to it are the explicit formulas of the module docstring, not autograd's."""
    b = {k: v.to(dtype) for k, v in b.items()}
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(True)
    w = [1.0] * J if weights is None else list(weights)
    hx, hy = levels(x, b, mode, J)[1], levels(y, b, mode, J)[1]
    N = x.shape[0]
    scores, kappa, cx, cy = torch.zeros(N, dtype=dtype), 0.0, [], []
    for j in range(J):
        S, gx, gy, k = level_terms(hx[j].detach(), hy[j].detach(), win, K)
        scores = scores + w[j] * S.mean(dim=(1, 2, 3, 4))
        kappa = max(kappa, k)
        scale = -(w[j] / sum(w)) / S.numel()                              # d(1 - S) / dS_j over count_j
        cx.append(gx * scale)
        cy.append(gy * scale)
    scores = scores / sum(w)
    out = {"loss": (1 - scores.mean()).double(), "scores": scores.double(), "kappa": kappa}
    if x_grad:
        torch.autograd.backward(hx, cx)
        out["dx"] = x.grad.double()
    if y_grad:
        torch.autograd.backward(hy, cy)
        out["dy"] = y.grad.double()
    return out


def restate_case(case):
    """The float64 restatement of a fixture case, computed once and shared (do not modify the arrays)."""
    key = case_name(case)
    if key not in _restated:
        bank, _, _, J, win, mode, weights, y_grad = case
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, bufs(bank), mode, J, win, weights, y_grad=y_grad)
    return _restated[key]


def loss_err(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_fixture_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 1 << 20
    g = gold()
    for case in fixture_cases():
        for k in ("loss", "scores", "dx") + (("dy",) if case[7] else ()):
            assert "%s/%s/%s" % (case[0], case[1], k) in g and "%s/%s/f32/%s" % (case[0], case[1], k) in g
        assert ("%s/%s/dy" % (case[0], case[1]) in g) == case[7]
        assert "%s/%s/kappa" % (case[0], case[1]) in g


@pytest.mark.parametrize("case", fixture_cases(), ids=case_name)
def test_restatement_matches_reference(case):
    g, ref = gold(), restate_case(case)
    pre = "%s/%s/" % (case[0], case[1])
    assert ref["kappa"] <= MAX_KAPPA, ref["kappa"]                        # the conditioning condition
    assert abs(ref["kappa"] - float(g[pre + "kappa"])) <= 1e-9 * ref["kappa"]
    assert loss_err(ref["loss"], g[pre + "loss"]) <= 1e-12
    assert rel_l2(ref["scores"], g[pre + "scores"]) <= 1e-12
    assert rel_l2(ref["dx"], g[pre + "dx"]) <= 1e-12
    if case[7]:
        assert rel_l2(ref["dy"], g[pre + "dy"]) <= 1e-12
    else:
        assert "dy" not in ref


def test_fp32_reference_error_is_meaningful():
    """The fp32 reference sits 1e-9 .. 2e-6 from the fp64 one: e_ref of the GPU test's bar is neither zero nor large."""
    g = gold()
    for case in fixture_cases():
        pre = "%s/%s/" % (case[0], case[1])
        for k in ("dx",) + (("dy",) if case[7] else ()):
            e = rel_l2(g[pre + "f32/" + k], g[pre + k])
            assert 1e-9 < e < 2e-6, (case_name(case), k, e)
        e = loss_err(g[pre + "f32/loss"], g[pre + "loss"])
        assert 1e-9 < e < 2e-6, (case_name(case), "loss", e)


def test_restated_properties():
    """S(x, x) = 1 exactly with zero gradients, symmetry, and per-image scores whose mean is the batch score, on the restatement."""
    case = ("a",) + CASES[2]
    b = bufs("a")
    x, y = fixture_inputs(case)
    same = restate(x, x, b, "symmetric", 2, 3)
    assert float(same["loss"]) == 0.0 and bool((same["scores"] == 1.0).all())
    assert not same["dx"].any() and not same["dy"].any()
    xy, yx = restate(x, y, b, "symmetric", 2, 3), restate(y, x, b, "symmetric", 2, 3)
    assert float(xy["loss"]) == float(yx["loss"]) and torch.equal(xy["scores"], yx["scores"])
    assert torch.equal(xy["dx"], yx["dy"]) and torch.equal(xy["dy"], yx["dx"])
    assert xy["scores"].shape == (2,) and 0 < float(xy["scores"].min()) and float(xy["scores"].max()) < 1
    assert abs(float(xy["scores"].mean()) - (1 - float(xy["loss"]))) <= 1e-15
    for n in range(2):                                                    # an image's score does not depend on its batch
        alone = restate(x[n:n + 1], y[n:n + 1], b, "symmetric", 2, 3)
        assert abs(float(alone["scores"][0]) - float(xy["scores"][n])) <= 1e-15


def test_restated_gradient_is_the_derivative():
    """A central difference along a random direction (kappa <= 2: |z| stays far from 0 over the step 1e-6)."""
    case = ("a",) + CASES[4]
    x, y = fixture_inputs(case)
    b = bufs("a")
    ref = restate_case(case)
    J, win, weights = case[3], case[4], case[6]
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    eps = 1e-6
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + eps * v, y) if which == 0 else (x, y.double() + eps * v)), b, "symmetric", J, win, weights)
        dn = restate(*((x.double() - eps * v, y) if which == 0 else (x, y.double() - eps * v)), b, "symmetric", J, win, weights)
        num, ana = (float(up["loss"]) - float(dn["loss"])) / (2 * eps), float((ref[key] * v).sum())
        assert abs(num - ana) <= 1e-7 * abs(ana), (key, num, ana)


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_exports_and_symbols(fa):
    assert fa.CWSSIM is fa.wavelets.CWSSIM and "CWSSIM" in fa.__all__
    assert callable(fa.ops.cw_ssim) and callable(fa.ops.cw_ssim_bands) and fa.ops.CWSSIM_MAX_WIN == 11
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"cwssim.hip"' in src


def test_signatures(fa):
    sig = inspect.signature(fa.CWSSIM.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("biort", "near_sym_a"), ("qshift", "qshift_a"), ("J", 3), ("mode", "symmetric"), ("win", 7), ("K", 1e-2), ("level_weights", None),
        ("per_image", False)]
    sig = inspect.signature(fa.ops.cw_ssim)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[4:]] == [
        ("qshift", None), ("J", 1), ("mode", 1), ("win", 7), ("K", 0.01), ("level_weights", None), ("per_image", False), ("h2o", None),
        ("h2ab", None)]
    sig = inspect.signature(fa.ops.cw_ssim_bands)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [("win", 7), ("K", 0.01), ("per_image", False)]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("cwssim_weight", "cwssim_levels", "cwssim_win", "cwssim_biort", "cwssim_qshift", "cwssim_mode")] == [
        0.0, 2, 7, "near_sym_a", "qshift_a", "symmetric"]
    sig = inspect.signature(fa.evaluate_pairs)
    assert sig.parameters["cw_ssim"].default is None


def test_image_metrics_keeps_its_four_columns_by_default(fa):
    sig = inspect.signature(fa.image_metrics)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("y", inspect.Parameter.empty), ("gt", inspect.Parameter.empty), ("data_range", 2.0), ("bins", 100), ("cw_ssim", None)]


@pytest.mark.parametrize("bank", BANKS)
def test_state_dict_names_are_those_of_the_transform(fa, bank):
    fb, fq = tuples(bank)
    mod, fwd = fa.CWSSIM(biort=fb, qshift=fq, J=3), fa.DTCWTForward(biort=fb, qshift=fq, J=3)
    assert list(mod.state_dict()) == list(fwd.state_dict()) == list(BUFS)
    for n in BUFS:
        assert torch.equal(getattr(mod, n), getattr(fwd, n)), n
        assert torch.equal(getattr(mod, n).reshape(-1), bufs(bank)[n].float())
    assert (mod.J, mod.mode, mod.win, mod.K, mod.level_weights, mod.per_image) == (3, "symmetric", 7, 1e-2, None, False)
    one = fa.CWSSIM(biort=fb, qshift=fq, J=1, level_weights=[2], win=3, per_image=True)
    assert list(one.state_dict()) == ["h0o", "h1o"] and one.level_weights == (2.0,) and one.per_image
    assert "win=3" in repr(one) and "J=1" in repr(one)


def test_three_filter_banks_register_in_the_transforms_order(fa):
    import test_rot_cpu
    fb, fq = test_rot_cpu.tuples(test_rot_cpu.bufs())
    mod, fwd = fa.CWSSIM(biort=fb, qshift=fq, J=2), fa.DTCWTForward(biort=fb, qshift=fq, J=2)
    assert list(mod.state_dict()) == list(fwd.state_dict()) and len(mod.state_dict()) == 9 and mod.bandpass_diag
    for n in mod.state_dict():
        assert torch.equal(getattr(mod, n), getattr(fwd, n)), n
    one = fa.CWSSIM(biort=fb, qshift=fq, J=1)
    assert list(one.state_dict()) == ["h0o", "h1o", "h2o"]
    with pytest.raises(ValueError, match="three-filter"):
        fa.CWSSIM(biort=fb, qshift=fq[:4], J=2)


def test_names_without_a_provider(fa, monkeypatch):
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("no_such_module_for_dtcwt.coeffs",))
    for biort in ("near_sym_a", "legall"):
        mod = fa.CWSSIM(biort=biort, J=1)                                 # qshift is not resolved at J = 1
        assert list(mod.state_dict()) == ["h0o", "h1o"]
    with pytest.raises(NotImplementedError, match="qshift_a.*4-tuple"):
        fa.CWSSIM(J=2)
    with pytest.raises(NotImplementedError, match="qshift_a.*4-tuple"):
        fa.CWSSIM()


def test_bp_names_stay_refused(fa):
    fb, fq = tuples("a")
    for kw in (dict(biort="near_sym_b_bp", qshift=fq), dict(biort=fb, qshift="qshift_b_bp"), dict(biort=fb, qshift="qshift_b_bp", J=1)):
        with pytest.raises(NotImplementedError, match="three-filter"):
            fa.CWSSIM(**kw)


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    (h0o, h1o), q = tuples("a")
    x = torch.zeros(1, 1, 32, 32)
    f = fa.ops.cw_ssim
    with pytest.raises(ValueError, match="float32"):
        f(x.double(), x.double(), h0o, h1o, q, 2, win=3)
    with pytest.raises(ValueError, match="float32"):
        f(x, x.half(), h0o, h1o, q, 2, win=3)
    with pytest.raises(ValueError, match="device"):
        f(x, x, h0o, h1o, q, 2, win=3)
    with pytest.raises(ValueError, match="device"):
        f(torch.zeros(1, 1, 13, 19), torch.zeros(1, 1, 13, 19), h0o, h1o, q, 2, win=3)
    with pytest.raises(ValueError, match="same shape"):
        f(x, torch.zeros(1, 1, 32, 16), h0o, h1o, q, 2, win=3)
    with pytest.raises(ValueError, match="4 dimensions"):
        f(x[0], x[0], h0o, h1o, q, 2, win=3)
    with pytest.raises(ValueError, match=r"level 2 .* 32 x 32 .* 8 x 8,.* 9 x 9"):
        f(x, x, h0o, h1o, q, 2, win=9)
    with pytest.raises(ValueError, match=r"level 1 .* 8 x 40 .* 4 x 20,.* 5 x 5"):
        f(torch.zeros(1, 1, 8, 40), torch.zeros(1, 1, 8, 40), h0o, h1o, q, 1, win=5)
    with pytest.raises(ValueError, match=r"level 3 .* 13 x 19 .* 2 x 3,"):
        f(torch.zeros(1, 1, 13, 19), torch.zeros(1, 1, 13, 19), h0o, h1o, q, 3, win=3)       # 14 x 20 -> 16 x 20 -> 8 x 12: bands 7 x 10, 4 x 5, 2 x 3
    for bad in (0.0, -1e-2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="constant K"):
            f(x, x, h0o, h1o, q, 2, win=3, K=bad)
        with pytest.raises(ValueError, match="constant K"):
            fa.CWSSIM(biort=(h0o, h1o), qshift=q, K=bad)
        with pytest.raises(ValueError, match="constant K"):
            fa.ops.cw_ssim_bands(torch.zeros(1, 1, 6, 8, 8, 2), torch.zeros(1, 1, 6, 8, 8, 2), 3, bad)
    for bad in (0, 12, -3, 2.5):
        with pytest.raises(ValueError, match="win"):
            f(x, x, h0o, h1o, q, 2, win=bad)
        with pytest.raises(ValueError, match="win"):
            fa.CWSSIM(biort=(h0o, h1o), qshift=q, win=bad)
        with pytest.raises(ValueError, match="win"):
            fa.ops.cw_ssim_bands(torch.zeros(1, 1, 6, 16, 16, 2), torch.zeros(1, 1, 6, 16, 16, 2), bad)
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, -1.0], [0.0, 0.0], [-1.0, -2.0]):
        with pytest.raises(ValueError, match="level_weights"):
            f(x, x, h0o, h1o, q, 2, win=3, level_weights=bad)
        with pytest.raises(ValueError, match="level_weights"):
            fa.CWSSIM(biort=(h0o, h1o), qshift=q, J=2, level_weights=bad)
    for J in (0, -1):
        with pytest.raises(ValueError, match="J >= 1"):
            f(x, x, h0o, h1o, q, J, win=3)
        with pytest.raises(ValueError, match="J >= 1"):
            fa.CWSSIM(biort=(h0o, h1o), qshift=q, J=J)
    with pytest.raises(ValueError, match="q-shift"):
        f(x, x, h0o, h1o, None, 2, win=3)
    with pytest.raises(ValueError, match="Unkown pad type"):
        f(x, x, h0o, h1o, q, 2, mode=9, win=3)
    with pytest.raises(ValueError, match="Unkown pad type"):
        fa.CWSSIM(biort=(h0o, h1o), qshift=q, mode="nope", J=2, win=3)(x, x)
    bands = fa.ops.cw_ssim_bands
    h = torch.zeros(1, 2, 6, 8, 12, 2)
    with pytest.raises(ValueError, match="float32"):
        bands(h.double(), h.double(), 3)
    with pytest.raises(ValueError, match="device"):
        bands(h, h, 3)
    with pytest.raises(ValueError, match="same shape"):
        bands(h, torch.zeros(1, 2, 6, 8, 8, 2), 3)
    with pytest.raises(ValueError, match=r"\(N, C, 6, h, w, 2\)"):
        bands(h[0], h[0], 3)
    with pytest.raises(ValueError, match="8 x 12 band holds no 9 x 9 window"):
        bands(h, h, 9)
    mod = fa.CWSSIM(biort=(h0o, h1o), qshift=q, J=2, win=3)
    with pytest.raises(ValueError, match="device"):
        mod(x, x)
    with pytest.raises(ValueError, match="device"):
        mod.index(x, x, True)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.CWSSIM

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "CWSSIM", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.cwssim_weight == 0.0 and ts.cwssim is None and not built
    _, fq = tuples("a")
    ts = fa.TrainStep(*nets, device="cpu", cwssim_weight=0.5, cwssim_levels=3, cwssim_win=5, cwssim_biort="legall", cwssim_qshift=fq,
                      cwssim_mode="zero")
    assert built == [dict(biort="legall", qshift=fq, J=3, mode="zero", win=5)]
    assert ts.cwssim_weight == 0.5 and (ts.cwssim.J, ts.cwssim.mode, ts.cwssim.win, ts.cwssim.per_image) == (3, "zero", 5, False)
    assert list(ts.cwssim.state_dict()) == list(BUFS)
    assert ts.cwt_loss is None
