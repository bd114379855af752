"""The DTCWT magnitude loss without a GPU: a plain-torch restatement

    L(x, y) = sum_j w_j * mean |r_j(x) - r_j(y)|,   r = sqrt(re^2 + im^2 + b^2)

on the dual-tree levels of tests/test_dtcwt_cpu.py, with its backward written out -- the cotangent band of x at level j is
``w_j / count_j * sign(r_x - r_y) * z_x / r_x`` (of y: the negative, with ``z_y / r_y``; sign(0) = 0), carried to the images by the
levels' adjoints ``inv_j2`` / ``inv_j1`` on the analysis taps --, pinned to the reference's own float64 results
(tests/golden/golden_cwt_loss.npz, tools/gen_golden_dtcwt_loss.py), and the host logic of ``ops.dtcwt_mag_loss``,
``DTCWTMagnitudeLoss`` and ``TrainStep(cwt_weight=...)`` (everything that raises before an entry point is reached).

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (the loss: absolute difference over |loss|; dx, dy:
relative L2).  Both sides are float64 sums of a few hundred terms and pointwise operations of condition number about 1 (b > 0
keeps r away from zero), about 1e-14 of rounding -- PROVIDED no sign flips, which the tie condition guarantees: every case's
smallest |r_x - r_y| / max(r_x, r_y) is at least 2^-16 (asserted here on the restatement's own magnitudes, coefficient by
coefficient, none excluded), eleven orders of magnitude above float64 rounding."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_dtcwt_cpu import forward_levels, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_cwt_loss.npz")
BANKS = ("a", "b", "c")
BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")
MAGBIAS = 1e-2
MIN_GAP = 2.0 ** -16
#: (case, shape, J, mode, level weights or None, y needs a gradient): the table of tools/gen_golden_dtcwt_loss.py
CASES = (("j1_symmetric", (2, 3, 16, 24), 1, "symmetric", None, True),
         ("j1_zero", (2, 3, 16, 24), 1, "zero", None, True),
         ("j2_symmetric", (2, 3, 16, 24), 2, "symmetric", None, True),
         ("j3_symmetric", (2, 3, 16, 24), 3, "symmetric", None, True),
         ("j3_8x8", (1, 1, 8, 8), 3, "symmetric", None, True),
         ("j3_weights", (1, 2, 8, 16), 3, "symmetric", (0.5, 1.25, 2.0), True),
         ("j2_zero_xonly", (1, 2, 8, 16), 2, "zero", None, False))
NEW_SYMBOLS = ("faoctasr_dtcwt_loss_workspace_floats", "faoctasr_dtcwt_loss_fwd_j1", "faoctasr_dtcwt_loss_fwd_j2", "faoctasr_dtcwt_loss_final")
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
    return torch.from_numpy(g["in/%s/x" % case[1]]), torch.from_numpy(g["in/%s/y" % case[1]])


# ------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------
def restate(x, y, b, mode, J, weights=None, bias=MAGBIAS, dtype=torch.float64, x_grad=True, y_grad=True):
    """{"loss", "dx", "dy", "gap"} in ``dtype``.  The levels (with the modules' padding of odd sides and of lowpass sides that
    are no multiple of 4) come from ``forward_levels``, whose backward is the levels' adjoints written out in test_dtcwt_cpu; the
    cotangent bands handed to it are the explicit formulas of the module docstring, not autograd's."""
    b = {k: v.to(dtype) for k, v in b.items()}
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(True)
    w = [1.0] * J if weights is None else list(weights)
    hx, hy = forward_levels(x, b, mode, J)[1], forward_levels(y, b, mode, J)[1]
    loss, gap, cx, cy = 0.0, float("inf"), [], []
    for j in range(J):
        zx, zy = hx[j].detach(), hy[j].detach()
        rx = torch.sqrt(zx[..., 0] ** 2 + zx[..., 1] ** 2 + bias * bias)
        ry = torch.sqrt(zy[..., 0] ** 2 + zy[..., 1] ** 2 + bias * bias)
        d = rx - ry
        loss = loss + w[j] * d.abs().sum() / d.numel()
        gap = min(gap, float((d.abs() / torch.maximum(rx, ry)).min()))
        s = torch.sign(d) * (w[j] / d.numel())
        cx.append((s / rx).unsqueeze(-1) * zx)
        cy.append((-s / ry).unsqueeze(-1) * zy)
    out = {"loss": loss.detach().double(), "gap": gap}
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
        bank, _, _, J, mode, weights, y_grad = case
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, bufs(bank), mode, J, weights, y_grad=y_grad)
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
        for k in ("loss", "dx") + (("dy",) if case[6] else ()):
            assert "%s/%s/%s" % (case[0], case[1], k) in g and "%s/%s/f32/%s" % (case[0], case[1], k) in g
        assert ("%s/%s/dy" % (case[0], case[1]) in g) == case[6]


@pytest.mark.parametrize("case", fixture_cases(), ids=case_name)
def test_restatement_matches_reference(case):
    g, ref = gold(), restate_case(case)
    pre = "%s/%s/" % (case[0], case[1])
    assert ref["gap"] >= MIN_GAP, ref["gap"]                              # the tie condition
    assert abs(ref["gap"] - float(g[pre + "gap"])) <= 1e-9 * ref["gap"]
    assert loss_err(ref["loss"], g[pre + "loss"]) <= 1e-12
    assert rel_l2(ref["dx"], g[pre + "dx"]) <= 1e-12
    if case[6]:
        assert rel_l2(ref["dy"], g[pre + "dy"]) <= 1e-12
    else:
        assert "dy" not in ref


def test_fp32_reference_error_is_meaningful():
    """The fp32 reference sits 1e-9 .. 2e-6 from the fp64 one: e_ref of the GPU test's bar is neither zero nor large."""
    g = gold()
    for case in fixture_cases():
        pre = "%s/%s/" % (case[0], case[1])
        for k in ("dx",) + (("dy",) if case[6] else ()):
            e = rel_l2(g[pre + "f32/" + k], g[pre + k])
            assert 1e-9 < e < 2e-6, (case_name(case), k, e)
        assert loss_err(g[pre + "f32/loss"], g[pre + "loss"]) < 1e-6


def test_restated_properties():
    """L(x, x) = 0 with zero gradients (sign(0) = 0), symmetry, and the weights' linearity, on the restatement itself."""
    b = bufs("a")
    x, y = fixture_inputs(("a",) + CASES[5])
    same = restate(x, x, b, "symmetric", 3)
    assert float(same["loss"]) == 0.0 and not same["dx"].any() and not same["dy"].any()
    xy, yx = restate(x, y, b, "symmetric", 3), restate(y, x, b, "symmetric", 3)
    assert float(xy["loss"]) == float(yx["loss"]) and torch.equal(xy["dx"], yx["dy"]) and torch.equal(xy["dy"], yx["dx"])
    half = restate(x, y, b, "symmetric", 3, weights=(0.5, 0.5, 0.5))
    assert float(half["loss"]) == 0.5 * float(xy["loss"]) and torch.equal(half["dx"], 0.5 * xy["dx"])


def test_restated_gradient_is_the_derivative():
    """A central difference along a random direction, well inside the region where no sign flips (gap 9e-4, step 1e-6)."""
    case = ("a",) + CASES[5]
    x, y = fixture_inputs(case)
    b = bufs("a")
    ref = restate_case(case)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    eps = 1e-6
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + eps * v, y) if which == 0 else (x, y.double() + eps * v)), b, "symmetric", 3, CASES[5][4])
        dn = restate(*((x.double() - eps * v, y) if which == 0 else (x, y.double() - eps * v)), b, "symmetric", 3, CASES[5][4])
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
    assert fa.DTCWTMagnitudeLoss is fa.wavelets.DTCWTMagnitudeLoss and "DTCWTMagnitudeLoss" in fa.__all__
    assert callable(fa.ops.dtcwt_mag_loss)
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"dtcwt_loss.hip"' in src


def test_signatures(fa):
    sig = inspect.signature(fa.DTCWTMagnitudeLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("biort", "near_sym_a"), ("qshift", "qshift_a"), ("J", 3), ("mode", "symmetric"), ("magbias", 1e-2), ("level_weights", None)]
    sig = inspect.signature(fa.ops.dtcwt_mag_loss)
    assert (sig.parameters["mode"].default, sig.parameters["magbias"].default, sig.parameters["level_weights"].default) == (1, 1e-2, None)
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("cwt_weight", "cwt_levels", "cwt_biort", "cwt_qshift", "cwt_mode")] == [
        0.0, 1, "near_sym_a", "qshift_a", "symmetric"]


def test_fused_size_rule(fa):
    f = fa.ops.dtcwt_mag_loss_fused
    for n in (192, 256, 512):
        assert all(f(n, n, J) for J in (1, 2, 3))
    assert f(8, 8, 3) and f(40, 264, 3) and f(2, 2, 1)
    assert not f(13, 19, 2) and not f(12, 16, 3) and not f(4, 8, 3) and not f(16, 24, 4)


@pytest.mark.parametrize("bank", BANKS)
def test_state_dict_names_are_those_of_the_transform(fa, bank):
    fb, fq = tuples(bank)
    crit, fwd = fa.DTCWTMagnitudeLoss(biort=fb, qshift=fq, J=3), fa.DTCWTForward(biort=fb, qshift=fq, J=3)
    assert list(crit.state_dict()) == list(fwd.state_dict()) == list(BUFS)
    for n in BUFS:
        assert torch.equal(getattr(crit, n), getattr(fwd, n)), n
        assert torch.equal(getattr(crit, n).reshape(-1), bufs(bank)[n].float())
    assert (crit.J, crit.mode, crit.magbias, crit.level_weights) == (3, "symmetric", 1e-2, None)
    one = fa.DTCWTMagnitudeLoss(biort=fb, qshift=fq, J=1, level_weights=[2])
    assert list(one.state_dict()) == ["h0o", "h1o"] and one.level_weights == (2.0,)


def test_names_without_a_provider(fa, monkeypatch):
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("no_such_module_for_dtcwt.coeffs",))
    for biort in ("near_sym_a", "legall"):
        crit = fa.DTCWTMagnitudeLoss(biort=biort, J=1)                    # qshift is not resolved at J = 1
        assert list(crit.state_dict()) == ["h0o", "h1o"]
    with pytest.raises(NotImplementedError, match="qshift_a.*4-tuple"):
        fa.DTCWTMagnitudeLoss(J=2)
    with pytest.raises(NotImplementedError, match="qshift_a.*4-tuple"):
        fa.DTCWTMagnitudeLoss()


def test_bp_banks_stay_refused(fa):
    fb, fq = tuples("a")
    for kw in (dict(biort="near_sym_b_bp", qshift=fq), dict(biort=fb, qshift="qshift_b_bp"), dict(biort=fb, qshift="qshift_b_bp", J=1)):
        with pytest.raises(NotImplementedError, match="three-filter"):
            fa.DTCWTMagnitudeLoss(**kw)


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    (h0o, h1o), q = tuples("a")
    x = torch.zeros(1, 1, 8, 8)
    loss = fa.ops.dtcwt_mag_loss
    with pytest.raises(ValueError, match="float32"):
        loss(x.double(), x.double(), h0o, h1o, q, 2)
    with pytest.raises(ValueError, match="float32"):
        loss(x, x.half(), h0o, h1o, q, 2)
    with pytest.raises(ValueError, match="device"):
        loss(x, x, h0o, h1o, q, 2)
    with pytest.raises(ValueError, match="device"):
        loss(torch.zeros(1, 1, 13, 19), torch.zeros(1, 1, 13, 19), h0o, h1o, q, 2)          # the composed path refuses as well
    with pytest.raises(ValueError, match="same shape"):
        loss(x, torch.zeros(1, 1, 8, 16), h0o, h1o, q, 2)
    with pytest.raises(ValueError, match="4 dimensions"):
        loss(x[0], x[0], h0o, h1o, q, 2)
    for bad in (0.0, -1e-2, float("nan")):
        with pytest.raises(ValueError, match="magbias"):
            loss(x, x, h0o, h1o, q, 2, magbias=bad)
        with pytest.raises(ValueError, match="magbias"):
            fa.DTCWTMagnitudeLoss(biort=(h0o, h1o), qshift=q, magbias=bad)
    with pytest.raises(ValueError, match="level_weights"):
        loss(x, x, h0o, h1o, q, 2, level_weights=[1.0])
    with pytest.raises(ValueError, match="level_weights"):
        fa.DTCWTMagnitudeLoss(biort=(h0o, h1o), qshift=q, J=3, level_weights=[1.0, 2.0])
    for J in (0, -1):
        with pytest.raises(ValueError, match="J >= 1"):
            loss(x, x, h0o, h1o, q, J)
        with pytest.raises(ValueError, match="J >= 1"):
            fa.DTCWTMagnitudeLoss(biort=(h0o, h1o), qshift=q, J=J)
    with pytest.raises(ValueError, match="q-shift"):
        loss(x, x, h0o, h1o, None, 2)
    with pytest.raises(ValueError, match="odd"):
        loss(x, x, [0.25] * 4, h1o, q, 2)
    with pytest.raises(ValueError, match="same length"):
        loss(x, x, h0o, h1o, (q[0], q[1], q[2], q[3][:4]), 2)
    with pytest.raises(ValueError, match="Unkown pad type"):
        loss(x, x, h0o, h1o, q, 2, mode=9)
    with pytest.raises(ValueError, match="Unkown pad type"):
        fa.DTCWTMagnitudeLoss(biort=(h0o, h1o), qshift=q, mode="nope")(x, x)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.DTCWTMagnitudeLoss

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "DTCWTMagnitudeLoss", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.cwt_weight == 0.0 and ts.cwt_loss is None and not built
    _, fq = tuples("a")
    ts = fa.TrainStep(*nets, device="cpu", cwt_weight=0.5, cwt_levels=2, cwt_biort="legall", cwt_qshift=fq, cwt_mode="zero")
    assert built == [dict(biort="legall", qshift=fq, J=2, mode="zero")]
    assert ts.cwt_weight == 0.5 and (ts.cwt_loss.J, ts.cwt_loss.mode) == (2, "zero")
    assert list(ts.cwt_loss.state_dict()) == list(BUFS)
