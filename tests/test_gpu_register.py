"""Phase-correlation registration and the Fourier shift on the MI355X: ``ops.phase_correlation`` / ``phase_correlation_surface`` /
``fourier_shift`` / ``Registered`` / ``RegistrationShift`` against the ``torch.fft`` restatement of tests/test_register_cpu.py, which
that file pins in float64 to the fixture (tests/golden/golden_register.npz, numpy with explicit DFT matrices).

The error bar is the one tests/test_gpu_phase_loss.py reasons for this DFT-as-GEMM path, relative to the error of the fp32 ``torch.fft``
run of the same definition on the CPU against float64:
  * surfaces, ``fourier_shift`` outputs and gradients, in relative L2:  e_hip <= 8 e_ref, e_ref that fp32 run's own error for the array;
  * ``peak``:  |p_hip - p_64| <= 8 r |p_64| + one fp32 ulp of p_64, r the fp32 run's largest relative peak error over the fixture.
The arg-max is discontinuous, so every comparison of a shift first re-asserts, on the float64 restatement, that the coarse and the
refined maximum lead their runners-up by at least 2^-12 of their value; under that guard the shift is held EXACTLY.

``fourier_shift`` takes the real part, which scales a Nyquist bin (even sides) by cos(pi d): a fractional shift and its inverse return
the image only on odd sides, where it is asserted against the image; on even sides it is asserted against the float64 restatement of
the same two shifts.  Figures of one run: profiles/register_error.txt."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("register_restatement", os.path.join(ROOT, "tests", "test_register_cpu.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

SHAPES, GAP = R.SHAPES, R.GAP
SEAMS, SEAMS_D = (2, 1, 72, 136), (-2.3, 1.7)
ODD = (1, 2, 37, 53)
SHIFTS = ((0.0, 0.0), (3.0, -2.0), (-2.3, 1.7), (0.5, 0.5))
ids = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLD)


@pytest.fixture(scope="module")
def peak_r(gold):
    """The largest relative peak error of the fp32 ``torch.fft`` run over the fixture's cases."""
    r = 0.0
    for key in gold.files:
        if key.startswith("peak32_"):
            r = max(r, float(np.max(np.abs(gold[key] - gold["peak_" + key[7:]]) / np.abs(gold["peak_" + key[7:]]))))
    assert 1e-8 < r < 1e-6
    return r


_pairs = {}


def pair(gold, shape, d):
    """The fixture's inputs of one case, built once."""
    key = (shape, d)
    if key not in _pairs:
        _pairs[key] = R.recipe(shape, d, gold["seed_" + R.case_name(shape, d)])
    return _pairs[key]


@pytest.fixture(scope="module")
def seams(fa, gold):
    """The tile-seam case displaced by (-2.3, 1.7), on the device, with the float64 restatement of its registration."""
    a, b = pair(gold, SEAMS, SEAMS_D)
    return a.cuda(), b.cuda(), R.register_ref(fa, a, b, 10, 8)


def rel_l2(got, want):
    return float((got.detach().double().cpu() - want.double()).norm() / want.double().norm())


def hold(name, got, ref64, ref32, scale=8.0):
    """Print e_ref, e_hip and their ratio, then assert e_hip <= scale e_ref."""
    e_ref, e_hip = rel_l2(ref32, ref64), rel_l2(got, ref64)
    print("REGISTER_ERR %-44s e_ref %.3e e_hip %.3e ratio %.2f (bar %g)" % (name, e_ref, e_hip, e_hip / e_ref, scale))
    assert e_hip <= scale * e_ref, (name, e_hip, e_ref)


def peak_bar(p64, r):
    return 8 * r * abs(float(p64)) + float(np.spacing(np.float32(abs(float(p64)))))


def guarded(ref):
    assert ref["coarse_gap"] >= GAP and ref["refined_gap"] >= GAP, (ref["coarse_gap"], ref["refined_gap"])
    return ref


# ------------------------------------------------------------------------------------------------------------------------
# the surface, the shift and the peak
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_surface_within_the_bar(fa, gold, shape):
    K = fa.radial_bins(shape[2], shape[3])[1].numel()
    for s, d in R.cases():
        if s != shape:
            continue
        a, b = pair(gold, shape, d)
        settings = [(None, "phase")] + ([(K // 2, "phase"), (None, None)] if d == R.DISPLACEMENTS[3] or shape[2] < 8 else [])
        for k_max, norm in settings:
            got = fa.phase_correlation_surface(a.cuda(), b.cuda(), k_max, R.EPS, norm)
            assert got.shape == (shape[0], shape[2], shape[3]) and got.dtype == torch.float32
            hold("surface %s k_max %s %s" % (R.case_name(shape, d), k_max, norm), got, R.surface_ref(fa, a, b, k_max, R.EPS, norm),
                 R.surface_ref(fa, a, b, k_max, R.EPS, norm, torch.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_shift_is_exact_and_peak_within_the_bar(fa, gold, peak_r, shape):
    """Every case at U = 1, 4, 10 and with the ring cut; with C = 2 (37 x 53) the one shift per sample is that of the summed surface."""
    ms = min(8, shape[2] // 2, shape[3] // 2)
    for s, d in R.cases():
        if s != shape:
            continue
        a, b = pair(gold, shape, d)
        for U, k_max, tag in R.fixture_settings(fa, shape):
            ref = guarded(R.register_ref(fa, a, b, U, ms, k_max))
            assert np.array_equal(ref["shift"].numpy(), gold["shift_%s_%s" % (R.case_name(shape, d), tag)])
            shift, peak = fa.phase_correlation(a.cuda(), b.cuda(), U, ms, k_max)
            assert shift.shape == (shape[0], 2) and peak.shape == (shape[0],) and shift.dtype == peak.dtype == torch.float32
            err = (peak.double().cpu() - ref["peak"]).abs()
            print("REGISTER_ERR peak %-28s %-7s shift %s peak rel err %.3e (bar %.3e)"
                  % (R.case_name(shape, d), tag, shift[0].tolist(), float((err / ref["peak"].abs()).max()), 8 * peak_r))
            assert torch.equal(shift.cpu(), ref["shift"].float()), (d, tag, shift.cpu(), ref["shift"])
            for e, p in zip(err.tolist(), ref["peak"].tolist()):
                assert e <= peak_bar(p, peak_r), (d, tag, e, peak_bar(p, peak_r))
            if tag != "U4" and shape[2] > 3:                       # T odd (or no refinement): the exchanged pair gives the negated shift
                back, _ = fa.phase_correlation(b.cuda(), a.cuda(), U, ms, k_max)
                guarded(R.register_ref(fa, b, a, U, ms, k_max))
                assert torch.equal(back.cpu(), -ref["shift"].float()), (d, tag, back.cpu(), ref["shift"])


def test_roll_identity_and_two_calls(fa, gold):
    a, b = (t.cuda() for t in pair(gold, (2, 1, 64, 64), (3, -2)))
    for U in (1, 4, 10):
        shift, peak = fa.phase_correlation(a, torch.roll(a, (3, -2), (-2, -1)), U)
        assert shift.tolist() == [[3.0, -2.0]] * 2
    for shape in ((2, 1, 64, 64), ODD, SEAMS):
        x = pair(gold, shape, (0, 0))[0]
        F = torch.fft.fft2(x.double())
        want = (F.abs() > 0).double().sum((1, 2, 3)) / (shape[1] * shape[2] * shape[3])          # (non-empty bins) / (HW), over C
        for U in (1, 10):
            shift, peak = fa.phase_correlation(x.cuda(), x.cuda(), U)
            ulps = ((peak.double().cpu() - want).abs() / np.spacing(np.float32(1.0))).max()
            print("REGISTER_ERR identity %s U %d peak %s: %.2f ulp of (non-empty bins) / (HW)" % (ids(shape), U, peak.tolist(), float(ulps)))
            assert shift.tolist() == [[0.0, 0.0]] * shape[0] and float(ulps) <= 4
    one, two = fa.phase_correlation(a, b), fa.phase_correlation(a, b)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    assert torch.equal(fa.phase_correlation_surface(a, b), fa.phase_correlation_surface(a, b))
    assert torch.equal(fa.fourier_shift(a, one[0]), fa.fourier_shift(a, one[0]))


def test_max_shift_window_and_all_nan(fa, gold):
    a, b = (t.cuda() for t in pair(gold, (2, 1, 64, 64), (3, -2)))
    assert fa.phase_correlation(a, b, 1, 8)[0].tolist() == [[3.0, -2.0]] * 2
    assert fa.phase_correlation(a, b, 1, (3, 2))[0].tolist() == [[3.0, -2.0]] * 2
    assert fa.phase_correlation(a, b, 1, 0)[0].tolist() == [[0.0, 0.0]] * 2
    for ms in (2, (8, 1)):
        d = fa.phase_correlation(a, b, 10, ms)[0].cpu()
        ref = R.register_ref(fa, a.cpu(), b.cpu(), 10, ms)
        my, mx = (ms, ms) if isinstance(ms, int) else ms
        assert torch.equal(d, ref["shift"].float()) and float(d[:, 0].abs().max()) <= my + 0.75 and float(d[:, 1].abs().max()) <= mx + 0.75
    nan = torch.full_like(a, float("nan"))
    shift, peak = fa.phase_correlation(a, nan, 10)                 # a NaN never wins: position 0, and the peak says so
    assert shift.tolist() == [[0.0, 0.0]] * 2 and bool(peak.isnan().all())
    shift, peak = fa.phase_correlation(a, nan, 1)
    assert shift.tolist() == [[0.0, 0.0]] * 2 and bool(peak.isnan().all())


# ------------------------------------------------------------------------------------------------------------------------
# the Fourier shift
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fourier_shift_and_its_gradients_within_the_bar(fa, gold, shape):
    x = pair(gold, shape, (0, 0))[0]
    g = torch.Generator().manual_seed(11)
    cot = torch.randn(*shape, generator=g)
    for d in SHIFTS:
        xd = x.cuda().requires_grad_(True)
        y = fa.fourier_shift(xd, d)
        assert y.shape == x.shape and y.dtype == torch.float32
        x64 = x.double().requires_grad_(True)
        y64 = R.fourier_shift_ref(x64, d)
        y32 = R.fourier_shift_ref(x, d, torch.float32)
        hold("fourier_shift %s d %s" % (ids(shape), d), y, y64.detach(), y32)
        if d == (0.0, 0.0):
            hold("fourier_shift %s zero shift against x" % ids(shape), y, x.double(), y32)
        if d == (3.0, -2.0):
            hold("fourier_shift %s against torch.roll" % ids(shape), y, torch.roll(x.double(), (3, -2), (-2, -1)), y32)
        # the gradients against autograd of the float64 restatement: a scalar cotangent (of the sum) and a random one
        e_random = None
        for name, c in (("random", cot), ("scalar", torch.full(shape, 0.75))):
            gx, = torch.autograd.grad(y, xd, c.cuda(), retain_graph=True)
            g64, = torch.autograd.grad(y64, x64, c.double(), retain_graph=True)
            x32 = x.clone().requires_grad_(True)
            g32, = torch.autograd.grad(R.fourier_shift_ref(x32, d, torch.float32), x32, c)
            if name == "random":
                e_random = rel_l2(g32, g64)
                hold("fourier_shift grad random %s d %s" % (ids(shape), d), gx, g64, g32)
            else:
                # a constant cotangent has a DC term alone, which an FFT carries exactly: the fp32 run's own error for this array can be
                # zero, so the yardstick is its error for the random cotangent of the same shape and shift
                e_hip = rel_l2(gx, g64)
                print("REGISTER_ERR %-44s e_ref %.3e (random cotangent; own %.3e) e_hip %.3e ratio %.2f"
                      % ("fourier_shift grad scalar %s d %s" % (ids(shape), d), e_random, rel_l2(g32, g64), e_hip, e_hip / e_random))
                assert e_hip <= 8 * e_random, (e_hip, e_random)
        # a tensor shift and the same pair of floats give the same bits
        t = torch.tensor([list(d)] * shape[0], device="cuda")
        assert torch.equal(fa.fourier_shift(x.cuda(), t), y.detach())
        # there and back, within twice the bar
        back = fa.fourier_shift(y.detach(), (-d[0], -d[1]))
        b64 = R.fourier_shift_ref(y64.detach(), (-d[0], -d[1]))
        b32 = R.fourier_shift_ref(R.fourier_shift_ref(x, d, torch.float32), (-d[0], -d[1]), torch.float32)
        hold("fourier_shift there and back %s d %s" % (ids(shape), d), back, b64, b32, 16.0)
        if shape[2] % 2 and shape[3] % 2:
            hold("fourier_shift there and back %s d %s against x" % (ids(shape), d), back, x.double(), b32, 16.0)


def test_fourier_shift_per_sample_and_no_gradient_to_the_shift(fa, gold):
    x = pair(gold, SEAMS, (0, 0))[0]
    t = torch.tensor([[1.25, -0.5], [-3.0, 2.75]])
    y = fa.fourier_shift(x.cuda(), t.cuda())
    hold("fourier_shift per-sample shifts", y, R.fourier_shift_ref(x, t), R.fourier_shift_ref(x, t, torch.float32))
    with pytest.raises(fa.KernelError, match="follow-up"):
        fa.fourier_shift(x.cuda(), t.cuda().requires_grad_(True))
    with pytest.raises(fa.KernelError, match=r"\(N, 2\)"):
        fa.fourier_shift(x.cuda(), t[:1].cuda())
    with pytest.raises(fa.KernelError, match=r"\(N, 2\)"):
        fa.fourier_shift(x.cuda(), t)                               # on the host


# ------------------------------------------------------------------------------------------------------------------------
# Registered, RegistrationShift and the evaluation path
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("SSIM", "FRC", "HaarPSI"))
def test_registered_is_the_composition(fa, seams, which):
    a, b, ref = seams
    guarded(ref)
    m = getattr(fa, which)()
    reg = fa.Registered(m)
    crop = lambda t: t[..., 9:-9, 9:-9].contiguous()
    ad, bd = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    got = reg.index(ad, bd, True)
    d, _ = fa.phase_correlation(a, b, 10, 8)
    assert torch.equal(d.cpu(), ref["shift"].float())
    a2, b2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = m.index(crop(a2), crop(fa.fourier_shift(b2, -d)), True)
    assert got.shape == (2,) and torch.equal(got, want)
    w = torch.tensor([0.75, -1.25], device="cuda")
    ga, gb = torch.autograd.grad(got, (ad, bd), w)
    wa, wb = torch.autograd.grad(want, (a2, b2), w)
    assert float(ga.abs().max()) > 0 and float(gb.abs().max()) > 0          # gradients reach both inputs
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
    assert bool((ga[..., :9, :] == 0).all()) and bool((ga[..., :, -9:] == 0).all())      # nothing outside the crop for img1
    assert float(gb[..., :9, :].abs().max()) > 0                           # the shift's adjoint spreads img2's gradient over the plane
    assert torch.equal(reg(a, b), m(crop(a), crop(fa.fourier_shift(b, -d))))


def test_registration_raises_the_frc_index(fa, gold, seams):
    """Misregistered by (-2.3, 1.7), the FRC index of the seam case is pulled down; registered, it recovers.  The float64 fixture
    asserts the same ordering first."""
    a, b, ref = seams
    assert (gold["frc_registered"] > gold["frc_unregistered"]).all()
    crop = lambda t: t[..., 9:-9, 9:-9].contiguous()
    frc = fa.FRC()
    reg, raw = fa.Registered(frc).index(a, b, True), frc.index(crop(a), crop(b), True)
    print("REGISTER_ERR FRC of the seam case: registered %s (float64 %s), unregistered %s (float64 %s)"
          % (reg.tolist(), gold["frc_registered"].tolist(), raw.tolist(), gold["frc_unregistered"].tolist()))
    assert bool((reg > raw).all())
    np.testing.assert_allclose(reg.cpu().numpy(), gold["frc_registered"], rtol=1e-4)
    np.testing.assert_allclose(raw.cpu().numpy(), gold["frc_unregistered"], rtol=1e-4, atol=1e-6)
    dist = fa.RegistrationShift().index(a, b, True)
    want = ref["shift"].float().square().sum(1).sqrt()
    assert torch.equal(dist.cpu(), want) and float(fa.RegistrationShift()(a, b)) == pytest.approx(float(want.mean()), rel=1e-6)
    assert want.tolist() == pytest.approx([float(np.hypot(2.3, 1.7))] * 2, rel=1e-6)


def test_evaluate_pairs_with_keys(fa, gold, seams, monkeypatch):
    """``evaluate_pairs_with(model, pairs, frc=Registered(FRC()), frc_cutoff=Registered(FRCResolution()), shift=RegistrationShift())``
    adds the three keys, unchanged otherwise.  ``super_resolve`` is replaced by the identity (the generator is not bit-reproducible)."""
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: lr)
    a, b, _ = seams
    pairs = [(b.clamp(-1, 1), a.clamp(-1, 1)), (a[:1].clamp(-1, 1), b[:1].clamp(-1, 1))]
    plain = fa.evaluate_pairs(None, pairs)
    mods = dict(frc=fa.Registered(fa.FRC()), frc_cutoff=fa.Registered(fa.FRCResolution()), shift=fa.RegistrationShift())
    out = fa.evaluate_pairs_with(None, pairs, **mods)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "frc", "frc_cutoff", "shift"] and all(out[k] == plain[k] for k in plain)
    with torch.no_grad():
        want = {k: float(torch.cat([m.index(lr, hr, True).double() for lr, hr in pairs]).mean()) for k, m in mods.items()}
    print("REGISTER_ERR evaluate_pairs_with: frc %.9f frc_cutoff %.9f shift %.9f px" % (out["frc"], out["frc_cutoff"], out["shift"]))
    assert all(out[k] == pytest.approx(want[k], rel=1e-12) for k in mods)
    assert out["frc"] > float(fa.FRC()(pairs[0][0], pairs[0][1])) and 2.5 < out["shift"] < 3.2


# ------------------------------------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------------------------------------
def test_capturable_with_the_shift_kept_on_the_device(fa, seams):
    """``phase_correlation`` followed by ``fourier_shift`` in one hipGraph: the shift never visits the host, nothing is allocated or
    read there, and every launch goes to the capturing stream in program order (a chain: the capture has no parallel branches).
    The replay reproduces the eager bits."""
    a, b, _ = seams
    d0, p0 = fa.phase_correlation(a, b, 10, 8)                     # warm-up: the tables exist before the capture
    y0 = fa.fourier_shift(b, -d0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d, p = fa.phase_correlation(a, b, 10, 8)
        y = fa.fourier_shift(b, -d)
    for t in (d, p, y):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d, d0) and torch.equal(p, p0) and torch.equal(y, y0)
