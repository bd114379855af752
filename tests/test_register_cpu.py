"""Host-side checks of phase-correlation registration and the Fourier shift (Kuglin & Hines 1975; Guizar-Sicairos, Thurman & Fienup
2008): the ``torch.fft`` restatement the GPU tests lean on, pinned in float64 to the fixture (tests/golden/golden_register.npz, written
by tools/gen_golden_register.py in numpy from explicit DFT matrices); hand-made cases of the definition (impulses, rolls, the
wrap-around sign at H//2, the ``max_shift`` window, the ``k_max`` cut); the public names, the host-side refusals and the C ABI's
argument checks.

The inputs are rebuilt from the seed the fixture records.  The generator displaces ``a`` through DFT matrices and this file through
``torch.fft``, so an input can differ from the generator's in its last fp32 bit; the arg-max guards (both maxima lead their runner-up
by 2^-12 of their value, re-asserted here) make every shift exact all the same, and values are held at 1e-6."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_register.npz")
NEW_SYMBOLS = ("faoctasr_pcorr_workspace_floats", "faoctasr_pcorr_fwd", "faoctasr_fourier_shift", "faoctasr_fourier_shift_workspace_floats")
SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
DISPLACEMENTS = ((0, 0), (1, -1), (3, -2), (-2.3, 1.7), (0.4, -0.6), (2.5, -0.5))
UPSAMPLE = (1, 4, 10)
SURFACES = (((2, 1, 8, 8), (1, -1)), ((1, 2, 37, 53), (-2.3, 1.7)), ((2, 1, 72, 136), (2.5, -0.5)))
EPS = 1e-16
GAP = 2.0 ** -12


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


@pytest.fixture(scope="module")
def lib(fa):
    return fa._lib.load()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def cases():
    return [(s, d) for s in SHAPES for d in DISPLACEMENTS if abs(d[0]) < s[2] / 2 and abs(d[1]) < s[3] / 2]


def case_name(shape, d):
    return "x".join(str(s) for s in shape) + "_" + "_".join(("%g" % v).replace("-", "m").replace(".", "p") for v in d)


def signed(n):
    """The indices of ``numpy.fft.fftfreq(n) * n``: Nyquist at -n/2."""
    return (torch.arange(n) + n // 2) % n - n // 2


def position(n):
    """The signed position of every index of a correlation surface: positions > n//2 wrap negative (n//2 itself stays positive)."""
    p = torch.arange(n)
    return torch.where(p > n // 2, p - n, p)


def smooth(t, r):
    return sum(torch.roll(t, (dy, dx), (-2, -1)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / (2 * r + 1) ** 2


def fourier_shift_ref(x, d, dtype=torch.float64):
    """``Re ifft2(fft2(x) exp(-2 pi i (f_u d_y + f_v d_x)))`` on the CPU in ``dtype`` (differentiable in x); d a pair or (N, 2)."""
    N, _, H, W = x.shape
    d = torch.as_tensor(d, dtype=torch.float64).reshape(-1, 2).expand(N, 2)
    ph = signed(H).double()[None, :, None] * d[:, 0, None, None] / H + signed(W).double()[None, None, :] * d[:, 1, None, None] / W
    ramp = torch.polar(torch.ones_like(ph), -2 * math.pi * ph)[:, None]
    return torch.fft.ifft2(torch.fft.fft2(x.to(dtype)) * ramp.to(torch.complex64 if dtype == torch.float32 else torch.complex128)).real


def recipe(shape, d, seed=0):
    """The fixture's inputs: a = 2 smooth(rn, 2) + 0.25 rn; b0 = shift(a, d) + 0.3 rn; b = 0.7 smooth(b0, 1) + 0.3 b0; as fp32."""
    g = torch.Generator().manual_seed(int(seed))
    rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64)
    a = 2 * smooth(rn(), 2) + 0.25 * rn()
    b0 = fourier_shift_ref(a, d) + 0.3 * rn()
    return a.float(), (0.7 * smooth(b0, 1) + 0.3 * b0).float()


def cross_power(fa, a, b, k_max=None, eps=EPS, normalization="phase", dtype=torch.float64):
    H, W = a.shape[-2:]
    F, G = torch.fft.fft2(a.detach().cpu().to(dtype)), torch.fft.fft2(b.detach().cpu().to(dtype))
    R = G * F.conj() / (H * W)
    if normalization == "phase":
        R = R / torch.sqrt(R.real ** 2 + R.imag ** 2 + eps)
    if k_max is not None:
        R = torch.where(fa.radial_bins(H, W)[0] > k_max, torch.zeros((), dtype=R.dtype), R)
    return R


def surface_ref(fa, a, b, k_max=None, eps=EPS, normalization="phase", dtype=torch.float64):
    return torch.fft.ifft2(cross_power(fa, a, b, k_max, eps, normalization, dtype)).real.sum(1)


def first_max(plane, allowed=None):
    """(flat index of the first maximum in row-major order, its value, (value - runner-up) / value) among the allowed positions."""
    flat = plane.detach().double().numpy().reshape(-1).copy()
    if allowed is not None:
        flat[~allowed.numpy().reshape(-1)] = -np.inf
    i = int(np.argmax(flat))
    top = float(flat[i])
    flat[i] = -np.inf
    return i, top, ((top - float(flat.max())) / top if flat.size > 1 else 1.0)


def register_ref(fa, a, b, upsample=10, max_shift=None, k_max=None, eps=EPS, normalization="phase", dtype=torch.float64):
    """``phase_correlation`` by its definition on the CPU in ``dtype``: dict of shift (N, 2) and peak (N,) as float64, the surface, and
    the smallest relative lead of the coarse and of the refined maximum over their runners-up."""
    N, C, H, W = a.shape
    Wh, U = W // 2 + 1, upsample
    my, mx = (H // 2, W // 2) if max_shift is None else ((max_shift, max_shift) if isinstance(max_shift, int) else max_shift)
    Rn = cross_power(fa, a, b, k_max, eps, normalization, dtype)
    surf = torch.fft.ifft2(Rn).real.sum(1)
    wy, wx, py, px = signed(H), signed(W), position(H), position(W)
    allowed = (py.abs()[:, None] <= my) & (px.abs()[None, :] <= mx)
    mv = torch.tensor([1.0 if v == 0 or 2 * v == W else 2.0 for v in range(Wh)], dtype=dtype)
    T = -(-3 * U // 2)
    j = torch.arange(T) - T // 2
    shift, peak, gc, gr = torch.zeros(N, 2, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), 1.0, 1.0
    for n in range(N):
        i, top, gap = first_max(surf[n], allowed)
        gc = min(gc, gap)
        sy, sx = int(py[i // W]), int(px[i % W])
        shift[n, 0], shift[n, 1], peak[n] = sy, sx, top / C
        if U == 1:
            continue
        ey = torch.polar(torch.ones(T, H, dtype=torch.float64), 2 * math.pi * ((wy[None, :] * (sy * U + j)[:, None]) % (U * H)).double() / (U * H))
        ex = torch.polar(torch.ones(Wh, T, dtype=torch.float64), 2 * math.pi * ((wx[:Wh, None] * (sx * U + j)[None, :]) % (U * W)).double() / (U * W))
        up = sum((ey.to(Rn.dtype) @ (Rn[n, c][:, :Wh] * mv[None, :]) @ ex.to(Rn.dtype)).real for c in range(C)) / (H * W)
        i, top, gap = first_max(up)
        gr = min(gr, gap)
        shift[n, 0], shift[n, 1], peak[n] = (sy * U + int(j[i // T])) / U, (sx * U + int(j[i % T])) / U, top / C
    return dict(shift=shift, peak=peak, surface=surf.double(), coarse_gap=gc, refined_gap=gr)


def fixture_settings(fa, shape):
    K = fa.radial_bins(shape[2], shape[3])[1].numel()
    return [(U, None, "U%d" % U) for U in UPSAMPLE] + [(10, K // 2, "U10_cut")]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_reproduces_the_fixture(fa, gold, shape):
    for s, d in cases():
        if s != shape:
            continue
        name = case_name(shape, d)
        a, b = recipe(shape, d, gold["seed_" + name])
        ms = min(8, shape[2] // 2, shape[3] // 2)
        for U, k_max, tag in fixture_settings(fa, shape):
            ref = register_ref(fa, a, b, U, ms, k_max)
            assert ref["coarse_gap"] >= GAP and ref["refined_gap"] >= GAP, (name, tag, ref["coarse_gap"], ref["refined_gap"])
            assert np.array_equal(ref["shift"].numpy(), gold["shift_%s_%s" % (name, tag)]), (name, tag)
            np.testing.assert_allclose(ref["peak"].numpy(), gold["peak_%s_%s" % (name, tag)], rtol=1e-6, atol=0)
            if k_max is not None:
                assert int(gold["kmax_%s_%s" % (name, tag)]) == k_max
            r32 = register_ref(fa, a, b, U, ms, k_max, dtype=torch.float32)
            assert np.array_equal(r32["shift"].numpy(), ref["shift"].numpy()), (name, tag)          # the fp32 run finds the same shift
        if (shape, d) in SURFACES:
            want = torch.from_numpy(gold["surface_" + name])
            got = surface_ref(fa, a, b)
            assert float((got - want).norm() / want.norm()) <= 1e-6


def test_fixture_holds_every_case_and_is_small(gold):
    assert os.path.getsize(GOLD) < 1 << 20
    assert sum(k.startswith("surface_") for k in gold.files) == 3
    for shape, d in cases():
        name = case_name(shape, d)
        for tag in ("U1", "U4", "U10", "U10_cut"):
            assert gold["shift_%s_%s" % (name, tag)].shape == (shape[0], 2) and gold["peak_%s_%s" % (name, tag)].shape == (shape[0],)
            assert gold["peak32_%s_%s" % (name, tag)].shape == (shape[0],)
    assert len(cases()) == 32
    # from 37 x 53 upward every displacement is recovered exactly on the 0.1 grid at U = 10
    for shape, d in cases():
        if shape[2] >= 37:
            np.testing.assert_allclose(gold["shift_%s_U10" % case_name(shape, d)], np.tile(np.float64(d), (shape[0], 1)), rtol=0, atol=1e-12)
    assert (gold["frc_registered"] > gold["frc_unregistered"]).all()


def test_impulse_pair_and_roll(fa):
    a = torch.zeros(1, 1, 9, 12)
    a[0, 0, 2, 3] = 1.0
    b = torch.zeros(1, 1, 9, 12)
    b[0, 0, 5, 1] = 1.0                                           # b(p) = a(p - d), d = (3, -2)
    for U in (1, 4, 10):
        ref = register_ref(fa, a, b, U)
        assert ref["shift"].tolist() == [[3.0, -2.0]] and abs(float(ref["peak"]) - 1.0) < 1e-7
    s = surface_ref(fa, a, b)[0]
    assert abs(float(s[3, 10]) - 1.0) < 1e-7 and float((s.abs() > 1e-7).sum()) == 1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 2, 16, 20, generator=g)
    y = torch.roll(x, (3, -2), (-2, -1))
    ref = register_ref(fa, x, y)
    assert ref["shift"].tolist() == [[3.0, -2.0]] * 2
    assert register_ref(fa, y, x)["shift"].tolist() == [[-3.0, 2.0]] * 2
    np.testing.assert_allclose(ref["peak"].numpy(), 1.0, rtol=1e-6)                # the value over C
    same = register_ref(fa, x, x)
    assert same["shift"].tolist() == [[0.0, 0.0]] * 2
    # an integer shift of the restated fourier_shift is a roll; a shift and its inverse return the image
    np.testing.assert_allclose(fourier_shift_ref(x, (3, -2)).numpy(), y.double().numpy(), atol=1e-12)
    # the real part scales a Nyquist bin by cos(pi d), so only odd sides (no Nyquist bin) return exactly from a fractional shift
    z = torch.randn(2, 2, 15, 21, generator=g, dtype=torch.float64)
    back = fourier_shift_ref(fourier_shift_ref(z, (-2.3, 1.7)), (2.3, -1.7))
    np.testing.assert_allclose(back.numpy(), z.numpy(), atol=1e-12)
    back = fourier_shift_ref(fourier_shift_ref(x, (-2.3, 1.7)), (2.3, -1.7))
    assert float((back - x.double()).abs().max()) > 1e-3           # 16 x 20: the Nyquist row and column came back scaled by cos^2


@pytest.mark.parametrize("H", (8, 9))
def test_wrap_around_sign_at_half_the_side(fa, H):
    g = torch.Generator().manual_seed(H)
    x = torch.randn(1, 1, H, H, generator=g)
    for s in range(H):
        want = s if s <= H // 2 else s - H                         # positions > H//2 wrap negative: H//2 itself stays positive
        ref = register_ref(fa, x, torch.roll(x, (s, 0), (-2, -1)), 1)
        assert ref["shift"].tolist() == [[float(want), 0.0]], (s, ref["shift"])
        ref = register_ref(fa, x, torch.roll(x, (0, s), (-2, -1)), 1)
        assert ref["shift"].tolist() == [[0.0, float(want)]], (s, ref["shift"])


def test_max_shift_window(fa):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 1, 32, 32, generator=g)
    y = torch.roll(x, (6, -3), (-2, -1))
    assert register_ref(fa, x, y, 1, 8)["shift"].tolist() == [[6.0, -3.0]]
    assert register_ref(fa, x, y, 1, (6, 3))["shift"].tolist() == [[6.0, -3.0]]
    for ms in (5, (8, 2), 0):
        d = register_ref(fa, x, y, 1, ms)["shift"][0]
        my, mx = (ms, ms) if isinstance(ms, int) else ms
        assert abs(float(d[0])) <= my and abs(float(d[1])) <= mx and d.tolist() != [6.0, -3.0]
    assert register_ref(fa, x, y, 1, 0)["shift"].tolist() == [[0.0, 0.0]]


def test_k_max_cut_zeroes_exactly_the_rings_above_it(fa):
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(1, 1, 12, 18, generator=g), torch.randn(1, 1, 12, 18, generator=g)
    bins, cnt = fa.radial_bins(12, 18)
    K = cnt.numel()
    for k_max in (0, 3, K - 2, K - 1):
        Rn = cross_power(fa, x, y, k_max)[0, 0]
        assert bool((Rn[bins > k_max] == 0).all()) and bool((Rn[bins <= k_max].abs() > 0.5).all())
        assert int((Rn != 0).sum()) == int(cnt[:k_max + 1].sum())
    assert torch.equal(cross_power(fa, x, y, K - 1), cross_power(fa, x, y, None))
    z = torch.randn(1, 1, 12, 12, generator=g)
    s = surface_ref(fa, z, z, 0)                                   # a square plane's ring 0 is DC alone: a flat surface of 1 / (HW)
    np.testing.assert_allclose(s.numpy(), 1.0 / 144, rtol=1e-9)


def test_public_names_and_signatures(fa):
    for name in ("phase_correlation", "phase_correlation_surface", "fourier_shift", "Registered", "RegistrationShift"):
        assert name in fa.__all__ and callable(getattr(fa, name)), name
    assert fa.phase_correlation is fa.ops.phase_correlation and fa.fourier_shift is fa.ops.fourier_shift
    assert fa.phase_correlation_surface is fa.ops.phase_correlation_surface
    assert fa.Registered is fa.ssim.Registered and fa.RegistrationShift is fa.ssim.RegistrationShift
    sig = inspect.signature(fa.phase_correlation)
    assert list(sig.parameters) == ["a", "b", "upsample", "max_shift", "k_max", "eps", "normalization"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [10, None, None, 1e-16, "phase"]
    sig = inspect.signature(fa.phase_correlation_surface)
    assert list(sig.parameters) == ["a", "b", "k_max", "eps", "normalization"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, 1e-16, "phase"]
    assert list(inspect.signature(fa.fourier_shift).parameters) == ["x", "shift"]
    sig = inspect.signature(fa.Registered.__init__)
    assert list(sig.parameters) == ["self", "index", "max_shift", "upsample", "k_max"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [8, 10, None]
    sig = inspect.signature(fa.RegistrationShift.__init__)
    assert list(sig.parameters) == ["self", "max_shift", "upsample", "k_max"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [8, 10, None]
    for m in (fa.Registered(fa.FRC()), fa.RegistrationShift()):
        assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(m.buffers())
        assert list(inspect.signature(m.forward).parameters) == ["img1", "img2"]
        assert list(inspect.signature(m.index).parameters) == ["img1", "img2", "per_image"]
    assert "skimage" in fa.phase_correlation.__doc__ and "-d" in fa.phase_correlation.__doc__
    assert fa.RegistrationShift(4, 20, 9).extra_repr() == "max_shift=4, upsample=20, k_max=9"
    assert "Registered" not in "".join(inspect.signature(fa.TrainStep.__init__).parameters)         # registration is not a loss
    assert len(fa.train.OPT_IN_TERMS) == 16


def test_host_side_refusals(fa):
    """Each refusal comes before any device call: none of these needs a GPU, and there is no CPU fallback."""
    x = torch.rand(2, 1, 32, 32)
    pc = fa.phase_correlation
    for bad in (0, 101, -1, 10.0, "10", None, True):
        with pytest.raises(ValueError, match="upsample"):
            pc(x, x, upsample=bad)
        with pytest.raises(ValueError, match="upsample"):
            fa.Registered(fa.FRC(), upsample=bad)
    for bad in (17, -1, (4, 17), (4,), (1, 2, 3), 4.0, "4", True, (True, 1)):
        with pytest.raises(ValueError, match="max_shift"):
            pc(x, x, max_shift=bad)
    for bad in (-1, 4.0, "4", None, True):
        with pytest.raises(ValueError, match="max_shift"):
            fa.Registered(fa.FRC(), max_shift=bad)
    K = fa.radial_bins(32, 32)[1].numel()
    for bad in (-1, K, 3.0, "3", True):
        with pytest.raises(ValueError, match="k_max"):
            pc(x, x, k_max=bad)
        with pytest.raises(ValueError, match="k_max"):
            fa.phase_correlation_surface(x, x, k_max=bad)
    for bad in (-1e-16, float("nan"), float("inf"), "1e-16", None, True):
        with pytest.raises(ValueError, match="eps"):
            pc(x, x, eps=bad)
    for bad in ("none", "magnitude", 0, False):
        with pytest.raises(ValueError, match="normalization"):
            pc(x, x, normalization=bad)
    with pytest.raises(fa.KernelError, match=r"\(N,C,H,W\)"):
        pc(x[0], x[0])
    with pytest.raises(fa.KernelError, match="fp32"):
        pc(x.double(), x.double())
    with pytest.raises(fa.KernelError, match="one shape"):
        pc(x, x[:, :, :16])
    with pytest.raises(fa.KernelError, match="fp32"):
        fa.fourier_shift(x.double(), (1.0, 2.0))
    for bad in ((1.0,), (1.0, float("nan")), "ab", None, 1.0):
        with pytest.raises(ValueError, match="shift"):
            fa.fourier_shift(x, bad)
    for call in (lambda: pc(x, x), lambda: fa.phase_correlation_surface(x, x), lambda: fa.fourier_shift(x, (1.0, 2.0)),
                 lambda: fa.Registered(fa.FRC())(x, x), lambda: fa.Registered(fa.SSIM()).index(x, x, True), lambda: fa.RegistrationShift()(x, x)):
        with pytest.raises(fa.KernelError, match="GPU"):
            call()
    small = torch.rand(1, 1, 18, 40)
    with pytest.raises(ValueError, match="sides must exceed"):
        fa.Registered(fa.FRC())(small, small)                      # 18 <= 2 (8 + 1)


def test_new_symbols_in_header_and_library(fa, lib):
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in fa._lib.declared_symbols(), s
        assert hasattr(lib, s), s


def test_workspace_queries(lib):
    K, T = 182, 15
    n = lib.faoctasr_pcorr_workspace_floats(8, 1, 256, 256, 129, K, 10)
    # [P | Q] of two images, Rn, the surface, the two twiddle tables, the refinement's [T1 | T2], the coarse peak
    assert n == 8 * (2 * 256 * 258 + 2 * 256 * 129 + 256 * 256 + 256 * 2 * T + 2 * 129 * T + T * 258 + 2)
    assert lib.faoctasr_pcorr_workspace_floats(8, 1, 256, 256, 129, K, 1) == 8 * (2 * 256 * 258 + 2 * 256 * 129 + 256 * 256 + 2)
    assert lib.faoctasr_pcorr_workspace_floats(1, 1, 2, 3, 2, 2, 100) > 0
    for bad in (0, 101, -3):
        assert lib.faoctasr_pcorr_workspace_floats(8, 1, 256, 256, 129, K, bad) < 0 and b"upsample" in lib.faoctasr_last_error()
    assert lib.faoctasr_pcorr_workspace_floats(1, 1, 1, 64, 33, 2, 10) < 0 and b"H" in lib.faoctasr_last_error()
    assert lib.faoctasr_pcorr_workspace_floats(1, 1, 8, 8, 8, 6, 10) < 0 and b"Wh" in lib.faoctasr_last_error()      # no full-spectrum switch
    assert lib.faoctasr_pcorr_workspace_floats(1, 1, 8, 8, 5, 7, 10) < 0 and b"radial bins" in lib.faoctasr_last_error()
    assert lib.faoctasr_pcorr_workspace_floats(1, 1, 1025, 8, 5, 6, 10) < 0 and b"1024" in lib.faoctasr_last_error()
    assert lib.faoctasr_pcorr_workspace_floats(40000, 1, 8, 8, 5, 6, 10) < 0 and b"65535" in lib.faoctasr_last_error()
    assert lib.faoctasr_fourier_shift_workspace_floats(8, 1, 256, 256) == 8 * 256 * 129 * 5
    assert lib.faoctasr_fourier_shift_workspace_floats(1, 1, 1, 64) < 0 and b"H" in lib.faoctasr_last_error()
    assert lib.faoctasr_fourier_shift_workspace_floats(1, 1, 8, 1025) < 0 and b"1024" in lib.faoctasr_last_error()
    assert lib.faoctasr_fourier_shift_workspace_floats(70000, 1, 8, 8) < 0 and b"65535" in lib.faoctasr_last_error()


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    fwd = lambda *a: lib.faoctasr_pcorr_fwd(*a)
    L = lambda H=64, W=64, Wh=33, K=46, eps=1e-16, k_max=45, U=10, my=8, mx=8: [p, p, p, p, p, eps, k_max, 1, U, my, mx, p, p, p, p, 1, 1, H, W, Wh, K,
                                                                                 None]
    for H, W in ((1, 64), (64, 1)):
        assert fwd(*L(H=H, W=W)) == -1 and b"pcorr_fwd" in lib.faoctasr_last_error()
    assert fwd(*L(H=1025)) == -2 and b"1024" in lib.faoctasr_last_error()
    assert fwd(*L(Wh=32)) == -1 and b"Wh" in lib.faoctasr_last_error()
    assert fwd(*L(Wh=64)) == -1 and b"Wh" in lib.faoctasr_last_error()
    assert fwd(*L(K=45, k_max=44)) == -1 and b"radial bins" in lib.faoctasr_last_error()
    for U in (0, 101, -1):
        assert fwd(*L(U=U)) == -1 and b"upsample" in lib.faoctasr_last_error()
    for my, mx in ((-1, 8), (8, -1), (33, 8), (8, 33)):
        assert fwd(*L(my=my, mx=mx)) == -1 and b"max_shift" in lib.faoctasr_last_error()
    for k_max in (-1, 46):
        assert fwd(*L(k_max=k_max)) == -1 and b"k_max" in lib.faoctasr_last_error()
    for eps in (-1.0, float("nan"), float("inf")):
        assert fwd(*L(eps=eps)) == -1 and b"eps" in lib.faoctasr_last_error()
    for k in (0, 1, 2, 3, 4, 14):                                 # a, b, tabH, halfW, binmap, workspace
        a = L()
        a[k] = None
        assert fwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    for k in (11, 12):                                            # shift without peak, peak without shift
        a = L()
        a[k] = None
        assert fwd(*a) == -1 and b"go together" in lib.faoctasr_last_error()
    a = L()
    a[11] = a[12] = a[13] = None                                  # neither a shift nor a surface asked for
    assert fwd(*a) == -1 and b"surface" in lib.faoctasr_last_error()
    fs = lambda *a: lib.faoctasr_fourier_shift(*a)
    S = lambda H=64, W=64, sign=1.0: [p, p, sign, p, p, p, p, 1, 1, H, W, None]
    for H, W in ((1, 64), (64, 1)):
        assert fs(*S(H=H, W=W)) == -1 and b"fourier_shift" in lib.faoctasr_last_error()
    assert fs(*S(W=1025)) == -2 and b"1024" in lib.faoctasr_last_error()
    for sign in (0.0, 2.0, float("nan")):
        assert fs(*S(sign=sign)) == -1 and b"sign" in lib.faoctasr_last_error()
    for k in (0, 1, 3, 4, 5, 6):
        a = S()
        a[k] = None
        assert fs(*a) == -1 and b"null" in lib.faoctasr_last_error(), k


def test_generator_script_is_independent_of_package_and_tests():
    with open(os.path.join(ROOT, "tools", "gen_golden_register.py")) as f:
        src = f.read()
    imports = re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, re.M)
    assert sorted(set(imports)) == ["math", "numpy", "os", "torch"]
    assert "faoctasr" not in src and "radial_bins" not in src and "np.fft" not in src
    assert "dft(x.shape[-2]) @ x @ dft(x.shape[-1])" in src and "range(2000)" in src and "GAP = 2.0 ** -12" in src
