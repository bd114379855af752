"""Host-side checks of the Fourier ring correlation (Saxton & Baumeister 1982; van Heel & Schatz 2005): the float64 ``torch.fft`` +
``index_add_`` restatement the GPU tests lean on, pinned to the fixture (tests/golden/golden_frc.npz, written by
tools/gen_golden_frc.py from explicit DFT matrices and a loop over the rings); the cutoff read-out ``frc_cutoff`` on hand-made curves;
the band-limit check (noise that shares its spectrum only below ring k0 loses its correlation at k0); the public names, the
host-side refusals and the C ABI's argument checks."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_frc.npz")
NEW_SYMBOLS = ("faoctasr_frc_workspace_floats", "faoctasr_frc_fwd", "faoctasr_frc_bwd")
SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
GRADIENTS = {(1, 1, 2, 3): (0, 1, 2), (2, 1, 8, 8): (0, 1, 2), (1, 2, 37, 53): (0,)}
BAND_LIMIT = ((64, 64, 16), (65, 63, 12), (72, 136, 20))
EPS = 1e-16


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


def bands_of(fa, H, W):
    """The three settings of the fixture: (1, None -> M//2), (0, K-1), (2, max(M//4, 2)), clipped into [0, K-1]."""
    K, M = fa.radial_bins(H, W)[1].numel(), min(H, W)
    out = []
    for a, b in ((1, M // 2), (0, K - 1), (2, max(M // 4, 2))):
        a = min(a, K - 1)
        out.append((a, max(a, min(b, K - 1))))
    return out


def ring_means(fa, x, y):
    """(Nk, Xk, Yk), each (N, C, K), through ``torch.fft.fft2`` and ``index_add_`` in x's dtype (differentiable)."""
    N, C, H, W = x.shape
    bins, cnt = fa.radial_bins(H, W)
    F, G = torch.fft.fft2(x), torch.fft.fft2(y)
    planes = ((F.real * G.real + F.imag * G.imag) / (H * W), (F.real ** 2 + F.imag ** 2) / (H * W), (G.real ** 2 + G.imag ** 2) / (H * W))
    return tuple(torch.zeros(N, C, cnt.numel(), dtype=x.dtype).index_add_(2, bins.flatten(), q.reshape(N, C, H * W)) / cnt.to(x.dtype)
                 for q in planes)


def restatement(fa, x, y, k_min=1, k_max=None, eps=EPS, dtype=torch.float64):
    """The definition on the CPU in ``dtype``: dict of index, per, gx, gy, curve, Xk, Yk as float64."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(True)
    if k_max is None:
        k_max = min(x.shape[-2:]) // 2
    Nk, Xk, Yk = ring_means(fa, x, y)
    curve = Nk / torch.sqrt(Xk * Yk + eps)
    per = curve[..., k_min:k_max + 1].mean((1, 2))
    index = per.mean()
    gx, gy = torch.autograd.grad(index, (x, y))
    return dict(index=index.detach().double(), per=per.detach().double(), gx=gx.double(), gy=gy.double(), curve=curve.detach().double(),
                Xk=Xk.detach().double(), Yk=Yk.detach().double())


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def case_inputs(g, shape):
    case = "x".join(str(s) for s in shape)
    return torch.from_numpy(g["x_" + case]), torch.from_numpy(g["y_" + case])


def band_limited_pair(fa, H, W, k0, seed):
    """s: white noise with its spectrum zeroed at the rings >= k0, unit std; x = s + 0.2 n1, y = s + 0.2 n2 (float64)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(1, 1, H, W, generator=g, dtype=torch.float64)
    bins = fa.radial_bins(H, W)[0]
    s = torch.fft.ifft2(torch.fft.fft2(rn()) * (bins < k0)).real
    s = s / s.std()
    return s + 0.2 * rn(), s + 0.2 * rn()


def test_restatement_reproduces_the_fixture(fa, gold):
    g = gold
    assert os.path.getsize(GOLD) < (1 << 19)
    assert [tuple(s) for s in g["shapes"]] == list(SHAPES) and float(g["eps"]) == EPS
    for shape in SHAPES:
        x, y = case_inputs(g, shape)
        case = "x".join(str(s) for s in shape)
        assert tuple(x.shape) == shape and x.dtype == torch.float32
        assert g["cnt_" + case].tolist() == fa.radial_bins(*shape[-2:])[1].tolist()
        bands = bands_of(fa, *shape[-2:])
        assert [tuple(b) for b in g["bands_" + case].tolist()] == bands
        for s, band in enumerate(bands):
            t = "%s_s%d" % (case, s)
            ref = restatement(fa, x, y, *band)
            assert abs(float(ref["index"]) - float(g["index64_" + t])) <= 1e-12 * abs(float(g["index64_" + t])), t
            assert rel_l2(ref["per"], torch.from_numpy(g["per64_" + t])) <= 1e-12, t
            assert rel_l2(ref["curve"], torch.from_numpy(g["curve64_" + case])) <= 1e-12, t
            assert ("gx64_" + t in g) == (s in GRADIENTS.get(shape, ())), t
            if "gx64_" + t in g:
                assert rel_l2(ref["gx"], torch.from_numpy(g["gx64_" + t])) <= 1e-12 and rel_l2(ref["gy"], torch.from_numpy(g["gy64_" + t])) <= 1e-12, t
            # the fp32 run of the same definition is the GPU tests' yardstick.  Its last bits depend on the host's FFT code path, so
            # the file's figures are held to the class of an fp32 error, and so is this host's run -- not to each other's bits
            r32 = restatement(fa, x, y, *band, dtype=torch.float32)
            for got in (float(g["index32_" + t]), float(g["index32dft_" + t]), float(r32["index"])):
                assert abs(got - float(ref["index"])) <= 1e-6 * abs(float(ref["index"])), t
            assert 1e-8 < float(g["gxerr32_" + t]) < 3e-6 and 1e-8 < float(g["gyerr32_" + t]) < 3e-6, t
            assert rel_l2(r32["gx"], ref["gx"]) < 3e-6 and rel_l2(r32["gy"], ref["gy"]) < 3e-6, t
        assert 1e-9 < float(g["curveerr32_" + case]) < 1e-6


def test_fixture_inputs_follow_the_recipe_of_the_sprof_tests(gold):
    spec = importlib.util.spec_from_file_location("sprof_gpu_tests", os.path.join(ROOT, "tests", "test_gpu_sprof.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for shape in SHAPES:
        x, y = mod.recipe(shape)
        fx, fy = case_inputs(gold, shape)
        assert float((fx - x).abs().max()) <= 1e-6 and float((fy - y).abs().max()) <= 1e-6


def test_power_rings_are_the_spectral_profile_and_guards_hold(fa, gold):
    """Xk, Yk of the restatement are ``profile_of`` of tests/test_gpu_sprof.py; the guards of the gradient comparisons on every case:
    min over k >= 1 of Xk / mean(x^2) >= 2^-8 for both images, |index| >= 0.25; and |r_k| <= 1 (Cauchy-Schwarz per ring)."""
    spec = importlib.util.spec_from_file_location("sprof_gpu_tests", os.path.join(ROOT, "tests", "test_gpu_sprof.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for shape in SHAPES:
        x, y = case_inputs(gold, shape)
        for band in bands_of(fa, *shape[-2:]):
            ref = restatement(fa, x, y, *band)
            assert abs(float(ref["index"])) >= 0.25
        assert torch.equal(ref["Xk"], mod.profile_of(fa, x.double())) and torch.equal(ref["Yk"], mod.profile_of(fa, y.double()))
        for img, A in ((x, ref["Xk"]), (y, ref["Yk"])):
            assert float((A[..., 1:] / (img.double() ** 2).mean((-2, -1))[..., None]).min()) >= 2.0 ** -8
        assert float(ref["curve"].abs().max()) <= 1 + 1e-12


def test_identities_of_the_definition(fa, gold):
    """frc(x, x) = 1 with a zero gradient, frc(x, -x) = -1, gain invariance, translation invariance, symmetry, and the gradient
    is orthogonal to its own image (the index does not change along a gain)."""
    x, y = case_inputs(gold, (1, 2, 37, 53))
    same = restatement(fa, x, x.clone())
    assert abs(float(same["index"]) - 1) <= 1e-12 and float(same["gx"].norm()) <= 1e-12
    assert abs(float(restatement(fa, x, -x)["index"]) + 1) <= 1e-12
    ref = restatement(fa, x, y)
    assert abs(float(restatement(fa, 2.5 * x.double(), 0.4 * y.double())["index"]) - float(ref["index"])) <= 1e-12
    rolled = restatement(fa, torch.roll(x, (3, 5), (-2, -1)), torch.roll(y, (3, 5), (-2, -1)))
    assert abs(float(rolled["index"]) - float(ref["index"])) <= 1e-12
    swapped = restatement(fa, y, x)
    assert abs(float(swapped["index"]) - float(ref["index"])) <= 1e-15 and rel_l2(swapped["gx"], ref["gy"]) <= 1e-12
    assert abs(float((ref["gx"] * x.double()).sum())) <= 1e-12 * float(ref["gx"].norm() * x.double().norm())
    # a ring with no power in one image: r_k = 0 there, finite everywhere
    z = torch.zeros(1, 1, 8, 8)
    dead = restatement(fa, z, x[:, :1, :8, :8])
    assert float(dead["index"]) == 0 and not dead["curve"].any() and torch.isfinite(dead["gx"]).all()


@pytest.mark.parametrize("H,W,k0", BAND_LIMIT)
@pytest.mark.parametrize("seed", [0, 1])
def test_band_limit(fa, H, W, k0, seed):
    """Two noisy copies of a signal band-limited to the rings below k0 decorrelate at k0: the 1/7 cutoff lies within one ring."""
    x, y = band_limited_pair(fa, H, W, k0, seed)
    curve = restatement(fa, x, y)["curve"]
    k = fa.ops.frc_cutoff(curve, H, W)
    assert k.dtype == torch.float64 and tuple(k.shape) == (1, 1)
    print("FRC band limit %dx%d k0 %d seed %d: cutoff %.2f" % (H, W, k0, seed, float(k)))
    assert abs(float(k) - k0) <= 1
    assert float(curve[0, 0, 1:k0 - 1].min()) > 0.8 and float(curve[0, 0, k0 + 1:min(H, W) // 2].abs().max()) < 0.5


def test_cutoff_on_hand_made_curves(fa):
    cut = fa.ops.frc_cutoff
    H = W = 8                                                                   # six rings, the Nyquist ring is 4
    c = lambda *v: torch.tensor([[list(v)]], dtype=torch.float64)
    assert fa.radial_bins(H, W)[1].numel() == 6
    assert cut(c(1, .9, .8, .7, .6, .5), H, W).tolist() == [[4.0]]              # no crossing -> k_max = M // 2
    assert cut(c(1, .9, .8, .7, .6, .5), H, W, k_max=5).tolist() == [[5.0]]
    assert cut(c(1, .9, .8, .7, .6, .0), H, W).tolist() == [[4.0]]              # the crossing lies beyond k_max
    assert cut(c(1, .1, .8, .7, .6, .5), H, W).tolist() == [[1.0]]              # crossing at k_min
    assert cut(c(0, .9, .8, .7, .6, .5), H, W, k_min=0).tolist() == [[0.0]]
    # threshold 1/4, r_2 = 3/4, r_3 = 1/8: d = 1/2, -1/8, k* = 2 + (1/2) / (5/8) = 2.8
    assert cut(c(1, 1, .75, .125, 0, 0), H, W, threshold=0.25).tolist() == [[2.8]]
    # the first crossing counts, not a later one; a batch of curves at once; fp32 curves are read in float64
    both = torch.cat((c(1, 1, .75, .125, 1, 0), c(1, .5, .25, .5, 0, 0)), 1).float()
    assert cut(both, H, W, threshold=0.375).tolist() == [[2 + .375 / .625, 1 + .125 / .25]]
    assert cut(c(1, float("nan"), .75, .125, 0, 0), H, W, threshold=0.25).tolist() == [[2.8]]          # nan is not below
    # smooth = 3 on a short curve: windows [0], [0..2], [1..3], [2..4], [3..5], [5]
    r = c(1, .75, .5, .25, 0, .5)
    sm = [1, .75, .5, .25, .25, .5]
    assert [sum(v) / len(v) for v in ([1], [1, .75, .5], [.75, .5, .25], [.5, .25, 0], [.25, 0, .5], [.5])] == sm
    # threshold 5/16: rings 2 and 3 keep their values under the average (d = 3/16, -1/16); threshold 1/8: ring 4 rises from 0 to 1/4
    assert cut(r, H, W, threshold=0.3125, smooth=3).tolist() == [[2 + .1875 / .25]]
    assert cut(r, H, W, threshold=0.3125, smooth=1).tolist() == [[2 + .1875 / .25]]
    assert cut(r, H, W, threshold=0.125, smooth=1).tolist() == [[3 + .125 / .25]]
    assert cut(r, H, W, threshold=0.125, smooth=3, k_max=5).tolist() == [[5.0]]                          # smoothed: never below 1/8
    assert cut(r, H, W, threshold=0.125, smooth=15, k_max=5).tolist() == [[5.0]] and cut(r, H, W, smooth=5).shape == (1, 1)
    # half-bit: T_k against the formula, and a curve that sits on T except at one ring
    cnt = fa.radial_bins(H, W)[1].double()
    T = fa.ops.frc_half_bit(H, W)
    want = [(0.2071 + 1.9102 / n ** 0.5) / (1.2071 + 0.9102 / n ** 0.5) for n in cnt.tolist()]
    assert T.dtype == torch.float64 and T.tolist() == pytest.approx(want, rel=1e-15) and abs(float(T[0]) - 1) < 1e-12
    assert int(cnt[1]) == 8 and abs(float(T[1]) - (0.2071 + 1.9102 / 8 ** 0.5) / (1.2071 + 0.9102 / 8 ** 0.5)) < 1e-15
    curve = T.clone()[None, None]
    curve[0, 0, 3] -= 0.25
    curve[0, 0, 2] += 0.25
    assert float(cut(curve, H, W, threshold="half-bit")) == pytest.approx(2.5, abs=1e-14)           # (T + 1/4) - T is 1/4 up to rounding
    assert cut(T[None, None] + 0.01, H, W, threshold="half-bit").tolist() == [[4.0]]


def test_cutoff_refusals(fa):
    cut = fa.ops.frc_cutoff
    c = torch.ones(1, 1, 6, dtype=torch.float64)
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, "one-bit", None, True, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            cut(c, 8, 8, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            fa.FRCResolution(threshold=bad)
    for bad in (0, 2, 17, -1, 3.0, "3", None, True):
        with pytest.raises(ValueError, match="smooth"):
            cut(c, 8, 8, smooth=bad)
        with pytest.raises(ValueError, match="smooth"):
            fa.FRCResolution(smooth=bad)
    for kw in (dict(k_min=-1), dict(k_min=1.0), dict(k_max=0), dict(k_max=6), dict(k_min=5, k_max=4), dict(k_max=2.0)):
        with pytest.raises(ValueError, match="k_m"):
            cut(c, 8, 8, **kw)
    for bad in (torch.ones(1, 1, 5), torch.ones(1, 6), torch.ones(1, 1, 6, dtype=torch.int64), [[1.0] * 6], None):
        with pytest.raises(ValueError, match="curve"):
            cut(bad, 8, 8)
    with pytest.raises(ValueError, match="radial_bins"):
        cut(c, 1, 8)


def test_public_names_and_signatures(fa):
    for name in ("FRC", "FRCResolution", "frc", "frc_curve", "frc_cutoff"):
        assert name in fa.__all__ and callable(getattr(fa, name)), name
    assert fa.FRC is fa.ssim.FRC and fa.FRCResolution is fa.ssim.FRCResolution and fa.frc is fa.ssim.frc
    assert fa.frc_curve is fa.ops.frc_curve and fa.frc_cutoff is fa.ops.frc_cutoff
    sig = inspect.signature(fa.ops.frc)
    assert list(sig.parameters) == ["a", "b", "k_min", "k_max", "eps", "per_image"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [1, None, 1e-16, False]
    sig = inspect.signature(fa.ops.frc_curve)
    assert list(sig.parameters) == ["a", "b", "eps"] and sig.parameters["eps"].default == 1e-16
    sig = inspect.signature(fa.ops.frc_cutoff)
    assert list(sig.parameters) == ["curve", "H", "W", "threshold", "smooth", "k_min", "k_max"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [1 / 7, 1, 1, None]
    sig = inspect.signature(fa.ssim.frc)
    assert list(sig.parameters) == ["img1", "img2", "k_min", "k_max", "eps", "size_average"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [1, None, 1e-16, True]
    sig = inspect.signature(fa.FRC.__init__)
    assert list(sig.parameters) == ["self", "k_min", "k_max", "eps", "size_average"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1, None, 1e-16, True]
    sig = inspect.signature(fa.FRCResolution.__init__)
    assert list(sig.parameters) == ["self", "threshold", "smooth", "k_min", "k_max", "eps"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1 / 7, 1, 1, None, 1e-16]
    for cls in (fa.FRC, fa.FRCResolution):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "img1", "img2"]
        assert list(inspect.signature(cls.index).parameters) == ["self", "img1", "img2", "per_image"]
        m = cls()
        assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(m.buffers())
    for name in ("curve", "resolution"):
        assert list(inspect.signature(getattr(fa.FRCResolution, name)).parameters) == ["self", "img1", "img2"]
    assert repr(fa.FRC()) == "FRC(k_min=1, k_max=None, eps=1e-16, size_average=True)"
    assert fa.FRCResolution("half-bit", 3, 2, 9, 1e-12).extra_repr() == "threshold=half-bit, smooth=3, k_min=2, k_max=9, eps=1e-12"
    assert "frc" not in inspect.signature(fa.TrainStep.__init__).parameters and len(fa.train.OPT_IN_TERMS) == 16      # no train term yet


def test_host_side_refusals(fa):
    """Each refusal comes before any device call: none of these needs a GPU, and there is no CPU fallback."""
    x = torch.rand(1, 1, 8, 8)
    f = fa.ops.frc
    for bad in (0.0, -1e-16, float("nan"), float("inf"), "1e-16", None, True):
        with pytest.raises(ValueError, match="eps"):
            f(x, x, eps=bad)
        with pytest.raises(ValueError, match="eps"):
            fa.FRC(eps=bad)
        with pytest.raises(ValueError, match="eps"):
            fa.ops.frc_curve(x, x, eps=bad)
        with pytest.raises(ValueError, match="eps"):
            fa.FRCResolution(eps=bad)
    for bad in (-1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="k_min"):
            f(x, x, k_min=bad)
        with pytest.raises(ValueError, match="k_min"):
            fa.FRC(k_min=bad)
    for bad in (0, 1.0, "4", True):
        with pytest.raises(ValueError, match="k_max"):
            f(x, x, k_max=bad)
        with pytest.raises(ValueError, match="k_max"):
            fa.FRC(k_max=bad)
    with pytest.raises(fa.KernelError, match=r"\(N,C,H,W\)"):
        f(x[0], x[0])
    with pytest.raises(fa.KernelError, match=r"\(N,C,H,W\)"):
        f(x, None)
    with pytest.raises(fa.KernelError, match="fp32"):
        f(x.double(), x.double())
    with pytest.raises(fa.KernelError, match="fp32"):
        f(x, x.half())
    for call in (lambda: f(x, x), lambda: fa.FRC()(x, x), lambda: fa.FRC().index(x, x, True), lambda: fa.frc(x, x), lambda: fa.ops.frc_curve(x, x),
                 lambda: fa.FRCResolution()(x, x), lambda: fa.FRCResolution().curve(x, x), lambda: fa.FRCResolution().resolution(x, x)):
        with pytest.raises(fa.KernelError, match="GPU"):
            call()
    with pytest.raises(fa.KernelError, match="fp32"):
        fa.ops.frc_curve(x.double(), x.double())
    assert fa.ops.frc_band(8, 8) == (1, 4, 6) and fa.ops.frc_band(37, 53, 0, 25) == (0, 25, 26)
    with pytest.raises(ValueError, match="k_max"):
        fa.ops.frc_band(8, 8, 1, 6)


def test_new_symbols_in_header_and_library(fa, lib):
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in fa._lib.declared_symbols(), s
        assert hasattr(lib, s), s


def test_workspace_query(lib):
    K = 182
    n = lib.faoctasr_frc_workspace_floats(8, 1, 256, 256, 129, K)
    assert n == 8 * 256 * 129 * (2 * 2 + 3)                                     # [P | Q] of two images and three weighted half planes
    assert n < lib.faoctasr_ffl_workspace_floats(8, 1, 256, 256)
    assert lib.faoctasr_frc_workspace_floats(1, 1, 2, 3, 2, 2) > 0
    assert lib.faoctasr_frc_workspace_floats(1, 1, 1, 64, 33, 2) < 0 and b"H" in lib.faoctasr_last_error()
    assert lib.faoctasr_frc_workspace_floats(1, 1, 8, 8, 4, 6) < 0 and b"Wh" in lib.faoctasr_last_error()
    assert lib.faoctasr_frc_workspace_floats(1, 1, 8, 8, 5, 7) < 0 and b"radial bins" in lib.faoctasr_last_error()
    assert lib.faoctasr_frc_workspace_floats(1, 1, 1025, 8, 5, 6) < 0 and b"1024" in lib.faoctasr_last_error()
    assert lib.faoctasr_frc_workspace_floats(40000, 1, 8, 8, 5, 6) < 0 and b"65535" in lib.faoctasr_last_error()


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    fwd = lambda *a: lib.faoctasr_frc_fwd(*a)
    bwd = lambda *a: lib.faoctasr_frc_bwd(*a)
    L = lambda H=64, W=64, Wh=33, K=46, eps=1e-16, k_min=1, k_max=32, per=0: [p, p, p, p, p, p, p, eps, k_min, k_max, per, p, p, p, p, p, p, 1, 1, H, W, Wh, K, None]
    B = lambda H=64, W=64, Wh=33, K=46: [p, 0, p, p, p, p, p, p, p, 1, 1, H, W, Wh, K, None]
    for H, W in ((1, 64), (64, 1)):
        for f, a, name in ((fwd, L, b"frc_fwd"), (bwd, B, b"frc_bwd")):
            assert f(*a(H=H, W=W)) == -1 and name in lib.faoctasr_last_error()
    for f, a in ((fwd, L), (bwd, B)):
        assert f(*a(H=1025)) == -2 and b"1024" in lib.faoctasr_last_error()
        assert f(*a(Wh=32)) == -1 and b"Wh" in lib.faoctasr_last_error()
        assert f(*a(K=45)) == -1 and b"radial bins" in lib.faoctasr_last_error()
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(*L(eps=eps)) == -1 and b"eps" in lib.faoctasr_last_error()
    for k_min, k_max in ((-1, 32), (33, 32), (1, 46), (46, 46)):
        assert fwd(*L(k_min=k_min, k_max=k_max)) == -1 and b"k_min" in lib.faoctasr_last_error()
    for k in (0, 1, 2, 3, 4, 5, 6, 11, 13, 14, 16):               # index_per_image (12) and save (15) may be null
        a = L()
        a[k] = None
        assert fwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    a = L(per=1)
    a[12] = None
    assert fwd(*a) == -1 and b"per_image" in lib.faoctasr_last_error()
    for k in (0, 3, 4, 5, 8):                                     # g, tabH, halfW, binmap, workspace
        a = B()
        a[k] = None
        assert bwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    for keep in (6, 7):                                           # a gradient wanted (dx or dy alone), nothing saved
        a = B()
        a[2] = None
        a[13 - keep] = None
        assert bwd(*a) == -1 and b"saved nothing" in lib.faoctasr_last_error()
    a = B()
    a[6] = a[7] = None                                            # neither gradient wanted: nothing to do, and nothing is launched
    assert bwd(*a) == 0


def test_generator_script_is_independent_of_package_and_tests():
    with open(os.path.join(ROOT, "tools", "gen_golden_frc.py")) as f:
        src = f.read()
    imports = re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, re.M)
    assert sorted(set(imports)) == ["math", "numpy", "os", "torch"]
    assert "faoctasr" not in src and "radial_bins" not in src and "CH @ x @ CW" in src and "for k in range(len(cnt))" in src
