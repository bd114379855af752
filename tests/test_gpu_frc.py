"""The Fourier ring correlation on the MI355X: ``ops.frc`` / ``ops.frc_curve`` / ``ops.frc_cutoff`` / ``FRC`` / ``FRCResolution``
against the float64 fixture (tests/golden/golden_frc.npz, explicit DFT matrices and a loop over the rings) and the float64
``torch.fft`` + ``index_add_`` restatement pinned to it by tests/test_frc_cpu.py; its exact properties; the cutoff read-out on
band-limited pairs; and its use through ``evaluate_pairs_with``.

The error bar is the one tests/test_gpu_phase_loss.py reasons for this DFT-as-GEMM path and tests/test_gpu_sprof.py reuses, relative
to the error of the fp32 ``torch.fft`` run of the same definition on the CPU against float64:
  * each gradient and the curve, in relative L2:  e_hip <= 8 e_ref, e_ref that fp32 run's own error for the same array;
  * the index:  |I_hip - I_64| <= 8 r |I_64| + one fp32 ulp of I_64, with r the largest relative index error of the fp32 run over
    the fixture's cases (one case's own error can be near zero by accident).
``1 / sqrt(Xk Yk + eps)`` amplifies rounding where a ring is nearly empty and a small index amplifies the relative error, so every
gradient comparison first asserts, on the float64 restatement, that min over k >= 1 of Xk / mean(x^2) >= 2^-8 for both images and
|I_64| >= 0.25.  Figures of one run: profiles/frc_error.txt."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_frc.npz")
SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
BENCH = (8, 1, 256, 256)
SEAMS = (2, 1, 72, 136)                                        # tile seams on both axes of the half plane (69 columns)
BAND_LIMIT = ((64, 64, 16), (65, 63, 12), (72, 136, 20))
EPS = 1e-16
GUARD = 2.0 ** -8
ULP = 2.0 ** -23


def smooth(t, r):
    return sum(torch.roll(t, (dy, dx), (-2, -1)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / (2 * r + 1) ** 2


def recipe(shape):
    """The input recipe of tests/test_gpu_sprof.py (seed 0, float64, rounded to fp32)."""
    g = torch.Generator().manual_seed(0)
    rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64)
    x = 2 * smooth(rn(), 2) + 0.25 * rn()
    y0 = x + 0.3 * rn()
    return x.float(), (0.7 * smooth(y0, 1) + 0.3 * y0).float()


def ring_means(fa, x, y):
    """(Nk, Xk, Yk), each (N, C, K), through ``torch.fft.fft2`` and ``index_add_`` on the CPU in x's dtype (differentiable)."""
    N, C, H, W = x.shape
    bins, cnt = fa.radial_bins(H, W)
    F, G = torch.fft.fft2(x), torch.fft.fft2(y)
    planes = ((F.real * G.real + F.imag * G.imag) / (H * W), (F.real ** 2 + F.imag ** 2) / (H * W), (G.real ** 2 + G.imag ** 2) / (H * W))
    return tuple(torch.zeros(N, C, cnt.numel(), dtype=x.dtype).index_add_(2, bins.flatten(), q.reshape(N, C, H * W)) / cnt.to(x.dtype)
                 for q in planes)


def restatement(fa, x, y, k_min=1, k_max=None, eps=EPS, dtype=torch.float64, g=None, y_grad=True):
    """The definition on the CPU in ``dtype``: dict of index, per, gx, gy, curve, Xk, Yk as float64.  ``g``: the upstream gradient, a
    scalar or one per sample (then of the per-image values)."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(y_grad)
    if k_max is None:
        k_max = min(x.shape[-2:]) // 2
    Nk, Xk, Yk = ring_means(fa, x, y)
    curve = Nk / torch.sqrt(Xk * Yk + eps)
    per = curve[..., k_min:k_max + 1].mean((1, 2))
    index = per.mean()
    ins = (x, y) if y_grad else (x,)
    if g is not None and torch.is_tensor(g) and g.dim() == 1:
        grads = torch.autograd.grad(per, ins, g.to(dtype))
    else:
        grads = torch.autograd.grad(index, ins)
        if g is not None:
            grads = tuple(t * float(g) for t in grads)
    return dict(index=index.detach().double(), per=per.detach().double(), gx=grads[0].double(), gy=grads[1].double() if y_grad else None,
                curve=curve.detach().double(), Xk=Xk.detach().double(), Yk=Yk.detach().double())


def guard(ref, x, y):
    """The conditioning guards of the module docstring, on the float64 restatement."""
    for img, A in ((x, ref["Xk"]), (y, ref["Yk"])):
        if A.shape[-1] > 1:
            ratio = float((A[..., 1:] / (img.double() ** 2).mean((-2, -1))[..., None]).min())
            assert ratio >= GUARD, ratio
    assert abs(float(ref["index"])) >= 0.25, float(ref["index"])


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def index_r(gold):
    """The largest relative index error of the fp32 reference over the file's cases."""
    r = 0.0
    for key in gold.files:
        if key.startswith("index64_"):
            r = max(r, abs(float(gold["index32_" + key[8:]]) - float(gold[key])) / abs(float(gold[key])))
    assert 1e-8 < r < 1e-6
    return r


@pytest.fixture(scope="module")
def seams(fa, gold):
    """The tile-seam case of the fixture with its float64 and fp32 restatements, computed once for the tests that need them."""
    x, y = fixture_pair(gold, SEAMS)
    return x, y, restatement(fa, x, y), restatement(fa, x, y, dtype=torch.float32)


def fixture_pair(gold, shape):
    case = "x".join(str(s) for s in shape)
    return torch.from_numpy(gold["x_" + case]), torch.from_numpy(gold["y_" + case])


def hip(fa, x, y, k_min=1, k_max=None, want_x=True, want_y=True, g=None, per_image=False, eps=EPS):
    """(index or per-image values, dx, dy) of ops.frc on the GPU, back on the host (a gradient not asked for is None)."""
    xd = x.cuda().requires_grad_(want_x)
    yd = y.cuda().requires_grad_(want_y)
    out = fa.ops.frc(xd, yd, k_min, k_max, eps, per_image)
    assert out.shape == ((x.shape[0],) if per_image else ()) and out.dtype == torch.float32
    if want_x or want_y:
        if per_image:
            out.backward(torch.ones(x.shape[0], device="cuda") if g is None else g.cuda().float())
        else:
            out.backward(None if g is None else torch.tensor(g, device="cuda"))
    torch.cuda.synchronize()
    return out.detach().cpu(), (xd.grad.cpu() if want_x else None), (yd.grad.cpu() if want_y else None)


def index_bar(i64, r):
    return 8 * r * abs(float(i64)) + float(np.spacing(np.float32(abs(float(i64)))))


def hold_to_bar(name, ref, e_gx, e_gy, got, r):
    """Print e_ref, e_hip and their ratio for the index and both gradients, then assert the bar of the module docstring."""
    e_idx = abs(float(got[0]) - float(ref["index"]))
    h_gx, h_gy = rel_l2(got[1], ref["gx"]), rel_l2(got[2], ref["gy"])
    print("FRC_ERR %-22s index %.9e rel err %.3e (bar %.3e) | gx e_ref %.3e e_hip %.3e ratio %.2f | gy e_ref %.3e e_hip %.3e ratio %.2f"
          % (name, float(got[0]), e_idx / abs(float(ref["index"])), index_bar(ref["index"], r) / abs(float(ref["index"])), e_gx, h_gx, h_gx / e_gx,
             e_gy, h_gy, h_gy / e_gy))
    assert e_idx <= index_bar(ref["index"], r), (name, "index", float(got[0]), float(ref["index"]))
    assert h_gx <= 8 * e_gx, (name, "gx", h_gx, e_gx)
    assert h_gy <= 8 * e_gy, (name, "gy", h_gy, e_gy)


def hold_curve(name, got, c64, e_ref):
    e_hip = rel_l2(got, c64)
    print("FRC_ERR curve %-16s e_ref %.3e e_hip %.3e ratio %.2f" % (name, e_ref, e_hip, e_hip / e_ref))
    assert got.dtype == torch.float32 and not got.requires_grad and e_hip <= 8 * e_ref, (name, e_hip, e_ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_fixture_parity(fa, gold, index_r, shape):
    """The fixture's inputs at its three bands: the smallest plane with an odd W and K = 2; one partial tile; odd and ragged with two
    channels; an exact tile with the even-W Nyquist column; one past and one short of a tile; tile seams on both axes.  Index against
    the file; gradients against the file where it carries them, else against the in-test float64 restatement (itself pinned to
    the file's index); the curve against the file; e_ref is the file's, per array."""
    x, y = fixture_pair(gold, shape)
    case = "x".join(str(s) for s in shape)
    for s, band in enumerate(tuple(b) for b in gold["bands_" + case].tolist()):
        t = "%s_s%d" % (case, s)
        ref = restatement(fa, x, y, *band)
        assert abs(float(ref["index"]) - float(gold["index64_" + t])) <= 1e-12 * abs(float(ref["index"]))
        guard(ref, x, y)
        ref["index"] = torch.tensor(float(gold["index64_" + t]), dtype=torch.float64)
        if "gx64_" + t in gold:
            ref["gx"], ref["gy"] = torch.from_numpy(gold["gx64_" + t]), torch.from_numpy(gold["gy64_" + t])
        hold_to_bar(t, ref, float(gold["gxerr32_" + t]), float(gold["gyerr32_" + t]), hip(fa, x, y, *band), index_r)
    curve = fa.ops.frc_curve(x.cuda(), y.cuda())
    assert tuple(curve.shape) == shape[:2] + (len(gold["cnt_" + case]),)
    hold_curve(case, curve, torch.from_numpy(gold["curve64_" + case]), float(gold["curveerr32_" + case]))


def test_the_benchmark_shape(fa, index_r):
    """(8,1,256,256) through the modules: K = 182, the Nyquist ring 128, eight tiles per plane in the half plane, the batch mean over 8."""
    x, y = recipe(BENCH)
    ref, ref32 = restatement(fa, x, y), restatement(fa, x, y, dtype=torch.float32)
    guard(ref, x, y)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    index = fa.FRC()(xd, yd)
    assert index.dim() == 0 and index.dtype == torch.float32
    (1 - index).backward()
    hold_to_bar("x".join(map(str, BENCH)), ref, rel_l2(ref32["gx"], ref["gx"]), rel_l2(ref32["gy"], ref["gy"]),
                (index.detach().cpu(), -xd.grad.cpu(), -yd.grad.cpu()), index_r)
    curve = fa.FRCResolution().curve(xd, yd)
    assert tuple(curve.shape) == (8, 1, 182)
    hold_curve("x".join(map(str, BENCH)), curve, ref["curve"], rel_l2(ref32["curve"], ref["curve"]))
    assert torch.equal(fa.frc(xd, yd, size_average=False), fa.FRC(size_average=False)(xd, yd))


@pytest.mark.parametrize("shape", [(2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 72, 136)])
def test_per_image_values_and_per_sample_upstream(fa, gold, index_r, shape):
    """``per_image``: (N,) of each sample's mean over c and the band (the file's), and a different upstream gradient per sample."""
    x, y = fixture_pair(gold, shape)
    g = torch.tensor([0.75, -1.5][:shape[0]], dtype=torch.float64)
    ref, ref32 = restatement(fa, x, y, g=g), restatement(fa, x, y, dtype=torch.float32, g=g)
    guard(ref, x, y)
    per, gx, gy = hip(fa, x, y, per_image=True, g=g)
    want = torch.from_numpy(gold["per64_%s_s0" % "x".join(str(s) for s in shape)])
    for n in range(shape[0]):
        assert abs(float(per[n]) - float(want[n])) <= index_bar(want[n], index_r), (n, float(per[n]), float(want[n]))
    e = (rel_l2(ref32["gx"], ref["gx"]), rel_l2(ref32["gy"], ref["gy"]))
    print("FRC_ERR per_image %-14s gx e_ref %.3e e_hip %.3e | gy e_ref %.3e e_hip %.3e" % ("x".join(map(str, shape)), e[0], rel_l2(gx, ref["gx"]), e[1], rel_l2(gy, ref["gy"])))
    assert rel_l2(gx, ref["gx"]) <= 8 * e[0] and rel_l2(gy, ref["gy"]) <= 8 * e[1]
    with torch.no_grad():
        assert torch.equal(fa.FRC().index(x.cuda(), y.cuda(), True).cpu(), per)
        assert torch.equal(fa.FRC().index(x.cuda(), y.cuda(), False).cpu(), hip(fa, x, y, want_x=False, want_y=False)[0])


@pytest.mark.parametrize("band", [(1, None), (0, 50), (2, 18)])
def test_bit_exact_properties(fa, seams, band):
    """Bit for bit, on tile seams along both axes: frc(x, y) == frc(y, x) with swapped gradients; two calls agree; halving the
    upstream gradient halves both gradients; either gradient alone equals the pair's."""
    x, y = seams[:2]
    first = hip(fa, x, y, *band)
    assert 0.25 < float(first[0]) < 1 and torch.isfinite(first[1]).all() and first[1].any() and first[2].any()
    swapped = hip(fa, y, x, *band)
    assert torch.equal(swapped[0], first[0]) and torch.equal(swapped[1], first[2]) and torch.equal(swapped[2], first[1])
    again = hip(fa, x, y, *band)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    half = hip(fa, x, y, *band, g=0.5)
    assert torch.equal(half[0], first[0]) and torch.equal(half[1], 0.5 * first[1]) and torch.equal(half[2], 0.5 * first[2])
    only_x, only_y = hip(fa, x, y, *band, want_y=False), hip(fa, x, y, *band, want_x=False)
    assert only_x[2] is None and only_y[1] is None
    assert torch.equal(only_x[0], first[0]) and torch.equal(only_y[0], first[0])
    assert torch.equal(only_x[1], first[1]) and torch.equal(only_y[2], first[2])


@pytest.mark.parametrize("shape", [(1, 2, 37, 53), (2, 1, 72, 136)])
def test_power_rings_are_the_spectral_profiles(fa, gold, shape):
    """The Xk / Yk by-products of the forward equal ``ops.spectral_profile`` of each image bit for bit (one code path up to the rings)."""
    x, y = (t.cuda() for t in fixture_pair(gold, shape))
    index, per, curve, rings, saved = fa.ops.frc_forward(x, y)
    K = fa.radial_bins(*shape[-2:])[1].numel()
    assert per is None and saved is None and tuple(rings.shape) == (3,) + shape[:2] + (K,) and tuple(curve.shape) == shape[:2] + (K,)
    assert torch.equal(rings[1], fa.ops.spectral_profile(x)) and torch.equal(rings[2], fa.ops.spectral_profile(y))
    want = rings[0].double() / torch.sqrt(rings[1].double() * rings[2].double() + EPS)
    assert float((curve.double() - want).abs().max()) <= ULP and torch.equal(curve, fa.ops.frc_curve(x, y))       # |r| <= 1
    assert torch.equal(index, fa.ops.frc(x, y)) and fa.ops.frc_forward(x, y, per_image=True, save=True)[4].numel() == x.numel() // shape[-1] * 4 * (shape[-1] // 2 + 1) + 3 * shape[0] * shape[1] * K


def test_identical_and_negated_images(fa, seams):
    """|1 - frc(x, x)| <= 2^-23 and frc(x, -x) within 2^-23 of -1; the gradient of frc(x, x.detach()) is a cancellation whose exact
    value is 0: its L2 norm is held to 8 x the fp32 restatement's own residual for the same input."""
    x = seams[0]
    same = hip(fa, x, x.clone(), want_y=False)
    resid32 = float(restatement(fa, x, x.clone(), dtype=torch.float32, y_grad=False)["gx"].norm())
    neg = hip(fa, x, -x, want_x=False, want_y=False)
    print("FRC_ERR identical: index %.9f, |dx| %.3e against the fp32 restatement's residual %.3e; negated: index %.9f"
          % (float(same[0]), float(same[1].double().norm()), resid32, float(neg[0])))
    assert abs(1 - float(same[0])) <= ULP and abs(float(neg[0]) + 1) <= ULP
    assert float(same[1].double().norm()) <= 8 * resid32


def test_gain_translation_and_orthogonality(fa, seams, index_r):
    """The index does not change under a gain on either image or a common circular shift (the index bar), and so the gradient is
    orthogonal to its own image: |<dx, x>| / (|dx| |x|) is held to 8 x the fp32 restatement's value + 1e-6."""
    x, y, ref, ref32 = seams
    guard(ref, x, y)
    bar = index_bar(ref["index"], index_r)
    base, dx, dy = hip(fa, x, y)
    gained = hip(fa, 2.5 * x, 0.4 * y, want_x=False, want_y=False)[0]
    rolled = hip(fa, torch.roll(x, (3, 5), (-2, -1)).contiguous(), torch.roll(y, (3, 5), (-2, -1)).contiguous(), want_x=False, want_y=False)[0]
    cos = lambda g, img: abs(float((g.double() * img.double()).sum())) / float(g.double().norm() * img.double().norm())
    print("FRC_ERR invariance: index %.9f gained %.9f rolled %.9f float64 %.9f (bar %.3e) | cos(dx, x) %.3e fp32 restatement %.3e | cos(dy, y) %.3e fp32 restatement %.3e"
          % (float(base), float(gained), float(rolled), float(ref["index"]), bar, cos(dx, x), cos(ref32["gx"], x), cos(dy, y), cos(ref32["gy"], y)))
    for got in (base, gained, rolled):
        assert abs(float(got) - float(ref["index"])) <= bar
    assert cos(dx, x) <= 8 * cos(ref32["gx"], x) + 1e-6 and cos(dy, y) <= 8 * cos(ref32["gy"], y) + 1e-6


def test_degenerate_rings_are_zero_with_finite_gradients(fa, gold):
    """A ring in which one image has no power: r_k = 0 there, and every gradient is finite."""
    x = fixture_pair(gold, (2, 1, 64, 64))[0]
    index, dx, dy = hip(fa, torch.zeros_like(x), x)
    assert float(index) == 0 and torch.isfinite(dx).all() and torch.isfinite(dy).all() and dx.any() and not dy.any()
    assert not fa.ops.frc_curve(torch.zeros_like(x).cuda(), x.cuda()).any()


def test_nothing_is_saved_without_a_gradient(fa, lib_ws, seams):
    """Under ``no_grad`` the peak memory above the workspace is the few small outputs: no saved spectra (4 H Wh floats per plane).
    With a gradient wanted, it is the workspace and the saved spectra."""
    x, y = (t.cuda() for t in seams[:2])
    N, C, H, W = x.shape
    ws_bytes, planes_bytes = 4 * lib_ws(N, C, H, W), 4 * N * C * 4 * H * (W // 2 + 1)
    fa.ops.frc(x, y)                                            # tables and the allocator's pools

    def peak(run):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = run()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out
    with torch.no_grad():
        quiet, out = peak(lambda: fa.ops.frc(x.requires_grad_(True), y))
    loud, kept = peak(lambda: fa.ops.frc(x.requires_grad_(True), y))
    print("FRC_ERR memory: workspace %d B, saved spectra %d B, peak above the inputs %d B under no_grad, %d B with a gradient" % (ws_bytes, planes_bytes, quiet, loud))
    assert out.grad_fn is None and not out.requires_grad and kept.requires_grad
    assert ws_bytes <= quiet < ws_bytes + planes_bytes // 4
    assert loud >= ws_bytes + planes_bytes
    assert not fa.ops.frc(x.detach(), y.detach()).requires_grad and not fa.ops.frc_curve(x, y).requires_grad


@pytest.fixture(scope="module")
def lib_ws(fa):
    lib = fa._lib.load()
    return lambda N, C, H, W: lib.faoctasr_frc_workspace_floats(N, C, H, W, W // 2 + 1, fa.radial_bins(H, W)[1].numel())


def test_runs_on_the_current_stream(fa, seams):
    x, y = seams[:2]
    want = hip(fa, x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = hip(fa, x, y)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(a, b) for a, b in zip(want, got))


def test_shape_refusals_on_the_device(fa):
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    with pytest.raises(ValueError, match="k_max"):
        fa.ops.frc(x, x, k_max=6)                               # an 8 x 8 spectrum has 6 rings
    with pytest.raises(ValueError, match="k_min"):
        fa.FRC(k_min=5)(x, x)                                   # above the default k_max = 4
    with pytest.raises(fa.KernelError, match="one shape"):
        fa.ops.frc(x, torch.zeros(1, 1, 8, 9, device="cuda"))
    with pytest.raises(fa.KernelError, match="1024"):
        fa.ops.frc_curve(torch.zeros(1, 1, 2, 1025, device="cuda"), torch.zeros(1, 1, 2, 1025, device="cuda"))
    with pytest.raises(fa.KernelError, match="H, W"):
        fa.ops.frc(torch.zeros(1, 1, 1, 8, device="cuda"), torch.zeros(1, 1, 1, 8, device="cuda"))
    with pytest.raises(fa.KernelError, match="fp32"):
        fa.ops.frc(x.double(), x.double())


def band_limited_pair(fa, H, W, k0, seed):
    """s: white noise with its spectrum zeroed at the rings >= k0, unit std; x = s + 0.2 n1, y = s + 0.2 n2, rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(1, 1, H, W, generator=g, dtype=torch.float64)
    bins = fa.radial_bins(H, W)[0]
    s = torch.fft.ifft2(torch.fft.fft2(rn()) * (bins < k0)).real
    s = s / s.std()
    return (s + 0.2 * rn()).float(), (s + 0.2 * rn()).float()


@pytest.mark.parametrize("H,W,k0", BAND_LIMIT)
@pytest.mark.parametrize("seed", [0, 1])
def test_cutoff_of_band_limited_pairs(fa, H, W, k0, seed):
    """Two noisy copies of a signal band-limited to the rings below k0: the device curve crosses 1/7 in the ring the float64 curve
    does, within one ring of k0, and |k*_hip - k*_64| <= 4 delta / max(s, 0.25) with delta the largest deviation of the device curve
    from the float64 one and s = |d_{k-1} - d_k| of the float64 run.  s is 0.86 - 1.10 in five of the six cases; at (64, 64, 16)
    seed 1 ring 16 stays just above 1/7 by chance, the crossing lies between rings 16 and 17 and s = 0.103.  To first order
    |dk*| <= delta (|d_{k-1}| + |d_k|) / s^2 = delta / s, which is within 4 delta / 0.25 for every s >= 1/16: s is asserted >= 1/16 and
    the tolerance of a case with s < 0.25 is the tighter 4 delta / 0.25."""
    x, y = band_limited_pair(fa, H, W, k0, seed)
    c64, c32 = restatement(fa, x, y)["curve"], restatement(fa, x, y, dtype=torch.float32)["curve"]
    k64 = float(fa.ops.frc_cutoff(c64, H, W))
    ring = int(k64) + 1                                          # k* = (ring - 1) + a fraction in [0, 1)
    s = abs(float(c64[0, 0, ring - 1] - c64[0, 0, ring]))
    assert abs(k64 - k0) <= 1 and s >= 1 / 16 and float(c64[0, 0, ring]) < 1 / 7 <= float(c64[0, 0, ring - 1])
    assert s >= 0.25 or (H, W, k0, seed) == (64, 64, 16, 1), s
    mod = fa.FRCResolution()
    curve = mod.curve(x.cuda(), y.cuda())
    k_hip = fa.ops.frc_cutoff(curve, H, W)
    assert k_hip.is_cuda and k_hip.dtype == torch.float64 and tuple(k_hip.shape) == (1, 1)
    delta = float((curve.cpu().double() - c64).abs().max())
    print("FRC_ERR cutoff %dx%d k0 %d seed %d: k* %.6f float64 %.6f, delta %.3e, s %.3f" % (H, W, k0, seed, float(k_hip), k64, delta, s))
    hold_curve("band limit %dx%d/%d" % (H, W, seed), curve, c64, rel_l2(c32, c64))
    assert int(float(k_hip)) + 1 == ring
    assert abs(float(k_hip) - k64) <= 4 * delta / max(s, 0.25)
    M = min(H, W)
    assert torch.equal(mod.index(x.cuda(), y.cuda(), True), (k_hip / M).mean(1)) and torch.equal(mod(x.cuda(), y.cuda()), (k_hip / M).mean())
    assert torch.equal(mod.resolution(x.cuda(), y.cuda()), M / k_hip)


def test_evaluate_pairs_with_keys(fa, gold, monkeypatch):
    """``evaluate_pairs_with(model, pairs, frc=FRC(), frc_cutoff=FRCResolution())`` adds both keys: the means of the modules' per-image
    values of (super_resolve(lr), hr).  ``super_resolve`` is replaced by a fixed map (the generator's forward is not bit-reproducible)."""
    blur = lambda t: (0.5 * t + 0.125 * (torch.roll(t, 1, -1) + torch.roll(t, -1, -1) + torch.roll(t, 1, -2) + torch.roll(t, -1, -2))).contiguous()
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: blur(lr))
    x, y = fixture_pair(gold, (2, 1, 64, 64))
    pairs = [(x.clamp(-1, 1).cuda(), y.clamp(-1, 1).cuda()), (y[:1].clamp(-1, 1).cuda(), x[:1].clamp(-1, 1).cuda())]
    plain = fa.evaluate_pairs(None, pairs)
    frc, res = fa.FRC(), fa.FRCResolution()
    out = fa.evaluate_pairs_with(None, pairs, frc=frc, frc_cutoff=res)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "frc", "frc_cutoff"] and all(out[k] == plain[k] for k in plain)
    with torch.no_grad():
        want = [float(torch.cat([m.index(blur(lr), hr, True).double() for lr, hr in pairs]).mean()) for m in (frc, res)]
    print("FRC_ERR evaluate_pairs_with: frc %.9f frc_cutoff %.9f cycles per pixel" % (out["frc"], out["frc_cutoff"]))
    assert out["frc"] == pytest.approx(want[0], rel=1e-12) and out["frc_cutoff"] == pytest.approx(want[1], rel=1e-12)
    assert 0.25 < out["frc"] < 1 and 1 / 64 <= out["frc_cutoff"] <= 0.5
