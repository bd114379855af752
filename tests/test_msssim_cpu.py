"""Multi-scale SSIM without a GPU: a plain-torch float64 restatement of

    MS[n] = prod_j max(F_j[n], 0)^w_j,   F_j[n] = mean_{c,h,w} cs_p at scale j < M,   F_M[n] = mean_{c,h,w} l_p cs_p at scale M,
    cs_p = (2 s12 + C2) / (s11 + s22 + C2),   l_p = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1),   C1 = (0.01 L)^2, C2 = (0.03 L)^2,

scale 1 the input and scale j + 1 = ``avg_pool2d(scale j, 2)``, the moments those of ssim.py:17-27 (11-tap sigma-1.5 Gaussian window
as ssim.py:7-15 builds it in fp32, zero padding 5), gradients by autograd; pinned to the reference's own float64 results
(tests/golden/golden_msssim.npz, tools/gen_golden_msssim.py), and the host logic of ``ops.ms_ssim``, ``ssim.MSSSIM``,
``ssim.ms_ssim``, ``evaluate_pairs(ms_ssim=...)`` and ``TrainStep(msssim_weight=...)`` (everything that raises before an entry point
is reached).

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (scores: absolute difference over |score|; arrays:
relative L2).  Both sides are float64 sums of a few thousand terms.  The only ill-conditioned step is ``w_j MS / F_j``, which
amplifies rounding where a factor is small; every gradient comparison first asserts that every F_j[n] of the float64 run is at
least 0.25 (the fixture's smallest is 0.81): about 1e-14 of rounding.  The fixture's fp32 arrays are the fp32 reference: they
enter only through the error they define (e_ref, E_ref of tests/test_gpu_msssim.py), which is bounded here by 1e-4 as a sanity
check of the fixture, three orders above fp32 rounding of these sums."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_msssim.npz")
DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
FACTOR_CAP = 0.25
#: (case, shape, levels, weights or None, data_range, per image, y needs a gradient): the table of tools/gen_golden_msssim.py
CASES = (("m5_mean", (2, 2, 32, 48), 5, None, 1.0, False, True),
         ("m5_per_image", (2, 2, 32, 48), 5, None, 1.0, True, True),
         ("m3_weights_range2", (2, 2, 32, 48), 3, (0.2, 0.5, 0.3), 2.0, False, True),
         ("m5_odd", (1, 1, 37, 53), 5, None, 1.0, False, True),
         ("m1", (1, 3, 16, 24), 1, (1.0,), 1.0, False, True),
         ("m5_xonly", (2, 2, 32, 48), 5, None, 1.0, False, False))
NEW_SYMBOLS = ("faoctasr_msssim_workspace_floats", "faoctasr_msssim_scale_fwd", "faoctasr_msssim_final", "faoctasr_msssim_scale_bwd")
_gold = {}
_restated = {}


def gold():
    if not _gold:
        with np.load(GOLDEN) as z:
            _gold.update({k: z[k] for k in z.files})
    return _gold


def case_name(case):
    return case[0]


def fixture_inputs(case):
    g = gold()
    key = "%dx%dx%dx%d" % tuple(case[1])
    return torch.from_numpy(g["in/%s/x" % key]), torch.from_numpy(g["in/%s/y" % key])


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def score_err(a, b):
    """The largest relative error of a score (0-d or (N,)) against b."""
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float(((a - b).abs() / b.abs()).max())


# ------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------
def window(channel, dtype):
    """ssim.py:7-15: the taps and their outer product in fp32, then cast (``window.type_as(img1)``, ssim.py:71)."""
    g = torch.tensor([np.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous().to(dtype)


def scale_maps(a, b, C1, C2):
    """(cs_p, l_p) of one scale."""
    ch = a.shape[1]
    w = window(ch, a.dtype)
    mu1, mu2 = F.conv2d(a, w, padding=5, groups=ch), F.conv2d(b, w, padding=5, groups=ch)
    s11 = F.conv2d(a * a, w, padding=5, groups=ch) - mu1 * mu1
    s22 = F.conv2d(b * b, w, padding=5, groups=ch) - mu2 * mu2
    s12 = F.conv2d(a * b, w, padding=5, groups=ch) - mu1 * mu2
    return (2 * s12 + C2) / (s11 + s22 + C2), (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)


def restate(x, y, levels=5, weights=None, data_range=1.0, per_image=False, x_grad=True, y_grad=True, dtype=torch.float64, upstream=None):
    """{"score", "factors" (M, N), "dx", "dy"} in ``dtype``: the score is the mean over n, or (N,) with ``per_image``; the gradients
    are those of ``(score * upstream).sum()`` (upstream 1 by default)."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(y_grad)
    w = DEFAULT_WEIGHTS[:levels] if weights is None else tuple(weights)
    assert len(w) == levels
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a, b, factors = x, y, []
    for j in range(levels):
        cs, lum = scale_maps(a, b, C1, C2)
        factors.append((lum * cs if j == levels - 1 else cs).mean(dim=(1, 2, 3)))
        if j < levels - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    fac = torch.stack(factors)                                            # (M, N)
    dead = (fac <= 0).any(dim=0)
    ms = torch.ones_like(fac[0])
    for f, wj in zip(factors, w):
        ms = ms * torch.where(dead, torch.ones_like(f), f) ** wj
    ms = torch.where(dead, torch.zeros_like(ms), ms)                      # a factor <= 0: score 0, gradient exactly zero
    score = ms if per_image else ms.mean()
    out = {"score": score.detach(), "factors": fac.detach()}
    if x_grad or y_grad:
        (score if upstream is None else score * upstream.to(dtype)).sum().backward()
    if x_grad:
        out["dx"] = x.grad
    if y_grad:
        out["dy"] = y.grad
    return out


def restate_case(case, dtype=torch.float64):
    key = (case[0], dtype)
    if key not in _restated:
        _, _, levels, weights, data_range, per_image, y_grad = case
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, levels, weights, data_range, per_image, True, y_grad, dtype)
    return _restated[key]


def well_conditioned(ref64):
    """The conditioning cap of every gradient comparison."""
    assert float(ref64["factors"].min()) >= FACTOR_CAP, float(ref64["factors"].min())


def smooth_pair(shape, seed, noise=0.15):
    """x = 5x5-box-smoothed N(0, 1) noise times 2, clipped to [-1, 1]; y = clip(x + noise n)."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(*shape, generator=g)
    x = (2.0 * F.conv2d(n, torch.ones(shape[1], 1, 5, 5) / 25.0, padding=2, groups=shape[1])).clamp(-1.0, 1.0)
    return x, (x + noise * torch.randn(*shape, generator=g)).clamp(-1.0, 1.0)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_is_the_fixture(case):
    g = gold()
    cid, y_grad = case[0], case[6]
    ref = restate_case(case)
    well_conditioned(ref)
    assert ref["score"].shape == g[cid + "/score"].shape
    assert score_err(ref["score"], g[cid + "/score"]) <= 1e-12
    assert rel_l2(ref["factors"], g[cid + "/factors"]) <= 1e-12
    assert rel_l2(ref["dx"], g[cid + "/dx"]) <= 1e-12
    assert ((cid + "/dy") in g) == y_grad == ("dy" in ref)
    if y_grad:
        assert rel_l2(ref["dy"], g[cid + "/dy"]) <= 1e-12
    # the fp32 arrays: only the error they define
    assert g[cid + "/f32/score"].dtype == np.float32 and g[cid + "/f32/dx"].dtype == np.float32
    assert score_err(g[cid + "/f32/score"], ref["score"]) <= 1e-4
    for k in ("dx", "dy") if y_grad else ("dx",):
        assert 0 < rel_l2(g["%s/f32/%s" % (cid, k)], ref[k]) <= 1e-4


def test_fixture_is_small_and_its_inputs_are_fp32():
    assert os.path.getsize(GOLDEN) < 1 << 20
    g = gold()
    for k, v in g.items():
        if k.startswith("in/"):
            assert v.dtype == np.float32 and np.abs(v).max() <= 1.0


def test_one_level_is_ssim():
    """levels = 1, weights (1,): the reference's ``ssim.ssim``, here the fixture's m1 score and the oracle's SSIM.  The oracle forms
    the window's outer product in the images' dtype, the reference (and the restatement) in fp32 before the cast: each weight moves
    by at most 2^-24 relative, hence 1e-6 and not 1e-12 against the oracle."""
    from oracle import octa_oracle as O
    case = [c for c in CASES if c[0] == "m1"][0]
    x, y = fixture_inputs(case)
    ref = restate(x, y, 1, (1.0,))
    assert score_err(ref["score"], gold()["m1/score"]) <= 1e-12
    assert abs(float(O.ssim(x.double(), y.double())) - float(ref["score"])) <= 1e-6 * float(ref["score"])
    rows = restate(x, y, 1, (1.0,), per_image=True)["score"]
    want = O.ssim(x.double(), y.double(), size_average=False)
    assert score_err(rows, want) <= 1e-6


def test_restated_gradient_is_the_derivative():
    """Central differences in float64 along a random direction, (1, 2, 19, 23) at M = 3 (a floor at scales 1 and 2)."""
    x, y = smooth_pair((1, 2, 19, 23), 11)
    ref = restate(x, y, 3)
    well_conditioned(ref)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    eps = 1e-6
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + eps * v, y) if which == 0 else (x, y.double() + eps * v)), 3, x_grad=False, y_grad=False)
        dn = restate(*((x.double() - eps * v, y) if which == 0 else (x, y.double() - eps * v)), 3, x_grad=False, y_grad=False)
        num, ana = (float(up["score"]) - float(dn["score"])) / (2 * eps), float((ref[key] * v).sum())
        assert abs(num - ana) <= 1e-6 * abs(ana), (key, num, ana)


def test_clamped_factor_gives_zero_score_and_zero_gradient():
    x, _ = smooth_pair((2, 1, 16, 16), 13)
    ref = restate(x, -x, 2)
    assert float(ref["factors"].min()) < 0 and float(ref["score"]) == 0.0
    assert not ref["dx"].any() and not ref["dy"].any() and not torch.isnan(ref["dx"]).any()


def test_conditioning_of_the_test_inputs():
    """The inputs the GPU tests use meet the cap with margin: smallest factor about 0.87 at M = 5."""
    for shape in ((2, 3, 48, 80), (1, 1, 37, 53), (2, 1, 64, 64)):
        x, y = smooth_pair(shape, 21)
        f = restate(x, y, 5, x_grad=False, y_grad=False)["factors"]
        assert float(f.min()) >= 0.8, (shape, float(f.min()))


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_exports_and_symbols(fa):
    assert fa.MSSSIM is fa.ssim.MSSSIM and fa.ms_ssim is fa.ssim.ms_ssim
    assert "MSSSIM" in fa.__all__ and "ms_ssim" in fa.__all__
    assert callable(fa.ops.ms_ssim) and fa.ops.MSSSIM_MAX_LEVELS == 5 and fa.ops.MSSSIM_WEIGHTS == DEFAULT_WEIGHTS
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"msssim.hip"' in src
    assert os.path.exists(os.path.join(os.path.dirname(fa._lib.__file__), "csrc", "msssim.hip"))


def test_signatures(fa):
    empty = inspect.Parameter.empty
    sig = inspect.signature(fa.ops.ms_ssim)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("a", empty), ("b", empty), ("levels", 5), ("weights", None), ("data_range", 1.0), ("per_image", False)]
    sig = inspect.signature(fa.MSSSIM.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("window_size", 11), ("size_average", True), ("levels", 5), ("weights", None), ("data_range", 1.0)]
    sig = inspect.signature(fa.ssim.ms_ssim)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("img1", empty), ("img2", empty), ("window_size", 11), ("size_average", True), ("levels", 5), ("weights", None), ("data_range", 1.0)]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("msssim_weight", "msssim_levels", "msssim_weights")] == [0.0, 5, None]
    sig = inspect.signature(fa.evaluate_pairs)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("model", empty), ("pairs", empty), ("cw_ssim", None), ("ms_ssim", None)]
    sig = inspect.signature(fa.MSSSIM.index)
    assert list(sig.parameters)[1:] == ["img1", "img2", "per_image"]


def test_module_attributes(fa):
    mod = fa.MSSSIM()
    assert (mod.window_size, mod.size_average, mod.levels, mod.weights, mod.data_range) == (11, True, 5, None, 1.0)
    assert not list(mod.state_dict())
    mod = fa.MSSSIM(size_average=False, levels=3, weights=[1, 2, 3], data_range=2)
    assert (mod.size_average, mod.levels, mod.weights, mod.data_range) == (False, 3, (1.0, 2.0, 3.0), 2.0)
    assert "levels=3" in repr(mod)


def test_module_passes_its_settings_on(fa, monkeypatch):
    seen = []
    monkeypatch.setattr(fa.ops, "ms_ssim", lambda *a: seen.append(a[2:]) or "r")
    x = torch.zeros(1, 1, 16, 16)
    assert fa.MSSSIM(levels=2, weights=(0.5, 0.5), data_range=2.0)(x, x) == "r"
    assert fa.MSSSIM(size_average=False).index(x, x, False) == "r"
    assert fa.MSSSIM(size_average=False)(x, x) == "r"
    assert fa.ssim.ms_ssim(x, x, 11, False, 3, None, 2.0) == "r"
    assert seen == [(2, (0.5, 0.5), 2.0, False), (5, None, 1.0, False), (5, None, 1.0, True), (3, None, 2.0, True)]


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    f = fa.ops.ms_ssim
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="device"):
        f(x, x)
    with pytest.raises(ValueError, match="device"):
        f(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))             # 16 = 2^4: the smallest side M = 5 takes
    with pytest.raises(ValueError, match=r"15 x 40 image leaves scale 5 empty.*at least 16"):
        f(torch.zeros(1, 1, 15, 40), torch.zeros(1, 1, 15, 40))
    with pytest.raises(ValueError, match=r"8 x 3 image leaves scale 3 empty.*at least 4"):
        f(torch.zeros(1, 1, 8, 3), torch.zeros(1, 1, 8, 3), levels=3)
    with pytest.raises(ValueError, match="device"):
        f(torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1), levels=1)
    for bad in (0, 6, -1, 2.5):
        with pytest.raises(ValueError, match="levels"):
            f(x, x, levels=bad)
        with pytest.raises(ValueError, match="levels"):
            fa.MSSSIM(levels=bad)
    for levels, bad in ((5, (1.0,)), (2, (0.1, 0.2, 0.3)), (1, ())):
        with pytest.raises(ValueError, match="one weight per scale"):
            f(x, x, levels=levels, weights=bad)
        with pytest.raises(ValueError, match="one weight per scale"):
            fa.MSSSIM(levels=levels, weights=bad)
    for bad in ((0.5, 0.0), (0.5, -0.5), (float("nan"), 1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="positive"):
            f(x, x, levels=2, weights=bad)
        with pytest.raises(ValueError, match="positive"):
            fa.MSSSIM(levels=2, weights=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            f(x, x, data_range=bad)
        with pytest.raises(ValueError, match="data_range"):
            fa.MSSSIM(data_range=bad)
    with pytest.raises(ValueError, match="float32"):
        f(x.double(), x.double())
    with pytest.raises(ValueError, match="float32"):
        f(x, x.half())
    with pytest.raises(ValueError, match="same shape"):
        f(x, torch.zeros(1, 1, 32, 16))
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        f(x[0], x[0])
    with pytest.raises(ValueError, match="non-empty"):
        f(torch.zeros(0, 1, 32, 32), torch.zeros(0, 1, 32, 32))
    for call in (lambda: fa.MSSSIM(window_size=7), lambda: fa.ssim.ms_ssim(x, x, window_size=7)):
        with pytest.raises(NotImplementedError, match="11-tap"):
            call()
    mod = fa.MSSSIM(levels=2)
    with pytest.raises(ValueError, match="device"):
        mod(x, x)
    with pytest.raises(ValueError, match="device"):
        mod.index(x, x, True)
    with pytest.raises(ValueError, match="device"):
        fa.ssim.ms_ssim(x, x)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.MSSSIM

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "MSSSIM", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.msssim_weight == 0.0 and ts.msssim is None and not built
    ts = fa.TrainStep(*nets, device="cpu", msssim_weight=0.25, msssim_levels=3, msssim_weights=(0.2, 0.3, 0.5))
    assert built == [dict(levels=3, weights=(0.2, 0.3, 0.5))]
    assert ts.msssim_weight == 0.25 and (ts.msssim.levels, ts.msssim.weights, ts.msssim.size_average) == (3, (0.2, 0.3, 0.5), True)
    assert ts.cwssim is None and ts.cwt_loss is None
    with pytest.raises(ValueError, match="levels"):
        fa.TrainStep(*nets, device="cpu", msssim_weight=0.25, msssim_levels=6)


def test_train_step_terms_call_the_module(fa):
    """``_extension_terms`` names ``loss_msssim``; with the module replaced by a stub no kernel runs (``generator_loss``:
    tests/test_train_terms_cpu.py)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu", msssim_weight=0.5, msssim_levels=2)
    ts.msssim = lambda rec, real: (rec * real).mean()
    rec, real = torch.full((1, 1, 4, 4), 0.5), torch.full((1, 1, 4, 4), 0.5)
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_msssim"] and float(t["loss_msssim"]) == 0.5 * (1 - 0.25)
    ts0 = fa.TrainStep(*nets, device="cpu")
    assert ts0._extension_terms(rec, real) == {}


def test_evaluate_pairs_keys(fa, monkeypatch):
    """With and without the module, ``image_metrics`` and ``super_resolve`` replaced: no kernel runs."""
    asked = []

    def metrics(y, gt, data_range=2.0, bins=100, cw_ssim=None):
        asked.append(cw_ssim)
        return torch.arange(4 if cw_ssim is None else 5, dtype=torch.float64).repeat(y.shape[0], 1)
    monkeypatch.setattr(fa.evaluate, "image_metrics", metrics)
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: lr * 2)

    class Mod:
        calls = []

        def index(self, a, b, per_image):
            self.calls.append((a, b, per_image))
            return torch.tensor([0.25, 0.75][:a.shape[0]])
    pairs = [(torch.ones(2, 1, 16, 16), torch.zeros(2, 1, 16, 16)), (torch.ones(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))]
    out = fa.evaluate_pairs(None, pairs)
    assert list(out) == ["psnr", "ssim", "mse", "nmi"] and out["mse"] == 2.0
    mod = Mod()
    out = fa.evaluate_pairs(None, pairs, ms_ssim=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "ms_ssim"]
    assert out["ms_ssim"] == pytest.approx((0.25 + 0.75 + 0.25) / 3) and out["psnr"] == 0.0
    assert len(mod.calls) == 2 and all(p is True for _, _, p in mod.calls)
    assert torch.equal(mod.calls[0][0], pairs[0][0] * 2) and mod.calls[0][1] is pairs[0][1]      # (super_resolve(lr), hr)
    assert asked == [None] * 4                                            # image_metrics keeps its call
    out = fa.evaluate_pairs(None, pairs, cw_ssim="cw", ms_ssim=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "cw_ssim", "ms_ssim"] and out["cw_ssim"] == 4.0
    assert out["ms_ssim"] == pytest.approx((0.25 + 0.75 + 0.25) / 3) and asked[4:] == ["cw", "cw"]
    assert fa.evaluate_pairs(None, [], ms_ssim=mod) == {"psnr": 0.0, "ssim": 0.0, "mse": 0.0, "nmi": 0.0, "ms_ssim": 0.0}
    sig = inspect.signature(fa.image_metrics)
    assert list(sig.parameters) == ["y", "gt", "data_range", "bins", "cw_ssim"]
