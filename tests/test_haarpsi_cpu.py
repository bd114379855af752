"""HaarPSI without a GPU: a plain-torch float64 restatement of

    u = (x - lo) 255 / (hi - lo),  u2 = the 2 x 2 mean of u at every second pixel (samples beyond the image 0, divisor 4),
    g^o_k = the Haar coefficients of u2 on 2^k x 2^k windows, k = 1, 2, 3, o in {v, h}:  ``F.pad`` by (K/2 - 1, K/2) per axis and a
            grouped ``F.conv2d`` with the +-2^-k kernel,  a_k = |g^o_k(x)|,  b_k = |g^o_k(y)|,
    S_o = 1/2 sum_{k = 1, 2} (2 a_k b_k + c) / (a_k^2 + b_k^2 + c),  W_o = max(a_3, b_3)  (the gradient of a tie goes to a_3),
    r[n] = sum_{ch, o, p} sigmoid(alpha S_o) W_o / sum W_o,  HaarPSI[n] = (log(r / (1 - r)) / alpha)^2,  1 where sum W_o == 0,

gradients by autograd; pinned to tests/golden/golden_haarpsi.npz, whose float64 values come from explicit slice sums
(tools/gen_golden_haarpsi.py; there also checked against central differences and the published ``convolve2d`` form), and the host
logic of ``ops.haarpsi``, ``ssim.HaarPSI``, ``ssim.haarpsi``, ``evaluate_pairs_with(haarpsi=...)`` and ``TrainStep(haarpsi_weight=...)``
(everything that raises before an entry point is reached).

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (scores: absolute difference over |score|; arrays: relative
L2): both sides are float64 sums of at most a few thousand terms.  The fixture's fp32 arrays are the fp32 reference: they enter only
through the error they define (e_ref, E_ref of tests/test_gpu_haarpsi.py), bounded here by 1e-4 as a sanity check of the fixture.

The tie caps.  ``sign()`` and ``max()`` are discontinuous: one flipped coefficient moves a gradient by about 2 / sqrt(#coefficients).
Every gradient comparison therefore first asserts, on the float64 restatement and in the mapped 0..255 units, that the smallest
|g^o_k|, k = 1, 2, both orientations, both images, is at least 2^-9 and the smallest | |g^o_3(x)| - |g^o_3(y)| | at least 2^-7; nothing
is excluded from a comparison.  Inputs: x = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = x + 0.1 n, not clipped;
off the fixture ``find_pair`` takes the first seed of range(2000) that meets the caps and fails if none does.

The seam case.  (1, 1, 72, 264) -- two 16 x 64 index tiles and a remainder per axis -- has 38016 level-1 and -2 coefficients and 9504
level-3 differences: with densities near zero of about 0.06 and 0.13 per mapped unit some 9 + 19 of them fall below the caps on
average, and no seed of range(2000) qualifies.  The fixture therefore holds one seam per axis, (2, 1, 40, 136) (half-resolution
20 x 68: 16 + 4 rows, 64 + 4 columns for ``haarpsi_index``; 16 + 4 rows and four 16-column tiles + 4 for ``haarpsi_grad``), first seed 561."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_haarpsi.npz")
COEF_CAP, TIE_CAP = 2.0 ** -9, 2.0 ** -7
#: (case, shape, c, alpha, value_range, per image, y needs a gradient, the case whose inputs it shares): the table of tools/gen_golden_haarpsi.py
CASES = (("tiny", (1, 1, 8, 8), 30.0, 4.2, (-1.0, 1.0), False, True, None),
         ("mean", (2, 1, 16, 16), 30.0, 4.2, (-1.0, 1.0), False, True, None),
         ("per_image_cfg", (2, 2, 32, 48), 20.0, 3.5, (0.0, 1.0), True, True, None),
         ("channels", (1, 3, 16, 24), 30.0, 4.2, (-1.0, 1.0), False, True, None),
         ("odd", (1, 1, 37, 53), 30.0, 4.2, (-1.0, 1.0), False, True, None),
         ("seam", (2, 1, 40, 136), 30.0, 4.2, (-1.0, 1.0), False, True, None),
         ("xonly", (2, 1, 16, 16), 30.0, 4.2, (-1.0, 1.0), False, False, "mean"))
NEW_SYMBOLS = ("faoctasr_haarpsi_workspace_floats", "faoctasr_haarpsi_index", "faoctasr_haarpsi_final", "faoctasr_haarpsi_grad")
_gold = {}
_restated = {}


def gold():
    if not _gold:
        with np.load(GOLDEN) as z:
            _gold.update({k: z[k] for k in z.files})
    return _gold


def kernel_tiles():
    """((HF_TY, HF_TX), (HB_T, HB_T)): the tiles of the half-resolution map of ``haarpsi_index`` and ``haarpsi_grad``, read out of
    csrc/haarpsi.hip."""
    import faoctasr
    with open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "csrc", "haarpsi.hip")) as f:
        src = f.read()
    v = {name: int(re.search(r"constexpr int [^;]*\b%s = (\d+)\b" % name, src).group(1)) for name in ("HF_TY", "HF_TX", "HB_T")}
    return (v["HF_TY"], v["HF_TX"]), (v["HB_T"], v["HB_T"])


def case_name(case):
    return case[0]


def fixture_inputs(case):
    g = gold()
    src = case[7] or case[0]
    return torch.from_numpy(g[src + "/x"]), torch.from_numpy(g[src + "/y"])


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
def half_map(x, lo, hi):
    u = (x - lo) * 255 / (hi - lo)
    return F.avg_pool2d(F.pad(u, (0, x.shape[-1] % 2, 0, x.shape[-2] % 2)), 2)


def haar(u2, k):
    """(g^v_k, g^h_k) of a (N, C, h, w) map."""
    K, ch = 2 ** k, u2.shape[1]
    kv = torch.full((K, K), 2.0 ** -k, dtype=u2.dtype)
    kv[K // 2:] *= -1
    p = F.pad(u2, (K // 2 - 1, K // 2, K // 2 - 1, K // 2))
    return (F.conv2d(p, kv.expand(ch, 1, K, K).contiguous(), groups=ch), F.conv2d(p, kv.t().expand(ch, 1, K, K).contiguous(), groups=ch))


def restate(x, y, c=30.0, alpha=4.2, value_range=(-1.0, 1.0), per_image=False, x_grad=True, y_grad=True, dtype=torch.float64, upstream=None):
    """{"score", "dx", "dy", "coef_min", "tie_min"} in ``dtype``: the score is the mean over n, or (N,) with ``per_image``; the
    gradients are those of ``(score * upstream).sum()`` (upstream 1 by default); ``coef_min`` and ``tie_min`` are what the caps bound."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(y_grad)
    lo, hi = value_range
    u2, v2 = half_map(x, lo, hi), half_map(y, lo, hi)
    gx, gy = [haar(u2, k) for k in (1, 2, 3)], [haar(v2, k) for k in (1, 2, 3)]
    num, den = 0, 0
    coef_min, tie_min = float("inf"), float("inf")
    for o in (0, 1):
        S = 0
        for k in (0, 1):
            a, b = gx[k][o].abs(), gy[k][o].abs()
            S = S + (2 * a * b + c) / (a * a + b * b + c)
            coef_min = min(coef_min, float(a.detach().min()), float(b.detach().min()))
        a3, b3 = gx[2][o].abs(), gy[2][o].abs()
        tie_min = min(tie_min, float((a3 - b3).detach().abs().min()))
        Wt = torch.where(a3 >= b3, a3, b3)                                 # at equality the gradient goes to a_3
        num = num + (torch.sigmoid(alpha * (S / 2)) * Wt).sum(dim=(1, 2, 3))
        den = den + Wt.sum(dim=(1, 2, 3))
    dead = den == 0                                                        # no structure at the coarse scale: score 1, gradients exactly zero
    r = torch.where(dead, torch.full_like(num, 0.75), num / torch.where(dead, torch.ones_like(den), den))
    rows = torch.where(dead, torch.ones_like(r), (torch.log(r / (1 - r)) / alpha) ** 2)
    score = rows if per_image else rows.mean()
    out = {"score": score.detach(), "coef_min": coef_min, "tie_min": tie_min}
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
        _, _, c, alpha, value_range, per_image, y_grad, _ = case
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, c, alpha, value_range, per_image, True, y_grad, dtype)
    return _restated[key]


def well_conditioned(ref64):
    """The tie caps of every gradient comparison."""
    assert ref64["coef_min"] >= COEF_CAP, ref64["coef_min"]
    assert ref64["tie_min"] >= TIE_CAP, ref64["tie_min"]


def make_pair(shape, seed, noise=0.1):
    """x = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = x + noise n; not clipped."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(*shape, generator=g, dtype=torch.float32)
    x = 2.0 * F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(shape[1], 1, 5, 5) / 25.0, groups=shape[1])
    return x, x + noise * torch.randn(*shape, generator=g, dtype=torch.float32)


def find_pair(shape, c=30.0, alpha=4.2, value_range=(-1.0, 1.0)):
    """The pair of the first seed of range(2000) that meets the tie caps."""
    for seed in range(2000):
        x, y = make_pair(shape, seed)
        r = restate(x, y, c, alpha, value_range, x_grad=False, y_grad=False)
        if r["coef_min"] >= COEF_CAP and r["tie_min"] >= TIE_CAP:
            return x, y
    raise AssertionError("no seed of range(2000) meets the tie caps for %s" % (shape,))


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_is_the_fixture(case):
    g = gold()
    cid, y_grad = case[0], case[6]
    ref = restate_case(case)
    well_conditioned(ref)
    assert ref["coef_min"] == pytest.approx(float(g[cid + "/coef_min"]), rel=1e-9) and ref["tie_min"] == pytest.approx(float(g[cid + "/tie_min"]), rel=1e-9)
    assert ref["score"].shape == g[cid + "/score"].shape == ((case[1][0],) if case[5] else ())
    assert score_err(ref["score"], g[cid + "/score"]) <= 1e-12
    assert rel_l2(ref["dx"], g[cid + "/dx"]) <= 1e-12
    assert ((cid + "/dy") in g) == y_grad == ("dy" in ref)
    if y_grad:
        assert rel_l2(ref["dy"], g[cid + "/dy"]) <= 1e-12
    # the fp32 arrays: only the error they define
    assert g[cid + "/f32/score"].dtype == np.float32 and g[cid + "/f32/dx"].dtype == np.float32
    assert score_err(g[cid + "/f32/score"], ref["score"]) <= 1e-4
    for k in ("dx", "dy") if y_grad else ("dx",):
        assert 0 < rel_l2(g["%s/f32/%s" % (cid, k)], ref[k]) <= 1e-4


def test_fixture_is_small_and_its_inputs_are_fp32_and_unclipped():
    assert os.path.getsize(GOLDEN) < 1 << 20
    g = gold()
    for case in CASES:
        if case[7] is None:
            x = g[case[0] + "/x"]
            assert x.dtype == np.float32 and g[case[0] + "/y"].dtype == np.float32 and x.shape == case[1]
            assert len(np.unique(x)) > x.size // 2                        # no flat regions
        else:
            assert case[0] + "/x" not in g


def test_seam_case_crosses_the_kernels_tiles():
    """The fixture's seam case has at least one full tile and a ragged remainder per axis for both kernels, with the tiles as
    csrc/haarpsi.hip has them, and a second plane that starts behind a ragged tile."""
    (_, (N, C, H, W), *_), = [c for c in CASES if c[0] == "seam"]
    h, w = (H + 1) // 2, (W + 1) // 2
    tiles = kernel_tiles()
    assert all(t > 0 for pair in tiles for t in pair)
    for ty, tx in tiles:
        assert h // ty >= 1 and h % ty and w // tx >= 1 and w % tx, (h, w, ty, tx)
    assert N * C > 1


def test_identical_images_score_one():
    x, _ = make_pair((2, 2, 19, 23), 5)
    r = restate(x, x)
    assert abs(float(r["score"]) - 1.0) <= 1e-12
    rows = restate(x, x, per_image=True, x_grad=False, y_grad=False)["score"]
    assert float((rows - 1).abs().max()) <= 1e-12
    scale = max(float(restate(x, x + 0.1)["dx"].norm()), 1e-30)
    assert float(r["dx"].norm()) <= 1e-9 * scale and float(r["dy"].norm()) <= 1e-9 * scale


def test_symmetric_in_its_arguments():
    x, y = make_pair((2, 1, 21, 18), 6)
    a, b = restate(x, y, per_image=True), restate(y, x, per_image=True)
    assert torch.equal(a["score"], b["score"])
    assert rel_l2(a["dx"], b["dy"]) <= 1e-14 and rel_l2(a["dy"], b["dx"]) <= 1e-14


def test_flat_pair_scores_one_with_zero_gradients():
    """Both images at ``lo``: every mapped sample is 0, no coefficient, the denominator exactly 0."""
    for value_range in ((-1.0, 1.0), (0.0, 1.0)):
        z = torch.full((2, 1, 9, 12), value_range[0])
        r = restate(z, z.clone(), value_range=value_range, per_image=True)
        assert bool((r["score"] == 1).all()) and not r["dx"].any() and not r["dy"].any()
        assert not torch.isnan(r["dx"]).any() and not torch.isnan(r["dy"]).any()
    # one flat image pair beside a live one: only the live one carries a gradient
    x, y = make_pair((1, 1, 9, 12), 7)
    z = torch.full((1, 1, 9, 12), -1.0)
    r = restate(torch.cat((z, x)), torch.cat((z, y)), per_image=True)
    assert float(r["score"][0]) == 1.0 and 0 < float(r["score"][1]) < 1
    assert not r["dx"][0].any() and r["dx"][1].abs().max() > 0 and not torch.isnan(r["dx"]).any()


def test_score_decreases_as_the_noise_grows():
    x, _ = make_pair((1, 1, 48, 48), 8)
    n = torch.randn(x.shape, generator=torch.Generator().manual_seed(9))
    scores = [float(restate(x, x + s * n, x_grad=False, y_grad=False)["score"]) for s in (0.0, 0.02, 0.05, 0.1, 0.2, 0.4, 0.8)]
    assert scores[0] == pytest.approx(1.0, abs=1e-12) and all(a > b for a, b in zip(scores, scores[1:])) and 0 < scores[-1] < 0.6


def test_value_range_is_an_affine_map():
    """(x, (lo, hi)) and (s x + t, (s lo + t, s hi + t)) are the same mapped images."""
    x, y = make_pair((1, 2, 16, 20), 10)
    a = restate(x, y, x_grad=False, y_grad=False)["score"]
    b = restate(0.5 * x + 0.5, 0.5 * y + 0.5, value_range=(0.0, 1.0), x_grad=False, y_grad=False)["score"]
    assert abs(float(a) - float(b)) <= 1e-6 * float(a)                    # the inputs are fp32 values: 0.5 x + 0.5 rounds


def test_restated_gradient_is_the_derivative():
    """Central differences in float64 along a random direction, (1, 2, 19, 23): odd sides."""
    x, y = find_pair((1, 2, 19, 23))
    ref = restate(x, y)
    well_conditioned(ref)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    eps = 1e-7                      # |v| <= 5: a coefficient moves by at most 1e-4 mapped units, a twentieth of the smaller cap
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + eps * v, y) if which == 0 else (x, y.double() + eps * v)), x_grad=False, y_grad=False)
        dn = restate(*((x.double() - eps * v, y) if which == 0 else (x, y.double() - eps * v)), x_grad=False, y_grad=False)
        num, ana = (float(up["score"]) - float(dn["score"])) / (2 * eps), float((ref[key] * v).sum())
        assert abs(num - ana) <= 1e-5 * abs(ana), (key, num, ana)


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_exports_and_symbols(fa):
    assert fa.HaarPSI is fa.ssim.HaarPSI and "HaarPSI" in fa.__all__
    assert callable(fa.ops.haarpsi) and callable(fa.ssim.haarpsi)
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"haarpsi.hip"' in src
    assert os.path.exists(os.path.join(os.path.dirname(fa._lib.__file__), "csrc", "haarpsi.hip"))


def test_signatures(fa):
    empty = inspect.Parameter.empty
    sig = inspect.signature(fa.ops.haarpsi)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("a", empty), ("b", empty), ("c", 30.0), ("alpha", 4.2), ("value_range", (-1.0, 1.0)), ("per_image", False)]
    sig = inspect.signature(fa.HaarPSI.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("c", 30.0), ("alpha", 4.2), ("value_range", (-1.0, 1.0)), ("size_average", True)]
    sig = inspect.signature(fa.ssim.haarpsi)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("img1", empty), ("img2", empty), ("c", 30.0), ("alpha", 4.2), ("value_range", (-1.0, 1.0)), ("size_average", True)]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("haarpsi_weight", "haarpsi_c", "haarpsi_alpha")] == [0.0, 30.0, 4.2]
    sig = inspect.signature(fa.evaluate_pairs_with)
    assert [(k, v.default, v.kind) for k, v in sig.parameters.items()] == [
        ("model", empty, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("pairs", empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("cw_ssim", None, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("indices", empty, inspect.Parameter.VAR_KEYWORD)]
    sig = inspect.signature(fa.evaluate_pairs)                            # keeps its parameters: further indices go through evaluate_pairs_with
    assert list(sig.parameters) == ["model", "pairs", "cw_ssim", "ms_ssim"]
    assert list(inspect.signature(fa.HaarPSI.index).parameters)[1:] == ["img1", "img2", "per_image"]
    assert list(inspect.signature(fa.HaarPSI.forward).parameters)[1:] == ["img1", "img2"]


def test_module_attributes(fa):
    mod = fa.HaarPSI()
    assert (mod.c, mod.alpha, mod.value_range, mod.size_average) == (30.0, 4.2, (-1.0, 1.0), True)
    assert not list(mod.state_dict())
    mod = fa.HaarPSI(c=5, alpha=2, value_range=[0, 255], size_average=False)
    assert (mod.c, mod.alpha, mod.value_range, mod.size_average) == (5.0, 2.0, (0.0, 255.0), False)
    assert "alpha=2.0" in repr(mod)


def test_module_passes_its_settings_on(fa, monkeypatch):
    seen = []
    monkeypatch.setattr(fa.ops, "haarpsi", lambda *a: seen.append(a[2:]) or "r")
    x = torch.zeros(1, 1, 16, 16)
    assert fa.HaarPSI(c=10.0, alpha=3.0, value_range=(0.0, 1.0))(x, x) == "r"
    assert fa.HaarPSI(size_average=False).index(x, x, False) == "r"
    assert fa.HaarPSI(size_average=False)(x, x) == "r"
    assert fa.ssim.haarpsi(x, x, 20.0, 4.0, (0.0, 2.0), False) == "r"
    assert seen == [(10.0, 3.0, (0.0, 1.0), False), (30.0, 4.2, (-1.0, 1.0), False), (30.0, 4.2, (-1.0, 1.0), True), (20.0, 4.0, (0.0, 2.0), True)]


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    f = fa.ops.haarpsi
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="device"):
        f(x, x)
    with pytest.raises(ValueError, match="device"):
        f(torch.zeros(2, 3, 2, 2), torch.zeros(2, 3, 2, 2))                 # 2: the smallest side
    for shape in ((1, 1, 1, 8), (1, 1, 8, 1)):
        with pytest.raises(ValueError, match="at least 2"):
            f(torch.zeros(shape), torch.zeros(shape))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="c must be positive"):
            f(x, x, c=bad)
        with pytest.raises(ValueError, match="c must be positive"):
            fa.HaarPSI(c=bad)
        with pytest.raises(ValueError, match="alpha must be positive"):
            f(x, x, alpha=bad)
        with pytest.raises(ValueError, match="alpha must be positive"):
            fa.HaarPSI(alpha=bad)
    for bad in ("30", None, True, torch.tensor(30.0)):
        with pytest.raises(TypeError, match="c must be a number"):
            f(x, x, c=bad)
        with pytest.raises(TypeError, match="alpha must be a number"):
            fa.HaarPSI(alpha=bad)
    for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="hi > lo"):
            f(x, x, value_range=bad)
        with pytest.raises(ValueError, match="hi > lo"):
            fa.HaarPSI(value_range=bad)
    for bad in (2.0, (0.0, 1.0, 2.0), ("0", "1"), None):
        with pytest.raises(TypeError, match="value_range"):
            f(x, x, value_range=bad)
        with pytest.raises(TypeError, match="value_range"):
            fa.HaarPSI(value_range=bad)
    with pytest.raises(TypeError, match="float32"):
        f(x.double(), x.double())
    with pytest.raises(TypeError, match="float32"):
        f(x, x.half())
    with pytest.raises(TypeError, match="tensor"):
        f(x, x.numpy())
    with pytest.raises(ValueError, match="same shape"):
        f(x, torch.zeros(1, 1, 32, 16))
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        f(x[0], x[0])
    with pytest.raises(ValueError, match="non-empty"):
        f(torch.zeros(0, 1, 32, 32), torch.zeros(0, 1, 32, 32))
    mod = fa.HaarPSI()
    with pytest.raises(ValueError, match="device"):
        mod(x, x)
    with pytest.raises(ValueError, match="device"):
        mod.index(x, x, True)
    with pytest.raises(ValueError, match="device"):
        fa.ssim.haarpsi(x, x)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.HaarPSI

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "HaarPSI", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.haarpsi_weight == 0.0 and ts.haarpsi is None and not built
    ts = fa.TrainStep(*nets, device="cpu", haarpsi_weight=0.25, haarpsi_c=10.0, haarpsi_alpha=3.0)
    assert built == [dict(c=10.0, alpha=3.0)]
    assert ts.haarpsi_weight == 0.25 and (ts.haarpsi.c, ts.haarpsi.alpha, ts.haarpsi.value_range, ts.haarpsi.size_average) == (10.0, 3.0, (-1.0, 1.0), True)
    assert ts.msssim is None and ts.cwssim is None and ts.ffl is None and ts.mi is None
    with pytest.raises(ValueError, match="alpha"):
        fa.TrainStep(*nets, device="cpu", haarpsi_weight=0.25, haarpsi_alpha=0.0)


def test_train_step_terms_call_the_module(fa):
    """``_extension_terms`` names ``loss_haarpsi``; with the module replaced by a stub no kernel runs (``generator_loss``:
    tests/test_train_terms_cpu.py)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu", haarpsi_weight=0.5)
    ts.haarpsi = lambda rec, real: (rec * real).mean()
    rec, real = torch.full((1, 1, 4, 4), 0.5), torch.full((1, 1, 4, 4), 0.5)
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_haarpsi"] and float(t["loss_haarpsi"]) == 0.5 * (1 - 0.25)
    ts0 = fa.TrainStep(*nets, device="cpu")
    assert ts0._extension_terms(rec, real) == {}


def test_evaluate_pairs_with_keys(fa, monkeypatch):
    """With and without the module, ``image_metrics`` and ``super_resolve`` replaced: no kernel runs."""
    asked = []

    def metrics(y, gt, data_range=2.0, bins=100, cw_ssim=None):
        asked.append(cw_ssim)
        return torch.arange(4 if cw_ssim is None else 5, dtype=torch.float64).repeat(y.shape[0], 1)
    monkeypatch.setattr(fa.evaluate, "image_metrics", metrics)
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: lr * 2)

    class Mod:
        def __init__(self, values):
            self.values, self.calls = values, []

        def index(self, a, b, per_image):
            self.calls.append((a, b, per_image))
            return torch.tensor(self.values[:a.shape[0]])
    pairs = [(torch.ones(2, 1, 16, 16), torch.zeros(2, 1, 16, 16)), (torch.ones(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))]
    out = fa.evaluate_pairs_with(None, pairs)
    assert list(out) == ["psnr", "ssim", "mse", "nmi"] and out["mse"] == 2.0
    mod = Mod([0.25, 0.75])
    out = fa.evaluate_pairs_with(None, pairs, haarpsi=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "haarpsi"]
    assert out["haarpsi"] == pytest.approx((0.25 + 0.75 + 0.25) / 3) and out["psnr"] == 0.0
    assert len(mod.calls) == 2 and all(p is True for _, _, p in mod.calls)
    assert torch.equal(mod.calls[0][0], pairs[0][0] * 2) and mod.calls[0][1] is pairs[0][1]      # (super_resolve(lr), hr)
    assert asked == [None] * 4                                            # image_metrics keeps its call
    ms = Mod([0.5, 0.5])
    out = fa.evaluate_pairs_with(None, pairs, cw_ssim="cw", ms_ssim=ms, haarpsi=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "cw_ssim", "ms_ssim", "haarpsi"] and out["cw_ssim"] == 4.0 and out["ms_ssim"] == 0.5
    assert out["haarpsi"] == pytest.approx((0.25 + 0.75 + 0.25) / 3) and asked[4:] == ["cw", "cw"]
    assert fa.evaluate_pairs_with(None, [], haarpsi=mod) == {"psnr": 0.0, "ssim": 0.0, "mse": 0.0, "nmi": 0.0, "haarpsi": 0.0}
    out = fa.evaluate_pairs_with(None, pairs, haarpsi=mod, ms_ssim=None, other=ms)                   # keyword order; None adds nothing
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "haarpsi", "other"] and out["other"] == 0.5
    assert fa.evaluate_pairs(None, pairs, ms_ssim=ms) == fa.evaluate_pairs_with(None, pairs, ms_ssim=ms)
    for bad in ("haarpsi", 1.0, (mod,), [mod], object(), torch.nn.Identity()):                       # no index module: refused before a pair is read
        with pytest.raises(TypeError, match=r"haarspi must be a module with index"):
            fa.evaluate_pairs_with(None, iter(()), haarspi=bad)
    for taken in ("psnr", "ssim", "mse", "nmi"):
        with pytest.raises(ValueError, match="a key of the result already"):
            fa.evaluate_pairs_with(None, pairs, **{taken: mod})
    assert fa.evaluate_pairs_with is fa.evaluate.evaluate_pairs_with and "evaluate_pairs_with" in fa.__all__
    sig = inspect.signature(fa.image_metrics)
    assert list(sig.parameters) == ["y", "gt", "data_range", "bins", "cw_ssim"]
