"""GMSD (Xue, Zhang, Mou & Bovik 2014) and MS-GMSD (Zhang, Shen, Wang & Li 2017) without a GPU.  The definition:

    Inputs a, b of (N, C, H, W), fp32; channels are independent grey planes pooled inside an image, there is no chroma term.
    u = (x - lo) / (hi - lo) with value_range = (lo, hi), default (-1, 1), hi > lo.
    pool(t) = avg_pool2d(t, 2): floor pooling, an odd last row or column is dropped.
    Prewitt gradients, zero padding 1, the size of their input:
        gx_p = (1/3) sum_{dy = -1..1} (t[y + dy][x - 1] - t[y + dy][x + 1]),  gy_p the same on the other axis,
        m_p = sqrt(gx_p^2 + gy_p^2), no epsilon.
    g_p = (2 ma_p mb_p + c) / (ma_p^2 + mb_p^2 + c), c = 0.0026 by default (170 / 255^2).
    V[n] = the population variance of g_p over the channels and positions of image n.
    GMSD[n] = sqrt(V[n]) on the once-pooled pair pool(u_a), pool(u_b); sides at least 2.
    MS-GMSD[n] = sqrt(sum_j w_j V_j[n]); scale 1 is the mapped input itself, scale j + 1 = pool(scale j); weights default to
        (0.096, 0.596, 0.289, 0.019); 1 <= M <= 5 weights, each finite and >= 0, not all zero; sides at least 2^(M - 1); a scale of
        weight 0 contributes exactly nothing, hence ms_gmsd(x, y, weights=(0, 1)) == gmsd(x, y).
    Both are distortions: 0 for identical images, larger is worse; the batch mean as a 0-d tensor, or (N,) per image; gradients reach
    both images; the value itself is the loss.  Where m_p == 0 that image's direction (gx, gy) / m is taken as (0, 0); where an image's
    score is 0 its gradient is exactly zero.

Here: a plain-torch restatement (``F.pad`` / grouped ``F.conv2d`` / ``avg_pool2d``, the variance as mean((g - mean)^2), gradients by
autograd) pinned to tests/golden/golden_gmsd.npz, whose values come from explicit slice sums (tools/gen_golden_gmsd.py; there also
checked against central differences), and the host logic of ``ops.gmsd``, ``ops.ms_gmsd``, ``ssim.GMSD``, ``ssim.MSGMSD`` and
``TrainStep(gmsd_weight=...)`` (everything that raises before an entry point is reached).

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (scores: absolute difference over |score|; arrays: relative
L2).  The restatement in fp32 against the fixture's float64 values: 1e-5.  Central differences along a random direction: 1e-5.

The conditioning caps, asserted on the float64 restatement before every gradient comparison; nothing is excluded from a comparison:
over both images and every scale of positive weight min_p m_p >= 2^-10 in mapped units (sqrt is not differentiable at 0); per image
and scale mean(d^2) / V <= 8 with d = 1 - g (the variance is a difference of two means); every score > 0.  Inputs: x = 2 x the
5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = x + 0.1 noise, rounded to values float16 holds exactly; off the fixture
``find_pair`` takes the first seed of range(2000) that qualifies.  Seed 0 meets all three caps at every fixture shape: min m is
1.9e-3 .. 2.4e-1 and mean(d^2) / V is 1.08 .. 1.29.

The seam cases.  ``kernel_tiles()`` reads the tiles out of csrc/gmsd.hip: ``gmsd_index`` 16 x 64 (rows x columns), ``gmsd_grad`` 16 x 32.
(2, 1, 40, 136) has, for the pooled forms (a 20 x 68 map) and for the forms that take a scale as it is (40 x 136, then 20 x 68), at
least one full tile and a ragged remainder per axis, and a second plane behind the ragged tiles.

The fixture keeps a plain-GMSD gradient as one value per 2 x 2 pooling cell (the four are one value, a dropped row or column is zero:
asserted where the fixture is written); ``gold()`` spreads them again.  Its eleven cases have 74 276 gradient entries in float64 (42 778
as stored), which no coding brings under the 305 698 bytes of golden_haarpsi.npz at the 1e-12 of the float64 comparison (about 5 bytes
an entry, before the 48 082 input samples): it is 519 779 bytes."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_gmsd.npz")
MIN_M, MAX_RATIO = 2.0 ** -10, 8.0
MS_WEIGHTS = (0.096, 0.596, 0.289, 0.019)
#: (case, shape, weights (None: plain GMSD), c, value range, per image, y needs a gradient, the case whose inputs it shares): the table
#: of tools/gen_golden_gmsd.py
CASES = (("g8", (1, 1, 8, 8), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("mean", (2, 1, 16, 16), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("xonly", (2, 1, 16, 16), None, 0.0026, (-1.0, 1.0), False, False, "mean"),
         ("per_image_cfg", (2, 2, 32, 48), None, 0.01, (0.0, 2.0), True, True, None),
         ("channels", (1, 3, 16, 24), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("odd", (1, 1, 37, 53), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("seam", (2, 1, 40, 136), None, 0.0026, (-1.0, 1.0), False, True, None),
         ("ms", (2, 1, 32, 48), MS_WEIGHTS, 0.0026, (-1.0, 1.0), False, True, None),
         ("ms_odd", (1, 1, 37, 53), MS_WEIGHTS, 0.0026, (-1.0, 1.0), False, True, "odd"),
         ("ms_seam", (2, 1, 40, 136), MS_WEIGHTS, 0.0026, (-1.0, 1.0), False, True, "seam"),
         ("ms2", (1, 1, 16, 16), (0.3, 0.7), 0.0026, (-1.0, 1.0), False, True, None))
NEW_SYMBOLS = ("faoctasr_gmsd_workspace_floats", "faoctasr_gmsd_index", "faoctasr_gmsd_final", "faoctasr_gmsd_grad")
_gold = {}
_restated = {}


def spread(q, shape):
    """A plain-GMSD gradient from its one value per 2 x 2 cell: zero on a dropped row or column."""
    full = np.zeros(shape, dtype=q.dtype)
    h, w = shape[-2] // 2, shape[-1] // 2
    full[..., :2 * h, :2 * w] = np.repeat(np.repeat(q, 2, axis=-2), 2, axis=-1)
    return full


def gold():
    """The fixture, with the fp32 run's gradients put back together, ``float32(dx) + dx_delta`` (exact, tools/gen_golden_gmsd.py), and
    the plain-GMSD gradients spread over their cells."""
    if not _gold:
        with np.load(GOLDEN) as z:
            _gold.update({k: z[k] for k in z.files})
        for k in [k for k in _gold if k.endswith("_delta")]:
            case, _, name = k.split("/")
            _gold["%s/f32/%s" % (case, name[:-6])] = _gold["%s/%s" % (case, name[:-6])].astype(np.float32) + _gold[k]
        for case in CASES:
            if case[2] is None:
                for k in ("dx", "dy", "f32/dx", "f32/dy"):
                    if "%s/%s" % (case[0], k) in _gold:
                        _gold["%s/%s" % (case[0], k)] = spread(_gold["%s/%s" % (case[0], k)], case[1])
    return _gold


def kernel_tiles():
    """((GF_TY, GF_TX), (GB_TY, GB_TX)): the tiles of ``gmsd_index`` and ``gmsd_grad``, read out of csrc/gmsd.hip."""
    import faoctasr
    with open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "csrc", "gmsd.hip")) as f:
        src = f.read()
    v = {name: int(re.search(r"constexpr int [^;]*\b%s = (\d+)\b" % name, src).group(1)) for name in ("GF_TY", "GF_TX", "GB_TY", "GB_TX")}
    return (v["GF_TY"], v["GF_TX"]), (v["GB_TY"], v["GB_TX"])


def case_name(case):
    return case[0]


def fixture_inputs(case):
    g = gold()
    src = case[7] or case[0]
    return torch.from_numpy(g[src + "/x"].astype(np.float32)), torch.from_numpy(g[src + "/y"].astype(np.float32))


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
def magnitude(t):
    ch = t.shape[1]
    kx = torch.tensor([[1.0, 0.0, -1.0]] * 3, dtype=t.dtype) / 3.0
    k = torch.stack((kx, kx.t()))[:, None].repeat(ch, 1, 1, 1)                       # per channel: gx, then gy
    g = F.conv2d(F.pad(t, (1, 1, 1, 1)), k, groups=ch)
    return torch.sqrt(g[:, 0::2] ** 2 + g[:, 1::2] ** 2)


def restate(x, y, weights=None, c=0.0026, value_range=(-1.0, 1.0), per_image=False, x_grad=True, y_grad=True, dtype=torch.float64,
            upstream=None):
    """{"score", "rows", "dx", "dy", "min_m", "ratio"} in ``dtype``; ``weights`` None is plain GMSD.  The score is the mean over n, or
    (N,) with ``per_image``; the gradients are those of ``(score * upstream).sum()`` (upstream 1 by default); ``min_m`` is the smallest
    gradient magnitude of either image over the scales of positive weight, ``ratio`` the largest mean(d^2) / V."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(y_grad)
    lo, hi = value_range
    a, b = (x - lo) / (hi - lo), (y - lo) / (hi - lo)
    scales = [(1.0, F.avg_pool2d(a, 2), F.avg_pool2d(b, 2))] if weights is None else []
    for j, w in enumerate(weights or ()):
        if j:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
        scales.append((float(w), a, b))
    acc, min_m, ratio = 0, float("inf"), 0.0
    for w, a, b in scales:
        if w > 0:
            ma, mb = magnitude(a), magnitude(b)
            g = (2 * ma * mb + c) / (ma * ma + mb * mb + c)
            V = ((g - g.mean(dim=(1, 2, 3), keepdim=True)) ** 2).mean(dim=(1, 2, 3))
            acc = acc + w * V
            d = (1 - g).detach()
            min_m = min(min_m, float(ma.detach().min()), float(mb.detach().min()))
            ratio = max(ratio, float(((d * d).mean(dim=(1, 2, 3)) / V.detach().clamp_min(1e-300)).max()))
    rows = torch.sqrt(acc)
    score = rows if per_image else rows.mean()
    out = {"score": score.detach(), "rows": rows.detach(), "min_m": min_m, "ratio": ratio}
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
        _, _, weights, c, vr, per_image, y_grad, _ = case
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, weights, c, vr, per_image, True, y_grad, dtype)
    return _restated[key]


def well_conditioned(ref64):
    """The conditioning caps of every gradient comparison."""
    assert ref64["min_m"] >= MIN_M, ref64["min_m"]
    assert ref64["ratio"] <= MAX_RATIO, ref64["ratio"]
    assert float(ref64["rows"].min()) > 0, ref64["rows"]


def smooth(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed):
    """x = 2 x the 5 x 5-box-smoothed N(0, 1) noise, y = x + 0.1 noise, both exact in float16."""
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.randn(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    x = 2.0 * smooth(n1)
    y = x + 0.1 * n2
    return x.half().float(), y.half().float()


def find_pair(shape, weights=None, c=0.0026, value_range=(-1.0, 1.0)):
    """The pair of the first seed of range(2000) that meets the conditioning caps."""
    for seed in range(2000):
        x, y = make_pair(shape, seed)
        r = restate(x, y, weights, c, value_range, per_image=True, x_grad=False, y_grad=False)
        if r["min_m"] >= MIN_M and r["ratio"] <= MAX_RATIO and float(r["rows"].min()) > 0:
            return x, y
    raise AssertionError("no seed of range(2000) meets the conditioning caps for %s" % (shape,))


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_is_the_fixture(case):
    g = gold()
    cid, y_grad = case[0], case[6]
    ref = restate_case(case)
    well_conditioned(ref)
    assert ref["min_m"] == pytest.approx(float(g[cid + "/min_m"]), rel=1e-9) and ref["ratio"] == pytest.approx(float(g[cid + "/ratio"]), rel=1e-9)
    assert ref["score"].shape == g[cid + "/score"].shape == ((case[1][0],) if case[5] else ())
    assert score_err(ref["score"], g[cid + "/score"]) <= 1e-12
    assert g[cid + "/dx"].shape == case[1] and rel_l2(ref["dx"], g[cid + "/dx"]) <= 1e-12
    assert ((cid + "/dy") in g) == y_grad == ("dy" in ref)
    if y_grad:
        assert rel_l2(ref["dy"], g[cid + "/dy"]) <= 1e-12
    # the fixture's fp32 run: only the error it defines
    assert g[cid + "/f32/score"].dtype == np.float32 and g[cid + "/f32/dx"].dtype == np.float32
    assert score_err(g[cid + "/f32/score"], ref["score"]) <= 1e-5
    for k in ("dx", "dy") if y_grad else ("dx",):
        assert 0 < rel_l2(g["%s/f32/%s" % (cid, k)], ref[k]) <= 1e-5


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_in_fp32_is_the_fixture_at_fp32_tolerance(case):
    g = gold()
    cid = case[0]
    well_conditioned(restate_case(case))
    r32 = restate_case(case, torch.float32)
    assert r32["score"].dtype == torch.float32 and r32["dx"].dtype == torch.float32
    assert score_err(r32["score"], g[cid + "/score"]) <= 1e-5
    for k in ("dx", "dy") if case[6] else ("dx",):
        assert rel_l2(r32[k], g["%s/%s" % (cid, k)]) <= 1e-5


def test_fixture_inputs_are_exact():
    g = gold()
    assert os.path.getsize(GOLDEN) <= 1 << 20
    for case in CASES:
        if case[7] is None:
            x = g[case[0] + "/x"]
            assert x.dtype == np.float16 and g[case[0] + "/y"].dtype == np.float16 and x.shape == case[1]
            assert len(np.unique(x)) > x.size // 2                        # no flat regions
            fx, fy = fixture_inputs(case)
            assert fx.dtype == torch.float32 and fy.dtype == torch.float32
        else:
            assert case[0] + "/x" not in g
            assert [c for c in CASES if c[0] == case[7]][0][1] == case[1]


def test_seam_cases_cross_the_kernels_tiles():
    """The seam cases have at least one full tile and a ragged remainder per axis for every kernel form, with the tiles as csrc/gmsd.hip
    has them: the pooled forms work on the (H / 2) x (W / 2) map, the others on scale 1 as it is (and on the same map at scale 2); a
    second plane starts behind the ragged tiles."""
    tiles = kernel_tiles()
    assert all(t > 0 for pair in tiles for t in pair)
    for name, maps in (("seam", lambda H, W: [(H // 2, W // 2)]), ("ms_seam", lambda H, W: [(H, W), (H // 2, W // 2)])):
        (_, (N, C, H, W), *_), = [c for c in CASES if c[0] == name]
        assert N * C > 1
        for h, w in maps(H, W):
            for ty, tx in tiles:
                assert h // ty >= 1 and h % ty and w // tx >= 1 and w % tx, (name, h, w, ty, tx)


def test_symmetric():
    x, y = make_pair((2, 1, 21, 18), 6)
    for weights in (None, MS_WEIGHTS[:3]):
        a, b = restate(x, y, weights, per_image=True), restate(y, x, weights, per_image=True)
        assert score_err(a["score"], b["score"]) <= 1e-14
        assert rel_l2(a["dx"], b["dy"]) <= 1e-12 and rel_l2(a["dy"], b["dx"]) <= 1e-12


def test_ms_gmsd_with_weights_0_1_is_gmsd():
    x, y = make_pair((2, 2, 21, 18), 3)
    a, b = restate(x, y, (0, 1), per_image=True), restate(x, y, None, per_image=True)
    assert score_err(a["score"], b["score"]) <= 1e-14
    assert rel_l2(a["dx"], b["dx"]) <= 1e-13 and rel_l2(a["dy"], b["dy"]) <= 1e-13


def test_identical_images_score_zero():
    x, _ = make_pair((2, 1, 16, 24), 1)
    for weights in (None, MS_WEIGHTS):
        r = restate(x, x, weights, per_image=True, x_grad=False, y_grad=False)
        assert float(r["rows"].abs().max()) == 0.0


def test_degenerate_shapes():
    """(1, 1, 2, 2) under GMSD pools to one position: the variance of one value is 0.  (1, 1, 8, 8) at M = 4 reaches a 1 x 1 scale, whose
    Prewitt response under zero padding is 0 for both images: g = 1 there and the scale adds nothing."""
    x, y = make_pair((1, 1, 2, 2), 0)
    assert float(restate(x, y, None, x_grad=False, y_grad=False)["score"]) == 0.0
    x, y = make_pair((1, 1, 8, 8), 0)
    full = restate(x, y, MS_WEIGHTS, x_grad=False, y_grad=False)
    three = restate(x, y, MS_WEIGHTS[:3], x_grad=False, y_grad=False)
    assert float(full["score"]) > 0 and float(full["score"]) == float(three["score"]) and full["min_m"] == 0.0


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS[:3]), ids=("gmsd", "ms_gmsd"))
def test_restated_gradient_is_the_derivative(weights):
    """Central differences in float64 along a random direction, (1, 2, 19, 23): odd sides."""
    x, y = find_pair((1, 2, 19, 23), weights)
    ref = restate(x, y, weights)
    well_conditioned(ref)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    h = 1e-6
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + h * v, y) if which == 0 else (x, y.double() + h * v)), weights, x_grad=False, y_grad=False)
        dn = restate(*((x.double() - h * v, y) if which == 0 else (x, y.double() - h * v)), weights, x_grad=False, y_grad=False)
        num, ana = (float(up["score"]) - float(dn["score"])) / (2 * h), float((ref[key] * v).sum())
        assert abs(num - ana) <= 1e-5 * abs(ana), (key, num, ana)


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_exports_and_symbols(fa):
    assert fa.GMSD is fa.ssim.GMSD and fa.MSGMSD is fa.ssim.MSGMSD and "GMSD" in fa.__all__ and "MSGMSD" in fa.__all__
    assert callable(fa.ops.gmsd) and callable(fa.ops.ms_gmsd) and callable(fa.ssim.gmsd) and callable(fa.ssim.ms_gmsd)
    assert fa.ops.MSGMSD_WEIGHTS == MS_WEIGHTS and fa.ops.GMSD_MAX_SCALES == 5
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    assert sorted(s for s in declared if "_gmsd_" in s) == sorted(NEW_SYMBOLS)
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"gmsd.hip"' in src
    assert os.path.exists(os.path.join(os.path.dirname(fa._lib.__file__), "csrc", "gmsd.hip"))


def test_signatures(fa):
    empty = inspect.Parameter.empty
    sig = inspect.signature(fa.ops.gmsd)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("a", empty), ("b", empty), ("c", 0.0026), ("value_range", (-1., 1.)), ("per_image", False)]
    sig = inspect.signature(fa.ops.ms_gmsd)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("a", empty), ("b", empty), ("weights", None), ("c", 0.0026), ("value_range", (-1., 1.)), ("per_image", False)]
    sig = inspect.signature(fa.GMSD.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("c", 0.0026), ("value_range", (-1., 1.)), ("size_average", True)]
    sig = inspect.signature(fa.MSGMSD.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("weights", None), ("c", 0.0026), ("value_range", (-1., 1.)), ("size_average", True)]
    sig = inspect.signature(fa.ssim.gmsd)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("img1", empty), ("img2", empty), ("c", 0.0026), ("value_range", (-1., 1.)), ("size_average", True)]
    sig = inspect.signature(fa.ssim.ms_gmsd)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("img1", empty), ("img2", empty), ("weights", None), ("c", 0.0026), ("value_range", (-1., 1.)), ("size_average", True)]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("gmsd_weight", "gmsd_multiscale", "gmsd_c")] == [0.0, False, 0.0026]
    names = list(sig.parameters)
    at = names.index("haarpsi_alpha")
    assert names[at + 1:at + 5] == ["gmsd_weight", "gmsd_multiscale", "gmsd_c", "lncc_weight"]     # between haarpsi_alpha and lncc_weight
    for cls in (fa.GMSD, fa.MSGMSD):
        assert list(inspect.signature(cls.index).parameters)[1:] == ["img1", "img2", "per_image"]
        assert list(inspect.signature(cls.forward).parameters)[1:] == ["img1", "img2"]


def test_module_attributes(fa):
    mod = fa.GMSD()
    assert (mod.c, mod.value_range, mod.size_average) == (0.0026, (-1.0, 1.0), True)
    assert not list(mod.state_dict())
    mod = fa.GMSD(c=1, value_range=(0, 255), size_average=False)
    assert (mod.c, mod.value_range, mod.size_average) == (1.0, (0.0, 255.0), False) and isinstance(mod.c, float)
    assert "c=1.0" in repr(mod)
    mod = fa.MSGMSD()
    assert (mod.weights, mod.c, mod.value_range, mod.size_average) == (MS_WEIGHTS, 0.0026, (-1.0, 1.0), True)
    assert not list(mod.state_dict())
    mod = fa.MSGMSD(weights=[0, 1], c=0.01, value_range=(0, 1), size_average=False)
    assert (mod.weights, mod.c, mod.value_range, mod.size_average) == ((0.0, 1.0), 0.01, (0.0, 1.0), False)
    assert "weights=(0.0, 1.0)" in repr(mod)


def test_modules_pass_their_settings_on(fa, monkeypatch):
    seen = []
    monkeypatch.setattr(fa.ops, "gmsd", lambda *a: seen.append(("g",) + a[2:]) or "r")
    monkeypatch.setattr(fa.ops, "ms_gmsd", lambda *a: seen.append(("m",) + a[2:]) or "s")
    x = torch.zeros(1, 1, 16, 16)
    assert fa.GMSD(c=0.01, value_range=(0, 2))(x, x) == "r"
    assert fa.GMSD(size_average=False).index(x, x, False) == "r"
    assert fa.GMSD(size_average=False)(x, x) == "r"
    assert fa.ssim.gmsd(x, x, 0.5, (0., 1.), False) == "r"
    assert fa.MSGMSD(weights=(0.3, 0.7), c=0.01, value_range=(0, 2))(x, x) == "s"
    assert fa.MSGMSD(size_average=False).index(x, x, False) == "s"
    assert fa.ssim.ms_gmsd(x, x, (1, 2), 0.5, (0., 1.), False) == "s"
    assert fa.ssim.ms_gmsd(x, x) == "s"
    assert seen == [("g", 0.01, (0.0, 2.0), False), ("g", 0.0026, (-1.0, 1.0), False), ("g", 0.0026, (-1.0, 1.0), True),
                    ("g", 0.5, (0., 1.), True), ("m", (0.3, 0.7), 0.01, (0.0, 2.0), False), ("m", MS_WEIGHTS, 0.0026, (-1.0, 1.0), False),
                    ("m", (1, 2), 0.5, (0., 1.), True), ("m", None, 0.0026, (-1., 1.), False)]


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    x = torch.zeros(1, 1, 32, 32)
    for f, mod in ((fa.ops.gmsd, fa.GMSD), (fa.ops.ms_gmsd, fa.MSGMSD)):
        with pytest.raises(ValueError, match="device"):
            f(x, x)
        for bad in (0.0, -1e-5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="c must be positive"):
                f(x, x, c=bad)
            with pytest.raises(ValueError, match="c must be positive"):
                mod(c=bad)
        for bad in ("1e-5", None, True, torch.tensor(1e-5)):
            with pytest.raises(TypeError, match="c must be a number"):
                f(x, x, c=bad)
            with pytest.raises(TypeError, match="c must be a number"):
                mod(c=bad)
        for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0)):
            with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
                f(x, x, value_range=bad)
            with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
                mod(value_range=bad)
        for bad in (1.0, (1.0,), (0.0, 1.0, 2.0), None):
            with pytest.raises(TypeError, match="value_range must be a pair"):
                f(x, x, value_range=bad)
        for bad in (("0", "1"), (None, 1.0), (False, True)):
            with pytest.raises(TypeError, match="value_range must hold two numbers"):
                f(x, x, value_range=bad)
        with pytest.raises(TypeError, match="float32"):
            f(x.double(), x.double())
        with pytest.raises(TypeError, match="float32"):
            f(x, x.half())
        with pytest.raises(TypeError, match="tensor"):
            f(x, x.numpy())
        with pytest.raises(TypeError, match="tensor"):
            f([[1.0]], x)
        with pytest.raises(ValueError, match="same shape"):
            f(x, torch.zeros(1, 1, 32, 16))
        with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
            f(x[0], x[0])
        for shape in ((0, 1, 32, 32), (1, 0, 32, 32), (1, 1, 0, 32), (1, 1, 32, 0)):
            with pytest.raises(ValueError, match="non-empty"):
                f(torch.zeros(shape), torch.zeros(shape))
        # scalar refusals come before tensor refusals, the device check last
        with pytest.raises(ValueError, match="c must be positive"):
            f(x.double(), x[0], c=0.0)
        with pytest.raises(ValueError, match="value_range"):
            f("no tensor", x, value_range=(1.0, 0.0))
        with pytest.raises(TypeError, match="float32"):
            f(x.double(), x.double()[0])
        with pytest.raises(ValueError, match="same shape"):
            f(x, torch.zeros(1, 1, 8, 8))
        m = mod()
        with pytest.raises(ValueError, match="device"):
            m(x, x)
        with pytest.raises(ValueError, match="device"):
            m.index(x, x, True)
    with pytest.raises(ValueError, match="device"):
        fa.ssim.gmsd(x, x)
    with pytest.raises(ValueError, match="device"):
        fa.ssim.ms_gmsd(x, x)
    # the minimum side: 2 for GMSD, 2^(M - 1) for MS-GMSD
    with pytest.raises(ValueError, match="every side must be at least 2, got 1 x 32"):
        fa.ops.gmsd(torch.zeros(1, 1, 1, 32), torch.zeros(1, 1, 1, 32))
    with pytest.raises(ValueError, match="device"):
        fa.ops.gmsd(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))
    with pytest.raises(ValueError, match="every side must be at least 8, got 32 x 7"):
        fa.ops.ms_gmsd(torch.zeros(1, 1, 32, 7), torch.zeros(1, 1, 32, 7))
    with pytest.raises(ValueError, match="device"):
        fa.ops.ms_gmsd(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError, match="every side must be at least 16"):
        fa.ops.ms_gmsd(torch.zeros(1, 1, 15, 16), torch.zeros(1, 1, 15, 16), weights=(1, 1, 1, 1, 1))
    with pytest.raises(ValueError, match="device"):
        fa.ops.ms_gmsd(torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1), weights=(1,))
    # the weights rule
    f = fa.ops.ms_gmsd
    for bad in ((), (1, 1, 1, 1, 1, 1)):
        with pytest.raises(ValueError, match="one weight per scale"):
            f(x, x, weights=bad)
        with pytest.raises(ValueError, match="one weight per scale"):
            fa.MSGMSD(weights=bad)
    for bad in ((-0.1, 1.0), (float("nan"), 1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="every weight must be finite and >= 0"):
            f(x, x, weights=bad)
        with pytest.raises(ValueError, match="every weight must be finite and >= 0"):
            fa.MSGMSD(weights=bad)
    for bad in ((0.0,), (0, 0, 0)):
        with pytest.raises(ValueError, match="must not all be zero"):
            f(x, x, weights=bad)
    for bad in (("1", "2"), (None,), (True, 1.0), 1.0, (torch.tensor(1.0),)):
        with pytest.raises(TypeError, match="weights must"):
            f(x, x, weights=bad)
        with pytest.raises(TypeError, match="weights must"):
            fa.MSGMSD(weights=bad)
    with pytest.raises(ValueError, match="one weight per scale"):
        f(x.double(), x[0], weights=())


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = {"GMSD": fa.train.GMSD, "MSGMSD": fa.train.MSGMSD}

    def record(name):
        def make(**kw):
            built.append((name, kw))
            return real[name](**kw)
        return make
    monkeypatch.setattr(fa.train, "GMSD", record("GMSD"))
    monkeypatch.setattr(fa.train, "MSGMSD", record("MSGMSD"))
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.gmsd_weight == 0.0 and ts.gmsd is None and not built
    ts = fa.TrainStep(*nets, device="cpu", gmsd_multiscale=True, gmsd_c=0.01)
    assert ts.gmsd is None and not built
    ts = fa.TrainStep(*nets, device="cpu", gmsd_weight=0.25, gmsd_c=0.01)
    assert built == [("GMSD", dict(c=0.01))]
    assert ts.gmsd_weight == 0.25 and (ts.gmsd.c, ts.gmsd.value_range, ts.gmsd.size_average) == (0.01, (-1.0, 1.0), True)
    assert ts.msssim is None and ts.haarpsi is None and ts.lncc is None and ts.mi is None
    ts = fa.TrainStep(*nets, device="cpu", gmsd_weight=0.5, gmsd_multiscale=True)
    assert built[1:] == [("MSGMSD", dict(c=0.0026))]
    assert (ts.gmsd.weights, ts.gmsd.c, ts.gmsd.size_average) == (MS_WEIGHTS, 0.0026, True)
    with pytest.raises(ValueError, match="c must be positive"):
        fa.TrainStep(*nets, device="cpu", gmsd_weight=0.25, gmsd_c=0.0)
    for bad in (-1.0, float("nan"), float("inf"), "1", None):               # validated as lncc_weight is
        with pytest.raises(ValueError, match="gmsd_weight must be a finite number >= 0"):
            fa.TrainStep(*nets, device="cpu", gmsd_weight=bad)


def test_train_step_adds_the_term_where_loss_haarpsi_is_added(fa):
    """``_extension_terms`` (one half per chain of the two-chain schedule, which ``GraphedTrainStep`` captures) names ``loss_gmsd``; with
    the module replaced by a stub no kernel runs (the single-stream ``generator_loss``: tests/test_train_terms_cpu.py)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu", gmsd_weight=0.5)
    ts.gmsd = lambda rec, real: (rec * real).mean()
    rec, real = torch.full((1, 1, 4, 4), 0.5), torch.full((1, 1, 4, 4), 0.5)
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_gmsd"] and float(t["loss_gmsd"]) == 0.5 * 0.25
    assert fa.TrainStep(*nets, device="cpu")._extension_terms(rec, real) == {}
    assert not hasattr(fa.GraphedTrainStep, "generator_loss")              # it captures the TrainStep's own terms
