"""The Hessian vesselness filter and the vessel Dice index without a GPU.  The definition:

    Inputs x, y of (N, C, H, W), fp32; channels are independent grey planes pooled inside an image; any sides >= 1.
    u = (x - lo) / (hi - lo) with value_range = (lo, hi), default (-1, 1), hi > lo.
    Per scale sigma: R = int(3 sigma + 0.5), t = -R..R, g = exp(-t^2 / (2 sigma^2)) normalised to sum 1, g1 = -t / sigma^2 g,
        g2 = (t^2 / sigma^4 - 1 / sigma^2) g: scipy's sampled kernels, nothing renormalised after the polynomial.
    a = sigma^2 (g2 along W, g along H) * u,  b = sigma^2 (g1, g1) * u,  d = sigma^2 (g along W, g2 along H) * u: true convolutions, zero
        padding, the size of the input; bright=False (dark ridges) negates a, b, d.
    m = (a + d) / 2, h = (a - d) / 2, r = sqrt(h^2 + b^2), kappa = r - m, mu = m + r (the eigenvalues ordered by value),
    E1 = mu^2 / (2 beta^2 kappa^2), E2 = (mu^2 + kappa^2) / (2 c^2),
    V = exp(-E1) (1 - exp(-E2)) where kappa > 0 and E1 < 87, exactly 0 with zero cotangents elsewhere.
    Rsp = sum_s w_s V_s over 1..3 sigmas in [0.5, 3]; weights default to equal, each finite and >= 0, not all zero, normalised to sum 1.
    S[n] = (2 mean(A B) + eps) / (mean(A^2) + mean(B^2) + eps), A = Rsp(x), B = Rsp(y), means over the channels and positions of image n.
    0 < S <= 1; 1 for identical images and for two vessel-free images; the batch mean as a 0-d tensor, or (N,) per image; gradients
    reach both images; the loss is 1 - S.  At r == 0 the direction (h, b) / r is taken as (0, 0).
    Defaults: sigmas (1, 2, 3), beta 0.5, c 0.1, eps 1e-6, value_range (-1, 1), bright.

Here: a plain-torch restatement (grouped ``F.conv2d`` with the kernels flipped into true convolutions, gradients by autograd) pinned to
tests/golden/golden_vessel.npz, whose values come from explicit slice sums (tools/gen_golden_vessel.py; there also checked against
scipy.ndimage.gaussian_filter and central differences), and the host logic of ``ops.vesselness``, ``ops.vessel_dice``,
``ssim.Vesselness``, ``ssim.VesselDice`` and ``TrainStep(vessel_weight=...)`` (everything that raises before an entry point is reached).

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (scores: absolute difference over |score|; arrays: relative
L2; the fixture keeps its float64 arrays to 41 significant bits, 2.3e-13 in the mean square).  The restatement in fp32 against the
fixture's float64 values: 1e-5.  Central differences along a random direction: 1e-5.

The conditioning caps, asserted on the float64 restatement before every gradient comparison; nothing is excluded from a comparison:
min r >= 2^-14 over both images and every scale of positive weight (sqrt is not differentiable at 0), every image's denominator
D >= 2^-6, every score > 0.  Inputs: x = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = x + 0.1 noise, rounded to
values float16 holds exactly; off the fixture ``find_pair`` takes the first seed of range(2000) that qualifies.  Seed 0 meets the caps
at every fixture shape: min r is 2.2e-4 .. 3.6e-3 and D is 0.139 .. 0.436.

The seam case.  ``kernel_tiles()`` reads the tiles out of csrc/vessel.hip: ``vessel_index`` 16 x 64 (rows x columns), ``vessel_grad``
16 x 32.  (2, 1, 40, 136) has two seams per axis of either tile and a second plane behind the ragged tiles."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vessel.npz")
MIN_R, MIN_D = 2.0 ** -14, 2.0 ** -6
E1_MAX = 87.0
DEFAULT = dict(sigmas=(1.0, 2.0, 3.0), weights=None, beta=0.5, c=0.1, eps=1e-6, value_range=(-1.0, 1.0), bright=True)
OTHER = dict(DEFAULT, sigmas=(1.5,), beta=0.7, c=0.05, value_range=(0.0, 2.0))
HALO = dict(DEFAULT, sigmas=(0.5, 3.0), weights=(1.0, 3.0))
DARK = dict(DEFAULT, bright=False)
#: (case, shape, settings, per image, y needs a gradient, the case whose inputs it shares, the filter alone): the table of
#: tools/gen_golden_vessel.py
CASES = (("v8", (1, 1, 8, 8), DEFAULT, False, True, None, False),
         ("mean", (2, 1, 16, 16), DEFAULT, False, True, None, False),
         ("xonly", (2, 1, 16, 16), DEFAULT, False, False, "mean", False),
         ("per_image_cfg", (2, 2, 32, 48), OTHER, True, True, None, False),
         ("channels", (1, 3, 16, 24), DEFAULT, False, True, None, False),
         ("odd", (1, 1, 37, 53), DEFAULT, False, True, None, False),
         ("seam", (2, 1, 40, 136), DEFAULT, False, True, None, False),
         ("halo", (1, 1, 5, 7), HALO, False, True, None, False),
         ("map_odd", (1, 1, 37, 53), DEFAULT, False, False, "odd", True),
         ("map_wide_dark", (1, 2, 18, 70), DARK, False, False, None, True))
NEW_SYMBOLS = ("faoctasr_vessel_workspace_floats", "faoctasr_vessel_index", "faoctasr_vessel_final", "faoctasr_vessel_grad")
_gold = {}
_restated = {}


def gold():
    """The fixture, with the fp32 run's arrays put back together from their bit-pattern distances (exact, tools/gen_golden_vessel.py) and
    the gradients of a case that shares an index case's inputs taken from that case."""
    if not _gold:
        with np.load(GOLDEN) as z:
            _gold.update({k: z[k] for k in z.files})
        for k in [k for k in _gold if k.endswith("_delta")]:
            case, _, name = k.split("/")
            near = np.ascontiguousarray(_gold["%s/%s" % (case, name[:-6])].astype(np.float32))
            _gold["%s/f32/%s" % (case, name[:-6])] = (near.view(np.int32) + _gold[k]).view(np.float32)
        for case in CASES:
            if case[5] is not None and not case[6]:
                for k in ("dx", "f32/dx"):
                    _gold["%s/%s" % (case[0], k)] = _gold["%s/%s" % (case[5], k)]
    return _gold


def kernel_tiles():
    """((VF_TY, VF_TX), (VB_TY, VB_TX)): the tiles of ``vessel_index`` and ``vessel_grad``, read out of csrc/vessel.hip."""
    import faoctasr
    with open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "csrc", "vessel.hip")) as f:
        src = f.read()
    v = {name: int(re.search(r"constexpr int [^;]*\b%s = (\d+)\b" % name, src).group(1)) for name in ("VF_TY", "VF_TX", "VB_TY", "VB_TX")}
    return (v["VF_TY"], v["VF_TX"]), (v["VB_TY"], v["VB_TX"])


def case_name(case):
    return case[0]


def fixture_inputs(case):
    """(x, y, cot): y None and cot the upstream map for a map case."""
    g = gold()
    src = case[5] or case[0]
    x = torch.from_numpy(g[src + "/x"].astype(np.float32))
    if case[6]:
        return x, None, torch.from_numpy(g[case[0] + "/cot"].astype(np.float32))
    return x, torch.from_numpy(g[src + "/y"].astype(np.float32)), None


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
def taps(sigma, dtype):
    R = int(3 * sigma + 0.5)
    t = torch.arange(-R, R + 1, dtype=torch.float64)
    g = torch.exp(-t * t / (2 * sigma * sigma))
    g = g / g.sum()
    return R, g.to(dtype), (-t / sigma ** 2 * g).to(dtype), ((t * t / sigma ** 4 - 1 / sigma ** 2) * g).to(dtype)


def hessian(u, sigma):
    """(a, b, d): one grouped ``F.conv2d`` per entry with the outer product of its two kernels, flipped: conv2d correlates."""
    ch = u.shape[1]
    R, g, g1, g2 = taps(sigma, u.dtype)
    out = []
    for kw, kh in ((g2, g), (g1, g1), (g, g2)):
        k = torch.outer(kh.flip(0), kw.flip(0))[None, None].repeat(ch, 1, 1, 1)
        out.append(sigma * sigma * F.conv2d(u, k, padding=R, groups=ch))
    return out


def measure(a, b, d, beta, c):
    m, h = (a + d) / 2, (a - d) / 2
    q = h * h + b * b
    pos = q > 0
    r = torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))
    kappa, mu = r - m, m + r
    ks = torch.where(kappa > 0, kappa, torch.ones_like(kappa))
    E1 = mu * mu / (2 * beta * beta * ks * ks)
    valid = (kappa > 0) & (E1 < E1_MAX)
    E1 = torch.where(valid, E1, torch.zeros_like(E1))
    E2 = (mu * mu + kappa * kappa) / (2 * c * c)
    return torch.where(valid, torch.exp(-E1) * -torch.expm1(-E2), torch.zeros_like(E1)), r


def response(x, sigmas=DEFAULT["sigmas"], weights=None, beta=0.5, c=0.1, value_range=(-1.0, 1.0), bright=True, **_):
    """(Rsp, the smallest r over the scales of positive weight) in x's dtype."""
    lo, hi = value_range
    u = (x - lo) / (hi - lo)
    w = weights or (1.0,) * len(sigmas)
    tot = sum(w)
    acc, rs = 0, []
    for sigma, wt in zip(sigmas, w):
        if wt > 0:
            a, b, d = hessian(u, sigma)
            if not bright:
                a, b, d = -a, -b, -d
            V, r = measure(a, b, d, beta, c)
            acc = acc + (wt / tot) * V
            rs.append(float(r.detach().min()))
    return acc, min(rs)


def restate(x, y, cfg=DEFAULT, per_image=False, x_grad=True, y_grad=True, dtype=torch.float64, upstream=None):
    """{"score", "rows", "A", "B", "dx", "dy", "min_r", "min_D"} in ``dtype``.  The score is the mean over n, or (N,) with ``per_image``; the
    gradients are those of ``(score * upstream).sum()`` (upstream 1 by default)."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(y_grad)
    A, ra = response(x, **cfg)
    B, rb = response(y, **cfg)
    D = (A * A).mean(dim=(1, 2, 3)) + (B * B).mean(dim=(1, 2, 3)) + cfg["eps"]
    rows = (2 * (A * B).mean(dim=(1, 2, 3)) + cfg["eps"]) / D
    score = rows if per_image else rows.mean()
    out = {"score": score.detach(), "rows": rows.detach(), "A": A.detach(), "B": B.detach(), "min_r": min(ra, rb), "min_D": float(D.detach().min())}
    if x_grad or y_grad:
        (score if upstream is None else score * upstream.to(dtype)).sum().backward()
    if x_grad:
        out["dx"] = x.grad
    if y_grad:
        out["dy"] = y.grad
    return out


def restate_map(x, cot, cfg=DEFAULT, dtype=torch.float64, x_grad=True):
    """{"map", "dx", "min_r"}: the filter alone and the gradient of ``(Rsp * cot).sum()``."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    A, r = response(x, **cfg)
    out = {"map": A.detach(), "min_r": r, "min_D": float("inf"), "rows": torch.ones(1)}
    if x_grad:
        (A * cot.to(dtype)).sum().backward()
        out["dx"] = x.grad
    return out


def restate_case(case, dtype=torch.float64):
    key = (case[0], dtype)
    if key not in _restated:
        _, _, cfg, per_image, y_grad, _, is_map = case
        x, y, cot = fixture_inputs(case)
        _restated[key] = restate_map(x, cot, cfg, dtype) if is_map else restate(x, y, cfg, per_image, True, y_grad, dtype)
    return _restated[key]


def well_conditioned(ref64):
    """The conditioning caps of every gradient comparison."""
    assert ref64["min_r"] >= MIN_R, ref64["min_r"]
    assert ref64["min_D"] >= MIN_D, ref64["min_D"]
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


def find_pair(shape, cfg=DEFAULT):
    """The pair of the first seed of range(2000) that meets the conditioning caps."""
    for seed in range(2000):
        x, y = make_pair(shape, seed)
        r = restate(x, y, cfg, per_image=True, x_grad=False, y_grad=False)
        if r["min_r"] >= MIN_R and r["min_D"] >= MIN_D and float(r["rows"].min()) > 0:
            return x, y
    raise AssertionError("no seed of range(2000) meets the conditioning caps for %s" % (shape,))


def line_image(inverted=False, lo=-1.0, hi=1.0):
    """32 x 32, background lo, a horizontal line of hi two pixels wide in rows 15 and 16."""
    img = torch.full((1, 1, 32, 32), lo)
    img[..., 15:17, :] = hi
    return (lo + hi) - img if inverted else img


def result_keys(case):
    return ("map", "dx") if case[6] else (("dx", "dy") if case[4] else ("dx",))


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_is_the_fixture(case):
    g = gold()
    cid = case[0]
    ref = restate_case(case)
    well_conditioned(ref)
    assert ref["min_r"] == pytest.approx(float(g[cid + "/min_r"]), rel=1e-9)
    if not case[6]:
        assert ref["min_D"] == pytest.approx(float(g[cid + "/min_D"]), rel=1e-9)
        assert ref["score"].shape == g[cid + "/score"].shape == ((case[1][0],) if case[3] else ())
        assert score_err(ref["score"], g[cid + "/score"]) <= 1e-12
        assert g[cid + "/f32/score"].dtype == np.float32 and score_err(g[cid + "/f32/score"], ref["score"]) <= 1e-5
    assert ((cid + "/dy") in g) == case[4] == ("dy" in ref)
    for k in result_keys(case):
        assert g["%s/%s" % (cid, k)].shape == case[1] and g["%s/%s" % (cid, k)].dtype == np.float64
        assert rel_l2(ref[k], g["%s/%s" % (cid, k)]) <= 1e-12, k
        # the fixture's fp32 run: only the error it defines
        assert g["%s/f32/%s" % (cid, k)].dtype == np.float32 and 0 < rel_l2(g["%s/f32/%s" % (cid, k)], ref[k]) <= 1e-5, k


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_in_fp32_is_the_fixture_at_fp32_tolerance(case):
    g = gold()
    cid = case[0]
    well_conditioned(restate_case(case))
    r32 = restate_case(case, torch.float32)
    assert r32["dx"].dtype == torch.float32
    if not case[6]:
        assert r32["score"].dtype == torch.float32 and score_err(r32["score"], g[cid + "/score"]) <= 1e-5
    for k in result_keys(case):
        assert rel_l2(r32[k], g["%s/%s" % (cid, k)]) <= 1e-5, k


def test_fixture_inputs_are_exact():
    g = gold()
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_gmsd.npz")) == 519779
    for case in CASES:
        if case[5] is None:
            x = g[case[0] + "/x"]
            assert x.dtype == np.float16 and x.shape == case[1] and len(np.unique(x)) > x.size // 2          # no flat regions
            assert ((case[0] + "/y") in g) == (not case[6])
            assert fixture_inputs(case)[0].dtype == torch.float32
        else:
            assert case[0] + "/x" not in g
            assert [c for c in CASES if c[0] == case[5]][0][1] == case[1]
        if case[6]:
            assert g[case[0] + "/cot"].dtype == np.float16 and g[case[0] + "/cot"].shape == case[1]


def test_seam_case_crosses_both_kernels_tiles():
    """(2, 1, 40, 136): two seams per axis of the 16 x 64 tile of ``vessel_index`` and of the 16 x 32 tile of ``vessel_grad``, a ragged last
    tile per axis, and a second plane behind the ragged tiles.  The halo case has a halo larger than the image."""
    tiles = kernel_tiles()
    assert tiles == ((16, 64), (16, 32))
    (_, (N, C, H, W), *_), = [c for c in CASES if c[0] == "seam"]
    assert N * C > 1
    for ty, tx in tiles:
        assert H // ty >= 2 and H % ty and W // tx >= 2 and W % tx, (H, W, ty, tx)
    (_, (_, _, H, W), cfg, *_), = [c for c in CASES if c[0] == "halo"]
    assert int(3 * max(cfg["sigmas"]) + 0.5) == 9 > max(H, W) and int(3 * min(cfg["sigmas"]) + 0.5) == 2


def test_symmetric():
    x, y = make_pair((2, 1, 21, 18), 6)
    a, b = restate(x, y, per_image=True), restate(y, x, per_image=True)
    assert score_err(a["score"], b["score"]) <= 1e-14
    assert rel_l2(a["dx"], b["dy"]) <= 1e-12 and rel_l2(a["dy"], b["dx"]) <= 1e-12


def test_identical_images_score_one():
    x, _ = make_pair((2, 1, 16, 24), 1)
    r = restate(x, x, per_image=True)
    assert float((r["rows"] - 1).abs().max()) <= 1e-15
    assert float(r["dx"].abs().max()) <= 1e-15 and float(r["dy"].abs().max()) <= 1e-15


def test_flat_images_score_one_with_zero_gradients():
    """Two vessel-free images: at value_range's lo the mapped image is 0, every Hessian entry 0, kappa == 0 and V exactly 0."""
    x, y = torch.full((2, 1, 12, 20), -1.0), torch.full((2, 1, 12, 20), -1.0)
    r = restate(x, y, per_image=True)
    assert float(r["A"].abs().max()) == 0.0 and r["rows"].tolist() == [1.0, 1.0]
    assert float(r["dx"].abs().max()) == 0.0 and float(r["dy"].abs().max()) == 0.0


def test_weight_zero_drops_the_scale():
    x, y = make_pair((1, 2, 21, 18), 3)
    a = restate(x, y, dict(DEFAULT, sigmas=(1.0, 2.0), weights=(1.0, 0.0)), per_image=True)
    b = restate(x, y, dict(DEFAULT, sigmas=(1.0,)), per_image=True)
    assert score_err(a["score"], b["score"]) == 0.0 and rel_l2(a["dx"], b["dx"]) == 0.0


def test_synthetic_line():
    """A bright line two pixels wide on a background at lo, c = 0.05: the response on the line is above 0.9, eight rows away it is exactly
    0 (the smoothed image is convex there: kappa <= 0 or E1 >= 87), the inverted image has none with bright=True and the same with
    bright=False.  The float64 prototype of the definition gave 0.9996, 0 and 2e-314."""
    cfg = dict(DEFAULT, c=0.05)
    A, _ = response(line_image().double(), **cfg)
    assert float(A[0, 0, 15, 16]) > 0.9 and float(A[0, 0, 16, 16]) > 0.9
    assert float(A[0, 0, 15 - 8, 16]) == 0.0 and float(A[0, 0, 16 + 8, 16]) == 0.0
    inv = line_image(inverted=True).double()
    assert float(response(inv, **cfg)[0][0, 0, 15, 16]) < 1e-6
    B, _ = response(inv, **dict(cfg, bright=False))
    assert float(B[0, 0, 15, 16]) > 0.9


@pytest.mark.parametrize("cfg", (DEFAULT, OTHER, DARK), ids=("default", "other", "dark"))
def test_restated_gradient_is_the_derivative(cfg):
    """Central differences in float64 along a random direction, (1, 2, 19, 23): odd sides."""
    x, y = find_pair((1, 2, 19, 23), cfg)
    ref = restate(x, y, cfg)
    well_conditioned(ref)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    h = 1e-6
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + h * v, y) if which == 0 else (x, y.double() + h * v)), cfg, x_grad=False, y_grad=False)
        dn = restate(*((x.double() - h * v, y) if which == 0 else (x, y.double() - h * v)), cfg, x_grad=False, y_grad=False)
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
    assert fa.Vesselness is fa.ssim.Vesselness and fa.VesselDice is fa.ssim.VesselDice and "Vesselness" in fa.__all__ and "VesselDice" in fa.__all__
    assert callable(fa.ops.vesselness) and callable(fa.ops.vessel_dice) and callable(fa.ssim.vessel_dice)
    assert fa.ops.VESSEL_SIGMAS == (1., 2., 3.) and fa.ops.VESSEL_MAX_SCALES == 3 and fa.ops.VESSEL_SIGMA_RANGE == (0.5, 3.0)
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    assert sorted(s for s in declared if "_vessel_" in s) == sorted(NEW_SYMBOLS)
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"vessel.hip"' in src
    assert os.path.exists(os.path.join(os.path.dirname(fa._lib.__file__), "csrc", "vessel.hip"))


def test_signatures(fa):
    empty = inspect.Parameter.empty
    common = [("sigmas", (1., 2., 3.)), ("weights", None), ("beta", 0.5), ("c", 0.1)]
    tail = [("value_range", (-1., 1.)), ("bright", True)]
    sig = inspect.signature(fa.ops.vesselness)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("x", empty)] + common + tail
    sig = inspect.signature(fa.ops.vessel_dice)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("a", empty), ("b", empty)] + common + [("eps", 1e-6)] + tail + [("per_image", False)]
    sig = inspect.signature(fa.ssim.vessel_dice)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("img1", empty), ("img2", empty)] + common + [("eps", 1e-6)] + tail + [
        ("size_average", True)]
    sig = inspect.signature(fa.Vesselness.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == common + tail
    sig = inspect.signature(fa.VesselDice.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == common + [("eps", 1e-6)] + tail + [("size_average", True)]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("vessel_weight", "vessel_sigmas", "vessel_c")] == [0.0, (1., 2., 3.), 0.1]
    names = list(sig.parameters)                     # keyword-only in practice; the tests of earlier terms pin the keywords from haarpsi_weight on
    at = names.index("mi_normalized")
    assert names[at + 1:at + 5] == ["vessel_weight", "vessel_sigmas", "vessel_c", "haarpsi_weight"]
    assert list(inspect.signature(fa.VesselDice.index).parameters)[1:] == ["img1", "img2", "per_image"]
    assert list(inspect.signature(fa.VesselDice.forward).parameters)[1:] == ["img1", "img2"]
    assert list(inspect.signature(fa.Vesselness.forward).parameters)[1:] == ["x"]


def test_module_attributes(fa):
    mod = fa.VesselDice()
    assert (mod.sigmas, mod.weights, mod.beta, mod.c, mod.eps, mod.value_range, mod.bright, mod.size_average) == (
        (1.0, 2.0, 3.0), None, 0.5, 0.1, 1e-6, (-1.0, 1.0), True, True)
    assert not list(mod.state_dict())
    mod = fa.VesselDice(sigmas=[1, 2], weights=[1, 3], beta=1, c=1, eps=0, value_range=(0, 255), bright=0, size_average=False)
    assert (mod.sigmas, mod.weights, mod.beta, mod.c, mod.eps, mod.value_range, mod.bright, mod.size_average) == (
        (1.0, 2.0), (1.0, 3.0), 1.0, 1.0, 0.0, (0.0, 255.0), False, False) and isinstance(mod.c, float)
    assert "sigmas=(1.0, 2.0)" in repr(mod) and "bright=False" in repr(mod)
    mod = fa.Vesselness(sigmas=(0.5,), c=0.05)
    assert (mod.sigmas, mod.weights, mod.beta, mod.c, mod.value_range, mod.bright) == ((0.5,), None, 0.5, 0.05, (-1.0, 1.0), True)
    assert not list(mod.state_dict()) and "c=0.05" in repr(mod)


def test_scalars_are_normalised_on_the_host(fa):
    """Weights are normalised to sum 1 and a scale of weight 0 is dropped before anything is launched."""
    f = fa.ops._vessel_check_scalars
    assert f((1, 2, 3), None, 0.5, 0.1, (-1, 1), 1e-6) == ((1.0, 2.0, 3.0), (1 / 3, 1 / 3, 1 / 3), 0.5, 0.1, 1e-6, -1.0, 1.0)
    assert f((0.5, 3), (1, 3), 0.5, 0.1, (-1, 1)) == ((0.5, 3.0), (0.25, 0.75), 0.5, 0.1, 0.0, -1.0, 1.0)
    assert f((1, 2), (1, 0), 0.5, 0.1, (-1, 1))[:2] == f((1,), None, 0.5, 0.1, (-1, 1))[:2] == ((1.0,), (1.0,))
    assert f((1, 2, 3), (0, 2, 0), 0.5, 0.1, (-1, 1))[:2] == ((2.0,), (1.0,))


def test_modules_pass_their_settings_on(fa, monkeypatch):
    seen = []
    monkeypatch.setattr(fa.ops, "vessel_dice", lambda *a: seen.append(("d",) + a[2:]) or "r")
    monkeypatch.setattr(fa.ops, "vesselness", lambda *a: seen.append(("v",) + a[1:]) or "m")
    x = torch.zeros(1, 1, 16, 16)
    assert fa.VesselDice(sigmas=(1, 2), weights=(1, 3), beta=0.7, c=0.05, eps=1e-5, value_range=(0, 2), bright=False)(x, x) == "r"
    assert fa.VesselDice(size_average=False).index(x, x, False) == "r"
    assert fa.VesselDice(size_average=False)(x, x) == "r"
    assert fa.ssim.vessel_dice(x, x, (2.,), None, 0.6, 0.2, 0.0, (0., 1.), False, False) == "r"
    assert fa.ssim.vessel_dice(x, x) == "r"
    assert fa.Vesselness(sigmas=(1.5,), beta=0.7, value_range=(0, 1), bright=False)(x) == "m"
    assert seen == [("d", (1.0, 2.0), (1.0, 3.0), 0.7, 0.05, 1e-5, (0.0, 2.0), False, False),
                    ("d", (1.0, 2.0, 3.0), None, 0.5, 0.1, 1e-6, (-1.0, 1.0), True, False),
                    ("d", (1.0, 2.0, 3.0), None, 0.5, 0.1, 1e-6, (-1.0, 1.0), True, True),
                    ("d", (2.,), None, 0.6, 0.2, 0.0, (0., 1.), False, True),
                    ("d", (1., 2., 3.), None, 0.5, 0.1, 1e-6, (-1., 1.), True, False),
                    ("v", (1.5,), None, 0.7, 0.1, (0.0, 1.0), False)]


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    x = torch.zeros(1, 1, 32, 32)
    dice, filt = fa.ops.vessel_dice, fa.ops.vesselness
    calls = ((lambda **kw: dice(x, x, **kw)), (lambda **kw: filt(x, **kw)), (lambda **kw: fa.VesselDice(**kw)), (lambda **kw: fa.Vesselness(**kw)))
    with pytest.raises(ValueError, match="device"):
        dice(x, x)
    with pytest.raises(ValueError, match="device"):
        filt(x)
    for f in calls:
        for name in ("beta", "c"):
            for bad in (0.0, -1e-5, float("nan"), float("inf")):
                with pytest.raises(ValueError, match="%s must be positive" % name):
                    f(**{name: bad})
            for bad in ("1e-5", None, True, torch.tensor(1e-5)):
                with pytest.raises(TypeError, match="%s must be a number" % name):
                    f(**{name: bad})
        for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0)):
            with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
                f(value_range=bad)
        for bad in (1.0, (1.0,), (0.0, 1.0, 2.0), None):
            with pytest.raises(TypeError, match="value_range must be a pair"):
                f(value_range=bad)
        for bad in (("0", "1"), (None, 1.0), (False, True)):
            with pytest.raises(TypeError, match="value_range's"):
                f(value_range=bad)
        # more than 3 scales, or none; a sigma outside [0.5, 3]
        for bad in ((), (1, 2, 3, 3)):
            with pytest.raises(ValueError, match=r"sigmas lists 1\.\.3 scales"):
                f(sigmas=bad)
        for bad in ((0.49,), (1.0, 3.01), (float("nan"),), (-1.0,)):
            with pytest.raises(ValueError, match=r"every sigma must lie in \[0\.5, 3\]"):
                f(sigmas=bad)
        for bad in (1.0, ("1",), (None,), (True,)):
            with pytest.raises(TypeError, match="sigma"):
                f(sigmas=bad)
        # the weights rule
        for bad in ((1, 1), (1, 1, 1, 1), ()):
            with pytest.raises(ValueError, match="one weight per scale"):
                f(weights=bad)
        for bad in ((-0.1, 1.0, 1.0), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)):
            with pytest.raises(ValueError, match="every weight must be finite and >= 0"):
                f(weights=bad)
        with pytest.raises(ValueError, match="must not all be zero"):
            f(weights=(0, 0, 0))
        for bad in (("1", "2", "3"), (None, 1, 1), (True, 1.0, 1.0), 1.0):
            with pytest.raises(TypeError, match="weight"):
                f(weights=bad)
    for f in (calls[0], calls[2]):
        for bad in (-1e-9, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="eps must be finite and >= 0"):
                f(eps=bad)
        with pytest.raises(TypeError, match="eps must be a number"):
            f(eps="0")
    # tensors: dtype, rank, shapes that differ, empty, the device check last
    with pytest.raises(TypeError, match="float32"):
        dice(x.double(), x.double())
    with pytest.raises(TypeError, match="float32"):
        dice(x, x.half())
    with pytest.raises(TypeError, match="float32"):
        filt(x.double())
    with pytest.raises(TypeError, match="tensor"):
        dice(x, x.numpy())
    with pytest.raises(TypeError, match="tensor"):
        filt([[1.0]])
    with pytest.raises(ValueError, match="same shape"):
        dice(x, torch.zeros(1, 1, 32, 16))
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        dice(x[0], x[0])
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        filt(x[0])
    for shape in ((0, 1, 32, 32), (1, 0, 32, 32), (1, 1, 0, 32), (1, 1, 32, 0)):
        with pytest.raises(ValueError, match="non-empty"):
            dice(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match="device"):                               # any sides >= 1
        dice(torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1))
    # scalar refusals come before tensor refusals
    with pytest.raises(ValueError, match="c must be positive"):
        dice(x.double(), x[0], c=0.0)
    with pytest.raises(ValueError, match="sigmas lists"):
        dice("no tensor", x, sigmas=())
    with pytest.raises(TypeError, match="float32"):
        dice(x.double(), x.double()[0])
    m = fa.VesselDice()
    with pytest.raises(ValueError, match="device"):
        m(x, x)
    with pytest.raises(ValueError, match="device"):
        m.index(x, x, True)
    with pytest.raises(ValueError, match="device"):
        fa.Vesselness()(x)
    with pytest.raises(ValueError, match="device"):
        fa.ssim.vessel_dice(x, x)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.VesselDice

    def make(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "VesselDice", make)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.vessel_weight == 0.0 and ts.vessel is None and not built
    ts = fa.TrainStep(*nets, device="cpu", vessel_sigmas=(1.0,), vessel_c=0.05)
    assert ts.vessel is None and not built
    ts = fa.TrainStep(*nets, device="cpu", vessel_weight=0.25, vessel_sigmas=(1.0, 2.0), vessel_c=0.05)
    assert built == [dict(sigmas=(1.0, 2.0), c=0.05)]
    assert ts.vessel_weight == 0.25 and (ts.vessel.sigmas, ts.vessel.c, ts.vessel.value_range, ts.vessel.size_average) == ((1.0, 2.0), 0.05, (-1.0, 1.0), True)
    assert ts.gmsd is None and ts.haarpsi is None and ts.lncc is None and ts.mi is None
    with pytest.raises(ValueError, match="c must be positive"):
        fa.TrainStep(*nets, device="cpu", vessel_weight=0.25, vessel_c=0.0)
    with pytest.raises(ValueError, match="every sigma must lie"):
        fa.TrainStep(*nets, device="cpu", vessel_weight=0.25, vessel_sigmas=(4.0,))
    for bad in (-1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="vessel_weight must be a finite number >= 0"):
            fa.TrainStep(*nets, device="cpu", vessel_weight=bad)


def test_train_step_adds_the_term_where_loss_gmsd_is_added(fa):
    """``_extension_terms`` (one half per chain of the two-chain schedule, which ``GraphedTrainStep`` captures) names ``loss_vessel``; with
    the module replaced by a stub no kernel runs (the single-stream ``generator_loss``: tests/test_train_terms_cpu.py)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu", vessel_weight=0.5)
    ts.vessel = lambda rec, real: (rec * real).mean()
    rec, real = torch.full((1, 1, 4, 4), 0.5), torch.full((1, 1, 4, 4), 0.5)
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_vessel"] and float(t["loss_vessel"]) == 0.5 * (1 - 0.25)
    assert fa.TrainStep(*nets, device="cpu")._extension_terms(rec, real) == {}
    assert not hasattr(fa.GraphedTrainStep, "generator_loss")              # it captures the TrainStep's own terms
