"""Local normalised cross-correlation without a GPU: a plain-torch restatement of

    Sa = box(a)  Sb = box(b)  Saa = box(a a)  Sbb = box(b b)  Sab = box(a b),  box = a grouped ``F.conv2d`` with a win x win kernel of
    ones and zero padding win // 2 (samples beyond the image 0, the divisor always n = win^2),
    u = Sab - Sa Sb / n,  va = Saa - Sa Sa / n,  vb = Sbb - Sb Sb / n,  cc_p = u^2 / (va vb + eps),
    LNCC[n] = the mean of cc_p over c, y, x;  the score is their mean over n, or (N,) per image,

gradients by autograd; pinned to tests/golden/golden_lncc.npz, whose values come from explicit slice sums (tools/gen_golden_lncc.py;
there also checked against central differences), and the host logic of ``ops.lncc``, ``ssim.LNCC``, ``ssim.lncc`` and
``TrainStep(lncc_weight=...)`` (everything that raises before an entry point is reached).

Bounds.  Restatement against the fixture's float64 values: 1e-12 relative (scores: absolute difference over |score|; arrays: relative
L2): both sides are float64 sums of at most 225 terms per window and a few thousand positions, in different orders.  The restatement in
fp32 against the fixture's float64 values: 1e-5 relative.  The fixture's own fp32 run shows gradient errors of 5e-7 .. 1e-6 and score
errors of at most 3e-7 under the conditioning cap below, which bounds the amplification of a rounding error of 2^-24 by 16; the
restatement sums the same terms in another order, and 1e-5 leaves a factor of ten over that.

The conditioning cap.  ``va = Saa - Sa^2 / n`` cancels and rounding is amplified by ``Saa / va``.  Every gradient comparison therefore
first asserts on the float64 restatement that ``min_p min(va / Saa, vb / Sbb) >= 2^-4``; nothing is excluded from a comparison.  Inputs:
x = 2 x the 5 x 5-box-smoothed (replicate-padded) N(0, 1) noise, y = -0.6 x + 0.2 + 0.6 x smoothed noise + 0.05 noise, rounded to values
float16 holds exactly (the fixture keeps them in two bytes); off the fixture ``find_pair`` takes the first seed of range(2000) that
meets the cap and fails if none does.  Win 3 meets it only on very small images, which is why it appears at (1, 1, 5, 7) alone.

The seam cases.  ``kernel_tiles()`` reads the tiles out of csrc/lncc.hip: ``lncc_index`` 16 x 32 (rows x columns), ``lncc_grad`` 16 x 16.
(2, 1, 20, 36) at win 9 has one full tile and a ragged remainder of 4 per axis for both kernels (and two 16-column tiles of the
gradient kernel), with a second plane behind the ragged tiles; (1, 1, 36, 40) at win 15 has two tile rows and a remainder, so that the
gradient's halo of 14 on either side crosses a seam from every tile."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_lncc.npz")
CAP = 2.0 ** -4
#: (case, shape, win, eps, per image, y needs a gradient, the case whose inputs it shares): the table of tools/gen_golden_lncc.py
CASES = (("win3", (1, 1, 5, 7), 3, 1e-5, False, True, None),
         ("win15_small", (1, 1, 5, 7), 15, 1e-5, False, True, None),
         ("mean", (2, 1, 16, 16), 9, 1e-5, False, True, None),
         ("xonly", (2, 1, 16, 16), 9, 1e-5, False, False, "mean"),
         ("per_image_cfg", (2, 2, 32, 48), 7, 1e-3, True, True, None),
         ("channels", (1, 3, 16, 24), 9, 1e-5, False, True, None),
         ("odd", (1, 1, 37, 53), 9, 1e-5, False, True, None),
         ("seam9", (2, 1, 20, 36), 9, 1e-5, False, True, None),
         ("seam15", (1, 1, 36, 40), 15, 1e-5, False, True, None))
NEW_SYMBOLS = ("faoctasr_lncc_workspace_floats", "faoctasr_lncc_index", "faoctasr_lncc_final", "faoctasr_lncc_grad")
_gold = {}
_restated = {}


def gold():
    """The fixture, with the fp32 run's gradients put back together: ``float32(dx) + dx_delta`` (exact, tools/gen_golden_lncc.py)."""
    if not _gold:
        with np.load(GOLDEN) as z:
            _gold.update({k: z[k] for k in z.files})
        for k in [k for k in _gold if k.endswith("_delta")]:
            case, _, name = k.split("/")
            _gold["%s/f32/%s" % (case, name[:-6])] = _gold["%s/%s" % (case, name[:-6])].astype(np.float32) + _gold[k]
    return _gold


def kernel_tiles():
    """((LF_TY, LF_TX), (LB_T, LB_T)): the tiles of ``lncc_index`` and ``lncc_grad``, read out of csrc/lncc.hip."""
    import faoctasr
    with open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "csrc", "lncc.hip")) as f:
        src = f.read()
    v = {name: int(re.search(r"constexpr int [^;]*\b%s = (\d+)\b" % name, src).group(1)) for name in ("LF_TY", "LF_TX", "LB_T")}
    return (v["LF_TY"], v["LF_TX"]), (v["LB_T"], v["LB_T"])


def case_name(case):
    return case[0]


def fixture_inputs(case):
    g = gold()
    src = case[6] or case[0]
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
def box(t, win):
    ch = t.shape[1]
    return F.conv2d(t, torch.ones(ch, 1, win, win, dtype=t.dtype), padding=win // 2, groups=ch)


def restate(x, y, win=9, eps=1e-5, per_image=False, x_grad=True, y_grad=True, dtype=torch.float64, upstream=None):
    """{"score", "dx", "dy", "cap"} in ``dtype``: the score is the mean over n, or (N,) with ``per_image``; the gradients are those of
    ``(score * upstream).sum()`` (upstream 1 by default); ``cap`` is ``min_p min(va / Saa, vb / Sbb)``."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(y_grad)
    n = float(win * win)
    Sa, Sb, Saa, Sbb, Sab = box(x, win), box(y, win), box(x * x, win), box(y * y, win), box(x * y, win)
    u, va, vb = Sab - Sa * Sb / n, Saa - Sa * Sa / n, Sbb - Sb * Sb / n
    rows = (u * u / (va * vb + eps)).mean(dim=(1, 2, 3))
    score = rows if per_image else rows.mean()
    out = {"score": score.detach(), "cap": min(float((va / Saa).detach().min()), float((vb / Sbb).detach().min()))}
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
        _, _, win, eps, per_image, y_grad, _ = case
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, win, eps, per_image, True, y_grad, dtype)
    return _restated[key]


def well_conditioned(ref64):
    """The conditioning cap of every gradient comparison."""
    assert ref64["cap"] >= CAP, ref64["cap"]


def smooth(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed):
    """x = 2 x the 5 x 5-box-smoothed N(0, 1) noise, y = -0.6 x + 0.2 + 0.6 x smoothed noise + 0.05 noise, both exact in float16."""
    g = torch.Generator().manual_seed(seed)
    n1, n2, n3 = (torch.randn(*shape, generator=g, dtype=torch.float32) for _ in range(3))
    x = 2.0 * smooth(n1)
    y = -0.6 * x + 0.2 + 0.6 * smooth(n2) + 0.05 * n3
    return x.half().float(), y.half().float()


def find_pair(shape, win=9, eps=1e-5):
    """The pair of the first seed of range(2000) that meets the conditioning cap."""
    for seed in range(2000):
        x, y = make_pair(shape, seed)
        if restate(x, y, win, eps, x_grad=False, y_grad=False)["cap"] >= CAP:
            return x, y
    raise AssertionError("no seed of range(2000) meets the conditioning cap for %s, win %d" % (shape, win))


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_is_the_fixture(case):
    g = gold()
    cid, y_grad = case[0], case[5]
    ref = restate_case(case)
    well_conditioned(ref)
    assert ref["cap"] == pytest.approx(float(g[cid + "/cap"]), rel=1e-9)
    assert ref["score"].shape == g[cid + "/score"].shape == ((case[1][0],) if case[4] else ())
    assert score_err(ref["score"], g[cid + "/score"]) <= 1e-12
    assert rel_l2(ref["dx"], g[cid + "/dx"]) <= 1e-12
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
    r32 = restate_case(case, torch.float32)
    assert r32["score"].dtype == torch.float32 and r32["dx"].dtype == torch.float32
    assert score_err(r32["score"], g[cid + "/score"]) <= 1e-5
    for k in ("dx", "dy") if case[5] else ("dx",):
        assert rel_l2(r32[k], g["%s/%s" % (cid, k)]) <= 1e-5


def test_fixture_is_small_and_its_inputs_are_exact():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_haarpsi.npz"))
    g = gold()
    for case in CASES:
        if case[6] is None:
            x = g[case[0] + "/x"]
            assert x.dtype == np.float16 and g[case[0] + "/y"].dtype == np.float16 and x.shape == case[1]
            assert len(np.unique(x)) > x.size // 2                        # no flat regions
            fx, fy = fixture_inputs(case)
            assert fx.dtype == torch.float32 and fy.dtype == torch.float32
        else:
            assert case[0] + "/x" not in g


def test_seam_cases_cross_the_kernels_tiles():
    """The fixture's seam cases have at least one full tile and a ragged remainder per axis for both kernels, with the tiles as
    csrc/lncc.hip has them; the win-9 case has a second plane that starts behind a ragged tile, the win-15 case two tile rows."""
    tiles = kernel_tiles()
    assert all(t > 0 for pair in tiles for t in pair)
    for name in ("seam9", "seam15"):
        (_, (N, C, H, W), *_), = [c for c in CASES if c[0] == name]
        for ty, tx in tiles:
            assert H // ty >= 1 and H % ty and W // tx >= 1 and W % tx, (name, H, W, ty, tx)
    assert [c for c in CASES if c[0] == "seam9"][0][1][0] > 1
    assert [c for c in CASES if c[0] == "seam15"][0][1][2] // max(ty for ty, _ in tiles) >= 2


def test_the_window_may_be_larger_than_the_image():
    """(1, 1, 5, 7) at win 15: every window holds the whole image, so every position has the same five sums."""
    (case,) = [c for c in CASES if c[0] == "win15_small"]
    x, y = fixture_inputs(case)
    xd, yd = x.double(), y.double()
    n = 225.0
    u = (xd * yd).sum() - xd.sum() * yd.sum() / n
    va, vb = (xd * xd).sum() - xd.sum() ** 2 / n, (yd * yd).sum() - yd.sum() ** 2 / n
    assert abs(float(u * u / (va * vb + 1e-5)) - float(restate_case(case)["score"])) <= 1e-12


def test_symmetric_and_affine_invariant():
    x, y = make_pair((2, 1, 21, 18), 6)
    a, b = restate(x, y, per_image=True), restate(y, x, per_image=True)
    assert score_err(a["score"], b["score"]) <= 1e-14
    assert rel_l2(a["dx"], b["dy"]) <= 1e-12 and rel_l2(a["dy"], b["dx"]) <= 1e-12
    # an affine map of one image changes nothing where the window lies inside the image (the zero padding is not mapped)
    win, r = 5, 2
    xd, yd = x.double(), y.double()

    def inner(p, q):
        n = float(win * win)
        Sa, Sb, Saa, Sbb, Sab = box(p, win), box(q, win), box(p * p, win), box(q * q, win), box(p * q, win)
        u, va, vb = Sab - Sa * Sb / n, Saa - Sa * Sa / n, Sbb - Sb * Sb / n
        return (u * u / (va * vb + 1e-12))[..., r:-r, r:-r]
    assert float((inner(xd, yd) - inner(xd, -3.0 * yd + 0.7)).abs().max()) <= 1e-8
    assert float((inner(xd, xd) - 1).abs().max()) <= 1e-8


def test_restated_gradient_is_the_derivative():
    """Central differences in float64 along a random direction, (1, 2, 19, 23): odd sides."""
    x, y = find_pair((1, 2, 19, 23))
    ref = restate(x, y)
    well_conditioned(ref)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    h = 1e-6
    for which, key in ((0, "dx"), (1, "dy")):
        up = restate(*((x.double() + h * v, y) if which == 0 else (x, y.double() + h * v)), x_grad=False, y_grad=False)
        dn = restate(*((x.double() - h * v, y) if which == 0 else (x, y.double() - h * v)), x_grad=False, y_grad=False)
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
    assert fa.LNCC is fa.ssim.LNCC and "LNCC" in fa.__all__
    assert callable(fa.ops.lncc) and callable(fa.ssim.lncc) and fa.ops.LNCC_MAX_WIN == 15
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    src = open(os.path.join(os.path.dirname(fa._lib.__file__), "build.py")).read()
    assert '"lncc.hip"' in src
    assert os.path.exists(os.path.join(os.path.dirname(fa._lib.__file__), "csrc", "lncc.hip"))


def test_signatures(fa):
    empty = inspect.Parameter.empty
    sig = inspect.signature(fa.ops.lncc)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("a", empty), ("b", empty), ("win", 9), ("eps", 1e-5), ("per_image", False)]
    sig = inspect.signature(fa.LNCC.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("win", 9), ("eps", 1e-5), ("size_average", True)]
    sig = inspect.signature(fa.ssim.lncc)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("img1", empty), ("img2", empty), ("win", 9), ("eps", 1e-5), ("size_average", True)]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("lncc_weight", "lncc_win", "lncc_eps")] == [0.0, 9, 1e-5]
    assert list(sig.parameters)[-3:] == ["lncc_weight", "lncc_win", "lncc_eps"]          # behind the existing keywords
    assert list(inspect.signature(fa.LNCC.index).parameters)[1:] == ["img1", "img2", "per_image"]
    assert list(inspect.signature(fa.LNCC.forward).parameters)[1:] == ["img1", "img2"]


def test_module_attributes(fa):
    mod = fa.LNCC()
    assert (mod.win, mod.eps, mod.size_average) == (9, 1e-5, True)
    assert not list(mod.state_dict())
    mod = fa.LNCC(win=5, eps=1, size_average=False)
    assert (mod.win, mod.eps, mod.size_average) == (5, 1.0, False) and isinstance(mod.eps, float)
    assert "win=5" in repr(mod)


def test_module_passes_its_settings_on(fa, monkeypatch):
    seen = []
    monkeypatch.setattr(fa.ops, "lncc", lambda *a: seen.append(a[2:]) or "r")
    x = torch.zeros(1, 1, 16, 16)
    assert fa.LNCC(win=7, eps=1e-3)(x, x) == "r"
    assert fa.LNCC(size_average=False).index(x, x, False) == "r"
    assert fa.LNCC(size_average=False)(x, x) == "r"
    assert fa.ssim.lncc(x, x, 5, 1e-4, False) == "r"
    assert seen == [(7, 1e-3, False), (9, 1e-5, False), (9, 1e-5, True), (5, 1e-4, True)]


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    f = fa.ops.lncc
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="device"):
        f(x, x)
    with pytest.raises(ValueError, match="device"):
        f(torch.zeros(2, 3, 1, 1), torch.zeros(2, 3, 1, 1), win=15)         # the window may be larger than the image
    for bad in (1, 2, 4, 8, 17, 0, -3):
        with pytest.raises(ValueError, match="win must be odd in 3..15"):
            f(x, x, win=bad)
        with pytest.raises(ValueError, match="win must be odd in 3..15"):
            fa.LNCC(win=bad)
    for bad in (9.0, "9", None, True, torch.tensor(9)):
        with pytest.raises(TypeError, match="win must be an integer"):
            f(x, x, win=bad)
        with pytest.raises(TypeError, match="win must be an integer"):
            fa.LNCC(win=bad)
    for bad in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps must be positive"):
            f(x, x, eps=bad)
        with pytest.raises(ValueError, match="eps must be positive"):
            fa.LNCC(eps=bad)
    for bad in ("1e-5", None, True, torch.tensor(1e-5)):
        with pytest.raises(TypeError, match="eps must be a number"):
            f(x, x, eps=bad)
        with pytest.raises(TypeError, match="eps must be a number"):
            fa.LNCC(eps=bad)
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
    with pytest.raises(ValueError, match="win must be odd"):
        f(x.double(), x[0], win=4)
    with pytest.raises(ValueError, match="eps must be positive"):
        f("no tensor", x, eps=0.0)
    with pytest.raises(TypeError, match="float32"):
        f(x.double(), x.double()[0])
    with pytest.raises(ValueError, match="same shape"):
        f(x, torch.zeros(1, 1, 8, 8))
    mod = fa.LNCC()
    with pytest.raises(ValueError, match="device"):
        mod(x, x)
    with pytest.raises(ValueError, match="device"):
        mod.index(x, x, True)
    with pytest.raises(ValueError, match="device"):
        fa.ssim.lncc(x, x)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.LNCC

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "LNCC", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.lncc_weight == 0.0 and ts.lncc is None and not built
    ts = fa.TrainStep(*nets, device="cpu", lncc_weight=0.25, lncc_win=7, lncc_eps=1e-3)
    assert built == [dict(win=7, eps=1e-3)]
    assert ts.lncc_weight == 0.25 and (ts.lncc.win, ts.lncc.eps, ts.lncc.size_average) == (7, 1e-3, True)
    assert ts.msssim is None and ts.haarpsi is None and ts.ffl is None and ts.mi is None
    with pytest.raises(ValueError, match="win must be odd"):
        fa.TrainStep(*nets, device="cpu", lncc_weight=0.25, lncc_win=8)
    for bad in (-1.0, float("nan"), float("inf"), "1", None):               # validated as mi_weight is
        with pytest.raises(ValueError, match="lncc_weight must be a finite number >= 0"):
            fa.TrainStep(*nets, device="cpu", lncc_weight=bad)
