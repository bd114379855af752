"""The pixel-domain visual information fidelity (csrc/vif.hip) without a GPU: the float64 restatement of the definition on grouped
``F.conv2d`` against tests/golden/golden_vif.npz, whose values come from explicit shifted-slice sums (tools/gen_golden_vif.py); the
conditioning caps; the fixture's layout; the seam case against the kernels' tiles; and the host logic of ``ops.vif``, ``ssim.VIF``,
``ssim.vif`` and ``TrainStep(vif_weight=..., vif_sigma_n_sq=...)`` -- signatures, refusals, plumbing -- none of which reaches an entry point.

The definition.  x is the image under test, r the reference, (N, C, H, W), H, W >= 41:

    u = (t - lo) * 255 / (hi - lo); EPS = 1e-8; scale s = 0..3: K_s = 2^(4-s) + 1, w_s[k] = exp(-(k - (K_s-1)/2)^2 / (2 (K_s/5)^2)) / sum
    s > 0: x_s = (W_s * x_{s-1})[::2, ::2], r_s likewise (valid convolution, the new scale's window)
    mx = W_s*x_s, mr = W_s*r_s, sxx = relu(W_s*(x_s x_s) - mx^2), srr = relu(W_s*(r_s r_s) - mr^2), sxr = W_s*(x_s r_s) - mx mr
    g = sxr / (srr + EPS), sv = sxx - g sxr; srr < EPS: g = 0, sv = sxx, srr = 0; sxx < EPS: g = 0, sv = 0; g < 0: sv = sxx, g = 0; sv <= EPS: sv = EPS
    V[n] = (sum_s sum log10(1 + g^2 srr / (sv + sigma_n_sq)) + EPS) / (sum_s sum log10(1 + srr / sigma_n_sq) + EPS)

The conditioning caps, asserted on the float64 restatement over all scales and positions before every gradient comparison:
min sxx >= 1, min srr >= 1, min g >= 0.5, min sv >= 2^-8: no clamp is anywhere near."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vif.npz")
EPS = 1e-8
CAPS = dict(min_sxx=1.0, min_srr=1.0, min_g=0.5, min_sv=2.0 ** -8)
DEFAULT = dict(sigma_n_sq=2.0, value_range=(-1.0, 1.0))
OTHER = dict(sigma_n_sq=0.4, value_range=(0.0, 2.0))
#: (case, shape, settings, per image, r needs a gradient, the case whose inputs it shares or None): tools/gen_golden_vif.py
CASES = (("min41", (1, 1, 41, 41), DEFAULT, False, True, None),
         ("mean", (2, 1, 48, 56), DEFAULT, False, True, None),
         ("xonly", (2, 1, 48, 56), DEFAULT, False, False, "mean"),
         ("per_image_cfg", (2, 2, 48, 72), OTHER, True, True, None),
         ("channels", (1, 3, 57, 73), DEFAULT, False, True, None),
         ("seam", (1, 1, 72, 200), DEFAULT, False, True, None))
NEW_SYMBOLS = ("faoctasr_vif_workspace_floats", "faoctasr_vif_scale_fwd", "faoctasr_vif_final", "faoctasr_vif_scale_bwd")
_gold = {}
_restated = {}


@pytest.fixture(autouse=True)
def _the_op_exists():
    """The restatement below stands for ``ops.vif``: without the op none of these tests says anything."""
    import faoctasr
    assert callable(getattr(faoctasr.ops, "vif", None)) and hasattr(faoctasr, "VIF")


def unplanes(p, dtype):
    """The inverse of ``planes`` of tools/gen_golden_vif.py: uint8 (itemsize,) + shape -> shape of ``dtype``."""
    return np.ascontiguousarray(np.moveaxis(p, 0, -1)).view(np.dtype(dtype)).reshape(p.shape[1:])


def gold():
    """The fixture, its byte planes put back together, the fp32 run's gradients rebuilt from their bit-pattern distances (exact,
    tools/gen_golden_vif.py) and the gradients of a case that shares another's inputs taken from that case."""
    if not _gold:
        with np.load(GOLDEN) as z:
            for k in z.files:
                if "#" in k:
                    name, dtype = k.split("#")
                    _gold[name] = unplanes(z[k], dtype)
                else:
                    _gold[k] = z[k]
        for k in [k for k in _gold if k.endswith("_delta")]:
            case, _, name = k.split("/")
            near = np.ascontiguousarray(_gold["%s/%s" % (case, name[:-6])].astype(np.float32))
            _gold["%s/f32/%s" % (case, name[:-6])] = (near.view(np.int32) + _gold[k]).view(np.float32)
        for case in CASES:
            if case[5] is not None:
                for k in ("dx", "f32/dx"):
                    _gold["%s/%s" % (case[0], k)] = _gold["%s/%s" % (case[5], k)]
    return _gold


def kernel_tiles():
    """((VI_TY, VI_TX), (VJ_TY, VJ_TX)): the tiles of ``vif_scale_fwd`` and ``vif_scale_bwd``, read out of csrc/vif.hip."""
    import faoctasr
    with open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "csrc", "vif.hip")) as f:
        src = f.read()
    v = {name: int(re.search(r"constexpr int [^;]*\b%s = (\d+)\b" % name, src).group(1)) for name in ("VI_TY", "VI_TX", "VJ_TY", "VJ_TX")}
    return (v["VI_TY"], v["VI_TX"]), (v["VJ_TY"], v["VJ_TX"])


def case_name(case):
    return case[0]


def fixture_inputs(case):
    """(x, r) as float32."""
    g = gold()
    src = case[5] or case[0]
    return torch.from_numpy(g[src + "/x"].astype(np.float32)), torch.from_numpy(g[src + "/r"].astype(np.float32))


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
def window(s, dtype):
    K = 2 ** (4 - s) + 1
    k = torch.arange(K, dtype=torch.float64)
    w = torch.exp(-((k - (K - 1) / 2.0) ** 2) / (2.0 * (K / 5.0) ** 2))
    return (w / w.sum()).to(dtype)


def filt(u, w):
    """The separable valid convolution as two grouped ``F.conv2d`` (the window is even: correlation is convolution)."""
    ch, K = u.shape[1], w.numel()
    u = F.conv2d(u, w.reshape(1, 1, 1, K).repeat(ch, 1, 1, 1), groups=ch)
    return F.conv2d(u, w.reshape(1, 1, K, 1).repeat(ch, 1, 1, 1), groups=ch)


def vif_rows(x, r, sigma_n_sq=2.0, value_range=(-1.0, 1.0)):
    """((N,) scores, the minima of sxx, srr, g, sv over all scales and positions before any branch) in the dtype of x."""
    lo, hi = value_range
    x, r = (x - lo) * 255.0 / (hi - lo), (r - lo) * 255.0 / (hi - lo)
    num = den = 0
    mins = dict(min_sxx=float("inf"), min_srr=float("inf"), min_g=float("inf"), min_sv=float("inf"), max_g=-float("inf"))
    for s in range(4):
        w = window(s, x.dtype)
        if s > 0:
            x, r = filt(x, w)[..., ::2, ::2], filt(r, w)[..., ::2, ::2]
        mx, mr = filt(x, w), filt(r, w)
        sxx = torch.relu(filt(x * x, w) - mx * mx)
        srr = torch.relu(filt(r * r, w) - mr * mr)
        sxr = filt(x * r, w) - mx * mr
        g = sxr / (srr + EPS)
        sv = sxx - g * sxr
        for k, v in (("min_sxx", sxx), ("min_srr", srr), ("min_g", g), ("min_sv", sv)):
            mins[k] = min(mins[k], float(v.detach().min()))
        mins["max_g"] = max(mins["max_g"], float(g.detach().max()))
        zero = torch.zeros_like(g)
        m = srr < EPS
        g, sv, srr = torch.where(m, zero, g), torch.where(m, sxx, sv), torch.where(m, zero, srr)
        m = sxx < EPS
        g, sv = torch.where(m, zero, g), torch.where(m, zero, sv)
        m = g < 0
        sv, g = torch.where(m, sxx, sv), torch.where(m, zero, g)
        sv = torch.where(sv <= EPS, torch.full_like(sv, EPS), sv)
        num = num + torch.log10(1 + g * g * srr / (sv + sigma_n_sq)).sum(dim=(1, 2, 3))
        den = den + torch.log10(1 + srr / sigma_n_sq).sum(dim=(1, 2, 3))
    return (num + EPS) / (den + EPS), mins


def restate(x, r, cfg=DEFAULT, per_image=False, x_grad=True, r_grad=True, dtype=torch.float64, upstream=None):
    """{"score", "dx", "dr", the minima}: the gradients are those of ``(score * upstream).sum()``."""
    x = x.to(dtype).clone().requires_grad_(x_grad)
    r = r.to(dtype).clone().requires_grad_(r_grad)
    rows, mins = vif_rows(x, r, cfg["sigma_n_sq"], cfg["value_range"])
    score = rows if per_image else rows.mean()
    out = dict(mins, score=score.detach())
    if x_grad or r_grad:
        (score if upstream is None else score * upstream.to(dtype)).sum().backward()
    if x_grad:
        out["dx"] = x.grad
    if r_grad:
        out["dr"] = r.grad
    return out


def restate_case(case, dtype=torch.float64):
    key = (case[0], dtype)
    if key not in _restated:
        x, r = fixture_inputs(case)
        _restated[key] = restate(x, r, case[2], case[3], True, case[4], dtype)
    return _restated[key]


def well_conditioned(ref64):
    """The conditioning caps."""
    for k, cap in CAPS.items():
        assert ref64[k] >= cap, (k, ref64[k], cap)


def smooth(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed):
    """(x, r) as the fixture makes them: r = 2 x smoothed noise, x = r + 0.1 noise, values float16 holds."""
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.randn(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    r = 2.0 * smooth(n1)
    x = r + 0.1 * n2
    return x.half().float(), r.half().float()


def find_pair(shape, cfg=DEFAULT):
    """The first seed's pair that meets the conditioning caps."""
    for seed in range(100):
        x, r = make_pair(shape, seed)
        with torch.no_grad():
            mins = vif_rows(x.double(), r.double(), cfg["sigma_n_sq"], cfg["value_range"])[1]
        if all(mins[k] >= cap for k, cap in CAPS.items()):
            return x, r
    raise AssertionError("no seed of range(100) meets the caps for %s" % (shape,))


def result_keys(case):
    return ("dx", "dr") if case[4] else ("dx",)


# ------------------------------------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_is_the_fixture(case):
    g = gold()
    cid = case[0]
    ref = restate_case(case)
    well_conditioned(ref)
    for k in CAPS:
        assert ref[k] == pytest.approx(float(g["%s/%s" % (cid, k)]), rel=1e-9)
    assert ref["score"].shape == g[cid + "/score"].shape == ((case[1][0],) if case[3] else ())
    assert g[cid + "/score"].dtype == np.float64 and score_err(ref["score"], g[cid + "/score"]) <= 1e-12
    assert g[cid + "/f32/score"].dtype == np.float32 and score_err(g[cid + "/f32/score"], ref["score"]) <= 1e-4
    assert ("dr" in ref) == case[4]
    for k in result_keys(case):
        assert g["%s/%s" % (cid, k)].shape == case[1] and g["%s/%s" % (cid, k)].dtype == np.float64
        assert rel_l2(ref[k], g["%s/%s" % (cid, k)]) <= 1e-12, k
        # the fixture's fp32 run: only the error it defines (the variances are differences of sums of order 255^2 / 3)
        assert g["%s/f32/%s" % (cid, k)].dtype == np.float32 and 0 < rel_l2(g["%s/f32/%s" % (cid, k)], ref[k]) <= 1e-3, k


def test_fixture_layout_and_size():
    g = gold()
    assert os.path.getsize(GOLDEN) < 1 << 20
    for case in CASES:
        if case[5] is None:
            for k in ("x", "r"):
                a = g["%s/%s" % (case[0], k)]
                assert a.dtype == np.float16 and a.shape == case[1] and len(np.unique(a)) > a.size // 8
            assert fixture_inputs(case)[0].dtype == torch.float32
            x, r = make_pair(case[1], 0)             # the family's inputs, seed 0
            assert torch.equal(x, fixture_inputs(case)[0]) and torch.equal(r, fixture_inputs(case)[1])
        else:
            assert case[0] + "/x" not in g
            assert [c for c in CASES if c[0] == case[5]][0][1] == case[1]


def test_cases_cover_what_they_are_for():
    """(1,1,41,41): the minimum, every filtered side odd, one position at the last scale.  (1,1,72,200): the stat maps of scales 0 and 1
    cross the seams of both kernels' tiles on both axes."""
    import faoctasr
    assert faoctasr.ops.vif_sides(41) == [41, 17, 7, 3] and faoctasr.ops.VIF_MIN_SIDE == 41
    sides, K = faoctasr.ops.vif_sides(41), [17, 9, 5, 3]
    assert sides[3] - K[3] + 1 == 1
    assert all((sides[s] - K[s + 1] + 1) % 2 == 1 for s in range(3))
    tiles = kernel_tiles()
    assert tiles == ((16, 64), (16, 32))
    (_, (_, _, H, W), *_), = [c for c in CASES if c[0] == "seam"]
    hs, ws = faoctasr.ops.vif_sides(H), faoctasr.ops.vif_sides(W)
    assert [(hs[s] - K[s] + 1, ws[s] - K[s] + 1) for s in (0, 1)] == [(56, 184), (24, 88)]
    for s in (0, 1):
        for ty, tx in tiles:
            sh, sw = hs[s] - K[s] + 1, ws[s] - K[s] + 1
            assert sh > ty and sh % ty and sw > tx and sw % tx, (s, sh, sw, ty, tx)
    # the decimated map is larger than half the stat map: the forward's grid covers the filtered map
    assert hs[0] - K[1] + 1 > hs[0] - K[0] + 1 and faoctasr.ops.vif_sides(41)[1] == 17 > (25 + 1) // 2


def test_windows():
    import faoctasr
    for s, K in enumerate((17, 9, 5, 3)):
        w = faoctasr.ops.vif_window(s)
        assert len(w) == K and abs(math.fsum(w) - 1) < 1e-15 and w == w[::-1]
        assert torch.allclose(torch.tensor(w, dtype=torch.float64), window(s, torch.float64), rtol=1e-14, atol=0)


def test_asymmetric_and_identical():
    """V(x, r) is not V(r, x); V(t, t) is 1 up to rounding; a contrast-enhanced image scores above 1 (1.10 on the prototype)."""
    x, r = make_pair((1, 1, 48, 56), 0)
    with torch.no_grad():
        a, b = float(vif_rows(x.double(), r.double())[0]), float(vif_rows(r.double(), x.double())[0])
        same = float(vif_rows(r.double(), r.double())[0])
        more = float(vif_rows(1.5 * r.double(), r.double(), value_range=(0.0, 1.0))[0])
    assert abs(a - b) > 1e-3 and abs(same - 1) < 1e-9 and 1.05 < more < 1.15


def test_dark_planes_and_regions():
    """A plane at ``lo`` lies in the srr < EPS branch: two dark images score 1 with zero gradients; a dark reference scores 1."""
    lo = torch.full((1, 1, 48, 56), -1.0)
    ref = restate(lo, lo.clone())
    assert float(ref["score"]) == 1.0 and float(ref["dx"].abs().max()) == 0.0 and float(ref["dr"].abs().max()) == 0.0
    x, _ = make_pair((1, 1, 48, 56), 1)
    assert float(restate(x, lo, x_grad=False, r_grad=False)["score"]) == 1.0
    x, r = make_pair((1, 1, 48, 128), 2)
    x[..., 60:] = -1.0
    r[..., 60:] = -1.0
    ref = restate(x, r)
    assert float(ref["dx"][..., 101:].abs().max()) == 0.0 and float(ref["dr"][..., 101:].abs().max()) == 0.0
    assert float(ref["dx"][..., :60].abs().max()) > 0


@pytest.mark.parametrize("cfg", [DEFAULT, OTHER], ids=["default", "other"])
def test_restated_gradient_is_the_derivative(cfg):
    x, r = find_pair((2, 1, 41, 44), cfg)
    up = torch.tensor([0.75, -1.25], dtype=torch.float64)
    ref = restate(x, r, cfg, per_image=True, upstream=up)
    well_conditioned(ref)
    h = 1e-6
    f = lambda a, b: float((vif_rows(a, b, cfg["sigma_n_sq"], cfg["value_range"])[0] * up).sum())
    for k, which in (("dx", 0), ("dr", 1)):
        flat = ref[k].abs().reshape(-1)
        for at in (int(flat.argmax()), 7, flat.numel() - 3):
            d = torch.zeros(x.numel(), dtype=torch.float64)
            d[at] = h
            d = d.reshape(x.shape)
            xd, rd = x.double(), r.double()
            with torch.no_grad():
                num = ((f(xd + d, rd) - f(xd - d, rd)) if which == 0 else (f(xd, rd + d) - f(xd, rd - d))) / (2 * h)
            ana = float(ref[k].reshape(-1)[at])
            assert abs(num - ana) <= 1e-5 * abs(ana) + 1e-9, (k, at, num, ana)


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_exports_and_symbols(fa):
    import ctypes
    assert fa.VIF is fa.ssim.VIF and "VIF" in fa.__all__
    assert callable(fa.ops.vif) and callable(fa.ssim.vif)
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared and s in fa._lib.declared_symbols(), s
    assert sorted(s for s in declared if "_vif_" in s) == sorted(NEW_SYMBOLS)
    here = os.path.dirname(fa._lib.__file__)
    assert '"vif.hip"' in open(os.path.join(here, "build.py")).read() and os.path.exists(os.path.join(here, "csrc", "vif.hip"))
    lib = ctypes.CDLL(fa._lib.LIB_PATH)              # the built library exports them
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None, s
    ws = lib.faoctasr_vif_workspace_floats
    ws.restype, ws.argtypes = ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int]
    assert ws(1, 1, 40, 41) == -1 and ws(1, 1, 41, 40) == -1
    # a partial of num and one of den per tile.  41 x 41: grids 33 x 33 (three tiles, the last past the 25 x 25 stat map), 13 x 13, 5 x 5, 1 x 1;
    # 72 x 200: grids 64 x 192, 28 x 92, 12 x 44, 4 x 20
    assert ws(1, 1, 41, 41) == 2 * (3 + 1 + 1 + 1) and ws(2, 3, 41, 41) == 72
    assert ws(1, 1, 72, 200) == 2 * (4 * 3 + 2 * 2 + 1 + 1)


def test_signatures(fa):
    empty = inspect.Parameter.empty
    tail = [("sigma_n_sq", 2.0), ("value_range", (-1., 1.))]
    sig = inspect.signature(fa.ops.vif)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("a", empty), ("b", empty)] + tail + [("per_image", False)]
    sig = inspect.signature(fa.ssim.vif)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("img1", empty), ("img2", empty)] + tail + [("size_average", True)]
    sig = inspect.signature(fa.VIF.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == tail + [("size_average", True)]
    assert list(inspect.signature(fa.VIF.index).parameters)[1:] == ["img1", "img2", "per_image"]
    assert list(inspect.signature(fa.VIF.forward).parameters)[1:] == ["img1", "img2"]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("vif_weight", "vif_sigma_n_sq")] == [0.0, 2.0]
    names = list(sig.parameters)                     # keyword-only in practice; the tests of earlier terms pin the keywords from mi_normalized on
    at = names.index("ffl_batch_matrix")
    assert names[at + 1:at + 4] == ["vif_weight", "vif_sigma_n_sq", "mi_weight"]


def test_module_attributes_and_plumbing(fa, monkeypatch):
    mod = fa.VIF()
    assert (mod.sigma_n_sq, mod.value_range, mod.size_average) == (2.0, (-1.0, 1.0), True) and not list(mod.state_dict())
    mod = fa.VIF(sigma_n_sq=1, value_range=(0, 255), size_average=False)
    assert (mod.sigma_n_sq, mod.value_range, mod.size_average) == (1.0, (0.0, 255.0), False) and isinstance(mod.sigma_n_sq, float)
    assert "sigma_n_sq=1.0" in repr(mod) and "size_average=False" in repr(mod)
    seen = []
    monkeypatch.setattr(fa.ops, "vif", lambda *a: seen.append(a[2:]) or "r")
    x = torch.zeros(1, 1, 41, 41)
    assert fa.VIF(sigma_n_sq=0.4, value_range=(0, 2))(x, x) == "r"
    assert fa.VIF(size_average=False).index(x, x, False) == "r"
    assert fa.VIF(size_average=False)(x, x) == "r"
    assert fa.ssim.vif(x, x, 0.5, (0., 1.), False) == "r"
    assert fa.ssim.vif(x, x) == "r"
    assert seen == [(0.4, (0.0, 2.0), False), (2.0, (-1.0, 1.0), False), (2.0, (-1.0, 1.0), True), (0.5, (0., 1.), True), (2.0, (-1., 1.), False)]


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: a check that let one through would reach the entry point and fail there as a KernelError."""
    x = torch.zeros(1, 1, 41, 41)
    vif = fa.ops.vif
    with pytest.raises(ValueError, match="device"):
        vif(x, x)
    for f in ((lambda **kw: vif(x, x, **kw)), (lambda **kw: fa.VIF(**kw)), (lambda **kw: fa.ssim.vif(x, x, **kw))):
        for bad in (0.0, -1e-5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="sigma_n_sq must be positive and finite"):
                f(sigma_n_sq=bad)
        for bad in ("2", None, True, torch.tensor(2.0)):
            with pytest.raises(TypeError, match="sigma_n_sq must be a number"):
                f(sigma_n_sq=bad)
        for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0)):          # hi <= lo
            with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
                f(value_range=bad)
        for bad in (1.0, (1.0,), (0.0, 1.0, 2.0), None):
            with pytest.raises(TypeError, match="value_range must be a pair"):
                f(value_range=bad)
        for bad in (("0", "1"), (None, 1.0), (False, True)):
            with pytest.raises(TypeError, match="value_range's"):
                f(value_range=bad)
    for shape in ((1, 1, 40, 41), (1, 1, 41, 40), (1, 1, 8, 64), (2, 3, 64, 1)):                 # sides below 41
        with pytest.raises(ValueError, match="sides >= 41"):
            vif(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(TypeError, match="float32"):
        vif(x.double(), x.double())
    with pytest.raises(TypeError, match="float32"):
        vif(x, x.half())
    with pytest.raises(TypeError, match="tensor"):
        vif(x, x.numpy())
    with pytest.raises(ValueError, match="same shape"):
        vif(x, torch.zeros(1, 1, 41, 42))
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        vif(x[0], x[0])
    for shape in ((0, 1, 41, 41), (1, 0, 41, 41)):
        with pytest.raises(ValueError, match="non-empty"):
            vif(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match="sigma_n_sq must be positive"):                          # scalar refusals come first
        vif(x.double(), x[0], sigma_n_sq=0.0)
    m = fa.VIF()
    with pytest.raises(ValueError, match="device"):
        m(x, x)
    with pytest.raises(ValueError, match="device"):
        m.index(x, x, True)


def test_train_step_builds_the_module_only_when_asked(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    built = []
    real = fa.train.VIF

    def make(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "VIF", make)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.vif_weight == 0.0 and ts.vif is None and not built
    ts = fa.TrainStep(*nets, device="cpu", vif_sigma_n_sq=0.4)
    assert ts.vif is None and not built
    ts = fa.TrainStep(*nets, device="cpu", vif_weight=0.25, vif_sigma_n_sq=0.4)
    assert built == [dict(sigma_n_sq=0.4)]
    assert ts.vif_weight == 0.25 and (ts.vif.sigma_n_sq, ts.vif.value_range, ts.vif.size_average) == (0.4, (-1.0, 1.0), True)
    assert ts.vessel is None and ts.gmsd is None and ts.haarpsi is None and ts.lncc is None and ts.mi is None
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2", None):
        with pytest.raises(ValueError, match="vif_sigma_n_sq must be a finite number > 0"):
            fa.TrainStep(*nets, device="cpu", vif_weight=0.25, vif_sigma_n_sq=bad)
    for bad in (-1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="vif_weight must be a finite number >= 0"):
            fa.TrainStep(*nets, device="cpu", vif_weight=bad)


def test_train_step_adds_the_term_where_loss_vessel_is_added(fa):
    """``_extension_terms`` (one half per chain of the two-chain schedule, which ``GraphedTrainStep`` captures) names ``loss_vif``; with
    the module replaced by a stub no kernel runs (the single-stream ``generator_loss``: tests/test_train_terms_cpu.py)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu", vif_weight=0.5)
    seen = []
    ts.vif = lambda rec, real: (seen.append((rec, real)), (rec * real).mean())[1]
    rec, real = torch.full((1, 1, 4, 4), 0.5), torch.full((1, 1, 4, 4), 0.25)
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_vif"] and float(t["loss_vif"]) == 0.5 * (1 - 0.125)
    assert seen[0][0] is rec and seen[0][1] is real                        # the reconstruction first, the ground truth second
    assert fa.TrainStep(*nets, device="cpu")._extension_terms(rec, real) == {}
    assert not hasattr(fa.GraphedTrainStep, "generator_loss")              # it captures the TrainStep's own terms
