"""Soft-clDice (csrc/cldice.hip) without a GPU: the float64 restatement of the definition on ``max_pool2d`` against
tests/golden/golden_cldice.npz, whose values come from minima and maxima over explicit shifted slices (tools/gen_golden_cldice.py); the
conditioning caps; the fixture's layout; the seam case against the kernels' tiles; and the host logic of ``ops.soft_skeleton``,
``ops.cldice``, ``ssim.cldice``, ``SoftSkeleton``, ``SoftClDice`` and ``TrainStep(cldice_weight=..., cldice_iters=...)`` -- signatures, refusals,
plumbing -- none of which reaches an entry point.

The definition.  x, y of (N, C, H, W), channels independent grey planes pooled inside an image:

    u = (x - lo) / (hi - lo), value_range = (lo, hi), hi > lo; bright = False uses (hi - x) / (hi - lo)
    E(I) = torch.min(-max_pool2d(-I, (3, 1), 1, (1, 0)), -max_pool2d(-I, (1, 3), 1, (0, 1)))     the minimum over the 5-point cross
    D(I) = max_pool2d(I, 3, 1, 1)                                                               the maximum over the 3 x 3 square
    I_0 = u, I_{k+1} = E(I_k), O_k = D(I_{k+1}), delta_k = relu(I_k - O_k), k = 0..K, K = iters
    s_0 = delta_0, s_k = s_{k-1} + relu(delta_k - s_{k-1} delta_k), skel(u) = s_K
    Tprec = (sum skel(x) u_y + smooth) / (sum skel(x) + smooth), Tsens = (sum skel(y) u_x + smooth) / (sum skel(y) + smooth) per image n
    S[n] = 2 Tprec Tsens / (Tprec + Tsens), 0 where the denominator is 0; the index is S, the loss 1 - S

The conditioning caps, asserted on the float64 restatement before every gradient comparison: the gradient of the pair flipped on both
axes, flipped back, equals the gradient to 1e-12 in relative L2 (no tie between different pixels decides anything: on plateaus the
kernel's documented rule and ``max_pool2d``'s scan order part ways), and 1 - max skel >= 2^-6 (no mask of the recurrence on its edge)."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_cldice.npz")
MAX_ITERS = 10
TIE_CAP, SKEL_CAP = 1e-12, 2.0 ** -6
GRID = 2.0 ** 23
DEFAULT = dict(iters=3, smooth=1.0, value_range=(-1.0, 1.0), bright=True)
DARK = dict(iters=5, smooth=1.0, value_range=(0.0, 2.0), bright=False)
#: (case, shape, settings, per image, y needs a gradient, the kind of input, the case whose inputs it shares or None): tools/gen_golden_cldice.py
CASES = (("mean", (2, 1, 41, 53), DEFAULT, False, True, "smooth", None),
         ("xonly", (2, 1, 41, 53), DEFAULT, False, False, "smooth", "mean"),
         ("per_image_dark", (1, 2, 70, 140), DARK, True, True, "noise", None),
         ("limit", (1, 1, 96, 96), dict(DEFAULT, iters=MAX_ITERS), False, True, "smooth", None),
         ("small", (1, 1, 5, 7), DEFAULT, False, True, "noise", None),
         ("row", (1, 1, 1, 40), dict(DEFAULT, iters=1), False, True, "noise", None))
NEW_SYMBOLS = ("faoctasr_cldice_workspace_floats", "faoctasr_cldice_index", "faoctasr_cldice_final", "faoctasr_cldice_grad")
_gold = {}
_restated = {}


@pytest.fixture(autouse=True)
def _the_op_exists():
    """The restatement below stands for ``ops.cldice``: without the op none of these tests says anything."""
    import faoctasr
    assert callable(getattr(faoctasr.ops, "cldice", None)) and callable(getattr(faoctasr.ops, "soft_skeleton", None)) and hasattr(faoctasr, "SoftClDice")


def generator():
    spec = importlib.util.spec_from_file_location("gen_golden_cldice", os.path.join(ROOT, "tools", "gen_golden_cldice.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def unplanes(p, dtype):
    """The inverse of ``planes`` of tools/gen_golden_cldice.py: uint8 (itemsize,) + shape -> shape of ``dtype``."""
    return np.ascontiguousarray(np.moveaxis(p, 0, -1)).view(np.dtype(dtype)).reshape(p.shape[1:])


def gold():
    """The fixture, its byte planes put back together, the fp32 run's gradients rebuilt from their bit-pattern distances (exact,
    tools/gen_golden_cldice.py) and the gradients of a case that shares another's inputs taken from that case."""
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
            if case[6] is not None:
                for k in ("dx", "f32/dx"):
                    _gold["%s/%s" % (case[0], k)] = _gold["%s/%s" % (case[6], k)]
    return _gold


def kernel_tiles():
    """((CF_TY, CF_TX), (CB_TY, CB_TX)): the tiles of ``cldice_index`` and ``cldice_grad``, read out of csrc/cldice.hip."""
    import faoctasr
    with open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "csrc", "cldice.hip")) as f:
        src = f.read()
    v = {name: int(re.search(r"constexpr int [^;]*\b%s = (\d+)\b" % name, src).group(1)) for name in ("CF_TY", "CF_TX", "CB_TY", "CB_TX")}
    return (v["CF_TY"], v["CF_TX"]), (v["CB_TY"], v["CB_TX"])


def case_name(case):
    return case[0]


def fixture_inputs(case):
    """(x, y) as float32."""
    g = gold()
    src = case[6] or case[0]
    return torch.from_numpy(g[src + "/x"].copy()), torch.from_numpy(g[src + "/y"].copy())


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
def erode(I):
    return torch.min(-F.max_pool2d(-I, (3, 1), 1, (1, 0)), -F.max_pool2d(-I, (1, 3), 1, (0, 1)))


def dilate(I):
    return F.max_pool2d(I, 3, 1, 1)


def to_unit(x, value_range=(-1.0, 1.0), bright=True):
    lo, hi = value_range
    return (x - lo) / (hi - lo) if bright else (hi - x) / (hi - lo)


def skeleton(u, iters):
    I, s = u, None
    for k in range(iters + 1):
        nxt = erode(I)
        delta = torch.relu(I - dilate(nxt))
        s = delta if s is None else s + torch.relu(delta - s * delta)
        I = nxt
    return s


def cldice_rows(x, y, iters=3, smooth=1.0, value_range=(-1.0, 1.0), bright=True):
    """((N,) scores, the largest skeleton value) in the dtype of x."""
    ux, uy = to_unit(x, value_range, bright), to_unit(y, value_range, bright)
    sx, sy = skeleton(ux, iters), skeleton(uy, iters)
    tprec = ((sx * uy).sum(dim=(1, 2, 3)) + smooth) / (sx.sum(dim=(1, 2, 3)) + smooth)
    tsens = ((sy * ux).sum(dim=(1, 2, 3)) + smooth) / (sy.sum(dim=(1, 2, 3)) + smooth)
    den = tprec + tsens
    S = torch.where(den != 0, 2 * tprec * tsens / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den))
    return S, max(float(sx.detach().max()), float(sy.detach().max()))


def restate(x, y, cfg=DEFAULT, per_image=False, x_grad=True, y_grad=True, dtype=torch.float64, upstream=None):
    """{"score", "dx", "dy", "max_skel"}: the gradients are those of ``(score * upstream).sum()``."""
    x = x.to(dtype).clone().requires_grad_(x_grad)
    y = y.to(dtype).clone().requires_grad_(y_grad)
    rows, top = cldice_rows(x, y, **cfg)
    score = rows if per_image else rows.mean()
    out = dict(max_skel=top, score=score.detach())
    if x_grad or y_grad:
        (score if upstream is None else score * upstream.to(dtype)).sum().backward()
    if x_grad:
        out["dx"] = x.grad
    if y_grad:
        out["dy"] = y.grad
    return out


def restate_skeleton(x, iters=3, value_range=(-1.0, 1.0), bright=True, dtype=torch.float64, upstream=None):
    """{"map", "dx", "max_skel"} of the soft skeleton alone; the gradient is that of ``(map * upstream).sum()``."""
    x = x.to(dtype).clone().requires_grad_(upstream is not None)
    s = skeleton(to_unit(x, value_range, bright), iters)
    out = dict(map=s.detach(), max_skel=float(s.detach().max()))
    if upstream is not None:
        (s * upstream.to(dtype)).sum().backward()
        out["dx"] = x.grad
    return out


def restate_case(case, dtype=torch.float64):
    key = (case[0], dtype)
    if key not in _restated:
        x, y = fixture_inputs(case)
        _restated[key] = restate(x, y, case[2], case[3], True, case[4], dtype)
    return _restated[key]


def well_conditioned(ref64, x, y, cfg=DEFAULT, per_image=False, upstream=None):
    """The conditioning caps; returns (the flip distance, 1 - max skel)."""
    assert 1 - ref64["max_skel"] >= SKEL_CAP, ref64["max_skel"]
    keys = [k for k in ("dx", "dy") if k in ref64]
    f = restate(torch.flip(x, (2, 3)), torch.flip(y, (2, 3)), cfg, per_image, "dx" in keys, "dy" in keys, upstream=upstream)
    tie = max([rel_l2(torch.flip(f[k], (2, 3)), ref64[k]) for k in keys] or [0.0])
    assert tie <= TIE_CAP, tie
    return tie, 1 - ref64["max_skel"]


def box(n):
    ch = n.shape[1]
    return F.conv2d(F.pad(n, (2, 2, 2, 2), mode="replicate"), torch.ones(ch, 1, 5, 5) / 25.0, groups=ch)


def make_pair(shape, seed, kind="smooth", cfg=DEFAULT, levels=None):
    """(x, y) as the fixture makes them: uniform noise, or its 5 x 5 box blur rescaled to [0, 1], the partner 0.8 * that + 0.2 * other noise,
    on the grid of 2^-23 (``levels``: that many equal steps of [0, 1] instead -- plateaus), mapped into the value range; float32, exact."""
    g = torch.Generator().manual_seed(seed)
    n1, n2 = (torch.rand(*shape, generator=g, dtype=torch.float32) for _ in range(2))
    base = n1
    if kind == "smooth":
        b = box(n1)
        base = (b - b.min()) / (b.max() - b.min())
    lo, hi = cfg["value_range"]
    grid = GRID if levels is None else float(levels - 1)

    def image(u):
        u = torch.round(u.double() * grid) / grid
        v = lo + u * (hi - lo) if cfg["bright"] else hi - u * (hi - lo)
        return v.float()
    return image(base), image(0.8 * base + 0.2 * n2)


def find_pair(shape, kind="smooth", cfg=DEFAULT, per_image=False, upstream=None):
    """The first seed's pair that meets the conditioning caps."""
    for seed in range(100):
        x, y = make_pair(shape, seed, kind, cfg)
        try:
            well_conditioned(restate(x, y, cfg, per_image, upstream=upstream), x, y, cfg, per_image, upstream)
        except AssertionError:
            continue
        return x, y
    raise AssertionError("no seed of range(100) meets the caps for %s" % (shape,))


def result_keys(case):
    return ("dx", "dy") if case[4] else ("dx",)


# ------------------------------------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------------------------------------
def test_generator_constants():
    """The cases, caps and grid here are the generator's, and its inputs are the fixture's."""
    gen = generator()
    assert gen.CASES == CASES and gen.DEFAULT == DEFAULT and gen.DARK == DARK
    assert (gen.TIE_CAP, gen.SKEL_CAP, gen.GRID, gen.MAX_ITERS) == (TIE_CAP, SKEL_CAP, GRID, MAX_ITERS)
    for case in CASES:
        if case[6] is None:
            x, y = gen.make_pair(case[1], gen.SEED, case[5], case[2])
            fx, fy = fixture_inputs(case)
            assert torch.equal(x, fx) and torch.equal(y, fy)
            mx, my = make_pair(case[1], gen.SEED, case[5], case[2])
            assert torch.equal(mx, fx) and torch.equal(my, fy)


def test_fixture_layout_and_size():
    g = gold()
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_vif.npz")) < 1 << 20
    for cid, shape, cfg, per_image, y_grad, kind, shared in CASES:
        N = shape[0]
        assert g[cid + "/score"].shape == ((N,) if per_image else ()) and g[cid + "/score"].dtype == np.float64
        assert g[cid + "/f32/score"].dtype == np.float32
        for k in ("dx", "dy") if y_grad else ("dx",):
            assert g["%s/%s" % (cid, k)].shape == shape and g["%s/%s" % (cid, k)].dtype == np.float64
            assert g["%s/f32/%s" % (cid, k)].shape == shape and g["%s/f32/%s" % (cid, k)].dtype == np.float32
        if shared is None:
            x, y = fixture_inputs((cid, shape, cfg, per_image, y_grad, kind, shared))
            lo, hi = cfg["value_range"]
            assert x.dtype == torch.float32 and tuple(x.shape) == shape and tuple(y.shape) == shape
            assert float(x.min()) >= lo and float(x.max()) <= hi and float(y.min()) >= lo and float(y.max()) <= hi
            u = to_unit(x.double(), cfg["value_range"], cfg["bright"])
            assert torch.equal(u * GRID, torch.round(u * GRID))          # on the grid: the map to u is exact in fp32
            assert torch.equal(to_unit(x, cfg["value_range"], cfg["bright"]).double(), u)
        assert float(g[cid + "/tie"]) <= TIE_CAP and 1 - float(g[cid + "/max_skel"]) >= SKEL_CAP
    assert {c[2]["iters"] for c in CASES} >= {1, 3, 5, MAX_ITERS}


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_reproduces_the_fixture(case):
    """The ``max_pool2d`` restatement in float64 against the slice computation of the generator: 1e-12 (the fixture keeps 41 bits)."""
    cid = case[0]
    g = gold()
    ref = restate_case(case)
    x, y = fixture_inputs(case)
    tie, room = well_conditioned(ref, x, y, case[2], case[3])
    print("CLDICE_ERR %-16s restatement: tie %.1e  1 - max skel %.3f" % (cid, tie, room))
    assert score_err(ref["score"], g[cid + "/score"]) <= 1e-12
    assert abs(ref["max_skel"] - float(g[cid + "/max_skel"])) <= 1e-12
    for k in result_keys(case):
        assert rel_l2(ref[k], g["%s/%s" % (cid, k)]) <= 1e-12, k
    assert ("dy" in ref) == case[4]


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fp32_reference_is_the_fp32_restatement(case):
    """The fixture's fp32 arrays are this restatement run in fp32 (the same ``max_pool2d`` composition), bit for bit on this build of
    torch or within a few ulp of the score elsewhere; their distance from float64 is the e_ref of the GPU tests."""
    cid = case[0]
    g = gold()
    ref64, ref32 = restate_case(case), restate_case(case, torch.float32)
    assert score_err(ref32["score"], g[cid + "/f32/score"]) <= 4 * 2.0 ** -23
    for k in result_keys(case):
        e_ref = rel_l2(g["%s/f32/%s" % (cid, k)], ref64[k])
        print("CLDICE_ERR %-16s %-3s fp32 reference e_ref %.3e" % (cid, k, e_ref))
        assert 0 < e_ref < 1e-5
        assert rel_l2(ref32[k], g["%s/f32/%s" % (cid, k)]) <= 2 * e_ref


def test_seam_case_crosses_both_kernels_tiles():
    """(1,2,70,140) has more than one tile and a remainder on both axes of both kernels."""
    (case,) = [c for c in CASES if c[0] == "per_image_dark"]
    H, W = case[1][2:]
    for ty, tx in kernel_tiles():
        assert H > ty and H % ty and W > tx and W % tx, (ty, tx)
    (limit,) = [c for c in CASES if c[0] == "limit"]
    assert limit[2]["iters"] == MAX_ITERS and all(limit[1][2] > ty and limit[1][3] > tx for ty, tx in kernel_tiles())


def test_definition_properties_of_the_restatement():
    """A constant plane has an empty skeleton and S = 1 with smooth > 0; a one-pixel-wide line of ones on zeros is its own skeleton;
    the index is symmetric; on an 8-level image the flipped-pair gradients differ (torch's choice on plateaus depends on scan order)
    while their sums agree."""
    c = torch.full((1, 1, 9, 12), 0.25, dtype=torch.float64)
    assert float(skeleton(c, 3).abs().max()) == 0.0 and cldice_rows(c, c)[0].tolist() == [1.0]
    line = torch.zeros(1, 1, 11, 13, dtype=torch.float64)
    line[0, 0, 5, 2:11] = 1.0
    assert torch.equal(skeleton(line, 3), line)
    x, y = make_pair((1, 1, 24, 24), 1)
    assert torch.equal(cldice_rows(x.double(), y.double())[0], cldice_rows(y.double(), x.double())[0])
    qx, qy = make_pair((1, 1, 48, 48), 0, levels=8)
    assert len(torch.unique(qx)) <= 8
    a = restate(qx, qy)
    f = restate(torch.flip(qx, (2, 3)), torch.flip(qy, (2, 3)))
    assert float(a["score"]) == pytest.approx(float(f["score"]), rel=1e-14)
    assert rel_l2(torch.flip(f["dx"], (2, 3)), a["dx"]) > 1e-3
    assert float(f["dx"].sum()) == pytest.approx(float(a["dx"].sum()), rel=1e-9)


# ------------------------------------------------------------------------------------------------------------------------
# the host side
# ------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols_and_signatures():
    import faoctasr
    lib = faoctasr._lib.load()
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        header = f.read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in faoctasr._lib.declared_symbols() and re.search(r"\b%s\(" % s, header), s
    assert lib.faoctasr_cldice_workspace_floats(2, 1, 41, 53) == 4 * 2 * 3 + 2 * 2         # 16 x 64 tiles: 3 x 1 per plane
    assert lib.faoctasr_cldice_workspace_floats(0, 1, 8, 8) == -1
    assert "cldice.hip" in open(os.path.join(os.path.dirname(faoctasr._lib.__file__), "build.py")).read()


def test_signatures():
    import faoctasr as fa
    empty = inspect.Parameter.empty
    sig = inspect.signature(fa.ops.soft_skeleton)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("x", empty), ("iters", 3), ("value_range", (-1., 1.)), ("bright", True)]
    sig = inspect.signature(fa.ops.cldice)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("a", empty), ("b", empty), ("iters", 3), ("smooth", 1.0), ("value_range", (-1., 1.)),
                                                                  ("bright", True), ("per_image", False)]
    sig = inspect.signature(fa.ssim.cldice)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("img1", empty), ("img2", empty), ("iters", 3), ("smooth", 1.0),
                                                                  ("value_range", (-1., 1.)), ("bright", True), ("size_average", True)]
    sig = inspect.signature(fa.SoftClDice.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("iters", 3), ("smooth", 1.0), ("value_range", (-1., 1.)), ("bright", True),
                                                                            ("size_average", True)]
    sig = inspect.signature(fa.SoftSkeleton.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("iters", 3), ("value_range", (-1., 1.)), ("bright", True)]
    assert list(inspect.signature(fa.SoftClDice.index).parameters)[1:] == ["img1", "img2", "per_image"]
    assert list(inspect.signature(fa.SoftClDice.forward).parameters)[1:] == ["img1", "img2"]
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("cldice_weight", "cldice_iters")] == [0.0, 3]
    assert fa.ops.CLDICE_MAX_ITERS == MAX_ITERS
    assert "SoftClDice" in fa.__all__ and "SoftSkeleton" in fa.__all__
    assert "first" in fa.ops.cldice.__doc__.lower() and "subgradient" in fa.ops.cldice.__doc__ and "1..10" in fa.ops.cldice.__doc__
    r = repr(fa.SoftClDice(iters=5, smooth=0.5, value_range=(0, 1), bright=False))
    assert "iters=5" in r and "smooth=0.5" in r and "value_range=(0.0, 1.0)" in r and "bright=False" in r


def test_argument_errors():
    """Every refusal that concerns no device: raised before a tensor's device is looked at."""
    import faoctasr as fa
    x = torch.zeros(1, 1, 8, 8)
    for bad in (0, MAX_ITERS + 1, -1):
        with pytest.raises(ValueError, match=r"iters must lie in 1\.\.10"):
            fa.ops.cldice(x, x, iters=bad)
        with pytest.raises(ValueError, match=r"iters must lie in 1\.\.10"):
            fa.ops.soft_skeleton(x, iters=bad)
        with pytest.raises(ValueError, match=r"iters must lie in 1\.\.10"):
            fa.SoftClDice(iters=bad)
    for bad in (2.0, True, "3", None):
        with pytest.raises(TypeError, match="iters must be an integer"):
            fa.ops.cldice(x, x, iters=bad)
    for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
            fa.ops.cldice(x, x, value_range=bad)
        with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
            fa.SoftSkeleton(value_range=bad)
    with pytest.raises(TypeError, match="value_range must be a pair"):
        fa.ops.cldice(x, x, value_range=1.0)
    for bad in (-1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="smooth must be finite and >= 0"):
            fa.ops.cldice(x, x, smooth=bad)
    with pytest.raises(TypeError, match="smooth must be a number"):
        fa.ops.cldice(x, x, smooth="1")
    with pytest.raises(TypeError, match="a must be a float32 tensor"):
        fa.ops.cldice(x.double(), x)
    with pytest.raises(TypeError, match="b must be a float32 tensor"):
        fa.ops.cldice(x, x.half())
    with pytest.raises(TypeError, match="x must be a float32 tensor"):
        fa.ops.soft_skeleton(x.double())
    with pytest.raises(ValueError, match="a and b must have the same shape"):
        fa.ops.cldice(x, torch.zeros(1, 1, 8, 9))
    with pytest.raises(ValueError, match=r"a must be \(N, C, H, W\)"):
        fa.ops.cldice(x[0], x[0])
    with pytest.raises(ValueError, match="non-empty"):
        fa.ops.cldice(x[:0], x[:0])
    with pytest.raises(ValueError, match="a must be on a GPU device"):
        fa.ops.cldice(x, x)
    with pytest.raises(TypeError, match="a must be a tensor"):
        fa.ops.cldice(x.numpy(), x)


def small_nets(fa):
    return (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))


def test_train_step_arguments(monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor): weight 0 builds no module."""
    import faoctasr as fa
    built = []
    real = fa.train.SoftClDice

    def make(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "SoftClDice", make)
    nets = small_nets(fa)
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.cldice_weight == 0.0 and ts.cldice is None and not built
    ts = fa.TrainStep(*nets, device="cpu", cldice_weight=0.25, cldice_iters=5)
    assert built == [dict(iters=5)]
    assert ts.cldice_weight == 0.25 and (ts.cldice.iters, ts.cldice.smooth, ts.cldice.value_range, ts.cldice.bright, ts.cldice.size_average) == (
        5, 1.0, (-1.0, 1.0), True, True)
    for bad in (0, 11):
        with pytest.raises(ValueError, match=r"iters must lie in 1\.\.10"):
            fa.TrainStep(*nets, device="cpu", cldice_weight=0.25, cldice_iters=bad)
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="cldice_weight must be a finite number >= 0"):
            fa.TrainStep(*nets, device="cpu", cldice_weight=bad)


def test_train_step_term_placement():
    """``_extension_terms`` (one half per chain of the two-chain schedule, which ``GraphedTrainStep`` captures) names ``loss_cldice``; with
    the module replaced by a stub no kernel runs (the single-stream ``generator_loss``: tests/test_train_terms_cpu.py).  The module's
    ``forward`` is the loss 1 - S, so the term is the weight times the module's value."""
    import faoctasr as fa
    nets = small_nets(fa)
    ts = fa.TrainStep(*nets, device="cpu", cldice_weight=0.5)
    rec, real = torch.zeros(1, 1, 4, 4), torch.ones(1, 1, 4, 4)
    seen = []
    ts.cldice = lambda a, b: (seen.append((a, b)), torch.tensor(0.125))[1]
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_cldice"] and float(t["loss_cldice"]) == 0.5 * 0.125
    assert seen[0][0] is rec and seen[0][1] is real
    assert fa.TrainStep(*nets, device="cpu")._extension_terms(rec, real) == {}
    x = torch.rand(2, 1, 8, 8)
    mod = fa.SoftClDice()
    mod.index = lambda a, b, per_image: torch.tensor([0.25, 0.75]) if per_image else torch.tensor(0.5)
    assert float(mod(x, x)) == 0.5 and fa.SoftClDice.forward(mod, x, x).shape == ()
    mod.size_average = False
    assert mod(x, x).tolist() == [0.75, 0.25]
