"""Soft-clDice (csrc/cldice.hip) on the MI355X: ``ops.cldice`` / ``ops.soft_skeleton`` / ``ssim.cldice`` / ``SoftSkeleton`` / ``SoftClDice``
against the float64 restatement of tests/test_cldice_cpu.py (pinned there to tests/golden/golden_cldice.npz, whose values come from
explicit shifted slices): every fixture case, an off-fixture per-image pair with an upstream gradient, the skeleton alone, the exact
properties, the closed forms, a quantised pair (ties), the composition with ``ops.vesselness``, the structure of the launches,
``evaluate_pairs_with(cldice=...)`` and the opt-in ``TrainStep(cldice_weight=...)`` term, eager in both schedules and as a captured graph.

The bars.  With ``e_ref`` the distance of the fp32 reference (the fixture's ``f32`` arrays, the torch composition in fp32; off the
fixture the restatement run in fp32) from float64 and ``E_ref`` the largest relative score error of the fp32 reference over the
fixture (and the case at hand):

    arrays, relative L2 per array:   e_hip <= 2 e_ref + 2^-23
    scores, relative:                e_hip <= 2 E_ref + 1 ulp

Both are measured against the reference; nothing is fixed in advance.

The conditioning caps (tests/test_cldice_cpu.py): every gradient comparison first asserts, on the float64 restatement, that the gradient
of the pair flipped on both axes, flipped back, equals the gradient to 1e-12 (no tie between different pixels decides anything) and
that 1 - max skel >= 2^-6.

Each array prints a ``CLDICE_ERR`` line (run with ``-s``; a run's lines are what profiles/cldice_error.txt holds)."""
import math
import random

import pytest
import torch

from test_cldice_cpu import (CASES, DEFAULT, MAX_ITERS, case_name, cldice_rows, find_pair, fixture_inputs, gold, kernel_tiles, make_pair, rel_l2,
                             restate, restate_case, restate_skeleton, score_err, well_conditioned)

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
# cldice_index(x, y, skel_x, skel_y, rec_x, sel_x, rec_y, sel_y, workspace, N, C, H, W, iters, lo, hi, bright, stream)
SKEL_X_ARG, SKEL_Y_ARG, REC_X_ARG, SEL_X_ARG, REC_Y_ARG, SEL_Y_ARG, WS_ARG = 2, 3, 4, 5, 6, 7, 8
TABLE_ARG = 9                                 # cldice_final(workspace, N, C, H, W, smooth, average, out_image, out_mean, table, stream)
# cldice_grad(x, y, rec_x, sel_x, rec_y, sel_y, skel_x, skel_y, table, g, gN, dx, dy, N, C, H, W, iters, lo, hi, bright, stream)
GREC_X_ARG, GREC_Y_ARG, GSKEL_X_ARG, GSKEL_Y_ARG, GTABLE_ARG, G_ARG, DX_ARG, DY_ARG = 2, 4, 6, 7, 8, 9, 11, 12
FWD_NAMES = ["cldice_index", "cldice_final"]
BWD_NAMES = ["cldice_grad"]


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def op(fa, x, y, cfg=DEFAULT, per_image=False):
    return fa.ops.cldice(x, y, cfg["iters"], cfg["smooth"], cfg["value_range"], cfg["bright"], per_image)


def run_hip(fa, x, y, cfg=DEFAULT, per_image=False, x_grad=True, y_grad=True, upstream=None):
    """{"score", "dx", "dy"} of the op on the GPU, back on the host; the gradients are those of ``(score * upstream).sum()``."""
    xd = x.float().cuda().detach().requires_grad_(x_grad)
    yd = y.float().cuda().detach().requires_grad_(y_grad)
    S = op(fa, xd, yd, cfg, per_image)
    assert S.dtype == torch.float32 and S.shape == ((x.shape[0],) if per_image else ())
    if x_grad or y_grad:
        (S if upstream is None else S * upstream.cuda()).sum().backward()
    torch.cuda.synchronize()
    out = {"score": S.detach().cpu()}
    if x_grad:
        out["dx"] = xd.grad.cpu()
    if y_grad:
        out["dy"] = yd.grad.cpu()
    return out


def ulp_rel(v):
    v = abs(float(v))
    return 2.0 ** (math.floor(math.log2(v)) - 23) / v


_E = []


def score_E_ref():
    """The largest relative error of the fp32 reference's score over all fixture cases."""
    if not _E:
        g = gold()
        _E.append(max(score_err(g[c[0] + "/f32/score"], restate_case(c)["score"]) for c in CASES))
    return _E[0]


def score_holds(got, ref64, E_ref=None):
    E_ref = score_E_ref() if E_ref is None else E_ref
    return all(score_err(s_got, s_ref) <= K2 * E_ref + ulp_rel(s_ref) for s_got, s_ref in zip(got.reshape(-1), ref64.reshape(-1)))


def array_holds(name, key, got, ref32, ref64, bad):
    assert tuple(got.shape) == tuple(ref64.shape)
    e_ref, e_hip = rel_l2(ref32, ref64), rel_l2(got, ref64)
    print("CLDICE_ERR %-34s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, key, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
    if not e_hip <= K2 * e_ref + FLOOR:
        bad.append((key, e_hip, e_ref))


def hold_to_bar(name, ref64, ref32, got, caps):
    """Print e_ref, e_hip and their ratio per array, then assert the bars of the module docstring on every one."""
    bad = []
    own = score_err(ref32["score"], ref64["score"])
    E_ref = max(score_E_ref(), own)
    e_hip = score_err(got["score"], ref64["score"])
    print("CLDICE_ERR %-34s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f tie %.1e 1 - max skel %.3f" % (
        name, "score", E_ref, own, e_hip, e_hip / E_ref, caps[0], caps[1]))
    assert tuple(got["score"].shape) == tuple(ref64["score"].shape)
    if not score_holds(got["score"], ref64["score"], E_ref):
        bad.append(("score", e_hip, E_ref))
    for k in ("dx", "dy"):
        if k not in ref64:
            assert k not in got
            continue
        array_holds(name, k, got[k], ref32[k], ref64[k], bad)
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """Every fixture case: (2,1,41,53) K = 3, the mean over the batch, and the same with y needing no gradient (the null ``dy``);
    (1,2,70,140) K = 5 per image with value_range (0, 2) and dark vessels, across the seams of both kernels' tiles on both axes;
    (1,1,96,96) K = 10, the limit; (1,1,5,7) K = 3 and (1,1,1,40) K = 1, images smaller than the halo and a side of 1."""
    cid, shape, cfg, per_image, y_grad, _, _ = case
    if cid == "per_image_dark":
        assert all(shape[2] > ty and shape[2] % ty and shape[3] > tx and shape[3] % tx for ty, tx in kernel_tiles())
    g = gold()
    ref64 = restate_case(case)
    x, y = fixture_inputs(case)
    caps = well_conditioned(ref64, x, y, cfg, per_image)
    ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("score", "dx", "dy") if k in ref64}
    hold_to_bar("%s %s" % (cid, "x".join(map(str, shape))), ref64, ref32, run_hip(fa, x, y, cfg, per_image, True, y_grad), caps)


def test_per_image_with_upstream(fa):
    """Per-image scores of an odd-sided pair with an upstream gradient per image, read on the device; off the fixture."""
    up = torch.tensor([0.25, -1.5])
    x, y = find_pair((2, 1, 45, 83), per_image=True, upstream=up)
    ref64 = restate(x, y, per_image=True, upstream=up)
    ref32 = restate(x, y, per_image=True, upstream=up, dtype=torch.float32)
    caps = well_conditioned(ref64, x, y, DEFAULT, True, up)
    hold_to_bar("upstream 2x1x45x83", ref64, ref32, run_hip(fa, x, y, per_image=True, upstream=up), caps)


@pytest.mark.parametrize("iters,value_range,bright,shape", [(3, (-1.0, 1.0), True, (2, 1, 41, 53)), (MAX_ITERS, (0.0, 2.0), False, (1, 2, 37, 70))],
                         ids=["K3", "K10_dark"])
def test_soft_skeleton_alone(fa, iters, value_range, bright, shape):
    """``ops.soft_skeleton``: the map, and its gradient under a random upstream map, at the array bar."""
    cfg = dict(DEFAULT, iters=iters, value_range=value_range, bright=bright)
    x, _ = make_pair(shape, 3, "smooth", cfg)
    up = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    ref64 = restate_skeleton(x, iters, value_range, bright, upstream=up)
    ref32 = restate_skeleton(x, iters, value_range, bright, dtype=torch.float32, upstream=up)
    flipped = restate_skeleton(torch.flip(x, (2, 3)), iters, value_range, bright, upstream=torch.flip(up, (2, 3)))
    assert rel_l2(torch.flip(flipped["dx"], (2, 3)), ref64["dx"]) <= 1e-12 and 1 - ref64["max_skel"] >= 2.0 ** -6
    xd = x.cuda().requires_grad_(True)
    m = fa.ops.soft_skeleton(xd, iters, value_range, bright)
    assert m.dtype == torch.float32 and m.shape == x.shape
    (m * up.cuda()).sum().backward()
    mod = fa.SoftSkeleton(iters, value_range, bright).cuda()
    assert torch.equal(mod(x.cuda()), m.detach())
    bad = []
    array_holds("skeleton K=%d %s" % (iters, "x".join(map(str, shape))), "map", m.detach().cpu(), ref32["map"], ref64["map"], bad)
    array_holds("skeleton K=%d %s" % (iters, "x".join(map(str, shape))), "dx", xd.grad.cpu(), ref32["dx"], ref64["dx"], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, y, cfg=DEFAULT, scale=None, per_image=False):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    S = op(fa, xd, yd, cfg, per_image)
    (S.sum() if scale is None else (S * scale).sum()).backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize("shape,iters", [((2, 2, 41, 72), 3), ((1, 3, 37, 73), MAX_ITERS), ((2, 1, 19, 130), 5)], ids=lambda s: str(s).replace(" ", ""))
def test_bit_for_bit_properties(fa, shape, iters):
    """``S(x, y) == S(y, x)`` with swapped gradients; two runs agree; halving the upstream gradient halves both gradients; an image alone
    scores what it scores in a batch."""
    cfg = dict(DEFAULT, iters=iters)
    x, y = (t.cuda() for t in make_pair(shape, 5))
    S, dx, dy = grads(fa, x, y, cfg)
    assert 0 < float(S) < 1 and dx.abs().max() > 0 and dy.abs().max() > 0
    again = grads(fa, x, y, cfg)
    assert torch.equal(again[0], S) and torch.equal(again[1], dx) and torch.equal(again[2], dy)
    swapped = grads(fa, y, x, cfg)
    assert torch.equal(swapped[0], S) and torch.equal(swapped[1], dy) and torch.equal(swapped[2], dx)
    _, hx, hy = grads(fa, x, y, cfg, scale=0.5)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hy, 0.5 * dy)         # the upstream gradient, applied on the device
    rows, rdx, rdy = grads(fa, x, y, cfg, per_image=True)
    for n in range(shape[0]):
        alone, adx, ady = grads(fa, x[n:n + 1], y[n:n + 1], cfg, per_image=True)
        assert torch.equal(alone[0], rows[n]) and torch.equal(adx[0], rdx[n]) and torch.equal(ady[0], rdy[n])


def test_bit_reproducible_on_a_side_stream(fa):
    x, y = make_pair((2, 1, 40, 150), 6)
    first = run_hip(fa, x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_hip(fa, x, y)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(first[k], side[k]) for k in first)


def test_one_sided_gradient_is_the_two_sided_one(fa):
    """A null ``dx`` / ``dy`` skips that side in ``cldice_grad`` and that side's records in ``cldice_index``; the side that is asked for keeps
    its bits.  (2, 1, 41, 72): several tiles and a remainder."""
    x, y = make_pair((2, 1, 41, 72), 8)
    both = run_hip(fa, x, y)
    only_x, only_y = run_hip(fa, x, y, y_grad=False), run_hip(fa, x, y, x_grad=False)
    assert "dy" not in only_x and "dx" not in only_y
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_y["dy"], both["dy"]) and both["dx"].abs().max() > 0
    assert torch.equal(only_x["score"], both["score"]) and torch.equal(only_y["score"], both["score"])


# ------------------------------------------------------------------------------------------------------------------------
# closed forms, ties, vessel maps
# ------------------------------------------------------------------------------------------------------------------------
def test_constant_plane(fa):
    """A constant plane has a skeleton of exactly 0; two of them score exactly 1 with smooth > 0, with gradients exactly 0."""
    c = torch.full((2, 1, 37, 70), 0.25)
    assert float(fa.ops.soft_skeleton(c.cuda()).abs().max()) == 0.0
    got = run_hip(fa, c, torch.full_like(c, -0.5), per_image=True)
    assert got["score"].tolist() == [1.0, 1.0] and float(got["dx"].abs().max()) == 0.0 and float(got["dy"].abs().max()) == 0.0


def test_line_is_its_own_skeleton(fa):
    """A one-pixel-wide line of ones on zeros, horizontal across a tile seam and vertical, is its own skeleton exactly."""
    line = torch.zeros(1, 2, 40, 90)
    line[0, 0, 17, 3:85] = 1.0
    line[0, 1, 2:38, 64] = 1.0
    for iters in (1, 3, MAX_ITERS):
        assert torch.equal(fa.ops.soft_skeleton(line.cuda(), iters, (0.0, 1.0)).cpu(), line)
    got = run_hip(fa, line, line.clone(), dict(DEFAULT, value_range=(0.0, 1.0)))
    assert float(got["score"]) == 1.0


def test_ties_on_a_quantised_pair(fa):
    """An 8-level (1,1,48,48) pair: plateaus everywhere.  The forward does not depend on ties, so the score meets the bar; the gradients
    follow the kernel's own rule (the first tied position in row-major order takes the whole cotangent), so they are finite, repeat bit
    for bit and conserve the total: the sums of dx and dy equal the float64 restatement's within twice the fp32 composition's error
    on those sums, plus one ulp.  No elementwise comparison."""
    x, y = make_pair((1, 1, 48, 48), 0, levels=8)
    assert len(torch.unique(x)) <= 8 and len(torch.unique(y)) <= 8
    ref64, ref32 = restate(x, y), restate(x, y, dtype=torch.float32)
    got, again = run_hip(fa, x, y), run_hip(fa, x, y)
    own = score_err(ref32["score"], ref64["score"])
    print("CLDICE_ERR ties 8 levels 1x1x48x48            score  e_ref %.3e e_hip %.3e" % (max(score_E_ref(), own), score_err(got["score"], ref64["score"])))
    assert score_holds(got["score"], ref64["score"], max(score_E_ref(), own))
    bad = []
    for k in ("dx", "dy"):
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], again[k]) and got[k].abs().max() > 0
        want, ref, have = float(ref64[k].sum()), float(ref32[k].double().sum()), float(got[k].double().sum())
        print("CLDICE_ERR ties 8 levels 1x1x48x48            sum %s float64 %.9e fp32 composition off by %.3e kernel off by %.3e" % (
            k, want, abs(ref - want), abs(have - want)))
        if not abs(have - want) <= K2 * abs(ref - want) + ulp_rel(want) * abs(want):
            bad.append((k, have - want, ref - want))
    assert not bad, bad


def test_composes_with_vesselness(fa):
    """``cldice(V(x), V(y), value_range=(0, 1))`` through autograd on (1,1,64,64): the score meets the bar against the composed restatements;
    a vesselness map has regions of exactly 0, plateaus on which the tie rule applies, so the gradients are only asked to be finite
    and reproducible."""
    from test_vessel_cpu import make_pair as vessel_pair, response
    x, y = vessel_pair((1, 1, 64, 64), 2)
    cfg = dict(DEFAULT, value_range=(0.0, 1.0))

    def composed(dtype):
        with torch.no_grad():
            return cldice_rows(response(x.to(dtype))[0], response(y.to(dtype))[0], **cfg)[0].mean()
    ref64, ref32 = composed(torch.float64), composed(torch.float32)

    def run():
        xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        S = op(fa, fa.ops.vesselness(xd), fa.ops.vesselness(yd), cfg)
        S.backward()
        torch.cuda.synchronize()
        return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()
    S, dx, dy = run()
    E_ref = max(score_E_ref(), score_err(ref32, ref64))
    print("CLDICE_ERR vesselness composition 1x1x64x64     score  %.9f restatement %.9f e_ref %.3e e_hip %.3e" % (S, ref64, E_ref, score_err(S, ref64)))
    assert 0 < float(ref64) < 1 and score_holds(S, ref64, E_ref)
    again = run()
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all() and dx.abs().max() > 0 and dy.abs().max() > 0
    assert torch.equal(again[0], S) and torch.equal(again[1], dx) and torch.equal(again[2], dy)


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def test_launch_counts(fa, monkeypatch):
    """Two entry points forward (``cldice_index``, ``cldice_final``) and one backward.  Records are kept for the inputs that need a
    gradient only, and the skeleton map of the other image with them."""
    x, y = (t.cuda() for t in make_pair((2, 2, 41, 72), 3))
    for x_grad, y_grad in ((True, True), (True, False), (False, True)):
        xd, yd = x.clone().requires_grad_(x_grad), y.clone().requires_grad_(y_grad)
        calls = spy(fa, monkeypatch)
        S = op(fa, xd, yd)
        assert [n for n, _ in calls] == FWD_NAMES and calls[1][1][TABLE_ARG] and calls[0][1][WS_ARG]
        a = calls[0][1]
        assert bool(a[REC_X_ARG]) == bool(a[SEL_X_ARG]) == bool(a[SKEL_Y_ARG]) == x_grad
        assert bool(a[REC_Y_ARG]) == bool(a[SEL_Y_ARG]) == bool(a[SKEL_X_ARG]) == y_grad
        del calls[:]
        S.backward()
        assert [n for n, _ in calls] == BWD_NAMES
        a = calls[0][1]
        assert bool(a[DX_ARG]) == bool(a[GREC_X_ARG]) == bool(a[GSKEL_Y_ARG]) == x_grad
        assert bool(a[DY_ARG]) == bool(a[GREC_Y_ARG]) == bool(a[GSKEL_X_ARG]) == y_grad and a[G_ARG] and a[GTABLE_ARG]
        assert (xd.grad is not None) == x_grad and (yd.grad is not None) == y_grad
        monkeypatch.undo()
    calls = spy(fa, monkeypatch)
    xd = x.clone().requires_grad_(True)
    m = fa.ops.soft_skeleton(xd)
    m.sum().backward()
    assert [n for n, _ in calls] == ["cldice_index", "cldice_grad"]
    assert calls[0][1][1] is None and calls[0][1][REC_X_ARG] and calls[0][1][WS_ARG] is None and calls[1][1][GTABLE_ARG] is None
    del calls[:]
    fa.ops.soft_skeleton(x)
    assert [n for n, _ in calls] == ["cldice_index"] and calls[0][1][REC_X_ARG] is None and calls[0][1][SEL_X_ARG] is None


def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch):
    N, C, H, W = 2, 3, 41, 72
    K = DEFAULT["iters"]
    x, y = (t.cuda() for t in make_pair((N, C, H, W), 2))
    calls = spy(fa, monkeypatch)
    Sg = op(fa, x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert calls[-1][0] == "cldice_final" and calls[-1][1][TABLE_ARG]
    # the two images, the table, and per side K + 1 coefficient maps, K + 1 maps of selection bytes and the other image's skeleton map
    saved = [(tuple(t.shape), t.dtype) for t in Sg.grad_fn.saved_tensors]
    side = [((K + 1, N, C, H, W), torch.float32), ((K + 1, N, C, H, W), torch.uint8), ((N, C, H, W), torch.float32)]
    assert saved == [((N, C, H, W), torch.float32)] * 2 + [((4, N), torch.float32)] + side * 2
    del calls[:]
    with torch.no_grad():
        Sn = op(fa, x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert [n for n, _ in calls] == FWD_NAMES and calls[1][1][TABLE_ARG] is None
    assert all(calls[0][1][i] is None for i in (SKEL_X_ARG, SKEL_Y_ARG, REC_X_ARG, SEL_X_ARG, REC_Y_ARG, SEL_Y_ARG))     # null pointers: nothing is stored
    assert not Sn.requires_grad and Sn.grad_fn is None
    del calls[:]
    Sp = op(fa, x, y)                                                      # inputs that need no gradient
    assert len(calls) == 2 and calls[1][1][TABLE_ARG] is None and calls[0][1][REC_X_ARG] is None and not Sp.requires_grad
    assert torch.equal(Sn, Sg) and torch.equal(Sp, Sg)


def test_module_and_function_are_the_op(fa):
    x, y = (t.cuda() for t in make_pair((2, 1, 41, 56), 4, cfg=dict(DEFAULT, value_range=(0.0, 2.0))))
    big = torch.cat((x, x), dim=3)
    vx, vy = big[:, :, :, 56:], torch.cat((y, y), dim=3)[:, :, :, 56:]      # views equal their contiguous copies
    assert not vx.is_contiguous()
    args = (5, 0.5, (0., 2.), False)
    want, rows = fa.ops.cldice(x, y, *args), fa.ops.cldice(x, y, *args, True)
    mod = fa.SoftClDice(*args).cuda()
    assert torch.equal(mod.index(x, y, False), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(mod(x, y), 1 - want)                                # forward is the loss
    assert torch.equal(fa.SoftClDice(*args, size_average=False)(x, y), 1 - rows)
    assert torch.equal(fa.ssim.cldice(x, y, *args), want)
    assert torch.equal(fa.ssim.cldice(x, y, *args, size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    assert torch.equal(mod.index(vx, vy, False), want)
    assert torch.equal(fa.SoftClDice().cuda().index(x, y, False), fa.ops.cldice(x, y))


def test_capturable(fa):
    """Forward and backward captured in one hipGraph replay to the eager bits: nothing is allocated or read on the host."""
    x, y = (t.cuda() for t in make_pair((2, 1, 41, 72), 9))
    eager = run_hip(fa, x.cpu(), y.cpu())
    xs = x.clone().requires_grad_(True)
    op(fa, xs, y).backward()                                               # warm-up: the workspace exists before the capture
    xs.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        S = op(fa, xs, y)
        (dx,) = torch.autograd.grad(S, xs)
    S.detach().zero_()
    dx.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(S.detach().cpu(), eager["score"]) and torch.equal(dx.cpu(), eager["dx"])


def test_argument_errors_on_the_device(fa):
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    for bad in (0, MAX_ITERS + 1):
        with pytest.raises(ValueError, match=r"iters must lie in 1\.\.10"):
            fa.ops.cldice(x, x, iters=bad)
    with pytest.raises(ValueError, match="value_range must be finite with hi > lo"):
        fa.ops.cldice(x, x, value_range=(1.0, 1.0))
    with pytest.raises(ValueError, match="smooth must be finite and >= 0"):
        fa.ops.cldice(x, x, smooth=-1.0)
    with pytest.raises(TypeError, match="a must be a float32 tensor"):
        fa.ops.cldice(x.double(), x)
    with pytest.raises(ValueError, match="a and b must have the same shape"):
        fa.ops.cldice(x, torch.zeros(1, 1, 8, 9, device="cuda"))
    with pytest.raises(ValueError, match="b must be on a GPU device"):
        fa.ops.cldice(x, x.cpu())
    lib = fa._lib.load()
    assert lib.faoctasr_cldice_index(x.data_ptr(), None, x.data_ptr(), None, None, None, None, None, None, 1, 1, 8, 8, 11, -1.0, 1.0, 1, None) != 0
    assert b"iters 11" in lib.faoctasr_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# the evaluation path
# ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pairs_with_key(fa, monkeypatch):
    """The key is the mean of the per-image index of (super_resolve(lr), hr) against the restatement on two 41 x 56 pairs.  The generator's
    forward is not bit-reproducible (split-K atomics), so ``super_resolve`` is replaced by a fixed map."""
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: (0.5 * lr).contiguous())
    pairs = []
    for seed, n in ((21, 2), (22, 1)):
        lr, hr = make_pair((n, 1, 41, 56), seed)
        pairs.append((lr.cuda(), hr.cuda()))
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs_with(None, pairs, cldice=fa.SoftClDice().cuda())
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "cldice"] and all(out[k] == plain[k] for k in plain)

    def rows_of(dtype):
        return torch.cat([restate((0.5 * lr).cpu(), hr.cpu(), per_image=True, x_grad=False, y_grad=False, dtype=dtype)["score"] for lr, hr in pairs])
    rows, rows32 = rows_of(torch.float64), rows_of(torch.float32)
    E_ref = max(score_E_ref(), score_err(rows32, rows))
    want = float(rows.mean())
    print("CLDICE_ERR evaluate_pairs_with: cldice %.9f restatement %.9f E_ref %.3e" % (out["cldice"], want, E_ref))
    assert rows.shape == (3,) and 0 < want < 1 and abs(out["cldice"] - want) <= (K2 * E_ref + ulp_rel(want)) * want


# ------------------------------------------------------------------------------------------------------------------------
# the train step's opt-in term
# ------------------------------------------------------------------------------------------------------------------------
def build_nets(fa, O, seed=0):
    nets = {"A2B": fa.NetworkA2B(), "B2A": fa.NetworkB2A(), "D_A": fa.FS_DiscriminatorA(1), "D_B": fa.FS_DiscriminatorB(1)}
    specs = {"A2B": O.spec_network_a2b(), "B2A": O.spec_network_b2a(), "D_A": O.spec_fs_discriminator("sum"), "D_B": O.spec_fs_discriminator("cat")}
    for k, n in nets.items():
        n.load_state_dict(O.make_state(specs[k], k, seed), strict=True)
        n.cuda().train()
    return nets


def fresh_step(fa, O, **kw):
    random.seed(1234)
    n = build_nets(fa, O)
    return fa.TrainStep(n["A2B"], n["B2A"], n["D_A"], n["D_B"], **kw)


def counted(calls):
    names = {}
    for n, _ in calls:
        names[n] = names.get(n, 0) + 1
    return names


@pytest.mark.parametrize("two_chains", [True, False])
def test_train_step_cldice_term(fa, O, two_chains, monkeypatch):
    """192^2, batch 1, the smallest step of tests/test_gpu_step.py.  With ``reproducible_forward`` the forward and the losses are
    bit-reproducible, so against the weight-0 step: the tensors and every other loss keep their bits; ``loss_cldice`` is the composition
    of the op on the step's own tensors -- 0.5 ((1 - S(recovered_A, real_A)) + (1 - S(recovered_B, real_B))), formed in double from the
    op's fp32 scores; the step forms it in fp32, in the two-chain schedule as two halves: absolute roundings of 2^-24 on values of order
    1, hence 4 * 2^-24 absolute -- and ``loss_G`` is the weight-0 step's plus the term, to fp32 rounding of the sum (1e-6 relative).
    The weight-0 step launches no ``cldice_*`` entry and the step with the term launches exactly two forwards and two one-sided
    backwards more; every other entry point keeps its count."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    calls = spy(fa, monkeypatch)
    try:
        tsd = fresh_step(fa, O, reproducible_forward=True)                 # the default step, first: it fills the process-wide tables
        Ld = tsd.step(a, b, sync=True, keep=True)
        ts = fresh_step(fa, O, reproducible_forward=True, cldice_weight=0.5)
        del calls[:]
        L = ts.step(a, b, sync=True, keep=True)
        with_term = counted(calls)
        grad_calls = [args for n, args in calls if n == "cldice_grad"]
        ts0 = fresh_step(fa, O, reproducible_forward=True, cldice_weight=0.0)
        del calls[:]
        L0 = ts0.step(a, b, sync=True, keep=True)
        without = counted(calls)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_cldice" not in L0 and ts0.cldice is None and tsd.cldice is None and isinstance(ts.cldice, fa.SoftClDice)
    assert L0["loss_G"] == Ld["loss_G"]                                    # weight 0 is the default step, bit for bit
    assert not [n for n in without if n.startswith("cldice")]
    assert {n: c for n, c in with_term.items() if n.startswith("cldice")} == {"cldice_index": 2, "cldice_final": 2, "cldice_grad": 2}
    assert {n: c for n, c in with_term.items() if not n.startswith("cldice")} == without
    assert all(bool(g[DX_ARG]) and not g[DY_ARG] and not g[GREC_Y_ARG] for g in grad_calls)      # the gradient reaches the reconstruction only
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    with torch.no_grad():
        want = 0.5 * sum(1.0 - float(ts.cldice.index(rec, real, False)) for rec, real in ((T["recovered_A"], a), (T["recovered_B"], b)))
    print("CLDICE_ERR step two_chains=%s: loss_cldice %.7f composition %.7f, loss_G %.6f against %.6f at weight 0" % (
        two_chains, L["loss_cldice"], want, L["loss_G"], L0["loss_G"]))
    assert want > 0 and abs(L["loss_cldice"] - want) <= 4 * 2.0 ** -24
    assert abs(L["loss_G"] - (L0["loss_G"] + L["loss_cldice"])) <= 1e-6 * abs(L["loss_G"])
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_cldice_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible: the
    replay's ``loss_cldice`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the caller's
    stream)."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, cldice_weight=0.5)
        Le = eager.step(a, b, sync=True)
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, cldice_weight=0.5)
        gs = fa.GraphedTrainStep(ts, a, b)
        Lg = gs.step(a, b, sync=True)
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    print("CLDICE_ERR graph step: loss_cldice %.9f eager %.9f, loss_G %.9f eager %.9f" % (Lg["loss_cldice"], Le["loss_cldice"], Lg["loss_G"], Le["loss_G"]))
    assert Lg["loss_cldice"] > 0
    assert Lg["loss_cldice"] == Le["loss_cldice"] and Lg["loss_G"] == Le["loss_G"]      # the eager bits
    assert ts.opt_G.step_count == 1
