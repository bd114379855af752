"""The Hessian vesselness filter and the vessel Dice index (csrc/vessel.hip) on the MI355X: ``ops.vesselness`` / ``ops.vessel_dice`` /
``Vesselness`` / ``VesselDice`` against the float64 restatement of tests/test_vessel_cpu.py (pinned there to
tests/golden/golden_vessel.npz, whose values come from explicit slice sums): every fixture case, an off-fixture per-image pair with
an upstream gradient, the exact properties, the structure of the launches, degenerate inputs, ``evaluate_pairs_with(vessel_dice=...)``
and the opt-in ``TrainStep(vessel_weight=...)`` term, eager in both schedules and as a captured graph.

The bars.  With ``e_ref`` the distance of the fp32 reference (the fixture's ``f32`` arrays; off the fixture the restatement run in
fp32) from float64 and ``E_ref`` the largest relative score error of the fp32 reference over the fixture (and the case at hand):

    gradients and maps, relative L2 per array:   e_hip <= 2 e_ref + 2^-23
    scores, relative:                            e_hip <= 2 E_ref + 1 ulp

Both are measured against the reference; nothing is fixed in advance.

The conditioning caps (tests/test_vessel_cpu.py): every gradient comparison first asserts, on the float64 restatement, min r >= 2^-14,
D >= 2^-6 and every score > 0.  The kernels' tiles are read out of csrc/vessel.hip (``kernel_tiles`` of tests/test_vessel_cpu.py, which
also asserts there that the seam case crosses them): ``vessel_index`` 16 x 64 (rows x columns), ``vessel_grad`` 16 x 32.

Each array prints a ``VESSEL_ERR`` line (run with ``-s``; a run's lines are what profiles/vessel_error.txt holds)."""
import math
import random

import pytest
import torch

from test_vessel_cpu import (CASES, DEFAULT, case_name, find_pair, fixture_inputs, gold, make_pair, rel_l2, restate, restate_case, restate_map,
                             score_err, well_conditioned)

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
MAPX_ARG, MAPY_ARG, WS_ARG = 2, 3, 4          # vessel_index(x, y, map_x, map_y, workspace, ...)
TABLE_ARG = 9                                 # vessel_final(workspace, N, C, H, W, eps, average, out_image, out_mean, table, stream)
Y_ARG, GTABLE_ARG, G_ARG, DX_ARG, DY_ARG = 1, 4, 5, 7, 8      # vessel_grad(x, y, map_x, map_y, table, g, gN, dx, dy, ...)
BIT_SHAPES = [(2, 2, 40, 72), (1, 3, 37, 53), (2, 1, 18, 130)]


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def settings(cfg):
    return (cfg["sigmas"], cfg["weights"], cfg["beta"], cfg["c"], cfg["eps"], cfg["value_range"], cfg["bright"])


def op(fa, x, y, cfg=DEFAULT, per_image=False):
    return fa.ops.vessel_dice(x, y, *settings(cfg), per_image)


def filt(fa, x, cfg=DEFAULT):
    return fa.ops.vesselness(x, cfg["sigmas"], cfg["weights"], cfg["beta"], cfg["c"], cfg["value_range"], cfg["bright"])


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


def run_hip_map(fa, x, cot, cfg=DEFAULT):
    xd = x.float().cuda().detach().requires_grad_(True)
    A = filt(fa, xd, cfg)
    assert A.dtype == torch.float32 and A.shape == x.shape
    (A * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    return {"map": A.detach().cpu(), "dx": xd.grad.cpu()}


def ulp_rel(v):
    v = abs(float(v))
    return 2.0 ** (math.floor(math.log2(v)) - 23) / v


_E = []


def score_E_ref():
    """The largest relative error of the fp32 reference's score over all fixture cases."""
    if not _E:
        g = gold()
        _E.append(max(score_err(g[c[0] + "/f32/score"], restate_case(c)["score"]) for c in CASES if not c[6]))
    return _E[0]


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bars of the module docstring on every one."""
    bad = []
    well_conditioned(ref64)                                               # the conditioning caps
    if "score" in ref64:
        own = score_err(ref32["score"], ref64["score"])
        E_ref = max(score_E_ref(), own)
        e_hip = score_err(got["score"], ref64["score"])
        print("VESSEL_ERR %-34s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f min r %.2e min D %.3f" % (
            name, "score", E_ref, own, e_hip, e_hip / E_ref, ref64["min_r"], ref64["min_D"]))
        assert tuple(got["score"].shape) == tuple(ref64["score"].shape)
        for s_got, s_ref in zip(got["score"].reshape(-1), ref64["score"].reshape(-1)):
            if not score_err(s_got, s_ref) <= K2 * E_ref + ulp_rel(s_ref):
                bad.append(("score", score_err(s_got, s_ref), E_ref))
    for k in ("map", "dx", "dy"):
        if k not in ref64:
            assert k not in got
            continue
        assert tuple(got[k].shape) == tuple(ref64[k].shape)
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("VESSEL_ERR %-34s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K2 * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """Every fixture case.  The index: (1,1,8,8); (2,1,16,16), the mean over the batch, and the same with y needing no gradient (the null
    ``dy``); (2,2,32,48) per image with sigma 1.5, beta 0.7, c 0.05 and value_range (0, 2); (1,3,16,24), channels pooled; (1,1,37,53), odd
    sides; (2,1,40,136), two seams per axis of both kernels' tiles; (1,1,5,7) with sigmas (0.5, 3): a halo of 9 round a 5 x 7 image.
    The filter with a random upstream map: (1,1,37,53) bright and (1,2,18,70) dark."""
    cid, shape, cfg, per_image, y_grad, _, is_map = case
    g = gold()
    ref64 = restate_case(case)
    x, y, cot = fixture_inputs(case)
    name = "%s %s" % (cid, "x".join(map(str, shape)))
    if is_map:
        ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("map", "dx")}
        hold_to_bar(name, ref64, ref32, run_hip_map(fa, x, cot, cfg))
    else:
        ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("score", "dx", "dy") if k in ref64}
        hold_to_bar(name, ref64, ref32, run_hip(fa, x, y, cfg, per_image, True, y_grad))


def test_per_image_with_upstream(fa):
    """Per-image scores of an odd-sided pair with an upstream gradient per image, read on the device; off the fixture."""
    x, y = find_pair((2, 1, 11, 19))
    up = torch.tensor([0.25, -1.5])
    ref64 = restate(x, y, per_image=True, upstream=up)
    ref32 = restate(x, y, per_image=True, upstream=up, dtype=torch.float32)
    hold_to_bar("upstream 2x1x11x19", ref64, ref32, run_hip(fa, x, y, per_image=True, upstream=up))


# ------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, y, cfg=DEFAULT, scale=None, per_image=False):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    S = op(fa, xd, yd, cfg, per_image)
    (S.sum() if scale is None else (S * scale).sum()).backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_for_bit_properties(fa, shape):
    """Swapping the images leaves the score's bits and swaps the gradients; halving the upstream gradient halves both gradients; two
    runs agree; an image alone scores what it scores in a batch."""
    x, y = (t.cuda() for t in make_pair(shape, 5))
    Sxy, dx, dy = grads(fa, x, y)
    Syx, ex, ey = grads(fa, y, x)
    assert torch.equal(Sxy, Syx)                                          # bit for bit
    assert torch.equal(dx, ey) and torch.equal(dy, ex)
    assert 0 < float(Sxy) < 1 and dx.abs().max() > 0 and dy.abs().max() > 0
    _, hx, hy = grads(fa, x, y, scale=0.5)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hy, 0.5 * dy)         # the upstream gradient, applied on the device
    again = grads(fa, x, y)
    assert torch.equal(again[0], Sxy) and torch.equal(again[1], dx) and torch.equal(again[2], dy)
    rows, rdx, rdy = grads(fa, x, y, per_image=True)
    for n in range(shape[0]):
        alone, adx, ady = grads(fa, x[n:n + 1], y[n:n + 1], per_image=True)
        assert torch.equal(alone[0], rows[n]) and torch.equal(adx[0], rdx[n]) and torch.equal(ady[0], rdy[n])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identical_images_score_one_with_zero_gradients(fa, shape):
    x, _ = make_pair(shape, 7)
    got = run_hip(fa, x, x.clone(), per_image=True)
    assert got["score"].tolist() == [1.0] * shape[0]
    for k in ("dx", "dy"):
        assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) == 0.0


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_scale_of_weight_zero_is_dropped_bit_for_bit(fa, shape):
    x, y = (t.cuda() for t in make_pair(shape, 4))
    S, dx, dy = grads(fa, x, y, dict(DEFAULT, sigmas=(1.0,)), per_image=True)
    T, ex, ey = grads(fa, x, y, dict(DEFAULT, sigmas=(1.0, 2.0), weights=(1.0, 0.0)), per_image=True)
    assert torch.equal(S, T) and torch.equal(dx, ex) and torch.equal(dy, ey)
    assert float(S.min()) > 0 and dx.abs().max() > 0


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dark_ridges_are_the_bright_ridges_of_the_negated_image(fa, shape):
    """With value_range (0, 1) the mapped image of -x is -u exactly, a, b, d are negated exactly, and ``bright=False`` negates them back."""
    x, _ = make_pair(shape, 3)
    x = x.cuda()
    dark = filt(fa, x, dict(DEFAULT, value_range=(0.0, 1.0), bright=False))
    bright = filt(fa, -x, dict(DEFAULT, value_range=(0.0, 1.0), bright=True))
    assert torch.equal(dark, bright) and float(dark.max()) > 0


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_filters_map_reproduces_the_index(fa, shape):
    """``ops.vesselness`` of either image, put through the Dice formula in double, is ``ops.vessel_dice``'s score within the score bar: both
    forms of ``vessel_index`` share one tile body."""
    x, y = (t.cuda() for t in make_pair(shape, 2))
    with torch.no_grad():
        A, B = filt(fa, x).double(), filt(fa, y).double()
        S = op(fa, x, y, per_image=True)
    D = (A * A).mean(dim=(1, 2, 3)) + (B * B).mean(dim=(1, 2, 3)) + DEFAULT["eps"]
    want = (2 * (A * B).mean(dim=(1, 2, 3)) + DEFAULT["eps"]) / D
    for s_got, s_ref in zip(S.cpu(), want.cpu()):
        assert score_err(s_got, s_ref) <= K2 * score_E_ref() + ulp_rel(s_ref), (float(s_got), float(s_ref))


def test_bit_reproducible_on_a_side_stream(fa):
    x, y = make_pair((2, 1, 64, 192), 6)
    first = run_hip(fa, x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_hip(fa, x, y)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(first[k], side[k]) for k in first)


# ------------------------------------------------------------------------------------------------------------------------
# degenerate inputs
# ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs_give_finite_results(fa):
    """1 x 1 images; two images at ``lo`` (vessel-free: S = 1, zero gradients); a constant image, r == 0 wherever its window lies inside,
    against a textured one."""
    x, y = make_pair((2, 1, 1, 1), 0)
    got = run_hip(fa, x, y, per_image=True)
    assert all(torch.isfinite(got[k]).all() for k in got) and float(got["score"].min()) > 0 and float(got["score"].max()) <= 1
    lo = torch.full((2, 1, 20, 70), -1.0)
    got = run_hip(fa, lo, lo.clone(), per_image=True)
    assert got["score"].tolist() == [1.0, 1.0] and float(got["dx"].abs().max()) == 0.0 and float(got["dy"].abs().max()) == 0.0
    x, _ = make_pair((1, 2, 37, 53), 8)
    for level in (-1.0, 0.3):
        flat = torch.full_like(x, level)
        got = run_hip(fa, flat, x)
        ref = restate(flat, x, x_grad=False, y_grad=False)
        assert all(torch.isfinite(got[k]).all() for k in got) and got["dy"].abs().max() > 0
        assert score_err(got["score"], ref["score"]) <= 1e-5
        A = filt(fa, flat.cuda())
        assert torch.isfinite(A).all()


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def test_launch_counts(fa, monkeypatch):
    """The index: two entry points forward (``vessel_index``, ``vessel_final``), one backward, whatever the number of scales.  The filter: one
    forward, one backward.  The dx / dy pointer is null for the input that needs no gradient."""
    x, y = (t.cuda() for t in make_pair((2, 2, 32, 48), 3))
    for x_grad, y_grad in ((True, True), (True, False), (False, True)):
        xd, yd = x.clone().requires_grad_(x_grad), y.clone().requires_grad_(y_grad)
        calls = spy(fa, monkeypatch)
        S = op(fa, xd, yd)
        assert [n for n, _ in calls] == ["vessel_index", "vessel_final"] and calls[-1][1][TABLE_ARG]
        assert calls[0][1][MAPX_ARG] and calls[0][1][MAPY_ARG] and calls[0][1][WS_ARG]
        del calls[:]
        S.backward()
        assert [n for n, _ in calls] == ["vessel_grad"]
        a = calls[0][1]
        assert bool(a[DX_ARG]) == x_grad and bool(a[DY_ARG]) == y_grad and a[G_ARG] and a[GTABLE_ARG]
        assert (xd.grad is not None) == x_grad and (yd.grad is not None) == y_grad
        monkeypatch.undo()
    calls = spy(fa, monkeypatch)
    xd = x.clone().requires_grad_(True)
    A = filt(fa, xd)
    assert [n for n, _ in calls] == ["vessel_index"] and calls[0][1][Y_ARG] is None and calls[0][1][WS_ARG] is None
    del calls[:]
    A.sum().backward()
    assert [n for n, _ in calls] == ["vessel_grad"] and calls[0][1][GTABLE_ARG] is None and calls[0][1][DY_ARG] is None


def test_one_sided_gradient_is_the_two_sided_one(fa):
    """A null ``dx`` / ``dy`` skips that side's staging, maps, gathers and stores in ``vessel_grad``; the side that is asked for keeps its
    bits.  (2, 1, 40, 72): several tiles and a remainder."""
    x, y = make_pair((2, 1, 40, 72), 8)
    both = run_hip(fa, x, y)
    only_x, only_y = run_hip(fa, x, y, y_grad=False), run_hip(fa, x, y, x_grad=False)
    assert "dy" not in only_x and "dx" not in only_y
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_y["dy"], both["dy"]) and both["dx"].abs().max() > 0
    assert torch.equal(only_x["score"], both["score"]) and torch.equal(only_y["score"], both["score"])


def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch):
    N, C, H, W = 2, 3, 32, 48
    x, y = (t.cuda() for t in make_pair((N, C, H, W), 2))
    calls = spy(fa, monkeypatch)
    Sg = op(fa, x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert calls[-1][0] == "vessel_final" and calls[-1][1][TABLE_ARG]
    # the two images, their two response maps and the table only
    assert [tuple(t.shape) for t in Sg.grad_fn.saved_tensors] == [(N, C, H, W)] * 4 + [(2, N)]
    del calls[:]
    with torch.no_grad():
        Sn = op(fa, x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert [n for n, _ in calls] == ["vessel_index", "vessel_final"]
    assert calls[0][1][MAPX_ARG] is None and calls[0][1][MAPY_ARG] is None and calls[1][1][TABLE_ARG] is None     # null pointers: nothing is kept
    assert not Sn.requires_grad and Sn.grad_fn is None
    del calls[:]
    Sp = op(fa, x, y)                                                      # inputs that need no gradient
    assert len(calls) == 2 and calls[0][1][MAPX_ARG] is None and calls[1][1][TABLE_ARG] is None and not Sp.requires_grad
    assert torch.equal(Sn, Sg) and torch.equal(Sp, Sg)
    del calls[:]
    with torch.no_grad():
        An = filt(fa, x.clone().requires_grad_(True))
    assert [n for n, _ in calls] == ["vessel_index"] and An.grad_fn is None
    assert torch.equal(An, filt(fa, x.clone().requires_grad_(True)))


def test_module_and_function_are_the_op(fa):
    x, y = (t.cuda() for t in make_pair((2, 1, 32, 48), 4))
    big = torch.cat((x, x), dim=3)
    vx, vy = big[:, :, :, 48:], torch.cat((y, y), dim=3)[:, :, :, 48:]      # views equal their contiguous copies
    assert not vx.is_contiguous()
    args = ((1.5, 2.5), (1.0, 3.0), 0.7, 0.05, 1e-5, (0., 2.), True)
    want, rows = fa.ops.vessel_dice(x, y, *args), fa.ops.vessel_dice(x, y, *args, True)
    mod = fa.VesselDice(*args).cuda()
    assert torch.equal(mod(x, y), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(fa.VesselDice(*args, size_average=False)(x, y), rows)
    assert torch.equal(fa.ssim.vessel_dice(x, y, *args), want)
    assert torch.equal(fa.ssim.vessel_dice(x, y, *args, size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    assert torch.equal(mod(vx, vy), want)
    assert torch.equal(fa.VesselDice().cuda()(x, y), fa.ops.vessel_dice(x, y))
    fargs = args[:4] + args[5:]
    assert torch.equal(fa.Vesselness(*fargs).cuda()(x), fa.ops.vesselness(x, *fargs))
    assert torch.equal(fa.Vesselness(*fargs)(vx), fa.ops.vesselness(x, *fargs))


def test_capturable(fa):
    """Forward and backward captured in one hipGraph replay to the eager bits: nothing is allocated or read on the host."""
    x, y = (t.cuda() for t in make_pair((2, 1, 40, 72), 9))
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


# ------------------------------------------------------------------------------------------------------------------------
# the evaluation path
# ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pairs_with_key(fa, monkeypatch):
    """The key is the mean of the per-image index of (super_resolve(lr), hr), against the restatement on two 32 x 32 pairs.  The
    generator's forward is not bit-reproducible (split-K atomics), so ``super_resolve`` is replaced by a fixed map; the four metric
    columns and the index run their kernels."""
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: (0.9 * lr).contiguous())
    pairs = []
    for seed, n in ((21, 2), (22, 1)):
        lr, hr = make_pair((n, 1, 32, 32), seed)
        pairs.append((lr.cuda(), hr.cuda()))
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs_with(None, pairs, vessel_dice=fa.VesselDice().cuda())
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "vessel_dice"] and all(out[k] == plain[k] for k in plain)

    def rows_of(dtype):
        return [restate((0.9 * lr).cpu(), hr.cpu(), per_image=True, x_grad=False, y_grad=False, dtype=dtype)["score"] for lr, hr in pairs]
    rows, rows32 = torch.cat(rows_of(torch.float64)), torch.cat(rows_of(torch.float32))
    E_ref = max(score_E_ref(), score_err(rows32, rows))
    want = float(rows.mean())
    print("VESSEL_ERR evaluate_pairs_with: vessel_dice %.9f restatement %.9f E_ref %.3e" % (out["vessel_dice"], want, E_ref))
    assert rows.shape == (3,) and 0 < want < 1 and abs(out["vessel_dice"] - want) <= (K2 * E_ref + ulp_rel(want)) * want


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
def test_train_step_vessel_term(fa, O, two_chains, monkeypatch):
    """192^2, batch 1, the smallest step of tests/test_gpu_step.py.  With ``reproducible_forward`` the forward and the losses are
    bit-reproducible, so against the weight-0 step: the tensors and every other loss keep their bits; ``loss_vessel`` is the composition
    of the op on the step's own tensors -- 0.5 ((1 - S(recovered_A, real_A)) + (1 - S(recovered_B, real_B))), formed in double from the
    op's fp32 scores; the step forms it in fp32, in the two-chain schedule as two halves, and 1 - S cancels: absolute roundings of
    2^-24 on values of order 1, hence 4 * 2^-24 absolute -- and ``loss_G`` is the weight-0 step's plus the term, to fp32 rounding of the
    sum (1e-6 relative).  The weight-0 step launches no ``vessel_*`` entry and the step with the term launches exactly two forwards and
    two one-sided backwards more; every other entry point keeps its count."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    calls = spy(fa, monkeypatch)
    try:
        tsd = fresh_step(fa, O, reproducible_forward=True)                 # the default step, first: it fills the process-wide tables
        Ld = tsd.step(a, b, sync=True, keep=True)
        ts = fresh_step(fa, O, reproducible_forward=True, vessel_weight=0.5)
        del calls[:]
        L = ts.step(a, b, sync=True, keep=True)
        with_term = counted(calls)
        grad_calls = [args for n, args in calls if n == "vessel_grad"]
        ts0 = fresh_step(fa, O, reproducible_forward=True, vessel_weight=0.0)
        del calls[:]
        L0 = ts0.step(a, b, sync=True, keep=True)
        without = counted(calls)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_vessel" not in L0 and ts0.vessel is None and tsd.vessel is None and isinstance(ts.vessel, fa.VesselDice)
    assert L0["loss_G"] == Ld["loss_G"]                                    # weight 0 is the default step, bit for bit
    assert not [n for n in without if n.startswith("vessel")]
    assert {n: c for n, c in with_term.items() if n.startswith("vessel")} == {"vessel_index": 2, "vessel_final": 2, "vessel_grad": 2}
    assert {n: c for n, c in with_term.items() if not n.startswith("vessel")} == without
    assert all(bool(g[DX_ARG]) and not g[DY_ARG] for g in grad_calls)      # the gradient reaches the reconstruction only
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    with torch.no_grad():
        want = 0.5 * sum(1.0 - float(ts.vessel(rec, real)) for rec, real in ((T["recovered_A"], a), (T["recovered_B"], b)))
    print("VESSEL_ERR step two_chains=%s: loss_vessel %.7f composition %.7f, loss_G %.6f against %.6f at weight 0" % (
        two_chains, L["loss_vessel"], want, L["loss_G"], L0["loss_G"]))
    assert want > 0 and abs(L["loss_vessel"] - want) <= 4 * 2.0 ** -24
    assert abs(L["loss_G"] - (L0["loss_G"] + L["loss_vessel"])) <= 1e-6 * abs(L["loss_G"])
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_vessel_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible: the
    replay's ``loss_vessel`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the
    caller's stream)."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, vessel_weight=0.5)
        Le = eager.step(a, b, sync=True)
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, vessel_weight=0.5)
        gs = fa.GraphedTrainStep(ts, a, b)
        Lg = gs.step(a, b, sync=True)
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    print("VESSEL_ERR graph step: loss_vessel %.9f eager %.9f, loss_G %.9f eager %.9f" % (
        Lg["loss_vessel"], Le["loss_vessel"], Lg["loss_G"], Le["loss_G"]))
    assert Lg["loss_vessel"] > 0
    assert Lg["loss_vessel"] == Le["loss_vessel"] and Lg["loss_G"] == Le["loss_G"]      # the eager bits
    assert ts.opt_G.step_count == 1
