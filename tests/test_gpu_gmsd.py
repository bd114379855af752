"""GMSD and MS-GMSD (csrc/gmsd.hip) on the MI355X: ``ops.gmsd`` / ``ops.ms_gmsd`` / ``GMSD`` / ``MSGMSD`` against the float64 restatement of
tests/test_gmsd_cpu.py (pinned there to tests/golden/golden_gmsd.npz, whose values come from explicit slice sums): every fixture case,
the null ``db`` path, an upstream gradient per image, the bit-for-bit properties, the degenerate inputs, the launch structure,
``evaluate_pairs_with(gmsd=..., ms_gmsd=...)`` and the opt-in ``TrainStep(gmsd_weight=...)`` term, eager in both schedules and
hipGraph-captured.

Every error is measured against the float64 restatement; the bars are the project's (tests/test_gpu_lncc.py), twice the fp32
reference's own error:

    gradients (relative L2, per array):        e_hip <= 2 e_ref + 2^-23
    score and per-image scores (relative):     e_hip <= 2 E_ref + 1 ulp of the score

e_ref is the fp32 reference's distance from the restatement (the fixture's ``f32`` arrays; off the fixture, the restatement run in
fp32 on the CPU).  A single scalar's e_ref can be small by luck, so E_ref is the LARGEST relative fp32-reference error of the score
over all fixture cases (off the fixture: that, or the case's own fp32 restatement if larger).

The conditioning caps (tests/test_gmsd_cpu.py): every gradient comparison first asserts, on the float64 restatement, min m >= 2^-10,
mean(d^2) / V <= 8 and every score > 0; nothing is excluded.

The kernels' tiles are read out of csrc/gmsd.hip (``kernel_tiles`` of tests/test_gmsd_cpu.py, which also asserts there that the
fixture's seam cases cross them): ``gmsd_index`` 16 x 64 (rows x columns), ``gmsd_grad`` 16 x 32.

Each array prints a ``GMSD_ERR`` line (run with ``-s``; a run's lines are what profiles/gmsd_error.txt holds)."""
import math
import random

import pytest
import torch

from test_gmsd_cpu import CASES, MS_WEIGHTS, case_name, find_pair, fixture_inputs, gold, kernel_tiles, make_pair, rel_l2, restate, restate_case, score_err, well_conditioned

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
WS_ARG = 4                                    # gmsd_index(a, b, next_a, next_b, workspace, ...)
TABLE_ARG = 11                                # gmsd_final(workspace, N, C, H, W, scales, pooled, weights, average, out_image, out_mean, table, stream)
G_ARG, DX_ARG, DY_ARG = 3, 7, 8               # gmsd_grad(a, b, table, g, gN, dca, dcb, da, db, ...)
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


def op(fa, x, y, weights=None, c=0.0026, value_range=(-1., 1.), per_image=False):
    """``ops.gmsd`` (``weights`` None) or ``ops.ms_gmsd``."""
    if weights is None:
        return fa.ops.gmsd(x, y, c, value_range, per_image)
    return fa.ops.ms_gmsd(x, y, weights, c, value_range, per_image)


def run_hip(fa, x, y, weights=None, c=0.0026, value_range=(-1., 1.), per_image=False, x_grad=True, y_grad=True, upstream=None):
    """{"score", "dx", "dy"} of the op on the GPU, back on the host; the gradients are those of ``(score * upstream).sum()``."""
    xd = x.float().cuda().detach().requires_grad_(x_grad)
    yd = y.float().cuda().detach().requires_grad_(y_grad)
    S = op(fa, xd, yd, weights, c, value_range, per_image)
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


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bars of the module docstring on every one."""
    bad = []
    well_conditioned(ref64)                                               # the conditioning caps
    own = score_err(ref32["score"], ref64["score"])
    E_ref = max(score_E_ref(), own)
    e_hip = score_err(got["score"], ref64["score"])
    print("GMSD_ERR %-34s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f min m %.2e ratio d %.3f" % (
        name, "score", E_ref, own, e_hip, e_hip / E_ref, ref64["min_m"], ref64["ratio"]))
    assert tuple(got["score"].shape) == tuple(ref64["score"].shape)
    for s_got, s_ref in zip(got["score"].reshape(-1), ref64["score"].reshape(-1)):
        if not score_err(s_got, s_ref) <= K2 * E_ref + ulp_rel(s_ref):
            bad.append(("score", score_err(s_got, s_ref), E_ref))
    for k in ("dx", "dy"):
        if k not in ref64:
            assert k not in got
            continue
        assert tuple(got[k].shape) == tuple(ref64[k].shape)
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("GMSD_ERR %-34s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K2 * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """The score, dx and dy of every fixture case.  GMSD: (1,1,8,8); (2,1,16,16), the mean over the batch, and the same with y needing no
    gradient (the null ``db``); (2,2,32,48) per image with c = 0.01 and value_range (0, 2); (1,3,16,24), channels pooled; (1,1,37,53),
    odd sides: a dropped row and column; (2,1,40,136), a seam per axis of both kernels.  MS-GMSD: (2,1,32,48), (1,1,37,53),
    (2,1,40,136) at the four default weights and (1,1,16,16) at M = 2 with weights (0.3, 0.7)."""
    cid, shape, weights, c, vr, per_image, y_grad, _ = case
    g = gold()
    ref64 = restate_case(case)
    ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("score", "dx", "dy") if k in ref64}
    x, y = fixture_inputs(case)
    hold_to_bar("%s %s" % (cid, "x".join(map(str, shape))), ref64, ref32, run_hip(fa, x, y, weights, c, vr, per_image, True, y_grad))


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS[:3]), ids=("gmsd", "ms_gmsd"))
def test_per_image_with_upstream(fa, weights):
    """Per-image scores of an odd-sided pair with an upstream gradient per image, read on the device; off the fixture."""
    x, y = find_pair((2, 1, 11, 19), weights)
    up = torch.tensor([0.25, -1.5])
    ref64 = restate(x, y, weights, per_image=True, upstream=up)
    ref32 = restate(x, y, weights, per_image=True, upstream=up, dtype=torch.float32)
    hold_to_bar("upstream 2x1x11x19 %s" % ("gmsd" if weights is None else "ms_gmsd M=3"), ref64, ref32,
                run_hip(fa, x, y, weights, per_image=True, upstream=up))


# ------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, y, weights, scale=None, per_image=False):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    S = op(fa, xd, yd, weights, per_image=per_image)
    (S.sum() if scale is None else (S * scale).sum()).backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_for_bit_properties(fa, shape, weights):
    """Swapping the images leaves the score's bits and swaps the gradients; halving the upstream gradient halves both gradients; an
    image alone scores what it scores in a batch."""
    x, y = (t.cuda() for t in make_pair(shape, 5))
    Sxy, dx, dy = grads(fa, x, y, weights)
    Syx, ex, ey = grads(fa, y, x, weights)
    assert torch.equal(Sxy, Syx)                                          # bit for bit
    assert torch.equal(dx, ey) and torch.equal(dy, ex)
    assert 0 < float(Sxy) < 1 and dx.abs().max() > 0 and dy.abs().max() > 0
    _, hx, hy = grads(fa, x, y, weights, scale=0.5)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hy, 0.5 * dy)         # the upstream gradient, applied on the device
    rows, rdx, rdy = grads(fa, x, y, weights, per_image=True)
    for n in range(shape[0]):
        alone, adx, ady = grads(fa, x[n:n + 1], y[n:n + 1], weights, per_image=True)
        assert torch.equal(alone[0], rows[n]) and torch.equal(adx[0], rdx[n]) and torch.equal(ady[0], rdy[n])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ms_gmsd_with_weights_0_1_is_gmsd_bit_for_bit(fa, shape):
    """``ops.ms_gmsd(x, y, weights=(0, 1))`` stores the pooled pair in fp32 and ``ops.gmsd`` stages it on the fly; both form the 2 x 2 mean
    of the mapped samples as ((t00 + t01) + (t10 + t11)) * 0.25 (``gm_mean4`` of csrc/gmsd.hip), the scale of weight 0 adds nothing to
    the score, and its backward launch only applies the adjoint of the pooling: the score and both gradients agree bit for bit."""
    x, y = (t.cuda() for t in make_pair(shape, 4))
    S, dx, dy = grads(fa, x, y, None, per_image=True)
    T, ex, ey = grads(fa, x, y, (0, 1), per_image=True)
    assert torch.equal(S, T) and torch.equal(dx, ex) and torch.equal(dy, ey)
    assert float(S.min()) > 0 and dx.abs().max() > 0


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
def test_bit_reproducible_and_on_a_side_stream(fa, weights):
    x, y = make_pair((2, 1, 64, 192), 6)
    first, again = run_hip(fa, x, y, weights), run_hip(fa, x, y, weights)
    assert all(torch.equal(first[k], again[k]) for k in first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_hip(fa, x, y, weights)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(first[k], side[k]) for k in first)


# ------------------------------------------------------------------------------------------------------------------------
# degenerate inputs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
def test_identical_images_score_zero_with_zero_gradients(fa, weights):
    x, _ = make_pair((2, 2, 40, 72), 7)
    got = run_hip(fa, x, x.clone(), weights, per_image=True)
    assert float(got["score"].abs().max()) == 0.0
    for k in ("dx", "dy"):
        assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) == 0.0


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
@pytest.mark.parametrize("level", (-1.0, 0.3))
def test_constant_image_against_a_textured_one(fa, weights, level):
    """A constant image has m == 0 wherever its window lies inside the image (at ``lo`` = -1, which maps to 0, everywhere): its direction
    there is taken as (0, 0), and every gradient is finite.  The score is the restatement's."""
    x, _ = make_pair((1, 2, 37, 53), 8)
    flat = torch.full_like(x, level)
    got = run_hip(fa, flat, x, weights)
    ref = restate(flat, x, weights, x_grad=False, y_grad=False)
    assert float(ref["score"]) > 0 and ref["min_m"] == 0.0
    assert score_err(got["score"], ref["score"]) <= 1e-5
    assert torch.isfinite(got["dx"]).all() and torch.isfinite(got["dy"]).all() and got["dy"].abs().max() > 0
    if level == -1.0:
        assert float(got["dx"].abs().max()) == 0.0                       # no direction anywhere


def test_degenerate_shapes(fa):
    """(1, 1, 2, 2) under GMSD pools to one position: the score is 0 and so are the gradients.  (1, 1, 8, 8) at M = 4 reaches a 1 x 1
    scale, which adds nothing: the score is that of the first three scales."""
    x, y = make_pair((1, 1, 2, 2), 0)
    got = run_hip(fa, x, y)
    assert float(got["score"]) == 0.0 and float(got["dx"].abs().max()) == 0.0 and float(got["dy"].abs().max()) == 0.0
    x, y = make_pair((1, 1, 8, 8), 0)
    full, three = run_hip(fa, x, y, MS_WEIGHTS), run_hip(fa, x, y, MS_WEIGHTS[:3])
    assert float(full["score"]) > 0 and all(torch.equal(full[k], three[k]) for k in full)


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS, (0.0, 0.5, 0.5)), ids=("gmsd", "ms_gmsd", "ms_gmsd_w0"))
def test_launch_counts(fa, monkeypatch, weights):
    """GMSD: two entry points forward (``gmsd_index``, ``gmsd_final``), one backward.  MS-GMSD: M + 1 forward, M backward; a scale of weight
    0 takes a null workspace.  The da / db pointer is null for the input that needs no gradient."""
    M = 1 if weights is None else len(weights)
    x, y = (t.cuda() for t in make_pair((2, 2, 32, 48), 3))
    for x_grad, y_grad in ((True, True), (True, False), (False, True)):
        xd, yd = x.clone().requires_grad_(x_grad), y.clone().requires_grad_(y_grad)
        calls = spy(fa, monkeypatch)
        S = op(fa, xd, yd, weights)
        assert [n for n, _ in calls] == ["gmsd_index"] * M + ["gmsd_final"] and calls[-1][1][TABLE_ARG]
        assert [bool(a[WS_ARG]) for _, a in calls[:M]] == [w > 0 for w in (weights or (1.0,))]
        del calls[:]
        S.backward()
        assert [n for n, _ in calls] == ["gmsd_grad"] * M
        for _, a in calls:
            assert bool(a[DX_ARG]) == x_grad and bool(a[DY_ARG]) == y_grad and a[G_ARG]
        assert (xd.grad is not None) == x_grad and (yd.grad is not None) == y_grad
        monkeypatch.undo()


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
def test_one_sided_gradient_is_the_two_sided_one(fa, weights):
    """A null ``da`` / ``db`` skips that side's maps, gathers and stores in ``gmsd_grad``; the side that is asked for keeps its bits.
    (2, 1, 40, 72): several tiles and a remainder."""
    x, y = make_pair((2, 1, 40, 72), 8)
    both = run_hip(fa, x, y, weights)
    only_x, only_y = run_hip(fa, x, y, weights, y_grad=False), run_hip(fa, x, y, weights, x_grad=False)
    assert "dy" not in only_x and "dx" not in only_y
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_y["dy"], both["dy"]) and both["dx"].abs().max() > 0
    assert torch.equal(only_x["score"], both["score"]) and torch.equal(only_y["score"], both["score"])


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch, weights):
    M = 1 if weights is None else len(weights)
    N, C, H, W = 2, 3, 32, 48
    x, y = (t.cuda() for t in make_pair((N, C, H, W), 2))
    calls = spy(fa, monkeypatch)
    Sg = op(fa, x.clone().requires_grad_(True), y.clone().requires_grad_(True), weights)
    assert calls[-1][0] == "gmsd_final" and calls[-1][1][TABLE_ARG]
    saved = Sg.grad_fn.saved_tensors
    # the table, the two images and the pooled pairs of scales 2..M only
    assert [tuple(t.shape) for t in saved] == [(2, M, N)] + [(N, C, H >> j, W >> j) for j in range(M) for _ in range(2)]
    del calls[:]
    with torch.no_grad():
        Sn = op(fa, x.clone().requires_grad_(True), y.clone().requires_grad_(True), weights)
    assert len(calls) == M + 1 and calls[-1][1][TABLE_ARG] is None         # a null table pointer
    assert not Sn.requires_grad and Sn.grad_fn is None
    del calls[:]
    Sp = op(fa, x, y, weights)                                             # inputs that need no gradient
    assert len(calls) == M + 1 and calls[-1][1][TABLE_ARG] is None and not Sp.requires_grad
    assert torch.equal(Sn, Sg) and torch.equal(Sp, Sg)


def test_module_and_function_are_the_op(fa):
    x, y = (t.cuda() for t in make_pair((2, 1, 32, 48), 4))
    big = torch.cat((x, x), dim=3)
    vx, vy = big[:, :, :, 48:], torch.cat((y, y), dim=3)[:, :, :, 48:]      # views equal their contiguous copies
    assert not vx.is_contiguous()
    want, rows = fa.ops.gmsd(x, y, 0.01, (0., 2.)), fa.ops.gmsd(x, y, 0.01, (0., 2.), True)
    mod = fa.GMSD(c=0.01, value_range=(0, 2)).cuda()
    assert torch.equal(mod(x, y), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(fa.GMSD(0.01, (0, 2), size_average=False)(x, y), rows)
    assert torch.equal(fa.ssim.gmsd(x, y, 0.01, (0., 2.)), want)
    assert torch.equal(fa.ssim.gmsd(x, y, 0.01, (0., 2.), size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    assert torch.equal(mod(vx, vy), want)
    want, rows = fa.ops.ms_gmsd(x, y, (0.3, 0.7), 0.01, (0., 2.)), fa.ops.ms_gmsd(x, y, (0.3, 0.7), 0.01, (0., 2.), True)
    mod = fa.MSGMSD(weights=(0.3, 0.7), c=0.01, value_range=(0, 2)).cuda()
    assert torch.equal(mod(x, y), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(fa.MSGMSD((0.3, 0.7), 0.01, (0, 2), size_average=False)(x, y), rows)
    assert torch.equal(fa.ssim.ms_gmsd(x, y, (0.3, 0.7), 0.01, (0., 2.)), want)
    assert torch.equal(fa.ssim.ms_gmsd(x, y, (0.3, 0.7), 0.01, (0., 2.), size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    assert torch.equal(mod(vx, vy), want)
    assert torch.equal(fa.MSGMSD().cuda()(x, y), fa.ops.ms_gmsd(x, y))


@pytest.mark.parametrize("weights", (None, MS_WEIGHTS), ids=("gmsd", "ms_gmsd"))
def test_capturable(fa, weights):
    """Forward and backward captured in one hipGraph replay to the eager bits: nothing is allocated or read on the host."""
    x, y = (t.cuda() for t in make_pair((2, 1, 40, 72), 9))
    eager = run_hip(fa, x.cpu(), y.cpu(), weights)
    xs = x.clone().requires_grad_(True)
    op(fa, xs, y, weights).backward()                                      # warm-up: the workspace exists before the capture
    xs.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        S = op(fa, xs, y, weights)
        (dx,) = torch.autograd.grad(S, xs)
    S.detach().zero_()
    dx.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(S.detach().cpu(), eager["score"]) and torch.equal(dx.cpu(), eager["dx"])


# ------------------------------------------------------------------------------------------------------------------------
# the evaluation path
# ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pairs_with_keys(fa, monkeypatch):
    """The keys are the means of the per-image indices of (super_resolve(lr), hr), against the restatement on two 32 x 32 pairs.  The
    generator's forward is not bit-reproducible (split-K atomics), so ``super_resolve`` is replaced by a fixed map; the four metric
    columns and the indices run their kernels."""
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: (0.9 * lr).contiguous())
    pairs = []
    for seed, n in ((21, 2), (22, 1)):
        lr, hr = make_pair((n, 1, 32, 32), seed)
        pairs.append((lr.cuda(), hr.cuda()))
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs_with(None, pairs, gmsd=fa.GMSD().cuda(), ms_gmsd=fa.MSGMSD().cuda())
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "gmsd", "ms_gmsd"] and all(out[k] == plain[k] for k in plain)
    for key, weights in (("gmsd", None), ("ms_gmsd", MS_WEIGHTS)):
        def rows_of(dtype):
            return [restate((0.9 * lr).cpu(), hr.cpu(), weights, per_image=True, x_grad=False, y_grad=False, dtype=dtype)["score"] for lr, hr in pairs]
        rows, rows32 = torch.cat(rows_of(torch.float64)), torch.cat(rows_of(torch.float32))
        E_ref = max(score_E_ref(), score_err(rows32, rows))
        want = float(rows.mean())
        print("GMSD_ERR evaluate_pairs_with: %s %.9f restatement %.9f E_ref %.3e" % (key, out[key], want, E_ref))
        assert rows.shape == (3,) and 0 < want < 1 and abs(out[key] - want) <= (K2 * E_ref + ulp_rel(want)) * want


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


@pytest.mark.parametrize("two_chains,multiscale", [(True, False), (False, False), (True, True)])
def test_train_step_gmsd_term(fa, O, two_chains, multiscale, monkeypatch):
    """192^2, batch 1, the smallest step of tests/test_gpu_step.py.  With ``reproducible_forward`` the forward and the losses are
    bit-reproducible, so against the weight-0 step: the tensors and every other loss keep their bits; ``loss_gmsd`` is the composition
    of the op on the step's own tensors -- 0.5 (G(recovered_A, real_A) + G(recovered_B, real_B)), formed in double from the op's fp32
    scores; the step forms it in fp32, in the two-chain schedule as two halves: 4 roundings of 2^-24 relative, hence 1e-6 relative --
    and ``loss_G`` is the weight-0 step's plus the term, to fp32 rounding of the sum (1e-6 relative).  The weight-0 step launches no
    ``gmsd_*`` entry and the step with the term launches exactly two forwards and two one-sided backwards more; every other entry
    point keeps its count.  Both places the term lives: the two-chain schedule and the single-stream ``generator_loss``."""
    M = 4 if multiscale else 1
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    calls = spy(fa, monkeypatch)
    try:
        tsd = fresh_step(fa, O, reproducible_forward=True)                 # the default step, first: it fills the process-wide tables
        Ld = tsd.step(a, b, sync=True, keep=True)
        ts = fresh_step(fa, O, reproducible_forward=True, gmsd_weight=0.5, gmsd_multiscale=multiscale)
        del calls[:]
        L = ts.step(a, b, sync=True, keep=True)
        with_term = counted(calls)
        grad_calls = [args for n, args in calls if n == "gmsd_grad"]
        ts0 = fresh_step(fa, O, reproducible_forward=True, gmsd_weight=0.0, gmsd_multiscale=multiscale)
        del calls[:]
        L0 = ts0.step(a, b, sync=True, keep=True)
        without = counted(calls)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_gmsd" not in L0 and ts0.gmsd is None and tsd.gmsd is None and isinstance(ts.gmsd, fa.MSGMSD if multiscale else fa.GMSD)
    assert L0["loss_G"] == Ld["loss_G"]                                    # weight 0 is the default step, bit for bit
    assert not [n for n in without if n.startswith("gmsd")]
    assert {n: c for n, c in with_term.items() if n.startswith("gmsd")} == {"gmsd_index": 2 * M, "gmsd_final": 2, "gmsd_grad": 2 * M}
    assert {n: c for n, c in with_term.items() if not n.startswith("gmsd")} == without
    assert all(bool(g[DX_ARG]) and not g[DY_ARG] for g in grad_calls)      # the gradient reaches the reconstruction only
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    with torch.no_grad():
        want = 0.5 * sum(float(ts.gmsd(rec, real)) for rec, real in ((T["recovered_A"], a), (T["recovered_B"], b)))
    print("GMSD_ERR step two_chains=%s multiscale=%s: loss_gmsd %.7f composition %.7f, loss_G %.6f against %.6f at weight 0" % (
        two_chains, multiscale, L["loss_gmsd"], want, L["loss_G"], L0["loss_G"]))
    assert want > 0 and abs(L["loss_gmsd"] - want) <= 1e-6 * abs(want)
    assert abs(L["loss_G"] - (L0["loss_G"] + L["loss_gmsd"])) <= 1e-6 * abs(L["loss_G"])
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_gmsd_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible: the
    replay's ``loss_gmsd`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the
    caller's stream)."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, gmsd_weight=0.5)
        Le = eager.step(a, b, sync=True)
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, gmsd_weight=0.5)
        gs = fa.GraphedTrainStep(ts, a, b)
        Lg = gs.step(a, b, sync=True)
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    print("GMSD_ERR graph step: loss_gmsd %.9f eager %.9f, loss_G %.9f eager %.9f" % (
        Lg["loss_gmsd"], Le["loss_gmsd"], Lg["loss_G"], Le["loss_G"]))
    assert Lg["loss_gmsd"] > 0
    assert Lg["loss_gmsd"] == Le["loss_gmsd"] and Lg["loss_G"] == Le["loss_G"]      # the eager bits
    assert ts.opt_G.step_count == 1
