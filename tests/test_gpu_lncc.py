"""Local normalised cross-correlation (csrc/lncc.hip) on the MI355X: ``ops.lncc`` / ``LNCC`` / ``ssim.lncc`` against the float64 restatement
of tests/test_lncc_cpu.py (pinned there to tests/golden/golden_lncc.npz, whose values come from explicit slice sums): the smallest
window, a window larger than the image, odd sides, tile seams at win 9 and 15, pooled channels, the null ``db`` path, the bit-for-bit
properties, the launch structure, ``evaluate_pairs_with(lncc=...)`` and the opt-in ``TrainStep(lncc_weight=...)`` term, eager in both
schedules and hipGraph-captured.

Every error is measured against the float64 restatement; the bars are the project's (tests/test_gpu_haarpsi.py), twice the fp32
reference's own error:

    gradients (relative L2, per array):        e_hip <= 2 e_ref + 2^-23
    score and per-image scores (relative):     e_hip <= 2 E_ref + 1 ulp of the score

e_ref is the fp32 reference's distance from the restatement (the fixture's ``f32`` arrays; off the fixture, the restatement run in
fp32 on the CPU).  A single scalar's e_ref can be small by luck, so E_ref is the LARGEST relative fp32-reference error of the score
over all fixture cases (off the fixture: that, or the case's own fp32 restatement if larger).

The conditioning cap (tests/test_lncc_cpu.py): every gradient comparison first asserts, on the float64 restatement,
min_p min(va / Saa, vb / Sbb) >= 2^-4; nothing is excluded.

The kernels' tiles are read out of csrc/lncc.hip (``kernel_tiles`` of tests/test_lncc_cpu.py, which also asserts there that the
fixture's seam cases cross them): ``lncc_index`` 16 x 32 (rows x columns), ``lncc_grad`` 16 x 16.

Each array prints an ``LNCC_ERR`` line (run with ``-s``; a run's lines are what profiles/lncc_error.txt holds)."""
import math
import random

import pytest
import torch

from test_lncc_cpu import CASES, case_name, find_pair, fixture_inputs, gold, kernel_tiles, make_pair, rel_l2, restate, restate_case, score_err, well_conditioned

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
FAC_ARG = 8                                   # lncc_final(workspace, N, C, H, W, average, out_image, out_mean, fac, stream)
G_ARG, DX_ARG, DY_ARG = 3, 5, 6               # lncc_grad(a, b, fac, g, gN, da, db, ...)


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def run_hip(fa, x, y, win=9, eps=1e-5, per_image=False, x_grad=True, y_grad=True, upstream=None):
    """{"score", "dx", "dy"} of ``ops.lncc`` on the GPU, back on the host; the gradients are those of ``(score * upstream).sum()``."""
    xd = x.float().cuda().detach().requires_grad_(x_grad)
    yd = y.float().cuda().detach().requires_grad_(y_grad)
    S = fa.ops.lncc(xd, yd, win, eps, per_image)
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
    well_conditioned(ref64)                                               # the conditioning cap
    own = score_err(ref32["score"], ref64["score"])
    E_ref = max(score_E_ref(), own)
    e_hip = score_err(got["score"], ref64["score"])
    print("LNCC_ERR %-32s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f cap %.3f" % (
        name, "score", E_ref, own, e_hip, e_hip / E_ref, ref64["cap"]))
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
        print("LNCC_ERR %-32s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K2 * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """The score, dx and dy of every fixture case: (1,1,5,7) at win 3, the smallest window, and at win 15, the window larger than the
    image on both axes; (2,1,16,16), the mean over the batch, and the same with y needing no gradient (the null ``db``); (2,2,32,48) per
    image with win 7 and eps 1e-3; (1,3,16,24), channels pooled; (1,1,37,53), odd sides; (2,1,20,36) at win 9 and (1,1,36,40) at win 15,
    a seam per axis of both kernels."""
    cid, shape, win, eps, per_image, y_grad, _ = case
    g = gold()
    ref64 = restate_case(case)
    ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("score", "dx", "dy") if k in ref64}
    x, y = fixture_inputs(case)
    hold_to_bar("%s %s win %d" % (cid, "x".join(map(str, shape)), win), ref64, ref32, run_hip(fa, x, y, win, eps, per_image, True, y_grad))


def test_per_image_with_upstream(fa):
    """Per-image scores of an odd-sided pair with an upstream gradient per image, read on the device; off the fixture."""
    x, y = find_pair((2, 1, 11, 19), win=5)
    up = torch.tensor([0.25, -1.5])
    ref64 = restate(x, y, 5, per_image=True, upstream=up)
    ref32 = restate(x, y, 5, per_image=True, upstream=up, dtype=torch.float32)
    hold_to_bar("upstream 2x1x11x19 win 5", ref64, ref32, run_hip(fa, x, y, 5, per_image=True, upstream=up))


# ------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, y, scale=None, per_image=False, **kw):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    S = fa.ops.lncc(xd, yd, per_image=per_image, **kw)
    (S.sum() if scale is None else (S * scale).sum()).backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize("shape,win", [((2, 2, 40, 72), 9), ((1, 3, 37, 53), 15), ((2, 1, 18, 130), 3)])
def test_bit_for_bit_properties(fa, shape, win):
    """Swapping the images leaves the score's bits and swaps the gradients; halving the upstream gradient halves both gradients; an
    image alone scores what it scores in a batch."""
    x, y = (t.cuda() for t in make_pair(shape, 5))
    Sxy, dx, dy = grads(fa, x, y, win=win)
    Syx, ex, ey = grads(fa, y, x, win=win)
    assert torch.equal(Sxy, Syx)                                          # bit for bit
    assert torch.equal(dx, ey) and torch.equal(dy, ex)
    assert 0 < float(Sxy) < 1 and dx.abs().max() > 0 and dy.abs().max() > 0
    _, hx, hy = grads(fa, x, y, scale=0.5, win=win)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hy, 0.5 * dy)         # the upstream gradient, applied on the device
    rows, rdx, rdy = grads(fa, x, y, per_image=True, win=win)
    for n in range(shape[0]):
        alone, adx, ady = grads(fa, x[n:n + 1], y[n:n + 1], per_image=True, win=win)
        assert torch.equal(alone[0], rows[n]) and torch.equal(adx[0], rdx[n]) and torch.equal(ady[0], rdy[n])


def test_bit_reproducible_and_on_a_side_stream(fa):
    x, y = make_pair((2, 1, 64, 192), 6)
    first, again = run_hip(fa, x, y), run_hip(fa, x, y)
    assert all(torch.equal(first[k], again[k]) for k in first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_hip(fa, x, y)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(first[k], side[k]) for k in first)


def test_identical_images_score_near_one_inside(fa):
    """cc_p of an image with itself is va^2 / (va^2 + eps): 1 up to eps and the rounding of va."""
    x, _ = make_pair((1, 2, 40, 72), 7)
    got = run_hip(fa, x, x.clone(), x_grad=False, y_grad=False)
    ref = restate(x, x, x_grad=False, y_grad=False)
    assert abs(float(got["score"]) - float(ref["score"])) <= 1e-5 and float(ref["score"]) > 0.99


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def test_launch_counts(fa, monkeypatch):
    """Two entry points forward (``lncc_index``, ``lncc_final``), one backward; the da / db pointer is null for the input that needs no
    gradient."""
    x, y = (t.cuda() for t in make_pair((2, 2, 32, 48), 3))
    for x_grad, y_grad in ((True, True), (True, False), (False, True)):
        xd, yd = x.clone().requires_grad_(x_grad), y.clone().requires_grad_(y_grad)
        calls = spy(fa, monkeypatch)
        S = fa.ops.lncc(xd, yd)
        assert [n for n, _ in calls] == ["lncc_index", "lncc_final"] and calls[-1][1][FAC_ARG]
        del calls[:]
        S.backward()
        assert [n for n, _ in calls] == ["lncc_grad"]
        a = calls[0][1]
        assert bool(a[DX_ARG]) == x_grad and bool(a[DY_ARG]) == y_grad and a[G_ARG]
        assert (xd.grad is not None) == x_grad and (yd.grad is not None) == y_grad
        monkeypatch.undo()


def test_one_sided_gradient_is_the_two_sided_one(fa):
    """A null ``da`` / ``db`` skips that side's maps, sums and stores in ``lncc_grad``; the side that is asked for keeps its bits.
    (2, 1, 40, 72): several tiles and a remainder."""
    x, y = make_pair((2, 1, 40, 72), 8)
    both = run_hip(fa, x, y)
    only_x, only_y = run_hip(fa, x, y, y_grad=False), run_hip(fa, x, y, x_grad=False)
    assert "dy" not in only_x and "dx" not in only_y
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_y["dy"], both["dy"]) and both["dx"].abs().max() > 0
    assert torch.equal(only_x["score"], both["score"]) and torch.equal(only_y["score"], both["score"])


def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch):
    x, y = (t.cuda() for t in make_pair((2, 3, 32, 48), 2))
    calls = spy(fa, monkeypatch)
    Sg = fa.ops.lncc(x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert calls[-1][0] == "lncc_final" and calls[-1][1][FAC_ARG]
    saved = Sg.grad_fn.saved_tensors
    assert len(saved) == 3 and tuple(saved[2].shape) == (2,)               # the two images and the factor table only
    del calls[:]
    with torch.no_grad():
        Sn = fa.ops.lncc(x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert len(calls) == 2 and calls[-1][1][FAC_ARG] is None               # a null table pointer
    assert not Sn.requires_grad and Sn.grad_fn is None
    del calls[:]
    Sp = fa.ops.lncc(x, y)                                                 # inputs that need no gradient
    assert len(calls) == 2 and calls[-1][1][FAC_ARG] is None and not Sp.requires_grad
    assert torch.equal(Sn, Sg) and torch.equal(Sp, Sg)


def test_module_and_function_are_the_op(fa):
    x, y = (t.cuda() for t in make_pair((2, 1, 32, 48), 4))
    want = fa.ops.lncc(x, y, 7, 1e-3)
    rows = fa.ops.lncc(x, y, 7, 1e-3, True)
    mod = fa.LNCC(win=7, eps=1e-3).cuda()
    assert torch.equal(mod(x, y), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(fa.LNCC(7, 1e-3, size_average=False)(x, y), rows)
    assert torch.equal(fa.ssim.lncc(x, y, 7, 1e-3), want)
    assert torch.equal(fa.ssim.lncc(x, y, 7, 1e-3, size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    big = torch.cat((x, x), dim=3)
    vx, vy = big[:, :, :, 48:], torch.cat((y, y), dim=3)[:, :, :, 48:]      # views equal their contiguous copies
    assert not vx.is_contiguous() and torch.equal(mod(vx, vy), want)


def test_capturable(fa):
    """Forward and backward captured in one hipGraph replay to the eager bits: nothing is allocated or read on the host."""
    x, y = (t.cuda() for t in make_pair((2, 1, 40, 72), 9))
    eager = run_hip(fa, x.cpu(), y.cpu())
    xs = x.clone().requires_grad_(True)
    fa.ops.lncc(xs, y).backward()                                          # warm-up: the workspace exists before the capture
    xs.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        S = fa.ops.lncc(xs, y)
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
    mod = fa.LNCC().cuda()
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs_with(None, pairs, lncc=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "lncc"] and all(out[k] == plain[k] for k in plain)
    rows = torch.cat([restate((0.9 * lr).cpu(), hr.cpu(), per_image=True, x_grad=False, y_grad=False)["score"] for lr, hr in pairs])
    E_ref = max(score_E_ref(), max(score_err(restate((0.9 * lr).cpu(), hr.cpu(), per_image=True, x_grad=False, y_grad=False,
                                                     dtype=torch.float32)["score"], rows[i:i + lr.shape[0]])
                                   for i, (lr, hr) in zip((0, 2), pairs)))
    want = float(rows.mean())
    print("LNCC_ERR evaluate_pairs_with: lncc %.9f restatement %.9f E_ref %.3e" % (out["lncc"], want, E_ref))
    assert rows.shape == (3,) and 0 < want < 1 and abs(out["lncc"] - want) <= (K2 * E_ref + ulp_rel(want)) * want


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
def test_train_step_lncc_term(fa, O, two_chains, monkeypatch):
    """192^2, batch 1, the smallest step of tests/test_gpu_step.py.  With ``reproducible_forward`` the forward and the losses are
    bit-reproducible, so against the weight-0 step: the tensors and every other loss keep their bits; ``loss_lncc`` is the composition
    of ``ops.lncc`` on the step's own tensors -- 0.5 ((1 - S(fake_B, real_A)) + (1 - S(fake_A, real_B))), formed in double from the op's
    fp32 scores; the step forms it in fp32, in the two-chain schedule as two halves: 4 roundings of 2^-24 relative to terms below 1,
    hence 1e-6 relative -- and ``loss_G`` is the weight-0 step's plus the term, to fp32 rounding of the sum (1e-6 relative).  The
    weight-0 step launches no LNCC kernel and the step with the term launches exactly two forwards and two one-sided backwards more;
    every other entry point keeps its count.  Both places the term lives: the two-chain schedule and the single-stream
    ``generator_loss``."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    calls = spy(fa, monkeypatch)
    try:
        tsd = fresh_step(fa, O, reproducible_forward=True)                 # the default step, first: it fills the process-wide tables
        Ld = tsd.step(a, b, sync=True, keep=True)
        ts = fresh_step(fa, O, reproducible_forward=True, lncc_weight=0.5)
        del calls[:]
        L = ts.step(a, b, sync=True, keep=True)
        with_term = counted(calls)
        grad_calls = [args for n, args in calls if n == "lncc_grad"]
        ts0 = fresh_step(fa, O, reproducible_forward=True, lncc_weight=0.0)
        del calls[:]
        L0 = ts0.step(a, b, sync=True, keep=True)
        without = counted(calls)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_lncc" not in L0 and ts0.lncc is None and tsd.lncc is None and ts.lncc is not None
    assert L0["loss_G"] == Ld["loss_G"]                                    # weight 0 is the default step, bit for bit
    assert not [n for n in without if n.startswith("lncc")]
    assert {n: c for n, c in with_term.items() if n.startswith("lncc")} == {"lncc_index": 2, "lncc_final": 2, "lncc_grad": 2}
    assert {n: c for n, c in with_term.items() if not n.startswith("lncc")} == without
    assert all(bool(g[DX_ARG]) and not g[DY_ARG] for g in grad_calls)      # the gradient reaches the fake only
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    with torch.no_grad():
        want = 0.5 * sum(1.0 - float(fa.ops.lncc(fake, real)) for fake, real in ((T["fake_B"], a), (T["fake_A"], b)))
    print("LNCC_ERR step two_chains=%s: loss_lncc %.7f composition %.7f, loss_G %.6f against %.6f at weight 0" % (
        two_chains, L["loss_lncc"], want, L["loss_G"], L0["loss_G"]))
    assert want > 0.05 and abs(L["loss_lncc"] - want) <= 1e-6 * abs(want)
    assert abs(L["loss_G"] - (L0["loss_G"] + L["loss_lncc"])) <= 1e-6 * abs(L["loss_G"])
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_lncc_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible: the
    replay's ``loss_lncc`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the
    caller's stream)."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, lncc_weight=0.5)
        Le = eager.step(a, b, sync=True)
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, lncc_weight=0.5)
        gs = fa.GraphedTrainStep(ts, a, b)
        Lg = gs.step(a, b, sync=True)
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    print("LNCC_ERR graph step: loss_lncc %.9f eager %.9f, loss_G %.9f eager %.9f" % (
        Lg["loss_lncc"], Le["loss_lncc"], Lg["loss_G"], Le["loss_G"]))
    assert Lg["loss_lncc"] > 0.05
    assert Lg["loss_lncc"] == Le["loss_lncc"] and Lg["loss_G"] == Le["loss_G"]      # the eager bits
    assert ts.opt_G.step_count == 1
