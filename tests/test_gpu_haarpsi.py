"""HaarPSI (csrc/haarpsi.hip) on the MI355X: ``ops.haarpsi`` / ``HaarPSI`` / ``ssim.haarpsi`` against the float64 restatement of
tests/test_haarpsi_cpu.py (pinned there to tests/golden/golden_haarpsi.npz, whose values come from explicit slice sums): the map smaller
than the filter, odd sides, tile seams, pooled channels, exact cases, the launch structure, ``evaluate_pairs_with(haarpsi=...)`` and the
opt-in ``TrainStep(haarpsi_weight=...)`` term, eager in both schedules and hipGraph-captured.

Every error is measured against the float64 restatement; the bars are the project's, twice the fp32 reference's own error:

    gradients (relative L2, per array):        e_hip <= 2 e_ref + 2^-23
    score and per-image scores (relative):     e_hip <= 2 E_ref + 1 ulp of the score

e_ref is the fp32 reference's distance from the restatement (the fixture's ``f32`` arrays; off the fixture, the restatement run in
fp32 on the CPU).  A single scalar's e_ref can be small by luck, so E_ref is the LARGEST relative fp32-reference error of the score
over all fixture cases (off the fixture: that, or the case's own fp32 restatement if larger).

The tie caps (tests/test_haarpsi_cpu.py): every gradient comparison first asserts, on the float64 restatement and in the mapped 0..255
units, min |g^o_k| >= 2^-9 (k = 1, 2) and min | |g^o_3(x)| - |g^o_3(y)| | >= 2^-7; nothing is excluded.

The kernels' tiles of the half-resolution map are read out of csrc/haarpsi.hip (``kernel_tiles`` of tests/test_haarpsi_cpu.py, which
also asserts there that the fixture's seam case crosses them): ``haarpsi_index`` 16 x 64 (rows x columns), ``haarpsi_grad`` 16 x 16.
No seed of range(2000) meets the caps at (1, 1, 72, 264), two index tiles and a remainder per axis (see tests/test_haarpsi_cpu.py), so
the gradients' seam case is one seam per axis, (2, 1, 40, 136): half-resolution 20 x 68.  The caps concern gradients only: the SCORE of
the two-tiles-and-a-remainder shape is held to its bar in ``test_two_index_tiles_per_axis_score``.

Each array prints a ``HAARPSI_ERR`` line (run with ``-s``; a run's lines are what profiles/haarpsi_error.txt holds)."""
import math
import random

import pytest
import torch

from test_haarpsi_cpu import CASES, case_name, find_pair, fixture_inputs, gold, kernel_tiles, make_pair, rel_l2, restate, restate_case, score_err, well_conditioned

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
FAC_ARG = 9                                   # haarpsi_final(workspace, N, C, H, W, alpha, average, out_image, out_mean, fac, stream)
G_ARG, DX_ARG, DY_ARG = 3, 5, 6               # haarpsi_grad(x, y, fac, g, gN, dx, dy, ...)


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def run_hip(fa, x, y, c=30.0, alpha=4.2, value_range=(-1.0, 1.0), per_image=False, x_grad=True, y_grad=True, upstream=None):
    """{"score", "dx", "dy"} of ``ops.haarpsi`` on the GPU, back on the host; the gradients are those of ``(score * upstream).sum()``."""
    xd = x.float().cuda().detach().requires_grad_(x_grad)
    yd = y.float().cuda().detach().requires_grad_(y_grad)
    S = fa.ops.haarpsi(xd, yd, c, alpha, value_range, per_image)
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
    well_conditioned(ref64)                                               # the tie caps
    own = score_err(ref32["score"], ref64["score"])
    E_ref = max(score_E_ref(), own)
    e_hip = score_err(got["score"], ref64["score"])
    print("HAARPSI_ERR %-30s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f min |g12| %.2e min tie %.2e" % (
        name, "score", E_ref, own, e_hip, e_hip / E_ref, ref64["coef_min"], ref64["tie_min"]))
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
        print("HAARPSI_ERR %-30s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K2 * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """The score, dx and dy of every fixture case: (1,1,8,8), whose 4 x 4 map is smaller than the 8 x 8 filter; (2,1,16,16), the mean over
    the batch; (2,2,32,48) per image with c = 20, alpha = 3.5 and value_range (0, 1); (1,3,16,24), channels pooled; (1,1,37,53), odd sides:
    the zero sample of the 2 x 2 mean and the last pixel of the adjoint; (2,1,40,136), a seam per axis of ``haarpsi_index`` and four of
    ``haarpsi_grad``; (2,1,16,16) with y needing no gradient."""
    cid, shape, c, alpha, value_range, per_image, y_grad, _ = case
    g = gold()
    ref64 = restate_case(case)
    ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("score", "dx", "dy") if k in ref64}
    x, y = fixture_inputs(case)
    hold_to_bar("%s %s" % (cid, "x".join(map(str, shape))), ref64, ref32, run_hip(fa, x, y, c, alpha, value_range, per_image, True, y_grad))


def test_two_index_tiles_per_axis_score(fa):
    """Two ``haarpsi_index`` tiles and a ragged remainder of 4 per axis at N = C = 1, from the kernel's tile constants ((1, 1, 72, 264) for
    16 x 64): the layout of the partials and ``haarpsi_final`` over six blocks of one image.  No seed meets the tie caps at this shape,
    and they concern the gradients alone (a flipped sign or maximum moves the score by nothing), so the scores -- the mean and the
    per-image form -- are held to their bar and no gradient is compared."""
    (ty, tx), _ = kernel_tiles()
    shape = (1, 1, 2 * (2 * ty + 4), 2 * (2 * tx + 4))
    x, y = make_pair(shape, 0)
    for per_image in (False, True):
        ref64 = restate(x, y, per_image=per_image, x_grad=False, y_grad=False)
        ref32 = restate(x, y, per_image=per_image, x_grad=False, y_grad=False, dtype=torch.float32)
        got = run_hip(fa, x, y, per_image=per_image, x_grad=False, y_grad=False)
        own = score_err(ref32["score"], ref64["score"])
        E_ref = max(score_E_ref(), own)
        e_hip = score_err(got["score"], ref64["score"])
        print("HAARPSI_ERR %-30s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f" % (
            "two tiles %s%s" % ("x".join(map(str, shape)), " per image" if per_image else ""), "score", E_ref, own, e_hip, e_hip / E_ref))
        assert tuple(got["score"].shape) == tuple(ref64["score"].shape)
        assert e_hip <= K2 * E_ref + ulp_rel(ref64["score"].reshape(-1)[0])


def test_per_image_with_upstream(fa):
    """Per-image scores of an odd-sided pair with an upstream gradient per image, read on the device; off the fixture."""
    x, y = find_pair((2, 1, 11, 19))
    up = torch.tensor([0.25, -1.5])
    ref64 = restate(x, y, per_image=True, upstream=up)
    ref32 = restate(x, y, per_image=True, upstream=up, dtype=torch.float32)
    hold_to_bar("upstream 2x1x11x19", ref64, ref32, run_hip(fa, x, y, per_image=True, upstream=up))


# ------------------------------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, y, scale=None, per_image=False, **kw):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    S = fa.ops.haarpsi(xd, yd, per_image=per_image, **kw)
    (S.sum() if scale is None else (S * scale).sum()).backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize("shape", [(2, 2, 40, 72), (1, 3, 37, 53), (2, 1, 18, 130)])
def test_exact_cases(fa, shape):
    x, y = (t.cuda() for t in make_pair(shape, 5))
    Sxy, dx, dy = grads(fa, x, y)
    Syx, ex, ey = grads(fa, y, x)
    assert torch.equal(Sxy, Syx)                                          # bit for bit
    assert torch.equal(dx, ey) and torch.equal(dy, ex)
    assert 0 < float(Sxy) < 1 and dx.abs().max() > 0 and dy.abs().max() > 0
    _, hx, hy = grads(fa, x, y, scale=0.5)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hy, 0.5 * dy)         # the upstream gradient, applied on the device
    S, ix, iy = grads(fa, x, x.clone())
    assert abs(float(S) - 1.0) <= 1e-6
    assert float(ix.norm()) <= 1e-6 * float(dx.norm()) and float(iy.norm()) <= 1e-6 * float(dy.norm())
    Sn, _, _ = grads(fa, x, x.clone(), per_image=True)
    assert float((Sn - 1).abs().max()) <= 1e-6
    rows, rdx, rdy = grads(fa, x, y, per_image=True)
    for n in range(shape[0]):
        alone, adx, ady = grads(fa, x[n:n + 1], y[n:n + 1], per_image=True)
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


def test_flat_pair(fa):
    """Both images at ``lo``: the denominator is exactly 0, every score exactly 1 and both gradients exactly zero; a flat pair beside a
    live one leaves the live one its gradient."""
    z = torch.full((2, 2, 9, 12), -1.0)
    for per_image in (False, True):
        got = run_hip(fa, z, z.clone(), per_image=per_image)
        assert bool((got["score"] == 1).all())
        for k in ("dx", "dy"):
            assert not torch.isnan(got[k]).any() and not got[k].any(), k
    x, y = make_pair((1, 2, 9, 12), 7)
    got = run_hip(fa, torch.cat((z[:1], x)), torch.cat((z[:1], y)), per_image=True)
    assert float(got["score"][0]) == 1.0 and 0 < float(got["score"][1]) < 1
    assert not got["dx"][0].any() and not got["dy"][0].any() and got["dx"][1].abs().max() > 0
    assert not torch.isnan(got["dx"]).any() and not torch.isnan(got["dy"]).any()


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def test_launch_counts(fa, monkeypatch):
    """Two entry points forward (``haarpsi_index``, ``haarpsi_final``), one backward; the dx / dy pointer is null for the input that
    needs no gradient."""
    x, y = (t.cuda() for t in make_pair((2, 2, 32, 48), 3))
    for x_grad, y_grad in ((True, True), (True, False), (False, True)):
        xd, yd = x.clone().requires_grad_(x_grad), y.clone().requires_grad_(y_grad)
        calls = spy(fa, monkeypatch)
        S = fa.ops.haarpsi(xd, yd)
        assert [n for n, _ in calls] == ["haarpsi_index", "haarpsi_final"] and calls[-1][1][FAC_ARG]
        del calls[:]
        S.backward()
        assert [n for n, _ in calls] == ["haarpsi_grad"]
        a = calls[0][1]
        assert bool(a[DX_ARG]) == x_grad and bool(a[DY_ARG]) == y_grad and a[G_ARG]
        assert (xd.grad is not None) == x_grad and (yd.grad is not None) == y_grad
        monkeypatch.undo()


def test_one_sided_gradient_is_the_two_sided_one(fa):
    """A null ``dx`` / ``dy`` skips that side's cotangents, maps and gathers in ``haarpsi_grad``; the side that is asked for keeps its
    bits.  (2, 1, 40, 72): several tiles and a remainder."""
    x, y = make_pair((2, 1, 40, 72), 8)
    both = run_hip(fa, x, y)
    only_x, only_y = run_hip(fa, x, y, y_grad=False), run_hip(fa, x, y, x_grad=False)
    assert "dy" not in only_x and "dx" not in only_y
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_y["dy"], both["dy"]) and both["dx"].abs().max() > 0
    assert torch.equal(only_x["score"], both["score"]) and torch.equal(only_y["score"], both["score"])


def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch):
    x, y = (t.cuda() for t in make_pair((2, 3, 32, 48), 2))
    calls = spy(fa, monkeypatch)
    Sg = fa.ops.haarpsi(x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert calls[-1][0] == "haarpsi_final" and calls[-1][1][FAC_ARG]
    saved = Sg.grad_fn.saved_tensors
    assert len(saved) == 3 and tuple(saved[2].shape) == (2, 2)             # the two images and the factor table only
    del calls[:]
    with torch.no_grad():
        Sn = fa.ops.haarpsi(x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert len(calls) == 2 and calls[-1][1][FAC_ARG] is None               # a null table pointer
    assert not Sn.requires_grad and Sn.grad_fn is None
    del calls[:]
    Sp = fa.ops.haarpsi(x, y)                                              # inputs that need no gradient
    assert len(calls) == 2 and calls[-1][1][FAC_ARG] is None and not Sp.requires_grad
    assert torch.equal(Sn, Sg) and torch.equal(Sp, Sg)


def test_module_and_function_are_the_op(fa):
    x, y = (t.cuda() for t in make_pair((2, 1, 32, 48), 4))
    want = fa.ops.haarpsi(x, y, 20.0, 3.5, (0.0, 1.0))
    rows = fa.ops.haarpsi(x, y, 20.0, 3.5, (0.0, 1.0), True)
    mod = fa.HaarPSI(c=20.0, alpha=3.5, value_range=(0.0, 1.0)).cuda()
    assert torch.equal(mod(x, y), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(fa.HaarPSI(20.0, 3.5, (0.0, 1.0), size_average=False)(x, y), rows)
    assert torch.equal(fa.ssim.haarpsi(x, y, 20.0, 3.5, (0.0, 1.0)), want)
    assert torch.equal(fa.ssim.haarpsi(x, y, 20.0, 3.5, (0.0, 1.0), size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    big = torch.cat((x, x), dim=3)
    vx, vy = big[:, :, :, 48:], torch.cat((y, y), dim=3)[:, :, :, 48:]      # views equal their contiguous copies
    assert not vx.is_contiguous() and torch.equal(mod(vx, vy), want)


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
        hr, lr = make_pair((n, 1, 32, 32), seed)
        pairs.append((lr.cuda(), hr.cuda()))
    mod = fa.HaarPSI().cuda()
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs_with(None, pairs, haarpsi=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "haarpsi"] and all(out[k] == plain[k] for k in plain)
    rows = torch.cat([restate((0.9 * lr).cpu(), hr.cpu(), per_image=True, x_grad=False, y_grad=False)["score"] for lr, hr in pairs])
    E_ref = max(score_E_ref(), max(score_err(restate((0.9 * lr).cpu(), hr.cpu(), per_image=True, x_grad=False, y_grad=False,
                                                     dtype=torch.float32)["score"], rows[i:i + lr.shape[0]])
                                   for i, (lr, hr) in zip((0, 2), pairs)))
    want = float(rows.mean())
    print("HAARPSI_ERR evaluate_pairs_with: haarpsi %.9f restatement %.9f E_ref %.3e" % (out["haarpsi"], want, E_ref))
    assert rows.shape == (3,) and 0 < want < 1 and abs(out["haarpsi"] - want) <= (K2 * E_ref + ulp_rel(want)) * want


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


@pytest.mark.parametrize("two_chains", [True, False])
def test_train_step_haarpsi_term(fa, O, two_chains):
    """192^2, batch 1, the smallest step of tests/test_gpu_step.py.  With ``reproducible_forward`` the forward and the losses are
    bit-reproducible, so against the weight-0 step (the step tests/test_gpu_step.py holds to the oracle): the tensors and every other
    loss keep their bits; ``loss_haarpsi`` is the module's value on the step's own tensors -- 0.5 ((1 - H_A) + (1 - H_B)), formed in
    double from the module's fp32 scores; the step forms it in fp32, in the two-chain schedule as two halves: 4 roundings of 2^-24
    relative to terms below 1, hence 1e-6 relative -- and ``loss_G`` is the weight-0 step's plus the term, to fp32 rounding of the sum
    (1e-6 relative).  Both places the opt-in terms live: the two-chain schedule and the single-stream ``generator_loss``."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    try:
        ts = fresh_step(fa, O, reproducible_forward=True, haarpsi_weight=0.5)
        L = ts.step(a, b, sync=True, keep=True)
        ts0 = fresh_step(fa, O, reproducible_forward=True)
        L0 = ts0.step(a, b, sync=True, keep=True)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_haarpsi" not in L0 and ts0.haarpsi is None and ts.haarpsi is not None
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    with torch.no_grad():
        want = 0.5 * sum(1.0 - float(ts.haarpsi(rec, real)) for rec, real in ((T["recovered_A"], a), (T["recovered_B"], b)))
    print("HAARPSI_ERR step two_chains=%s: loss_haarpsi %.7f module %.7f, loss_G %.6f against %.6f at weight 0" % (
        two_chains, L["loss_haarpsi"], want, L["loss_G"], L0["loss_G"]))
    assert want > 0.05 and abs(L["loss_haarpsi"] - want) <= 1e-6 * abs(want)
    assert abs(L["loss_G"] - (L0["loss_G"] + L["loss_haarpsi"])) <= 1e-6 * abs(L["loss_G"])
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_haarpsi_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible: the
    replay's ``loss_haarpsi`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the
    caller's stream)."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, haarpsi_weight=0.5)
        Le = eager.step(a, b, sync=True)
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, haarpsi_weight=0.5)
        gs = fa.GraphedTrainStep(ts, a, b)
        Lg = gs.step(a, b, sync=True)
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    print("HAARPSI_ERR graph step: loss_haarpsi %.9f eager %.9f, loss_G %.9f eager %.9f" % (
        Lg["loss_haarpsi"], Le["loss_haarpsi"], Lg["loss_G"], Le["loss_G"]))
    assert Lg["loss_haarpsi"] > 0.05
    assert Lg["loss_haarpsi"] == Le["loss_haarpsi"] and Lg["loss_G"] == Le["loss_G"]      # the eager bits
    assert ts.opt_G.step_count == 1
