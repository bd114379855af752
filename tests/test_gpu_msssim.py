"""Multi-scale SSIM (csrc/msssim.hip) on the MI355X: ``ops.ms_ssim`` / ``MSSSIM`` / ``ssim.ms_ssim`` against the reference's own CPU
results (tests/golden/golden_msssim.npz) and the float64 restatement of tests/test_msssim_cpu.py (pinned to that fixture there):
tile seams, floors, exact cases, the clamp, M = 1 against ``ops.ssim``, the launch structure, ``evaluate_pairs(ms_ssim=...)`` and the
opt-in ``TrainStep(msssim_weight=...)`` term, eager in both schedules and hipGraph-captured.

Every error is measured against the float64 restatement; the bars are the project's, twice the fp32 reference's own error:

    gradients (relative L2, per array):        e_hip <= 2 e_ref + 2^-23
    score and per-image scores (relative):     e_hip <= 2 E_ref + 1 ulp of the score

e_ref is the fp32 reference's distance from the restatement (the fixture's ``f32`` arrays; off the fixture, the restatement run in
fp32 on the CPU).  A single scalar's e_ref can be small by luck, so E_ref is the LARGEST relative fp32-reference error of the score
over all fixture cases (off the fixture: that, or the case's own fp32 restatement if larger).

The conditioning cap.  ``w_j MS / F_j`` amplifies rounding where a factor is small: every test that compares gradients first
asserts, on the float64 restatement, that every F_j[n] is at least 0.25.  The inputs are x = 5x5-box-smoothed N(0, 1) noise times 2
clipped to [-1, 1] and y = clip(x + 0.15 n), whose smallest factor is about 0.87; nothing is excluded.

The kernels' tiles: ``msssim_scale_fwd`` 16 x 64 (rows x columns) of a plane of a scale, ``msssim_scale_bwd`` 16 x 32.

Each array prints an ``MSSSIM_ERR`` line (run with ``-s``; a run's lines are what profiles/msssim_error.txt holds)."""
import math
import random

import pytest
import torch

from test_msssim_cpu import CASES, case_name, fixture_inputs, gold, rel_l2, restate, restate_case, score_err, smooth_pair, well_conditioned

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
FWD_TILE, BWD_TILE = (16, 64), (16, 32)       # csrc/msssim.hip MF_TY x MF_TX, MB_TY x MB_TX
PA_ARG, PB_ARG = 2, 3                         # msssim_scale_fwd(a, b, pa, pb, workspace, ...)
COEF_ARG = 10                                 # msssim_final(workspace, N, C, H, W, levels, weights, average, out_image, out_mean, coef, stream)
G_ARG, DCA_ARG, DCB_ARG, DA_ARG, DB_ARG = 3, 5, 6, 7, 8       # msssim_scale_bwd(a, b, coef, g, gN, dca, dcb, da, db, ...)


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def run_hip(fa, x, y, levels=5, weights=None, data_range=1.0, per_image=False, x_grad=True, y_grad=True, upstream=None):
    """{"score", "dx", "dy"} of ``ops.ms_ssim`` on the GPU, back on the host; the gradients are those of ``(score * upstream).sum()``."""
    xd = x.float().cuda().detach().requires_grad_(x_grad)
    yd = y.float().cuda().detach().requires_grad_(y_grad)
    S = fa.ops.ms_ssim(xd, yd, levels, weights, data_range, per_image)
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
    print("MSSSIM_ERR %-34s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f smallest factor %.3f" % (
        name, "score", E_ref, own, e_hip, e_hip / E_ref, float(ref64["factors"].min())))
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
        print("MSSSIM_ERR %-34s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K2 * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


def against_restatement(fa, name, x, y, levels, **kw):
    ref64 = restate(x, y, levels, **kw)
    ref32 = restate(x, y, levels, dtype=torch.float32, **kw)
    hold_to_bar(name, ref64, ref32, run_hip(fa, x, y, levels, **kw))


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """The score, dx and dy of every fixture case."""
    cid, _, levels, weights, data_range, per_image, y_grad = case
    g = gold()
    ref64 = restate_case(case)
    ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ref64}
    x, y = fixture_inputs(case)
    hold_to_bar(cid, ref64, ref32, run_hip(fa, x, y, levels, weights, data_range, per_image, True, y_grad))


def test_tile_seams(fa):
    """(1, 1, 150, 278) at M = 5: scale 1 spans nine 16-row tiles and a remainder of 6 rows for both kernels, four 64-column tiles and
    a remainder of 22 for ``msssim_scale_fwd`` (tile 16 x 64), eight 32-column tiles and the same remainder for ``msssim_scale_bwd``
    (tile 16 x 32); scales 2 and 3 (75 x 139, 37 x 69) still span several tiles, and 75, 139, 37, 69 are odd: a floor at each."""
    H, W = 150, 278
    for ty, tx in (FWD_TILE, BWD_TILE):
        assert H // ty >= 3 and H % ty and W // tx >= 3 and W % tx
    x, y = smooth_pair((1, 1, H, W), 41)
    against_restatement(fa, "seams 1x1x150x278 M5", x, y, 5)


@pytest.mark.parametrize("levels", [3, 5])
@pytest.mark.parametrize("shape", [(1, 2, 37, 53), (2, 1, 23, 45)])
def test_floors(fa, shape, levels):
    """Odd sides: 37 x 53 -> 18 x 26 -> 9 x 13 -> 4 x 6 -> 2 x 3 and 23 x 45 -> 11 x 22 -> 5 x 11 -> 2 x 5 -> 1 x 2: a dropped row or
    column receives nothing from the coarser scale."""
    x, y = smooth_pair(shape, 42)
    against_restatement(fa, "floors %s M%d" % ("x".join(map(str, shape)), levels), x, y, levels)


def test_floors_per_image_with_upstream(fa):
    """Per-image scores with an upstream gradient per image, read on the device."""
    x, y = smooth_pair((2, 1, 23, 45), 43)
    up = torch.tensor([0.25, -1.5])
    against_restatement(fa, "floors 2x1x23x45 M4 per image", x, y, 4, per_image=True, upstream=up)


def test_side_below_the_last_scale_is_refused(fa):
    z = torch.zeros(1, 1, 15, 45).cuda()
    with pytest.raises(ValueError, match="leaves scale 5 empty"):
        fa.ops.ms_ssim(z, z)
    assert float(fa.ops.ms_ssim(z, z, levels=4)) == 1.0


# ------------------------------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, y, scale=None, per_image=False, levels=5, weights=None):
    xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    S = fa.ops.ms_ssim(xd, yd, levels, weights, 1.0, per_image)
    (S.sum() if scale is None else (S * scale).sum()).backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


@pytest.mark.parametrize("levels,shape", [(5, (2, 2, 40, 72)), (3, (1, 3, 37, 53)), (1, (2, 1, 18, 130))])
def test_exact_cases(fa, levels, shape):
    x, y = (t.cuda() for t in smooth_pair(shape, 5))
    S, dx, dy = grads(fa, x, x.clone(), levels=levels)
    assert float(S) == 1.0 and not dx.any() and not dy.any()
    Sn, dxn, dyn = grads(fa, x, x.clone(), per_image=True, levels=levels)
    assert bool((Sn == 1.0).all()) and not dxn.any() and not dyn.any()
    Sxy, dx, dy = grads(fa, x, y, levels=levels)
    Syx, ex, ey = grads(fa, y, x, levels=levels)
    assert torch.equal(Sxy, Syx)                                          # bit for bit
    assert torch.equal(dx, ey) and torch.equal(dy, ex)
    assert 0 < float(Sxy) < 1 and dx.abs().max() > 0 and dy.abs().max() > 0
    _, hx, hy = grads(fa, x, y, scale=0.5, levels=levels)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hy, 0.5 * dy)         # the upstream gradient, applied on the device
    rows, rdx, rdy = grads(fa, x, y, per_image=True, levels=levels)
    for n in range(shape[0]):
        alone, adx, ady = grads(fa, x[n:n + 1], y[n:n + 1], per_image=True, levels=levels)
        assert torch.equal(alone[0], rows[n]) and torch.equal(adx[0], rdx[n]) and torch.equal(ady[0], rdy[n])


def test_bit_reproducible_and_on_a_side_stream(fa):
    x, y = smooth_pair((2, 1, 64, 192), 6)
    first, again = run_hip(fa, x, y), run_hip(fa, x, y)
    assert all(torch.equal(first[k], again[k]) for k in first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_hip(fa, x, y)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(first[k], side[k]) for k in first)


def test_clamp(fa):
    """y = -x: the contrast-structure factor is negative, every image's score is exactly 0 and both gradients exactly zero."""
    x, _ = smooth_pair((2, 2, 37, 53), 7)
    assert float(restate(x, -x, 5, x_grad=False, y_grad=False)["factors"].min()) < 0
    for per_image in (False, True):
        got = run_hip(fa, x, -x, 5, per_image=per_image)
        assert not got["score"].any() and not torch.isnan(got["score"]).any()
        for k in ("dx", "dy"):
            assert not torch.isnan(got[k]).any() and not got[k].any(), k
    # one clamped image beside a live one: only the live one carries a gradient
    y = torch.cat((-x[:1], smooth_pair((1, 2, 37, 53), 8)[1]))
    x2 = torch.cat((x[:1], smooth_pair((1, 2, 37, 53), 8)[0]))
    got = run_hip(fa, x2, y, 5, per_image=True)
    assert float(got["score"][0]) == 0.0 and 0 < float(got["score"][1]) < 1
    assert not got["dx"][0].any() and not got["dy"][0].any() and got["dx"][1].abs().max() > 0
    assert not torch.isnan(got["dx"]).any() and not torch.isnan(got["dy"]).any()


def test_one_level_is_ssim(fa):
    """M = 1, weights (1,): ``ops.ssim`` on the same pair, within the bars above (not bitwise: ``ops.ssim`` sums with atomics); an odd
    width takes ``ops.ssim``'s tiled kernels, an even one its sliding-window kernels.  One plane per image and at most 22 x 64 (tiled)
    or 32 x 128 (sliding) pixels keep ``ops.ssim`` to one atomic per image, so that its side of the comparison does not vary from
    run to run; ``msssim_scale_fwd`` still takes two tiles per plane."""
    for shape, seed in (((2, 1, 21, 53), 9), ((2, 1, 32, 64), 10)):
        x, y = smooth_pair(shape, seed)
        ref64 = restate(x, y, 1, (1.0,))
        ref32 = restate(x, y, 1, (1.0,), dtype=torch.float32)
        well_conditioned(ref64)
        got = run_hip(fa, x, y, 1, (1.0,))
        xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        S = fa.ops.ssim(xd, yd)
        S.backward()
        E_ref = max(score_E_ref(), score_err(ref32["score"], ref64["score"]))
        e = score_err(got["score"], S.detach().cpu())
        print("MSSSIM_ERR M1 against ops.ssim %-12s score  e_ref %.3e difference %.3e" % ("x".join(map(str, shape)), E_ref, e))
        assert e <= K2 * E_ref + ulp_rel(ref64["score"])
        for k, t in (("dx", xd.grad), ("dy", yd.grad)):
            e_ref, e = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], t.cpu())
            print("MSSSIM_ERR M1 against ops.ssim %-12s %-6s e_ref %.3e difference %.3e" % ("x".join(map(str, shape)), k, e_ref, e))
            assert e <= K2 * e_ref + FLOOR
        rows = run_hip(fa, x, y, 1, (1.0,), per_image=True, x_grad=False, y_grad=False)["score"]
        want = fa.ops.ssim(x.cuda(), y.cuda(), False).cpu()
        assert score_err(rows, want) <= K2 * E_ref + ulp_rel(want.min())


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("M", [1, 3, 5])
def test_launch_counts(fa, monkeypatch, M):
    """M + 1 launches forward (one ``msssim_scale_fwd`` per scale, pooled pointers null at the last, then ``msssim_final``), M
    backward, coarsest first; the da / db pointer is null for the input that needs no gradient."""
    x, y = (t.cuda() for t in smooth_pair((2, 2, 32, 48), 3))
    for x_grad, y_grad in ((True, True), (True, False), (False, True)):
        xd, yd = x.clone().requires_grad_(x_grad), y.clone().requires_grad_(y_grad)
        calls = spy(fa, monkeypatch)
        S = fa.ops.ms_ssim(xd, yd, M)
        assert [n for n, _ in calls] == ["msssim_scale_fwd"] * M + ["msssim_final"]
        fwd = [a for n, a in calls if n == "msssim_scale_fwd"]
        assert all(a[PA_ARG] and a[PB_ARG] for a in fwd[:-1]) and fwd[-1][PA_ARG] is None and fwd[-1][PB_ARG] is None
        assert [a[9] for a in fwd] == list(range(M))                      # the scale index
        assert calls[-1][1][COEF_ARG]
        del calls[:]
        S.backward()
        assert [n for n, _ in calls] == ["msssim_scale_bwd"] * M
        assert [a[14] for _, a in calls] == list(range(M - 1, -1, -1))    # coarsest first
        for i, (_, a) in enumerate(calls):
            assert bool(a[DA_ARG]) == x_grad and bool(a[DB_ARG]) == y_grad and a[G_ARG]
            assert bool(a[DCA_ARG]) == (x_grad and i > 0) and bool(a[DCB_ARG]) == (y_grad and i > 0)
        assert (xd.grad is not None) == x_grad and (yd.grad is not None) == y_grad
        monkeypatch.undo()


def test_no_grad_forward_writes_no_table_and_changes_no_bit(fa, monkeypatch):
    x, y = (t.cuda() for t in smooth_pair((2, 3, 32, 48), 2))
    calls = spy(fa, monkeypatch)
    Sg = fa.ops.ms_ssim(x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert calls[-1][0] == "msssim_final" and calls[-1][1][COEF_ARG]
    assert len(Sg.grad_fn.saved_tensors) == 1 + 2 * 5                     # the table, the inputs and the pooled pairs of scales 2..5
    assert sum(t.numel() for t in Sg.grad_fn.saved_tensors[3:]) <= (2 * x.numel()) // 3
    del calls[:]
    with torch.no_grad():
        Sn = fa.ops.ms_ssim(x.clone().requires_grad_(True), y.clone().requires_grad_(True))
    assert len(calls) == 6 and calls[-1][1][COEF_ARG] is None              # a null table pointer
    assert not Sn.requires_grad and Sn.grad_fn is None
    del calls[:]
    Sp = fa.ops.ms_ssim(x, y)                                              # inputs that need no gradient
    assert len(calls) == 6 and calls[-1][1][COEF_ARG] is None and not Sp.requires_grad
    assert torch.equal(Sn, Sg) and torch.equal(Sp, Sg)


def test_module_and_function_are_the_op(fa):
    x, y = (t.cuda() for t in smooth_pair((2, 1, 32, 48), 4))
    want = fa.ops.ms_ssim(x, y, 3, (0.2, 0.3, 0.5), 2.0)
    rows = fa.ops.ms_ssim(x, y, 3, (0.2, 0.3, 0.5), 2.0, True)
    mod = fa.MSSSIM(levels=3, weights=(0.2, 0.3, 0.5), data_range=2.0).cuda()
    assert torch.equal(mod(x, y), want) and torch.equal(mod.index(x, y, True), rows)
    assert torch.equal(fa.MSSSIM(size_average=False, levels=3, weights=(0.2, 0.3, 0.5), data_range=2.0)(x, y), rows)
    assert torch.equal(fa.ms_ssim(x, y, levels=3, weights=(0.2, 0.3, 0.5), data_range=2.0), want)
    assert torch.equal(fa.ms_ssim(x, y, size_average=False, levels=3, weights=(0.2, 0.3, 0.5), data_range=2.0), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    big = torch.cat((x, x), dim=3)
    vx, vy = big[:, :, :, 48:], torch.cat((y, y), dim=3)[:, :, :, 48:]      # views equal their contiguous copies
    assert not vx.is_contiguous() and torch.equal(mod(vx, vy), want)


# ------------------------------------------------------------------------------------------------------------------------
# the evaluation path
# ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pairs_key(fa, monkeypatch):
    """The key is the mean of the per-image index of (super_resolve(lr), hr).  The generator's forward is not bit-reproducible
    (split-K atomics), so ``super_resolve`` is replaced by a fixed map; the four metric columns and the index run their kernels."""
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: (0.9 * lr).contiguous())
    pairs = []
    for seed, n in ((21, 2), (22, 1)):
        hr, lr = smooth_pair((n, 1, 64, 64), seed)
        pairs.append((lr.cuda(), hr.cuda()))
    mod = fa.MSSSIM().cuda()
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs(None, pairs, ms_ssim=mod)
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "ms_ssim"] and all(out[k] == plain[k] for k in plain)
    with torch.no_grad():
        rows = torch.cat([mod.index((0.9 * lr).contiguous(), hr, True) for lr, hr in pairs]).double()
    assert rows.shape == (3,) and out["ms_ssim"] == pytest.approx(float(rows.mean()), rel=1e-12) and 0 < out["ms_ssim"] < 1


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


def restated_term(weight, T, a, b, levels=5):
    return weight * sum(1.0 - float(restate(rec, real, levels, x_grad=False, y_grad=False)["score"])
                        for rec, real in ((T["recovered_A"], a), (T["recovered_B"], b)))


@pytest.mark.parametrize("two_chains", [True, False])
def test_train_step_msssim_term(fa, O, two_chains):
    """192^2, batch 2, the shapes of the CW-SSIM step tests.  The weight-0 step is the step tests/test_gpu_step.py holds to the
    oracle; with ``reproducible_forward`` its forward and losses are bit-reproducible, so: a step built with ``msssim_weight=0.0``
    equals the plain step bit for bit; ``loss_msssim`` is the restated term on the step's own tensors (1e-5 relative: twice the fp32
    rounding of a score near 1 over a term 1 - MS of a few tenths); every other loss keeps its bits, and ``loss_G`` is the plain step's
    plus the term to fp32 rounding of the sum (1e-6 relative); the term moves the generators' gradient: two runs of one step agree to
    1e-5 relative on the gradient arenas (``test_reproducible_forward_mode``), so a generator's gradient norm that moves by more than
    1e-4 relative has moved by ten times what the atomics' summation order explains (the untrained generators' reconstructions score
    MS of about 0.005, where the term's gradient is small).  Both places the opt-in terms live: the two-chain schedule and the
    single-stream ``generator_loss``."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    try:
        ts = fresh_step(fa, O, reproducible_forward=True, msssim_weight=0.5)
        L = ts.step(a, b, sync=True, keep=True)
        gn = ts.grad_norms()
        ts0 = fresh_step(fa, O, reproducible_forward=True)
        L0 = ts0.step(a, b, sync=True, keep=True)
        gn0 = ts0.grad_norms()
        tsz = fresh_step(fa, O, reproducible_forward=True, msssim_weight=0.0)
        Lz = tsz.step(a, b, sync=True, keep=True)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_msssim" not in L0 and ts0.msssim is None and tsz.msssim is None
    assert set(Lz) == set(L0)
    for k, v in L0.items():                                               # weight 0: unchanged bit for bit
        if k == "tensors":
            assert all(torch.equal(Lz[k][n], t) for n, t in v.items())
        else:
            assert Lz[k] == v, (k, Lz[k], v)
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    want = restated_term(0.5, T, a, b)
    print("MSSSIM_ERR step two_chains=%s: loss_msssim %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0, |grad A2B| %.5f against %.5f, "
          "|grad B2A| %.5f against %.5f" % (two_chains, L["loss_msssim"], want, L["loss_G"], L0["loss_G"], gn["A2B"], gn0["A2B"], gn["B2A"], gn0["B2A"]))
    assert want > 0.05 and abs(L["loss_msssim"] - want) <= 1e-5 * abs(want)
    assert abs(L["loss_G"] - (L0["loss_G"] + want)) <= 1e-6 * abs(L["loss_G"])
    assert abs(gn["A2B"] - gn0["A2B"]) > 1e-4 * gn0["A2B"] or abs(gn["B2A"] - gn0["B2A"]) > 1e-4 * gn0["B2A"], (gn, gn0)
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_msssim_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible:
    the replay's ``loss_msssim`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the
    caller's stream).  Two more replays follow the eager step at the bars of the existing graph tests."""
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, msssim_weight=0.5)
        Le = [eager.step(a, b, sync=True) for a, b in batches]
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, msssim_weight=0.5)
        gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
        Lg = [gs.step(a, b, sync=True) for a, b in batches]
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    for s in range(3):
        print("MSSSIM_ERR graph step %d: loss_msssim %.9f eager %.9f, loss_G %.9f eager %.9f" % (
            s, Lg[s]["loss_msssim"], Le[s]["loss_msssim"], Lg[s]["loss_G"], Le[s]["loss_G"]))
    assert Lg[0]["loss_msssim"] == Le[0]["loss_msssim"] and Lg[0]["loss_G"] == Le[0]["loss_G"]      # the eager bits
    for s in (1, 2):
        assert Lg[s]["loss_msssim"] == pytest.approx(Le[s]["loss_msssim"], abs=0.03 if s == 1 else 0.06)
        assert Lg[s]["loss_G"] == pytest.approx(Le[s]["loss_G"], rel=3e-3, abs=1e-6)
    assert ts.opt_G.step_count == 3
