"""The pixel-domain visual information fidelity (csrc/vif.hip) on the MI355X: ``ops.vif`` / ``ssim.vif`` / ``VIF`` against the float64
restatement of tests/test_vif_cpu.py (pinned there to tests/golden/golden_vif.npz, whose values come from explicit slice sums): every
fixture case, an off-fixture per-image pair with an upstream gradient, the exact properties, the asymmetry, every branch of the
definition, the structure of the launches, ``evaluate_pairs_with(vif=...)`` and the opt-in ``TrainStep(vif_weight=...)`` term, eager in
both schedules and as a captured graph.

The bars.  With ``e_ref`` the distance of the fp32 reference (the fixture's ``f32`` arrays; off the fixture the restatement run in
fp32) from float64 and ``E_ref`` the largest relative score error of the fp32 reference over the fixture (and the case at hand):

    gradients, relative L2 per array:   e_hip <= 2 e_ref + 2^-23
    scores, relative:                   e_hip <= 2 E_ref + 1 ulp

Both are measured against the reference; nothing is fixed in advance.

The conditioning caps (tests/test_vif_cpu.py): every gradient comparison first asserts, on the float64 restatement over all scales and
positions, min sxx >= 1, min srr >= 1, min g >= 0.5 and min sv >= 2^-8.

Each array prints a ``VIF_ERR`` line (run with ``-s``; a run's lines are what profiles/vif_error.txt holds)."""
import math
import random

import pytest
import torch

from test_vif_cpu import (CASES, DEFAULT, case_name, find_pair, fixture_inputs, gold, make_pair, rel_l2, restate, restate_case, score_err,
                          well_conditioned)

pytestmark = pytest.mark.gpu

K2, FLOOR = 2.0, 2.0 ** -23
NEXT_X_ARG, NEXT_R_ARG, WS_ARG = 2, 3, 4      # vif_scale_fwd(x, r, next_x, next_r, workspace, N, C, H, W, scale, ...)
FWD_SCALE_ARG = 9
TABLE_ARG = 8                                 # vif_final(workspace, N, C, H, W, average, out_image, out_mean, table, stream)
GTABLE_ARG, G_ARG, DNX_ARG, DNR_ARG, DX_ARG, DR_ARG, BWD_SCALE_ARG = 2, 3, 5, 6, 7, 8, 13    # vif_scale_bwd(x, r, table, g, gN, dnext_x, dnext_r, dx, dr, N, C, H, W, scale, ...)
FWD_NAMES = ["vif_scale_fwd"] * 4 + ["vif_final"]
BWD_NAMES = ["vif_scale_bwd"] * 4


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def op(fa, x, r, cfg=DEFAULT, per_image=False):
    return fa.ops.vif(x, r, cfg["sigma_n_sq"], cfg["value_range"], per_image)


def run_hip(fa, x, r, cfg=DEFAULT, per_image=False, x_grad=True, r_grad=True, upstream=None):
    """{"score", "dx", "dr"} of the op on the GPU, back on the host; the gradients are those of ``(score * upstream).sum()``."""
    xd = x.float().cuda().detach().requires_grad_(x_grad)
    rd = r.float().cuda().detach().requires_grad_(r_grad)
    V = op(fa, xd, rd, cfg, per_image)
    assert V.dtype == torch.float32 and V.shape == ((x.shape[0],) if per_image else ())
    if x_grad or r_grad:
        (V if upstream is None else V * upstream.cuda()).sum().backward()
    torch.cuda.synchronize()
    out = {"score": V.detach().cpu()}
    if x_grad:
        out["dx"] = xd.grad.cpu()
    if r_grad:
        out["dr"] = rd.grad.cpu()
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


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bars of the module docstring on every one."""
    bad = []
    well_conditioned(ref64)                                               # the conditioning caps
    own = score_err(ref32["score"], ref64["score"])
    E_ref = max(score_E_ref(), own)
    e_hip = score_err(got["score"], ref64["score"])
    print("VIF_ERR %-30s %-6s e_ref %.3e (this case %.3e) e_hip %.3e ratio %.3f min sxx %.1f srr %.1f g %.3f sv %.4f" % (
        name, "score", E_ref, own, e_hip, e_hip / E_ref, ref64["min_sxx"], ref64["min_srr"], ref64["min_g"], ref64["min_sv"]))
    assert tuple(got["score"].shape) == tuple(ref64["score"].shape)
    if not score_holds(got["score"], ref64["score"], E_ref):
        bad.append(("score", e_hip, E_ref))
    for k in ("dx", "dr"):
        if k not in ref64:
            assert k not in got
            continue
        assert tuple(got[k].shape) == tuple(ref64[k].shape)
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("VIF_ERR %-30s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K2 * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_fixture_parity(fa, case):
    """Every fixture case: (1,1,41,41), the minimum, one position at the last scale and a forward tile past the stat map; (2,1,48,56), the
    mean over the batch, and the same with the reference needing no gradient (the null ``dr``); (2,2,48,72) per image with sigma_n_sq 0.4
    and value_range (0, 2); (1,3,57,73), channels pooled, odd sides; (1,1,72,200), the stat maps of scales 0 and 1 across the seams of both
    kernels' tiles on both axes."""
    cid, shape, cfg, per_image, r_grad, _ = case
    g = gold()
    ref64 = restate_case(case)
    x, r = fixture_inputs(case)
    ref32 = {k: torch.from_numpy(g["%s/f32/%s" % (cid, k)]) for k in ("score", "dx", "dr") if k in ref64}
    hold_to_bar("%s %s" % (cid, "x".join(map(str, shape))), ref64, ref32, run_hip(fa, x, r, cfg, per_image, True, r_grad))


def test_per_image_with_upstream(fa):
    """Per-image scores of an odd-sided pair with an upstream gradient per image, read on the device; off the fixture."""
    x, r = find_pair((2, 1, 45, 83))
    up = torch.tensor([0.25, -1.5])
    ref64 = restate(x, r, per_image=True, upstream=up)
    ref32 = restate(x, r, per_image=True, upstream=up, dtype=torch.float32)
    hold_to_bar("upstream 2x1x45x83", ref64, ref32, run_hip(fa, x, r, per_image=True, upstream=up))


# ------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------
def grads(fa, x, r, cfg=DEFAULT, scale=None, per_image=False):
    xd, rd = x.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
    V = op(fa, xd, rd, cfg, per_image)
    (V.sum() if scale is None else (V * scale).sum()).backward()
    torch.cuda.synchronize()
    return V.detach().cpu(), xd.grad.cpu(), rd.grad.cpu()


@pytest.mark.parametrize("shape", [(2, 2, 48, 72), (1, 3, 57, 73), (2, 1, 43, 130)], ids=lambda s: "x".join(map(str, s)))
def test_bit_for_bit_properties(fa, shape):
    """Two runs agree; halving the upstream gradient halves both gradients; an image alone scores what it scores in a batch."""
    x, r = (t.cuda() for t in make_pair(shape, 5))
    V, dx, dr = grads(fa, x, r)
    assert 0 < float(V) < 1 and dx.abs().max() > 0 and dr.abs().max() > 0
    again = grads(fa, x, r)
    assert torch.equal(again[0], V) and torch.equal(again[1], dx) and torch.equal(again[2], dr)
    _, hx, hr = grads(fa, x, r, scale=0.5)
    assert torch.equal(hx, 0.5 * dx) and torch.equal(hr, 0.5 * dr)         # the upstream gradient, applied on the device
    rows, rdx, rdr = grads(fa, x, r, per_image=True)
    for n in range(shape[0]):
        alone, adx, adr = grads(fa, x[n:n + 1], r[n:n + 1], per_image=True)
        assert torch.equal(alone[0], rows[n]) and torch.equal(adx[0], rdx[n]) and torch.equal(adr[0], rdr[n])


def test_bit_reproducible_on_a_side_stream(fa):
    x, r = make_pair((2, 1, 64, 192), 6)
    first = run_hip(fa, x, r)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_hip(fa, x, r)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(first[k], side[k]) for k in first)


def test_one_sided_gradient_is_the_two_sided_one(fa):
    """A null ``dx`` / ``dr`` skips that side's gathers, adjoint and stores in ``vif_scale_bwd``; the side that is asked for keeps its
    bits.  (2, 1, 48, 72): several tiles and a remainder."""
    x, r = make_pair((2, 1, 48, 72), 8)
    both = run_hip(fa, x, r)
    only_x, only_r = run_hip(fa, x, r, r_grad=False), run_hip(fa, x, r, x_grad=False)
    assert "dr" not in only_x and "dx" not in only_r
    assert torch.equal(only_x["dx"], both["dx"]) and torch.equal(only_r["dr"], both["dr"]) and both["dx"].abs().max() > 0
    assert torch.equal(only_x["score"], both["score"]) and torch.equal(only_r["score"], both["score"])


def test_asymmetric(fa):
    """V(x, r) is not V(r, x): both hold the score bar against the float64 restatement, and they differ by far more than the bar."""
    (case,) = [c for c in CASES if c[0] == "mean"]
    x, r = fixture_inputs(case)
    fwd, rev = restate(x, r, x_grad=False, r_grad=False)["score"], restate(r, x, x_grad=False, r_grad=False)["score"]
    got_fwd, got_rev = run_hip(fa, x, r, x_grad=False, r_grad=False)["score"], run_hip(fa, r, x, x_grad=False, r_grad=False)["score"]
    print("VIF_ERR asymmetry: V(x, r) %.9f (restatement %.9f)  V(r, x) %.9f (restatement %.9f)" % (got_fwd, fwd, got_rev, rev))
    assert score_holds(got_fwd, fwd) and score_holds(got_rev, rev)
    assert abs(float(fwd) - float(rev)) > 100 * (K2 * score_E_ref() + ulp_rel(fwd)) * float(fwd)
    assert not score_holds(got_rev, fwd) and not score_holds(got_fwd, rev)


# ------------------------------------------------------------------------------------------------------------------------
# the branches of the definition
# ------------------------------------------------------------------------------------------------------------------------
def test_branch_anticorrelated(fa):
    """x = -r + 0.1 noise: g < 0 everywhere, so g = 0 and sv = sxx: the score is of order 1e-12 and dx is exactly zero."""
    shape = (1, 1, 48, 56)
    _, r = make_pair(shape, 3)
    x = (-r + 0.1 * torch.randn(shape, generator=torch.Generator().manual_seed(33))).half().float()
    ref = restate(x, r)
    assert ref["max_g"] <= -0.5
    got = run_hip(fa, x, r)
    print("VIF_ERR anticorrelated: score %.6e restatement %.6e max g %.3f" % (got["score"], ref["score"], ref["max_g"]))
    assert 0 < float(ref["score"]) < 1e-10 and score_holds(got["score"], ref["score"])
    assert float(got["dx"].abs().max()) == 0.0 and float(ref["dx"].abs().max()) == 0.0
    assert torch.isfinite(got["dr"]).all() and got["dr"].abs().max() > 0


def test_branch_dark_region(fa):
    """Both images equal ``lo`` on columns >= 60 of (1,1,48,128): every position that sees a pixel of columns >= 101 sees only zeros (the
    reach of a pixel through the four scales is 40 columns), lies in the srr < EPS branch and has zero cotangents."""
    x, r = make_pair((1, 1, 48, 128), 2)
    x[..., 60:] = -1.0
    r[..., 60:] = -1.0
    ref = restate(x, r)
    got = run_hip(fa, x, r)
    assert score_holds(got["score"], ref["score"])
    for k in ("dx", "dr"):
        assert float(got[k][..., 101:].abs().max()) == 0.0 and float(ref[k][..., 101:].abs().max()) == 0.0
        assert torch.isfinite(got[k]).all() and got[k][..., :60].abs().max() > 0


def test_branch_dark_planes(fa):
    """Two all-``lo`` images score 1 with all-zero gradients; an all-``lo`` reference against a textured x scores 1."""
    lo = torch.full((2, 1, 48, 72), -1.0)
    got = run_hip(fa, lo, lo.clone(), per_image=True)
    assert got["score"].tolist() == [1.0, 1.0] and float(got["dx"].abs().max()) == 0.0 and float(got["dr"].abs().max()) == 0.0
    x, _ = make_pair((2, 1, 48, 72), 1)
    got = run_hip(fa, x, lo, per_image=True)
    ref = restate(x, lo, per_image=True, x_grad=False, r_grad=False)
    assert ref["score"].tolist() == [1.0, 1.0] and score_holds(got["score"], ref["score"])
    assert torch.isfinite(got["dx"]).all() and torch.isfinite(got["dr"]).all()


def test_branch_enhancement(fa):
    """V(1.5 r, r) at value_range (0, 1) exceeds 1: 1.10 on the prototype at (1,1,48,56).  An exact multiple of the reference sits on the
    last clamp just as an identical image does: g = 1.5 and sv = sxx - g sxr = 0 exactly, so in fp32 the rounding of sv (a few 1e-2
    either way on variances of 1e4 - 1e5, against sigma_n_sq = 2) decides between sv = EPS and sv = the rounding.  The fp32 restatement
    itself is 0.9e-4 - 1.0e-4 off the float64 one here (by the host's conv2d), some 25 times the fixture's E_ref of 3.7e-6, so E_ref
    takes in the case at hand, as the family's off-fixture bar does; measured on an MI355X: e_hip 1.03e-4, 1.0 - 1.2 of the reference's
    own error (bar 2)."""
    _, r = make_pair((1, 1, 48, 56), 0)
    cfg = dict(DEFAULT, value_range=(0.0, 1.0))
    ref = restate(1.5 * r, r, cfg, x_grad=False, r_grad=False)
    own = score_err(restate(1.5 * r, r, cfg, x_grad=False, r_grad=False, dtype=torch.float32)["score"], ref["score"])
    got = run_hip(fa, 1.5 * r, r, cfg)
    print("VIF_ERR enhancement: score %.9f restatement %.9f e_hip %.3e e_ref (this case) %.3e fixture E_ref %.3e" % (
        got["score"], ref["score"], score_err(got["score"], ref["score"]), own, score_E_ref()))
    assert float(got["score"]) > 1 and 1.05 < float(ref["score"]) < 1.15
    assert score_holds(got["score"], ref["score"], max(score_E_ref(), own))
    assert torch.isfinite(got["dx"]).all() and torch.isfinite(got["dr"]).all()


def test_branch_identical_images(fa):
    """V(t, t) is 1 up to rounding (sv sits on the last clamp): within the score bar of 1, and everything finite."""
    _, r = make_pair((2, 1, 48, 72), 7)
    got = run_hip(fa, r, r.clone(), per_image=True)
    print("VIF_ERR identical: scores %s" % (got["score"].tolist(),))
    assert score_holds(got["score"], torch.ones(2, dtype=torch.float64))
    assert all(torch.isfinite(got[k]).all() for k in got)


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def test_launch_counts(fa, monkeypatch):
    """Five entry points forward (four ``vif_scale_fwd``, ``vif_final``, each one launch) and four backward, coarsest first.  The dx / dr
    pointer, and that side's gradient of the next scale, is null for the input that needs no gradient."""
    x, r = (t.cuda() for t in make_pair((2, 2, 48, 72), 3))
    for x_grad, r_grad in ((True, True), (True, False), (False, True)):
        xd, rd = x.clone().requires_grad_(x_grad), r.clone().requires_grad_(r_grad)
        calls = spy(fa, monkeypatch)
        V = op(fa, xd, rd)
        assert [n for n, _ in calls] == FWD_NAMES and len(calls) <= 5 and calls[-1][1][TABLE_ARG]
        assert [a[FWD_SCALE_ARG] for _, a in calls[:4]] == [0, 1, 2, 3]
        assert all(a[NEXT_X_ARG] and a[NEXT_R_ARG] and a[WS_ARG] for _, a in calls[:3])
        assert calls[3][1][NEXT_X_ARG] is None and calls[3][1][NEXT_R_ARG] is None
        del calls[:]
        V.backward()
        assert [n for n, _ in calls] == BWD_NAMES and len(calls) <= 4
        assert [a[BWD_SCALE_ARG] for _, a in calls] == [3, 2, 1, 0]
        for i, (_, a) in enumerate(calls):
            assert bool(a[DX_ARG]) == x_grad and bool(a[DR_ARG]) == r_grad and a[G_ARG] and a[GTABLE_ARG]
            assert bool(a[DNX_ARG]) == (x_grad and i > 0) and bool(a[DNR_ARG]) == (r_grad and i > 0)
        assert (xd.grad is not None) == x_grad and (rd.grad is not None) == r_grad
        monkeypatch.undo()


def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch):
    N, C, H, W = 2, 3, 48, 72
    x, r = (t.cuda() for t in make_pair((N, C, H, W), 2))
    calls = spy(fa, monkeypatch)
    Vg = op(fa, x.clone().requires_grad_(True), r.clone().requires_grad_(True))
    assert calls[-1][0] == "vif_final" and calls[-1][1][TABLE_ARG]
    # the two images, the pairs of scales 1..3 (a third of the inputs) and the table only
    hs, ws = fa.ops.vif_sides(H), fa.ops.vif_sides(W)
    shapes = [(N, C, hs[s], ws[s]) for s in range(4)]
    assert [tuple(t.shape) for t in Vg.grad_fn.saved_tensors] == shapes * 2 + [(2, N)]
    assert sum(h * w for _, _, h, w in shapes[1:]) * 3 <= H * W
    del calls[:]
    with torch.no_grad():
        Vn = op(fa, x.clone().requires_grad_(True), r.clone().requires_grad_(True))
    assert [n for n, _ in calls] == FWD_NAMES and calls[-1][1][TABLE_ARG] is None        # a null pointer: no table is kept
    assert not Vn.requires_grad and Vn.grad_fn is None
    del calls[:]
    Vp = op(fa, x, r)                                                      # inputs that need no gradient
    assert len(calls) == 5 and calls[-1][1][TABLE_ARG] is None and not Vp.requires_grad
    assert torch.equal(Vn, Vg) and torch.equal(Vp, Vg)


def test_module_and_function_are_the_op(fa):
    x, r = (t.cuda() for t in make_pair((2, 1, 48, 56), 4))
    big = torch.cat((x, x), dim=3)
    vx, vr = big[:, :, :, 56:], torch.cat((r, r), dim=3)[:, :, :, 56:]      # views equal their contiguous copies
    assert not vx.is_contiguous()
    args = (0.4, (0., 2.))
    want, rows = fa.ops.vif(x, r, *args), fa.ops.vif(x, r, *args, True)
    mod = fa.VIF(*args).cuda()
    assert torch.equal(mod(x, r), want) and torch.equal(mod.index(x, r, True), rows)
    assert torch.equal(fa.VIF(*args, size_average=False)(x, r), rows)
    assert torch.equal(fa.ssim.vif(x, r, *args), want)
    assert torch.equal(fa.ssim.vif(x, r, *args, size_average=False), rows)
    assert float(want) == pytest.approx(float(rows.double().mean()), rel=1e-6)
    assert torch.equal(mod(vx, vr), want)
    assert torch.equal(fa.VIF().cuda()(x, r), fa.ops.vif(x, r))


def test_capturable(fa):
    """Forward and backward captured in one hipGraph replay to the eager bits: nothing is allocated or read on the host."""
    x, r = (t.cuda() for t in make_pair((2, 1, 48, 72), 9))
    eager = run_hip(fa, x.cpu(), r.cpu())
    xs = x.clone().requires_grad_(True)
    op(fa, xs, r).backward()                                               # warm-up: the workspace exists before the capture
    xs.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        V = op(fa, xs, r)
        (dx,) = torch.autograd.grad(V, xs)
    V.detach().zero_()
    dx.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(V.detach().cpu(), eager["score"]) and torch.equal(dx.cpu(), eager["dx"])


# ------------------------------------------------------------------------------------------------------------------------
# the evaluation path
# ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pairs_with_key(fa, monkeypatch):
    """The key is the mean of the per-image index of (super_resolve(lr), hr) -- the reconstruction first, the ground truth second --
    against the restatement on two 48 x 56 pairs.  The generator's forward is not bit-reproducible (split-K atomics), so
    ``super_resolve`` is replaced by a fixed map; the four metric columns and the index run their kernels."""
    monkeypatch.setattr(fa.evaluate, "super_resolve", lambda model, lr: (0.9 * lr).contiguous())
    pairs = []
    for seed, n in ((21, 2), (22, 1)):
        lr, hr = make_pair((n, 1, 48, 56), seed)
        pairs.append((lr.cuda(), hr.cuda()))
    plain = fa.evaluate_pairs(None, pairs)
    out = fa.evaluate_pairs_with(None, pairs, vif=fa.VIF().cuda())
    assert list(out) == ["psnr", "ssim", "mse", "nmi", "vif"] and all(out[k] == plain[k] for k in plain)

    def rows_of(dtype, swap=False):
        return torch.cat([restate(*(((0.9 * lr).cpu(), hr.cpu())[::-1 if swap else 1]), per_image=True, x_grad=False, r_grad=False, dtype=dtype)["score"]
                          for lr, hr in pairs])
    rows, rows32 = rows_of(torch.float64), rows_of(torch.float32)
    E_ref = max(score_E_ref(), score_err(rows32, rows))
    want, swapped = float(rows.mean()), float(rows_of(torch.float64, True).mean())
    print("VIF_ERR evaluate_pairs_with: vif %.9f restatement %.9f (arguments swapped %.9f) E_ref %.3e" % (out["vif"], want, swapped, E_ref))
    assert rows.shape == (3,) and want > 0 and abs(out["vif"] - want) <= (K2 * E_ref + ulp_rel(want)) * want
    assert abs(out["vif"] - swapped) > 100 * (K2 * E_ref + ulp_rel(want)) * want


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
def test_train_step_vif_term(fa, O, two_chains, monkeypatch):
    """192^2, batch 1, the smallest step of tests/test_gpu_step.py.  With ``reproducible_forward`` the forward and the losses are
    bit-reproducible, so against the weight-0 step: the tensors and every other loss keep their bits; ``loss_vif`` is the composition
    of the op on the step's own tensors -- 0.5 ((1 - V(recovered_A, real_A)) + (1 - V(recovered_B, real_B))), formed in double from the
    op's fp32 scores; the step forms it in fp32, in the two-chain schedule as two halves: absolute roundings of 2^-24 on values of order
    1, hence 4 * 2^-24 absolute -- and ``loss_G`` is the weight-0 step's plus the term, to fp32 rounding of the sum (1e-6 relative).
    The weight-0 step launches no ``vif_*`` entry and the step with the term launches exactly two forwards and two one-sided backwards
    more; every other entry point keeps its count."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    calls = spy(fa, monkeypatch)
    try:
        tsd = fresh_step(fa, O, reproducible_forward=True)                 # the default step, first: it fills the process-wide tables
        Ld = tsd.step(a, b, sync=True, keep=True)
        ts = fresh_step(fa, O, reproducible_forward=True, vif_weight=0.5)
        del calls[:]
        L = ts.step(a, b, sync=True, keep=True)
        with_term = counted(calls)
        grad_calls = [args for n, args in calls if n == "vif_scale_bwd"]
        ts0 = fresh_step(fa, O, reproducible_forward=True, vif_weight=0.0)
        del calls[:]
        L0 = ts0.step(a, b, sync=True, keep=True)
        without = counted(calls)
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_vif" not in L0 and ts0.vif is None and tsd.vif is None and isinstance(ts.vif, fa.VIF)
    assert L0["loss_G"] == Ld["loss_G"]                                    # weight 0 is the default step, bit for bit
    assert not [n for n in without if n.startswith("vif")]
    assert {n: c for n, c in with_term.items() if n.startswith("vif")} == {"vif_scale_fwd": 8, "vif_final": 2, "vif_scale_bwd": 8}
    assert {n: c for n, c in with_term.items() if not n.startswith("vif")} == without
    assert all(bool(g[DX_ARG]) and not g[DR_ARG] and not g[DNR_ARG] for g in grad_calls)      # the gradient reaches the reconstruction only
    T = L["tensors"]
    for k in ("recovered_A", "recovered_B", "fake_A", "fake_B"):
        assert torch.equal(T[k], L0["tensors"][k]), k
    with torch.no_grad():
        want = 0.5 * sum(1.0 - float(ts.vif(rec, real)) for rec, real in ((T["recovered_A"], a), (T["recovered_B"], b)))
    print("VIF_ERR step two_chains=%s: loss_vif %.7f composition %.7f, loss_G %.6f against %.6f at weight 0" % (
        two_chains, L["loss_vif"], want, L["loss_G"], L0["loss_G"]))
    assert want > 0 and abs(L["loss_vif"] - want) <= 4 * 2.0 ** -24
    assert abs(L["loss_G"] - (L0["loss_G"] + L["loss_vif"])) <= 1e-6 * abs(L["loss_G"])
    for k in ("loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"):
        assert L[k] == L0[k], (k, L[k], L0[k])


def test_graph_captured_step_with_vif_term(fa, O):
    """The step with the term as one captured hipGraph.  With ``reproducible_forward`` the forward of step 0 is bit-reproducible: the
    replay's ``loss_vif`` and ``loss_G`` equal the bits of the eager step in the arrangement the capture uses (chain A on the caller's
    stream)."""
    a, b = (t.cuda() for t in O.synthetic_batch(1, 192))
    keep, saved = fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels
    fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = False, 0
    try:
        eager = fresh_step(fa, O, precision="f32", reproducible_forward=True, vif_weight=0.5)
        Le = eager.step(a, b, sync=True)
        ts = fresh_step(fa, O, precision="f32", reproducible_forward=True, vif_weight=0.5)
        gs = fa.GraphedTrainStep(ts, a, b)
        Lg = gs.step(a, b, sync=True)
    finally:
        fa.TrainStep.eager_chain_A_forked, fa.TrainStep.overlap_min_pixels = keep, saved
    print("VIF_ERR graph step: loss_vif %.9f eager %.9f, loss_G %.9f eager %.9f" % (Lg["loss_vif"], Le["loss_vif"], Lg["loss_G"], Le["loss_G"]))
    assert Lg["loss_vif"] > 0
    assert Lg["loss_vif"] == Le["loss_vif"] and Lg["loss_G"] == Le["loss_G"]      # the eager bits
    assert ts.opt_G.step_count == 1
