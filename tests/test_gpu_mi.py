"""The differentiable mutual information on the MI355X: ``ops.mutual_information`` against the float64 torch restatement of its
definition (pinned to tests/golden/golden_mi.npz by tests/test_mi_cpu.py), its bit-for-bit properties, and the opt-in
``TrainStep(mi_weight=...)`` term, eager in both schedules and hipGraph-captured.

The error bar is relative to the error of the fp32 run of the same restatement (softmax, bmm, autograd) on the CPU against
float64:
  * each gradient, in relative L2:  e_hip <= 8 e_ref  (e_ref is 3.0e-7 - 1.4e-6 over the fixture, never accidentally tiny);
  * the score:  |S_hip - S_64| <= 8 r |S_64| + one fp32 ulp of S_64, with r the largest relative score error of the fp32 run
    over the fixture's cases (3.1e-6; one case's own error can be near zero by accident).
The factor 8 is the bar tests/test_gpu_phase_loss.py and tests/test_gpu_ffl.py hold the other GEMM-reduction paths to.
Mutual information is a difference of entropies, so every comparison first asserts that each plane carries at least 0.03 nats
in float64.  Figures of one run: profiles/mi_error.txt."""
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_mi.npz")
TIGHT = ("loss_G", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")
SETTINGS = ((32, 1.0), (64, 0.5), (24, 1.0), (40, 0.75))
ALL = tuple((k, s, n) for k, s in SETTINGS for n in (False, True))
FIXTURE_SHAPES = ((2, 1, 7, 9), (1, 1, 33, 31), (3, 1, 63, 50), (2, 2, 96, 64))
GUARD = 0.03
MI_STEP_WEIGHT = 1000.0


def restatement(x, y, bins=32, sigma_ratio=1.0, normalized=False, dtype=torch.float64, value_range=(-1.0, 1.0), eps=1e-6, per_image=False):
    """The literal definition with softmax, bmm and autograd on the CPU in ``dtype``: (score, dS/dx, dS/dy, per-plane MI) as
    float64; with ``per_image`` the score is (N,) and the gradients are those of its sum."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    N, C, H, W = x.shape
    lo, hi = value_range
    d = (hi - lo) / bins
    c = lo + (torch.arange(bins, dtype=dtype) + 0.5) * d
    sigma = sigma_ratio * d

    def weights(v):
        return torch.softmax(-(v.reshape(N * C, H * W, 1) - c) ** 2 / (2 * sigma ** 2), dim=-1)

    P = torch.bmm(weights(x).transpose(1, 2), weights(y)) / (H * W)
    pa, pb = P.sum(2), P.sum(1)
    Ha = -(pa * torch.log(pa + eps)).sum(1)
    Hb = -(pb * torch.log(pb + eps)).sum(1)
    Hab = -(P * torch.log(P + eps)).sum((1, 2))
    mi = Ha + Hb - Hab
    planes = (Ha + Hb) / Hab if normalized else mi
    score = planes.reshape(N, C).mean(1) if per_image else planes.mean()
    gx, gy = torch.autograd.grad(score.sum(), (x, y))
    return score.detach().double(), gx.double(), gy.double(), mi.detach().double()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tag_of(shape, bins, sigma_ratio, normalized):
    return "%s_k%d_s%g_n%d" % ("x".join(str(s) for s in shape), bins, sigma_ratio, int(normalized))


def pair(shape, seed):
    """The fixture's recipe: a smooth image and a nonlinear intensity map of it plus noise."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(*shape, generator=g)
    x = torch.clamp(2 * F.avg_pool2d(n, 5, stride=1, padding=2), -1, 1)
    y = torch.clamp(0.8 * x ** 3 - 0.1 + 0.15 * torch.randn(*shape, generator=g), -1, 1)
    return x, y


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def score_r(gold):
    """The largest relative score error of the fp32 reference over the file's cases."""
    r = 0.0
    for shape in gold["shapes"]:
        for k, s, n in ALL:
            t = tag_of(tuple(shape), k, s, n)
            r = max(r, abs(float(gold["score32_" + t]) - float(gold["score64_" + t])) / abs(float(gold["score64_" + t])))
    assert 1e-7 < r < 1e-5
    return r


def fixture_pair(gold, shape):
    case = "x".join(str(s) for s in shape)
    return torch.from_numpy(gold["x_" + case]), torch.from_numpy(gold["y_" + case])


def hip(fa, x, y, setting=ALL[0], want_x=True, want_y=True, g=None, **kw):
    """(score, dx, dy) of ops.mutual_information on the GPU, back on the host (a gradient that was not asked for is None)."""
    xd = x.cuda().requires_grad_(want_x)
    yd = y.cuda().requires_grad_(want_y)
    s = fa.ops.mutual_information(xd, yd, bins=setting[0], sigma_ratio=setting[1], normalized=setting[2], **kw)
    assert s.dtype == torch.float32 and s.shape == ((x.shape[0],) if kw.get("per_image") else ())
    if want_x or want_y:
        s.sum().backward(None if g is None else torch.tensor(g, device="cuda"))
    torch.cuda.synchronize()
    return s.detach().cpu(), (xd.grad.cpu() if want_x else None), (yd.grad.cpu() if want_y else None)


def score_bar(s64, r):
    return 8 * r * abs(float(s64)) + float(np.spacing(np.float32(abs(float(s64)))))


def hold_to_bar(name, ref64, e_ref_x, e_ref_y, got, r):
    """Assert the conditioning guard, print e_ref, e_hip and their ratio for the score and both gradients, then assert the bar of
    the module docstring."""
    assert float(ref64[3].min()) >= GUARD, (name, ref64[3])
    e_s = abs(float(got[0]) - float(ref64[0]))
    e_gx, e_gy = rel_l2(got[1], ref64[1]), rel_l2(got[2], ref64[2])
    print("MI_ERR %-34s score %.9e rel err %.3e (bar %.3e) | gx e_ref %.3e e_hip %.3e ratio %.2f | gy e_ref %.3e e_hip %.3e ratio %.2f  (min plane MI %.4f)"
          % (name, float(got[0]), e_s / abs(float(ref64[0])), score_bar(ref64[0], r) / abs(float(ref64[0])), e_ref_x, e_gx, e_gx / e_ref_x,
             e_ref_y, e_gy, e_gy / e_ref_y, float(ref64[3].min())))
    assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    assert e_s <= score_bar(ref64[0], r), (name, "score", float(got[0]), float(ref64[0]))
    assert e_gx <= 8 * e_ref_x, (name, "gx", e_gx, e_ref_x)
    assert e_gy <= 8 * e_ref_y, (name, "gy", e_gy, e_ref_y)


@pytest.mark.parametrize("shape", FIXTURE_SHAPES)
def test_fixture_parity(fa, gold, score_r, shape):
    """The fixture's inputs at the four settings, MI and NMI: 63 pixels (less than one chain), an odd plane, several chains plus
    a remainder, and 6144 pixels (three full blocks' worth of chains) in two channels; one tile, four full tiles, padded bins in
    one tile and in two per axis.  e_ref is the file's (the fp32 restatement against float64)."""
    x, y = fixture_pair(gold, shape)
    for k, s, n in ALL:
        t = tag_of(shape, k, s, n)
        ref64 = restatement(x, y, k, s, n)
        assert abs(float(ref64[0]) - float(gold["score64_" + t])) <= 1e-12 * abs(float(ref64[0]))
        hold_to_bar("fixture " + t, ref64, float(gold["gxerr32_" + t]), float(gold["gyerr32_" + t]), hip(fa, x, y, (k, s, n)), score_r)


@pytest.fixture(scope="module")
def big():
    return pair((2, 1, 256, 256), seed=256)


@pytest.mark.parametrize("setting", ALL)
def test_parity_at_256(fa, big, score_r, setting):
    """(2,1,256,256): 32 blocks per plane, every wave's chain full; through the module.  e_ref from the fp32 restatement here."""
    x, y = big
    k, s, n = setting
    crit = fa.MutualInformationLoss(bins=k, sigma_ratio=s, normalized=n)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    score = crit(xd, yd)
    assert score.dim() == 0 and score.dtype == torch.float32
    score.backward()
    ref64, ref32 = restatement(x, y, k, s, n), restatement(x, y, k, s, n, dtype=torch.float32)
    hold_to_bar(tag_of(x.shape, k, s, n), ref64, rel_l2(ref32[1], ref64[1]), rel_l2(ref32[2], ref64[2]),
                (score.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()), score_r)


@pytest.mark.parametrize("normalized", [False, True])
def test_bit_for_bit_properties(fa, normalized):
    """On (2,1,65,70), K = 40 (two tiles per axis with padded bins; two blocks per plane, the second with a remainder): two calls
    agree; S(x, y) == S(y, x) with swapped gradients; halving the upstream gradient halves dx and dy; a gradient asked for alone
    equals the pair's; the convolution precision setting does not matter; the side stream gives the same bits."""
    x, y = pair((2, 1, 65, 70), seed=5)
    st = (40, 0.75, normalized)
    first = hip(fa, x, y, st)
    assert float(first[0]) > 0 and torch.isfinite(first[1]).all() and first[1].any() and first[2].any()
    again = hip(fa, x, y, st)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    swapped = hip(fa, y, x, st)
    assert torch.equal(swapped[0], first[0]) and torch.equal(swapped[1], first[2]) and torch.equal(swapped[2], first[1])
    half = hip(fa, x, y, st, g=0.5)
    assert torch.equal(half[0], first[0]) and torch.equal(half[1], 0.5 * first[1]) and torch.equal(half[2], 0.5 * first[2])
    only_x, only_y = hip(fa, x, y, st, want_y=False), hip(fa, x, y, st, want_x=False)
    assert only_x[2] is None and only_y[1] is None
    assert torch.equal(only_x[0], first[0]) and torch.equal(only_y[0], first[0])
    assert torch.equal(only_x[1], first[1]) and torch.equal(only_y[2], first[2])
    saved = fa.ops.conv_precision
    try:
        for prec in (0, 3):
            fa.ops.conv_precision = prec
            got = hip(fa, x, y, st)
            assert all(torch.equal(a, b) for a, b in zip(first, got)), prec
    finally:
        fa.ops.conv_precision = saved
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = hip(fa, x, y, st)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(first, got))


def test_nothing_saved_without_a_gradient(fa, monkeypatch):
    """Under ``no_grad``, and for inputs that need no gradient, the forward is handed no table and keeps no graph."""
    x, y = pair((2, 1, 63, 50), seed=9)
    want = hip(fa, x, y)[0]
    tables = []
    real = fa.ops.call

    def spy(name, *args):
        if name == "mi_fwd":
            tables.append(args[3])
        return real(name, *args)
    monkeypatch.setattr(fa.ops, "call", spy)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    with torch.no_grad():
        s_n = fa.ops.mutual_information(xd, yd)
    s_p = fa.ops.mutual_information(xd.detach(), yd.detach())
    s_g = fa.ops.mutual_information(xd, yd.detach())
    assert tables[0] is None and tables[1] is None and tables[2] is not None
    assert s_n.grad_fn is None and not s_n.requires_grad and s_p.grad_fn is None and not s_p.requires_grad and s_g.requires_grad
    assert torch.equal(s_n.cpu(), want) and torch.equal(s_p.cpu(), want) and torch.equal(s_g.detach().cpu(), want)


@pytest.mark.parametrize("normalized", [False, True])
def test_per_image(fa, gold, score_r, normalized):
    """``per_image`` equals the per-sample calls bit for bit -- score and gradients under an all-ones upstream gradient -- and
    for C = 2 it is the mean over the two channels' planes (against the restatement, at the bars)."""
    x, y = fixture_pair(gold, (2, 2, 96, 64))
    st = (32, 1.0, normalized)
    s, gx, gy = hip(fa, x, y, st, per_image=True)
    for i in range(2):
        si, gxi, gyi = hip(fa, x[i:i + 1], y[i:i + 1], st)
        assert torch.equal(s[i], si) and torch.equal(gx[i:i + 1], gxi) and torch.equal(gy[i:i + 1], gyi)
    ref64 = restatement(x, y, *st, per_image=True)
    ref32 = restatement(x, y, *st, dtype=torch.float32, per_image=True)
    assert float(ref64[3].min()) >= GUARD
    for i in range(2):
        assert abs(float(s[i]) - float(ref64[0][i])) <= score_bar(ref64[0][i], score_r), i
    want = restatement(x[:1, :1], y[:1, :1], *st)[0] / 2 + restatement(x[:1, 1:], y[:1, 1:], *st)[0] / 2
    assert abs(float(ref64[0][0]) - float(want)) <= 1e-12
    e_x, e_y = rel_l2(ref32[1], ref64[1]), rel_l2(ref32[2], ref64[2])
    print("MI_ERR per_image n%d: gx e_ref %.3e e_hip %.3e | gy e_ref %.3e e_hip %.3e" % (normalized, e_x, rel_l2(gx, ref64[1]), e_y, rel_l2(gy, ref64[2])))
    assert rel_l2(gx, ref64[1]) <= 8 * e_x and rel_l2(gy, ref64[2]) <= 8 * e_y
    g = torch.tensor([0.25, -2.0], device="cuda")
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    fa.ops.mutual_information(xd, yd, normalized=normalized, per_image=True).backward(g)
    assert torch.equal(xd.grad.cpu()[0], 0.25 * gx[0]) and torch.equal(yd.grad.cpu()[1], -2.0 * gy[1])


@pytest.mark.parametrize("setting", [(32, 1.0, False), (64, 0.5, True)])
def test_out_of_range_values(fa, score_r, setting):
    """An image pair scaled to [-3, 3] with the default range (-1, 1): two thirds of the values lie outside it, up to 64 bin
    widths away.  Scores and gradients are finite and within the same bars."""
    x, y = pair((2, 1, 63, 50), seed=21)
    x, y = 3 * x, 3 * y
    assert float(x.abs().max()) > 2 and float((x.abs() > 1).float().mean()) > 0.1
    ref64, ref32 = restatement(x, y, *setting), restatement(x, y, *setting, dtype=torch.float32)
    got = hip(fa, x, y, setting)
    assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    hold_to_bar("out of range " + tag_of(x.shape, *setting), ref64, rel_l2(ref32[1], ref64[1]), rel_l2(ref32[2], ref64[2]), got, score_r)


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
def test_train_step_mi_term(fa, O, two_chains):
    """192^2, batch 2: the term is what the restatement gives on the step's own fakes against their sources, it is what loss_G
    gains, it moves a generator's gradient, and a weight-0 step does not know it.  Both places the term lives: the two-chain
    schedule (next to ``loss_tv``) and the single-stream ``generator_loss``.  The weight is 1000 because the score's gradient
    carries 1 / (planes * n_pix) and the untrained generators' gradient norms are ~100: the other keys are held equal at 1e-3,
    so a gradient norm counts as moved only beyond that same resolution, which a weight of order 1 cannot reach here (the
    forward values of a first step do not depend on the weight).  The untrained fakes share ~0.002 nats with their sources, below
    the conditioning guard of the parity tests; it does not apply here, where the quantity compared is U - S (~3.46 per pair)."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    try:
        ts = fresh_step(fa, O, precision="f16x2", mi_weight=MI_STEP_WEIGHT)
        L = ts.step(a, b, sync=True, keep=True)
        gn = ts.grad_norms()
        ts0 = fresh_step(fa, O, precision="f16x2")
        L0 = ts0.step(a, b, sync=True, keep=True)
        gn0 = ts0.grad_norms()
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_mi" not in L0 and ts0.mi is None
    T = L["tensors"]
    U = math.log(32)
    ref_B, ref_A = restatement(T["fake_B"], a), restatement(T["fake_A"], b)
    want = MI_STEP_WEIGHT * ((U - float(ref_B[0])) + (U - float(ref_A[0])))
    print("MI_ERR step two_chains=%s: plane MI of (fake_B, real_A) %s, of (fake_A, real_B) %s" % (two_chains, ref_B[3].tolist(), ref_A[3].tolist()))
    print("MI_ERR step two_chains=%s: loss_mi %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0, |grad A2B| %.5f against %.5f, |grad B2A| %.5f against %.5f"
          % (two_chains, L["loss_mi"], want, L["loss_G"], L0["loss_G"], gn["A2B"], gn0["A2B"], gn["B2A"], gn0["B2A"]))
    assert want > 0 and abs(L["loss_mi"] - want) <= 1e-3 * abs(want)
    assert abs((L["loss_G"] - L0["loss_G"]) - L["loss_mi"]) <= 1e-3 * abs(L["loss_G"])
    assert abs(gn["A2B"] - gn0["A2B"]) > 1e-3 * gn0["A2B"] or abs(gn["B2A"] - gn0["B2A"]) > 1e-3 * gn0["B2A"], (gn, gn0)
    for k in L0:
        if k not in ("tensors", "loss_G"):
            assert abs(L[k] - L0[k]) <= 1e-3 * max(abs(L0[k]), 2e-2), (k, L[k], L0[k])


def test_graph_captured_step_with_mi_term(fa, O):
    """The step with the mutual-information term as one captured hipGraph: three replays follow the eager step at the bars of
    the existing graph tests (2e-4 relative at step 0; later 3e-3 on the tight losses, 0.03 / 0.06 absolute on the others)."""
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    eager = fresh_step(fa, O, precision="f32", mi_weight=0.5)
    Le = [eager.step(a, b, sync=True) for a, b in batches]
    ts = fresh_step(fa, O, precision="f32", mi_weight=0.5)
    gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
    Lg = [gs.step(a, b, sync=True) for a, b in batches]
    for s in range(3):
        print("MI_ERR graph step %d: loss_mi %.7f eager %.7f, loss_G %.6f eager %.6f" % (s, Lg[s]["loss_mi"], Le[s]["loss_mi"], Lg[s]["loss_G"], Le[s]["loss_G"]))
        for k in ("loss_mi", "loss_G"):
            tol = 2e-4 if s == 0 else (3e-3 if k in TIGHT else None)
            if tol is not None:
                assert Lg[s][k] == pytest.approx(Le[s][k], rel=tol, abs=1e-6), (s, k, Lg[s][k], Le[s][k])
            else:
                assert Lg[s][k] == pytest.approx(Le[s][k], abs=0.03 if s == 1 else 0.06), (s, k)
    assert ts.opt_G.step_count == 3
