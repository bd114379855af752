"""The total-variation loss (reference model.py:17-33) on the MI355X: ``ops.tv_loss`` / ``TVLoss`` against the reference's own
CPU result (tests/golden/golden_tv.npz) and against a float64 restatement of the formula (pinned to that fixture by
tests/test_tv_loss_cpu.py), its exact cases, its semantics, reproducibility, and the opt-in ``TrainStep(tv_weight=...)`` term,
eager and hipGraph-captured.

The error bar is relative to the reference's own error.  With e_ref the fp32 reference's distance from fp64 (the fixture's for
the fixture shapes, the fp32 torch composition's on the CPU for the sweep) and e_hip the kernels':

    loss:      e_hip <= 2 e_ref + 1 ulp            (ulp = |loss| 2^-23)
    gradient:  e_hip <= 2 e_ref + 2^-24            (relative L2)

Where 2 comes from: tools/tv_loss_error_model.py emulates the kernels' summation order in fp32 on the CPU (per-thread running
sums with a fused multiply-add per term, the 64-lane butterfly, the four waves, the final kernel's double sums) over every shape
used here.  Both the emulation and the reference land within an ulp of the float64 value (e_ref 0.13 - 1.02 ulp, emulation
0.11 - 0.29 ulp); the worst ratio emulation / e_ref is 1.000 for the loss (0.21 - 1.00) and 1.002 for the gradient (0.80 - 1.002),
and twice the worst ratio is the margin, for a block order or a contraction the emulation does not model and for an e_ref that
is luckily small.  The floors keep the bar satisfiable when e_ref is zero: one ulp of the loss (its final rounding from double
alone is half of one), and for the gradient half an ulp relative (one rounding of each element).
Measured on an MI355X: loss within 0.29 ulp of float64 on every case, gradient at 0.80x - 1.002x of e_ref.
Figures: profiles/tv_loss_error.txt (the phase loss's bar, 8 e_ref + 2 ulp, was the one to beat)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_tv.npz")
TIGHT = ("loss_G", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")
K_LOSS, FLOOR_LOSS_ULPS = 2.0, 1.0
K_GRAD, FLOOR_GRAD = 2.0, 2.0 ** -24


def restatement(x, weight=1.0, dtype=torch.float64):
    """The reference's formula with stock ops on the CPU in ``dtype``: (loss, dloss/dx) as float64."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    b, c, h, w = x.shape
    h_tv = ((x[:, :, 1:, :] - x[:, :, :h - 1, :]) ** 2).sum()
    w_tv = ((x[:, :, :, 1:] - x[:, :, :, :w - 1]) ** 2).sum()
    loss = weight * 2 * (h_tv / (c * (h - 1) * w) + w_tv / (c * h * (w - 1))) / b
    g, = torch.autograd.grad(loss, x)
    return loss.detach().double(), g.double()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def image(B, C, H, W, seed):
    return torch.tanh(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)))


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def hip(fa, x, weight=1.0, want_grad=True):
    """(loss, dx) of ops.tv_loss on the GPU, back on the host (dx is None when no gradient was asked for)."""
    xd = x.cuda().requires_grad_(want_grad)
    loss = fa.ops.tv_loss(xd, weight)
    assert loss.shape == () and loss.dtype == torch.float32
    if want_grad:
        loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), (xd.grad.cpu() if want_grad else None)


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio for the loss and the gradient, then assert the bar of the module docstring."""
    ulp = abs(float(ref64[0])) * 2.0 ** -23
    e_ref = [abs(float(ref32[0]) - float(ref64[0])), rel_l2(ref32[1], ref64[1])]
    e_hip = [abs(float(got[0]) - float(ref64[0])), rel_l2(got[1], ref64[1])]
    print("TV_ERR %-26s loss %.7f e_ref %.3e (%.2f ulp) e_hip %.3e (%.2f ulp) | grad e_ref %.3e e_hip %.3e ratio %.3f  (|g| %.3e)"
          % (name, float(ref64[0]), e_ref[0], e_ref[0] / ulp, e_hip[0], e_hip[0] / ulp, e_ref[1], e_hip[1], e_hip[1] / e_ref[1], float(ref64[1].norm())))
    assert e_hip[0] <= K_LOSS * e_ref[0] + FLOOR_LOSS_ULPS * ulp, (name, "loss", e_hip[0], e_ref[0], ulp)
    assert e_hip[1] <= K_GRAD * e_ref[1] + FLOOR_GRAD, (name, "gradient", e_hip[1], e_ref[1])


def test_fixture_parity(fa):
    """The reference's own inputs, weights 1 and 0.5: e_ref is the fixture's (reference, fp32, CPU) error against fp64."""
    g = np.load(GOLD)
    for shape in g["shapes"]:
        tag = "%dx%dx%dx%d" % tuple(shape)
        x = torch.from_numpy(g["x_" + tag])
        for w in g["weights"]:
            ref32 = (torch.from_numpy(g["loss_w%g_%s" % (w, tag)]), torch.from_numpy(g["g_w%g_%s" % (w, tag)]))
            hold_to_bar("fixture %s w%g" % (tag, w), restatement(x, float(w)), ref32, hip(fa, x, float(w)))


@pytest.mark.parametrize("B,C,H,W", [(8, 1, 256, 256), (2, 1, 192, 192), (3, 1, 63, 50), (2, 2, 96, 64), (1, 1, 2, 2), (1, 1, 2, 257),
                                     (1, 1, 130, 2)])
def test_shape_sweep(fa, B, C, H, W):
    """Vector and scalar paths, odd widths, H or W of 2; e_ref from the fp32 torch composition on the CPU; through the module."""
    x = image(B, C, H, W, seed=77 + H + 3 * C + W)
    xd = x.cuda().requires_grad_(True)
    loss = fa.TVLoss()(xd)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    hold_to_bar("B%d C%d %dx%d" % (B, C, H, W), restatement(x), restatement(x, dtype=torch.float32), (loss.detach().cpu(), xd.grad.cpu()))


@pytest.mark.parametrize("B,C,H,W", [(2, 1, 64, 64), (3, 2, 33, 50), (1, 1, 2, 2)])
def test_constant_image_is_exactly_zero(fa, B, C, H, W):
    loss, g = hip(fa, torch.full((B, C, H, W), 0.37))
    assert float(loss) == 0.0
    assert bool((g == 0).all())


@pytest.mark.parametrize("B,C,H,W,a,b,weight", [(1, 1, 64, 64, 0.5, 0.25, 1.0), (3, 2, 40, 48, 0.125, 2.0, 0.5), (2, 3, 33, 50, 0.25, 0.0625, 1.0),
                                                (5, 1, 2, 2, 1.0, 0.5, 0.5)])
def test_ramp_is_exact(fa, B, C, H, W, a, b, weight):
    """x[.,.,i,j] = a i + b j with a, b powers of two: every difference is exactly a or b, every partial sum an integer multiple of
    a^2 or b^2 below 2^24 of them, so the loss is exactly weight 2 (a^2 + b^2), for any B and C."""
    i = torch.arange(H, dtype=torch.float32)[:, None]
    j = torch.arange(W, dtype=torch.float32)[None, :]
    x = (a * i + b * j).expand(B, C, H, W).contiguous()
    loss, _ = hip(fa, x, weight)
    assert float(loss) == weight * 2 * (a * a + b * b), (float(loss), weight * 2 * (a * a + b * b))


def test_weight_scales_and_module_is_the_op(fa):
    x = image(2, 2, 96, 64, seed=11)
    one, g_one = hip(fa, x, 1.0)
    half, g_half = hip(fa, x, 0.5)
    assert float(half) == 0.5 * float(one)                       # a power of two: exact
    assert torch.equal(g_half, 0.5 * g_one)
    for w in (1, 0.5):
        xd = x.cuda().requires_grad_(True)
        crit = fa.TVLoss(TVLoss_weight=w)
        assert crit.TVLoss_weight == w
        loss = crit(xd)
        loss.backward()
        want, g_want = hip(fa, x, float(w))
        assert torch.equal(loss.detach().cpu(), want) and torch.equal(xd.grad.cpu(), g_want)


def test_non_contiguous_view_equals_its_copy(fa):
    big = image(2, 2, 70, 90, seed=13).cuda()
    for view in (big[:, :, 3:67, 5:69], big.transpose(2, 3), big[:, :, ::2, 1:51]):
        assert not view.is_contiguous()
        v = view.detach().requires_grad_(True)
        c = view.detach().contiguous().requires_grad_(True)
        lv, lc = fa.ops.tv_loss(v), fa.ops.tv_loss(c)
        lv.backward()
        lc.backward()
        assert torch.equal(lv, lc) and torch.equal(v.grad, c.grad)


def test_input_without_gradient(fa):
    x = image(3, 1, 63, 50, seed=17)
    with_grad, _ = hip(fa, x)
    without, none = hip(fa, x, want_grad=False)
    assert none is None and torch.equal(with_grad, without)
    # a graph in which another leaf needs a gradient and the TV input does not: backward runs and skips the stencil launch
    xd = x.cuda()
    s = torch.ones((), device="cuda", requires_grad=True)
    (fa.ops.tv_loss(xd) * s).backward()
    torch.cuda.synchronize()
    assert float(s.grad) == float(with_grad) and xd.grad is None


def test_bit_reproducible_and_independent_of_conv_precision(fa):
    x = image(8, 1, 256, 256, seed=33)
    first = hip(fa, x)
    again = hip(fa, x)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    saved = fa.ops.conv_precision
    try:
        for prec in (0, 3):
            fa.ops.conv_precision = prec
            got = hip(fa, x)
            assert all(torch.equal(a, b) for a, b in zip(first, got)), prec
    finally:
        fa.ops.conv_precision = saved


def test_runs_on_the_current_stream(fa):
    x = image(2, 1, 64, 64, seed=41)
    want = hip(fa, x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = hip(fa, x)
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(a, b) for a, b in zip(want, got))


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
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_train_step_tv_term(fa, O, precision, two_chains):
    """192^2, batch 2: the term is what the restatement gives on the step's own fakes, it is what loss_G gains, it moves the
    generators' gradient, and a weight-0 step does not know it.  Both places the opt-in terms live: the two-chain schedule and
    the single-stream ``generator_loss``."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    try:
        ts = fresh_step(fa, O, precision=precision, tv_weight=0.5)
        L = ts.step(a, b, sync=True, keep=True)
        gn = ts.grad_norms()
        ts0 = fresh_step(fa, O, precision=precision)
        L0 = ts0.step(a, b, sync=True, keep=True)
        gn0 = ts0.grad_norms()
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_tv" not in L0
    T = L["tensors"]
    want = 0.5 * (float(restatement(T["fake_B"])[0]) + float(restatement(T["fake_A"])[0]))
    print("TV_ERR step %s two_chains=%s: loss_tv %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0, |grad A2B| %.5f against %.5f, |grad B2A| %.5f against %.5f"
          % (precision, two_chains, L["loss_tv"], want, L["loss_G"], L0["loss_G"], gn["A2B"], gn0["A2B"], gn["B2A"], gn0["B2A"]))
    assert abs(L["loss_tv"] - want) <= 1e-3 * abs(want)
    assert abs((L["loss_G"] - L0["loss_G"]) - L["loss_tv"]) <= 1e-3 * abs(L["loss_G"])
    assert abs(gn["A2B"] - gn0["A2B"]) > 1e-3 * gn0["A2B"] or abs(gn["B2A"] - gn0["B2A"]) > 1e-3 * gn0["B2A"], (gn, gn0)
    for k in L0:
        if k not in ("tensors", "loss_G"):
            assert abs(L[k] - L0[k]) <= 1e-3 * max(abs(L0[k]), 2e-2), (k, L[k], L0[k])


def test_graph_captured_step_with_tv_term(fa, O):
    """The step with the TV term as one captured hipGraph: three replays follow the eager step at the bars of the existing
    graph test (2e-4 relative at step 0; later 3e-3 on the tight losses, 0.03 / 0.06 absolute on the others)."""
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    eager = fresh_step(fa, O, precision="f32", tv_weight=0.5)
    Le = [eager.step(a, b, sync=True) for a, b in batches]
    ts = fresh_step(fa, O, precision="f32", tv_weight=0.5)
    gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
    Lg = [gs.step(a, b, sync=True) for a, b in batches]
    for s in range(3):
        print("TV_ERR graph step %d: loss_tv %.7f eager %.7f, loss_G %.6f eager %.6f" % (s, Lg[s]["loss_tv"], Le[s]["loss_tv"], Lg[s]["loss_G"], Le[s]["loss_G"]))
        for k in ("loss_tv", "loss_G"):
            tol = 2e-4 if s == 0 else (3e-3 if k in TIGHT else None)
            if tol is not None:
                assert Lg[s][k] == pytest.approx(Le[s][k], rel=tol, abs=1e-6), (s, k, Lg[s][k], Le[s][k])
            else:
                assert Lg[s][k] == pytest.approx(Le[s][k], abs=0.03 if s == 1 else 0.06), (s, k)
    assert ts.opt_G.step_count == 3
