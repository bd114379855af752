"""The spectral phase-consistency loss (reference model.py:36-58) on the MI355X: ``ops.phase_loss`` against the reference's own
CPU result (tests/golden/golden_phase.npz) and against a float64 ``torch.fft`` restatement of the formula (pinned to that
fixture by tests/test_phase_loss_cpu.py), its batch / channel / radius semantics, reproducibility, and the opt-in
``TrainStep(phase_weight=...)`` term, eager and hipGraph-captured.

The error bar is relative to the reference's own error: with e_ref the fp32 reference's distance from fp64 and e_hip the
kernels', the loss must satisfy e_hip <= 8 e_ref + 2.4e-7 (two fp32 ulps at |loss| ~ 1) and each gradient, in relative L2,
e_hip <= 8 e_ref.  Why 8: the rounding of a DFT done as a GEMM grows like sqrt(n) against the FFT's log n -- on the CPU in fp32
the GEMM form measured 0.8x - 3.5x of the reference's error -- doubled for the MFMA's different accumulation order.
Figures of one run: profiles/r06_phase_loss_error.txt."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_phase.npz")
TIGHT = ("loss_G", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")


def restatement(x, y, radius=5.0, dtype=torch.float64):
    """The reference's formula with stock ops on the CPU in ``dtype``, per sample and averaged over the batch:
    (loss, dloss/dx, dloss/dy) as float64.  The mask is built in double and rounded once, as the reference does."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    B, C, H, W = x.shape
    i = torch.arange(H, dtype=torch.float64)[:, None] - H // 2
    j = torch.arange(W, dtype=torch.float64)[None, :] - W // 2
    m = (1 - torch.exp(-0.5 * (i * i + j * j) / radius ** 2)).to(dtype)
    total = 0
    for b in range(B):
        ax = (m * torch.log(torch.abs(torch.fft.fftshift(torch.fft.fft2(x[b]), dim=(-2, -1))))).flatten()
        ay = (m * torch.log(torch.abs(torch.fft.fftshift(torch.fft.fft2(y[b]), dim=(-2, -1))))).flatten()
        total = total - torch.cosine_similarity(ax, ay, dim=0)
    loss = total / B
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach().double(), gx.double(), gy.double()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def pair(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(B, C, H, W, generator=g))
    y = torch.tanh(x + 0.3 * torch.randn(B, C, H, W, generator=g))
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


def hip(fa, x, y, radius=5.0, want_x=True, want_y=True):
    """(loss, dx, dy) of ops.phase_loss on the GPU, back on the host (a gradient that was not asked for is None)."""
    xd = x.cuda().requires_grad_(want_x)
    yd = y.cuda().requires_grad_(want_y)
    loss = fa.ops.phase_loss(xd, yd, radius)
    assert loss.shape == () and loss.dtype == torch.float32
    if want_x or want_y:
        loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), (xd.grad.cpu() if want_x else None), (yd.grad.cpu() if want_y else None)


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio for the loss and both gradients, then assert the bar of the module docstring."""
    e_ref = [abs(float(ref32[0]) - float(ref64[0])), rel_l2(ref32[1], ref64[1]), rel_l2(ref32[2], ref64[2])]
    e_hip = [abs(float(got[0]) - float(ref64[0])), rel_l2(got[1], ref64[1]), rel_l2(got[2], ref64[2])]
    print("PHASE_ERR %-22s loss e_ref %.3e e_hip %.3e | gx e_ref %.3e e_hip %.3e ratio %.2f | gy e_ref %.3e e_hip %.3e ratio %.2f  (|gx| %.3e)"
          % (name, e_ref[0], e_hip[0], e_ref[1], e_hip[1], e_hip[1] / e_ref[1], e_ref[2], e_hip[2], e_hip[2] / e_ref[2], float(ref64[1].norm())))
    assert e_hip[0] <= 8 * e_ref[0] + 2.4e-7, (name, "loss", e_hip[0], e_ref[0])
    assert e_hip[1] <= 8 * e_ref[1], (name, "gx", e_hip[1], e_ref[1])
    assert e_hip[2] <= 8 * e_ref[2], (name, "gy", e_hip[2], e_ref[2])


def test_fixture_parity(fa):
    """The reference's own inputs: e_ref is the fixture's (reference, fp32, CPU) error against fp64."""
    g = np.load(GOLD)
    for H, W in g["shapes"]:
        tag = "%dx%d" % (H, W)
        x, y = torch.from_numpy(g["x_" + tag]), torch.from_numpy(g["y_" + tag])
        ref32 = (torch.from_numpy(g["loss_" + tag]), torch.from_numpy(g["gx_" + tag]), torch.from_numpy(g["gy_" + tag]))
        hold_to_bar("fixture " + tag, restatement(x, y), ref32, hip(fa, x, y))


@pytest.mark.parametrize("B,C,H,W,radius", [(8, 1, 256, 256, 5.0), (2, 1, 192, 192, 5.0), (3, 1, 63, 50, 5.0), (2, 2, 96, 64, 5.0),
                                            (2, 1, 64, 64, 3.0), (2, 1, 64, 64, 12.0)])
def test_shapes_and_semantics(fa, B, C, H, W, radius):
    """e_ref from the fp32 torch.fft composition on the CPU; the module through its ``radius`` attribute."""
    x, y = pair(B, C, H, W, seed=77 + H + 3 * C + int(radius))
    crit = fa.phase_consistency_loss()
    crit.radius = radius
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    loss = crit(xd, yd)
    assert loss.dim() == 0
    loss.backward()
    got = (loss.detach().cpu(), xd.grad.cpu(), yd.grad.cpu())
    hold_to_bar("B%d C%d %dx%d r%g" % (B, C, H, W, radius), restatement(x, y, radius), restatement(x, y, radius, torch.float32), got)


def test_identical_inputs_give_minus_one(fa):
    x, y = pair(2, 1, 64, 64, seed=5)
    loss, gx, _ = hip(fa, x, x.clone())
    assert abs(float(loss) + 1.0) <= 2.4e-7, float(loss)
    _, gx_ind, _ = hip(fa, x, y)
    print("PHASE_ERR y = x: loss + 1 = %.3e, |gx| %.3e against %.3e for an independent y" % (float(loss) + 1.0, float(gx.norm()), float(gx_ind.norm())))
    assert float(gx.norm()) < 1e-5 * float(gx_ind.norm())


def test_gradient_to_either_input_alone(fa):
    x, y = pair(2, 1, 63, 50, seed=9)
    l_b, gx_b, gy_b = hip(fa, x, y)
    l_x, gx, none_y = hip(fa, x, y, want_y=False)
    l_y, none_x, gy = hip(fa, x, y, want_x=False)
    assert none_x is None and none_y is None
    assert torch.equal(l_b, l_x) and torch.equal(l_b, l_y)
    assert torch.equal(gx, gx_b) and torch.equal(gy, gy_b)


def test_batch_is_the_mean_of_the_samples(fa):
    x, y = pair(8, 1, 256, 256, seed=21)
    whole, _, _ = hip(fa, x, y, want_x=False, want_y=False)
    singles = [float(hip(fa, x[b:b + 1], y[b:b + 1], want_x=False, want_y=False)[0]) for b in range(8)]
    assert abs(float(whole) - sum(singles) / 8) <= 1.2e-7, (float(whole), singles)


def test_bit_reproducible_and_independent_of_conv_precision(fa):
    x, y = pair(8, 1, 256, 256, seed=33)
    first = hip(fa, x, y)
    again = hip(fa, x, y)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    saved = fa.ops.conv_precision
    try:
        for prec in (0, 3):
            fa.ops.conv_precision = prec
            got = hip(fa, x, y)
            assert all(torch.equal(a, b) for a, b in zip(first, got)), prec
    finally:
        fa.ops.conv_precision = saved


def test_runs_on_the_current_stream(fa):
    x, y = pair(2, 1, 64, 64, seed=41)
    want = hip(fa, x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = hip(fa, x, y)
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
def test_train_step_phase_term(fa, O, precision, two_chains):
    """192^2, batch 2: the term is what the restatement gives on the step's own tensors, it is what loss_G gains, it moves the
    generators' gradient, and a weight-0 step does not know it.  Both places the opt-in terms live: the two-chain schedule
    (``_extension_terms``) and the single-stream ``generator_loss``."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    try:
        ts = fresh_step(fa, O, precision=precision, phase_weight=0.5)
        L = ts.step(a, b, sync=True, keep=True)
        gn = ts.grad_norms()
        ts0 = fresh_step(fa, O, precision=precision)
        L0 = ts0.step(a, b, sync=True, keep=True)
        gn0 = ts0.grad_norms()
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_phase" not in L0
    T = L["tensors"]
    want = 0.5 * ((1 + float(restatement(T["recovered_A"], a)[0])) + (1 + float(restatement(T["recovered_B"], b)[0])))
    print("PHASE_ERR step %s two_chains=%s: loss_phase %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0, |grad A2B| %.5f against %.5f"
          % (precision, two_chains, L["loss_phase"], want, L["loss_G"], L0["loss_G"], gn["A2B"], gn0["A2B"]))
    assert abs(L["loss_phase"] - want) <= 1e-3 * abs(want)
    assert abs((L["loss_G"] - L0["loss_G"]) - L["loss_phase"]) <= 1e-3 * abs(L["loss_G"])
    assert abs(gn["A2B"] - gn0["A2B"]) > 1e-3 * gn0["A2B"] or abs(gn["B2A"] - gn0["B2A"]) > 1e-3 * gn0["B2A"], (gn, gn0)
    for k in L0:
        if k not in ("tensors", "loss_G"):
            assert abs(L[k] - L0[k]) <= 1e-3 * max(abs(L0[k]), 2e-2), (k, L[k], L0[k])


def test_graph_captured_step_with_phase_term(fa, O):
    """The step with the spectral term as one captured hipGraph: three replays follow the eager step at the bars of the existing
    graph test (2e-4 relative at step 0; later 3e-3 on the tight losses, 0.03 / 0.06 absolute on the others)."""
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    eager = fresh_step(fa, O, precision="f32", phase_weight=0.5)
    Le = [eager.step(a, b, sync=True) for a, b in batches]
    ts = fresh_step(fa, O, precision="f32", phase_weight=0.5)
    gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
    Lg = [gs.step(a, b, sync=True) for a, b in batches]
    for s in range(3):
        print("PHASE_ERR graph step %d: loss_phase %.7f eager %.7f, loss_G %.6f eager %.6f" % (s, Lg[s]["loss_phase"], Le[s]["loss_phase"], Lg[s]["loss_G"], Le[s]["loss_G"]))
        for k in ("loss_phase", "loss_G"):
            tol = 2e-4 if s == 0 else (3e-3 if k in TIGHT else None)
            if tol is not None:
                assert Lg[s][k] == pytest.approx(Le[s][k], rel=tol, abs=1e-6), (s, k, Lg[s][k], Le[s][k])
            else:
                assert Lg[s][k] == pytest.approx(Le[s][k], abs=0.03 if s == 1 else 0.06), (s, k)
    assert ts.opt_G.step_count == 3
