"""The focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021) on the MI355X: ``ops.focal_frequency_loss`` against the float64
``torch.fft`` restatement of its definition (pinned to tests/golden/golden_ffl.npz by tests/test_ffl_cpu.py), its exact
properties, and the opt-in ``TrainStep(ffl_weight=...)`` term, eager in both schedules and hipGraph-captured.

The error bar is relative to the error of the fp32 ``torch.fft`` run of the same definition on the CPU against float64:
  * each gradient, in relative L2:  e_hip <= 8 e_ref  (e_ref is 1.0e-7 - 4.7e-7 over the fixture, never accidentally tiny);
  * the loss:  |L_hip - L_64| <= 8 r |L_64| + one fp32 ulp of L_64, with r the largest relative loss error of the fp32
    run over the fixture's cases (2.2e-7; one case's own error can be near zero by accident).
The factor 8 is the bar tests/test_gpu_phase_loss.py holds this DFT-as-GEMM path to, for the reasons its docstring gives.
Figures of one run: profiles/ffl_error.txt."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_ffl.npz")
TIGHT = ("loss_G", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")
SETTINGS = ((1.0, False, False), (0.5, True, False), (2.0, False, True), (0.0, False, False))
FIXTURE_SHAPES = ((1, 1, 2, 2), (1, 1, 2, 3), (3, 1, 63, 50), (2, 1, 65, 70), (2, 2, 96, 64))
SAME = (3, 1, 16, 16)


def restatement(x, y, alpha=1.0, log_matrix=False, batch_matrix=False, dtype=torch.float64):
    """The literal definition with ``torch.fft`` on the CPU in ``dtype``: (loss, dL/dx, dL/dy) as float64."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    D = torch.fft.fft2(x, norm="ortho") - torch.fft.fft2(y, norm="ortho")
    q = D.real ** 2 + D.imag ** 2
    with torch.no_grad():
        w = torch.sqrt(q) ** alpha
        if log_matrix:
            w = torch.log(w + 1)
        w = w / (w.max() if batch_matrix else w.amax(dim=(-2, -1), keepdim=True))
        w[torch.isnan(w)] = 0
        w = torch.clamp(w, 0, 1)
    loss = (w * q).mean()
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach().double(), gx.double(), gy.double()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tag_of(shape, setting):
    return "%s_a%g_l%d_b%d" % ("x".join(str(s) for s in shape), setting[0], setting[1], setting[2])


def pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(*shape, generator=g))
    y = torch.tanh(x + 0.3 * torch.randn(*shape, generator=g))
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
def loss_r(gold):
    """The largest relative loss error of the fp32 reference over the file's cases."""
    r = 0.0
    for shape in gold["shapes"]:
        for st in SETTINGS:
            t = tag_of(tuple(shape), st)
            r = max(r, abs(float(gold["loss32_" + t]) - float(gold["loss64_" + t])) / abs(float(gold["loss64_" + t])))
    assert 1e-8 < r < 1e-6
    return r


def fixture_pair(gold, shape):
    case = "x".join(str(s) for s in shape)
    return torch.from_numpy(gold["x_" + case]), torch.from_numpy(gold["y_" + case])


def hip(fa, x, y, setting=SETTINGS[0], want_x=True, want_y=True, g=None):
    """(loss, dx, dy) of ops.focal_frequency_loss on the GPU, back on the host (a gradient that was not asked for is None)."""
    xd = x.cuda().requires_grad_(want_x)
    yd = y.cuda().requires_grad_(want_y)
    loss = fa.ops.focal_frequency_loss(xd, yd, *setting)
    assert loss.shape == () and loss.dtype == torch.float32
    if want_x or want_y:
        loss.backward(None if g is None else torch.tensor(g, device="cuda"))
    torch.cuda.synchronize()
    return loss.detach().cpu(), (xd.grad.cpu() if want_x else None), (yd.grad.cpu() if want_y else None)


def loss_bar(l64, r):
    return 8 * r * abs(float(l64)) + float(np.spacing(np.float32(abs(float(l64)))))


def hold_to_bar(name, ref64, e_ref_g, got, r):
    """Print e_ref, e_hip and their ratio for the loss and both gradients, then assert the bar of the module docstring."""
    e_loss = abs(float(got[0]) - float(ref64[0]))
    e_gx, e_gy = rel_l2(got[1], ref64[1]), rel_l2(got[2], ref64[2])
    print("FFL_ERR %-34s loss %.9e rel err %.3e (bar %.3e) | gx e_ref %.3e e_hip %.3e ratio %.2f | gy e_hip %.3e ratio %.2f  (|gx| %.3e)"
          % (name, float(got[0]), e_loss / abs(float(ref64[0])), loss_bar(ref64[0], r) / abs(float(ref64[0])), e_ref_g, e_gx, e_gx / e_ref_g,
             e_gy, e_gy / e_ref_g, float(ref64[1].norm())))
    assert e_loss <= loss_bar(ref64[0], r), (name, "loss", float(got[0]), float(ref64[0]))
    assert e_gx <= 8 * e_ref_g, (name, "gx", e_gx, e_ref_g)
    assert e_gy <= 8 * e_ref_g, (name, "gy", e_gy, e_ref_g)


@pytest.mark.parametrize("shape", FIXTURE_SHAPES)
def test_fixture_parity(fa, gold, loss_r, shape):
    """The fixture's inputs at the four settings: a 2 x 2 plane, an odd side, a single tile with remainders on both axes, two
    tiles per axis with remainders of 1 and 6, and two channels.  e_ref is the file's (fp32 torch.fft against float64)."""
    x, y = fixture_pair(gold, shape)
    for st in SETTINGS:
        t = tag_of(shape, st)
        ref64 = restatement(x, y, *st)
        assert abs(float(ref64[0]) - float(gold["loss64_" + t])) <= 1e-12 * abs(float(ref64[0]))
        hold_to_bar("fixture " + t, ref64, float(gold["gerr32_" + t]), hip(fa, x, y, st), loss_r)


@pytest.mark.parametrize("shape,settings", [((2, 1, 64, 64), SETTINGS), ((8, 1, 256, 256), SETTINGS[:1])])
def test_exact_tile_and_the_benchmark_shape(fa, loss_r, shape, settings):
    """An exact 64 x 64 tile (no remainder lanes) at the four settings and the benchmark's shape at the default one, through the
    module; e_ref from the fp32 torch.fft run on the CPU."""
    x, y = pair(shape, seed=77 + shape[0] + shape[2])
    for st in settings:
        crit = fa.FocalFrequencyLoss(1.0, *st)
        xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        loss = crit(xd, yd)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward()
        ref64, ref32 = restatement(x, y, *st), restatement(x, y, *st, dtype=torch.float32)
        hold_to_bar(tag_of(shape, st), ref64, rel_l2(ref32[1], ref64[1]), (loss.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()), loss_r)


@pytest.mark.parametrize("setting", SETTINGS)
def test_exact_properties(fa, setting):
    """Bit for bit, on two tiles per axis with remainders: L(x, x) = 0 with all-zero gradients; L(x, y) = L(y, x);
    dy = -dx; halving the upstream gradient halves dx; two calls agree; the convolution precision setting does not matter."""
    x, y = pair((2, 1, 65, 70), seed=5)
    l0, gx0, gy0 = hip(fa, x, x.clone(), setting)
    assert float(l0) == 0.0 and not gx0.any() and not gy0.any()
    first = hip(fa, x, y, setting)
    assert float(first[0]) > 0 and torch.isfinite(first[1]).all() and first[1].any()
    assert torch.equal(first[2], -first[1])
    swapped = hip(fa, y, x, setting)
    assert torch.equal(swapped[0], first[0]) and torch.equal(swapped[1], first[2]) and torch.equal(swapped[2], first[1])
    half = hip(fa, x, y, setting, g=0.5)
    assert torch.equal(half[0], first[0]) and torch.equal(half[1], 0.5 * first[1]) and torch.equal(half[2], 0.5 * first[2])
    again = hip(fa, x, y, setting)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    saved = fa.ops.conv_precision
    try:
        for prec in (0, 3):
            fa.ops.conv_precision = prec
            got = hip(fa, x, y, setting)
            assert all(torch.equal(a, b) for a, b in zip(first, got)), prec
    finally:
        fa.ops.conv_precision = saved


def test_sample_with_identical_images(fa, gold, loss_r):
    """The (3,1,16,16) case whose middle sample has y == x: its own maximum is 0 and its weight NaN -> 0.  The loss is finite
    and the restatement's, that sample's gradient is exactly zero; with ``batch_matrix`` the plane is normalised by the batch's
    maximum, not zero-weighted by its own -- the result is still the restatement's."""
    x, y = fixture_pair(gold, SAME)
    assert torch.equal(x[1], y[1])
    for st in SETTINGS + ((1.0, False, True), (0.5, True, True)):
        ref64, ref32 = restatement(x, y, *st), restatement(x, y, *st, dtype=torch.float32)
        got = hip(fa, x, y, st)
        assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all()
        assert not got[1][1].any() and not got[2][1].any() and got[1][0].any() and got[1][2].any()
        hold_to_bar("identical middle sample " + tag_of(SAME, st), ref64, rel_l2(ref32[1], ref64[1]), got, loss_r)


@pytest.mark.parametrize("shape", [(3, 1, 63, 50), (2, 2, 96, 64)])
def test_alpha_zero_is_the_mean_squared_error(fa, loss_r, shape):
    """Independent of torch.fft: by Parseval the loss at alpha = 0 is mean((x - y)^2), here in float64."""
    x, y = pair(shape, seed=13)
    d = x.double() - y.double()
    mse, gx = (d * d).mean(), 2 * d / d.numel()
    got = hip(fa, x, y, (0.0, False, False))
    print("FFL_ERR alpha = 0 %-16s loss %.9e mse %.9e rel err %.3e (bar %.3e) | gx against 2 (x - y) / n: %.3e"
          % ("x".join(map(str, shape)), float(got[0]), float(mse), abs(float(got[0]) - float(mse)) / float(mse), loss_bar(mse, loss_r) / float(mse),
             rel_l2(got[1], gx)))
    assert abs(float(got[0]) - float(mse)) <= loss_bar(mse, loss_r)
    assert torch.equal(got[2], -got[1])


def test_gradient_to_one_input_and_nothing_saved_without_one(fa, monkeypatch):
    """Either gradient alone equals the pair's; under ``no_grad``, and for inputs without a gradient, the forward is handed no
    plane buffer and keeps no graph."""
    x, y = pair((2, 1, 63, 50), seed=9)
    l_b, gx_b, gy_b = hip(fa, x, y)
    l_x, gx, none_y = hip(fa, x, y, want_y=False)
    l_y, none_x, gy = hip(fa, x, y, want_x=False)
    assert none_x is None and none_y is None
    assert torch.equal(l_b, l_x) and torch.equal(l_b, l_y)
    assert torch.equal(gx, gx_b) and torch.equal(gy, gy_b)
    planes = []
    real = fa.ops.call

    def spy(name, *args):
        if name == "ffl_fwd":
            planes.append(args[8])
        return real(name, *args)
    monkeypatch.setattr(fa.ops, "call", spy)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    with torch.no_grad():
        l_n = fa.ops.focal_frequency_loss(xd, yd)
    l_p = fa.ops.focal_frequency_loss(xd.detach(), yd.detach())
    l_g = fa.ops.focal_frequency_loss(xd, yd.detach())
    assert planes[0] is None and planes[1] is None and planes[2] is not None
    assert l_n.grad_fn is None and not l_n.requires_grad and not l_p.requires_grad and l_g.requires_grad
    assert torch.equal(l_n.cpu(), l_b) and torch.equal(l_p.cpu(), l_b) and torch.equal(l_g.detach().cpu(), l_b)


def test_runs_on_the_current_stream(fa):
    x, y = pair((2, 1, 64, 64), seed=41)
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
def test_train_step_ffl_term(fa, O, two_chains):
    """192^2, batch 2: the term is what the restatement gives on the step's own tensors, it is what loss_G gains, it moves the
    generators' gradient, and a weight-0 step does not know it.  Both places the opt-in terms live: the two-chain schedule
    (``_extension_terms``) and the single-stream ``generator_loss``."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    saved = fa.TrainStep.overlap_min_pixels
    fa.TrainStep.overlap_min_pixels = 0 if two_chains else 1 << 40
    try:
        ts = fresh_step(fa, O, precision="f16x2", ffl_weight=0.5)
        L = ts.step(a, b, sync=True, keep=True)
        gn = ts.grad_norms()
        ts0 = fresh_step(fa, O, precision="f16x2")
        L0 = ts0.step(a, b, sync=True, keep=True)
        gn0 = ts0.grad_norms()
    finally:
        fa.TrainStep.overlap_min_pixels = saved
    assert "loss_ffl" not in L0 and ts0.ffl is None
    T = L["tensors"]
    want = 0.5 * (float(restatement(T["recovered_A"], a)[0]) + float(restatement(T["recovered_B"], b)[0]))
    print("FFL_ERR step two_chains=%s: loss_ffl %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0, |grad A2B| %.5f against %.5f"
          % (two_chains, L["loss_ffl"], want, L["loss_G"], L0["loss_G"], gn["A2B"], gn0["A2B"]))
    assert want > 0 and abs(L["loss_ffl"] - want) <= 1e-3 * abs(want)
    assert abs((L["loss_G"] - L0["loss_G"]) - L["loss_ffl"]) <= 1e-3 * abs(L["loss_G"])
    assert abs(gn["A2B"] - gn0["A2B"]) > 1e-3 * gn0["A2B"] or abs(gn["B2A"] - gn0["B2A"]) > 1e-3 * gn0["B2A"], (gn, gn0)
    for k in L0:
        if k not in ("tensors", "loss_G"):
            assert abs(L[k] - L0[k]) <= 1e-3 * max(abs(L0[k]), 2e-2), (k, L[k], L0[k])


def test_graph_captured_step_with_ffl_term(fa, O):
    """The step with the focal frequency term as one captured hipGraph: three replays follow the eager step at the bars of the
    existing graph tests (2e-4 relative at step 0; later 3e-3 on the tight losses, 0.03 / 0.06 absolute on the others)."""
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    eager = fresh_step(fa, O, precision="f32", ffl_weight=0.5)
    Le = [eager.step(a, b, sync=True) for a, b in batches]
    ts = fresh_step(fa, O, precision="f32", ffl_weight=0.5)
    gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
    Lg = [gs.step(a, b, sync=True) for a, b in batches]
    for s in range(3):
        print("FFL_ERR graph step %d: loss_ffl %.7f eager %.7f, loss_G %.6f eager %.6f" % (s, Lg[s]["loss_ffl"], Le[s]["loss_ffl"], Lg[s]["loss_G"], Le[s]["loss_G"]))
        for k in ("loss_ffl", "loss_G"):
            tol = 2e-4 if s == 0 else (3e-3 if k in TIGHT else None)
            if tol is not None:
                assert Lg[s][k] == pytest.approx(Le[s][k], rel=tol, abs=1e-6), (s, k, Lg[s][k], Le[s][k])
            else:
                assert Lg[s][k] == pytest.approx(Le[s][k], abs=0.03 if s == 1 else 0.06), (s, k)
    assert ts.opt_G.step_count == 3
