"""The stationary wavelet transform (csrc/swt.hip) on the MI355X: ``SWTForward`` / ``SWTInverse`` against the reference's own CPU
results (tests/golden/golden_swt*.npz) and against the float64 restatement of tests/test_swt_cpu.py (pinned to those fixtures
there), structural properties, and the opt-in stationary wavelet-HF term of ``TrainStep``.

The error bar, in relative L2 against the float64 restatement:   e_hip <= 2 e_ref + 2^-23
with e_ref the fp32 reference's own distance from it (the fixture's arrays; for off-fixture shapes the restatement run in fp32
on the CPU).  It is the bar of the DWT and TV tests, for their reason: both sides add L terms per pass in fp32, in different
orders (and the kernels contract to fused multiply-adds).  Every compared array prints ``SWT_ERR name e_ref e_hip ratio``; an
MI355X run is kept in profiles/swt_error.txt."""
import random

import pytest
import torch

from test_swt_cpu import (A_BUFS, MODES, S_BUFS, analysis_bank, decode, fixture_cases, forward_grad, forward_levels, gold,
                          inverse_levels, rel_l2, restate_case, synthesis_bank, waves)

pytestmark = pytest.mark.gpu

K, FLOOR = 2.0, 2.0 ** -23


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def hold_to_bar(name, ref64, ref32, got):
    bad = []
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (name, k, tuple(got[k].shape), tuple(ref64[k].shape))
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("SWT_ERR %-40s %-8s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


def run_forward(fa, bank, mode, J, x, cots):
    """Every level's output and x.grad from the module on the GPU; ``x`` may be a device view."""
    fwd = fa.SWTForward(J=J, wave=waves(fa, bank)[0], mode=mode).cuda()
    xd = x.cuda().detach().requires_grad_(True) if not x.is_cuda else x.detach().requires_grad_(True)
    ys = fwd(xd)
    assert isinstance(ys, list) and len(ys) == J
    assert all(y.is_contiguous() and tuple(y.shape) == (x.shape[0], x.shape[1], 4, x.shape[2], x.shape[3]) for y in ys)
    out = {"y%d" % j: y.detach().cpu() for j, y in enumerate(ys)}
    torch.autograd.backward(ys, [c.cuda() for c in cots])
    out["xgrad"] = xd.grad.cpu()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_fixture_parity(fa, case):
    """Outputs and x.grad of every fixture case; e_ref is the fixture's own distance from the restatement."""
    cid, bank, mode, J, shape = case
    g = gold()
    ref64 = restate_case(*case)
    ref32 = {k: torch.from_numpy(g[cid + "/" + k]) for k in ref64}
    got = run_forward(fa, bank, mode, J, torch.from_numpy(g["x_%dx%dx%dx%d" % shape]), [decode(g[cid + "/cot_y%d" % j]) for j in range(J)])
    hold_to_bar(cid, ref64, ref32, got)


def module_banks(fa, bank, mode="periodic", J=1):
    wf, wi = waves(fa, bank)
    fwd, inv = fa.SWTForward(J=J, wave=wf, mode=mode), fa.SWTInverse(wave=wi)
    return [getattr(fwd, n) for n in A_BUFS], [getattr(inv, n) for n in S_BUFS]


def free_forward(fa, name, bank, mode, J, x, view=None):
    """An off-fixture shape: the restatement in float64 and in fp32 on the module's own (fp32) buffers, then the kernels."""
    ab, _ = module_banks(fa, bank, mode, J)
    gen = torch.Generator().manual_seed(99)
    cots = [torch.rand((x.shape[0], x.shape[1], 4) + tuple(x.shape[2:]), generator=gen) - 0.5 for _ in range(J)]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        b = analysis_bank(ab, dtype)
        out = {"y%d" % j: y for j, y in enumerate(forward_levels(x.to(dtype), b, mode, J))}
        out["xgrad"] = forward_grad([c.to(dtype) for c in cots], b, mode)
        ref[dtype] = {k: v.double() for k, v in out.items()}
    got = run_forward(fa, bank, mode, J, x if view is None else view, cots)
    hold_to_bar(name, ref[torch.float64], ref[torch.float32], got)


@pytest.mark.parametrize("mode", MODES)
def test_off_fixture_sweep(fa, mode):
    """16 taps at an odd size; four levels of db2 (dilation 8, minimum side 17) at a size that is no multiple of 8, so the residue
    classes differ in length; three levels at 256^2, four tiles per axis."""
    g = torch.Generator().manual_seed(7)
    free_forward(fa, "3x2x33x50 db8 J1 %s" % mode, "db8", mode, 1, torch.randn(3, 2, 33, 50, generator=g))
    free_forward(fa, "2x1x40x72 db2 J4 %s" % mode, "db2", mode, 4, torch.randn(2, 1, 40, 72, generator=g))
    free_forward(fa, "2x1x256x256 db4 J3 %s" % mode, "db4", mode, 3, torch.randn(2, 1, 256, 256, generator=g))


@pytest.mark.parametrize("mode", ("symmetric", "periodization"))
def test_non_contiguous_view(fa, mode):
    big = torch.randn(2, 2, 60, 90, generator=torch.Generator().manual_seed(13))
    view = big.cuda()[:, :, 3:40, 5:69]
    assert not view.is_contiguous()
    free_forward(fa, "view 2x2x37x64 db4 J2 %s" % mode, "db4", "periodic" if mode == "periodization" else mode, 2,
                 big[:, :, 3:40, 5:69].contiguous(), view=view)
    if mode == "periodization":                                     # the alias computes what 'periodic' does, bit for bit
        w = waves(fa, "db4")[0]
        a = fa.SWTForward(J=2, wave=w, mode="periodization").cuda()(view)
        b = fa.SWTForward(J=2, wave=w, mode="periodic").cuda()(view)
        assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("bank", ("db2", "db4", "db8", "db2db4"))
def test_inverse_reconstructs(fa, bank):
    """SWTInverse(SWTForward(x)) against x itself (what the float64 restatement reconstructs to 1e-10) at 2x2x37x64, J = 2;
    e_ref is the restatement's round trip in fp32."""
    x = torch.randn(2, 2, 37, 64, generator=torch.Generator().manual_seed(21))
    wf, wi = waves(fa, bank)
    fwd, inv = fa.SWTForward(J=2, wave=wf, mode="periodic").cuda(), fa.SWTInverse(wave=wi, mode="periodic").cuda()
    y = inv(fwd(x.cuda()))
    assert y.is_contiguous() and tuple(y.shape) == tuple(x.shape)
    ab, sb = module_banks(fa, bank, "periodic", 2)
    y32 = inverse_levels(forward_levels(x, analysis_bank(ab, torch.float32), "periodic", 2), synthesis_bank(sb, torch.float32))
    hold_to_bar("reconstruction 2x2x37x64 J2 %s" % bank, {"x": x.double()}, {"x": y32}, {"x": y.cpu()})


@pytest.mark.parametrize("bank", ("db4", "db2db4"))
def test_inverse_and_its_gradients_on_random_coefficients(fa, bank):
    """Three levels of random coefficients at 2x1x33x40: the inverse and its gradient with respect to every level against the
    restatement (whose gradients come from autograd through it).  The finer levels' band 0 gets a zero gradient."""
    gen = torch.Generator().manual_seed(31)
    J, shape = 3, (2, 1, 4, 33, 40)
    coeffs = [torch.randn(shape, generator=gen) for _ in range(J)]
    cot = torch.rand((2, 1, 33, 40), generator=gen) - 0.5
    _, sb = module_banks(fa, bank)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        cs = [c.clone().to(dtype).requires_grad_(True) for c in coeffs]          # a copy: .to(float32) would hand back c itself
        y = inverse_levels(cs, synthesis_bank(sb, dtype))
        y.backward(cot.to(dtype))
        ref[dtype] = {"inv": y.detach().double(), "g_coarse": cs[-1].grad.double()}
        for j in range(J - 1):
            assert float(cs[j].grad[:, :, 0].abs().max()) == 0.0
            ref[dtype]["g_high%d" % j] = cs[j].grad[:, :, 1:].double()
    inv = fa.SWTInverse(wave=waves(fa, bank)[1]).cuda()
    cd = [c.cuda().requires_grad_(True) for c in coeffs]
    y = inv(cd)
    y.backward(cot.cuda())
    got = {"inv": y.detach().cpu(), "g_coarse": cd[-1].grad.cpu()}
    for j in range(J - 1):
        assert float(cd[j].grad[:, :, 0].abs().max()) == 0.0
        got["g_high%d" % j] = cd[j].grad[:, :, 1:].cpu()
    hold_to_bar("inverse 2x1x33x40 J3 %s" % bank, ref[torch.float64], ref[torch.float32], got)


@pytest.mark.parametrize("mode", MODES)
def test_backward_is_the_adjoint(fa, mode):
    """<A x, c> == <x, A^T c> with A^T the backward, relative 1e-5, sums in float64: two levels of db4 at 2x2x37x50."""
    g = torch.Generator().manual_seed(5)
    fwd = fa.SWTForward(J=2, wave=fa.daubechies(4), mode=mode).cuda()
    x = torch.randn(2, 2, 37, 50, generator=g).cuda().requires_grad_(True)
    ys = fwd(x)
    cs = [torch.randn(y.shape, generator=g).cuda() for y in ys]
    lhs = sum(float((y.double() * c.double()).sum()) for y, c in zip(ys, cs))
    torch.autograd.backward(ys, cs)
    rhs = float((x.detach().double() * x.grad.double()).sum())
    print("SWT_ERR adjoint identity %s: %.9e against %.9e" % (mode, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_synthesis_backward_is_its_adjoint(fa):
    g = torch.Generator().manual_seed(6)
    inv = fa.SWTInverse(wave=fa.daubechies(4)).cuda()
    c = torch.randn(2, 2, 4, 37, 50, generator=g).cuda().requires_grad_(True)
    y = inv([c])
    cy = torch.randn(y.shape, generator=g).cuda()
    lhs = float((y.double() * cy.double()).sum())
    y.backward(cy)
    rhs = float((c.detach().double() * c.grad.double()).sum())
    print("SWT_ERR adjoint identity synthesis: %.9e against %.9e" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_bit_reproducible_and_on_the_current_stream(fa):
    x = torch.randn(1, 3, 70, 150, generator=torch.Generator().manual_seed(3))
    cots = [torch.full((1, 3, 4, 70, 150), 0.25), torch.full((1, 3, 4, 70, 150), -0.5)]
    w = fa.daubechies(4)

    def once():
        out = run_forward(fa, "db4", "symmetric", 2, x, cots)
        inv = fa.SWTInverse(wave=w).cuda()
        c = [out["y0"].cuda().requires_grad_(True), out["y1"].cuda()]
        y = inv(c)
        y.backward(torch.full_like(y, 0.5))
        out["inv"], out["inv_g"] = y.detach().cpu(), c[0].grad.cpu()
        return out
    first, again = once(), once()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = once()
    torch.cuda.current_stream().wait_stream(s)
    for k in first:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], side[k]), k


def test_small_side_raises_before_any_launch(fa, monkeypatch):
    """db4 at J = 2 runs at 9x9; a side of 8 raises ``ValueError`` in every mode, for the forward and for the inverse, and the
    rejected call reaches no kernel entry point."""
    d4 = fa.daubechies(4)
    ys = fa.SWTForward(J=2, wave=d4, mode="reflect").cuda()(torch.zeros(1, 1, 9, 9, device="cuda"))
    assert [tuple(y.shape) for y in ys] == [(1, 1, 4, 9, 9)] * 2
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for mode in MODES + ("periodization",):
        fwd = fa.SWTForward(J=2, wave=d4, mode=mode).cuda()
        for shape in ((1, 1, 8, 12), (1, 1, 12, 8)):
            with pytest.raises(ValueError, match="minimum side"):
                fwd(torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError, match="minimum side"):
        fa.SWTInverse(wave=d4).cuda()([torch.zeros(1, 1, 4, 8, 12, device="cuda")] * 2)
    assert calls == []
    fa.SWTForward(J=2, wave=d4, mode="zero").cuda()(torch.zeros(1, 1, 9, 12, device="cuda"))
    assert calls == ["swt2d_analysis", "swt2d_analysis"]
    torch.cuda.synchronize()


def test_entry_points_refuse_bad_arguments(fa):
    """Tap count, mode, dilation and geometry come back as the library's error with a text, not as a launch."""
    from faoctasr import ops
    x, y = torch.zeros(1, 1, 16, 16, device="cuda"), torch.empty(1, 1, 4, 16, 16, device="cuda")
    t4, t3 = ops._tap_array((0.5,) * 4), ops._tap_array((0.5,) * 3)
    good = dict(Lh=4, Lw=4, d=1, mode=0, H=16, W=16)
    for bad, text in ((dict(Lh=3), "tap counts"), (dict(mode=2), "extension"), (dict(d=3), "dilation"), (dict(d=8), "minimum side"),
                      (dict(d=16), "dilation")):
        a = dict(good, **bad)
        for name, args in (("swt2d_analysis", (x.data_ptr(), 256, y.data_ptr())), ("swt2d_adjoint", (y.data_ptr(), x.data_ptr(), 256, None, 0, 0))):
            with pytest.raises(fa.KernelError, match=text):
                fa.ops.call(name, *args, 1, a["H"], a["W"], t3 if a["Lh"] == 3 else t4, t4, a["Lh"], t4, t4, a["Lw"], a["d"], a["mode"], 1.0,
                            fa._lib.stream_ptr())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------
# the stationary wavelet-HF term of the training step
# ----------------------------------------------------------------------------------------
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


def whf_restatement(fa, T, weight, J, mode):
    """weight * sum over both cycles and all levels of mean |bands 1..3 (recovered) - bands 1..3 (real)|, in float64."""
    b = analysis_bank([getattr(fa.SWTForward(J=J, wave=fa.daubechies(4), mode=mode), n) for n in A_BUFS])
    tot = 0.0
    for rec, real in (("recovered_A", "real_A"), ("recovered_B", "real_B")):
        yr = forward_levels(T[rec].detach().cpu().double(), b, mode, J)
        yt = forward_levels(T[real].detach().cpu().double(), b, mode, J)
        tot += sum(float((p[:, :, 1:] - q[:, :, 1:]).abs().mean()) for p, q in zip(yr, yt))
    return weight * tot


SWT_KW = dict(whf_weight=0.1, dwt_levels=2, dwt_mode="periodic", dwt_stationary=True)


def test_train_step_stationary_whf_term(fa, O):
    """192^2, batch 2, f32: the term is what the restatement gives on the step's own tensors, it is what loss_G gains, and the other
    losses stay at the weight-0 step's values (the bars of the db4 term's test)."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    ts = fresh_step(fa, O, precision="f32", dwt_wave=fa.daubechies(4), **SWT_KW)
    L = ts.step(a, b, sync=True, keep=True)
    L0 = fresh_step(fa, O, precision="f32").step(a, b, sync=True, keep=True)
    assert "loss_whf" not in L0
    T = dict(L["tensors"])
    T.setdefault("real_A", a)
    T.setdefault("real_B", b)
    want = whf_restatement(fa, T, 0.1, 2, "periodic")
    print("SWT_ERR step: loss_whf %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0" % (L["loss_whf"], want, L["loss_G"], L0["loss_G"]))
    assert abs(L["loss_whf"] - want) <= 1e-3 * abs(want)
    assert abs((L["loss_G"] - L0["loss_G"]) - L["loss_whf"]) <= 1e-3 * abs(L["loss_G"])
    for k in L0:
        if k not in ("tensors", "loss_G"):
            assert abs(L[k] - L0[k]) <= 1e-3 * max(abs(L0[k]), 2e-2), (k, L[k], L0[k])


def test_graph_captured_step_with_stationary_whf_term(fa, O):
    """Three replays of the captured step follow the eager one at the bars of the db4 term's graph test."""
    kw = dict(dwt_wave=fa.daubechies(4), **SWT_KW)
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    eager = fresh_step(fa, O, precision="f32", **kw)
    Le = [eager.step(a, b, sync=True) for a, b in batches]
    ts = fresh_step(fa, O, precision="f32", **kw)
    gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
    Lg = [gs.step(a, b, sync=True) for a, b in batches]
    for s in range(3):
        print("SWT_ERR graph step %d: loss_whf %.7f eager %.7f, loss_G %.6f eager %.6f" % (s, Lg[s]["loss_whf"], Le[s]["loss_whf"], Lg[s]["loss_G"], Le[s]["loss_G"]))
        for k in ("loss_whf", "loss_G"):
            tol = 2e-4 if s == 0 else 3e-3
            assert Lg[s][k] == pytest.approx(Le[s][k], rel=tol, abs=1e-6), (s, k, Lg[s][k], Le[s][k])
    assert ts.opt_G.step_count == 3
