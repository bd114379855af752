"""The general filter-bank DWT / IDWT (csrc/dwt.hip) on the MI355X: ``DWTForward`` / ``DWTInverse`` built from taps against the
reference's own CPU results (tests/golden/golden_dwt*.npz) and against the float64 restatement of tests/test_dwt_general_cpu.py
(pinned to those fixtures there), structural properties, and the opt-in wavelet-HF term of ``TrainStep`` on a db4 bank.

The error bar, in relative L2 against the float64 restatement:   e_hip <= 2 e_ref + 2^-23
with e_ref the fp32 reference's own distance from it (the fixture's arrays; for off-fixture shapes the restatement run in fp32
on the CPU).  The kernels and the reference both round after the first pass and add L terms per pass in fp32; they differ in
the order of those sums (and the kernels contract to fused multiply-adds), which is what the factor 2 -- the TV loss test's --
leaves room for; 2^-23 keeps the bar satisfiable where e_ref happens to be tiny.  Measured on an MI355X over 509 arrays:
e_hip / e_ref 0.79 - 1.82, median 1.00 (profiles/dwt_error.txt).

The backward passes are the reference's definitions (wavelets.py), so the dot-product identity is asserted only where those are
the adjoint: 'zero' at any size and 'periodization' at even sizes."""
import os
import random

import numpy as np
import pytest
import torch

from test_dwt_general_cpu import (A_BUFS, MODES, S_BUFS, analysis_2d, decode, fixture_cases, forward_grad, forward_levels, gold,
                                  inverse_grads, inverse_levels, rel_l2, restate_case)

pytestmark = pytest.mark.gpu

K, FLOOR = 2.0, 2.0 ** -23
TIGHT = ("loss_G", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


@pytest.fixture(scope="module")
def O():
    from oracle import octa_oracle
    return octa_oracle


def bank_waves(fa, bank):
    d = {"db2": fa.daubechies(2), "db4": fa.daubechies(4), "db8": fa.daubechies(8)}
    if bank == "db2db4":
        a, b = d["db2"], d["db4"]
        return (a.dec_lo, a.dec_hi, b.dec_lo, b.dec_hi), (a.rec_lo, a.rec_hi, b.rec_lo, b.rec_hi)
    return d[bank], d[bank]


def run_hip(fa, bank, mode, J, x, cots, coeffs, cot_inv):
    """Everything a fixture case holds, from the modules on the GPU.  ``coeffs`` = (yl, [yh]) the inverse runs on (None: the
    forward's own), cots / cot_inv the cotangents (None: no backward)."""
    wf, wi = bank_waves(fa, bank)
    fwd, inv = fa.DWTForward(J=J, wave=wf, mode=mode).cuda(), fa.DWTInverse(wave=wi, mode=mode).cuda()
    xd = x.cuda().requires_grad_(True)
    yl, yh = fwd(xd)
    assert yl.is_contiguous() and all(h.is_contiguous() for h in yh) and len(yh) == J
    out = {"yl": yl.detach().cpu()}
    for j, h in enumerate(yh):
        out["yh%d" % j] = h.detach().cpu()
    if cots is not None:
        torch.autograd.backward([yl] + list(yh), [c.cuda() for c in cots])
        out["xgrad"] = xd.grad.cpu()
        cl, ch = (coeffs[0], coeffs[1]) if coeffs is not None else (out["yl"], [out["yh%d" % j] for j in range(J)])
        cl = cl.cuda().requires_grad_(True)
        ch = [h.cuda() for h in ch]
        ch[0].requires_grad_(True)
        y = inv((cl, ch))
        assert y.is_contiguous()
        out["inv"] = y.detach().cpu()
        y.backward(cot_inv.cuda())
        out["inv_gyl"], out["inv_gyh0"] = cl.grad.cpu(), ch[0].grad.cpu()
        with torch.no_grad():
            out["inv_none"] = inv((cl.detach(), [h.detach() for h in ch[:-1]] + [None])).cpu()
    torch.cuda.synchronize()
    return out


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bar of the module docstring on every one."""
    bad = []
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (name, k, tuple(got[k].shape), tuple(ref64[k].shape))
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("DWT_ERR %-46s %-8s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_fixture_parity(fa, case):
    """Outputs, x.grad, the inverse, its gradients and the None level of every fixture case; e_ref is the fixture's own error.
    The case the reference refuses (db4 / reflect / 9x6) takes e_ref from the restatement in fp32, outputs only."""
    cid, bank, mode, J, shape = case
    g = gold()
    x = torch.from_numpy(g["x_%dx%dx%dx%d" % shape])
    ref64 = restate_case(*case)
    if cid + "/reference_refuses" in g:
        ref32 = restate_case(*case, dtype=torch.float32)
        got = run_hip(fa, bank, mode, J, x, None, None, None)
    else:
        ref32 = {k: torch.from_numpy(g[cid + "/" + k]) for k in ref64}
        cots = [decode(g[cid + "/cot_yl"])] + [decode(g[cid + "/cot_yh%d" % j]) for j in range(J)]
        coeffs = (ref32["yl"], [ref32["yh%d" % j] for j in range(J)])
        got = run_hip(fa, bank, mode, J, x, cots, coeffs, decode(g[cid + "/cot_inv"]))
    hold_to_bar(cid, ref64, ref32, got)


def restate_free(fa, bank, mode, J, x, cots, cot_inv, dtype):
    """The restatement on an off-fixture input; the inverse runs on the fp64 forward's coefficients rounded to fp32."""
    wf, wi = bank_waves(fa, bank)
    fwd, inv = fa.DWTForward(J=J, wave=wf, mode=mode), fa.DWTInverse(wave=wi, mode=mode)
    ab = [getattr(fwd, n).to(dtype) for n in A_BUFS]
    sb = [getattr(inv, n).to(dtype) for n in S_BUFS]
    x64 = x.double()
    shapes, ll = [], x64
    ab64 = [b.double() for b in ab]
    for _ in range(J):
        shapes.append(ll.shape[-2:])
        ll = analysis_2d(ll, ab64, mode)[0]
    cl64, ch64 = forward_levels(x64, ab64, mode, J)
    coeffs = (cl64.float(), [h.float() for h in ch64])
    yl, yh = forward_levels(x.to(dtype), ab, mode, J)
    out = {"yl": yl}
    for j, h in enumerate(yh):
        out["yh%d" % j] = h
    out["xgrad"] = forward_grad(shapes, cots[0].to(dtype), [c.to(dtype) for c in cots[1:]], ab, mode)
    trims = []
    out["inv"] = inverse_levels(coeffs[0].to(dtype), [h.to(dtype) for h in coeffs[1]], sb, mode, trims)
    out["inv_gyl"], out["inv_gyh0"] = inverse_grads(cot_inv.to(dtype), trims, sb, mode)
    out["inv_none"] = inverse_levels(coeffs[0].to(dtype), [h.to(dtype) for h in coeffs[1][:-1]] + [None], sb, mode)
    return {k: v.double() for k, v in out.items()}, coeffs


def free_case(fa, name, bank, mode, J, x, view=None):
    gen = torch.Generator().manual_seed(99)
    wf, _ = bank_waves(fa, bank)
    ab = [getattr(fa.DWTForward(J=J, wave=wf, mode=mode), n).double() for n in A_BUFS]
    yl, yh = forward_levels(x.double(), ab, mode, J)
    cots = [torch.rand(t.shape, generator=gen) - 0.5 for t in [yl] + yh]
    inv_shape = inverse_levels(yl, yh, [getattr(fa.DWTInverse(wave=bank_waves(fa, bank)[1], mode=mode), n).double() for n in S_BUFS], mode).shape
    cot_inv = torch.rand(inv_shape, generator=gen) - 0.5
    ref64, coeffs = restate_free(fa, bank, mode, J, x, cots, cot_inv, torch.float64)
    ref32, _ = restate_free(fa, bank, mode, J, x, cots, cot_inv, torch.float32)
    got = run_hip(fa, bank, mode, J, x if view is None else view, cots, coeffs, cot_inv)
    hold_to_bar(name, ref64, ref32, got)


@pytest.mark.parametrize("mode", MODES)
def test_off_fixture_sweep(fa, mode):
    """16 taps at an odd size over several tiles' worth of planes, the minimum side of db8 (9 = L/2 + 1, where the folding modes
    fold more than once), three levels at 256^2."""
    g = torch.Generator().manual_seed(7)
    free_case(fa, "3x2x33x50 db8 %s" % mode, "db8", mode, 1, torch.randn(3, 2, 33, 50, generator=g))
    free_case(fa, "1x1x9x9 db8 %s" % mode, "db8", mode, 1, torch.randn(1, 1, 9, 9, generator=g))
    free_case(fa, "2x1x256x256 db4 J3 %s" % mode, "db4", mode, 3, torch.randn(2, 1, 256, 256, generator=g))


@pytest.mark.parametrize("mode", ("symmetric", "periodization"))
def test_non_contiguous_view(fa, mode):
    big = torch.randn(2, 2, 60, 90, generator=torch.Generator().manual_seed(13))
    view = big.cuda()[:, :, 3:40, 5:69]
    assert not view.is_contiguous()
    free_case(fa, "view 2x2x37x64 db4 %s" % mode, "db4", mode, 2, big[:, :, 3:40, 5:69].contiguous(), view=view)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bank", ("db2", "db4", "db8"))
def test_perfect_reconstruction(fa, bank, mode):
    """inv(fwd(x))[..., :H, :W] == x within 4e-6 max-abs at 2x2x37x64, J = 2: about 5x the 8.3e-7 the reference itself showed
    with 4 taps, for up to 16."""
    x = torch.randn(2, 2, 37, 64, generator=torch.Generator().manual_seed(21)).cuda()
    wf, wi = bank_waves(fa, bank)
    fwd, inv = fa.DWTForward(J=2, wave=wf, mode=mode).cuda(), fa.DWTInverse(wave=wi, mode=mode).cuda()
    yl, yh = fwd(x)
    L = 2 * int(bank[2:])
    sizes = [(37, 64)]
    for _ in range(2):
        sizes.append(tuple((n + 1) // 2 if mode == "periodization" else (n + L - 1) // 2 for n in sizes[-1]))
    assert tuple(yl.shape) == (2, 2) + sizes[2] and [tuple(h.shape) for h in yh] == [(2, 2, 3) + sizes[1], (2, 2, 3) + sizes[2]]
    y = inv((yl, yh))
    assert tuple(y.shape) == (2, 2, 38, 64)
    err = float((y[..., :37, :64] - x).abs().max())
    print("DWT_ERR reconstruction %s %s max-abs %.3e" % (bank, mode, err))
    assert err <= 4e-6


@pytest.mark.parametrize("mode,shape", [("zero", (2, 2, 37, 50)), ("zero", (1, 1, 64, 64)), ("periodization", (2, 2, 36, 50))])
def test_backward_is_the_adjoint_where_the_reference_is(fa, mode, shape):
    """<A x, c> == <x, A^T c> with A^T the backward, relative 1e-5, for the analysis and for the synthesis level."""
    g = torch.Generator().manual_seed(5)
    w = fa.daubechies(4)
    fwd, inv = fa.DWTForward(J=1, wave=w, mode=mode).cuda(), fa.DWTInverse(wave=w, mode=mode).cuda()
    x = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    yl, yh = fwd(x)
    cl, ch = torch.randn(yl.shape, generator=g).cuda(), torch.randn(yh[0].shape, generator=g).cuda()
    lhs = float((yl.double() * cl.double()).sum() + (yh[0].double() * ch.double()).sum())
    torch.autograd.backward([yl, yh[0]], [cl, ch])
    rhs = float((x.detach().double() * x.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    cl.requires_grad_(True)
    ch.requires_grad_(True)
    y = inv((cl, [ch]))
    cy = torch.randn(y.shape, generator=g).cuda()
    lhs = float((y.double() * cy.double()).sum())
    y.backward(cy)
    rhs = float((cl.detach().double() * cl.grad.double()).sum() + (ch.detach().double() * ch.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_bit_reproducible_and_on_the_current_stream(fa):
    x = torch.randn(1, 3, 70, 150, generator=torch.Generator().manual_seed(3))
    cots = None

    def once():
        nonlocal cots
        wf, wi = bank_waves(fa, "db4")
        ab = [getattr(fa.DWTForward(J=2, wave=wf, mode="symmetric"), n).double() for n in A_BUFS]
        if cots is None:
            yl, yh = forward_levels(x.double(), ab, "symmetric", 2)
            cots = [torch.ones(t.shape) * 0.25 for t in [yl] + yh]
        return run_hip(fa, "db4", "symmetric", 2, x, cots, None, torch.full((1, 3, 70, 150), 0.5))
    first, again = once(), once()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = once()
    torch.cuda.current_stream().wait_stream(s)
    for k in first:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], side[k]), k


def test_small_side_raises_before_any_launch(fa, monkeypatch):
    """5x7 is the smallest db2 case of the fixture; one step below it -- a side of L/2 = 2 -- raises ``ValueError``, for the
    forward and for a second level that shrinks below the minimum, and the rejected call reaches no kernel entry point."""
    d2 = fa.daubechies(2)
    fwd = fa.DWTForward(J=1, wave=d2, mode="symmetric").cuda()
    yl, _ = fwd(torch.zeros(1, 1, 5, 7, device="cuda"))
    assert tuple(yl.shape) == (1, 1, 4, 5)
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for mode in MODES:
        fwd = fa.DWTForward(J=1, wave=d2, mode=mode).cuda()
        for shape in ((1, 1, 2, 7), (1, 1, 5, 2)):
            with pytest.raises(ValueError, match="minimum side"):
                fwd(torch.zeros(shape, device="cuda"))
    assert calls == []
    with pytest.raises(ValueError, match="minimum side"):           # periodization: 5x7 -> 3x4 -> 2x2, below the minimum of 3
        fa.DWTForward(J=3, wave=d2, mode="periodization").cuda()(torch.zeros(1, 1, 5, 7, device="cuda"))
    assert calls == ["dwt2d_analysis", "dwt2d_analysis"]
    torch.cuda.synchronize()


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
    """weight * sum over both cycles and all levels of mean |yh(recovered) - yh(real)|, in float64."""
    ab = [getattr(fa.DWTForward(J=J, wave=fa.daubechies(4), mode=mode), n).double() for n in A_BUFS]
    tot = 0.0
    for rec, real in (("recovered_A", "real_A"), ("recovered_B", "real_B")):
        _, yr = forward_levels(T[rec].detach().cpu().double(), ab, mode, J)
        _, yt = forward_levels(T[real].detach().cpu().double(), ab, mode, J)
        tot += sum(float((a - b).abs().mean()) for a, b in zip(yr, yt))
    return weight * tot


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_train_step_whf_term_on_db4(fa, O, precision):
    """192^2, batch 2: the term is what the restatement gives on the step's own tensors, it is what loss_G gains, it moves the
    generators' gradient norms, and the other losses stay at the weight-0 step's values (the TV test's bars).

    "Moves" is measured against the step's own repeatability: the weight-0 step is run twice from the same state, and the norm
    of at least one generator has to differ from the weight-0 norm by more than ten times the difference between those twins,
    and by more than 1e-5 relative (five times the 2e-6 by which two runs' gradient arenas differ through the order of their fp32
    atomics) where the twins happen to agree.  A fixed fraction of the norm would say nothing here: the
    term's gradient (weight 0.1, the sign pattern of band differences) is nearly orthogonal to the cycle terms' (weight 2), so
    the norm changes in second order."""
    a, b = (t.cuda() for t in O.synthetic_batch(2, 192))
    kw = dict(whf_weight=0.1, dwt_levels=2, dwt_wave=fa.daubechies(4), dwt_mode="symmetric")
    ts = fresh_step(fa, O, precision=precision, **kw)
    L = ts.step(a, b, sync=True, keep=True)
    gn = ts.grad_norms()
    ts0 = fresh_step(fa, O, precision=precision)
    L0 = ts0.step(a, b, sync=True, keep=True)
    gn0 = ts0.grad_norms()
    twin = fresh_step(fa, O, precision=precision)
    twin.step(a, b, sync=True)
    gn1 = twin.grad_norms()
    assert "loss_whf" not in L0
    T = dict(L["tensors"])
    T.setdefault("real_A", a)
    T.setdefault("real_B", b)
    want = whf_restatement(fa, T, 0.1, 2, "symmetric")
    print("DWT_ERR step %s: loss_whf %.7f restatement %.7f, loss_G %.6f against %.6f at weight 0, |grad A2B| %.5f against %.5f, |grad B2A| %.5f against %.5f"
          % (precision, L["loss_whf"], want, L["loss_G"], L0["loss_G"], gn["A2B"], gn0["A2B"], gn["B2A"], gn0["B2A"]))
    assert abs(L["loss_whf"] - want) <= 1e-3 * abs(want)
    assert abs((L["loss_G"] - L0["loss_G"]) - L["loss_whf"]) <= 1e-3 * abs(L["loss_G"])
    moved = {k: abs(gn[k] - gn0[k]) for k in ("A2B", "B2A")}
    noise = {k: abs(gn1[k] - gn0[k]) for k in ("A2B", "B2A")}
    print("DWT_ERR step %s: gradient norms moved by %s, weight-0 twins differ by %s" % (precision, moved, noise))
    assert any(moved[k] > max(10.0 * noise[k], 1e-5 * gn0[k]) for k in moved), (gn, gn0, gn1)
    for k in L0:
        if k not in ("tensors", "loss_G"):
            assert abs(L[k] - L0[k]) <= 1e-3 * max(abs(L0[k]), 2e-2), (k, L[k], L0[k])


def test_graph_captured_step_with_db4_whf_term(fa, O):
    """Three replays of the captured step follow the eager one at the bars of the existing graph tests; ``loss_whf``, an L1 on the
    recovered images like the cycle terms, is held to their relative bar (3e-3 after step 0), not to an absolute one: at weight
    0.1 its value is of the size of the absolute bars."""
    kw = dict(whf_weight=0.1, dwt_levels=2, dwt_wave=fa.daubechies(4), dwt_mode="symmetric")
    batches = [tuple(t.cuda() for t in O.synthetic_batch(2, 192, seed=1234 + 17 * s)) for s in range(3)]
    eager = fresh_step(fa, O, precision="f32", **kw)
    Le = [eager.step(a, b, sync=True) for a, b in batches]
    ts = fresh_step(fa, O, precision="f32", **kw)
    gs = fa.GraphedTrainStep(ts, batches[0][0], batches[0][1])
    Lg = [gs.step(a, b, sync=True) for a, b in batches]
    for s in range(3):
        print("DWT_ERR graph step %d: loss_whf %.7f eager %.7f, loss_G %.6f eager %.6f" % (s, Lg[s]["loss_whf"], Le[s]["loss_whf"], Lg[s]["loss_G"], Le[s]["loss_G"]))
        for k in ("loss_whf", "loss_G"):
            tol = 2e-4 if s == 0 else 3e-3
            assert Lg[s][k] == pytest.approx(Le[s][k], rel=tol, abs=1e-6), (s, k, Lg[s][k], Le[s][k])
    assert ts.opt_G.step_count == 3
