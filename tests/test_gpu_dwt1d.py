"""The 1-D filter-bank DWT / IDWT (csrc/dwt1d.hip) on the MI355X: ``DWT1DForward`` / ``DWT1DInverse`` against the reference's own
CPU results (tests/golden/golden_dwt1d*.npz) and against the float64 restatement of tests/test_dwt1d_cpu.py (pinned to those
fixtures there), the two launch shapes, and structural properties.

The error bar is the 2-D test's, in relative L2 against the float64 restatement:   e_hip <= 2 e_ref + 2^-23
with e_ref the fp32 reference's own distance from it (the fixture's arrays; for off-fixture shapes and the cases the reference
refuses, the restatement run in fp32 on the CPU).  Kernel and reference both add L terms per level in fp32 and differ in the
order of those sums (the kernels contract to fused multiply-adds), which the factor 2 leaves room for; 2^-23 keeps the bar
satisfiable where e_ref happens to be tiny.  Measured on an MI355X (profiles/dwt1d_error.txt): over 598 arrays e_hip / e_ref
0.40 - 1.85, median 1.00; reconstruction max-abs at most 6.6e-7.

The backward passes are the reference's definitions (wavelets.py), so the dot-product identity is asserted only where those are
the adjoint: 'zero' at any length and 'periodization' while every level's input is even."""
import pytest
import torch

from test_dwt1d_cpu import (BANK_ORDER, MODES, fixture_cases, fixture_inputs, forward_levels, gold, inverse_levels, out_size, refused,
                            rel_l2, restate, restate_case)

pytestmark = pytest.mark.gpu

K, FLOOR = 2.0, 2.0 ** -23


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def modules(fa, bank, mode, J):
    w = fa.daubechies(BANK_ORDER[bank])
    return fa.DWT1DForward(J=J, wave=w, mode=mode), fa.DWT1DInverse(wave=w, mode=mode)


def bufs64(fa, bank, mode="zero"):
    fwd, inv = modules(fa, bank, mode, 1)
    return tuple(b.double() for b in (fwd.h0, fwd.h1, inv.g0, inv.g1))


def run_hip(fa, bank, mode, J, x, cots, coeffs, cot_inv, fused=None):
    """Everything a fixture case holds, from the GPU: through the modules (``fused`` None), or through ``ops.dwt1d_analysis`` /
    ``ops.dwt1d_synthesis`` with the launch shape forced.  ``x`` may be a device tensor (a view is passed on as it is)."""
    fwd, inv = (m.cuda() for m in modules(fa, bank, mode, J))
    m = fa.wavelets.mode_to_int(mode)
    if fused is None:
        analysis, synthesis = fwd, inv
    else:
        analysis = lambda t: fa.ops.dwt1d_analysis(t, fwd.h0, fwd.h1, m, J, fused=fused)
        synthesis = lambda c: fa.ops.dwt1d_synthesis(c[0], c[1], inv.g0, inv.g1, m, fused=fused)
    xd = (x if x.is_cuda else x.cuda()).detach().requires_grad_(True)
    yl, yh = analysis(xd)
    assert yl.is_contiguous() and all(h.is_contiguous() for h in yh) and len(yh) == J
    out = {"yl": yl.detach().cpu()}
    for j, h in enumerate(yh):
        out["yh%d" % j] = h.detach().cpu()
    if cots is not None:
        torch.autograd.backward([yl] + list(yh), [c.cuda() for c in cots])
        out["xgrad"] = xd.grad.cpu()
        cl = coeffs[0].cuda().requires_grad_(True)
        ch = [h.cuda() for h in coeffs[1]]
        ch[0].requires_grad_(True)
        y = synthesis((cl, ch))
        assert y.is_contiguous()
        out["inv"] = y.detach().cpu()
        y.backward(cot_inv.cuda())
        out["inv_gyl"], out["inv_gyh0"] = cl.grad.cpu(), ch[0].grad.cpu()
        with torch.no_grad():
            out["inv_none"] = synthesis((cl.detach(), [h.detach() for h in ch[:-1]] + [None])).cpu()
    torch.cuda.synchronize()
    return out


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bar of the module docstring on every one."""
    bad = []
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (name, k, tuple(got[k].shape), tuple(ref64[k].shape))
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("DWT1D_ERR %-40s %-8s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_fixture_parity(fa, case):
    """Outputs, x.grad, the inverse, its gradients and the None level of every fixture case; e_ref is the fixture's own error.
    The two cases the reference refuses ('reflect' at the minimum length) take e_ref from the restatement in fp32, outputs only."""
    cid, bank, mode, J, shape = case
    g = gold()
    x, cots, coeffs, cot_inv = fixture_inputs(case)
    ref64 = restate_case(case)
    ref32 = restate_case(case, torch.float32) if refused(cid) else {k: torch.from_numpy(g[cid + "/" + k]) for k in ref64}
    hold_to_bar(cid, ref64, ref32, run_hip(fa, bank, mode, J, x, cots, coeffs, cot_inv))


def free_inputs(fa, bank, mode, J, x):
    """Cotangents and the coefficients the inverse runs on (the fp64 forward's, rounded to fp32) for an off-fixture input."""
    gen = torch.Generator().manual_seed(99)
    b = bufs64(fa, bank)
    yl, yh = forward_levels(x.double(), b[0], b[1], mode, J)
    cots = [torch.rand(t.shape, generator=gen) - 0.5 for t in [yl] + yh]
    coeffs = (yl.float(), [h.float() for h in yh])
    cot_inv = torch.rand(inverse_levels(yl, yh, b[2], b[3], mode).shape, generator=gen) - 0.5
    return cots, coeffs, cot_inv


def free_case(fa, name, bank, mode, J, x, view=None, fused=None):
    cots, coeffs, cot_inv = free_inputs(fa, bank, mode, J, x)
    b = bufs64(fa, bank)
    ref64 = restate(x, b, mode, J, cots, coeffs, cot_inv, torch.float64)
    ref32 = restate(x, b, mode, J, cots, coeffs, cot_inv, torch.float32)
    got = run_hip(fa, bank, mode, J, x if view is None else view, cots, coeffs, cot_inv, fused=fused)
    hold_to_bar(name, ref64, ref32, got)
    return got


@pytest.mark.parametrize("mode", MODES)
def test_off_fixture_sweep(fa, mode):
    """16 taps at an odd length, the minimum length of db8 (9 = L/2 + 1, where the folding modes fold more than once and a level
    is longer than its input), three levels at 301, eight levels of db2 at 1000."""
    g = torch.Generator().manual_seed(7)
    free_case(fa, "3x2x33 db8 %s" % mode, "db8", mode, 1, torch.randn(3, 2, 33, generator=g))
    free_case(fa, "1x1x9 db8 %s" % mode, "db8", mode, 1, torch.randn(1, 1, 9, generator=g))
    free_case(fa, "2x1x301 db4 J3 %s" % mode, "db4", mode, 3, torch.randn(2, 1, 301, generator=g))
    free_case(fa, "1x2x1000 db2 J8 %s" % mode, "db2", mode, 8, torch.randn(1, 2, 1000, generator=g))


def counted(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def four_steps(fa, calls, bank, mode, J, x, fused):
    """[forward, its backward, inverse, its backward] -> the entry points each reached, and every output and gradient."""
    fwd, inv = (m.cuda() for m in modules(fa, bank, mode, J))
    m = fa.wavelets.mode_to_int(mode)
    seen, out = [], {}

    def step():
        seen.append(list(calls))
        del calls[:]
    del calls[:]
    xd = x.cuda().requires_grad_(True)
    yl, yh = fwd(xd) if fused is None else fa.ops.dwt1d_analysis(xd, fwd.h0, fwd.h1, m, J, fused=fused)
    step()
    torch.autograd.backward([yl] + list(yh), [torch.full_like(t, 0.25) for t in [yl] + list(yh)])
    step()
    cl = yl.detach().clone().requires_grad_(True)
    ch = [h.detach().clone().requires_grad_(True) for h in yh]
    y = inv((cl, ch)) if fused is None else fa.ops.dwt1d_synthesis(cl, ch, inv.g0, inv.g1, m, fused=fused)
    step()
    y.backward(torch.full_like(y, 0.5))
    step()
    torch.cuda.synchronize()
    out.update(yl=yl.detach(), xgrad=xd.grad, inv=y.detach(), inv_gyl=cl.grad)
    for j in range(J):
        out["yh%d" % j], out["inv_gyh%d" % j] = yh[j].detach(), ch[j].grad
    return seen, {k: v.cpu() for k, v in out.items()}


def test_launch_shapes(fa, monkeypatch):
    """One entry-point call per pass when fused, J when tiled, the tiled launch beyond the limit -- and the same bits either way."""
    calls = counted(fa, monkeypatch)
    x = torch.randn(2, 3, 301, generator=torch.Generator().manual_seed(31))
    a, s = "dwt1d_analysis", "dwt1d_synthesis"
    seen, fused = four_steps(fa, calls, "db4", "symmetric", 3, x, None)
    assert seen == [[a], [s], [s], [a]], seen
    seen, forced = four_steps(fa, calls, "db4", "symmetric", 3, x, True)
    assert seen == [[a], [s], [s], [a]], seen
    seen, tiled = four_steps(fa, calls, "db4", "symmetric", 3, x, False)
    assert seen == [[a] * 3, [s] * 3, [s] * 3, [a] * 3], seen
    assert sorted(fused) == sorted(tiled) and len(fused) == 4 + 2 * 3
    for k in fused:
        assert torch.equal(fused[k], tiled[k]) and torch.equal(fused[k], forced[k]), k
    n = fa.DWT1D_FUSED_MAX + 37
    xl = torch.randn(2, 1, n, generator=torch.Generator().manual_seed(32))
    seen, _ = four_steps(fa, calls, "db4", "symmetric", 2, xl, None)
    assert seen == [[a] * 2, [s] * 2, [s] * 2, [a] * 2], seen
    with pytest.raises(ValueError, match="DWT1D_FUSED_MAX"):
        fa.ops.dwt1d_analysis(xl.cuda(), *modules(fa, "db4", "symmetric", 2)[0].cuda().buffers(), 1, 2, fused=True)


@pytest.mark.parametrize("mode", ("symmetric", "periodization"))
def test_beyond_the_fused_limit(fa, mode):
    """DWT1D_FUSED_MAX + 37 samples, 2 x 1 rows, J = 2: several tiles a row, at the bar of the fixture test."""
    n = fa.DWT1D_FUSED_MAX + 37
    free_case(fa, "2x1x%d db4 J2 %s" % (n, mode), "db4", mode, 2, torch.randn(2, 1, n, generator=torch.Generator().manual_seed(33)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bank", ("db2", "db4", "db8"))
def test_perfect_reconstruction(fa, bank, mode):
    """inv(fwd(x))[..., :L] == x within 4e-6 max-abs at 2 x 3 x 101, J = 2: the 2-D test's bar, which covers two passes per level
    where this has one; the reference's own figure on the CPU was at most 7.2e-7."""
    x = torch.randn(2, 3, 101, generator=torch.Generator().manual_seed(21)).cuda()
    fwd, inv = (m.cuda() for m in modules(fa, bank, mode, 2))
    yl, yh = fwd(x)
    L = 2 * BANK_ORDER[bank]
    n1 = out_size(101, L, mode)
    n2 = out_size(n1, L, mode)
    assert tuple(yl.shape) == (2, 3, n2) and [tuple(h.shape) for h in yh] == [(2, 3, n1), (2, 3, n2)]
    y = inv((yl, yh))
    assert tuple(y.shape) == (2, 3, 102)
    err = float((y[..., :101] - x).abs().max())
    print("DWT1D_ERR reconstruction %s %s max-abs %.3e" % (bank, mode, err))
    assert err <= 4e-6


@pytest.mark.parametrize("mode,shape", [("zero", (2, 3, 37)), ("zero", (1, 1, 64)), ("periodization", (2, 3, 64))])
def test_backward_is_the_adjoint_where_the_reference_is(fa, mode, shape):
    """<A x, c> == <x, A^T c> with A^T the backward, relative 1e-5, for the J = 2 forward and for the J = 2 inverse."""
    g = torch.Generator().manual_seed(5)
    fwd, inv = (m.cuda() for m in modules(fa, "db4", mode, 2))
    x = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    yl, yh = fwd(x)
    outs = [yl] + list(yh)
    cs = [torch.randn(t.shape, generator=g).cuda() for t in outs]
    lhs = sum(float((t.detach().double() * c.double()).sum()) for t, c in zip(outs, cs))
    torch.autograd.backward(outs, cs)
    rhs = float((x.detach().double() * x.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    # the inverse drops a surplus sample between levels at 64 ('zero': 21 -> 36 for a highpass of 35); its backward's zero is the drop's adjoint
    cs = [c.detach().clone().requires_grad_(True) for c in cs]
    y = inv((cs[0], cs[1:]))
    cy = torch.randn(y.shape, generator=g).cuda()
    lhs = float((y.detach().double() * cy.double()).sum())
    y.backward(cy)
    rhs = sum(float((c.detach().double() * c.grad.double()).sum()) for c in cs)
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_strided_rows_give_the_bits_of_their_copy(fa, monkeypatch):
    """Rows 3:40 of every plane of a 2 x 4 x 90 x 64 tensor, as 8 x 37 rows of 64 samples: a view whose samples are contiguous
    and whose leading dimensions are not.  It is read in place (no copy kernel: one entry-point call, and ``contiguous`` is not
    asked for) and gives the bits of its contiguous copy, in the forward and, as a cotangent, in the inverse's backward."""
    big = torch.randn(2, 4, 90, 64, generator=torch.Generator().manual_seed(13)).cuda()
    view = big.reshape(8, 90, 64)[:, 3:40]
    assert not view.is_contiguous() and view.stride(-1) == 1 and view.data_ptr() == big[:, :, 3:40].data_ptr()
    copy = view.contiguous()
    fwd, inv = (m.cuda() for m in modules(fa, "db4", "symmetric", 2))
    want = fwd(copy)
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("the view was copied")))
    got = fwd(view)
    monkeypatch.undo()
    assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    x = torch.randn(8, 37, 64, generator=torch.Generator().manual_seed(14)).cuda()
    got, want = fwd(x.transpose(1, 2).contiguous().transpose(1, 2)), fwd(x)         # samples not contiguous: made contiguous first
    assert torch.equal(got[0], want[0])
    grads = []
    for cot in (view, copy):                                    # a strided cotangent and a strided lowpass
        cl = want[0].detach().clone().requires_grad_(True)
        y = inv((cl, [h.detach() for h in want[1]]))
        assert tuple(y.shape) == (8, 37, 64)
        y.backward(cot)
        grads.append(cl.grad)
    assert torch.equal(grads[0], grads[1])
    wide = torch.zeros(8, 37, want[0].shape[-1] + 5, device="cuda")
    wide[..., :want[0].shape[-1]] = want[0]
    y0 = inv((want[0], want[1]))
    y1 = inv((wide[..., :want[0].shape[-1]], want[1]))
    assert torch.equal(y0, y1)
    torch.cuda.synchronize()


def test_bit_reproducible_on_streams_and_in_a_graph(fa):
    x = torch.randn(2, 3, 301, generator=torch.Generator().manual_seed(3))
    cots, coeffs, cot_inv = free_inputs(fa, "db4", "symmetric", 3, x)

    def once():
        return run_hip(fa, "db4", "symmetric", 3, x, cots, coeffs, cot_inv)
    first, again = once(), once()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = once()
    torch.cuda.current_stream().wait_stream(s)
    for k in first:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], side[k]), k

    # a captured forward + backward replays to the eager bits (the modules were called above: their taps are on the host)
    fwd = modules(fa, "db4", "symmetric", 3)[0].cuda()
    xs = x.cuda().requires_grad_(True)
    cd = [c.cuda() for c in cots]
    fwd(xs.detach())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yl, yh = fwd(xs)
        (gx,) = torch.autograd.grad([yl] + list(yh), [xs], cd)
    for t in [yl, gx] + list(yh):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yl.cpu(), first["yl"]) and torch.equal(gx.cpu(), first["xgrad"])
    for j, h in enumerate(yh):
        assert torch.equal(h.cpu(), first["yh%d" % j])


def test_none_levels_and_the_surplus_sample(fa, monkeypatch):
    """Length 13, db4, 'symmetric', J = 2: 13 -> 10 -> 8, and the inverse's coarsest level returns 10 = 2 * 8 - 6 samples for a
    highpass of 10, the finest 14 for the 13 that went in; with a lowpass one sample too long at BOTH levels (yl of 9 for a
    highpass of 8 ...) the surplus is dropped and its gradient is a zero.  Held to the fixture test's bar with every gradient;
    then a lowpass two samples too long raises ``ValueError`` and reaches no entry point."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(2, 3, 13, generator=g)
    got = free_case(fa, "2x3x13 db4 J2 symmetric", "db4", "symmetric", 2, x)
    assert got["yl"].shape[-1] == 8 and got["yh0"].shape[-1] == 10 and got["inv"].shape[-1] == 14
    # the surplus-sample path: 9 coefficients where 8 belong -> 8 -> a result of 10 ...; and periodization 13 -> 7 -> 4: 2 * 4 = 8 > 7
    b = bufs64(fa, "db4")
    for mode, lens in (("symmetric", (9, [10, 8])), ("periodization", (4, [7, 4])), ("periodization", (5, [7, 4]))):
        cl = torch.randn(2, 3, lens[0], generator=g)
        ch = [torch.randn(2, 3, n, generator=g) for n in lens[1]]
        cot = torch.rand(inverse_levels(cl.double(), [h.double() for h in ch], b[2], b[3], mode).shape, generator=g) - 0.5
        name = "surplus %s %d %s" % (mode, lens[0], lens[1])
        ref = {}
        for dtype in (torch.float64, torch.float32):
            r = restate(x, b, mode, 2, [torch.zeros(2, 3, out_size(out_size(13, 8, mode), 8, mode))] + [torch.zeros(2, 3, n) for n in lens[1]],
                        (cl, ch), cot, dtype, none_level=False)
            ref[dtype] = {k: r[k] for k in ("inv", "inv_gyl", "inv_gyh0")}
        inv = modules(fa, "db4", mode, 2)[1].cuda()
        cld = cl.cuda().requires_grad_(True)
        chd = [h.cuda().requires_grad_(True) for h in ch]
        y = inv((cld, chd))
        y.backward(cot.cuda())
        out = {"inv": y.detach().cpu(), "inv_gyl": cld.grad.cpu(), "inv_gyh0": chd[0].grad.cpu()}
        hold_to_bar(name, ref[torch.float64], ref[torch.float32], out)
        if lens[0] > lens[1][1]:
            assert float(cld.grad[..., -1].abs().max()) == 0.0          # the dropped sample
    calls = counted(fa, monkeypatch)
    inv = modules(fa, "db4", "symmetric", 2)[1].cuda()
    with pytest.raises(ValueError, match="does not belong"):
        inv((torch.zeros(2, 3, 10, device="cuda"), [torch.zeros(2, 3, 10, device="cuda"), torch.zeros(2, 3, 8, device="cuda")]))
    with pytest.raises(ValueError, match="minimum length"):
        modules(fa, "db4", "symmetric", 1)[0].cuda()(torch.zeros(1, 1, 4, device="cuda"))
    assert calls == []
    torch.cuda.synchronize()
