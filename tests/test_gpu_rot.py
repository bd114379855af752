"""The three-filter (rotationally symmetric) forms of the dual-tree and scattering kernels on the MI355X: ``ScatLayer`` /
``ScatLayerj2`` / ``DTCWTForward`` / ``DTCWTInverse`` with 3-tuple / 6-tuple taps against the reference's own CPU results
(tests/golden/golden_rot_*.npz) and the float64 restatement of tests/test_rot_cpu.py (pinned to those fixtures there), tile seams
with the fixture bank and with a synthetic one, the launch structure and structural properties.

The error bar is the project's, in relative L2 against the float64 restatement:   e_hip <= 2 e_ref + 2^-23
with e_ref the fp32 reference's own distance from it (the fixture's ``f32`` arrays; off the fixtures, the restatement run in fp32
on the CPU).  Every array prints e_ref, e_hip and their ratio as a ``ROT_ERR`` line (run with ``-s``; a run's lines are what
profiles/rot_error.txt holds)."""
import pytest
import torch
import torch.nn.functional as F

from test_dtcwt_cpu import decode, rel_l2
from test_scat_cpu import tuples as scat_tuples
from test_rot_cpu import (DT_J, bufs, dt_cases, dt_inputs, forward_levels, gold, inverse_levels, restate_dt, restate_scat,
                          scat_cases, synthetic_bufs, third_filter, tuples)

pytestmark = pytest.mark.gpu

K, FLOOR = 2.0, 2.0 ** -23
PHASE_ARG = {"scat_fwd_j1": 12, "scat_fwd_j2": 11}           # position of the phasor pointer in the entry points' arguments
# the third filter's position is THIRD_ARG of test_rot_cpu.py (the CPU tests build calls from it): third_filter(name, args) reads it
DEFAULT = ("n", "c", "o", "h", "w", "r")
BANKS = {"fixture": bufs, "synthetic": synthetic_bufs}


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def layer(fa, b, order, mode="symmetric", colour=False):
    fb, fq = tuples(b)
    if order == 1:
        return fa.ScatLayer(biort=fb, mode=mode, combine_colour=colour).cuda()
    return fa.ScatLayerj2(biort=fb, qshift=fq, mode=mode, combine_colour=colour).cuda()


def modules(fa, b, mode="symmetric", J=DT_J, **kw):
    (fb, fq), (gb, gq) = tuples(b), tuples(b, analysis=False)
    o = {k: kw[k] for k in ("o_dim", "ri_dim") if k in kw}
    return fa.DTCWTForward(biort=fb, qshift=fq, J=J, mode=mode, **kw).cuda(), fa.DTCWTInverse(biort=gb, qshift=gq, mode=mode, **o).cuda()


def run_scat(mod, x, cot):
    xd = (x if x.is_cuda else x.float().cuda()).detach().requires_grad_(True)
    Z = mod(xd)
    Z.backward(cot.cuda())
    torch.cuda.synchronize()
    return {"Z": Z.detach().cpu(), "xgrad": xd.grad.cpu()}


def run_dt(fa, b, mode, J, x, cots, coeffs, cot_inv):
    """Everything a golden_rot_dtcwt.npz case holds, from the GPU."""
    fwd, inv = modules(fa, b, mode, J)
    xd = x.float().cuda().requires_grad_(True)
    yl, yh = fwd(xd)
    assert yl.is_contiguous() and all(h.is_contiguous() for h in yh) and len(yh) == J
    out = {"yl": yl.detach().cpu()}
    out.update({"yh%d" % j: h.detach().cpu() for j, h in enumerate(yh)})
    torch.autograd.backward([yl] + list(yh), [c.cuda() for c in cots])
    out["xgrad"] = xd.grad.cpu()
    cl = coeffs[0].cuda().requires_grad_(True)
    ch = [h.cuda().requires_grad_(True) for h in coeffs[1]]
    y = inv((cl, ch))
    out["inv"] = y.detach().cpu()
    y.backward(cot_inv.cuda())
    out["inv_gyl"] = cl.grad.cpu()
    out.update({"inv_gyh%d" % j: h.grad.cpu() for j, h in enumerate(ch)})
    torch.cuda.synchronize()
    return out


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bar of the module docstring on every one."""
    bad = []
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (name, k, tuple(got[k].shape), tuple(ref64[k].shape))
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("ROT_ERR %-40s %-9s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------------------------------
# parity
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", scat_cases(), ids=lambda c: c[0])
def test_scat_fixture_parity(fa, case):
    """Z and x.grad of every case of golden_rot_scat.npz."""
    cid, order, mode, shape, colour = case
    g = gold("scat")
    x, cot = torch.from_numpy(g["x_%dx%dx%dx%d" % shape]), decode(g[cid + "/cot"])
    ref64 = restate_scat(x, bufs(), order, mode, colour, cot, torch.float64)
    ref32 = {k: torch.from_numpy(g[cid + "/f32/" + k]) for k in ref64}
    hold_to_bar(cid, ref64, ref32, run_scat(layer(fa, bufs(), order, mode, colour), x, cot))


@pytest.mark.parametrize("case", dt_cases(), ids=lambda c: c[0])
def test_dtcwt_fixture_parity(fa, case):
    """Outputs, x.grad, the inverse and its gradients to yl and every yh of every case of golden_rot_dtcwt.npz."""
    cid, mode, shape = case
    g = gold("dtcwt")
    x, cots, coeffs, cot_inv = dt_inputs(case)
    ref64, _ = restate_dt(x, bufs(), mode, DT_J, cots, coeffs, cot_inv, torch.float64)
    ref32 = {k: torch.from_numpy(g[cid + "/f32/" + k]) for k in ref64}
    hold_to_bar(cid, ref64, ref32, run_dt(fa, bufs(), mode, DT_J, x, cots, coeffs, cot_inv))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("bank", list(BANKS))
def test_scat_tile_seams(fa, bank, order):
    """``ScatLayer`` on 36 x 252: the level-1 kernels tile 16 x 64 (two tiles + 4 rows, four tiles - 4 columns).  ``ScatLayerj2`` on
    40 x 136: level 1 on 40 x 136 and, second order, on 20 x 68; the level-2 forward tiles 16 x 128 of its input, the level-2
    backward 32 x 64 of its result -- each of the six launches crosses a tile boundary in both axes and ends in a remainder tile.
    The fixture bank has the 19-tap halo and m/2 odd (7); the synthetic one a 3-tap third filter under a 7-tap halo (its own
    centring offset), m/2 even (8), and pads ``ScatLayer`` with zeros."""
    b = BANKS[bank]()
    shape = (1, 2, 36, 252) if order == 1 else (1, 2, 40, 136)
    gen = torch.Generator().manual_seed(21 + order)
    x = torch.randn(*shape, generator=gen)
    mode = "zero" if (order, bank) == (1, "synthetic") else "symmetric"
    out = (shape[0], (7 if order == 1 else 49) * shape[1], shape[2] // (2 * order), shape[3] // (2 * order))
    cot = torch.rand(out, generator=gen) - 0.5
    ref64 = restate_scat(x, b, order, mode, False, cot, torch.float64)
    ref32 = restate_scat(x, b, order, mode, False, cot, torch.float32)
    hold_to_bar("seams %s j%d %s %s" % ("x".join(map(str, shape)), order, bank, mode), ref64, ref32, run_scat(layer(fa, b, order, mode), x, cot))


@pytest.mark.parametrize("bank", list(BANKS))
def test_dtcwt_tile_seams(fa, bank):
    """36 x 252, two channels, J = 3 (the third level pads its 18 x 126 input to 20 x 128, the inverse crops it back).  The
    level-1 kernels tile 16 x 64 (36 = 2 tiles + 4, 252 = 4 tiles - 4), the level-2 forward 16 x 128 of its input (two tiles + 4
    rows, two tiles - 4 columns), the level-2 inverse 32 x 64 of its result (one tile + 4, four tiles - 4): every kernel
    crosses its tiles in both axes and ends in a remainder tile.  The synthetic bank runs level 1 with zero padding."""
    b = BANKS[bank]()
    mode = "zero" if bank == "synthetic" else "symmetric"
    x = torch.randn(1, 2, 36, 252, generator=torch.Generator().manual_seed(31))
    gen = torch.Generator().manual_seed(99)
    with torch.no_grad():
        yl, yh = forward_levels(x.double(), b, mode, DT_J)
        coeffs = (yl.float(), [h.float() for h in yh])
        cot_inv = torch.rand(inverse_levels(yl, yh, b, mode).shape, generator=gen) - 0.5
    cots = [torch.rand(t.shape, generator=gen) - 0.5 for t in [yl] + yh]
    ref64, _ = restate_dt(x, b, mode, DT_J, cots, coeffs, cot_inv, torch.float64)
    ref32, _ = restate_dt(x, b, mode, DT_J, cots, coeffs, cot_inv, torch.float32)
    hold_to_bar("seams 1x2x36x252 J3 %s %s" % (bank, mode), ref64, ref32, run_dt(fa, b, mode, DT_J, x, cots, coeffs, cot_inv))


@pytest.mark.parametrize("bank,mode", [("fixture", "symmetric"), ("synthetic", "zero")])
def test_consistency_with_the_dtcwt_kernels(fa, bank, mode):
    """The pooled lowpass and the magnitudes from ``ops.dtcwt_fwd_j1(..., h2o=...)``'s outputs by torch ops: the filters' sums are the
    same, the pointwise operations may differ by a rounding -- 2^-22 in relative L2."""
    x = torch.randn(2, 2, 36, 72, generator=torch.Generator().manual_seed(7)).cuda()
    mod = layer(fa, BANKS[bank](), 1, mode)
    with torch.no_grad():
        Z = mod(x).view(2, 7, 2, 18, 36)
        ll, h = fa.ops.dtcwt_fwd_j1(x, mod.h0o, mod.h1o, False, 2, -1, mod.mode, h2o=mod.h2o)
        b = torch.tensor(mod.magbias, dtype=torch.float32, device="cuda")
        mag = torch.sqrt(h[..., 0] ** 2 + h[..., 1] ** 2 + b * b) - b                      # (N, C, 6, h, w)
        e_low, e_mag = rel_l2(Z[:, 0].cpu(), F.avg_pool2d(ll, 2).cpu()), rel_l2(Z[:, 1:].cpu(), mag.transpose(1, 2).cpu())
    print("ROT_CONSIST bank %s %s low %.3e mag %.3e" % (bank, mode, e_low, e_mag))
    assert e_low <= 2.0 ** -22 and e_mag <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def launches(calls, third=True):
    """The entry points of the recorded calls, in order, once every one of them has (has not) its third filter."""
    assert all(third_filter(n, a) == third for n, a in calls), [(n, third_filter(n, a)) for n, a in calls]
    return [n for n, _ in calls]


@pytest.mark.parametrize("colour", [False, True])
def test_launch_counts_and_names(fa, monkeypatch, colour):
    x = torch.randn(1, 3, 64, 64).cuda().requires_grad_(True)
    one, two = layer(fa, bufs(), 1, "symmetric", colour), layer(fa, bufs(), 2, "symmetric", colour)
    calls = spy(fa, monkeypatch)
    Z = one(x)
    assert launches(calls) == ["scat_fwd_j1"]
    del calls[:]
    Z.backward(torch.ones_like(Z))
    assert launches(calls) == ["scat_bwd_j1"]
    del calls[:]
    Z = two(x)
    assert launches(calls) == ["scat_fwd_j1", "scat_fwd_j2", "scat_fwd_j1"]
    assert tuple(Z.shape) == (1, 51 if colour else 147, 16, 16) and Z.is_contiguous()
    del calls[:]
    Z.backward(torch.ones_like(Z))
    assert launches(calls) == ["scat_bwd_j1", "scat_bwd_j2", "scat_bwd_j1"]


def test_transform_launches(fa, monkeypatch):
    """One launch per level each way, every one with its third filter (at levels >= 2 both pointers of the pair); a level that
    skips its bandpass has no third filter to run and passes a NULL one: the two-filter lowpass form."""
    x = torch.randn(1, 2, 32, 32, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_(True)
    fwd, inv = modules(fa, bufs(), "symmetric", 3)
    calls = spy(fa, monkeypatch)
    yl, yh = fwd(x)
    assert launches(calls) == ["dtcwt_fwd_j1", "dtcwt_fwd_j2", "dtcwt_fwd_j2"]
    del calls[:]
    torch.autograd.backward([yl] + list(yh), [torch.ones_like(t) for t in [yl] + list(yh)])
    assert launches(calls) == ["dtcwt_inv_j2", "dtcwt_inv_j2", "dtcwt_inv_j1"]
    del calls[:]
    cl, ch = yl.detach().requires_grad_(True), [h.detach().requires_grad_(True) for h in yh]
    y = inv((cl, ch))
    assert launches(calls) == ["dtcwt_inv_j2", "dtcwt_inv_j2", "dtcwt_inv_j1"]
    del calls[:]
    y.backward(torch.ones_like(y))
    assert launches(calls) == ["dtcwt_fwd_j1", "dtcwt_fwd_j2", "dtcwt_fwd_j2"]
    del calls[:]
    skip = modules(fa, bufs(), "symmetric", 2, skip_hps=[False, True])[0]
    sl, sh = skip(x.detach())
    assert launches(calls[:1]) == ["dtcwt_fwd_j1"] and launches(calls[1:], third=False) == ["dtcwt_fwd_j2"] and sh[1].dim() == 0
    two = modules(fa, bufs(), "symmetric", 2)[0](x.detach())
    assert torch.equal(sl, two[0]) and torch.equal(sh[0], two[1][0])


@pytest.mark.parametrize("order,colour", [(1, False), (1, True), (2, False), (2, True)])
def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch, order, colour):
    mod = layer(fa, bufs(), order, "symmetric", colour)
    x = torch.randn(2, 3, 16, 24, generator=torch.Generator().manual_seed(2)).cuda()
    calls = spy(fa, monkeypatch)
    Zg = mod(x.clone().requires_grad_(True))
    assert len(calls) == (1 if order == 1 else 3) and all(a[PHASE_ARG[n]] for n, a in calls)      # phasors stored
    del calls[:]
    with torch.no_grad():
        Zn = mod(x.clone().requires_grad_(True))
    assert len(calls) == (1 if order == 1 else 3) and all(a[PHASE_ARG[n]] is None for n, a in calls)      # null phasor pointers
    del calls[:]
    Zp = mod(x)                                                       # an input that needs no gradient
    assert all(a[PHASE_ARG[n]] is None for n, a in calls) and not Zp.requires_grad
    assert torch.equal(Zn, Zg) and torch.equal(Zp, Zg)


@pytest.mark.parametrize("order", [1, 2])
def test_reproducible_and_batch_independent(fa, order):
    x = torch.randn(3, 2, 40, 72, generator=torch.Generator().manual_seed(9)).cuda()
    mod = layer(fa, bufs(), order)

    def both(t):
        t = t.detach().requires_grad_(True)
        Z = mod(t)
        Z.backward(torch.cos(torch.arange(Z.numel(), device="cuda", dtype=torch.float32)).reshape(Z.shape))
        return Z.detach(), t.grad

    Z, g = both(x)
    Z2, g2 = both(x)
    assert torch.equal(Z, Z2) and torch.equal(g, g2)
    planes = 7 if order == 1 else 49
    x1 = x[1:2, 1:2].contiguous().requires_grad_(True)
    Z1 = mod(x1)
    Zs = Z.view(3, planes, 2, Z.shape[2], Z.shape[3])[1:2, :, 1:2]
    assert torch.equal(Z1.view(Zs.shape), Zs)
    cot = torch.cos(torch.arange(Z.numel(), device="cuda", dtype=torch.float32)).reshape(3, planes, 2, Z.shape[2], Z.shape[3])[1:2, :, 1:2]
    Z1.backward(cot.reshape(Z1.shape))
    assert torch.equal(x1.grad, g[1:2, 1:2])
    cmod = layer(fa, bufs(), order, "symmetric", True)                # the colour form: the batch slice only
    xc = torch.randn(3, 3, 16, 24, generator=torch.Generator().manual_seed(10)).cuda()
    assert torch.equal(cmod(xc), cmod(xc)) and torch.equal(cmod(xc[1:2].contiguous()), cmod(xc)[1:2])


@pytest.mark.parametrize("order", [1, 2])
def test_a_strided_input_gives_its_contiguous_copys_bits(fa, order):
    big = torch.randn(2, 5, 16, 24, generator=torch.Generator().manual_seed(3)).cuda()
    mod = layer(fa, bufs(), order)
    view = big[:, 1:4]
    assert not view.is_contiguous()
    a, b = view.detach().requires_grad_(True), view.contiguous().requires_grad_(True)
    Za, Zb = mod(a), mod(b)
    assert torch.equal(Za, Zb)
    Za.backward(torch.ones_like(Za))
    Zb.backward(torch.ones_like(Zb))
    assert torch.equal(a.grad, b.grad)
    fwd = modules(fa, bufs(), "symmetric", 2)[0]
    (yl_v, yh_v), (yl_c, yh_c) = fwd(big[:, ::2]), fwd(big[:, ::2].contiguous())
    assert torch.equal(yl_v, yl_c) and all(torch.equal(p, q) for p, q in zip(yh_v, yh_c))


@pytest.mark.parametrize("o_dim,ri_dim", [(1, 2), (3, 0), (-2, 2)])
def test_a_layout_gives_the_default_layouts_values(fa, o_dim, ri_dim):
    """The forward's bandpass equals the default layout permuted; the inverse of it, and of a permuted VIEW of the default
    tensors, equals the default inverse -- bit for bit."""
    x = torch.randn(2, 2, 16, 24, generator=torch.Generator().manual_seed(5)).cuda()
    fwd, inv = modules(fa, bufs(), "symmetric", 2)
    yl, yh = fwd(x)
    y = inv((yl, yh))
    perm = [DEFAULT.index(k) for k in fa.ops.dtcwt_layout(o_dim, ri_dim)]
    f2, i2 = modules(fa, bufs(), "symmetric", 2, o_dim=o_dim, ri_dim=ri_dim)
    yl2, yh2 = f2(x)
    assert torch.equal(yl2, yl)
    for a, b in zip(yh2, yh):
        assert a.is_contiguous() and torch.equal(a, b.permute(perm))
    assert torch.equal(i2((yl2, yh2)), y)
    assert torch.equal(i2((yl, [h.permute(perm) for h in yh])), y)


def test_the_forwards_backward_is_the_inverse_kernel(fa):
    """Fed identical cotangents, ``DTCWTForward``'s gradient is ``DTCWTInverse.forward`` on the analysis taps with the trees swapped,
    the third pair included, bit for bit; and the inverse's gradients are the forward's outputs on the swapped synthesis taps."""
    b = bufs()
    (fb, fq), (gb, gq) = tuples(b), tuples(b, analysis=False)
    swap = lambda q: (q[1], q[0], q[3], q[2], q[5], q[4])       # noqa: E731
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(2, 2, 16, 24, generator=gen).cuda().requires_grad_(True)
    fwd, inv = modules(fa, b, "symmetric", 2)
    yl, yh = fwd(x)
    cots = [(torch.rand(t.shape, generator=gen) - 0.5).cuda() for t in [yl] + list(yh)]
    torch.autograd.backward([yl] + list(yh), cots)
    adj = fa.DTCWTInverse(biort=fb, qshift=swap(fq)).cuda()
    with torch.no_grad():
        assert torch.equal(adj((cots[0], cots[1:])), x.grad)
    cl, ch = yl.detach().requires_grad_(True), [h.detach().requires_grad_(True) for h in yh]
    y = inv((cl, ch))
    cot = (torch.rand(y.shape, generator=gen) - 0.5).cuda()
    y.backward(cot)
    with torch.no_grad():
        al, ah = fa.DTCWTForward(biort=gb, qshift=swap(gq), J=2).cuda()(cot)
    assert torch.equal(al, cl.grad) and all(torch.equal(p, q.grad) for p, q in zip(ah, ch))


def test_the_two_filter_path_is_untouched(fa, monkeypatch):
    """A two-filter ``ScatLayerj2`` and ``DTCWTForward`` on the two-filter fixture bank pass a NULL third filter to every entry point."""
    fb, fq = scat_tuples("a")
    two = fa.ScatLayerj2(biort=fb, qshift=fq).cuda()
    fwd = fa.DTCWTForward(biort=fb, qshift=fq, J=2).cuda()
    x = torch.randn(1, 2, 16, 24, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    calls = spy(fa, monkeypatch)
    Z = two(x)
    Z.backward(torch.ones_like(Z))
    yl, yh = fwd(x)
    torch.autograd.backward([yl] + list(yh), [torch.ones_like(t) for t in [yl] + list(yh)])
    assert launches(calls, third=False) == ["scat_fwd_j1", "scat_fwd_j2", "scat_fwd_j1", "scat_bwd_j1", "scat_bwd_j2", "scat_bwd_j1",
                                            "dtcwt_fwd_j1", "dtcwt_fwd_j2", "dtcwt_inv_j2", "dtcwt_inv_j1"]
