"""The dual-tree complex wavelet transform (csrc/dtcwt.hip) on the MI355X: ``DTCWTForward`` / ``DTCWTInverse`` against the
reference's own CPU results (tests/golden/golden_dtcwt_*.npz) and the float64 restatement of tests/test_dtcwt_cpu.py (pinned to
those fixtures there), tile seams, the layout and skip options, and structural properties.

The error bar is the project's, in relative L2 against the float64 restatement:   e_hip <= 2 e_ref + 2^-23
with e_ref the fp32 reference's own distance from it (the fixture's ``f32`` arrays; off the fixtures, the restatement run in fp32
on the CPU).  Kernel and reference both add the taps of a pass in fp32 and differ in the order and contraction of those sums,
which the factor 2 leaves room for; 2^-23 keeps the bar satisfiable where e_ref happens to be tiny.  Every array prints e_ref,
e_hip and their ratio as a ``DTCWT_ERR`` line (run with ``-s``; a run's lines are what profiles/dtcwt_error.txt is to hold)."""
import pytest
import torch

from test_dtcwt_cpu import (BANKS, FWD_BUFS, INV_BUFS, bufs, fixture_cases, fixture_inputs, forward_levels, gold, inverse_levels, rel_l2,
                            restate, restate_case, tuples)
from test_rot_cpu import third_filter

pytestmark = pytest.mark.gpu

K, FLOOR = 2.0, 2.0 ** -23
DEFAULT = ("n", "c", "o", "h", "w", "r")


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def modules(fa, bank, mode="symmetric", J=3, **kw):
    (fb, fq), (ib, iq) = tuples(bank)
    o = {k: kw[k] for k in ("o_dim", "ri_dim") if k in kw}
    return fa.DTCWTForward(biort=fb, qshift=fq, J=J, mode=mode, **kw).cuda(), fa.DTCWTInverse(biort=ib, qshift=iq, mode=mode, **o).cuda()


def run_hip(fa, bank, mode, J, x, cots, coeffs, cot_inv):
    """Everything a fixture case holds, from the GPU; ``x`` may be a device tensor (a view is passed on as it is)."""
    fwd, inv = modules(fa, bank, mode, J)
    xd = (x if x.is_cuda else x.float().cuda()).detach().requires_grad_(True)
    yl, yh = fwd(xd)
    assert yl.is_contiguous() and all(h.is_contiguous() for h in yh) and len(yh) == J
    out = {"yl": yl.detach().cpu()}
    for j, h in enumerate(yh):
        out["yh%d" % j] = h.detach().cpu()
    torch.autograd.backward([yl] + list(yh), [c.cuda() for c in cots])
    out["xgrad"] = xd.grad.cpu()
    cl = coeffs[0].cuda().requires_grad_(True)
    ch = [h.cuda() for h in coeffs[1]]
    ch[0].requires_grad_(True)
    y = inv((cl, ch))
    out["inv"] = y.detach().cpu()
    y.backward(cot_inv.cuda())
    out["inv_gyl"], out["inv_gyh0"] = cl.grad.cpu(), ch[0].grad.cpu()
    with torch.no_grad():
        out["inv_none"] = inv((cl.detach(), [h.detach() for h in ch[:-1]] + [None])).cpu()
        sl, sh = modules(fa, bank, mode, J, skip_hps=[False, True] + [False] * (J - 2))[0](xd.detach())
        assert sh[1].dim() == 0 and torch.equal(sh[0], yh[0])
        out["skip_yl"] = sl.cpu()
        for j in range(2, J):
            out["skip_yh%d" % j] = sh[j].cpu()
    torch.cuda.synchronize()
    return out


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bar of the module docstring on every one."""
    bad = []
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (name, k, tuple(got[k].shape), tuple(ref64[k].shape))
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("DTCWT_ERR %-34s %-9s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_fixture_parity(fa, case):
    """Outputs, x.grad, the inverse, its two gradients, the None level and the skip_hps forward of every fixture case."""
    cid, bank, mode, J, shape = case
    g = gold(bank, mode)
    ref64 = restate_case(case)
    ref32 = {k: torch.from_numpy(g[cid + "/f32/" + k]) for k in ref64}
    hold_to_bar(cid, ref64, ref32, run_hip(fa, bank, mode, J, *fixture_inputs(case)))


def free_case(fa, name, bank, mode, J, x, view=None):
    gen = torch.Generator().manual_seed(99)
    b = bufs(bank)
    with torch.no_grad():
        yl, yh = forward_levels(x.double(), b, mode, J)
        coeffs = (yl.float(), [h.float() for h in yh])
        cot_inv = torch.rand(inverse_levels(yl, yh, b, mode).shape, generator=gen) - 0.5
    cots = [torch.rand(t.shape, generator=gen) - 0.5 for t in [yl] + yh]
    ref64 = restate(x, b, mode, J, cots, coeffs, cot_inv, torch.float64)
    ref32 = restate(x, b, mode, J, cots, coeffs, cot_inv, torch.float32)
    got = run_hip(fa, bank, mode, J, x if view is None else view, cots, coeffs, cot_inv)
    hold_to_bar(name, ref64, ref32, got)
    return got


@pytest.mark.parametrize("bank,mode", [("a", "symmetric"), ("b", "zero"), ("c", "symmetric")])
def test_tile_seams(fa, bank, mode):
    """36 x 252, two channels, J = 2.  The level-1 kernels tile 16 x 64 (36 = 2 tiles + 4, 252 = 4 tiles - 4), the level-2 forward
    8 x 64 of its lowpass = 16 x 128 of its input (one tile + 4 rows twice over, two tiles - 4 columns), the level-2 inverse
    32 x 64 of its result (one tile + 4, four tiles - 4): every kernel crosses its tiles in both axes and ends in a remainder
    tile.  Bank a and c have m/2 odd (5, 9), bank b even (8)."""
    x = torch.randn(1, 2, 36, 252, generator=torch.Generator().manual_seed(11))
    free_case(fa, "seams 1x2x36x252 %s %s" % (bank, mode), bank, mode, 2, x)


def test_strided_inputs_cost_no_copy_and_change_no_bit(fa):
    """A channel slice of the input, and a lowpass the inverse crops by [1:-1] (13 x 18: every level pads), against contiguous
    copies."""
    g = torch.Generator().manual_seed(3)
    big = torch.randn(2, 5, 13, 18, generator=g).cuda()
    fwd, inv = modules(fa, "a", "symmetric", 3)
    view = big[:, 1:4]
    yl_v, yh_v = fwd(view)
    yl_c, yh_c = fwd(view.contiguous())
    assert torch.equal(yl_v, yl_c) and all(torch.equal(a, b) for a, b in zip(yh_v, yh_c))
    x_even = torch.randn(2, 5, 16, 24, generator=g).cuda()
    ll_v, h_v = fa.ops.dtcwt_fwd_j1(x_even[:, ::2], fwd.h0o, fwd.h1o)
    ll_c, h_c = fa.ops.dtcwt_fwd_j1(x_even[:, ::2].contiguous(), fwd.h0o, fwd.h1o)
    assert torch.equal(ll_v, ll_c) and torch.equal(h_v, h_c)
    y = inv((yl_c, yh_c))                                             # crops low[1:-1] at levels 2 and 1: strided lowpass inputs
    assert tuple(y.shape) == (2, 3, 14, 18)
    low = yl_c
    for j in (2, 1):
        if low.shape[2] != 2 * yh_c[j].shape[3]:
            low = low[:, :, 1:-1]
        if low.shape[3] != 2 * yh_c[j].shape[4]:
            low = low[:, :, :, 1:-1]
        low = fa.ops.dtcwt_inv_j2(low.contiguous(), yh_c[j], inv.g0a, inv.g0b, inv.g1a, inv.g1b)
    if low.shape[2] != 2 * yh_c[0].shape[3]:
        low = low[:, :, 1:-1]
    if low.shape[3] != 2 * yh_c[0].shape[4]:
        low = low[:, :, :, 1:-1]
    assert torch.equal(fa.ops.dtcwt_inv_j1(low.contiguous(), yh_c[0], inv.g0o, inv.g1o), y)
    assert float((y[:, :, :13] - view).abs().max()) < 1e-5


def test_every_layout_gives_the_default_layouts_bits(fa):
    """Every (o_dim, ri_dim) the reference accepts: the forward's bandpass equals the default layout permuted, the inverse of it
    (and of a permuted VIEW of the default tensors, for the matching module) equals the default inverse, bit for bit."""
    x = torch.randn(2, 2, 8, 12, generator=torch.Generator().manual_seed(5)).cuda()
    fwd, inv = modules(fa, "a", "symmetric", 2)
    yl, yh = fwd(x)
    y = inv((yl, yh))
    seen = 0
    for o in range(-6, 6):
        for r in range(-6, 6):
            try:
                names = fa.ops.dtcwt_layout(o, r)
            except ValueError:
                continue
            perm = [DEFAULT.index(k) for k in names]
            f2, i2 = modules(fa, "a", "symmetric", 2, o_dim=o, ri_dim=r)
            yl2, yh2 = f2(x)
            assert torch.equal(yl2, yl)
            for a, b in zip(yh2, yh):
                assert a.is_contiguous() and torch.equal(a, b.permute(perm)), (o, r)
            assert torch.equal(i2((yl2, yh2)), y), (o, r)
            assert torch.equal(i2((yl, [h.permute(perm) for h in yh])), y), (o, r)
            seen += 1
    assert seen > 100


def test_include_scale_skip_and_none(fa):
    x = torch.randn(1, 2, 16, 24, generator=torch.Generator().manual_seed(6)).cuda()
    fwd, inv = modules(fa, "b", "zero", 3)
    yl, yh = fwd(x)
    scales, yh2 = modules(fa, "b", "zero", 3, include_scale=[True, False, True])[0](x)
    assert len(scales) == 3 and tuple(scales[0].shape) == (1, 2, 16, 24) and scales[1].dim() == 0 and torch.equal(scales[2], yl)
    assert all(torch.equal(a, b) for a, b in zip(yh, yh2))
    scales, _ = modules(fa, "b", "zero", 3, include_scale=True)[0](x)
    assert [tuple(s.shape[2:]) for s in scales] == [(16, 24), (8, 12), (4, 6)]
    sl, sh = modules(fa, "b", "zero", 3, skip_hps=True)[0](x)
    assert torch.equal(sl, yl) and all(h.dim() == 0 for h in sh)
    for j in range(3):                                                # a None level, an empty tensor and zeros give the same bits
        hs = list(yh)
        hs[j] = None
        a = inv((yl, hs))
        hs[j] = torch.zeros_like(yh[j])
        assert torch.equal(a, inv((yl, hs)))
        hs[j] = torch.tensor([], device="cuda")
        assert torch.equal(a, inv((yl, hs)))
    assert torch.equal(inv((None, yh)), inv((torch.zeros_like(yl), yh)))
    # gradients: a skipped level sends nothing back, an unused output is a null pointer to the kernel
    xg = x.clone().requires_grad_(True)
    sl, sh = modules(fa, "b", "zero", 3, skip_hps=[False, True, True])[0](xg)
    (sl.sum() + sh[0].sum()).backward()
    xg2 = x.clone().requires_grad_(True)
    yl2, yh2 = fwd(xg2)
    (yl2.sum() + yh2[0].sum()).backward()
    assert rel_l2(xg.grad.cpu(), xg2.grad.cpu()) < 1e-6


@pytest.mark.parametrize("bank", BANKS)
def test_reconstruction(fa, bank):
    """DTCWTInverse(DTCWTForward(x)) on (2, 1, 32, 48) at J = 3: max-abs error at most twice the fp32 CPU restatement's, plus
    2^-23 max|x|."""
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(8))
    b32 = bufs(bank, torch.float32)
    with torch.no_grad():
        e_cpu = float((inverse_levels(*forward_levels(x, b32, "symmetric", 3), b32, "symmetric") - x).abs().max())
        fwd, inv = modules(fa, bank, "symmetric", 3)
        e_hip = float((inv(fwd(x.cuda())).cpu() - x).abs().max())
    print("DTCWT_RECON bank %s e_cpu32 %.3e e_hip %.3e" % (bank, e_cpu, e_hip))
    assert e_hip <= 2 * e_cpu + FLOOR * float(x.abs().max())


def test_reproducible_and_batch_independent(fa):
    x = torch.randn(3, 2, 36, 72, generator=torch.Generator().manual_seed(9)).cuda()
    fwd, inv = modules(fa, "c", "symmetric", 3)
    yl, yh = fwd(x)
    yl2, yh2 = fwd(x)
    assert torch.equal(yl, yl2) and all(torch.equal(a, b) for a, b in zip(yh, yh2))
    y = inv((yl, yh))
    assert torch.equal(y, inv((yl, yh)))
    yl1, yh1 = fwd(x[1:2, 1:2].contiguous())
    assert torch.equal(yl1, yl[1:2, 1:2]) and all(torch.equal(a, b[1:2, 1:2]) for a, b in zip(yh1, yh))
    assert torch.equal(inv((yl1, yh1)), y[1:2, 1:2])


def test_a_forward_is_one_launch_per_level(fa, monkeypatch):
    calls, thirds = [], []                                            # the entry points and whether each got a third filter
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append(name), thirds.append(third_filter(name, a)), real(name, *a))[2])
    fwd, inv = modules(fa, "a", "symmetric", 3)
    x = torch.randn(1, 1, 64, 64).cuda().requires_grad_(True)
    yl, yh = fwd(x)
    assert calls == ["dtcwt_fwd_j1", "dtcwt_fwd_j2", "dtcwt_fwd_j2"]
    del calls[:]
    torch.autograd.backward([yl] + yh, [torch.ones_like(t) for t in [yl] + yh])
    assert calls == ["dtcwt_inv_j2", "dtcwt_inv_j2", "dtcwt_inv_j1"]
    del calls[:]
    inv((yl.detach(), [h.detach() for h in yh]))
    assert calls == ["dtcwt_inv_j2", "dtcwt_inv_j2", "dtcwt_inv_j1"]
    assert len(thirds) == 9 and not any(thirds)                       # a two-filter bank: NULL every time


def test_refusals_come_before_any_launch(fa):
    """Each with a CPU tensor, which the device check -- the last one -- would refuse: the named check fires first."""
    ops, x = fa.ops, torch.zeros(1, 1, 8, 8)
    o3, o5, e10 = [0.25, 0.5, 0.25], [0.1] * 5, [0.1] * 10
    with pytest.raises(ValueError, match="odd"):
        ops.dtcwt_fwd_j1(x, [0.5] * 4, o3)
    with pytest.raises(ValueError, match="even"):
        ops.dtcwt_fwd_j2(x, *([[0.1] * 22] * 4))
    with pytest.raises(ValueError, match="same length"):
        ops.dtcwt_fwd_j2(x, e10, e10, [0.1] * 8, e10)
    with pytest.raises(ValueError, match="different dimensions"):
        ops.dtcwt_fwd_j1(x, o5, o3, False, 3, 3)
    with pytest.raises(ValueError, match="6 orientations"):
        ops.dtcwt_inv_j1(x, torch.zeros(1, 1, 5, 4, 4, 2), o5, o3)
    with pytest.raises(ValueError, match="float32"):
        ops.dtcwt_fwd_j1(x.double(), o5, o3)
    with pytest.raises(ValueError, match="device"):
        ops.dtcwt_fwd_j1(x, o5, o3)
    (fb, fq), _ = tuples("a")
    with pytest.raises(ValueError, match="even"):
        fa.DTCWTForward(biort=fb, qshift=[[0.1] * 32] * 4)
    assert set(FWD_BUFS) | set(INV_BUFS) == set(bufs("a"))
