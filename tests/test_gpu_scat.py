"""The DTCWT scattering layers (csrc/scat.hip) on the MI355X: ``ScatLayer`` / ``ScatLayerj2`` against the reference's own CPU
results (tests/golden/golden_scat_*.npz) and the float64 restatement of tests/test_scat_cpu.py (pinned to those fixtures there),
tile seams, the launch structure and structural properties.

The error bar is the project's, in relative L2 against the float64 restatement:   e_hip <= 2 e_ref + 2^-23
with e_ref the fp32 reference's own distance from it (the fixture's ``f32`` arrays; off the fixtures, the restatement run in fp32
on the CPU).  Every array prints e_ref, e_hip and their ratio as a ``SCAT_ERR`` line (run with ``-s``; a run's lines are what
profiles/scat_error.txt holds)."""
import pytest
import torch
import torch.nn.functional as F

from test_dtcwt_cpu import rel_l2
from test_rot_cpu import third_filter
from test_scat_cpu import BANKS, bufs, case_name, fixture_cases, fixture_inputs, gold, restate, restate_case, tuples

pytestmark = pytest.mark.gpu

K, FLOOR = 2.0, 2.0 ** -23
PHASE_ARG = {"scat_fwd_j1": 12, "scat_fwd_j2": 11}           # position of the phasor pointer in the entry points' arguments


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def layer(fa, bank, order, mode="symmetric", colour=False):
    fb, fq = tuples(bank)
    if order == 1:
        return fa.ScatLayer(biort=fb, mode=mode, combine_colour=colour).cuda()
    return fa.ScatLayerj2(biort=fb, qshift=fq, mode=mode, combine_colour=colour).cuda()


def run_hip(mod, x, cot):
    xd = (x if x.is_cuda else x.float().cuda()).detach().requires_grad_(True)
    Z = mod(xd)
    Z.backward(cot.cuda())
    torch.cuda.synchronize()
    return {"Z": Z.detach().cpu(), "xgrad": xd.grad.cpu()}


def hold_to_bar(name, ref64, ref32, got):
    """Print e_ref, e_hip and their ratio per array, then assert the bar of the module docstring on every one."""
    bad = []
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (name, k, tuple(got[k].shape), tuple(ref64[k].shape))
        e_ref, e_hip = rel_l2(ref32[k], ref64[k]), rel_l2(got[k], ref64[k])
        print("SCAT_ERR %-36s %-6s e_ref %.3e e_hip %.3e ratio %.3f" % (name, k, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))
        if not e_hip <= K * e_ref + FLOOR:
            bad.append((k, e_hip, e_ref))
    assert not bad, (name, bad)


@pytest.mark.parametrize("case", fixture_cases(), ids=case_name)
def test_fixture_parity(fa, case):
    """Z and x.grad of every fixture case."""
    cid, bank, order, mode, shape, colour = case
    g = gold(bank)
    ref64 = restate_case(case)
    ref32 = {k: torch.from_numpy(g[cid + "/f32/" + k]) for k in ref64}
    x, cot = fixture_inputs(case)
    hold_to_bar(case_name(case), ref64, ref32, run_hip(layer(fa, bank, order, mode, colour), x, cot))


@pytest.mark.parametrize("bank,order", [(b, o) for b in BANKS for o in (1, 2)])
def test_tile_seams(fa, bank, order):
    """``ScatLayer`` on 36 x 252: the level-1 kernels tile 16 x 64 (two tiles + 4 rows, four tiles - 4 columns).  ``ScatLayerj2`` on
    40 x 136: level 1 on 40 x 136 and, second order, on 20 x 68; the level-2 forward tiles 16 x 128 of its input, the level-2
    backward 32 x 64 of its result -- each of the six launches crosses a tile boundary in both axes and ends in a remainder tile.
    Banks a and c have m/2 odd (5, 9), bank b even (8); ``ScatLayer`` with bank b pads with zeros."""
    shape = (1, 2, 36, 252) if order == 1 else (1, 2, 40, 136)
    gen = torch.Generator().manual_seed(11 + order)
    x = torch.randn(*shape, generator=gen)
    b = bufs(bank)
    mode = "zero" if (order, bank) == (1, "b") else "symmetric"
    out = (shape[0], (7 if order == 1 else 49) * shape[1], shape[2] // (2 * order), shape[3] // (2 * order))
    cot = torch.rand(out, generator=gen) - 0.5
    ref64 = restate(x, b, order, mode, False, cot, torch.float64)
    ref32 = restate(x, b, order, mode, False, cot, torch.float32)
    hold_to_bar("seams %s j%d %s %s" % ("x".join(map(str, shape)), order, bank, mode), ref64, ref32, run_hip(layer(fa, bank, order, mode), x, cot))


def two_filter(calls):
    """The entry points of the recorded calls, in order, once every one of them has a NULL third filter."""
    assert not any(third_filter(n, a) for n, a in calls)
    return [n for n, _ in calls]


def spy(fa, monkeypatch):
    calls = []
    real = fa.ops.call
    monkeypatch.setattr(fa.ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("order,colour", [(1, False), (1, True), (2, False), (2, True)])
def test_no_grad_forward_saves_nothing_and_changes_no_bit(fa, monkeypatch, order, colour):
    mod = layer(fa, "a", order, "symmetric", colour)
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


@pytest.mark.parametrize("colour", [False, True])
def test_launch_counts(fa, monkeypatch, colour):
    x = torch.randn(1, 3, 64, 64).cuda().requires_grad_(True)
    one, two = layer(fa, "a", 1, "symmetric", colour), layer(fa, "a", 2, "symmetric", colour)
    calls = spy(fa, monkeypatch)
    Z = one(x)
    assert two_filter(calls) == ["scat_fwd_j1"]
    del calls[:]
    Z.backward(torch.ones_like(Z))
    assert two_filter(calls) == ["scat_bwd_j1"]
    del calls[:]
    Z = two(x)
    assert two_filter(calls) == ["scat_fwd_j1", "scat_fwd_j2", "scat_fwd_j1"]
    assert tuple(Z.shape) == (1, 51 if colour else 147, 16, 16) and Z.is_contiguous()
    del calls[:]
    Z.backward(torch.ones_like(Z))
    assert two_filter(calls) == ["scat_bwd_j1", "scat_bwd_j2", "scat_bwd_j1"]


@pytest.mark.parametrize("bank,mode", [("a", "symmetric"), ("b", "zero"), ("c", "symmetric")])
def test_consistency_with_the_dtcwt_kernels(fa, bank, mode):
    """The pooled lowpass and the magnitudes from ``ops.dtcwt_fwd_j1``'s outputs by torch ops: the filters' sums are the same, the
    pointwise operations may differ by a rounding -- 2^-22 in relative L2."""
    x = torch.randn(2, 2, 36, 72, generator=torch.Generator().manual_seed(7)).cuda()
    mod = layer(fa, bank, 1, mode)
    with torch.no_grad():
        Z = mod(x).view(2, 7, 2, 18, 36)
        ll, h = fa.ops.dtcwt_fwd_j1(x, mod.h0o, mod.h1o, False, 2, -1, mod.mode)
        b = torch.tensor(mod.magbias, dtype=torch.float32, device="cuda")
        mag = torch.sqrt(h[..., 0] ** 2 + h[..., 1] ** 2 + b * b) - b                      # (N, C, 6, h, w)
        e_low, e_mag = rel_l2(Z[:, 0].cpu(), F.avg_pool2d(ll, 2).cpu()), rel_l2(Z[:, 1:].cpu(), mag.transpose(1, 2).cpu())
    print("SCAT_CONSIST bank %s %s low %.3e mag %.3e" % (bank, mode, e_low, e_mag))
    assert e_low <= 2.0 ** -22 and e_mag <= 2.0 ** -22


@pytest.mark.parametrize("order", [1, 2])
def test_reproducible_and_batch_independent(fa, order):
    x = torch.randn(3, 2, 40, 72, generator=torch.Generator().manual_seed(9)).cuda()
    mod = layer(fa, "c", order)

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
    # the colour form: the batch slice only
    cmod = layer(fa, "c", order, "symmetric", True)
    xc = torch.randn(3, 3, 16, 24, generator=torch.Generator().manual_seed(10)).cuda()
    assert torch.equal(cmod(xc), cmod(xc)) and torch.equal(cmod(xc[1:2].contiguous()), cmod(xc)[1:2])


@pytest.mark.parametrize("order", [1, 2])
def test_a_strided_input_gives_its_contiguous_copys_bits(fa, order):
    big = torch.randn(2, 5, 16, 24, generator=torch.Generator().manual_seed(3)).cuda()
    mod = layer(fa, "a", order)
    view = big[:, 1:4]
    assert not view.is_contiguous()
    a, b = view.detach().requires_grad_(True), view.contiguous().requires_grad_(True)
    Za, Zb = mod(a), mod(b)
    assert torch.equal(Za, Zb)
    Za.backward(torch.ones_like(Za))
    Zb.backward(torch.ones_like(Zb))
    assert torch.equal(a.grad, b.grad)
    assert torch.equal(mod(big[:, ::2]), mod(big[:, ::2].contiguous()))
