"""The GEMM / table layer under everything spectral on the GPU: ``faoctasr_sgemm_batched`` at its tile edges, leading dimensions,
batch strides (zero, negative) and the six call shapes of spectral.hip and ops._lowpass2d; ``faoctasr_dft_tables`` and
``faoctasr_circulant_lowpass`` entry by entry; and their composition ``frequency_split`` / ``high_pass`` / ``low_pass`` with its
gradients -- against the float64 restatements of tests/test_sgemm_cpu.py (pinned there to torch, numpy and the oracle).  The case
tables, the input builders, the bars and their derivation live in that file; its test_every_form_is_reached ties the tables to
the constants of the sources.

The three kernels are called through the C ABI on buffers of this file's own making: operands are NaN outside their elements,
C is the sentinel (test_gpu_norm.SENTINEL) outside its elements, so a read or a store outside an operand shows.  The composition
goes through the public operators with every output allocated under ``sentinel_outputs``.

``SGEMM_ERR <case> <array> e_ref e_hip ratio ulp`` lines record the relative L2 error of the kernels (e_hip) and of the fp32
restatement on the CPU (e_ref: torch's fp32 matmul; a table's float64 value rounded once; the circulant form of the split in fp32)
against float64, and the kernels' worst error in fp32 ulps of the reference; ``SGEMM_SYM`` lines count the circulant entries
that differ from their transpose.  profiles/sgemm_error.txt keeps an MI355X run's.  Reported, not asserted."""
import pytest
import torch

import test_sgemm_cpu as S
from test_gpu_norm import SENTINEL, dev, leaf, sentinel_outputs
from test_norm_cpu import rel_l2, ulp32
from test_pointwise_cpu import worst_ulps

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def ids(op, table):
    return [S.ident(op, c) for c in table]


def filled(*shape):
    return torch.full(shape, SENTINEL, dtype=F32, device="cuda")


def report(case, name, got, ref, ref32):
    e_ref, e_hip = rel_l2(ref32, ref), rel_l2(got, ref)
    print("SGEMM_ERR %-52s %-5s e_ref %.3e e_hip %.3e ratio %.3f ulp %.2f"
          % (case, name, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf") if e_hip else 1.0, worst_ulps(got, ref)))


def stored(tag, name, g):
    assert bool(torch.isfinite(g).all()) and (g.numel() == 0 or float(g.abs().max()) < 1e29), "%s %s: an element was never stored" % (tag, name)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def at(t, offset):
    """Device address of element ``offset`` of a flat fp32 tensor."""
    return t.data_ptr() + 4 * offset


# ----------------------------------------------------------------------------------------
# sgemm_batched
# ----------------------------------------------------------------------------------------
def run_sgemm(fa, c, built):
    """Returns (C's whole buffer on the host, the device copies of A and B)."""
    A, B = dev(built["A"]), dev(built["B"])
    C = filled(S.layout(c, "C")[0])
    fa._lib.call("sgemm_batched", at(A, S.layout(c, "A")[1]), at(B, S.layout(c, "B")[1]), at(C, S.layout(c, "C")[1]), c.M, c.N, c.K,
                 c.lda, c.ldb, c.ldc, c.sA, c.sB, c.sC, c.batch, fa._lib.stream_ptr())
    torch.cuda.synchronize()
    return C.cpu(), A, B


@pytest.mark.parametrize("data", ["integer", "random"])
@pytest.mark.parametrize("c", S.SGEMM_CASES, ids=ids("sgemm", S.SGEMM_CASES))
def test_sgemm_batched(fa, c, data):
    tag = S.ident("sgemm", c) + ("_int" if data == "integer" else "")
    built = S.build_sgemm(c, data)
    ref, ref32 = S.gemm_ref(c, built), S.gemm_ref(c, built, F32)
    out, A, B = run_sgemm(fa, c, built)
    idx = S.index(c, "C")
    live = torch.zeros(out.numel(), dtype=torch.bool)
    live[idx.reshape(-1)] = True
    got = out[idx]
    stored(tag, "C", got)
    # padding columns, gaps between batch entries, the guard elements on either side
    assert int((~live).sum()) >= 2 * S.GUARD and bool((out[~live] == SENTINEL).all()), "%s: C was written outside its elements" % tag
    assert torch.equal(bits(A), bits(built["A"])) and torch.equal(bits(B), bits(built["B"])), "%s: an operand was written" % tag
    report(tag, "C", got, ref["C"], ref32["C"])
    if data == "integer":
        n = S.exact_violations(got, ref["C"])
        assert n == 0, "%s: %d of %d elements differ from the exact integer result" % (tag, n, got.numel())
    else:
        n, worst = S.gemm_violations(got, ref, c.K)
        assert n == 0, "%s: %d elements outside gamma_K |A| |B| + 1 ulp, worst at %.3g of the bar" % (tag, n, worst)
    if c.K == 0:
        assert float(got.abs().max()) == 0.0


@pytest.mark.parametrize("c", S.SGEMM_EMPTY, ids=ids("sgemm", S.SGEMM_EMPTY))
def test_sgemm_batched_with_nothing_to_do_leaves_c_alone(fa, c):
    out, _, _ = run_sgemm(fa, c, S.build_sgemm(c))
    assert out.numel() >= 2 * S.GUARD and bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------
# the tables
# ----------------------------------------------------------------------------------------
def run_table(fa, name, numel, *args):
    buf = filled(numel + 2 * S.GUARD)
    fa._lib.call(name, at(buf, S.GUARD), *args, fa._lib.stream_ptr())
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:S.GUARD] == SENTINEL).all()) and bool((out[S.GUARD + numel:] == SENTINEL).all()), "%s wrote outside its table" % name
    return out[S.GUARD:S.GUARD + numel]


@pytest.mark.parametrize("n", S.DFT_N, ids=ids("dft", S.DFT_N))
def test_dft_tables(fa, n):
    tag = S.ident("dft", n)
    ref = S.dft_ref(n)
    got = run_table(fa, "dft_tables", 4 * n * n, n)
    stored(tag, "table", got)
    report(tag, "table", got, ref["flat"], ref["flat"].float())
    bad, worst = S.table_violations(got, ref["flat"])
    assert bad == 0, "%s: %d entries further than 1 ulp from float64, worst %.3g ulp" % (tag, bad, worst)
    ex = ref["exact"]
    assert bool((got[ex].double() == ref["flat"][ex]).all()), "%s: an entry whose value is 0 or +-1 is not stored exactly" % tag
    # both layouts hold the same bits; C_n and S_n are symmetric to the bit; row 0 and column 0 are 1 and 0
    cs, st = got[:2 * n * n].view(n, 2 * n), got[2 * n * n:].view(2 * n, n)
    C, Sn = cs[:, :n], cs[:, n:]
    assert torch.equal(bits(C), bits(st[:n])) and torch.equal(bits(Sn), bits(st[n:])), "%s: [C | S] and [C ; S] differ" % tag
    assert torch.equal(bits(C), bits(C.T)) and torch.equal(bits(Sn), bits(Sn.T)), "%s: a table is not symmetric to the bit" % tag
    assert bool((C[0] == 1).all()) and bool((C[:, 0] == 1).all()) and bool((Sn[0] == 0).all()) and bool((Sn[:, 0] == 0).all())
    # the operators' cached table is this one
    assert torch.equal(bits(fa.ops.dft_tables(n, torch.device("cuda"))), bits(got))


@pytest.mark.parametrize("case", S.CIRC_CASES, ids=ids("circ", S.CIRC_CASES))
def test_circulant_lowpass(fa, case):
    n, r = case
    r = S.radius(n, r)
    tag = S.ident("circ", case)
    ref = S.circulant_ref(n, r)
    got = run_table(fa, "circulant_lowpass", n * n, n, r).view(n, n)
    stored(tag, "C", got)
    report(tag, "C", got, ref, ref.float())
    extra = S.circulant_extra(n, r)
    bad, worst = S.table_violations(got, ref, extra)
    assert bad == 0, "%s: %d entries outside 1 ulp + the double sum's bound, worst at %.3g of the bar" % (tag, bad, worst)
    # circulant to the bit: every entry is computed from (a - b) mod n alone
    assert torch.equal(bits(got), bits(torch.roll(got, (1, 1), (0, 1)))), "%s: not a circulant to the bit" % tag
    # symmetric to the bit, so within the ulp that _FreqSplit.backward needs to use C as its own adjoint: the kernel sums entry
    # j and entry n - j at the same phases.  (Summed at their own phases they agreed to the bit up to n = 64, but at n = 257 with
    # radius 5 / 10, where the far taps cancel to ~1e-17 instead of ~1e-100, 30840 / 46774 of the 66049 entries differed from their
    # transpose, by up to 8e8 / 6e26 ulp of the entry: nothing in absolute terms, far outside an ulp.)
    diff = (got.double() - got.double().T).abs()
    print("SGEMM_SYM %-52s %d of %d entries differ from their transpose, worst %.2f ulp" % (tag, int((diff > 0).sum()), n * n,
                                                                                         float((diff / ulp32(ref)).max())))
    assert bool((diff <= ulp32(ref)).all()), "%s: C and its transpose differ by more than 1 ulp" % tag
    assert torch.equal(bits(got), bits(got.T)), "%s: C is not symmetric to the bit" % tag
    # every row sums to the DC tap t[0] = 1, within the sum of its entries' bars
    rows = got.double().sum(1)
    bar = (ulp32(ref) + extra).sum(1)
    assert S.circulant_taps(n, r)[0] == 1.0 and bool(((rows - 1.0).abs() <= bar).all()), (tag, float((rows - 1).abs().max()), float(bar.max()))
    assert torch.equal(bits(fa.ops.circulant_lowpass(n, r, torch.device("cuda"))), bits(got))


# ----------------------------------------------------------------------------------------
# the composition
# ----------------------------------------------------------------------------------------
class _Ctx:
    """What _FreqSplit reads of an autograd context, to reach backward with an upstream gradient that is None (autograd itself
    hands the function zeros for an unused output)."""
    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def check_fs(tag, got, ref, ref32, names=("hf", "lf", "dx")):
    torch.cuda.synchronize()
    for name in names:
        g = got[name].detach().cpu()
        stored(tag, name, g)
        report(tag, name, g, ref[name], ref32[name])
    S.assert_fs_bars(tag, got, ref, names)


@pytest.mark.parametrize("case", S.FS_CASES, ids=ids("fs", S.FS_CASES))
def test_frequency_split(fa, case):
    shape, radii, grads = case
    tag = S.ident("fs", case)
    c, ref, ref32 = S.freq_split_case(case)
    g_hf, g_lf = S.upstream(c, grads)
    xd = leaf(c["x"])
    with sentinel_outputs():
        hf, lf = fa.frequency_split(xd, *radii)
        torch.autograd.backward([t for t, g in ((hf, g_hf), (lf, g_lf)) if g is not None], [dev(g) for g in (g_hf, g_lf) if g is not None])
        again = fa.frequency_split(xd.detach(), *radii)
        torch.cuda.synchronize()
    check_fs(tag, {"hf": hf, "lf": lf, "dx": xd.grad}, ref, ref32)
    assert torch.equal(bits(again[0]), bits(hf)) and torch.equal(bits(again[1]), bits(lf)), "%s: two calls differ in bits" % tag
    assert torch.equal(xd.detach().cpu(), c["x"])
    if grads == "both gradients":
        return
    # the same through _FreqSplit itself with the absent gradient None: freq_mix_bwd's NULL forms inside the whole operator
    ctx = _Ctx()
    with sentinel_outputs(), torch.no_grad():
        hf2, lf2 = fa.ops._FreqSplit.forward(ctx, dev(c["x"]), float(radii[0]), float(radii[1]))
        dx2 = fa.ops._FreqSplit.backward(ctx, dev(g_hf), dev(g_lf))[0]
        torch.cuda.synchronize()
    assert torch.equal(bits(hf2), bits(hf)) and torch.equal(bits(lf2), bits(lf))
    check_fs(tag + "_none", {"dx": dx2}, ref, ref32, ("dx",))
    assert torch.equal(dx2, xd.grad), "%s: a None upstream gradient and a zero one give different dx" % tag


def test_high_pass_and_low_pass_are_the_planes_of_frequency_split(fa):
    r = S.PASS_RADIUS
    x = torch.randn(S.PASS_SHAPE, generator=torch.Generator().manual_seed(11)) * 0.5 + 0.1
    ref = S.freq_split_ref(x[None], r, r)
    bars = S.forward_bars(x[None], r, r, ref)
    with sentinel_outputs():
        hp, lp = fa.high_pass(dev(x), r), fa.low_pass(dev(x), r)
        hf, lf = fa.frequency_split(dev(x)[None], r, r)
        torch.cuda.synchronize()
    assert hp.shape == S.PASS_SHAPE[1:] and lp.shape == S.PASS_SHAPE[1:]
    assert torch.equal(bits(lp), bits(lf[0, 0])), "low_pass is not frequency_split's lf plane"
    # high_pass = 2 hf - x (ops.axpby): 2 hf is exact, so the float64 difference rounded once
    want = (2 * hf[0, 0].cpu().double() - x[0].double()).float()
    assert torch.equal(hp.cpu(), want), "high_pass is not 2 hf - x of frequency_split's hf plane, rounded once"
    tol = 2 * bars["hf"][0, 0] + ulp32(ref["hp_abs"][0, 0])
    assert bool(((hp.cpu().double() - ref["hp_abs"][0, 0]).abs() <= tol).all())
    assert bool(((lp.cpu().double() - ref["lf"][0, 0]).abs() <= bars["lf"][0, 0]).all())
