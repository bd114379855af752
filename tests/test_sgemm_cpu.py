"""The GEMM / table layer under everything spectral, without a GPU: ``faoctasr_sgemm_batched`` and ``faoctasr_circulant_lowpass``
(csrc/sgemm.hip), ``faoctasr_dft_tables`` (csrc/spectral.hip) and their composition ``ops.freq_split``.  This file holds the case
tables, the input builders, the float64 restatements (each pinned here), the bars and the host-side refusals;
tests/test_gpu_sgemm.py runs the tables through the kernels and takes everything from here.

Restatements
  gemm_ref          C_b = A_b B_b gathered from the case's strided buffers by index arithmetic (lda, ldb, ldc, the three batch strides,
                    stride 0, a negative stride); pinned to torch.matmul of the dense operands the builder scattered.
  dft_ref           cos / sin of 2 pi ((k l) mod n) / n in both layouts, exact at the quarter points; pinned to numpy.fft.fft(eye(n)).
  circulant_ref     oracle.circulant_lowpass_matrix with the radius as the fp32 value that crosses the ABI; pinned to the FFT form
                    ifft(ifftshift(fftshift(fft x) g)) at odd and even n.
  freq_split_ref    the oracle's FFT form for (B, C, H, W) with autograd gradients, the mask kept in float64 (the kernels never
                    round it); pinned to oracle.freq_split at C = 1 (which rounds its mask to fp32: ``mask32``) and to the
                    circulant form C_H x C_W (``freq_split_circulant``), whose fp32 evaluation is the e_ref of the SGEMM_ERR lines.

Inputs: every operand buffer of a GEMM case is NaN outside the operands themselves (padding columns, gaps between batch entries,
``GUARD`` elements on either side), so a read outside an operand poisons the result even where it meets a zero.

The bars (none is measured on the kernels), u = 2^-24, gamma_K = K u / (1 - K u):
  exact     integer operands in [-8, 8]: with K <= 1024 every product (<= 64) and every partial sum (<= 65536) is an fp32 integer, so
            the kernel's result equals the float64 one to the bit.  Any indexing error shows here.
  GEMM      the f32 MFMA is a k-ordered fmaf chain from 0: an element passes K roundings, so
                |got - ref64| <= gamma_K (|A| |B|) + 1 ulp32(ref)
            (Higham's bound for a K-term inner product, any order; the ulp is slack).  K = 0: exactly 0.
  tables    an entry is a float64 value (device cospi / sinpi / exp, a few 2^-53) rounded once: |got - ref64| <= 1 ulp32(ref), and
            the entries whose exact value is 0 or +-1 (k l = 0 mod n / 4) are stored exactly.  The circulant's entry is a sum of n
            terms t_k cos(.) in double, divided by n: n 2^-53 sum |t_k| is added for the sum, the exp and the cospi of every term.
  low-pass  Y = C_H (x C_W), T = x C_W kept in fp32: |T^ - T| <= gamma_W |x| |C_W|, |Y^ - C_H T^| <= gamma_H |C_H| |T^|, and each
            table entry is within 1 ulp32 (2 u relative) of its exact value:
                |Y^ - Y| <= (gamma_H + gamma_W + gamma_H gamma_W + 4 u) (|C_H| |x| |C_W|) + 1 ulp32(Y)                    =: bar_low
  hf, lf    lf = -|low_lp| is exact in its operand and |.| is 1-Lipschitz: bar_lf = bar_low(r_lp).  hf = (|x - low_hp| + x) / 2 has
            test_pointwise_cpu.FREQ_BARS' two roundings on top of half of its operand's error:
                bar_hf = bar_low(r_hp) / 2 + 2 u (|x - low_hp| + |x|) / 2 + 1 ulp32(hf)
  dx        dx = dx_direct - C_H s_hp C_W + C_H s_lp C_W.  freq_mix_bwd's three outputs are exact (FREQ_BARS) once the signs agree:
            the upstream gradients are zero wherever |x - low_hp| (g_hf) or |low_lp| (g_lf) of the float64 reference is below
            its forward bar (the KINK rule of test_norm_cpu.py; at most 1 % of the positions of any case, asserted here).  Then
                bar_dx = bar_low(s_hp; r_hp) + bar_low(s_lp; r_lp) + 2 u (|dx_direct| + |C_H s_hp C_W| + |C_H s_lp C_W|) + 1 ulp32(dx)
            (the two in-place axpby calls have coefficients +-1: one rounding each).  The backward applies C where the adjoint is
            C^T; both are within 1 ulp32 of the same symmetric matrix, which the 4 u already covers.
``SGEMM_ERR`` lines (tests/test_gpu_sgemm.py) record e_ref / e_hip / worst ulp; reported, not asserted."""
import collections
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_norm_cpu import CSRC, PIN, rel_l2, ulp32
from test_pointwise_cpu import FREQ_BARS, U, f32, sgn

F64 = torch.float64
TILE, KC, NT, WAVE_N = 64, 16, 64, 32          # block tile (rows and columns), K chunk, B_s row length, columns per wave
BATCH_CAP, N_CAP, MFMA_K = 65535, 8192, 2
GUARD = 4
KINK_CAP = 0.01


def read_constants():
    """The constants the forms below depend on, read out of the two sources."""
    s = open(os.path.join(CSRC, "sgemm.hip")).read()
    p = open(os.path.join(CSRC, "spectral.hip")).read()
    m = re.search(r"constexpr int KC = (\d+), LDA = KC \+ 1, NT = (\d+);", s)
    t = re.search(r"const int m0 = blockIdx\.y \* (\d+), n0 = blockIdx\.x \* (\d+);", s)
    g = re.search(r"dim3 grid\(\(N \+ (\d+)\) / (\d+), \(M \+ (\d+)\) / (\d+), batch\);", s)
    w = re.findall(r"w[mn] \* (\d+) \+ l31", s)
    out = {"KC": int(m.group(1)), "NT": int(m.group(2)), "tile": sorted({int(v) for v in t.groups()} | {int(g.group(2)), int(g.group(4))}),
           "round": sorted({int(g.group(1)) + 1, int(g.group(3)) + 1}), "wave": sorted({int(v) for v in w}),
           "mfma_k": int(re.search(r"for \(int kk0 = 0; kk0 < KC; kk0 \+= (\d+)\)", s).group(1)),
           "batch_cap": int(re.search(r"if \(batch > (\d+)\)", s).group(1)),
           "m_cap": [int(v) for v in re.search(r"if \(M > (\d+) \* (\d+)\)", s).groups()],
           "circ_n_cap": int(re.search(r"if \(n < 1 \|\| n > (\d+) \|\| !\(radius > 0\.f\)\)", s).group(1)),
           "dft_n_cap": int(re.search(r'if \(n < 1 \|\| n > (\d+)\) return fail\(FAOCTASR_EINVAL, "dft_tables', p).group(1)),
           "table_block": sorted({int(v) for v in re.findall(r"const long e = \(long\)blockIdx\.x \* (\d+) \+ threadIdx\.x;", s)}
                                 | {int(re.search(r"void dft_tables_kernel\(.*?blockIdx\.x \* (\d+) \+ threadIdx\.x", p, re.S).group(1))})}
    return out


# ----------------------------------------------------------------------------------------
# the case tables: the smallest that reach each form; a case's seed is its position in its table
# ----------------------------------------------------------------------------------------
Gemm = collections.namedtuple("Gemm", "name M N K lda ldb ldc sA sB sC batch offB")


def gemm(name, M, N, K, lda=None, ldb=None, ldc=None, sA=None, sB=None, sC=None, batch=1, offB=0):
    lda, ldb, ldc = K if lda is None else lda, N if ldb is None else ldb, N if ldc is None else ldc
    dflt = (lambda rows, ld: rows * ld if batch > 1 else 0)
    return Gemm(name, M, N, K, lda, ldb, ldc, dflt(M, lda) if sA is None else sA, dflt(K, ldb) if sB is None else sB,
                dflt(M, ldc) if sC is None else sC, batch, offB)


def caller_cases(H, W, imgs=2, B=3):
    """The call shapes of spectral.hip (x and y as the two batch entries, ``gap`` floats between the allocations) and of
    ops._lowpass2d, named by their caller."""
    Wh, rows, gap, tag = W // 2 + 1, imgs * H, 11, "_%dx%d" % (H, W)
    return [
        gemm("phase_loss_fwd_row_pass" + tag, rows, 2 * W, W, W, 2 * W, 2 * W, rows * W + gap, 0, rows * 2 * W, 2),
        gemm("sprof_fwd_half_row_pass" + tag, rows, 2 * Wh, W, W, 2 * Wh, 2 * Wh, rows * W + gap, 0, rows * 2 * Wh, 2),
        gemm("phase_loss_bwd_stacked_table" + tag, rows, W, 2 * W, 2 * W, W, W, rows * 2 * W, 0, rows * W + gap, 2, offB=2 * W * W),
        gemm("sprof_bwd_half_stacked_table" + tag, rows, W, 2 * Wh, 2 * Wh, W, W, rows * 2 * Wh, 0, rows * W + gap, 2, offB=2 * W * Wh),
        gemm("lowpass2d_row_pass_shared_B" + tag, B * H, W, W),
        gemm("lowpass2d_column_pass_shared_A" + tag, H, W, H, H, W, W, 0, H * W, H * W, B),
    ]


_EDGE = (33, 40, 21)                                              # M tail, N tail, odd K tail: the base of the stride cases
SGEMM_CASES = (
    [gemm("one_tile", 64, 64, 16)]
    + [gemm("M%d" % m, m, 64, 16) for m in (1, 63, 65)]
    + [gemm("N%d" % n, 64, n, 16) for n in (1, 31, 33, 65)]
    + [gemm("K%d" % k, 64, 64, k) for k in (0, 1, 15, 17, 33)]
    + [gemm("lda", *_EDGE, lda=29), gemm("ldb", *_EDGE, ldb=47), gemm("ldc", *_EDGE, ldc=45), gemm("ld_all", *_EDGE, lda=29, ldb=47, ldc=45)]
    + [gemm("batch3_strideA0", *_EDGE, sA=0, sB=21 * 40 + 5, sC=33 * 40 + 7, batch=3),
       gemm("batch3_strideB0", *_EDGE, sA=33 * 21 + 3, sB=0, sC=33 * 40 + 7, batch=3),
       gemm("batch3_all_strides", *_EDGE, sA=33 * 21 + 3, sB=21 * 40 + 5, sC=33 * 40 + 7, batch=3),
       gemm("batch2_negative_strideA", *_EDGE, sA=-(33 * 21 + 3), sB=0, sC=33 * 40, batch=2)]
    + caller_cases(37, 53) + caller_cases(8, 8))
#: C must stay untouched: nothing is launched
SGEMM_EMPTY = [gemm("M0", 0, 40, 21), gemm("N0", 33, 0, 21), gemm("batch0", *_EDGE, batch=0)]
DFT_N = [1, 2, 3, 4, 16, 37, 53, 64, 255, 256, 257, 1024]
CIRC_N = [1, 2, 3, 15, 16, 17, 37, 53, 64, 257]
CIRC_R = [0.3, 5, 10, "2n"]
CIRC_CASES = [(n, r) for n in CIRC_N for r in CIRC_R]
FS_SHAPES = [(2, 3, 37, 53), (1, 2, 8, 72), (3, 1, 65, 15), (1, 1, 64, 64)]
FS_RADII = [(10, 8), (4, 14)]
FS_GRADS = ["both gradients", "g_hf only", "g_lf only"]
FS_CASES = [(s, r, g) for s in FS_SHAPES for r in FS_RADII for g in FS_GRADS]
PASS_SHAPE, PASS_RADIUS = (1, 37, 53), 4                          # high_pass / low_pass against frequency_split's planes
TABLES = {"sgemm": SGEMM_CASES, "dft": DFT_N, "circ": CIRC_CASES, "fs": FS_CASES}


def radius(n, r):
    return 2.0 * n if r == "2n" else float(r)


def ident(op, case):
    if op == "sgemm":
        return "sgemm_" + case.name
    if op == "dft":
        return "dft_%d" % case
    if op == "circ":
        return "circ_%d_r%s" % case
    shape, radii, grads = case
    return "fs_%s_r%dx%d_%s" % ("x".join(map(str, shape)), radii[0], radii[1], grads.replace(" ", "_"))


def table_forms(op, n, k):
    out = {op + (": n = 1" if n == 1 else ": odd n" if n % 2 else ": even n")}
    blk = k["table_block"][0]
    if n * n > blk:
        out.add(op + ": several blocks")
    if n * n % blk:
        out.add(op + ": last block cut short")
    return out


def forms(op, case, k=None):
    """The forms of the code that ``case`` (a row of ``op``'s table) reaches, by the constants ``k`` of the source."""
    k = k or read_constants()
    tile, kc = k["tile"][0], k["KC"]
    if op == "sgemm":
        c, out = case, set()
        if c.M % tile == 0 and c.N % tile == 0 and c.K % kc == 0 and c.K > 0:
            out.add("sgemm: full tiles only")
        if c.M % tile:
            out.add("sgemm: M tail")
        if c.M == 1:
            out.add("sgemm: M = 1")
        if c.M > tile:
            out.add("sgemm: several row tiles")
        if c.N % tile:
            out.add("sgemm: N tail")
        if 0 < c.N % tile <= k["wave"][0]:
            out.add("sgemm: upper column wave idle")
        if c.N % tile > k["wave"][0]:
            out.add("sgemm: upper column wave cut short")
        if c.N > tile:
            out.add("sgemm: several column tiles")
        if c.K == 0:
            out.add("sgemm: K = 0")
        if c.K % kc:
            out.add("sgemm: K tail")
        if c.K % k["mfma_k"]:
            out.add("sgemm: K tail, odd")
        if 0 < c.K < kc:
            out.add("sgemm: K below one chunk")
        if c.K > kc:
            out.add("sgemm: several K chunks")
        for name, ld, row in (("lda", c.lda, c.K), ("ldb", c.ldb, c.N), ("ldc", c.ldc, c.N)):
            if ld > row:
                out.add("sgemm: %s > row" % name)
        if c.lda > c.K and c.ldb > c.N and c.ldc > c.N:
            out.add("sgemm: every ld > row")
        if c.batch > 1:
            out.add("sgemm: strideA = 0" if c.sA == 0 else "sgemm: negative strideA" if c.sA < 0 else "sgemm: strideA > 0")
            out.add("sgemm: strideB = 0" if c.sB == 0 else "sgemm: strideB > 0")
            if c.sA and c.sB and c.sC:
                out.add("sgemm: all three strides non-zero")
            if c.sA > c.M * c.lda or c.sC > c.M * c.ldc:
                out.add("sgemm: gap between batch entries")
        if c.offB:
            out.add("sgemm: B at an offset")
        m = re.match(r"(\w+?)_(\d+)x(\d+)$", c.name)
        if m:
            out.add("caller: " + m.group(1))
        return out
    if op == "dft":
        out = table_forms("dft", case, k)
        if case % 4 == 0:
            out.add("dft: quarter points exact")
        if (case - 1) ** 2 >= 1 << 19:
            out.add("dft: k l needs 20 bits")
        return out
    if op == "circ":
        n, r = case
        out = table_forms("circ", n, k)
        r = radius(n, r)
        out.add("circ: taps nearly a delta" if r < 1 else "circ: taps nearly flat" if r >= 2 * n else "circ: working radius")
        return out
    (B, C, H, W), radii, grads = case
    out = {"fs: " + grads, "fs: square" if H == W else "fs: non-square"}
    if C > 1:
        out.add("fs: C > 1")
    if B > 1:
        out.add("fs: B > 1")
    for name, v in (("H", H), ("W", W)):
        if v < kc:
            out.add("fs: %s below one K chunk" % name)
        if v > tile:
            out.add("fs: %s above one tile" % name)
        if v % 2:
            out.add("fs: odd " + name)
    return out


CALLERS = ("phase_loss_fwd_row_pass", "sprof_fwd_half_row_pass", "phase_loss_bwd_stacked_table", "sprof_bwd_half_stacked_table",
           "lowpass2d_row_pass_shared_B", "lowpass2d_column_pass_shared_A")
FORMS = ({"sgemm: " + f for f in (
    "full tiles only", "M tail", "M = 1", "several row tiles", "N tail", "upper column wave idle", "upper column wave cut short",
    "several column tiles", "K = 0", "K tail", "K tail, odd", "K below one chunk", "several K chunks", "lda > row", "ldb > row",
    "ldc > row", "every ld > row", "strideA = 0", "strideA > 0", "negative strideA", "strideB = 0", "strideB > 0",
    "all three strides non-zero", "gap between batch entries", "B at an offset")}
    | {"caller: " + c for c in CALLERS}
    | {"dft: " + f for f in ("n = 1", "odd n", "even n", "several blocks", "last block cut short", "quarter points exact", "k l needs 20 bits")}
    | {"circ: " + f for f in ("n = 1", "odd n", "even n", "several blocks", "last block cut short", "taps nearly a delta", "taps nearly flat",
                              "working radius")}
    | {"fs: " + f for f in ("both gradients", "g_hf only", "g_lf only", "square", "non-square", "C > 1", "B > 1", "H below one K chunk",
                            "W below one K chunk", "H above one tile", "W above one tile", "odd H", "odd W")})


def covered_forms(tables=None, k=None):
    k = k or read_constants()
    got = set()
    for op, table in (tables or TABLES).items():
        for case in table:
            got |= forms(op, case, k)
    return got


# ----------------------------------------------------------------------------------------
# sgemm_batched: buffers, builder, restatement
# ----------------------------------------------------------------------------------------
def _span(rows, ld, cols):
    return (rows - 1) * ld + cols if rows > 0 and cols > 0 else 0


def _operand(c, which):
    """(rows, ld, cols, stride, elements in front of the pointer besides the guard) of operand ``which``."""
    if which == "A":
        return c.M, c.lda, c.K, c.sA, 0
    if which == "B":
        return c.K, c.ldb, c.N, c.sB, c.offB
    return c.M, c.ldc, c.N, c.sC, 0


def layout(c, which):
    """(buffer length, offset of the pointer the call receives): GUARD elements, what lies in front of the pointer (a negative
    stride's later entries, B's offset), the batch entries, GUARD elements."""
    rows, ld, cols, stride, off = _operand(c, which)
    offs = [b * stride for b in range(max(c.batch, 1))]
    front = off - min(offs)
    return GUARD + front + max(offs) + _span(rows, ld, cols) + GUARD, GUARD + front


def index(c, which):
    """Buffer positions of the operand's elements, (batch, rows, cols)."""
    rows, ld, cols, stride, _ = _operand(c, which)
    b, r, j = torch.arange(c.batch).view(-1, 1, 1), torch.arange(rows).view(1, -1, 1), torch.arange(cols).view(1, 1, -1)
    return layout(c, which)[1] + b * stride + r * ld + j


def build_sgemm(c, data="random"):
    """Dense operands (a shared operand once) scattered into NaN buffers: {"A", "B": flat buffers, "dense_A", "dense_B"}."""
    where = [x.name for x in SGEMM_CASES + SGEMM_EMPTY]
    g = torch.Generator().manual_seed(7000 + 10 * where.index(c.name) + (data == "integer"))
    out = {}
    for which in ("A", "B"):
        rows, ld, cols, stride, _ = _operand(c, which)
        n = 1 if stride == 0 else max(c.batch, 1)
        if data == "integer":
            dense = torch.randint(-8, 9, (n, rows, cols), generator=g).float()
        else:
            dense = torch.randn(n, rows, cols, generator=g)
        buf = torch.full((layout(c, which)[0],), float("nan"))
        idx = index(c, which)
        if idx.numel():
            buf[idx.reshape(-1)] = dense.expand(c.batch, rows, cols).reshape(-1)
        out[which], out["dense_" + which] = buf, dense
    return out


def gemm_ref(c, built, dtype=F64):
    """C_b = A_b B_b from the strided buffers: {"C": (batch, M, N), "abs_C": |A| |B|}."""
    A, B = built["A"][index(c, "A")].to(dtype), built["B"][index(c, "B")].to(dtype)
    return {"C": torch.matmul(A, B), "abs_C": torch.matmul(A.abs(), B.abs())}


def gamma(K):
    return K * U / (1 - K * U)


def _viol(err, tol):
    bad = ~(err <= tol)                                                  # a NaN is a violation
    return int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0


def _flat(got, ref):
    return got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)


def gemm_violations(got, ref, K):
    """|got - ref| <= gamma_K |A| |B| + 1 ulp32(ref).  Returns (count, worst error as a fraction of the bar)."""
    g, r = _flat(got, ref["C"])
    return _viol((g - r).abs(), gamma(K) * ref["abs_C"].double().reshape(-1) + ulp32(r))


def exact_violations(got, ref):
    g, r = _flat(got, ref)
    return int((~(g == r)).sum())


# ----------------------------------------------------------------------------------------
# the tables
# ----------------------------------------------------------------------------------------
def dft_ref(n):
    """{"cs": [C_n | S_n] (n, 2n), "stacked": [C_n ; S_n] (2n, n), "flat": both as the kernel lays them out, "exact": the entries
    of "flat" whose exact value is 0 or +-1}."""
    k = np.arange(n, dtype=np.int64)
    ph = (k[:, None] * k[None, :]) % n
    # the angle reduced in integers to [0, pi / 4], where its float64 rounding is below 2^-53: quadrant q, remainder r4 / n of a
    # quarter turn, mirrored about pi / 4.  The quarter points come out as exact 0 and +-1.
    q, r4 = (4 * ph) // n, (4 * ph) % n
    quarter, mirrored = r4 == 0, 2 * r4 > n
    phi = (np.pi / 2) * np.where(mirrored, n - r4, r4).astype(np.float64) / n
    ct, st_ = np.where(mirrored, np.sin(phi), np.cos(phi)), np.where(mirrored, np.cos(phi), np.sin(phi))
    c = np.choose(q, [ct, -st_, -ct, st_]) + 0.0                           # + 0.0: no negative zeros
    s = np.choose(q, [st_, ct, -st_, -ct]) + 0.0
    cs, st = np.concatenate([c, s], 1), np.concatenate([c, s], 0)
    ex_cs, ex_st = np.concatenate([quarter, quarter], 1), np.concatenate([quarter, quarter], 0)
    return {"cs": torch.from_numpy(cs), "stacked": torch.from_numpy(st), "flat": torch.from_numpy(np.concatenate([cs.ravel(), st.ravel()])),
            "exact": torch.from_numpy(np.concatenate([ex_cs.ravel(), ex_st.ravel()]))}


def table_violations(got, ref, extra=0.0):
    """|got - ref| <= 1 ulp32(ref) + extra.  Returns (count, worst as a fraction of the bar)."""
    g, r = _flat(got, ref)
    return _viol((g - r).abs(), ulp32(r) + extra)


def circulant_taps(n, r):
    """t[k] = g[(k + n // 2) mod n] of the centred Gaussian g: the taps as they meet spectrum bin k (ifftshift)."""
    k = np.arange(n)
    return np.fft.ifftshift(np.exp(-0.5 * (k - int(n / 2)) ** 2 / f32(r) ** 2))


def circulant_ref(n, r):
    from oracle import octa_oracle as O
    return O.circulant_lowpass_matrix(n, f32(r))


def circulant_extra(n, r):
    return n * 2.0 ** -53 * float(np.abs(circulant_taps(n, r)).sum())


def circulant_kernel_formula(n, r, shift=None):
    """circulant_lowpass_kernel's own sum in float64 numpy, term by term: t[k] = exp(-d^2 / (2 r^2)) with d = (k + shift) mod n - n/2,
    shift = n/2 (the kernel's; n - n/2 is the other direction), phase (k min(j, n - j)) mod n."""
    c0 = n // 2
    shift = c0 if shift is None else shift
    k = np.arange(n, dtype=np.int64)
    d = ((k + shift) % n - c0).astype(np.float64)
    t = np.exp(-d * d * (0.5 / (float(f32(r)) * float(f32(r)))))
    ph = (k[None, :] * np.minimum(k, n - k)[:, None]) % n                  # [j][k], entry j summed at min(j, n - j)
    col = (t[None, :] * np.cos(2 * np.pi * ph / n)).sum(1) / n
    return torch.from_numpy(col[(k[:, None] - k[None, :]) % n])


# ----------------------------------------------------------------------------------------
# freq_split
# ----------------------------------------------------------------------------------------
def gauss2d(H, W, r, dtype, high=False, mask32=False):
    i = torch.arange(H, dtype=F64)[:, None] - int(H / 2)
    j = torch.arange(W, dtype=F64)[None, :] - int(W / 2)
    g = torch.exp(-0.5 * (i * i + j * j) / (r ** 2))
    g = 1 - g if high else g
    return (g.float() if mask32 else g).to(dtype)


def freq_split_ref(x, r_hp, r_lp, g_hf=None, g_lf=None, dtype=F64, mask32=False):
    """The oracle's FFT form on (B, C, H, W): hf = (|ifft2(ifftshift(fftshift(fft2 x) (1 - g_hp)))| + x) / 2,
    lf = -|ifft2(ifftshift(fftshift(fft2 x) g_lp))|, and dx for the upstream gradients given (None: that output is unused)."""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    H, W = x.shape[-2:]
    dims = (-2, -1)
    F = torch.fft.fftshift(torch.fft.fft2(x), dim=dims)
    back = lambda f: torch.fft.ifft2(torch.fft.ifftshift(f, dim=dims))
    mask = lambda r, high=False: gauss2d(H, W, r, dtype, high, mask32)
    hp_abs, low_lp = back(F * mask(r_hp, True)).abs(), back(F * mask(r_lp))
    hf, lf = (hp_abs + x) / 2, -low_lp.abs()
    out = {"hf": hf.detach(), "lf": lf.detach(), "hp_abs": hp_abs.detach(), "low_hp": back(F * mask(r_hp)).real.detach(), "low_lp": low_lp.real.detach()}
    outs = [t for t, g in ((hf, g_hf), (lf, g_lf)) if g is not None]
    if outs:
        (out["dx"],) = torch.autograd.grad(outs, [x], [g.to(dtype) for g in (g_hf, g_lf) if g is not None])
    return out


def lowpass_circulant(v, ch, cw):
    return torch.matmul(ch, torch.matmul(v, cw))


def freq_split_circulant(x, r_hp, r_lp, g_hf=None, g_lf=None, dtype=F64):
    """The same operator as the kernels evaluate it: low = C_H x C_W with the circulants rounded to ``dtype``, the mixing of
    freq_mix_fwd / _bwd, dx = dx_direct - C_H s_hp C_W + C_H s_lp C_W.  With the pieces the bars are made of."""
    x = x.detach().to(dtype)
    H, W = x.shape[-2:]
    m = {r: (circulant_ref(H, r).to(dtype), circulant_ref(W, r).to(dtype)) for r in {r_hp, r_lp}}
    low_hp, low_lp = lowpass_circulant(x, *m[r_hp]), lowpass_circulant(x, *m[r_lp])
    z = torch.zeros_like(x)
    gh, gl = (z if g_hf is None else g_hf.to(dtype)), (z if g_lf is None else g_lf.to(dtype))
    s_hp, s_lp = 0.5 * gh * sgn(x - low_hp), -gl * sgn(low_lp)
    a, b = lowpass_circulant(s_hp, *m[r_hp]), lowpass_circulant(s_lp, *m[r_lp])
    direct = 0.5 * gh + s_hp
    out = {"hf": ((x - low_hp).abs() + x) * 0.5, "lf": -low_lp.abs(), "low_hp": low_hp, "low_lp": low_lp, "hp_abs": (x - low_hp).abs(),
           "dx": direct - a + b, "s_hp": s_hp, "s_lp": s_lp, "a": a, "b": b, "dx_direct": direct}
    return out


def lowpass_bar(v, r, ref_low):
    """bar_low of the docstring for C_H v C_W at radius r, (.., H, W) float64."""
    H, W = v.shape[-2:]
    p = lowpass_circulant(v.double().abs(), circulant_ref(H, r).abs(), circulant_ref(W, r).abs())
    return (gamma(H) + gamma(W) + gamma(H) * gamma(W) + 4 * U) * p + ulp32(ref_low.double())


assert FREQ_BARS["hf"] == ("short", 2) and all(FREQ_BARS[k] == ("exact",) for k in ("lf", "s_hp", "s_lp", "dx_direct"))


def forward_bars(x, r_hp, r_lp, ref):
    x = x.double()
    low = lowpass_bar(x, r_hp, ref["low_hp"])
    return {"low_hp": low, "low_lp": lowpass_bar(x, r_lp, ref["low_lp"]), "lf": lowpass_bar(x, r_lp, ref["lf"]),
            "hf": 0.5 * low + FREQ_BARS["hf"][1] * U * (ref["hp_abs"] + x.abs()) * 0.5 + ulp32(ref["hf"])}


@functools.lru_cache(maxsize=None)
def build_freq_split(shape, radii):
    """x, the two upstream gradients (zero at the kinks) and the forward reference of a (shape, radii) pair: computed once and
    shared by the three gradient cases and by every test that needs them; nobody writes to them."""
    g = torch.Generator().manual_seed(9000 + 10 * FS_SHAPES.index(shape) + FS_RADII.index(radii) if shape in FS_SHAPES else 9999)
    x = torch.randn(shape, generator=g) * 0.5 + 0.1
    g_hf, g_lf = torch.randn(shape, generator=g) + 0.25, torch.randn(shape, generator=g) - 0.25
    fwd = freq_split_ref(x, *radii)
    bars = forward_bars(x, *radii, fwd)
    kink_hp, kink_lp = fwd["hp_abs"] <= bars["low_hp"], fwd["low_lp"].abs() <= bars["low_lp"]
    g_hf, g_lf = g_hf * ~kink_hp, g_lf * ~kink_lp
    return {"x": x, "g_hf": g_hf, "g_lf": g_lf, "fwd": fwd, "bars": bars, "kink_hp": kink_hp, "kink_lp": kink_lp}


def upstream(c, grads):
    return (None if grads == "g_lf only" else c["g_hf"]), (None if grads == "g_hf only" else c["g_lf"])


@functools.lru_cache(maxsize=None)
def freq_split_case(case):
    """(inputs, float64 reference with "bar_hf", "bar_lf", "bar_dx", fp32 restatement) of a row of FS_CASES."""
    shape, radii, grads = case
    c = build_freq_split(shape, radii)
    g_hf, g_lf = upstream(c, grads)
    ref = dict(freq_split_ref(c["x"], *radii, g_hf, g_lf))
    circ = freq_split_circulant(c["x"], *radii, g_hf, g_lf)
    ref["bar_hf"], ref["bar_lf"] = c["bars"]["hf"], c["bars"]["lf"]
    ref["bar_dx"] = (lowpass_bar(circ["s_hp"], radii[0], circ["a"]) + lowpass_bar(circ["s_lp"], radii[1], circ["b"])
                     + 2 * U * (circ["dx_direct"].abs() + circ["a"].abs() + circ["b"].abs()) + ulp32(ref["dx"]))
    return c, ref, freq_split_circulant(c["x"], *radii, g_hf, g_lf, torch.float32)


def bar_violations(got, ref, name):
    g, r = _flat(got, ref[name])
    return _viol((g - r).abs(), ref["bar_" + name].double().reshape(-1))


def assert_fs_bars(tag, got, ref, names=("hf", "lf", "dx")):
    for name in names:
        assert tuple(got[name].shape) == tuple(ref[name].shape), (tag, name, got[name].shape, ref[name].shape)
        n, worst = bar_violations(got[name], ref, name)
        assert n == 0, "%s %s: %d elements outside the bar, worst at %.3g of it" % (tag, name, n, worst)


# ----------------------------------------------------------------------------------------
# the pins
# ----------------------------------------------------------------------------------------
def _pin(a, b, what, tol=PIN):
    assert tuple(a.shape) == tuple(b.shape), (what, a.shape, b.shape)
    assert rel_l2(a, b) <= tol, (what, rel_l2(a, b))


@pytest.mark.parametrize("c", SGEMM_CASES, ids=[ident("sgemm", c) for c in SGEMM_CASES])
def test_gemm_restatement_gathers_what_the_builder_scattered(c):
    """gemm_ref's index arithmetic against torch.matmul of the dense operands, which the builder placed with the same ``index``:
    so the layout itself is checked too -- entries do not overlap, the pointer offset leaves GUARD elements in front of the
    lowest entry, everything else is NaN."""
    for data in ("random", "integer"):
        b = build_sgemm(c, data)
        ref = gemm_ref(c, b)
        want = torch.matmul(b["dense_A"].double().expand(c.batch, c.M, c.K), b["dense_B"].double().expand(c.batch, c.K, c.N))
        assert torch.equal(ref["C"], want) and tuple(ref["C"].shape) == (c.batch, c.M, c.N)
        assert bool((ref["abs_C"] >= ref["C"].abs()).all()) and bool(torch.isfinite(ref["C"]).all())
        if data == "integer":
            assert c.K <= 1024 and float(b["dense_A"].abs().max() if c.K else 0) <= 8 and torch.equal(ref["C"], ref["C"].round())
            assert torch.equal(gemm_ref(c, b, torch.float32)["C"].double(), ref["C"])                    # exact in fp32, any order
    for which in ("A", "B", "C"):
        rows, ld, cols, stride, off = _operand(c, which)
        size, p = layout(c, which)
        idx = index(c, which)
        assert ld >= cols and p >= GUARD
        if idx.numel():
            assert int(idx.min()) == GUARD + off and int(idx.max()) == size - GUARD - 1
            if which == "C" or stride != 0:
                assert idx.unique().numel() == idx.numel(), "%s: batch entries of %s overlap" % (c.name, which)
        if which != "C":
            live = torch.zeros(size, dtype=torch.bool)
            live[idx.reshape(-1)] = True
            assert torch.equal(torch.isnan(b[which]), ~live)
    # a hand-written loop on the one case that has every stride, every ld and B's offset in play
    if c.name == "ld_all" or c.name.startswith("phase_loss_bwd_stacked_table_8x8"):
        b = build_sgemm(c)
        ref = gemm_ref(c, b)["C"]
        pa, pb = layout(c, "A")[1], layout(c, "B")[1]
        for bi in range(c.batch):
            for m in range(0, c.M, 5):
                for n in range(0, c.N, 7):
                    s = sum(float(b["A"][pa + bi * c.sA + m * c.lda + k]) * float(b["B"][pb + bi * c.sB + k * c.ldb + n]) for k in range(c.K))
                    assert abs(s - float(ref[bi, m, n])) <= 1e-12 * max(1.0, abs(s))


@pytest.mark.parametrize("n", DFT_N)
def test_dft_restatement_is_numpy_fft_of_the_identity(n):
    ref = dft_ref(n)
    f = np.fft.fft(np.eye(n, dtype=np.longdouble))          # in double the FFT itself is 1.4e-15 off at n = 257 (a prime: Bluestein)
    assert f.dtype == np.clongdouble and np.finfo(np.longdouble).eps < 2e-19
    cs, st = ref["cs"].numpy(), ref["stacked"].numpy()
    assert cs.shape == (n, 2 * n) and st.shape == (2 * n, n) and ref["flat"].numel() == 4 * n * n
    assert np.abs(cs[:, :n] - f.real).max() <= 1e-15 and np.abs(cs[:, n:] + f.imag).max() <= 1e-15        # F = C - i S
    assert np.array_equal(st[:n], cs[:, :n]) and np.array_equal(st[n:], cs[:, n:])
    assert np.array_equal(cs[:, :n], cs[:, :n].T) and np.array_equal(cs[:, n:], cs[:, n:].T)
    ex = ref["flat"][ref["exact"]]
    assert bool(((ex == 0) | (ex.abs() == 1)).all()) and int(ref["exact"].sum()) >= 4 * (2 * n - 1)       # row 0 and column 0 at least
    rest = ref["flat"][~ref["exact"]]
    assert bool(((rest != 0) & (rest.abs() < 1)).all())


@pytest.mark.parametrize("case", CIRC_CASES, ids=[ident("circ", c) for c in CIRC_CASES])
def test_circulant_restatement_is_the_fft_form(case):
    """C x == ifft(ifftshift(fftshift(fft x) g)) for the centred taps g, odd and even n; and the kernel's own sum, restated in
    float64, rounds to within the table bar of it -- with the shift the other way it does so for even n only."""
    n, r = case
    r = radius(n, r)
    C = circulant_ref(n, r)
    k = np.arange(n)
    g = np.exp(-0.5 * (k - int(n / 2)) ** 2 / f32(r) ** 2)
    x = np.random.RandomState(n).randn(n)
    y = np.fft.ifft(np.fft.ifftshift(np.fft.fftshift(np.fft.fft(x)) * g))
    assert np.abs(C.numpy() @ x - y.real).max() <= 1e-12 * np.abs(x).max() and np.abs(y.imag).max() <= 1e-12 * np.abs(x).max()
    assert float((C - C.T).abs().max()) <= 1e-15
    assert np.array_equal(circulant_taps(n, r), np.fft.ifftshift(g)) and circulant_taps(n, r)[0] == 1.0
    assert abs(float(C.sum(1)[0]) - 1.0) <= 1e-13
    extra = circulant_extra(n, r)
    assert table_violations(circulant_kernel_formula(n, r).float(), C, extra)[0] == 0
    wrong = table_violations(circulant_kernel_formula(n, r, shift=n - n // 2).float(), C, extra)[0]
    assert (wrong > 0) == (n % 2 == 1 and n > 1), (n, r, wrong)


@pytest.mark.parametrize("radii", FS_RADII)
def test_freq_split_restatement_is_the_oracle_and_the_circulant_form(radii):
    from oracle import octa_oracle as O
    g = torch.Generator().manual_seed(3)
    for H, W in ((37, 53), (8, 72), (16, 16)):
        x = torch.randn(2, 1, H, W, generator=g)
        gh, gl = torch.randn(2, 1, H, W, generator=g), torch.randn(2, 1, H, W, generator=g)
        xo = x.double().requires_grad_(True)
        hf, lf = O.freq_split(xo, *radii)
        (dx,) = torch.autograd.grad([hf, lf], [xo], [gh.double(), gl.double()])
        ref = freq_split_ref(x, *radii, gh, gl, mask32=True)                   # the oracle rounds its mask to fp32
        _pin(ref["hf"], hf, "hf")
        _pin(ref["lf"], lf, "lf")
        _pin(ref["dx"], dx, "dx")
        # the float64 mask moves the result by the mask's rounding only
        full = freq_split_ref(x, *radii, gh, gl)
        assert float((full["hf"] - ref["hf"]).abs().max()) <= 2 * U * float(x.abs().sum(dim=(-2, -1)).max()) and rel_l2(full["hf"], ref["hf"]) > 0
        # any C: every (b, c) plane on its own
        x3 = torch.randn(2, 3, H, W, generator=g)
        many = freq_split_ref(x3, *radii, x3 * 0 + 1, x3 * 0 - 2)
        for ch in range(3):
            one = freq_split_ref(x3[:, ch:ch + 1], *radii, x3[:, ch:ch + 1] * 0 + 1, x3[:, ch:ch + 1] * 0 - 2)
            for name in ("hf", "lf", "dx"):
                _pin(many[name][:, ch:ch + 1], one[name], name)
        # the circulant form: the low-pass part, then everything
        circ = freq_split_circulant(x, *radii, gh, gl)
        _pin(lowpass_circulant(x.double(), circulant_ref(H, radii[1]), circulant_ref(W, radii[1])), full["low_lp"], "C_H x C_W")
        for name in ("low_hp", "low_lp", "hf", "lf", "dx"):
            _pin(circ[name], full[name], name)
        for grads in FS_GRADS[1:]:
            a, b = (gh, None) if grads == "g_hf only" else (None, gl)
            _pin(freq_split_circulant(x, *radii, a, b)["dx"], freq_split_ref(x, *radii, a, b)["dx"], "dx, " + grads)


# ----------------------------------------------------------------------------------------
# the tables and the bars themselves
# ----------------------------------------------------------------------------------------
def test_constants_match_the_source():
    k = read_constants()
    assert k["KC"] == KC and k["NT"] == NT and k["tile"] == [TILE] and k["round"] == [TILE] and k["wave"] == [WAVE_N] and k["mfma_k"] == MFMA_K
    assert NT == TILE and 2 * WAVE_N == TILE                                  # 2 x 2 waves of 32 x 32 on one 64 x 64 tile
    assert k["batch_cap"] == BATCH_CAP and k["m_cap"] == [BATCH_CAP, TILE]
    assert k["circ_n_cap"] == N_CAP and k["dft_n_cap"] == N_CAP and k["table_block"] == [256]


def test_every_form_is_reached():
    got = covered_forms()
    assert got == FORMS, (sorted(FORMS - got), sorted(got - FORMS))
    test_constants_match_the_source()
    # no case is redundant in name, every caller shape is there at both sizes, and the issue's sizes are in the tables
    names = [c.name for c in SGEMM_CASES + SGEMM_EMPTY]
    assert len(set(names)) == len(names)
    for caller in CALLERS:
        assert {caller + "_37x53", caller + "_8x8"} <= set(names)
    by = {c.name: c for c in SGEMM_CASES}
    assert forms("sgemm", by["one_tile"]) == {"sgemm: full tiles only"}
    assert forms("sgemm", by["N31"]) == {"sgemm: N tail", "sgemm: upper column wave idle"}
    assert "sgemm: upper column wave idle" in forms("sgemm", by["N1"]) and "sgemm: upper column wave idle" not in forms("sgemm", by["N33"])
    assert forms("sgemm", by["N65"]) >= {"sgemm: several column tiles", "sgemm: upper column wave idle"}
    assert forms("sgemm", by["K17"]) == {"sgemm: K tail", "sgemm: K tail, odd", "sgemm: several K chunks"}
    assert forms("sgemm", by["K0"]) == {"sgemm: K = 0"} and "sgemm: K below one chunk" in forms("sgemm", by["K15"])
    assert forms("sgemm", by["batch2_negative_strideA"]) >= {"sgemm: negative strideA", "sgemm: strideB = 0"}
    assert all(c.K <= 1024 for c in SGEMM_CASES)                                                 # the exact bar's condition
    # a tile constant that moves takes forms away: the tables would have to follow
    k = read_constants()
    for change in ({"KC": 32}, {"tile": [128]}, {"wave": [64]}, {"KC": 8}, {"tile": [32]}):
        assert covered_forms(k=dict(k, **change)) != FORMS, change
    # a case that is the only one of its form takes the form with it
    assert {op: len(t) for op, t in TABLES.items()} == {"sgemm": 33, "dft": 12, "circ": 40, "fs": 24} and len(SGEMM_EMPTY) == 3
    for drop in ("one_tile", "M1", "K0", "ld_all", "batch2_negative_strideA", "sprof_bwd_half_stacked_table_37x53"):
        rest = [c for c in SGEMM_CASES if c.name != drop]
        if drop.endswith("37x53"):
            rest = [c for c in rest if c.name != drop.replace("37x53", "8x8")]
        assert covered_forms(dict(TABLES, sgemm=rest)) != FORMS, drop
    assert covered_forms(dict(TABLES, dft=[n for n in DFT_N if n != 1024])) != FORMS
    assert covered_forms(dict(TABLES, circ=[c for c in CIRC_CASES if c[1] != 0.3])) != FORMS
    assert covered_forms(dict(TABLES, circ=[c for c in CIRC_CASES if c[0] != 1])) != FORMS
    assert covered_forms(dict(TABLES, fs=[c for c in FS_CASES if c[0] != (1, 2, 8, 72)])) != FORMS
    assert covered_forms(dict(TABLES, fs=[c for c in FS_CASES if c[2] != "g_lf only"])) != FORMS


@pytest.mark.parametrize("c", SGEMM_CASES, ids=[ident("sgemm", c) for c in SGEMM_CASES])
def test_fp32_gemm_meets_the_bars(c):
    """torch's fp32 matmul on the CPU is a K-term inner product in some order: it must meet the same bar, and be exact on integers."""
    b = build_sgemm(c)
    n, worst = gemm_violations(gemm_ref(c, b, torch.float32)["C"], gemm_ref(c, b), c.K)
    assert n == 0, (c.name, n, worst)
    # the bar is not vacuous: a hundredth of one typical product a b is outside it everywhere
    if c.K:
        ref = gemm_ref(c, b)
        assert gemm_violations(ref["C"] + 0.01, ref, c.K)[0] == ref["C"].numel()


@pytest.mark.parametrize("shape,radii", [(s, r) for s in FS_SHAPES for r in FS_RADII], ids=lambda v: "x".join(map(str, v)))
def test_freq_split_kinks_are_rare_and_the_fp32_circulant_form_meets_the_bars(shape, radii):
    c = build_freq_split(shape, radii)
    n = c["x"].numel()
    assert int(c["kink_hp"].sum()) <= KINK_CAP * n and int(c["kink_lp"].sum()) <= KINK_CAP * n, (int(c["kink_hp"].sum()), int(c["kink_lp"].sum()), n)
    assert float(c["g_hf"][c["kink_hp"]].abs().sum()) == 0.0 and float(c["g_lf"][c["kink_lp"]].abs().sum()) == 0.0
    assert bool((c["bars"]["hf"] < 1e-5).all()) and bool((c["bars"]["lf"] < 1e-5).all())           # |values| are O(1)
    for grads in FS_GRADS:
        _, ref, ref32 = freq_split_case((shape, radii, grads))
        assert_fs_bars(ident("fs", (shape, radii, grads)), ref32, ref)
        assert bool((ref["bar_dx"] < 1e-4).all())
        # a flipped sign of one s_hp / s_lp element would be far outside the bar
        assert float(ref["dx"].abs().mean()) > 1e3 * float(ref["bar_dx"].mean())


# ----------------------------------------------------------------------------------------
# refusals on the host: the checks come before any launch, so pointers are never dereferenced and no device is needed
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import faoctasr
    return faoctasr._lib.load()


def test_bad_arguments_are_refused_with_a_message(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    EINVAL, EUNSUPPORTED = -1, -2

    def sgemm(A=p, B=p, C=p, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, sA=0, sB=0, sC=0, batch=1):
        return lib.faoctasr_sgemm_batched(A, B, C, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, None)
    for kw in ({"A": None}, {"B": None}, {"C": None}):
        assert sgemm(**kw) == EINVAL and b"sgemm_batched: null" in lib.faoctasr_last_error(), kw
    for kw in ({"lda": 7}, {"ldb": 7}, {"ldc": 7}, {"M": -1}, {"N": -1, "ldb": 0, "ldc": 0}, {"K": -1}, {"batch": -1}):
        assert sgemm(**kw) == EINVAL and b"sgemm_batched: bad shape" in lib.faoctasr_last_error(), kw
    assert sgemm(batch=BATCH_CAP + 1) == EUNSUPPORTED and b"batch 65536" in lib.faoctasr_last_error()
    # the row grid: (M + 63) / 64 blocks in y, at most 65535
    assert sgemm(M=(BATCH_CAP + 1) * TILE) == EUNSUPPORTED
    assert b"sgemm_batched: M 4194304" in lib.faoctasr_last_error()
    assert sgemm(M=BATCH_CAP * TILE + 1) == EUNSUPPORTED and sgemm(M=2 ** 31 - 1) == EUNSUPPORTED
    # nothing to do is not an error, whatever else the call holds
    assert sgemm(M=0) == 0 and sgemm(N=0) == 0 and sgemm(batch=0) == 0
    assert sgemm(M=0, batch=BATCH_CAP + 1) == 0 and sgemm(N=0, M=(BATCH_CAP + 1) * TILE) == 0
    # a bad shape is refused even where there is nothing to do
    assert sgemm(M=0, lda=7) == EINVAL and sgemm(batch=0, A=None) == EINVAL

    def circ(out=p, n=8, r=5.0):
        return lib.faoctasr_circulant_lowpass(out, n, r, None)
    assert circ(out=None) == EINVAL and b"circulant_lowpass: null" in lib.faoctasr_last_error()
    for kw in ({"n": 0}, {"n": -3}, {"n": N_CAP + 1}, {"r": 0.0}, {"r": -1.0}, {"r": float("nan")}):
        assert circ(**kw) == EINVAL and b"circulant_lowpass: n" in lib.faoctasr_last_error(), kw
    assert lib.faoctasr_dft_tables(None, 8, None) == EINVAL and b"dft_tables: null" in lib.faoctasr_last_error()
    for n in (0, -1, N_CAP + 1):
        assert lib.faoctasr_dft_tables(p, n, None) == EINVAL and b"dft_tables: n" in lib.faoctasr_last_error(), n
