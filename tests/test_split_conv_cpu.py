"""The split-precision convolutions, without a GPU: the wide gather kernel (csrc/igemm_bf16x3.hip, route 4, precisions 2 "bf16x3" and
3 "f16x2"), the f16x2 narrow-map kernel (csrc/igemm_nm_x2.hip, route 8) and the split weight gradient (csrc/wgrad_x3.hip, route 15).
This file holds the case tables, the input builders, the float64 restatements (each pinned here), the bars, the map from a case to
the forms of the launchers it reaches, and the host probes; tests/test_gpu_split_conv.py runs the tables through the C ABI and takes
everything from here.

Restatements
  conv_ref    float64 F.conv2d / F.conv_transpose2d for the six entry points, in the kernels' order act(conv + bias) + res (weight
              gradients: + the content of dw when accumulating).  Reflection padding is F.pad(mode="reflect"); for a reflecting
              layer the input gradient is the gradient with respect to the PADDED input (include/faoctasr.h).  The gradient kinds
              are closed forms (a transposed convolution; a convolution over the batch axis with dilation = stride) pinned to
              torch autograd.
  split_ref   the same contraction on the operands the kernels really multiply: bf16x3 hi = bf16(x), lo = bf16(x - hi); f16x2
              hi = f16(x s), lo = f16(x s - hi) with s = f16x2_scale(max |x|) restated from csrc/split16.h (a zero, tiny (< 2^-111),
              infinite or NaN maximum leaves the tensor unscaled).  hi*hi + hi*lo + lo*hi summed in float64, descaled.
              Pinned twice: on integer data it equals conv_ref to the bit; on random data it is within the representation bound
                  bf16x3: |lo| <= 2^-9 |x|, so lo*lo <= 2^-18 |x||w|, and x - hi - lo <= 2^-18 |x| per operand:  3 * 2^-18 < 2^-16
                  f16x2 : |lo| <= 2^-11 |x|, so lo*lo <= 2^-22 |x||w|, and x - hi - lo <= 2^-22 |x| per operand: 3 * 2^-22 < 2^-20
              of the same convolution on |x|, |w| (the fp16 subnormal quantum, 2^-38 of the maximum, is far below the data here).

Bars (none measured on the kernels), u = 2^-24, gamma_n = n u / (1 - n u)
  integer   x, dy in [-8, 8], w in [-4, 4], bias / residual / accumulated dw small integers.  Every hi half is exact (bf16 holds 8
            bits, f16 11; the f16x2 scale is a power of two), every lo half is 0, every product is an integer times one power of two
            and every partial sum stays below 2^24 of that unit while  P K + 100 < 2^24  (P = 32 for a gather, K = channels x taps;
            P = 64 for a weight gradient, K = N OH OW: asserted for every case).  The descale is a power of two.  So bias, residual,
            split-K atomics in any order, the two-pass reductions and accumulate != 0 are all exact: the result equals conv_ref TO
            THE BIT.  ReLU is exact; LeakyReLU is the single fp32 product fp32(v) * fp32(slope), and a residual on top of it one fp32
            addition, both of which torch's fp32 reproduces.  tanh has no integer mode.
  random    |got - split_ref| <= gamma_n (|terms| summed) + 1 ulp32: Higham's bound for an n-term sum in any order; the products
            of two 8-bit (11-bit) halves are exact in fp32.  n = 3 K (three families) + one addition each for bias, residual,
            LeakyReLU's product and every K slice the launcher makes for the case (``additions``: x3_plan's and nx2_plan's ksplit; a
            weight gradient's slices, the 16 group sums of its reduction kernel and the addition into dw).  |terms| is the same
            contraction on the absolute values of the emulated halves, plus |bias|, |res|, |dw0|.  ReLU / LeakyReLU are 1-Lipschitz, so the bar before the activation holds after it; tanh is
            1-Lipschitz too and adds the library bar of test_pointwise (rtol 1e-6, atol 1e-6).
            A case that leaves the split routes runs on an exact-f32 kernel: the same bar with hi = x, lo = 0 and n = K + bias +
            residual + LeakyReLU.  Those kernels' own K slices (not restated here) only regroup the same K terms, which the
            any-order bound already covers; the first partial lands on a zeroed output exactly.
  aggregate the bars the suite already holds are asserted as well: rel_l2 < 3e-5 (bf16x3), < 2e-6 (f16x2) against conv_ref.
``SPLIT_ERR`` lines (tests/test_gpu_split_conv.py) record e_split / e_hip / ratio / worst ulp; reported, not asserted.

Forms that no admissible shape reaches are listed in UNREACHABLE with the reason."""
import collections
import ctypes
import functools
import math
import os
import re
import struct
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_norm_cpu import CSRC, PIN, rel_l2, ulp32

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
GATHER = ("conv2d_fwd", "conv2d_dgrad", "conv_transpose2d_fwd", "conv_transpose2d_dgrad")
WGRAD = ("conv2d_wgrad", "conv_transpose2d_wgrad")
KIND_ID = {k: i for i, k in enumerate(GATHER + WGRAD)}
ARITH = {"bf16x3": 2, "f16x2": 3}
REP_BOUND = {"bf16x3": 2.0 ** -16, "f16x2": 2.0 ** -20, "f32": 0.0}
AGGREGATE = {"bf16x3": 3e-5, "f16x2": 2e-6}
ACT_ID = {None: 0, "relu": 1, "lrelu": 2, "tanh": 3}
NO_SPLIT_K = 0x100
SLOT_WORDS, SLOT_PARTS, SLOT_STRIDE = 128, 8, 16
ROUTE_X3, ROUTE_NX2, ROUTE_WX3 = 4, 8, 15


# ----------------------------------------------------------------------------------------
# constants of the sources
# ----------------------------------------------------------------------------------------
def _int(pattern, text, group=1):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(group))


@functools.lru_cache(maxsize=None)
def read_constants():
    """The constants the form map depends on, read out of the sources."""
    s = open(os.path.join(CSRC, "igemm_bf16x3.hip")).read()
    n = open(os.path.join(CSRC, "igemm_nm_x2.hip")).read()
    w = open(os.path.join(CSRC, "wgrad_x3.hip")).read()
    i = open(os.path.join(CSRC, "igemm.hip")).read()
    nx = re.search(r"constexpr int NX_MT = (\d+), NX_NT = (\d+), NX_KS = (\d+);", n)
    x3 = re.findall(r"\(C & (\d+)\) \|\| \(M & (\d+)\) \|\| \(OW & (\d+)\) \|\| \(OH & (\d+)\)", w)
    assert len(x3) == 2 and x3[0] == x3[1], x3
    return {
        "SP_MIN_W": _int(r"#define SP_MIN_W (\d+)", s), "SP_SPLIT_BELOW": _int(r"#define SP_SPLIT_BELOW (\d+)", s),
        "SP_NCW8": _int(r"#define SP_NCW8 (\d+)", s), "SP_MT": _int(r"constexpr int SP_MT = (\d+);", s),
        "SP_NPI": _int(r"constexpr int SP_NPI = (\d+);", s), "SP_LDS_MAX": 1024 * _int(r"constexpr size_t SP_LDS_MAX = (\d+) \* 1024;", s),
        "SP_ITEMS": _int(r"2 \* PH \* PW > (\d+) \* SP_NPI", s), "SP_GRID": _int(r"ksplit = \(int\)\((\d+) / blocks\);", s),
        "SP_GROUPS_PER_SLICE": _int(r"if \(ksplit > ngroups / (\d+)\) ksplit = ngroups / \1;", s),
        "SP_MIN_C": _int(r"if \(g\.C < (\d+) \|\| \(g\.SI != 1 && g\.SI != 2\)\) return 0;", s),
        "SP_QUAD_ITEMS": _int(r"2 \* PH \* nq > (\d+) \|\| 2 \* PH \* ns > \1", s),
        "NX_MT": int(nx.group(1)), "NX_NT": int(nx.group(2)), "NX_KS": int(nx.group(3)),
        "NX_MIN_M": _int(r"if \(!g\.f16 \|\| g\.M < (\d+) \|\| \(g\.C & 15\)", n), "NX_SPLIT_BELOW": _int(r"if \(split_ok && blocks < (\d+)\)", n),
        "NX_TARGET": _int(r"ksplit = \(int\)\(\((\d+) \+ blocks - 1\) / blocks\);", n), "NX_MAX_SLICES": _int(r"if \(ksplit > (\d+)\) ksplit = \1;", n),
        "NX_MIN_CHUNKS": _int(r"if \(ksplit > minchunks / (\d+)\) ksplit = minchunks / \1;", n),
        "WX_C": int(x3[0][0]) + 1, "WX_M": int(x3[0][1]) + 1, "WX_OW": int(x3[0][2]) + 1, "WX_OH": int(x3[0][3]) + 1,
        "WX_IW": _int(r"\(OH & 1\) \|\| \(IW & (\d+)\) \|\| wsc", w) + 1, "WX_GRID": _int(r"long slices = (\d+) / \(\(long\)g\.gx \* g\.gy\);", w),
        "WX_MIN_W": _int(r"if \(OW >= (\d+)\) \{      // wide maps", i), "WX_REFLECT_MIN_W": _int(r"if \(reflect && \(IH <= pad \|\| IW < (\d+)\)\) return 0;", w),
        "MAX_TAPS": _int(r"if \(KH \* KW > (\d+) \|\| KH > 16 \|\| KW > 16\)", i), "MAX_PAD": _int(r"if \(pad > (\d+)\) return fail", i),
    }


# ----------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name kind N C H W M k s p reflect out_pad bias act slope res align nosplit ws acc")


def case(name, kind, dims, reflect=0, out_pad=0, bias=False, act=None, slope=0.2, res=False, align="", nosplit=False, ws="exact", acc=0):
    """dims = (N, C, H, W, M, k, s, p) as the C ABI receives them (a transposed convolution's weights are [C, M, k, k]; a reflecting
    layer's input gradient is called with the padded size and pad 0, as ops.py does, but is listed here with the layer's own numbers).
    align: which of "x", "y", "r" (residual) sit 4 bytes past a 16-byte boundary.  ws: "exact" | "none" | "short" (one float short)."""
    return Case(name, kind, *dims, reflect, out_pad, bias, act, slope, res, align, nosplit, ws, acc)


def out_hw(c):
    if c.kind in ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad"):
        return (c.H + 2 * c.p - c.k) // c.s + 1, (c.W + 2 * c.p - c.k) // c.s + 1
    return (c.H - 1) * c.s - 2 * c.p + c.k + c.out_pad, (c.W - 1) * c.s - 2 * c.p + c.k + c.out_pad


def shapes(c):
    """(shape of operand a, shape of operand b, shape of the output).  a is the gathered activation (x or dy) of a gather kind and x
    of a weight gradient; b is the weights of a gather kind and dy of a weight gradient."""
    OH, OW = out_hw(c)
    wshape = (c.M, c.C, c.k, c.k) if c.kind.startswith("conv2d") else (c.C, c.M, c.k, c.k)
    xs, ys = (c.N, c.C, c.H, c.W), (c.N, c.M, OH, OW)
    if c.kind in ("conv2d_fwd", "conv_transpose2d_fwd"):
        return xs, wshape, ys
    if c.kind in WGRAD:
        return xs, ys, wshape
    if c.reflect:
        xs = (c.N, c.C, c.H + 2 * c.p, c.W + 2 * c.p)
    return ys, wshape, xs


def abi_dims(c):
    """(N, C, IH, IW, M, KH, KW, stride, pad) as the call passes them."""
    if c.kind == "conv2d_dgrad" and c.reflect:
        return (c.N, c.C, c.H + 2 * c.p, c.W + 2 * c.p, c.M, c.k, c.k, c.s, 0)
    return (c.N, c.C, c.H, c.W, c.M, c.k, c.k, c.s, c.p)


def reduction(c):
    """(K, P): the terms of one output element (an upper bound where phases differ) and the largest product of integer operands."""
    OH, OW = out_hw(c)
    if c.kind in WGRAD:
        return c.N * max(OH * OW, c.H * c.W), 64
    taps = c.k * c.k if c.kind in ("conv2d_fwd", "conv_transpose2d_dgrad") else math.ceil(c.k / c.s) ** 2
    return (c.C if c.kind in ("conv2d_fwd", "conv_transpose2d_fwd") else c.M) * taps, 32


def ident(c):
    return c.name


D = "conv2d_fwd", "conv2d_dgrad", "conv_transpose2d_fwd", "conv_transpose2d_dgrad", "conv2d_wgrad", "conv_transpose2d_wgrad"
FWD, DGR, TFWD, TDGR, WGR, TWGR = D
BASE = (1, 16, 8, 32, 64, 3, 1, 1)


def _with(dims=BASE, **kw):
    names = "N C H W M k s p".split()
    d = dict(zip(names, dims), **kw)
    return tuple(d[n] for n in names)


def _epilogues(tag, dims):
    out = []
    for act, slope in ((None, 0.2), ("relu", 0.2), ("lrelu", 0.2), ("lrelu", 0.0), ("tanh", 0.2)):
        for bias in (False, True):
            for res in (False, True):
                if act is None and not bias and not res:
                    continue
                name = "%s_%s%s%s" % (tag, (act or "none") + ("0" if act == "lrelu" and slope == 0.0 else ""), "_bias" if bias else "", "_res" if res else "")
                out.append(case(name, FWD, dims, bias=bias, act=act, slope=slope, res=res))
    return out


WIDE_CASES = (
    [case("plain", FWD, BASE)]
    + [case("M%d" % m, FWD, _with(M=m), bias=True) for m in (24, 65, 130)]
    + [case("W%d" % w, FWD, _with(W=w)) for w in (24, 36, 34, 23)]
    + [case("H%d" % h, FWD, _with(H=h)) for h in (1, 9, 17)]
    + [case("C%d" % ch, FWD, _with(C=ch)) for ch in (17, 24, 31, 15)]
    + [case("splitk_C64_even", FWD, _with(C=64)), case("splitk_C80_uneven", FWD, _with(C=80)), case("splitk_C96_three", FWD, _with(C=96)),
       case("splitk_C144_empty_slice", FWD, _with(C=144)),
       case("splitk_bias", FWD, _with(C=64), bias=True), case("splitk_res", FWD, _with(C=64), res=True),
       case("splitk_bias_res_M65", FWD, _with(C=80, M=65), bias=True, res=True), case("splitk_off", FWD, _with(C=64), bias=True, nosplit=True),
       case("splitk_dword_W34", FWD, _with(C=64, W=34), bias=True, res=True)]
    + [case("persistent_M512", FWD, _with(N=3, M=512, H=17, W=100))]
    + [case("k5", FWD, _with(k=5, p=2)), case("k7_zero", FWD, _with(k=7, p=3)), case("k7_reflect", FWD, _with(k=7, p=3), reflect=1),
       case("k4_s1", FWD, _with(k=4, p=1)), case("k8_64taps", FWD, _with(k=8, p=3, H=10))]
    + [case("reflect_W36_mirrored_piece", FWD, _with(W=36, k=7, p=3), reflect=1), case("reflect_k3_W32", FWD, _with(), reflect=1),
       case("reflect_k3_W64_inside", FWD, _with(W=64), reflect=1), case("reflect_H_pad_plus_1", FWD, _with(H=4, k=7, p=3), reflect=1),
       case("reflect_dgrad_k7", DGR, _with(k=7, p=3), reflect=1), case("reflect_dgrad_k3", DGR, _with(), reflect=1)]
    + [case("s2_k4", FWD, _with(H=16, W=48, k=4, s=2, p=1)), case("s2_k3", FWD, _with(H=16, W=48, k=3, s=2, p=1)),
       case("s2_k3_W50", FWD, _with(H=15, W=50, k=3, s=2, p=1), bias=True), case("s2_k2_staged", FWD, _with(H=18, W=48, k=2, s=2, p=0), res=True)]
    + [case("dgrad_s1", DGR, _with(), res=True), case("dgrad_s1_M24_C65", DGR, _with(C=65, M=24)),
       case("dgrad_s2_k4", DGR, _with(H=16, W=48, k=4, s=2, p=1)), case("dgrad_s2_k3", DGR, _with(H=16, W=48, k=3, s=2, p=1), res=True),
       case("dgrad_s2_k3_odd", DGR, _with(H=15, W=49, k=3, s=2, p=1)),
       case("tfwd_k4", TFWD, _with(H=8, W=24, k=4, s=2, p=1), bias=True), case("tfwd_k3_outpad1", TFWD, _with(H=8, W=24, k=3, s=2, p=1), out_pad=1, act="relu"),
       case("tfwd_k3_outpad0_W24", TFWD, _with(H=8, W=24, k=3, s=2, p=1)), case("tfwd_k3_outpad0_W25", TFWD, _with(H=8, W=25, k=3, s=2, p=1), bias=True, res=True),
       case("tdgrad_k4", TDGR, _with(H=8, W=24, k=4, s=2, p=1)), case("tdgrad_k3_outpad1", TDGR, _with(H=8, W=24, k=3, s=2, p=1), out_pad=1, res=True)]
    + [case("align_x", FWD, BASE, align="x"), case("align_y", FWD, BASE, align="y", res=True), case("align_r", FWD, BASE, align="r", res=True, bias=True),
       case("align_r_tail", FWD, _with(H=9, W=36, M=65), align="r", res=True), case("align_xyr", FWD, BASE, align="xyr", res=True)]
    + _epilogues("epi_interior", BASE) + _epilogues("epi_tail", _with(H=9, W=36, M=65))
    + [case("act_switches_splitk_off", FWD, _with(C=64), act="relu", bias=True)])

NX_BASE = (1, 16, 4, 4, 64, 4, 1, 1)
NARROW_CASES = (
    [case("nx_min", FWD, NX_BASE)]
    + [case("nx_M%d" % m, FWD, _with(NX_BASE, M=m), bias=True) for m in (128, 192, 63)]
    + [case("nx_C24", FWD, _with(NX_BASE, C=24)), case("nx_C48_k3_chunks", FWD, _with(NX_BASE, C=48, k=3)), case("nx_C64_k3_unsplit_epilogue", FWD, _with(NX_BASE, C=64, k=3), bias=True, act="lrelu", res=True)]
    + [case("nx_pix1", FWD, _with(NX_BASE, H=2, W=2, p=1, k=4)), case("nx_pix63", FWD, _with(NX_BASE, N=7, H=4, W=4)),
       case("nx_pix64", FWD, _with(NX_BASE, H=9, W=9)), case("nx_pix65", FWD, _with(NX_BASE, N=5, H=2, W=14, M=192), bias=True, res=True)]
    + [case("nx_dgrad_s2_k4", DGR, _with(NX_BASE, C=64, H=8, W=8, M=64, s=2), res=True), case("nx_dgrad_s2_k3_empty_slice", DGR, _with(NX_BASE, C=64, H=8, W=8, M=1024, k=3, s=2)),
       case("nx_tfwd_k3_outpad1", TFWD, _with(NX_BASE, C=1024, H=4, W=4, k=3, s=2), out_pad=1, bias=True, act="lrelu", res=True),
       case("nx_tdgrad_k4", TDGR, _with(NX_BASE, C=64, H=4, W=4, M=64, s=2))]
    + [case("nx_splitk_%d" % ch, FWD, _with(NX_BASE, C=ch), bias=True, act="lrelu", res=True) for ch in (64, 128, 256, 512)]
    + [case("nx_splitk_no_ws", FWD, _with(NX_BASE, C=256), bias=True, ws="none"), case("nx_splitk_short_ws", FWD, _with(NX_BASE, C=256), bias=True, ws="short"),
       case("nx_splitk_off", FWD, _with(NX_BASE, C=256), bias=True, nosplit=True), case("nx_reflect", FWD, _with(NX_BASE, C=64, H=6, W=6, k=3), reflect=1)])

WX_BASE = (1, 64, 2, 32, 64, 3, 1, 1)
WGRAD_CASES = (
    [case("wx_roll", WGR, WX_BASE)]
    + [case("wx_roll_W%d" % w, WGR, _with(WX_BASE, W=w, H=6), acc=1) for w in (64, 96)]
    + [case("wx_roll_H%d" % h, WGR, _with(WX_BASE, H=h)) for h in (6, 10)]
    + [case("wx_roll_C128", WGR, _with(WX_BASE, C=128, H=6)), case("wx_roll_M128", WGR, _with(WX_BASE, M=128, H=6), acc=1),
       case("wx_roll_N3", WGR, _with(WX_BASE, N=3, H=6)), case("wx_roll_atomics", WGR, _with(WX_BASE, N=3, H=6), ws="none", acc=1),
       case("wx_roll_short_ws", WGR, _with(WX_BASE, N=3, H=6), ws="short")]
    + [case("wx_row_k7_zero", WGR, _with(WX_BASE, H=6, W=64, k=7, p=3)), case("wx_row_k7_reflect", WGR, _with(WX_BASE, H=6, W=64, k=7, p=3), reflect=1, acc=1),
       case("wx_row_k7_reflect_W32", WGR, _with(WX_BASE, N=2, H=4, k=7, p=3), reflect=1), case("wx_row_k7_zero_W32_atomics", WGR, _with(WX_BASE, N=2, H=4, k=7, p=3), ws="none"),
       case("wx_row_k4_s2", WGR, _with(WX_BASE, N=3, H=4, W=64, k=4, s=2), acc=1), case("wx_row_k3_s2", WGR, _with(WX_BASE, H=12, W=128, k=3, s=2)),
       case("wx_row_k4_s2_M128_atomics", WGR, _with(WX_BASE, H=4, W=64, M=128, k=4, s=2), ws="none"),
       case("wx_t_k4", TWGR, _with(WX_BASE, N=2, H=2, W=32, k=4, s=2), acc=1), case("wx_t_k3_outpad1", TWGR, _with(WX_BASE, H=6, W=32, M=128, k=3, s=2), out_pad=1)]
    + [case("wx_out_OW48", WGR, _with(WX_BASE, W=48)), case("wx_out_OH3", WGR, _with(WX_BASE, H=3)), case("wx_out_C96", WGR, _with(WX_BASE, C=96)),
       case("wx_out_M32", WGR, _with(WX_BASE, M=32), acc=1), case("wx_out_IW66_s2", WGR, _with(WX_BASE, H=4, W=66, k=4, s=2)),
       case("wx_out_k5", WGR, _with(WX_BASE, k=5, p=2)), case("wx_out_t_outpad0", TWGR, _with(WX_BASE, H=2, W=32, k=3, s=2))])
TABLES = {"wide": WIDE_CASES, "narrow": NARROW_CASES, "wgrad": WGRAD_CASES}
ALL_CASES = WIDE_CASES + NARROW_CASES + WGRAD_CASES


def modes(c):
    return ("random",) if c.act == "tanh" else ("integer", "random")


# ----------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(c, mode, scale_a=1.0, scale_b=1.0):
    """{"a", "b", "bias", "res", "dw0"}: fp32 operands (a, b as in ``shapes``); integer mode: a in [-8, 8] (dy of a weight gradient
    too), weights in [-4, 4], the rest small integers.  scale_a / scale_b multiply a / b (powers of two: scale invariance)."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    sa, sb, so = shapes(c)
    if mode == "integer":
        a = torch.randint(-8, 9, sa, generator=g).float()
        b = torch.randint(-8, 9, sb, generator=g).float() if c.kind in WGRAD else torch.randint(-4, 5, sb, generator=g).float()
        bias, res, dw0 = (torch.randint(-8, 9, s, generator=g).float() for s in ((so[1],), so, so))
    else:
        a = torch.randn(sa, generator=g)
        b = torch.randn(sb, generator=g) * (1.0 if c.kind in WGRAD else 0.1)
        bias, res, dw0 = (torch.randn(s, generator=g) for s in ((so[1],), so, so))
    return {"a": a * scale_a, "b": b * scale_b, "bias": bias if c.bias else None, "res": res if c.res else None,
            "dw0": dw0 if c.kind in WGRAD and c.acc else None}


# ----------------------------------------------------------------------------------------
# restatements
# ----------------------------------------------------------------------------------------
def _pad(c, x):
    return F.pad(x, (c.p,) * 4, mode="reflect") if c.reflect else x


def bilinear(c, a, b):
    """The contraction of a case without bias, activation, residual; a, b as in ``shapes``, any floating dtype."""
    s, p, k = c.s, c.p, c.k
    if c.kind == "conv2d_fwd":
        return F.conv2d(_pad(c, a), b, stride=s, padding=0 if c.reflect else p)
    if c.kind == "conv2d_dgrad":
        pp = 0 if c.reflect else p
        H, W = (c.H + 2 * c.p, c.W + 2 * c.p) if c.reflect else (c.H, c.W)
        return F.conv_transpose2d(a, b, stride=s, padding=pp, output_padding=((H + 2 * pp - k) % s, (W + 2 * pp - k) % s))
    if c.kind == "conv_transpose2d_fwd":
        return F.conv_transpose2d(a, b, stride=s, padding=p, output_padding=c.out_pad)
    if c.kind == "conv_transpose2d_dgrad":
        return F.conv2d(a, b, stride=s, padding=p)
    if c.kind == "conv2d_wgrad":             # dw[m, c, i, j] = sum_n,o x_pad[n, c, o s + (i, j)] dy[n, m, o]: a convolution over the batch axis
        xp = _pad(c, a) if c.reflect else F.pad(a, (p,) * 4)
        return F.conv2d(xp.transpose(0, 1), b.transpose(0, 1), dilation=s)[:, :, :k, :k].transpose(0, 1)
    # conv_transpose2d_wgrad: dw[c, m, i, j] = sum x[n, c, o] dy_pad[n, m, o s + (i, j)]
    return F.conv2d(F.pad(b, (p,) * 4).transpose(0, 1), a.transpose(0, 1), dilation=s)[:, :, :k, :k].transpose(0, 1)


def epilogue(c, v, d, integer=False):
    """act(v + bias) + res (+ dw0), in v's dtype; ``integer``: v is an integer below 2^24, so the kernels' own fp32 operations are
    reproduced one by one: the sums are exact, LeakyReLU is the fp32 product v * slope, the residual is one fp32 addition to it."""
    if integer:
        assert bool((v == v.float().to(v.dtype)).all())
        return epilogue(c, v.float(), d).to(v.dtype)
    if d["bias"] is not None:
        v = v + d["bias"].to(v.dtype).view(1, -1, 1, 1)
    if c.act == "relu":
        v = v.clamp_min(0)
    elif c.act == "lrelu":
        v = torch.where(v > 0, v, v * torch.tensor(c.slope, dtype=F32).to(v.dtype))
    elif c.act == "tanh":
        v = torch.tanh(v)
    for extra in (d["res"], d["dw0"]):
        if extra is not None:
            v = v + extra.to(v.dtype)
    return v


def conv_ref(kind, c, d, integer=False):
    assert kind == c.kind
    return epilogue(c, bilinear(c, d["a"].double(), d["b"].double()), d, integer)


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def f16x2_scale(absmax_bits):
    """csrc/split16.h f16x2_scale: 2^(141 - e) for a maximum 1.m x 2^(e - 127); unscaled for e < 16 (zero, tiny) and e = 255 (inf, NaN)."""
    e = (absmax_bits >> 23) & 0xff
    return 1.0 if e < 16 or e == 255 else 2.0 ** (141 - e)


def absmax_bits(t):
    """The slot's content: the largest fp32 bit pattern of |t| (a NaN orders above everything, as the kernel's unsigned maximum does)."""
    return int(t.float().abs().contiguous().view(torch.int32).max()) if t.numel() else 0


def halves(t, arith):
    """(hi, lo, scale) of an fp32 tensor as float64 tensors in scaled units."""
    t = t.float()
    if arith == "f32":
        return t.double(), torch.zeros_like(t, dtype=F64), 1.0
    if arith == "bf16x3":
        hi = t.bfloat16().float()
        return hi.double(), (t - hi).bfloat16().double(), 1.0
    s = f16x2_scale(absmax_bits(t))
    ts = t * s
    hi = ts.half().float()
    return hi.double(), (ts - hi).half().double(), s


def split_ref(kind, c, d, arith, dtype=F64, families=("hh", "hl", "lh"), integer=False):
    """{"out", "abs", "pre"}: the contraction of the emulated halves (``dtype`` = float32 gives the fp32 evaluation the bar is
    checked against), the sum of the absolute values of every term, and the value before the activation."""
    assert kind == c.kind
    ah, al, sa = halves(d["a"], arith)
    bh, bl, sb = halves(d["b"], arith)
    pairs = {"hh": (ah, bh), "hl": (ah, bl), "lh": (al, bh)}
    v = sum(bilinear(c, pairs[f][0].to(dtype), pairs[f][1].to(dtype)) for f in families) / sa / sb
    tot = sum(bilinear(c, pairs[f][0].abs(), pairs[f][1].abs()) for f in ("hh", "hl", "lh")) / sa / sb
    for extra in (d["bias"].view(1, -1, 1, 1) if d["bias"] is not None else None, d["res"], d["dw0"]):
        if extra is not None:
            tot = tot + extra.double().abs()
    return {"out": epilogue(c, v, d, integer), "abs": tot}


def gamma(n):
    return n * U / (1 - n * U)


def additions(c, arith):
    """The additions on top of the products' own: bias, residual, LeakyReLU's product, accumulate, and one per K slice of the launch."""
    n = int(c.bias) + int(c.res) + int(c.act == "lrelu") + int(bool(c.acc))
    k = read_constants()
    if arith == "f32" or route(c, arith, k) is None:                 # no launch of a split route to count
        return n
    if c.kind in WGRAD:
        return n + wx3_slices(c, None, k)[0] + 16 + 1
    g = gather_geom(c)
    if route(c, arith, k) == ROUTE_NX2:
        return n + nx2_plan(c, g, k, c.ws != "none")[1]
    return n + x3_plan(c, g, k)["ksplit"]


def terms(c, arith):
    """n of the random bar; ``arith`` is the arithmetic the case's route really uses ("f32" off the split routes)."""
    K, _ = reduction(c)
    return (K if arith == "f32" else 3 * K) + additions(c, arith)


def bar(c, ref, arith):
    tol = gamma(terms(c, arith)) * ref["abs"] + ulp32(ref["out"])
    if c.act == "tanh":
        tol = tol + 1e-6 * ref["out"].abs() + 1e-6
    return tol


def violations(got, tol, want):
    err = (got.detach().cpu().double() - want).abs()
    bad = ~(err <= tol)
    return int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0


def exact_violations(got, want):
    """Elements that differ in value from the float64 reference (which is itself an fp32 number in integer mode).  Compared by value:
    every finite fp32 value but zero has one bit pattern, and -0 (LeakyReLU with slope 0 of a negative sum) counts as +0."""
    g = got.detach().cpu().double()
    return int((~(g == want)).sum())


# ----------------------------------------------------------------------------------------
# the launchers' decisions, restated
# ----------------------------------------------------------------------------------------
Geom = collections.namedtuple("Geom", "N C IH IW M OH OW SI SO reflect phases")          # C gathered channels, M output channels
Phase = collections.namedtuple("Phase", "py px gh gw taps")                                # taps: [(oy, ox)]


def geom_fwd(N, C, IH, IW, M, OH, OW, k, s, p, reflect):
    return Geom(N, C, IH, IW, M, OH, OW, s, 1, reflect, [Phase(0, 0, OH, OW, [(i - p, j - p) for i in range(k) for j in range(k)])])


def geom_transposed(N, C, IH, IW, M, OH, OW, k, s, p):
    ph = []
    for py in range(s):
        for px in range(s):
            taps = [((py + p - i) // s, (px + p - j) // s) for i in range(k) if (py + p - i) % s == 0 for j in range(k) if (px + p - j) % s == 0]
            ph.append(Phase(py, px, (OH - py + s - 1) // s if OH > py else 0, (OW - px + s - 1) // s if OW > px else 0, taps))
    return Geom(N, C, IH, IW, M, OH, OW, 1, s, 0, ph)


def gather_geom(c):
    N, C, H, W, M, k, _, s, p = abi_dims(c)
    OH, OW = out_hw(c)
    if c.kind == "conv2d_fwd":
        return geom_fwd(N, C, H, W, M, OH, OW, k, s, p, c.reflect)
    if c.kind == "conv2d_dgrad":
        return geom_transposed(N, M, OH, OW, C, H, W, k, s, p)
    if c.kind == "conv_transpose2d_fwd":
        return geom_transposed(N, C, H, W, M, OH, OW, k, s, p)
    return geom_fwd(N, M, OH, OW, C, H, W, k, s, p, 0)


def tap_group(T):
    if T <= 9:
        return T
    return next((cand for cand in range(9, 4, -1) if T % cand == 0), 8)


def spans(ph):
    ys, xs = [t[0] for t in ph.taps], [t[1] for t in ph.taps]
    return min(ys), min(xs), max(ys) - min(ys), max(xs) - min(xs)


def sp_lds(g, NI, staging, k):
    TH, best = 4 * NI, 0
    for ph in g.phases:
        _, _, sy, sx = spans(ph)
        PH, PW = (TH - 1) * g.SI + sy + 1, 31 * g.SI + sx + 1
        best = max(best, 4 * tap_group(len(ph.taps)) * 2048 + 4 * (2 * PH * PW) * 16 + (4096 * 4 if staging else 0) + 2048)
    return best


def sp_fits(g, NI, k):
    TH = 4 * NI
    for ph in g.phases:
        _, _, sy, sx = spans(ph)
        if 2 * ((TH - 1) * g.SI + sy + 1) * (31 * g.SI + sx + 1) > k["SP_ITEMS"] * k["SP_NPI"]:
            return False
    return sp_lds(g, NI, False, k) <= k["SP_LDS_MAX"]


def split_geom_from(g, narrow, k):
    if g.C < k["SP_MIN_C"] or g.SI not in (1, 2):
        return False
    for ph in g.phases:
        if not ph.taps or (not narrow and ph.gw < k["SP_MIN_W"]):
            return False
    return narrow or sp_fits(g, 2, k) or sp_fits(g, 1, k)


def sp_quad_ok(g, NI, x_aligned, k):
    if g.IW & 3 or not x_aligned:
        return False
    TH = 4 * NI
    for ph in g.phases:
        _, ox0, sy, sx = spans(ph)
        PH, PW = (TH - 1) * g.SI + sy + 1, 31 * g.SI + sx + 1
        qx0 = (-ox0) & 3
        cover = not g.reflect
        qs = qx0 - 4 if cover and qx0 else qx0
        nq = (PW - qs + 3) >> 2 if cover else (PW - qx0) >> 2
        ns = 0 if cover else PW - 4 * nq
        if nq < 1 or 2 * PH * nq > k["SP_QUAD_ITEMS"] or 2 * PH * ns > k["SP_QUAD_ITEMS"] or PH > 255 or PW > 240:
            return False
        if g.reflect and (ox0 + qx0 < 0 or ((ph.gw + 31) // 32 - 1) * 32 * g.SI + ox0 + qx0 + 4 * nq > g.IW):
            return False
    return True


def x3_plan(c, g, k):
    """What sp_launch decides for a case the wide split kernel takes."""
    NI = 2 if sp_fits(g, 2, k) else 1
    TH, MT = 4 * NI, k["SP_MT"]
    per_phase = [g.N * ((ph.gw + 31) // 32) * ((ph.gh + TH - 1) // TH) for ph in g.phases]
    mx, gy, nph = max(per_phase), (g.M + MT - 1) // MT, len(g.phases)
    blocks, ngroups, ksplit = mx * gy * nph, (g.C + 15) // 16, 1
    if c.act is None and blocks < k["SP_SPLIT_BELOW"]:
        ksplit = max(1, min(k["SP_GRID"] // blocks, ngroups // k["SP_GROUPS_PER_SLICE"]))
    if c.nosplit:
        ksplit = 1
    staging = sp_lds(g, NI, True, k) <= k["SP_LDS_MAX"]
    nbx = min(max(1, k["SP_GRID"] // (gy * nph * ksplit)), mx)
    wide = (staging and g.SO == 1 and nph == 1 and g.OW % 4 == 0 and "y" not in c.align and ksplit == 1
            and all(ph.gw % 4 == 0 and ph.px % 4 == 0 for ph in g.phases))
    return {"NI": NI, "TH": TH, "ksplit": ksplit, "staging": staging, "nbx": nbx, "wide": wide, "quad": sp_quad_ok(g, NI, "x" not in c.align, k),
            "tiles": per_phase, "gy": gy, "ngroups": ngroups, "blocks": blocks}


def nx2_plan(c, g, k, have_ws=True):
    """(eligible, ksplit) of igemm_nm_x2.hip's nx2_plan for the narrow geometry g."""
    if g.M < k["NX_MIN_M"] or g.C & 15:
        return False, 0
    chunks = []
    for ph in g.phases:
        if not ph.taps or ((g.C >> 4) * len(ph.taps)) % k["NX_KS"]:
            return False, 0
        chunks.append((g.C >> 4) * len(ph.taps) // k["NX_KS"])
    maxpix = max(g.N * ph.gh * ph.gw for ph in g.phases)
    if maxpix == 0:
        return False, 0
    blocks = ((maxpix + k["NX_NT"] - 1) // k["NX_NT"]) * ((g.M + k["NX_MT"] - 1) // k["NX_MT"]) * len(g.phases)
    ksplit = 1
    if have_ws and not c.nosplit and blocks < k["NX_SPLIT_BELOW"]:
        ksplit = max(1, min((k["NX_TARGET"] + blocks - 1) // blocks, k["NX_MAX_SLICES"], min(chunks) // k["NX_MIN_CHUNKS"]))
    return True, ksplit


def wx3_form(N, C, IH, IW, M, OH, OW, kk, s, p, reflect, k):
    """launch_wgrad_x3 / launch_wgrad_x3_row: "roll", "row" or None."""
    tile = bool(C % k["WX_C"] or M % k["WX_M"] or OW % k["WX_OW"] or OH % k["WX_OH"])
    if (s == 1 and kk == 7) or s == 2:
        if tile or IW % k["WX_IW"]:
            return None
        if s == 1 and kk == 7 and p == 3 and OH == IH and OW == IW:
            return None if reflect and (IH <= p or IW < k["WX_REFLECT_MIN_W"]) else "row"
        return "row" if s == 2 and p == 1 and not reflect and IH == 2 * OH and IW == 2 * OW and kk in (3, 4) else None
    if s != 1 or kk != 3 or p != 1 or reflect or OH != IH or OW != IW or tile:
        return None
    return "roll"


def wgrad_args(c):
    """The launcher's view (N, C, IH, IW, M, OH, OW) of a weight-gradient case: the transposed one swaps x and dy."""
    OH, OW = out_hw(c)
    return (c.N, c.C, c.H, c.W, c.M, OH, OW) if c.kind == "conv2d_wgrad" else (c.N, c.M, OH, OW, c.C, c.H, c.W)


def wx3_slices(c, form, k):
    """(slices, tiles per slice, tiles) of a route-15 launch; ``form`` None: looked up."""
    N, C, IH, IW, M, OH, OW = wgrad_args(c)
    form = form or wx3_form(N, C, IH, IW, M, OH, OW, c.k, c.s, c.p, c.reflect, k)
    ntiles, blocks = N * (OH // 2) * (OW // 32), (C // 64) * (M // 64) * (1 if form == "roll" else c.k)
    slices = max(1, k["WX_GRID"] // blocks)
    if slices > ntiles // 4:
        slices = max(ntiles // 4, 1)
    per = (ntiles + slices - 1) // slices
    return (ntiles + per - 1) // per, per, ntiles


def route(c, arith, k=None):
    """The route the dispatch takes: ROUTE_X3, ROUTE_NX2, ROUTE_WX3 or None (an exact-f32 kernel)."""
    k = k or read_constants()
    if c.kind in WGRAD:
        N, C, IH, IW, M, OH, OW = wgrad_args(c)
        if OW < k["WX_MIN_W"]:
            return None
        return ROUTE_WX3 if wx3_form(N, C, IH, IW, M, OH, OW, c.k, c.s, c.p, c.reflect, k) else None
    g = gather_geom(c)
    if split_geom_from(g, False, k):
        return ROUTE_X3
    if arith == "f16x2" and split_geom_from(g, True, k) and any(ph.gw < k["SP_MIN_W"] for ph in g.phases) and nx2_plan(c, g, k)[0]:
        return ROUTE_NX2
    return None


def forms(kind, c, alignment=None, k=None):
    """The forms of the launchers and kernels a case reaches (both arithmetics take the same decisions, except that route 8 exists at
    f16x2 only).  ``alignment`` overrides the case's own."""
    assert kind == c.kind
    k = k or read_constants()
    if alignment is not None:
        c = c._replace(align=alignment)
    out = set()
    if c.kind in WGRAD:
        r = route(c, "f16x2", k)
        if r is None:
            return {"wx: left to the f32 weight gradients"}
        N, C, IH, IW, M, OH, OW = wgrad_args(c)
        form = wx3_form(N, C, IH, IW, M, OH, OW, c.k, c.s, c.p, c.reflect, k)
        slices, per, ntiles = wx3_slices(c, form, k)
        out |= {"wx: %s kernel" % ("3x3 rolling" if form == "roll" else "%dx%d stride %d row" % (c.k, c.k, c.s)),
                "wx: %s tile column%s" % ({1: "one", 2: "two"}.get(OW // 32, "three or more"), "" if OW == 32 else "s"),
                "wx: two-pass reduction" if c.ws == "exact" else "wx: atomics", "wx: accumulate" if c.acc else "wx: overwrite"}
        out |= {"wx: one tile row" if OH == 2 else "wx: several tile rows"}
        if C > 64:
            out.add("wx: two input slabs")
        if M > 64:
            out.add("wx: two output slabs")
        if N % 2 and N > 1:
            out.add("wx: odd batch")
        if slices > 1:
            out.add("wx: several slices")
        if ntiles % per:
            out.add("wx: ragged last slice")
        if c.ws == "short":
            out.add("wx: workspace one float short")
        if c.reflect:
            out.add("wx: reflection" + (", both borders in one tile" if OW == 32 else ""))
        if c.kind == "conv_transpose2d_wgrad":
            out.add("wx: transposed, operands swapped")
        return out
    g = gather_geom(c)
    r = route(c, "f16x2", k)
    if r is None:
        return {"gather: left to the f32 kernels"}
    if r == ROUTE_NX2:
        ok, ksplit = nx2_plan(c, g, k, c.ws != "none")
        chunks = [(g.C >> 4) * len(ph.taps) // k["NX_KS"] for ph in g.phases]
        pix = [g.N * ph.gh * ph.gw for ph in g.phases]
        out |= {"nx: %d slice%s" % (ksplit, "" if ksplit == 1 else "s") if ksplit < 3 else "nx: three or more slices",
                "nx: one phase" if len(g.phases) == 1 else "nx: several phases"}
        if ksplit > 1:
            out.add("nx: reduce kernel" + (" with bias, activation, residual" if c.bias and c.act and c.res else ""))
            cps = (max(chunks) + ksplit - 1) // ksplit
            if any((ksplit - 1) * cps >= n for n in chunks):
                out.add("nx: an empty slice writes zeros")
            if c.ws == "short":
                out.discard("nx: reduce kernel")
                out.add("nx: workspace one float short, unsplit")
        elif c.ws == "none" and nx2_plan(c, g, k, True)[1] > 1:
            out.add("nx: no workspace, unsplit")
        elif c.nosplit and nx2_plan(c._replace(nosplit=False), g, k, True)[1] > 1:
            out.add("nx: split-K switched off")
        if g.M % k["NX_MT"]:
            out.add("nx: half-empty row block")
        if g.M > k["NX_MT"]:
            out.add("nx: several row blocks")
        if any(n % k["NX_NT"] for n in pix):
            out.add("nx: pixel tail")
        if max(pix) > k["NX_NT"]:
            out.add("nx: several pixel blocks")
        if max(pix) == 1:
            out.add("nx: a single pixel")
        if g.reflect:
            out.add("nx: reflection")
        return out
    pl = x3_plan(c, g, k)
    TH, NI, MT = pl["TH"], pl["NI"], k["SP_MT"]
    out |= {"x3: %d-row tiles" % TH, "x3: 4-pixel patch items" if pl["quad"] else "x3: single-pixel patch items",
            "x3: 16-byte stores" if pl["wide"] else "x3: dword stores", "x3: tap group of %d" % max(tap_group(len(ph.taps)) for ph in g.phases),
            "x3: input stride %d" % g.SI, "x3: %d phase%s" % (len(g.phases), "" if len(g.phases) == 1 else "s")}
    if not pl["staging"]:
        out.add("x3: no output staging")
    if pl["wide"] and TH == 4:
        out.add("x3: 16-byte stores from 4-row tiles")
    if len({len(ph.taps) for ph in g.phases}) > 1:
        out.add("x3: phases with different tap counts")
    if len({(ph.gh, ph.gw) for ph in g.phases}) > 1:
        out.add("x3: phases of different sizes")
    if max(len(ph.taps) for ph in g.phases) > tap_group(max(len(ph.taps) for ph in g.phases)):
        out.add("x3: several tap groups")
    if g.C % 16:
        out.add("x3: partial channel group")
    if g.C >= 32:
        out.add("x3: several channel groups")
    if g.reflect:
        out.add("x3: reflection, " + ("every piece inside" if pl["quad"] else "mirrored piece: single pixels"))
        if g.IH == c.p + 1:
            out.add("x3: reflection, H = pad + 1")
    # tiles and waves: interior (straight-line) against predicated epilogues
    for ph, ntile in zip(g.phases, pl["tiles"]):
        tx_n, ty_n = (ph.gw + 31) // 32, (ph.gh + TH - 1) // TH
        if ntile > pl["nbx"]:
            out.add("x3: a block walks several tiles")
            last = ntile - 1                                         # the last tile of the walk is some block's second
            if (last % tx_n) * 32 + 32 > ph.gw or ((last // tx_n) % ty_n) * TH + TH > ph.gh:
                out.add("x3: a tail tile as a block's second")
        for m0 in range(0, g.M, MT):
            full_m = m0 + MT <= g.M
            for ty in range(ty_n):
                for tx in range(tx_n):
                    for wn in range(4):
                        rows_in = ty * TH + wn * NI + NI <= ph.gh
                        cols_in = tx * 32 + 32 <= ph.gw
                        if ty * TH + wn * NI >= ph.gh:
                            out.add("x3: a wave with no row")
                        elif pl["wide"]:
                            out.add("x3: interior epilogue" if full_m and rows_in and cols_in else "x3: predicated 16-byte epilogue")
                        else:
                            out.add("x3: straight-line dword epilogue" if full_m else "x3: predicated dword epilogue")
                        if not cols_in and tx * 32 + 32 - ph.gw >= 28:
                            out.add("x3: a 4-column tail tile")
            if not full_m:
                out.add("x3: M tail" + (" below one block" if g.M < MT else ""))
    if pl["ksplit"] > 1:
        gps = (pl["ngroups"] + pl["ksplit"] - 1) // pl["ksplit"]
        out |= {"x3: split-K, %s slices" % {2: "two", 3: "three"}.get(pl["ksplit"], "four or more"),
                "x3: split-K, uneven slices" if pl["ngroups"] % pl["ksplit"] else "x3: split-K, even slices"}
        if (pl["ksplit"] - 1) * gps >= pl["ngroups"]:
            out.add("x3: split-K, an empty slice")
        if c.bias:
            out.add("x3: split-K, bias by slice 0")
        if c.res:
            out.add("x3: split-K, residual by slice 0")
    elif c.nosplit and x3_plan(c._replace(nosplit=False), g, k)["ksplit"] > 1:
        out.add("x3: split-K switched off by the caller")
    elif c.act and x3_plan(c._replace(act=None), g, k)["ksplit"] > 1:
        out.add("x3: split-K switched off by the activation")
    for a, what in (("x", "x"), ("y", "y"), ("r", "residual")):
        if a in c.align:
            out.add("x3: %s 4 bytes past a 16-byte boundary" % what)
    if c.res and pl["wide"] and "r" in c.align:
        out.add("x3: 16-byte residual loads at a misaligned address")
    if c.act or c.bias or c.res:
        out.add("x3: epilogue %s%s%s" % (c.act or "none", " + bias" if c.bias else "", " + residual" if c.res else ""))
    if c.act == "lrelu" and c.slope == 0.0:
        out.add("x3: LeakyReLU with slope 0")
    return out


def covered_forms(tables=None, k=None):
    got = set()
    for c in sum((tables or TABLES).values(), []):
        got |= forms(c.kind, c, k=k)
    return got


#: forms the kernels hold that no admissible call reaches, and why
UNREACHABLE = {
    "x3: 16-byte stores without output staging": "wide_ok requires the staging buffer; the 3x3 and 4x4 stride-2 layers (4-row tiles, a 70-pixel wide patch) "
                                                 "have no room for it and store dwords, whatever their alignment",
    "x3: no output staging at stride 1": "over every square kernel up to the 64-tap limit the largest stride-1 footprint that passes sp_fits is 8x8 "
                                         "with 8-row tiles: 158848 bytes with staging against SP_LDS_MAX = 159744 (test_every_form_is_reached searches them all)",
    "x3: 8 consumer waves": "SP_NCW8 is 0: sp_launch_wide_block returns before it looks at the shape; the form is compiled out",
}
_EPI = {"x3: epilogue %s%s%s" % (a, b, r) for a in ("none", "relu", "lrelu", "tanh") for b in ("", " + bias") for r in ("", " + residual")} - {"x3: epilogue none"}
FORMS = _EPI | {
    "gather: left to the f32 kernels", "wx: left to the f32 weight gradients",
    "x3: 8-row tiles", "x3: 4-row tiles", "x3: 4-pixel patch items", "x3: single-pixel patch items", "x3: 16-byte stores", "x3: dword stores",
    "x3: no output staging", "x3: 16-byte stores from 4-row tiles", "x3: tap group of 9", "x3: tap group of 5", "x3: tap group of 7", "x3: tap group of 8", "x3: tap group of 4", "x3: several tap groups",
    "x3: input stride 1", "x3: input stride 2", "x3: 1 phase", "x3: 4 phases", "x3: phases with different tap counts", "x3: phases of different sizes",
    "x3: partial channel group", "x3: several channel groups",
    "x3: reflection, every piece inside", "x3: reflection, mirrored piece: single pixels", "x3: reflection, H = pad + 1",
    "x3: a block walks several tiles", "x3: a tail tile as a block's second", "x3: a wave with no row", "x3: interior epilogue",
    "x3: predicated 16-byte epilogue", "x3: straight-line dword epilogue", "x3: predicated dword epilogue", "x3: a 4-column tail tile",
    "x3: M tail", "x3: M tail below one block",
    "x3: split-K, two slices", "x3: split-K, three slices", "x3: split-K, four or more slices", "x3: split-K, uneven slices", "x3: split-K, even slices",
    "x3: split-K, an empty slice", "x3: split-K, bias by slice 0", "x3: split-K, residual by slice 0", "x3: split-K switched off by the caller",
    "x3: split-K switched off by the activation",
    "x3: x 4 bytes past a 16-byte boundary", "x3: y 4 bytes past a 16-byte boundary", "x3: residual 4 bytes past a 16-byte boundary",
    "x3: 16-byte residual loads at a misaligned address", "x3: LeakyReLU with slope 0",
    "nx: 1 slice", "nx: 2 slices", "nx: three or more slices", "nx: one phase", "nx: several phases", "nx: reduce kernel",
    "nx: reduce kernel with bias, activation, residual", "nx: an empty slice writes zeros", "nx: workspace one float short, unsplit",
    "nx: no workspace, unsplit", "nx: split-K switched off", "nx: half-empty row block", "nx: several row blocks", "nx: pixel tail",
    "nx: several pixel blocks", "nx: a single pixel", "nx: reflection",
    "wx: 3x3 rolling kernel", "wx: 7x7 stride 1 row kernel", "wx: 4x4 stride 2 row kernel", "wx: 3x3 stride 2 row kernel",
    "wx: one tile column", "wx: two tile columns", "wx: three or more tile columns", "wx: one tile row", "wx: several tile rows",
    "wx: two-pass reduction", "wx: atomics", "wx: accumulate", "wx: overwrite", "wx: two input slabs", "wx: two output slabs", "wx: odd batch",
    "wx: several slices", "wx: ragged last slice", "wx: workspace one float short", "wx: reflection", "wx: reflection, both borders in one tile",
    "wx: transposed, operands swapped",
}
#: (case, route at bf16x3, route at f16x2) of the shapes that sit just outside a predicate
LEAVES = {"W23": (None, None), "C15": (None, None), "tfwd_k3_outpad0_W24": (None, None), "nx_M63": (None, None), "nx_C24": (None, None),
          "nx_C48_k3_chunks": (None, None), "wx_out_OW48": (None, None), "wx_out_OH3": (None, None), "wx_out_C96": (None, None),
          "wx_out_M32": (None, None), "wx_out_IW66_s2": (None, None), "wx_out_k5": (None, None), "wx_out_t_outpad0": (None, None)}


# ----------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------
def test_constants_match_the_source():
    k = read_constants()
    assert k == {"SP_MIN_W": 24, "SP_SPLIT_BELOW": 128, "SP_NCW8": 0, "SP_MT": 64, "SP_NPI": 6, "SP_LDS_MAX": 156 * 1024, "SP_ITEMS": 256,
                 "SP_GRID": 256, "SP_GROUPS_PER_SLICE": 2, "SP_MIN_C": 16, "SP_QUAD_ITEMS": 512, "NX_MT": 128, "NX_NT": 64, "NX_KS": 4,
                 "NX_MIN_M": 64, "NX_SPLIT_BELOW": 384, "NX_TARGET": 512, "NX_MAX_SLICES": 8, "NX_MIN_CHUNKS": 8, "WX_C": 64, "WX_M": 64,
                 "WX_OW": 32, "WX_OH": 2, "WX_IW": 4, "WX_GRID": 256, "WX_MIN_W": 24, "WX_REFLECT_MIN_W": 8, "MAX_TAPS": 64, "MAX_PAD": 60}, k
    assert f16x2_scale(f32_bits(8.0)) == 2.0 ** 11 and f16x2_scale(f32_bits(4.0)) == 2.0 ** 12 and f16x2_scale(f32_bits(1.5e-5)) == 2.0 ** 31
    for v in (0.0, 2.0 ** -112, float("inf"), float("nan")):
        assert f16x2_scale(f32_bits(v)) == 1.0, v
    assert f16x2_scale(f32_bits(2.0 ** -111)) == 2.0 ** 125
    for v in (1.0, 3.7, 65504.0, 1e-20, 1e30):                            # the maximum lands in [2^14, 2^15)
        assert 2.0 ** 14 <= v * f16x2_scale(f32_bits(v)) < 2.0 ** 15, v


def _search_no_staging(k):
    """The largest sp_lds with staging among the square kernels that keep it, and the (kind, k, stride, pad, NI) that drop it."""
    worst, hits = 0, []
    for kk in range(1, 9):
        for s in (1, 2):
            for p in range(0, kk):
                for kind in GATHER:
                    c = case("probe", kind, (1, 16, 40, 40, 64, kk, s, p))
                    if min(out_hw(c)) < 1 or (kind.startswith("conv_transpose") and s == 1 and p > kk - 1):
                        continue
                    g = gather_geom(c)
                    if any(not ph.taps for ph in g.phases):
                        continue
                    for NI in (2, 1):
                        if sp_fits(g, NI, k):
                            with_staging = sp_lds(g, NI, True, k)
                            if with_staging > k["SP_LDS_MAX"]:
                                hits.append((kind, kk, s, p, NI))
                            else:
                                worst = max(worst, with_staging)
                            break
    return worst, hits


def test_every_form_is_reached():
    k = read_constants()
    got = covered_forms()
    assert got == FORMS, (sorted(FORMS - got), sorted(got - FORMS))
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in ALL_CASES}
    # the plainest case is nothing but full interior tiles
    assert forms(FWD, by["plain"]) == {"x3: 8-row tiles", "x3: 4-pixel patch items", "x3: 16-byte stores", "x3: tap group of 9", "x3: input stride 1",
                                       "x3: 1 phase", "x3: interior epilogue"}
    assert "x3: a 4-column tail tile" in forms(FWD, by["W36"]) and "x3: 16-byte stores" in forms(FWD, by["W36"])
    assert {"x3: dword stores", "x3: single-pixel patch items"} <= forms(FWD, by["W34"])
    assert "x3: 4-row tiles" in forms(FWD, by["s2_k4"]) and "x3: 4 phases" in forms(DGR, by["dgrad_s2_k4"])
    assert "x3: phases with different tap counts" in forms(TFWD, by["tfwd_k3_outpad1"])
    assert "x3: tap group of 8" in forms(FWD, by["k8_64taps"]) and len(gather_geom(by["k8_64taps"]).phases[0].taps) == k["MAX_TAPS"]
    assert "x3: 16-byte residual loads at a misaligned address" in forms(FWD, by["align_r"])
    assert "x3: split-K switched off by the activation" in forms(FWD, by["act_switches_splitk_off"])
    assert "nx: an empty slice writes zeros" in forms(DGR, by["nx_dgrad_s2_k3_empty_slice"])
    assert "wx: reflection, both borders in one tile" in forms(WGR, by["wx_row_k7_reflect_W32"])
    # the misaligned variants of one shape take other forms than the aligned call
    assert "x3: single-pixel patch items" in forms(FWD, by["plain"], "x") and "x3: dword stores" in forms(FWD, by["plain"], "y")
    # the shapes just outside a predicate leave their route, in both arithmetics
    for name, want in LEAVES.items():
        assert (route(by[name], "bf16x3"), route(by[name], "f16x2")) == want, name
    assert all(route(c, "bf16x3") == ROUTE_X3 and route(c, "f16x2") == ROUTE_X3 for c in WIDE_CASES if c.name not in LEAVES)
    assert all(route(c, "bf16x3") is None and route(c, "f16x2") == ROUTE_NX2 for c in NARROW_CASES if c.name not in LEAVES)
    assert all(route(c, "bf16x3") == ROUTE_WX3 and route(c, "f16x2") == ROUTE_WX3 for c in WGRAD_CASES if c.name not in LEAVES)
    # the exact bar's condition, and a float64 reference of at most ~1e9 multiply-adds
    for c in ALL_CASES:
        K, P = reduction(c)
        assert P * K + 100 < 2 ** 24, c.name
        assert K * math.prod(shapes(c)[2]) < 1e9, c.name
    # a constant that moves takes forms away: the tables would have to follow
    for change in ({"SP_MIN_W": 32}, {"SP_MT": 128}, {"SP_NPI": 3}, {"SP_LDS_MAX": 96 * 1024}, {"SP_LDS_MAX": 176 * 1024}, {"SP_GROUPS_PER_SLICE": 4},
                   {"NX_MT": 64}, {"NX_KS": 8}, {"NX_SPLIT_BELOW": 1}, {"NX_MAX_SLICES": 2}, {"NX_MIN_CHUNKS": 64}, {"WX_OW": 16}):
        assert covered_forms(k=dict(k, **change)) != FORMS, change
    # ... or takes a boundary case into the route it must leave (IW % 4 of the row kernel is implied by OW % 32 on every shape it takes)
    for change, name in (({"SP_MIN_W": 16}, "W23"), ({"SP_MIN_W": 16}, "tfwd_k3_outpad0_W24"), ({"SP_MIN_C": 8}, "C15"), ({"NX_MIN_M": 16}, "nx_M63"),
                         ({"WX_C": 32}, "wx_out_C96"), ({"WX_OH": 1}, "wx_out_OH3"), ({"WX_OW": 16}, "wx_out_OW48")):
        assert route(by[name], "f16x2", dict(k, **change)) is not None, (change, name)
    # a case that is the only one of its form takes the form with it
    sole = {}
    for c in ALL_CASES:
        for f in forms(c.kind, c):
            sole.setdefault(f, []).append(c.name)
    carriers = sorted({v[0] for v in sole.values() if len(v) == 1})
    assert len(carriers) >= 15, carriers
    for drop in carriers:
        rest = {t: [c for c in cs if c.name != drop] for t, cs in TABLES.items()}
        assert covered_forms(rest) != FORMS, drop
    # the forms nothing reaches
    assert len(UNREACHABLE) == 3 and not (set(UNREACHABLE) & FORMS)
    assert k["SP_NCW8"] == 0
    worst, hits = _search_no_staging(k)
    assert worst == 158848 <= k["SP_LDS_MAX"] and hits and all(s == 2 and kk in (3, 4) and NI == 1 for _, kk, s, _, NI in hits), (worst, hits)
    assert all("x3: 16-byte stores" not in forms(c.kind, c) for c in WIDE_CASES if "x3: no output staging" in forms(c.kind, c))


GRADIENT_CASES = [c for c in ALL_CASES if c.kind not in ("conv2d_fwd", "conv_transpose2d_fwd")]


def test_gradient_cases_cover_every_kind():
    assert {c.kind for c in GRADIENT_CASES} == {DGR, TDGR, WGR, TWGR}
    assert {(c.kind, c.reflect) for c in GRADIENT_CASES} >= {(DGR, 1), (WGR, 1)} and any(c.out_pad for c in GRADIENT_CASES if c.kind == TDGR)


@pytest.mark.parametrize("c", GRADIENT_CASES, ids=ident)
def test_gradient_restatements_equal_autograd(c):
    """The closed forms of the four gradient kinds, every case of them, against torch autograd through the float64 forward."""
    d = build(c._replace(res=False, acc=0), "random")
    a, b = d["a"].double(), d["b"].double()
    so = shapes(c)[2]
    fwd_case = c._replace(kind="conv2d_fwd" if c.kind.startswith("conv2d") else "conv_transpose2d_fwd", res=False, acc=0, bias=False, act=None)
    leaf = torch.zeros(so, dtype=F64, requires_grad=True)
    if c.kind in WGRAD:
        bilinear(fwd_case, a, leaf).backward(b)
    elif c.reflect:                                                   # the gradient with respect to the padded input
        F.conv2d(leaf, b, stride=c.s).backward(a)
    else:
        bilinear(fwd_case, leaf, b).backward(a)
    got, want = bilinear(c, a, b), leaf.grad
    assert got.shape == want.shape and float((got - want).abs().max()) <= PIN * max(1.0, float(want.abs().max())), c.name


@pytest.mark.parametrize("c", ALL_CASES, ids=ident)
def test_restatements_and_bars(c):
    """split_ref against conv_ref (bit equality on integers, the representation bound on random data); the fp32 evaluation of
    split_ref meets the random bar in both arithmetics; output shapes; LeakyReLU's integer reference is an fp32 number."""
    for arith in ("bf16x3", "f16x2"):
        if "integer" in modes(c):
            d = build(c, "integer")
            ref = conv_ref(c.kind, c, d, integer=True)
            assert ref.shape == shapes(c)[2]
            assert torch.equal(split_ref(c.kind, c, d, arith, integer=True)["out"], ref), (c.name, arith)
            assert torch.equal(ref.float().double(), ref), c.name
            assert all(float(halves(d[n], arith)[1].abs().max()) == 0.0 for n in "ab")
        d = build(c, "random")
        ref, sp, sp32 = conv_ref(c.kind, c, d), split_ref(c.kind, c, d, arith), split_ref(c.kind, c, d, arith, dtype=F32)
        plain = split_ref(c.kind, c, d, "f32")
        n, worst = violations(sp["out"], REP_BOUND[arith] * plain["abs"], ref)
        assert n == 0, (c.name, arith, n, worst)
        n, worst = violations(sp32["out"], bar(c, sp, arith), sp["out"])
        assert n == 0, (c.name, arith, n, worst)
        assert rel_l2(sp["out"], ref) < AGGREGATE[arith] / 4, (c.name, arith)
    d = build(c, "random")
    n, worst = violations(split_ref(c.kind, c, d, "f32", dtype=F32)["out"], bar(c, plain, "f32"), plain["out"])
    assert n == 0 and torch.equal(plain["out"], ref), (c.name, n, worst)


def test_the_random_bar_is_not_vacuous():
    """Without the hi*lo family the smallest-K cases fall outside the bar; so does one wrong tap of one output."""
    small = [c for c in ALL_CASES if c.kind in GATHER and reduction(c)[0] <= 16 * 9 and c.act != "tanh"]
    assert len(small) >= 10
    for c in small:
        d = build(c, "random")
        for arith in ("bf16x3", "f16x2"):
            sp = split_ref(c.kind, c, d, arith)
            n, worst = violations(split_ref(c.kind, c, d, arith, families=("hh", "lh"))["out"], bar(c, sp, arith), sp["out"])
            assert n > 0 and worst > 2, (c.name, arith, n, worst)
            assert violations(sp["out"] + 1e-3 * sp["abs"], bar(c, sp, arith), sp["out"])[0] == sp["out"].numel()


# ----------------------------------------------------------------------------------------
# host probes: the form map's route prediction against the library's own dispatch code, no device needed
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import faoctasr
    return faoctasr._lib.load()


def probe_args(c):
    return (KIND_ID[c.kind],) + abi_dims(c) + (c.reflect if c.kind in ("conv2d_fwd", "conv2d_wgrad") else 0, c.out_pad)


@pytest.mark.parametrize("c", ALL_CASES, ids=ident)
def test_route_prediction_matches_the_library(lib, c):
    k = read_constants()
    r = route(c, "f16x2")
    needs = lib.faoctasr_conv_needs_scales(*probe_args(c))
    if c.kind in WGRAD:
        assert needs == (3 if r == ROUTE_WX3 else 0), (c.name, needs, r)
        return
    assert needs == (1 if r in (ROUTE_X3, ROUTE_NX2) else 0), (c.name, needs, r)
    ws = lib.faoctasr_conv_gather_workspace_floats(*probe_args(c))
    g = gather_geom(c)
    ksplit = nx2_plan(c._replace(nosplit=False), g, k)[1] if r == ROUTE_NX2 else 1
    assert ws == (ksplit * g.N * g.M * g.OH * g.OW if ksplit > 1 else 0), (c.name, ws, ksplit)
    N, C, H, W, M, KH, KW, s, p = abi_dims(c)
    floats = lib.faoctasr_conv_wpack_floats(KIND_ID[c.kind], C, M, KH, KW, s, p, 3)
    if r is not None:
        plane = sum(((g.C + 15) // 16) * len(ph.taps) * 16 * ((g.M + 63) // 64 * 64) for ph in g.phases)
        assert floats >= ((plane + 7) & ~7) + 512, (c.name, floats, plane)


def test_bad_arguments_are_refused_with_a_message(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    EINVAL, EUNSUPPORTED = -1, -2

    def fwd(x=p, N=1, C=16, H=32, W=32, M=8, k=3, s=1, pad=1, reflect=0, precision=2):
        return lib.faoctasr_conv2d_fwd(x, p, None, p, N, C, H, W, M, k, k, s, pad, reflect, 0, 0.2, None, 0, precision, None)
    assert fwd(k=9, pad=4) == EUNSUPPORTED and b"kernel 9x9 too large" in lib.faoctasr_last_error()
    assert fwd(k=3, pad=61) == EUNSUPPORTED and b"pad 61 too large" in lib.faoctasr_last_error()
    assert fwd(H=3, pad=3, k=7, reflect=1) == EINVAL and b"reflect pad 3 >= input size" in lib.faoctasr_last_error()
    assert fwd(precision=4) == EINVAL and b"unknown conv precision 4" in lib.faoctasr_last_error()
    assert fwd(x=None) == EINVAL and b"conv2d_fwd: null pointer" in lib.faoctasr_last_error()
    assert fwd(C=0) == EINVAL and b"conv2d_fwd: bad shape" in lib.faoctasr_last_error()
    assert lib.faoctasr_conv2d_wgrad(p, p, p, 1, 64, 2, 32, 64, 3, 3, 1, 1, 0, 0, 3, None) == EINVAL and b"needs both absmax slots" in lib.faoctasr_last_error()
    assert lib.faoctasr_conv2d_wgrad(p, p, p, 1, 64, 2, 32, 64, 3, 3, 1, 1, 0, 0, 7, None) == EINVAL and b"unknown conv precision 7" in lib.faoctasr_last_error()
    assert lib.faoctasr_conv_transpose2d_fwd(p, p, None, p, 1, 16, 8, 24, 64, 9, 9, 2, 1, 0, 0, 0.2, None, 0, 2, None) == EUNSUPPORTED
    assert b"kernel 9x9 too large" in lib.faoctasr_last_error()
    assert lib.faoctasr_conv_needs_scales(0, 1, 16, 8, 32, 64, 9, 9, 1, 4, 0, 0) == EUNSUPPORTED
    assert lib.faoctasr_conv_needs_scales(6, 1, 16, 8, 32, 64, 3, 3, 1, 1, 0, 0) == EINVAL and b"unknown kind 6" in lib.faoctasr_last_error()
