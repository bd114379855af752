"""The pointwise kernels of csrc/pointwise.hip without a GPU: activations, cat + activation, axpby / add / fill, the per-channel
sum, the reflection-pad gradient fold, the Haar butterflies (either band absent), the discriminator front ends, the frequency
split's mixing, the three losses, mean_mix and AdamW, each restated in plain torch and parametrised by dtype.  The float64
restatement is pinned here to torch (``F.*``, autograd through ``F.pad(mode="reflect")``, ``torch.optim.AdamW``) and to
oracle.octa_oracle at 1e-12; tests/test_gpu_pointwise.py measures every kernel against it and takes its case tables, input
builders and bars from this file.  bn_eval_*, absmax_bits and prep_crop_resize are covered elsewhere.

Scalars (slope, alpha, beta, the loss scale weight / n, the mean_mix weights) cross the C ABI as ``float``: the restatement rounds
them to fp32 first, as the call does, so that an "exact" operator can be asked for the float64 result rounded to fp32.

The dispatch of pointwise.hip -- block size, ``grid_for(n, per_block, cap)`` of every launch site, loss_fwd's 2048 / 1024,
channel_sum's 1024 / 4096 -- is stated in ``LAUNCH`` and read back from the source; ``forms(op, case)`` names the branches a case
reaches, and test_every_form_is_reached fails when a case is removed or a constant changes so that a branch is no longer run.

The bars (tests/test_gpu_pointwise.py applies the same ones; none is tuned on the kernels), u = 2^-24:
  exact     ReLU, LeakyReLU, cat, fill, -|x|, and every backward that is a product of two fp32 values: the float64 result rounded
            to fp32, to the bit.
  short     |got - ref64| <= k u sum |terms| + 1 ulp, k = roundings of the kernel's expression (a contracted multiply-add
            rounds less):
              axpby      alpha a + beta b                         2 products + 1 add                  k = 3
              axpby bwd  alpha dy + 0 dy                          1 product (+ 0)                     k = 2
              Haar       (a +- b +- c +- d) * 0.5                 3 adds, the scale is exact          k = 3
              dfront 1   (a +- b +- c +- d) * 0.25 + 0.5          3 adds + 1                          k = 4
              reflect    at most 9 terms added to 0               8 adds                              k = 8
              freq hf    (|x - lo| + x) * 0.5                     1 difference + 1 add                k = 2
              MSE grad   (g scale) * (2 (a - b))                  g scale, a - b, the product         k = 3
              L1 / BCE-target grad   (g scale) * (sgn | -a)       g scale, the product                k = 2
              mean_mix bwd   g w / L                              1 product + 1 quotient              k = 2
              AdamW m    b1 m + (1 - b1) (g s)                    g s, 1 - b1, 2 products, 1 add      k = 5 per step
              AdamW v    b2 v + (1 - b2) (g s) (g s)              g s, 1 - b2, 3 products, 1 add      k = 6 per step
  library   tanh, the BCE value terms and the sigmoid of the BCE gradient go through the device math library, whose error nobody
            here has measured: the bars of tests/test_gpu_ops.py -- rtol 1e-6 atol 1e-6 forward, rtol 1e-5 atol 1e-6 backward
            (test_pointwise), rtol 1e-4 atol 1e-7 (test_losses_head_adamw).  The POINTWISE_ERR lines record what is observed.
  sums      channel sums, loss values, mean_mix: |got - ref64| <= GAMMA_SUM sum |terms| + 2 ulp with test_norm_cpu.GAMMA_SUM =
            128 u; ``depth(op, case)`` states the number of additions an addend passes through (block_sum_256 = 9) and
            test_every_form_is_reached checks it stays below 112, leaving 16 u for the roundings inside a term.  The BCE value
            adds rtol 1e-4 sum |log1p terms| + 1e-7 for the library.
  AdamW     p against float64: rtol 1e-6 atol 1e-7, as test_losses_head_adamw; adamw_step_dev against adamw_step: bitwise."""
import math
import os
import re
import struct

import pytest
import torch
import torch.nn.functional as F

from test_norm_cpu import CSRC, GAMMA_SUM, KINK, PIN, SPIKE, rel_l2, sum_violations, ulp32

U = 2.0 ** -24
SLOPE = 0.2
BLOCK = 256
#: kernel -> (elements per block, cap on the blocks) of its launch site's grid_for(n, per_block, cap); cap defaults to 4096
LAUNCH = {"act_fwd_kernel": (1024, 4096), "act_bwd_kernel": (1024, 4096), "cat2_act_fwd_kernel": (256, 4096),
          "cat2_act_bwd_kernel": (256, 4096), "axpby_kernel": (256, 4096), "fill_kernel": (256, 4096),
          "reflect_pad_bwd_kernel": (256, 4096), "haar_fwd_kernel": (256, 4096), "haar_inv_kernel": (256, 4096),
          "haar_dfront_fwd_kernel": (256, 4096), "haar_dfront_bwd_kernel": (256, 4096), "freq_mix_fwd_kernel": (256, 4096),
          "freq_mix_bwd_kernel": (256, 4096), "loss_bwd_kernel": (256, 4096), "adamw_kernel": (1024, 2048),
          "adamw_dev_kernel": (1024, 2048)}
LOSS_PER_BLOCK, LOSS_MAX_BLOCKS = 2048, 1024                 # loss_fwd: nb = grid_for(n, 2048, 1024) partials
CSUM_BLOCKS, CSUM_MIN_RANGE = 1024, 4096                     # channel_sum: ~1024 blocks in total, ranges of at least 4096
MEAN_MIX_BWD_BLOCK = 64
ACT_PASS = LAUNCH["act_fwd_kernel"][1] * BLOCK * 4           # elements one grid pass of the float4 body covers
ADAMW_PASS = LAUNCH["adamw_kernel"][1] * BLOCK * 4
FLAT_PASS = LAUNCH["axpby_kernel"][1] * BLOCK                # one element (or one 2x2 block) per thread and pass


def f32(v):
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def read_launch_sites(src):
    """{kernel: (per_block, cap, block)} of every launch in ``src`` whose grid comes from grid_for."""
    default = int(re.search(r"grid_for\(long n, int per_block, int cap = (\d+)\)", src).group(1))
    out = {}
    for m in re.finditer(r"hipLaunchKernelGGL\((\w+), dim3\(grid_for\(\w+, (\d+)(?:, (\d+))?\)\), dim3\((\d+)\)", src):
        out[m.group(1)] = (int(m.group(2)), int(m.group(3) or default), int(m.group(4)))
    return out


# ----------------------------------------------------------------------------------------
# the dispatch, restated
# ----------------------------------------------------------------------------------------
def grid_for(n, per_block, cap):
    return max(1, min((n + per_block - 1) // per_block, cap))


def csum_split(L, C):
    """(S, per) of faoctasr_channel_sum: the N * HW elements of a channel are cut into S ranges [s * per, (s + 1) * per)."""
    s = max(1, min((CSUM_BLOCKS + C - 1) // C, (L + CSUM_MIN_RANGE - 1) // CSUM_MIN_RANGE))
    per = (L + s - 1) // s
    per = (per + 3) & ~3
    return (L + per - 1) // per, per


def loss_blocks(n):
    return grid_for(n, LOSS_PER_BLOCK, LOSS_MAX_BLOCKS)


def reflect_both_borders(H, p):
    """A row that the fold collects from the top and the bottom border at once: 1 <= y <= p and H - 1 - p <= y <= H - 2."""
    return max(1, H - 1 - p) <= min(p, H - 2)


def vec_forms(n, kernel):
    """act_fwd / act_bwd / adamw_body: a float4 body over n // 4 quads, then a scalar tail that starts at 4 (n // 4) + global id."""
    per, cap = LAUNCH[kernel]
    out = {"vector body"} if n >= 4 else {"n < 4"}
    if n % 4:
        out.add("scalar tail")
        if grid_for(n, per, cap) > 1:
            out.add("scalar tail, several blocks")
    if n // 4 > cap * BLOCK:
        out.add("second grid pass")
    return out


def flat_forms(units, kernel):
    per, cap = LAUNCH[kernel]
    assert per == BLOCK                                                  # one unit per thread and pass
    return {"second grid pass"} if units > cap * BLOCK else set()


def forms(op, case):
    """The branches of pointwise.hip that ``case`` (a row of ``op``'s table) reaches."""
    if op == "act":
        return {"act: " + f for f in vec_forms(case[0], "act_fwd_kernel")}
    if op == "adamw":
        return {"adamw: " + f for f in vec_forms(case[0], "adamw_kernel")} | {"adamw_kernel", "adamw_dev_kernel"}
    if op == "cat2":
        (N, Ca, Cb, H, W), _, needs = case
        return {"cat2: " + f for f in flat_forms(N * (Ca + Cb) * H * W, "cat2_act_fwd_kernel")} | {"cat2: grads " + needs}
    if op == "axpby":
        n, _, _, inplace = case
        return {"axpby: " + f for f in flat_forms(n, "axpby_kernel")} | ({"axpby: y is a"} if inplace else set())
    if op == "csum":
        (N, C, H, W), acc = case
        S, per = csum_split(N * H * W, C)
        out = {"csum: float4" if H * W % 4 == 0 else "csum: scalar"}
        if S > 1:
            out.add("csum: S > 1, " + ("float4" if H * W % 4 == 0 else "scalar"))
        if S * per > N * H * W:
            out.add("csum: last range cut short")
            if S > 1:
                out.add("csum: S > 1, last range cut short, " + ("float4" if H * W % 4 == 0 else "scalar"))
        if C > CSUM_BLOCKS:
            out.add("csum: C > 1024")
        if acc:
            out.add("csum: accumulate")
        return out
    if op == "reflect":
        NC, H, W, p = case
        out = {"reflect: " + f for f in flat_forms(NC * H * W, "reflect_pad_bwd_kernel")}
        if reflect_both_borders(H, p) or reflect_both_borders(W, p):
            out.add("reflect: both borders on one pixel")
        if reflect_both_borders(H, p) and reflect_both_borders(W, p):
            out.add("reflect: 9 terms")
        if H == p + 1 and W == p + 1:
            out.add("reflect: smallest size")
        return out
    if op == "haar":
        (N, C, H, W), bands = case
        return {"haar: " + f for f in flat_forms(N * C * (H // 2) * (W // 2), "haar_fwd_kernel")} | {"haar: " + bands}
    if op == "dfront":
        (N, H, W), mode = case
        return {"dfront: mode %d" % mode}
    if op == "freq":
        n, grads = case
        return {"freq_mix: " + f for f in flat_forms(n, "freq_mix_fwd_kernel")} | {"freq_mix: " + grads}
    if op == "loss":
        kind, n = case
        nb = loss_blocks(n)
        out = {"loss: one block"} if nb == 1 else set()
        if nb > BLOCK:
            out.add("loss_final: nb > 256")
        if nb == LOSS_MAX_BLOCKS and n > nb * LOSS_PER_BLOCK:
            out.add("loss_final: nb at cap")
        out |= {"loss: " + f for f in flat_forms(n, "loss_bwd_kernel")}
        return out
    if op == "mean_mix":
        (N, La, Lb), _ = case
        out = set()
        for L in (La, Lb):
            out.add("mean_mix: row < 256" if L < BLOCK else "mean_mix: row > 256" if L > BLOCK else "mean_mix: row = 256")
            if L > MEAN_MIX_BWD_BLOCK:
                out.add("mean_mix_bwd: row > 64")
        return out
    raise KeyError(op)


def depth(op, case):
    """Additions an addend of the reduction passes through, from the code: per-thread adds + block_sum_256 (6 shuffle steps + 3)
    + what combines the blocks."""
    if op == "loss":
        n = case[1]
        nb = loss_blocks(n)
        return -(-n // (nb * BLOCK)) + 9 + -(-nb // BLOCK) + 9                   # loss_partial, then loss_final
    if op == "mean_mix":
        (N, La, Lb), _ = case
        return -(-max(La, Lb) // BLOCK) + 9 + 1                                  # + the mix of the two means
    if op == "csum":
        (N, C, H, W), acc = case
        S, per = csum_split(N * H * W, C)
        per_thread = 4 * -(-per // (4 * BLOCK)) if H * W % 4 == 0 else -(-per // BLOCK)
        return per_thread + 9 + S + acc                                          # + S atomic partials (+ what db held)
    raise KeyError(op)


# ----------------------------------------------------------------------------------------
# the case tables: the smallest that reach each branch; a case's seed is its position in its table
# ----------------------------------------------------------------------------------------
ACT_KINDS = [("relu", 0.2), ("lrelu", 0.2), ("lrelu", 0.0), ("tanh", 0.2)]
ACT_CASES = [(n, a, s) for n in (1, 3, 4, 5, 1027, 262147, ACT_PASS + 1031) for (a, s) in ACT_KINDS]
CAT2_SHAPES = [(1, 1, 1, 1, 1), (2, 5, 3, 7, 9), (3, 1, 64, 5, 3), (2, 64, 1, 6, 6), (2, 33, 31, 96, 96)]     # last: > one pass
CAT2_CASES = [(s, a, g) for s in CAT2_SHAPES for a in (None, "relu", "lrelu", "tanh") for g in ("ab", "a", "b")]
AXPBY_CASES = [(n, al, be, ip) for n in (1, 255, 257, FLAT_PASS + 513) for (al, be) in ((1.0, 1.0), (0.7, -0.3), (1.0, 0.0))
               for ip in (False, True)]
FILL_CASES = [1, 255, 257, FLAT_PASS + 513]
CSUM_SHAPES = [(1, 1, 1, 1), (3, 5, 7, 9),      # scalar, S = 1
               (2, 3, 8, 8),                    # float4, S = 1
               (3, 2, 64, 66),                  # float4, L = 12672, S = 4 ranges of 3168
               (3, 2, 42, 46),                  # float4, L = 5796, S = 2, per = 2900: the last range is cut at L
               (2, 1, 97, 101),                 # scalar, L = 19594, S = 5, per = 3920: the last range is cut at L
               (1, 1100, 4, 4)]                 # C > 1024: one range per channel
CSUM_CASES = [(s, acc) for s in CSUM_SHAPES for acc in (0, 1)]
REFLECT_CASES = [(nc, h, w, p) for p in (1, 2, 3) for (h, w) in ((p + 1, p + 1), (p + 1, 4 * p + 3), (2 * p + 1, 2 * p), (20, 24))
                 for nc in (1, 6)] + [(6, 420, 420, 3)]                         # last: 1,058,400 > one pass
HAAR_SHAPES = [(1, 1, 2, 2), (2, 3, 2, 10), (2, 3, 10, 2), (1, 3, 24, 40), (2, 2, 1026, 1024)]              # last: > one pass
HAAR_CASES = [(s, b) for s in HAAR_SHAPES for b in ("both bands", "ll only", "hi only")]
DFRONT_CASES = [(s, m) for s in ((1, 2, 2), (3, 6, 10), (2, 64, 48)) for m in (0, 1)]
FREQ_CASES = [(n, g) for n in (1, 1027, FLAT_PASS + 7) for g in ("both gradients", "g_hf only", "g_lf only")]
LOSS_KINDS = ("mse", "l1", "bce")
LOSS_N = (1, 255, 2048, 2049, 524289, 2097152 + 4097)                            # nb = 1, 1, 1, 2, 257, 1024 (the cap)
LOSS_CASES = [(k, n) for k in LOSS_KINDS for n in LOSS_N]
LOSS_WEIGHT, LOSS_UPSTREAM = 1.7, 0.6
BCE_LOGITS = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0)
MEAN_MIX_CASES = [(s, w) for s in ((1, 1, 1), (3, 36, 4), (2, 255, 257), (3, 256, 1024), (2, 4096, 900)) for w in ((0.7, 0.3), (1.0, 0.0))]
ADAMW_N = (1, 3, 4, 5, 1027, ADAMW_PASS + 1031)
#: (n, start, weight_decay, grad_scale); start "zero": steps 1, 2, 3 from zero moments; "late": step 1000 from given moments
ADAMW_CASES = [(n, st, wd, gs) for n in ADAMW_N for st in ("zero", "late") for wd in (0.0, 1e-2) for gs in (1.0, 0.125)]
ADAMW_LR, ADAMW_BETAS, ADAMW_EPS = 1.3e-4, (0.9, 0.999), 1e-8
TABLES = {"act": ACT_CASES, "cat2": CAT2_CASES, "axpby": AXPBY_CASES, "csum": CSUM_CASES, "reflect": REFLECT_CASES, "haar": HAAR_CASES,
          "dfront": DFRONT_CASES, "freq": FREQ_CASES, "loss": LOSS_CASES, "mean_mix": MEAN_MIX_CASES, "adamw": ADAMW_CASES}
FORMS = {"act: vector body", "act: scalar tail", "act: scalar tail, several blocks", "act: n < 4", "act: second grid pass",
         "adamw: vector body", "adamw: scalar tail", "adamw: scalar tail, several blocks", "adamw: n < 4", "adamw: second grid pass",
         "adamw_kernel", "adamw_dev_kernel",
         "cat2: second grid pass", "cat2: grads ab", "cat2: grads a", "cat2: grads b", "axpby: second grid pass", "axpby: y is a",
         "csum: float4", "csum: scalar", "csum: S > 1, float4", "csum: S > 1, scalar", "csum: last range cut short",
         "csum: S > 1, last range cut short, float4", "csum: S > 1, last range cut short, scalar", "csum: C > 1024", "csum: accumulate",
         "reflect: second grid pass", "reflect: both borders on one pixel", "reflect: 9 terms", "reflect: smallest size",
         "haar: second grid pass", "haar: both bands", "haar: ll only", "haar: hi only", "dfront: mode 0", "dfront: mode 1",
         "freq_mix: second grid pass", "freq_mix: both gradients", "freq_mix: g_hf only", "freq_mix: g_lf only",
         "loss: one block", "loss_final: nb > 256", "loss_final: nb at cap", "loss: second grid pass",
         "mean_mix: row < 256", "mean_mix: row > 256", "mean_mix: row = 256", "mean_mix_bwd: row > 64"}


def ident(op, case):
    def one(v):
        if isinstance(v, tuple):
            return "x".join(map(str, v))
        return "none" if v is None else str(v).replace(" ", "_")
    return op + "_" + "_".join(one(v) for v in (case if isinstance(case, tuple) else (case,)))


# ----------------------------------------------------------------------------------------
# the restatements.  Each takes the case's inputs (fp32 CPU tensors) and a dtype and returns a dict of outputs; "abs_<name>" is the
# sum of the absolute values of the addends of <name>.
# ----------------------------------------------------------------------------------------
def act_fn(v, act, slope):
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == "lrelu":
        return torch.where(v > 0, v, v * f32(slope))
    if act == "tanh":
        return torch.tanh(v)
    assert act is None
    return v


def act_dfn(pre, out, act, slope):
    if act == "relu":
        return (pre > 0).to(pre.dtype)
    if act == "lrelu":
        return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, f32(slope)))
    if act == "tanh":
        return 1 - out * out
    return torch.ones_like(pre)


def act_ref(c, act, slope, dtype=torch.float64):
    x = c["x"].to(dtype)
    y = act_fn(x, act, slope)
    return {"y": y, "dx": c["cot"].to(dtype) * act_dfn(x, y, act, slope)}


def cat2_ref(c, act, slope, dtype=torch.float64):
    pre = torch.cat([c["a"].to(dtype), c["b"].to(dtype)], 1)
    y = act_fn(pre, act, slope)
    g = c["cot"].to(dtype) * act_dfn(pre, y, act, slope)
    Ca = c["a"].shape[1]
    return {"y": y, "da": g[:, :Ca], "db": g[:, Ca:]}


def axpby_ref(c, alpha, beta, dtype=torch.float64):
    a, b, cot = c["a"].to(dtype), c["b"].to(dtype), c["cot"].to(dtype)
    al, be = f32(alpha), f32(beta)
    return {"y": al * a + be * b, "abs_y": (al * a).abs() + (be * b).abs(), "da": al * cot, "abs_da": (al * cot).abs(), "db": be * cot,
            "abs_db": (be * cot).abs()}


def csum_ref(c, acc, dtype=torch.float64):
    dy = c["dy"].to(dtype)
    s, a = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
    if acc:
        s, a = s + c["prior"].to(dtype), a + c["prior"].to(dtype).abs()
    return {"db": s, "abs_db": a}


def reflect_index(n, p):
    """Source index of every position of a row of n reflection-padded by p (no repeat of the border element)."""
    j = torch.arange(-p, n + p)
    j = j.abs()
    return torch.where(j > n - 1, 2 * (n - 1) - j, j)


def reflect_fold_ref(c, p, dtype=torch.float64):
    """Gradient of ReflectionPad2d(p): every padded position adds its cotangent to the source pixel it mirrors."""
    dxp = c["dxp"].to(dtype)
    NC, HP, WP = dxp.shape
    H, W = HP - 2 * p, WP - 2 * p
    iy, ix = reflect_index(H, p), reflect_index(W, p)
    out = {}
    for name, v in (("dx", dxp), ("abs_dx", dxp.abs())):
        rows = torch.zeros(NC, H, WP, dtype=dtype).index_add_(1, iy, v)
        out[name] = torch.zeros(NC, H, W, dtype=dtype).index_add_(2, ix, rows)
    return out


def _quads(x):
    return x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]


def haar_fwd_ref(x, dtype=torch.float64):
    """One Haar analysis level of (N, C, H, W): ll (N, C, h, w), hi (N, C, 3, h, w) in the order LH, HL, HH."""
    a, b, c, d = _quads(x.to(dtype))
    s = (a.abs() + b.abs() + c.abs() + d.abs()) * 0.5
    return {"ll": (a + b + c + d) * 0.5, "hi": torch.stack([(a + b - c - d) * 0.5, (a - b + c - d) * 0.5, (a - b - c + d) * 0.5], 2),
            "abs_ll": s, "abs_hi": torch.stack([s, s, s], 2)}


def haar_inv_ref(ll, hi, shape, dtype=torch.float64):
    """One Haar synthesis level; an absent band is zeros.  Also the adjoint of the analysis (the bank is orthogonal)."""
    N, C, H, W = shape
    z = torch.zeros(N, C, H // 2, W // 2, dtype=dtype)
    l = z if ll is None else ll.to(dtype)
    lh, hl, hh = (z, z, z) if hi is None else (hi[:, :, k].to(dtype) for k in range(3))
    x, s = torch.empty(N, C, H, W, dtype=dtype), torch.empty(N, C, H, W, dtype=dtype)
    x[..., 0::2, 0::2] = (l + lh + hl + hh) * 0.5
    x[..., 0::2, 1::2] = (l + lh - hl - hh) * 0.5
    x[..., 1::2, 0::2] = (l - lh + hl - hh) * 0.5
    x[..., 1::2, 1::2] = (l - lh - hl + hh) * 0.5
    for k in range(4):
        s[..., k // 2::2, k % 2::2] = (l.abs() + lh.abs() + hl.abs() + hh.abs()) * 0.5
    return {"x": x, "abs_x": s}


def dfront_ref(c, mode, dtype=torch.float64):
    """Discriminator front ends on (N, 1, H, W): mode 0 -> LL; mode 1 -> (LH, HL, HH) * 0.5 + 0.5 as 3 channels; and dx."""
    f = haar_fwd_ref(c["x"], dtype)
    N, _, H, W = c["x"].shape
    cot = c["cot"].to(dtype)
    if mode == 0:
        b = haar_inv_ref(cot, None, (N, 1, H, W), dtype)
        return {"y": f["ll"], "abs_y": f["abs_ll"], "dx": b["x"], "abs_dx": b["abs_x"]}
    b = haar_inv_ref(None, (cot * 0.5).unsqueeze(1), (N, 1, H, W), dtype)
    return {"y": f["hi"][:, 0] * 0.5 + 0.5, "abs_y": f["abs_hi"][:, 0] * 0.5 + 0.5, "dx": b["x"], "abs_dx": b["abs_x"]}


def sgn(v):
    return (v > 0).to(v.dtype) - (v < 0).to(v.dtype)


def freq_mix_ref(c, grads="both gradients", dtype=torch.float64):
    """hf = (|x - lo_hp| + x) / 2, lf = -|lo_lp|; backward with lo_hp, lo_lp as independent operands:
    s_hp = -d/d lo_hp, s_lp = d/d lo_lp, dx_direct = d/dx.  An absent upstream gradient is zeros; sgn(0) = 0."""
    x, hp, lp = c["x"].to(dtype), c["lo_hp"].to(dtype), c["lo_lp"].to(dtype)
    gh = c["g_hf"].to(dtype) if grads != "g_lf only" else torch.zeros_like(x)
    gl = c["g_lf"].to(dtype) if grads != "g_hf only" else torch.zeros_like(x)
    sh = 0.5 * gh * sgn(x - hp)
    return {"hf": ((x - hp).abs() + x) * 0.5, "abs_hf": ((x - hp).abs() + x.abs()) * 0.5, "lf": -lp.abs(), "s_hp": sh, "s_lp": -gl * sgn(lp),
            "dx_direct": 0.5 * gh + sh}


def loss_ref(c, kind, dtype=torch.float64):
    """weight * mean(term) and its gradients for an upstream gradient g: term = (a - b)^2 | |a - b| |
    max(a, 0) - a b + log1p(exp(-|a|)) (BCE with logits a and targets b)."""
    a, b = c["a"].to(dtype), c["b"].to(dtype)
    scale = f32(LOSS_WEIGHT / a.numel())
    gs = float(c["g"]) * scale
    d = a - b
    if kind == "mse":
        term, da, db = d * d, gs * 2 * d, -gs * 2 * d
        pieces = term
    elif kind == "l1":
        term, da, db = d.abs(), gs * sgn(d), -gs * sgn(d)
        pieces = term
    else:
        lg = torch.log1p(torch.exp(-a.abs()))
        term, da, db = a.clamp_min(0) - a * b + lg, gs * (torch.sigmoid(a) - b), -gs * a
        pieces = a.clamp_min(0) + (a * b).abs() + lg
    out = {"value": term.sum() * scale, "abs_value": pieces.sum() * scale, "da": da, "db": db, "abs_da": da.abs(), "abs_db": db.abs()}
    if kind == "bce":
        out["lib_value"] = lg.sum() * scale
    return out


def mean_mix_ref(c, wa, wb, dtype=torch.float64):
    a, b, g = c["a"].to(dtype), c["b"].to(dtype), c["g"].to(dtype)
    wa, wb = f32(wa), f32(wb)
    N, La, Lb = a.shape[0], a[0].numel(), b[0].numel()
    fa, fb = a.reshape(N, La), b.reshape(N, Lb)
    da = (g * wa / La).reshape([N] + [1] * (a.dim() - 1)).expand_as(a)
    db = (g * wb / Lb).reshape([N] + [1] * (b.dim() - 1)).expand_as(b)
    return {"out": wa * (fa.sum(1) / La) + wb * (fb.sum(1) / Lb), "abs_out": abs(wa) * fa.abs().sum(1) / La + abs(wb) * fb.abs().sum(1) / Lb,
            "da": da, "db": db, "abs_da": da.abs(), "abs_db": db.abs()}


def adamw_ref(p, g, m, v, step, lr, betas, eps, wd, gscale, dtype=torch.float64, round_scalars=False, abs_m=None):
    """One step of torch.optim.AdamW in its single-tensor order on grad = g * gscale: decay, moments, bias corrections, update.
    ``round_scalars``: the hyper-parameters as the fp32 values the kernel receives.  Returns (p, m, v, abs_m, abs_v); abs_m is the
    sum of the absolute values of m's addends over all steps so far, A' = b1 A + |(1 - b1) g| from A = |m| before the first
    (an earlier step's rounding error is relative to ITS addends, which may cancel in m since), and v has only positive addends."""
    r = f32 if round_scalars else float
    lr, b1, b2, eps, wd, gscale = r(lr), r(betas[0]), r(betas[1]), r(eps), r(wd), r(gscale)
    p, g, m, v = p.to(dtype), g.to(dtype) * gscale, m.to(dtype), v.to(dtype)
    p = p * (1 - lr * wd)
    m2, v2 = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    abs_m = b1 * (m.abs() if abs_m is None else abs_m.to(dtype)) + ((1 - b1) * g).abs()
    return p - (lr / bc1) * (m2 / denom), m2, v2, abs_m, v2


def adamw_run(c, case, dtype=torch.float64, round_scalars=False):
    """The case's steps; returns per step (p, m, v, abs_m, abs_v)."""
    n, start, wd, gs = case
    p, m, v = c["p"], c["m"], c["v"]
    out, am = [], None
    for i, g in enumerate(c["grads"]):
        p, m, v, am, av = adamw_ref(p, g, m, v, c["first_step"] + i, ADAMW_LR, ADAMW_BETAS, ADAMW_EPS, wd, gs, dtype, round_scalars, am)
        out.append((p, m, v, am, av))
    return out


# ----------------------------------------------------------------------------------------
# input builders (fp32 CPU tensors; the same in every process).  Spikes of 40 sit where ranges end.
# ----------------------------------------------------------------------------------------
def gen(op, case):
    """A case's seed is its position in its table (999 for the pins' own small cases)."""
    return torch.Generator().manual_seed(1000 * sorted(TABLES).index(op) + (TABLES[op].index(case) if case in TABLES[op] else 999))


def range_ends(n, marks=()):
    """First and last element, and either side of every mark inside (0, n)."""
    s = {0, n - 1}
    for m in marks:
        s |= {k for k in (m - 1, m) if 0 <= k < n}
    return torch.tensor(sorted(s))


def pass_marks(n, pass_elems):
    return list(range(pass_elems, n, pass_elems))


def build_act(case):
    n, act, slope = case
    g = gen("act", case)
    x, cot = torch.randn(n, generator=g) * 2 + 0.3, torch.randn(n, generator=g) + 0.5
    ends = range_ends(n, [n // 4 * 4] + pass_marks(n, ACT_PASS))
    x[ends] = SPIKE
    cot[ends] = SPIKE
    if act in ("relu", "lrelu"):
        cot = cot * (x.abs() > KINK)
    return {"x": x, "cot": cot, "ends": ends}


def build_cat2(case):
    (N, Ca, Cb, H, W), act, _ = case
    g = gen("cat2", case)
    a, b = torch.randn(N, Ca, H, W, generator=g) * 2 + 0.3, torch.randn(N, Cb, H, W, generator=g) * 2 - 0.3
    cot = torch.randn(N, Ca + Cb, H, W, generator=g) + 0.5
    for t in (a, b):
        t.view(-1)[range_ends(t.numel())] = SPIKE
    cot.view(-1)[range_ends(cot.numel(), pass_marks(cot.numel(), FLAT_PASS))] = SPIKE
    if act in ("relu", "lrelu"):
        cot = cot * (torch.cat([a, b], 1).abs() > KINK)
    return {"a": a, "b": b, "cot": cot}


def build_axpby(case):
    n = case[0]
    g = gen("axpby", case)
    a, b, cot = (torch.randn(n, generator=g) for _ in range(3))
    ends = range_ends(n, pass_marks(n, FLAT_PASS))
    a[ends] = SPIKE
    b[ends] = -SPIKE / 4
    cot[ends] = SPIKE
    return {"a": a, "b": b, "cot": cot}


def build_csum(case):
    (N, C, H, W), acc = case
    g = gen("csum", case)
    dy = torch.randn(N, C, H, W, generator=g) + 0.25
    S, per = csum_split(N * H * W, C)
    ends = range_ends(N * H * W, [s * per for s in range(1, S)])
    rows = dy.permute(1, 0, 2, 3).reshape(C, -1)                       # a copy: the channel's N * HW elements in the kernel's order
    rows[:, ends] = SPIKE
    dy = rows.reshape(C, N, H, W).permute(1, 0, 2, 3).contiguous()
    return {"dy": dy, "prior": torch.randn(C, generator=g) * 30, "ends": ends}


def build_reflect(case):
    NC, H, W, p = case
    g = gen("reflect", case)
    dxp = torch.randn(NC, H + 2 * p, W + 2 * p, generator=g) + 0.5
    dxp.view(-1)[range_ends(dxp.numel())] = SPIKE
    dxp[:, [0, p, H + p - 1, H + 2 * p - 1], :] += SPIKE / 4            # border rows / columns and the image's own edge
    dxp[:, :, [0, p, W + p - 1, W + 2 * p - 1]] -= SPIKE / 8
    return {"dxp": dxp}


def build_haar(case):
    (N, C, H, W), _ = case
    g = gen("haar", case)
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.3
    ll, hi = torch.randn(N, C, H // 2, W // 2, generator=g) + 0.5, torch.randn(N, C, 3, H // 2, W // 2, generator=g)
    for t in (x, ll, hi):
        t.view(-1)[range_ends(t.numel())] = SPIKE
    units = N * C * (H // 2) * (W // 2)
    ll.view(-1)[range_ends(units, pass_marks(units, FLAT_PASS))] = SPIKE
    return {"x": x, "ll": ll, "hi": hi}


def build_dfront(case):
    (N, H, W), mode = case
    g = gen("dfront", case)
    x, cot = torch.randn(N, 1, H, W, generator=g) * 2 + 0.3, torch.randn(N, 3 if mode else 1, H // 2, W // 2, generator=g) + 0.5
    for t in (x, cot):
        t.view(-1)[range_ends(t.numel())] = SPIKE
    return {"x": x, "cot": cot}


def ties(n, g, every=20):
    """About one position in ``every``, at least one when n >= 2."""
    m = torch.rand(n, generator=g) < 1.0 / every
    if n >= 2:
        m[n // 2] = True
    return m


def build_freq(case):
    n, _ = case
    g = gen("freq", case)
    x, hp, lp, gh, gl = (torch.randn(n, generator=g) for _ in range(5))
    ends = range_ends(n, pass_marks(n, FLAT_PASS))
    x[ends] = SPIKE
    gh[ends] = SPIKE
    gl[ends] = -SPIKE
    t_hp, t_lp = ties(n, g), ties(n, g)
    hp[t_hp] = x[t_hp]                                                   # x == lo_hp exactly
    lp[t_lp] = 0.0
    return {"x": x, "lo_hp": hp, "lo_lp": lp, "g_hf": gh, "g_lf": gl, "tie_hp": t_hp, "tie_lp": t_lp}


def build_loss(case):
    kind, n = case
    g = gen("loss", case)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ends = range_ends(n, pass_marks(n, loss_blocks(n) * BLOCK) + pass_marks(n, FLAT_PASS))
    tie = torch.zeros(n, dtype=torch.bool)
    if kind == "bce":
        a = a * 3
        b = torch.rand(n, generator=g)                                   # targets in [0, 1] ...
        b[3::7] = torch.randn(n, generator=g)[3::7] * 2                  # ... and outside it
        sp = torch.tensor(BCE_LOGITS)
        a[ends] = sp[torch.arange(len(ends)) % len(sp)]
        k = min(n, 4 * len(sp))
        a[n - k:] = sp[torch.arange(k) % len(sp)]                        # every special logit, next to targets of either kind
    else:
        a[ends] = SPIKE
        if kind == "l1":
            tie = ties(n, g)
            tie[ends] = False
            b[tie] = a[tie]
    return {"a": a, "b": b, "g": torch.tensor(LOSS_UPSTREAM), "tie": tie, "ends": ends}


def build_mean_mix(case):
    (N, La, Lb), _ = case
    g = gen("mean_mix", case)
    a, b = torch.randn(N, 1, La, generator=g) + 0.5, torch.randn(N, 1, Lb, generator=g) - 0.25
    for t, L in ((a, La), (b, Lb)):
        t[:, 0, range_ends(L, pass_marks(L, BLOCK)[:1] + [L - L % BLOCK])] = SPIKE
    return {"a": a, "b": b, "g": torch.randn(N, generator=g) + 2.0}


def build_adamw(case):
    n, start, wd, gs = case
    g = gen("adamw", case)
    p = torch.randn(n, generator=g)
    ends = range_ends(n, [n // 4 * 4] + pass_marks(n, ADAMW_PASS))
    p[ends] = SPIKE
    steps = 3 if start == "zero" else 1
    grads = [torch.randn(n, generator=g) / gs for _ in range(steps)]
    for gr in grads:
        gr[ends] = SPIKE / gs
    if start == "zero":
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 0.01
    return {"p": p, "m": m, "v": v, "grads": grads, "first_step": 1 if start == "zero" else 1000, "ends": ends}


# ----------------------------------------------------------------------------------------
# the bars
# ----------------------------------------------------------------------------------------
def _pair(got, ref):
    return got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)


def _count(err, tol):
    bad = ~(err <= tol)                                                  # a NaN is a violation
    return int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0


def exact_violations(got, ref):
    """got == float64 reference rounded to fp32.  Returns (count, worst error in fp32 ulps)."""
    g, r = _pair(got, ref)
    err = (g - r.float().double()).abs()
    return int((~(err == 0)).sum()), float((err / ulp32(r)).max()) if err.numel() else 0.0


def short_violations(got, ref, abs_terms, k):
    """|got - ref| <= k 2^-24 sum |terms| + 1 ulp.  Returns (count, worst error as a fraction of the bar)."""
    g, r = _pair(got, ref)
    return _count((g - r).abs(), k * U * abs_terms.detach().double().reshape(-1) + ulp32(r))


def close_violations(got, ref, rtol, atol):
    g, r = _pair(got, ref)
    return _count((g - r).abs(), rtol * r.abs() + atol)


def worst_ulps(got, ref):
    g, r = _pair(got, ref)
    return float(((g - r).abs() / ulp32(r)).max()) if g.numel() else 0.0


def bce_value_violations(got, ref):
    g, r = _pair(got, ref["value"])
    tol = GAMMA_SUM * ref["abs_value"].double().reshape(-1) + 2 * ulp32(r) + 1e-4 * ref["lib_value"].double().reshape(-1) + 1e-7
    return _count((g - r).abs(), tol)


def judge(got, ref, name, bar):
    """(violations, worst) of output ``name`` under ``bar``: ("exact",) | ("short", k) | ("close", rtol, atol) | ("sum",) |
    ("bce_value",)."""
    if bar[0] == "exact":
        return exact_violations(got, ref[name])
    if bar[0] == "short":
        return short_violations(got, ref[name], ref["abs_" + name], bar[1])
    if bar[0] == "close":
        return close_violations(got, ref[name], bar[1], bar[2])
    if bar[0] == "sum":
        return sum_violations(got, ref[name], ref["abs_" + name])
    assert bar[0] == "bce_value"
    return bce_value_violations(got, ref)


def act_bars(act):
    if act == "tanh":
        return {"y": ("close", 1e-6, 1e-6), "dx": ("close", 1e-5, 1e-6)}
    return {"y": ("exact",), "dx": ("exact",)}


def cat2_bars(act):
    b = act_bars(act)
    return {"y": b["y"], "da": b["dx"], "db": b["dx"]}


AXPBY_BARS = {"y": ("short", 3), "da": ("short", 2), "db": ("short", 2)}
CSUM_BARS = {"db": ("sum",)}
REFLECT_BARS = {"dx": ("short", 8)}
HAAR_BARS = {"ll": ("short", 3), "hi": ("short", 3), "x": ("short", 3)}
FREQ_BARS = {"hf": ("short", 2), "lf": ("exact",), "s_hp": ("exact",), "s_lp": ("exact",), "dx_direct": ("exact",)}
MEAN_MIX_BARS = {"out": ("sum",), "da": ("short", 2), "db": ("short", 2)}
ADAMW_P_BAR = ("close", 1e-6, 1e-7)


def dfront_bars(mode):
    return {"y": ("short", 3), "dx": ("short", 3)} if mode == 0 else {"y": ("short", 4), "dx": ("short", 3)}


def loss_bars(kind):
    if kind == "mse":
        return {"value": ("sum",), "da": ("short", 3), "db": ("short", 3)}
    if kind == "l1":
        return {"value": ("sum",), "da": ("short", 2), "db": ("short", 2)}
    return {"value": ("bce_value",), "da": ("close", 1e-4, 1e-7), "db": ("short", 2)}


def assert_bars(case, got, ref, bars, names=None):
    for name in names or bars:
        assert got[name].shape == ref[name].shape, (case, name, got[name].shape, ref[name].shape)
        n, worst = judge(got[name], ref, name, bars[name])
        assert n == 0, "%s %s: %d elements outside %s, worst %.3g" % (case, name, n, bars[name], worst)


def adamw_assert(case, steps_got, steps_ref, steps_ref_rounded):
    """p of every step against the float64 restatement (rtol 1e-6 atol 1e-7); m and v against the restatement with the scalars
    the kernel receives, within k = 5 / 6 roundings per step taken."""
    for i, (got, ref, rr) in enumerate(zip(steps_got, steps_ref, steps_ref_rounded)):
        n, worst = close_violations(got[0], ref[0], *ADAMW_P_BAR[1:])
        assert n == 0, "%s step %d p: %d elements outside rtol 1e-6 atol 1e-7, worst %.3g" % (case, i, n, worst)
        for j, name, k in ((1, "m", 5), (2, "v", 6)):
            n, worst = short_violations(got[j], rr[j], rr[j + 2], k * (i + 1))
            assert n == 0, "%s step %d %s: %d elements outside the bar, worst %.3g" % (case, i, name, n, worst)


# ----------------------------------------------------------------------------------------
# the pin: restatement against torch in float64
# ----------------------------------------------------------------------------------------
def _pin(a, b, what):
    assert tuple(a.shape) == tuple(b.shape), (what, a.shape, b.shape)
    assert rel_l2(a, b) <= PIN, (what, rel_l2(a, b))


def _torch_act(v, act, slope):
    return {None: lambda t: t, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, f32(slope)), "tanh": torch.tanh}[act](v)


@pytest.mark.parametrize("act,slope", ACT_KINDS + [(None, 0.2)])
def test_activation_restatement_is_torch_float64(act, slope):
    c = build_act((1027, act, slope))
    x = c["x"].double().requires_grad_(True)
    y = _torch_act(x, act, slope)
    y.backward(c["cot"].double())
    ref = act_ref(c, act, slope)
    _pin(ref["y"], y, "y")
    _pin(ref["dx"], x.grad, "dx")


@pytest.mark.parametrize("act", [None, "relu", "lrelu", "tanh"])
def test_cat2_restatement_is_torch_float64(act):
    c = build_cat2(((2, 5, 3, 7, 9), act, "ab"))
    a, b = c["a"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    y = _torch_act(torch.cat([a, b], 1), act, SLOPE)
    y.backward(c["cot"].double())
    ref = cat2_ref(c, act, SLOPE)
    _pin(ref["y"], y, "y")
    _pin(ref["da"], a.grad, "da")
    _pin(ref["db"], b.grad, "db")


@pytest.mark.parametrize("alpha,beta", [(1.0, 1.0), (0.7, -0.3), (1.0, 0.0)])
def test_axpby_restatement_is_torch_float64(alpha, beta):
    c = build_axpby((257, alpha, beta, False))
    a, b = c["a"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    y = f32(alpha) * a + f32(beta) * b
    y.backward(c["cot"].double())
    ref = axpby_ref(c, alpha, beta)
    _pin(ref["y"], y, "y")
    _pin(ref["da"], a.grad, "da")
    _pin(ref["db"], b.grad, "db")
    assert bool((ref["abs_y"] >= ref["y"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("acc", [0, 1])
def test_channel_sum_restatement_is_torch_float64(acc):
    """The per-channel sum is the bias gradient of a convolution: autograd through x + bias."""
    c = build_csum(((3, 5, 7, 9), acc))
    bias = torch.zeros(5, dtype=torch.float64, requires_grad=True)
    if acc:
        bias.grad = c["prior"].double().clone()
    (torch.zeros(3, 5, 7, 9, dtype=torch.float64) + bias.view(1, 5, 1, 1)).backward(c["dy"].double())
    ref = csum_ref(c, acc)
    _pin(ref["db"], bias.grad, "db")
    pos = csum_ref({"dy": c["dy"].abs(), "prior": c["prior"].abs()}, acc)
    _pin(pos["abs_db"], pos["db"], "abs_db")


@pytest.mark.parametrize("case", [(2, 2, 2, 1), (2, 3, 11, 2), (3, 7, 6, 3), (1, 4, 4, 3), (2, 9, 8, 2)], ids=lambda c: "x".join(map(str, c)))
def test_reflect_fold_restatement_is_torch_float64(case):
    NC, H, W, p = case
    c = build_reflect(case)
    x = torch.zeros(1, NC, H, W, dtype=torch.float64, requires_grad=True)
    F.pad(x, (p, p, p, p), mode="reflect").backward(c["dxp"].double().unsqueeze(0))
    ref = reflect_fold_ref(c, p)
    _pin(ref["dx"], x.grad[0], "dx")
    _pin(reflect_fold_ref({"dxp": c["dxp"].abs()}, p)["dx"], ref["abs_dx"], "abs_dx")


def test_haar_restatement_is_the_oracle_float64():
    from oracle import octa_oracle as O
    shape = (2, 3, 6, 10)
    c = build_haar((shape, "both bands"))
    x = c["x"].double().requires_grad_(True)
    ll, hi = O.haar_dwt2_level(x)
    f = haar_fwd_ref(c["x"])
    _pin(f["ll"], ll, "ll")
    _pin(f["hi"], hi, "hi")
    lc, hc = c["ll"].double(), c["hi"].double()
    z_l, z_h = torch.zeros_like(lc), torch.zeros_like(hc)
    for bands, l_, h_ in (("both", lc, hc), ("ll", lc, None), ("hi", None, hc)):
        inv = haar_inv_ref(l_, h_, shape)
        _pin(inv["x"], O.haar_idwt2_level(z_l if l_ is None else l_, z_h if h_ is None else h_), "synthesis " + bands)
        (gx,) = torch.autograd.grad([ll, hi], [x], [z_l if l_ is None else l_, z_h if h_ is None else h_], retain_graph=True)
        _pin(inv["x"], gx, "adjoint of the analysis " + bands)                 # AFB2D.backward is the synthesis kernel
    # the analysis is the adjoint of the synthesis: <A x, c> = <x, A^T c>
    lhs = (f["ll"] * lc).sum() + (f["hi"] * hc).sum()
    rhs = (c["x"].double() * haar_inv_ref(lc, hc, shape)["x"]).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))


@pytest.mark.parametrize("mode", [0, 1])
def test_haar_dfront_restatement_is_the_oracle_float64(mode):
    from oracle import octa_oracle as O
    c = build_dfront(((3, 6, 10), mode))
    x = c["x"].double().requires_grad_(True)
    ll, hi = O.haar_dwt2_level(x)
    y = ll if mode == 0 else hi[:, 0] * 0.5 + 0.5                               # (N, 1, 3, h, w) -> three channels
    y.backward(c["cot"].double())
    ref = dfront_ref(c, mode)
    _pin(ref["y"], y, "y")
    _pin(ref["dx"], x.grad, "dx")


@pytest.mark.parametrize("grads", ["both gradients", "g_hf only", "g_lf only"])
def test_freq_mix_restatement_is_torch_float64(grads):
    c = build_freq((1027, grads))
    assert int(c["tie_hp"].sum()) > 20 and int(c["tie_lp"].sum()) > 20
    x, hp, lp = (c[k].double().requires_grad_(True) for k in ("x", "lo_hp", "lo_lp"))
    hf, lf = ((x - hp).abs() + x) / 2, -lp.abs()
    out = [t for t, on in ((hf, grads != "g_lf only"), (lf, grads != "g_hf only")) if on]
    cot = [c[k].double() for k, on in (("g_hf", grads != "g_lf only"), ("g_lf", grads != "g_hf only")) if on]
    gx, ghp, glp = torch.autograd.grad(out, [x, hp, lp], cot, allow_unused=True)
    ref = freq_mix_ref(c, grads)
    _pin(ref["hf"], hf, "hf")
    _pin(ref["lf"], lf, "lf")
    z = torch.zeros(1027, dtype=torch.float64)
    _pin(ref["dx_direct"], z if gx is None else gx, "dx_direct")
    _pin(ref["s_hp"], z if ghp is None else -ghp, "s_hp")
    _pin(ref["s_lp"], z if glp is None else glp, "s_lp")
    if grads != "g_lf only":
        assert float(ref["s_hp"][c["tie_hp"]].abs().max()) == 0.0              # torch's abs has gradient 0 at 0
    if grads != "g_hf only":
        assert float(ref["s_lp"][c["tie_lp"]].abs().max()) == 0.0


@pytest.mark.parametrize("kind", LOSS_KINDS)
def test_loss_restatement_is_torch_float64(kind):
    c = build_loss((kind, 2049))
    if kind == "l1":
        assert int(c["tie"].sum()) > 50
    if kind == "bce":
        assert set(BCE_LOGITS) <= set(c["a"].tolist()) and bool((c["b"] < 0).any()) and bool((c["b"] > 1).any())
    a, b = c["a"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "bce": F.binary_cross_entropy_with_logits}[kind]
    val = fn(a, b) * (f32(LOSS_WEIGHT / 2049) * 2049)
    val.backward(c["g"].double())
    ref = loss_ref(c, kind)
    _pin(ref["value"], val, "value")
    _pin(ref["da"], a.grad, "da")
    _pin(ref["db"], b.grad, "db")
    assert float(ref["abs_value"]) >= abs(float(ref["value"])) * (1 - 1e-12)


@pytest.mark.parametrize("wa,wb", [(0.7, 0.3), (1.0, 0.0)])
def test_mean_mix_restatement_is_torch_float64(wa, wb):
    c = build_mean_mix(((3, 300, 36), (wa, wb)))
    a, b = c["a"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    out = torch.flatten(f32(wa) * a.mean(dim=(1, 2)).view(3, -1) + f32(wb) * b.mean(dim=(1, 2)).view(3, -1))
    out.backward(c["g"].double())
    ref = mean_mix_ref(c, wa, wb)
    _pin(ref["out"], out, "out")
    _pin(ref["da"], a.grad, "da")
    if wb:
        _pin(ref["db"], b.grad, "db")
    else:
        assert float(ref["db"].abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0


@pytest.mark.parametrize("start,wd,gs", [("zero", 1e-2, 1.0), ("zero", 0.0, 0.125), ("late", 1e-2, 0.125)])
def test_adamw_restatement_is_torch_float64(start, wd, gs):
    from oracle import octa_oracle as O
    case = (1027, start, wd, gs)
    c = build_adamw(case)
    p = torch.nn.Parameter(c["p"].double().clone())
    opt = torch.optim.AdamW([p], lr=ADAMW_LR, betas=ADAMW_BETAS, eps=ADAMW_EPS, weight_decay=wd, foreach=False)
    po = c["p"].double().clone().requires_grad_(True)
    oracle = O.AdamW([po], lr=ADAMW_LR, betas=ADAMW_BETAS, eps=ADAMW_EPS, weight_decay=wd)
    if start == "late":
        opt.state[p] = {"step": torch.tensor(999.0), "exp_avg": c["m"].double().clone(), "exp_avg_sq": c["v"].double().clone()}
        oracle.state[id(po)] = {"t": 999, "m": c["m"].double().clone(), "v": c["v"].double().clone()}
    for g, ref in zip(c["grads"], adamw_run(c, case)):
        p.grad = g.double() * gs
        po.grad = g.double() * gs
        opt.step()
        oracle.step()
        _pin(ref[0], p.detach(), "p")
        _pin(ref[0], po.detach(), "p (oracle)")
        _pin(ref[1], opt.state[p]["exp_avg"], "m")
        _pin(ref[2], opt.state[p]["exp_avg_sq"], "v")
    assert int(opt.state[p]["step"]) == c["first_step"] + len(c["grads"]) - 1


# ----------------------------------------------------------------------------------------
# the tables and the builders themselves
# ----------------------------------------------------------------------------------------
def test_dispatch_constants_match_the_source():
    src = open(os.path.join(CSRC, "pointwise.hip")).read()
    sites = read_launch_sites(src)
    for k, (per, cap) in LAUNCH.items():
        assert sites.get(k) == (per, cap, BLOCK), (k, sites.get(k))
    assert "const int nb = n > 0 ? grid_for(n, %d, %d) : 0;" % (LOSS_PER_BLOCK, LOSS_MAX_BLOCKS) in src
    assert "long faoctasr_loss_workspace_floats(void) { return %d; }" % LOSS_MAX_BLOCKS in src
    for line in ("hipLaunchKernelGGL(loss_partial_kernel, dim3(nb), dim3(256)", "hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256)",
                 "for (int i = threadIdx.x; i < np; i += 256) s += part[i];",
                 "long S = (%d + C - 1) / C;" % CSUM_BLOCKS, "const long maxs = (L + %d) / %d;" % (CSUM_MIN_RANGE - 1, CSUM_MIN_RANGE),
                 "per = (per + 3) & ~3L;", "S = (L + per - 1) / per;", "hipLaunchKernelGGL(channel_sum_kernel, dim3((unsigned)S, C), dim3(256)",
                 "for (long e = e0 + 4L * threadIdx.x; e < e1; e += 1024) {", "for (long e = e0 + threadIdx.x; e < e1; e += 256) {",
                 "hipLaunchKernelGGL(mean_mix_fwd_kernel, dim3(N), dim3(256)",
                 "hipLaunchKernelGGL(mean_mix_bwd_kernel, dim3(N), dim3(%d)" % MEAN_MIX_BWD_BLOCK,
                 "for (int i = threadIdx.x; i < La; i += 256) sa += a[(long)n * La + i];"):
        assert line in src, line
    # every kernel of the file that this pair covers has a launch site that was read, and no grid_for site is unknown here
    known = set(LAUNCH) | {"bn_eval_fwd_kernel", "bn_eval_bwd_kernel", "prep_crop_resize_kernel", "absmax_bits_kernel"}
    assert set(sites) == known, set(sites) ^ known


def covered_forms():
    got = set()
    for op, table in TABLES.items():
        for case in table:
            got |= forms(op, case)
    return got


def test_every_form_is_reached():
    got = covered_forms()
    assert got == FORMS, (sorted(FORMS - got), sorted(got - FORMS))
    # the forms that the tables' comments promise
    assert csum_split(12672, 2) == (4, 3168) and csum_split(5796, 2) == (2, 2900) and csum_split(19594, 1) == (5, 3920)
    assert csum_split(16, 1100) == (1, 16) and csum_split(189, 5) == (1, 192) and csum_split(1, 1) == (1, 4)
    assert [loss_blocks(n) for n in LOSS_N] == [1, 1, 1, 2, 257, 1024]
    assert forms("act", (ACT_PASS + 1031, "relu", 0.2)) == {"act: vector body", "act: scalar tail", "act: scalar tail, several blocks",
                                                            "act: second grid pass"}
    assert forms("act", (3, "relu", 0.2)) == {"act: n < 4", "act: scalar tail"} and forms("act", (4, "relu", 0.2)) == {"act: vector body"}
    assert "adamw: second grid pass" in forms("adamw", ADAMW_CASES[-1]) and "adamw: second grid pass" not in forms("adamw", (ACT_PASS // 2, "zero", 0, 1))
    assert forms("reflect", (1, 3, 2, 1)) >= {"reflect: both borders on one pixel"} and "reflect: both borders on one pixel" not in forms("reflect", (1, 2, 2, 1))
    assert "reflect: 9 terms" in forms("reflect", (1, 3, 3, 2)) and "reflect: 9 terms" in forms("reflect", (6, 4, 4, 3))
    for shape in CAT2_SHAPES[-1:]:
        assert shape[0] * (shape[1] + shape[2]) * shape[3] * shape[4] > FLAT_PASS
    # addition depth of every reduction case: below 112, so that 16 of GAMMA_SUM's 128 roundings remain for the terms themselves
    for op in ("loss", "mean_mix", "csum"):
        for case in TABLES[op]:
            assert depth(op, case) < 112, (op, case, depth(op, case))
    assert depth("loss", ("mse", LOSS_N[-1])) == 9 + 9 + 4 + 9 and depth("mean_mix", ((2, 4096, 900), (0.7, 0.3))) == 26
    assert depth("csum", ((2, 1, 97, 101), 1)) == 16 + 9 + 5 + 1 and depth("csum", ((3, 2, 64, 66), 0)) == 16 + 9 + 4


def test_spikes_sit_where_ranges_end():
    assert range_ends(10, [4, 8]).tolist() == [0, 3, 4, 7, 8, 9] and range_ends(1).tolist() == [0] and range_ends(3, [0]).tolist() == [0, 2]
    n = ACT_PASS + 1031
    c = build_act((n, "relu", 0.2))
    assert c["ends"].tolist() == [0, ACT_PASS - 1, ACT_PASS, n - 4, n - 3, n - 1]
    assert bool((c["x"][c["ends"]] == SPIKE).all()) and bool((c["cot"][c["ends"]] == SPIKE).all())
    c = build_csum(((2, 1, 97, 101), 0))
    assert c["ends"].tolist() == sorted({0, 19593} | {s * 3920 for s in range(1, 5)} | {s * 3920 - 1 for s in range(1, 5)})
    assert bool((c["dy"].permute(1, 0, 2, 3).reshape(1, -1)[:, c["ends"]] == SPIKE).all())
    c = build_adamw(ADAMW_CASES[-1])
    assert ADAMW_PASS in c["ends"].tolist() and ADAMW_PASS - 1 in c["ends"].tolist() and float(c["grads"][0][0]) * 0.125 == SPIKE
    c = build_loss(("l1", 524289))
    assert 257 * 256 in c["ends"].tolist() and not bool(c["tie"][c["ends"]].any()) and bool((c["a"][c["tie"]] == c["b"][c["tie"]]).all())
    assert 0.03 < float(c["tie"].float().mean()) < 0.07


# ----------------------------------------------------------------------------------------
# the fp32 restatement meets the bars on every case: a bar that no fp32 evaluation can meet is found here, not on the GPU
# ----------------------------------------------------------------------------------------
def run_fp32(op, case, dtype=torch.float32):
    """(reference, restatement in ``dtype``, bars) of a case; tests/test_gpu_pointwise.py reports the fp32 one as e_ref."""
    if op == "act":
        c = build_act(case)
        return act_ref(c, case[1], case[2]), act_ref(c, case[1], case[2], dtype), act_bars(case[1])
    if op == "cat2":
        c = build_cat2(case)
        return cat2_ref(c, case[1], SLOPE), cat2_ref(c, case[1], SLOPE, dtype), cat2_bars(case[1])
    if op == "axpby":
        c = build_axpby(case)
        return axpby_ref(c, case[1], case[2]), axpby_ref(c, case[1], case[2], dtype), AXPBY_BARS
    if op == "csum":
        c = build_csum(case)
        return csum_ref(c, case[1]), csum_ref(c, case[1], dtype), CSUM_BARS
    if op == "reflect":
        c = build_reflect(case)
        return reflect_fold_ref(c, case[3]), reflect_fold_ref(c, case[3], dtype), REFLECT_BARS
    if op == "haar":
        c = build_haar(case)
        shape, bands = case
        l_, h_ = (None if bands == "hi only" else c["ll"]), (None if bands == "ll only" else c["hi"])
        out = []
        for dt in (torch.float64, dtype):
            d = haar_fwd_ref(c["x"], dt)
            d.update(haar_inv_ref(l_, h_, shape, dt))
            out.append(d)
        return out[0], out[1], HAAR_BARS
    if op == "dfront":
        c = build_dfront(case)
        return dfront_ref(c, case[1]), dfront_ref(c, case[1], dtype), dfront_bars(case[1])
    if op == "freq":
        c = build_freq(case)
        return freq_mix_ref(c, case[1]), freq_mix_ref(c, case[1], dtype), FREQ_BARS
    if op == "loss":
        c = build_loss(case)
        return loss_ref(c, case[0]), loss_ref(c, case[0], dtype), loss_bars(case[0])
    if op == "mean_mix":
        c = build_mean_mix(case)
        return mean_mix_ref(c, *case[1]), mean_mix_ref(c, *case[1], dtype), MEAN_MIX_BARS
    raise KeyError(op)


CHECKED = [(op, case) for op in ("act", "cat2", "axpby", "csum", "reflect", "haar", "dfront", "freq", "loss", "mean_mix") for case in TABLES[op]]


@pytest.mark.parametrize("op,case", CHECKED, ids=[ident(op, case) for (op, case) in CHECKED])
def test_fp32_restatement_meets_the_bars(op, case):
    ref, got, bars = run_fp32(op, case)
    assert_bars(ident(op, case), got, ref, bars)


@pytest.mark.parametrize("case", ADAMW_CASES, ids=[ident("adamw", c) for c in ADAMW_CASES])
def test_fp32_adamw_restatement_meets_the_bars(case):
    c = build_adamw(case)
    adamw_assert(ident("adamw", case), adamw_run(c, case, torch.float32, True), adamw_run(c, case), adamw_run(c, case, round_scalars=True))


# ----------------------------------------------------------------------------------------
# the operators' host-side checks: mismatched operands and a negative LeakyReLU slope are refused before anything is launched
# ----------------------------------------------------------------------------------------
def mismatched_calls(ops, make):
    """(what, call, pattern of the error) for every host check; ``make(*shape)`` builds an operand."""
    t = make
    return [
        ("cat2_act N", lambda: ops.cat2_act(t(2, 3, 4, 4), t(3, 3, 4, 4)), "agree in N, H and W"),
        ("cat2_act H", lambda: ops.cat2_act(t(2, 3, 4, 4), t(2, 5, 6, 4)), "agree in N, H and W"),
        ("cat2_act W", lambda: ops.cat2_act(t(2, 3, 4, 4), t(2, 5, 4, 2), "relu"), "agree in N, H and W"),
        ("cat2_act rank", lambda: ops.cat2_act(t(2, 3, 4, 4), t(2, 3, 16)), "agree in N, H and W"),
        ("mean_mix", lambda: ops.mean_mix(t(3, 1, 6, 6), t(2, 1, 2, 2)), "differ in batch size"),
        ("add", lambda: ops.add(t(2, 3, 4, 4), t(2, 3, 4, 3)), "add operands differ in shape"),
        ("add numel", lambda: ops.add(t(4, 6), t(6, 4)), "add operands differ in shape"),
        ("axpby", lambda: ops.axpby(t(17), t(16), 0.7, -0.3), "axpby operands differ in shape"),
        ("activation", lambda: ops.activation(t(2, 3, 4, 4), "lrelu", -0.1), "slope must be >= 0"),
        ("activation nan", lambda: ops.activation(t(2, 3, 4, 4), "lrelu", float("nan")), "slope must be >= 0"),
        ("cat2_act slope", lambda: ops.cat2_act(t(2, 3, 4, 4), t(2, 1, 4, 4), "lrelu", -0.1), "slope must be >= 0"),
        ("conv2d", lambda: ops.conv2d(t(1, 2, 6, 6), t(3, 2, 3, 3), None, 1, 1, False, "lrelu", -0.2), "slope must be >= 0"),
        ("conv_transpose2d", lambda: ops.conv_transpose2d(t(1, 2, 6, 6), t(2, 3, 4, 4), None, 2, 1, 0, "lrelu", -0.2), "slope must be >= 0"),
        ("batchnorm_train", lambda: ops.batchnorm_train(t(2, 3, 4, 4), t(3), t(3), act="lrelu", slope=-0.2), "slope must be >= 0"),
        ("batchnorm_eval", lambda: ops.batchnorm_eval(t(2, 3, 4, 4), t(3), t(3), t(3), t(3), act="lrelu", slope=-0.2), "slope must be >= 0"),
        ("instance_norm", lambda: ops.instance_norm(t(2, 3, 4, 4), act="lrelu", slope=-0.2), "slope must be >= 0"),
    ]


def refuse_launches(monkeypatch, ops):
    """Any kernel launch through the operators' entry points fails the test."""
    def launched(name, *a, **k):
        raise AssertionError("faoctasr_%s was launched" % (name,))
    monkeypatch.setattr(ops, "call", launched)
    monkeypatch.setattr(ops, "_producer_call", launched)
    monkeypatch.setattr(ops, "_conv_call", launched)


def test_mismatched_operands_and_negative_slopes_are_refused_on_the_host(monkeypatch):
    import faoctasr
    ops = faoctasr.ops
    refuse_launches(monkeypatch, ops)
    made = []

    def make(*shape):
        made.append(torch.randn(*shape))
        return made[-1]
    for what, fn, pattern in mismatched_calls(ops, make):
        with pytest.raises(faoctasr._lib.KernelError, match=pattern):
            fn()
    # the slope is only read by LeakyReLU, and 0 is a valid one: these pass the check and stop at the CPU operand instead
    for fn in (lambda: ops.activation(make(5), "relu", -0.1), lambda: ops.activation(make(5), "tanh", -0.1),
               lambda: ops.activation(make(5), "lrelu", 0.0), lambda: ops.cat2_act(make(1, 1, 2, 2), make(1, 2, 2, 2), None, -1.0)):
        with pytest.raises(faoctasr._lib.KernelError, match="no CPU/eager fallback"):
            fn()
