"""BatchNorm2d (training and inference statistics) and InstanceNorm2d without a GPU: a plain float64 restatement of what
csrc/norm.hip and the bn_eval kernels of csrc/pointwise.hip compute, written with elementwise torch ops and sums, pinned here to
``torch.nn.functional.batch_norm`` / ``instance_norm`` plus autograd in float64 at 1e-12 relative.  tests/test_gpu_norm.py
measures every kernel form against this restatement and takes its case tables and its input builders from this file, so both
files see the same data.

Per row (BatchNorm: a channel, L = N*H*W elements gathered from N images; InstanceNorm: one (n, c) map, L = H*W), with
g = cotangent * act'(.):
    mean = sum x / L        var = sum (x - mean)^2 / L        invstd = 1 / sqrt(var + eps)        xhat = (x - mean) * invstd
    y = act(xhat * gamma + beta [+ residual])
    running_mean' = (1 - m) running_mean + m mean             running_var' = (1 - m) running_var + m var L / (L - 1)
    s1 = sum g (dbeta)      s2 = sum g * xhat (dgamma)        dx = gamma * invstd * (g - s1 / L - xhat * s2 / L)     dres = g
InstanceNorm sums s1 and s2 over the N rows of a channel.  Every reduced quantity comes with the sum of the absolute values of its
addends: the GPU tests' bar for a reduction is a multiple of that sum (the first-order rounding bound of an fp32 summation).
The kernels accumulate the statistics around a per-row shift (the row's first element), so the mean's addends are x - shift.

The dispatch of csrc/norm.hip (which kernel form a shape reaches, and the split of a row into ranges) is restated here too, and
its constants are read back from the source, so that a changed threshold fails here instead of silently un-testing a form."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frequency-aware-inverse-consistent-octa-super-resolution_amd", "csrc")
SLOPE = 0.2
EPS = 1e-5
SPIKE = 40.0
KINK = 1e-4                      # ReLU / LeakyReLU: cotangents are zeroed where the float64 pre-activation is this close to 0
PIN = 1e-12


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def act_apply(v, act):
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == "lrelu":
        return torch.where(v > 0, v, v * SLOPE)
    if act == "tanh":
        return torch.tanh(v)
    assert act is None
    return v


def act_grad(pre, out, act):
    if act == "relu":
        return (pre > 0).to(pre.dtype)
    if act == "lrelu":
        return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))
    if act == "tanh":
        return 1 - out * out
    return torch.ones_like(pre)


def _per_channel(v, C, dtype):
    return None if v is None else v.to(dtype).reshape(1, C, 1, 1)


def norm_ref(x, gamma=None, beta=None, res=None, act=None, cot=None, instance=False, rmean=None, rvar=None, momentum=0.1, eps=EPS,
             dtype=torch.float64):
    """Training-mode BatchNorm2d (``instance=False``) or InstanceNorm2d of an (N, C, H, W) tensor in ``dtype``.  Statistics have
    one entry per row: C for BatchNorm, N*C (row n*C + c) for InstanceNorm.  With ``cot`` the gradients are returned as well."""
    x = x.to(dtype)
    N, C, H, W = x.shape
    dims = (2, 3) if instance else (0, 2, 3)
    L = H * W if instance else N * H * W
    g_, b_ = _per_channel(gamma, C, dtype), _per_channel(beta, C, dtype)
    mean = x.sum(dims, keepdim=True) / L
    shift = x[:, :, :1, :1] if instance else x[:1, :, :1, :1]            # the row's first element
    xc = x - mean
    var = (xc * xc).sum(dims, keepdim=True) / L
    invstd = 1 / torch.sqrt(var + eps)
    xhat = xc * invstd
    pre = xhat
    if g_ is not None:
        pre = pre * g_
    if b_ is not None:
        pre = pre + b_
    if res is not None:
        pre = pre + res.to(dtype)
    y = act_apply(pre, act)
    out = {"y": y, "pre": pre, "xhat": xhat, "L": L, "save_mean": mean.reshape(-1), "save_invstd": invstd.reshape(-1),
           "var": var.reshape(-1), "abs_mean": ((x - shift).abs().sum(dims) / L).reshape(-1)}
    if rmean is not None:
        out["rmean"] = (1 - momentum) * rmean.to(dtype) + momentum * mean.reshape(-1)
        out["rvar"] = (1 - momentum) * rvar.to(dtype) + momentum * var.reshape(-1) * (L / (L - 1))
    if cot is not None:
        g = cot.to(dtype) * act_grad(pre, y, act)
        t2 = g * xhat
        s1, s2 = g.sum(dims, keepdim=True), t2.sum(dims, keepdim=True)
        dx = invstd * (g - s1 / L - xhat * (s2 / L))
        if g_ is not None:
            dx = dx * g_
        csum = (lambda v: v.sum(0).reshape(-1)) if instance else (lambda v: v.reshape(-1))      # over the N rows of a channel
        out.update(dx=dx, dbeta=csum(s1), dgamma=csum(s2), abs_dbeta=csum(g.abs().sum(dims, keepdim=True)),
                   abs_dgamma=csum(t2.abs().sum(dims, keepdim=True)))
        if res is not None:
            out["dres"] = g
    return out


def bn_eval_ref(x, gamma, beta, rmean, rvar, act=None, cot=None, eps=EPS, dtype=torch.float64):
    """Inference-mode BatchNorm2d: y = act(gamma (x - running_mean) / sqrt(running_var + eps) + beta), and its dx."""
    x = x.to(dtype)
    C = x.shape[1]
    sc = 1 / torch.sqrt(_per_channel(rvar, C, dtype) + eps)
    if gamma is not None:
        sc = sc * _per_channel(gamma, C, dtype)
    pre = (x - _per_channel(rmean, C, dtype)) * sc
    if beta is not None:
        pre = pre + _per_channel(beta, C, dtype)
    y = act_apply(pre, act)
    out = {"y": y, "pre": pre}
    if cot is not None:
        out["dx"] = cot.to(dtype) * act_grad(pre, y, act) * sc
    return out


# ----------------------------------------------------------------------------------------
# the dispatch of csrc/norm.hip, restated
# ----------------------------------------------------------------------------------------
BN_SMALL_FWD, BN_SMALL_BWD, BN_MAX_SPLIT = 16384, 8192, 64


def norm_split(L, R):
    """(S, per) of norm.hip's norm_split: a row of L elements is cut into S ranges [s*per, (s+1)*per)."""
    want = (2048 + R - 1) // R
    maxs = (L + 4095) // 4096
    s = max(1, min(want, maxs, BN_MAX_SPLIT))
    per = (L + s - 1) // s
    per = (per + 3) & ~3
    return (L + per - 1) // per, per


def rows_of(shape, instance):
    """(R, L, HW): rows, elements per row, map size."""
    N, C, H, W = shape
    return (N * C, H * W, H * W) if instance else (C, N * H * W, H * W)


def forms(shape, act, res, instance=False):
    """The kernels of norm.hip that one forward + backward call of this case launches, plus tags for the split's regimes."""
    R, L, HW = rows_of(shape, instance)
    S, _ = norm_split(L, R)
    vec = HW % 4 == 0
    has_y = act == "tanh" or (act is not None and res)                  # ops.py keeps y for these; otherwise y == NULL
    out = set()
    if vec and L <= BN_SMALL_FWD:
        out.add("norm_fwd_small_kernel<%d>" % (4 if L <= 4096 else 8 if L <= 8192 else 16))
    elif vec:
        out |= {"norm_stats_kernel", "norm_apply_kernel"}
    else:
        out |= {"norm_stats_generic_kernel", "norm_apply_generic_kernel"}
    if vec and L <= BN_SMALL_BWD:
        out.add("norm_bwd_small_kernel<%d>" % (4 if L <= 4096 else 8))
    elif vec:
        tag = "true" if has_y else "false"
        out |= {"norm_bwd_reduce_kernel<%s>" % tag, "norm_bwd_dx_kernel<%s>" % tag}
    else:
        out |= {"norm_bwd_reduce_generic_kernel", "norm_bwd_dx_generic_kernel"}
    if not (vec and L <= BN_SMALL_BWD):
        if not vec and S > 1:
            out.add("generic, S > 1")
        if vec and S > 1:
            out.add("streaming, S > 1")
        if S == BN_MAX_SPLIT:
            out.add("split cap")
    if R > 2048:
        out.add("R > 2048")
    if instance and shape[0] > 1:
        out.add("atomic dgamma over N rows")
    return out


NORM_KERNELS = {"norm_fwd_small_kernel<4>", "norm_fwd_small_kernel<8>", "norm_fwd_small_kernel<16>", "norm_bwd_small_kernel<4>",
                "norm_bwd_small_kernel<8>", "norm_stats_kernel", "norm_apply_kernel", "norm_bwd_reduce_kernel<true>",
                "norm_bwd_reduce_kernel<false>", "norm_bwd_dx_kernel<true>", "norm_bwd_dx_kernel<false>", "norm_stats_generic_kernel",
                "norm_apply_generic_kernel", "norm_bwd_reduce_generic_kernel", "norm_bwd_dx_generic_kernel"}
REGIMES = {"generic, S > 1", "streaming, S > 1", "split cap", "R > 2048", "atomic dgamma over N rows"}

# ----------------------------------------------------------------------------------------
# the case tables (N, C, H, W); a case's seed is its position in its table
# ----------------------------------------------------------------------------------------
BN_SHAPES = [
    (1, 3, 64, 64),          # L 4096: top of K = 4, every thread's last chunk is live
    (1, 3, 41, 100),         # L 4100: first size past K = 4, nearly every second chunk dead
    (2, 5, 64, 64),          # L 8192: top of the small backward
    (1, 3, 12, 683),         # L 8196: forward K = 16, first streaming backward
    (4, 3, 64, 64),          # L 16384: top of the small forward
    (1, 3, 34, 482),         # L 16388: first streaming forward
    (3, 4, 44, 31),          # L 4092: chunks cross image boundaries
    (3, 3, 76, 76),          # L 17328: S = 5, per = 3468, ranges cross image boundaries mid-image
    (2048, 3, 2, 2),         # HW = 4: image index up to 2047 from the float reciprocal
    (4096, 2, 2, 2),         # HW = 4, streaming backward: one piece per image
    (3, 5, 45, 43),          # L 5805, odd HW: generic, S = 2, per = 2904
    (1, 2, 65, 67),          # L 4355: generic, one image, S = 2
    (4, 8, 256, 256),        # L 262144: the split cap S = 64 (the only large case)
    (2, 2100, 4, 4),         # R > 2048 rows (want = 1), L = 32: many blocks with mostly dead chunks
]
BN_CONFIGS = [(None, False), ("relu", False), ("lrelu", True), ("tanh", False)]       # (activation, residual)
BN_CASES = [(s, a, r) for s in BN_SHAPES for (a, r) in BN_CONFIGS]
# (what, shape, act, res) on one small-row and one streaming shape
BN_VARIANTS = [(w, s, a, r) for s in [(3, 4, 44, 31), (3, 3, 76, 76)]
               for (w, a, r) in [("no_affine", "relu", False), ("no_running", "lrelu", True), ("momentum", None, False), ("noncontig", "lrelu", True)]]
ACC_SHAPES = [(3, 4, 44, 31), (3, 3, 76, 76), (3, 5, 45, 43)]                       # small-row, streaming, generic
IN_SHAPES = [(3, 6, 12, 8), (4, 3, 64, 128), (2, 3, 132, 128), (3, 2, 65, 67), (5, 7, 4, 4)]
# (shape, act, affine)
IN_CASES = [(s, a, True) for s in IN_SHAPES for a in ("relu", None)] + [((2, 3, 132, 128), "tanh", True), ((4, 3, 64, 128), "relu", False)]
EVAL_SHAPES = [(3, 7, 5, 3), (2, 64, 24, 24), (2, 5, 330, 330)]                     # the last: more elements than one grid pass covers
EVAL_CASES = [(s, a, True) for s in EVAL_SHAPES for a in (None, "relu", "lrelu", "tanh")] + [((2, 64, 24, 24), "lrelu", False)]
EVAL_GRID_PASS = 4096 * 256                                                          # pointwise.hip grid_for: at most 4096 blocks of 256
STAT_SHAPES = [(4, 3, 64, 64), (1, 3, 34, 482)]                                      # x = 0.01 randn + 100: small-row and streaming
DETERMINISM_SHAPE = (3, 3, 76, 76)


def case_id(shape, act=None, res=False, what=None):
    return "x".join(map(str, shape)) + "_" + (act or "none") + ("_res" if res else "") + ("_" + what if what else "")


def covered_forms():
    got = set()
    for shape, act, res in BN_CASES:
        got |= forms(shape, act, res)
    for shape, act, _ in IN_CASES:
        got |= forms(shape, act, False, instance=True)
    return got


def assert_forms_covered():
    """Every kernel of norm.hip (both HAS_Y instantiations, every K) and every regime of the split is reached by a case."""
    got = covered_forms()
    if any(a is not None for (_, a, _) in EVAL_CASES):                  # forward, and a backward that reads the mask
        got |= {"bn_eval_fwd_kernel", "bn_eval_bwd_kernel"}
    missing = (NORM_KERNELS | REGIMES | {"bn_eval_fwd_kernel", "bn_eval_bwd_kernel"}) - got
    assert not missing, "no case reaches %s" % sorted(missing)


# ----------------------------------------------------------------------------------------
# input builders (fp32 CPU tensors; the same in every process)
# ----------------------------------------------------------------------------------------
def spike_mask(shape, instance, for_x):
    """Positions where row ranges end: the last element of every row and of every image, the first and last element of every
    split range.  Element 0 of a row is never spiked in x: it is the kernels' variance shift."""
    N, C, H, W = shape
    R, L, HW = rows_of(shape, instance)
    S, per = norm_split(L, R)
    e = torch.zeros(L, dtype=torch.bool)
    e[L - 1] = True
    every = -(-64 // HW)             # every image while H*W >= 64; below that every 64/(H*W)-th one: see spikes_are_outliers
    e[every * HW - 1::every * HW] = True
    for s in range(S):
        e[s * per] = True
        e[min((s + 1) * per, L) - 1] = True
    if for_x:
        e[0] = False
    m = e.reshape(1, 1, H, W) if instance else e.reshape(N, 1, H, W)
    return m.expand(N, C, H, W).clone()


def spikes_are_outliers(shape, instance):
    """At most one element in 32 of a row is a spike.  Denser spikes carry the row's mean and variance themselves: dx at a spike,
    gamma invstd (40 - m1 - xhat m2), is then the small residue of a projection whose two means the spikes dominate, and
    xhat gamma + beta + residual at a spike is of order 1 and can land near 0.  No fp32 evaluation is within rtol alone of such a
    value (test_fp32_restatement_meets_the_bars fails if asked to), so
      * with H*W < 64 only every 64/(H*W)-th image end is spiked (H*W = 4 with every image end spiked makes every fourth element
        a spike, ReLU then zeroes every other element's cotangent and ALL of dx is cancellation residue: the float32 restatement
        on the CPU is 1.9e-4 in relative L2 from float64 there), and
      * rows that still are denser (the 32-element rows of 2 x 2100 x 4 x 4: two spikes) are compared like spike-free ones: rtol
        plus the spike-free atol at every position."""
    _, L, _ = rows_of(shape, instance)
    m = spike_mask(shape, instance, False)
    return 32 * int(m[0, 0].sum() if instance else m[:, 0].sum()) <= L


def build_case(shape, act, res, seed, instance=False, affine=True, spikes=True, x_scale=2.0, x_offset=0.7):
    """x = x_scale randn + x_offset; cotangent = randn + 0.5 + 0.3 xhat (xhat from the float64 restatement: the backward means stay
    away from zero); spikes of 40 in both where ranges end; ReLU / LeakyReLU: zero cotangent where the pre-activation is within
    1e-4 of 0 (there the derivative may take either branch on either side)."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * x_scale + x_offset
    gamma = torch.randn(C, generator=g) * 0.1 + 1 if affine else None
    beta = torch.randn(C, generator=g) * 0.1 if affine else None
    r = torch.randn(shape, generator=g) if res else None
    rmean, rvar = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    noise = torch.randn(shape, generator=g)
    mx = spike_mask(shape, instance, True) if spikes else torch.zeros(shape, dtype=torch.bool)
    mc = spike_mask(shape, instance, False) if spikes else mx
    x[mx] = SPIKE
    fwd = norm_ref(x, gamma, beta, r, act, instance=instance)
    cot = (noise.double() + 0.5 + 0.3 * fwd["xhat"]).float()
    cot[mc] = SPIKE
    if act in ("relu", "lrelu"):
        cot = cot * (fwd["pre"].abs() > KINK)
    return {"x": x, "gamma": gamma, "beta": beta, "res": r, "cot": cot, "rmean": rmean, "rvar": rvar, "spikes": mx,
            "rtol_only": mx if spikes_are_outliers(shape, instance) else torch.zeros(shape, dtype=torch.bool)}


def build_eval_case(shape, act, affine, seed):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 2 + 0.7
    gamma = torch.randn(C, generator=g) * 0.1 + 1 if affine else None
    beta = torch.randn(C, generator=g) * 0.1 if affine else None
    rmean, rvar = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.1
    cot = torch.randn(shape, generator=g) + 0.5
    spikes = torch.zeros(shape, dtype=torch.bool)
    spikes.view(-1)[-1] = True                                            # the last element the grid-stride loop reaches
    x[spikes] = SPIKE
    cot[spikes] = SPIKE
    if act in ("relu", "lrelu"):
        cot = cot * (bn_eval_ref(x, gamma, beta, rmean, rvar, act)["pre"].abs() > KINK)
    return {"x": x, "gamma": gamma, "beta": beta, "rmean": rmean, "rvar": rvar, "cot": cot, "spikes": spikes, "rtol_only": spikes}


# ----------------------------------------------------------------------------------------
# the bars (tests/test_gpu_norm.py derives them in its docstring)
# ----------------------------------------------------------------------------------------
GAMMA_SUM = 128 * 2.0 ** -24
BARS = {"y": (1e-4, 2e-5), "dx": (2e-3, 2e-4), "dres": (1e-5, 1e-6)}             # rtol, atol of test_gpu_ops.test_batchnorm_train
DX_REL_L2 = 1e-4


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def ulp32(v):
    """Spacing of fp32 at |v| (float64 tensor in, float64 tensor out)."""
    f = v.abs().float().clamp_min(2.0 ** -126)
    return (torch.nextafter(f, torch.full_like(f, float("inf"))) - f).double()


def elementwise_violations(got, ref, spikes, rtol_only, rtol, atol):
    """|got - ref| <= rtol |ref| + atol * (RMS of the reference away from the spikes); at ``rtol_only`` positions (the spikes,
    where they are outliers) rtol alone.  Returns (count, worst excess)."""
    got, ref = got.detach().cpu().double(), ref.double()
    free = ref[~spikes]
    scale = float(free.pow(2).mean().sqrt()) if free.numel() else 0.0
    tol = rtol * ref.abs() + (~rtol_only).double() * (atol * scale)
    err = (got - ref).abs()
    bad = ~(err <= tol)                                                  # a NaN is a violation
    worst = float((err - tol).max())
    return int(bad.sum()), worst


def sum_violations(got, ref, abs_terms):
    """|got - ref| <= GAMMA_SUM * sum |terms| + 2 ulp_fp32(ref)."""
    got, ref = got.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    tol = GAMMA_SUM * abs_terms.double().reshape(-1) + 2 * ulp32(ref)
    err = (got - ref).abs()
    return int((~(err <= tol)).sum()), float((err / tol).max())


# ----------------------------------------------------------------------------------------
# the pin: restatement against torch in float64
# ----------------------------------------------------------------------------------------
def _pin(a, b, what):
    assert rel_l2(a, b) <= PIN, (what, rel_l2(a, b))


def _torch_act(v, act):
    return {None: lambda t: t, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, SLOPE), "tanh": torch.tanh}[act](v)


PIN_BN = [((3, 7, 5, 3), None, False, True), ((2, 4, 6, 8), "relu", False, True), ((3, 3, 9, 5), "lrelu", True, True),
          ((2, 5, 4, 4), "tanh", False, True), ((2, 3, 7, 6), "relu", False, False)]


@pytest.mark.parametrize("shape,act,res,affine", PIN_BN)
def test_batchnorm_restatement_is_torch_float64(shape, act, res, affine):
    c = build_case(shape, act, res, 100 + PIN_BN.index((shape, act, res, affine)), affine=affine)
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta", "res") if d[k] is not None}
    rm, rv = d["rmean"].clone(), d["rvar"].clone()
    out = F.batch_norm(leaves["x"], rm, rv, leaves.get("gamma"), leaves.get("beta"), True, 0.3, EPS)
    if res:
        out = out + leaves["res"]
    out = _torch_act(out, act)
    out.backward(d["cot"])
    ref = norm_ref(c["x"], c["gamma"], c["beta"], c["res"], act, c["cot"], rmean=c["rmean"], rvar=c["rvar"], momentum=0.3)
    _pin(ref["y"], out, "y")
    _pin(ref["rmean"], rm, "running_mean")
    _pin(ref["rvar"], rv, "running_var")
    _pin(ref["save_mean"], d["x"].mean((0, 2, 3)), "save_mean")
    _pin(ref["save_invstd"], 1 / torch.sqrt(d["x"].var((0, 2, 3), unbiased=False) + EPS), "save_invstd")
    _pin(ref["dx"], leaves["x"].grad, "dx")
    if affine:
        _pin(ref["dgamma"], leaves["gamma"].grad, "dgamma")
        _pin(ref["dbeta"], leaves["beta"].grad, "dbeta")
    if res:
        _pin(ref["dres"], leaves["res"].grad, "dres")
    # the absolute sums bound their sums, and reduce to them when every addend has one sign
    assert bool((ref["abs_dbeta"] >= ref["dbeta"].abs() * (1 - 1e-12)).all()) and bool((ref["abs_dgamma"] >= ref["dgamma"].abs() * (1 - 1e-12)).all())
    pos = norm_ref(c["x"].abs() + 1, None, None, None, None, c["cot"].abs())
    _pin(pos["abs_dbeta"], pos["dbeta"], "abs_dbeta")
    shift = d["x"][:1, :, :1, :1]
    _pin(ref["abs_mean"], (d["x"] - shift).abs().mean((0, 2, 3)), "abs_mean")


PIN_IN = [((3, 6, 12, 8), "relu", True), ((2, 3, 5, 7), None, True), ((4, 2, 6, 6), "tanh", True), ((3, 4, 4, 4), "lrelu", False)]


@pytest.mark.parametrize("shape,act,affine", PIN_IN)
def test_instancenorm_restatement_is_torch_float64(shape, act, affine):
    c = build_case(shape, act, False, 200 + PIN_IN.index((shape, act, affine)), instance=True, affine=affine)
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta") if d[k] is not None}
    out = _torch_act(F.instance_norm(leaves["x"], weight=leaves.get("gamma"), bias=leaves.get("beta"), eps=EPS), act)
    out.backward(d["cot"])
    ref = norm_ref(c["x"], c["gamma"], c["beta"], None, act, c["cot"], instance=True)
    _pin(ref["y"], out, "y")
    _pin(ref["save_mean"], d["x"].mean((2, 3)).reshape(-1), "save_mean")
    _pin(ref["save_invstd"], (1 / torch.sqrt(d["x"].var((2, 3), unbiased=False) + EPS)).reshape(-1), "save_invstd")
    _pin(ref["dx"], leaves["x"].grad, "dx")
    if affine:
        assert ref["dgamma"].shape == (shape[1],)
        _pin(ref["dgamma"], leaves["gamma"].grad, "dgamma")
        _pin(ref["dbeta"], leaves["beta"].grad, "dbeta")


@pytest.mark.parametrize("shape,act,affine", [((3, 7, 5, 3), None, True), ((2, 4, 6, 8), "relu", True), ((2, 3, 4, 5), "lrelu", False),
                                              ((1, 5, 3, 3), "tanh", True)])
def test_batchnorm_eval_restatement_is_torch_float64(shape, act, affine):
    c = build_eval_case(shape, act, affine, 300 + shape[1])
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    xl = d["x"].clone().requires_grad_(True)
    out = _torch_act(F.batch_norm(xl, d["rmean"], d["rvar"], d["gamma"], d["beta"], False, 0.1, EPS), act)
    out.backward(d["cot"])
    ref = bn_eval_ref(c["x"], c["gamma"], c["beta"], c["rmean"], c["rvar"], act, c["cot"])
    _pin(ref["y"], out, "y")
    _pin(ref["dx"], xl.grad, "dx")


# ----------------------------------------------------------------------------------------
# the tables and the builders themselves
# ----------------------------------------------------------------------------------------
def test_dispatch_constants_match_the_source():
    src = open(os.path.join(CSRC, "norm.hip")).read()
    assert int(re.search(r"#define BN_SMALL_FWD (\d+)", src).group(1)) == BN_SMALL_FWD
    assert int(re.search(r"#define BN_SMALL_BWD (\d+)", src).group(1)) == BN_SMALL_BWD
    assert int(re.search(r"constexpr int BN_MAX_SPLIT = (\d+);", src).group(1)) == BN_MAX_SPLIT
    for line in ("if (L <= 4096) go(norm_fwd_small_kernel<4>);", "else if (L <= 8192) go(norm_fwd_small_kernel<8>);",
                 "if (L <= 4096) go(norm_bwd_small_kernel<4>);", "long want = (2048 + R - 1) / R;", "long maxs = (L + 4095) / 4096;"):
        assert line in src, line
    for k in NORM_KERNELS:
        assert re.search(r"\b%s\b" % k.split("<")[0], src), k
    assert "grid_for(total, 1024)" in open(os.path.join(CSRC, "pointwise.hip")).read()


def test_every_kernel_form_is_reached():
    assert_forms_covered()
    # and the forms that the table's comments promise
    assert norm_split(17328, 3) == (5, 3468) and norm_split(5805, 5) == (2, 2904) and norm_split(262144, 8)[0] == BN_MAX_SPLIT
    assert norm_split(4355, 2)[0] == 2 and norm_split(32, 2100) == (1, 32) and norm_split(4355, 6)[0] == 2
    assert forms((1, 3, 12, 683), "relu", False) == {"norm_fwd_small_kernel<16>", "norm_bwd_reduce_kernel<false>", "norm_bwd_dx_kernel<false>",
                                                     "streaming, S > 1"}
    assert forms((2, 3, 132, 128), "tanh", False, instance=True) >= {"norm_stats_kernel", "norm_apply_kernel", "norm_bwd_reduce_kernel<true>"}
    assert max(s[0] * s[1] * s[2] * s[3] for s in EVAL_SHAPES) > EVAL_GRID_PASS
    for shape in ACC_SHAPES + STAT_SHAPES + [DETERMINISM_SHAPE] + [v[1] for v in BN_VARIANTS]:
        assert shape in BN_SHAPES


def test_spikes_sit_where_ranges_end():
    shape = (3, 3, 76, 76)
    mx, mc = spike_mask(shape, False, True), spike_mask(shape, False, False)
    ex, ec = mx[:, 0].reshape(-1), mc[:, 0].reshape(-1)
    want = {17327, 5775, 11551} | {s * 3468 for s in range(5)} | {s * 3468 - 1 for s in range(1, 5)}
    assert set(torch.nonzero(ec).reshape(-1).tolist()) == want and set(torch.nonzero(ex).reshape(-1).tolist()) == want - {0}
    assert bool((mx == mx[:, :1]).all())
    c = build_case(shape, "relu", False, 7)
    assert bool((c["x"][mx] == SPIKE).all()) and bool((c["cot"][mc] == SPIKE).all()) and not bool(c["x"][:, :, 0, 0].eq(SPIKE).any())
    mi = spike_mask((3, 2, 65, 67), True, False)[0, 0].reshape(-1)
    assert set(torch.nonzero(mi).reshape(-1).tolist()) == {0, 2179, 2180, 4354}


@pytest.mark.parametrize("shape,act,res", [c for c in BN_CASES if c[0] != (4, 8, 256, 256)], ids=lambda v: None)
def test_fp32_restatement_meets_the_bars(shape, act, res):
    """The bars are the ones the GPU tests apply; the float32 restatement on the CPU must pass them, or the inputs (spikes, kinks)
    would make them unreachable for any fp32 implementation."""
    c = build_case(shape, act, res, BN_CASES.index((shape, act, res)))
    ref = norm_ref(c["x"], c["gamma"], c["beta"], c["res"], act, c["cot"])
    got = norm_ref(c["x"], c["gamma"], c["beta"], c["res"], act, c["cot"], dtype=torch.float32)
    for k in ("y", "dx") + (("dres",) if res else ()):
        assert elementwise_violations(got[k], ref[k], c["spikes"], c["rtol_only"], *BARS[k])[0] == 0, k
    assert rel_l2(got["dx"], ref["dx"]) < DX_REL_L2
