"""Every kernel form of csrc/norm.hip (BatchNorm2d in training mode, InstanceNorm2d) and the inference-mode bn_eval kernels of
csrc/pointwise.hip on the GPU, at the sizes where the form changes, against the float64 restatement of tests/test_norm_cpu.py
(pinned there to torch in float64).  The case tables, the input builders and the bar helpers live in that file.

Inputs: x = 2 randn + 0.7; cotangent = randn + 0.5 + 0.3 xhat; a spike of 40 in both wherever a range ends (row, image, split
range -- ``spike_mask``), so a dropped or doubled element moves a sum by 40 (1600 in the squared sums); ReLU / LeakyReLU
cotangents are zero within 1e-4 of the kink.  Every buffer an operator allocates is filled with a finite sentinel (1.2345e30)
before the kernel runs (``sentinel_outputs``): an element that is never stored fails its comparison.

The bars -- none is tuned on the kernels:
  * y, dx, dres (and the inference-mode y, dx): those of test_gpu_ops.test_batchnorm_train, since every form evaluates the same
    expression per element: y rtol 1e-4 atol 2e-5; dx rtol 2e-3 atol 2e-4 and relative L2 < 1e-4; dres rtol 1e-5 atol 1e-6.
    The atol is multiplied by the RMS of the reference away from the spikes; at the spikes rtol alone applies (where the spikes
    are outliers: test_norm_cpu.spikes_are_outliers).
  * save_mean, running_mean: rtol 1e-5, atol 1e-6; save_invstd, running_var: rtol 1e-4.
  * reductions (dgamma, dbeta, and the mean as shift + sum (x - shift) / L):
        |got - ref64| <= gamma * sum |terms| + 2 ulp_fp32(ref64),    gamma = 128 * 2^-24.
    An fp32 sum in which no addend passes through more than D additions is within D 2^-24 sum |terms| of the exact sum (first
    order); the remaining 128 - D cover the roundings inside a term (xhat = (x - mean) * invstd, the product with g, the
    activation derivative).  D per form, from the code (block_sum_256 = 6 shuffle steps + 3 adds = 9):
        small rows, K chunks of 4 per thread    4 K + 9                         25 / 41 / 73 for K = 4 / 8 / 16
        streaming, ranges of ``per`` elements   4 ceil(per / 1024) + 4 (a piece per image can add a chunk) + 9 + S partials
                                                per <= 4100 in every case here: 29 + S, 93 at the cap S = 64
        generic                                 ceil(per / 256) + 9 + S          12 + 9 + 2 = 23 at per = 2904
        InstanceNorm                            + N atomic adds (N <= 5);  accumulate_affine: + 1
    so D <= 98 < 112 everywhere.  At L = 16388 the bound is about 0.1 for dbeta: one dropped spike (40) is far outside.
  * ``NORM_ERR <case> <array> e_ref e_hip ratio`` lines record the relative L2 of the kernels (e_hip) and of the restatement run in
    float32 on the CPU (e_ref) against float64; profiles/norm_error.txt keeps an MI355X run's.  Reported, not asserted: torch's
    CPU sums carry wider accumulators than the kernels."""
import contextlib

import pytest
import torch

from test_norm_cpu import (ACC_SHAPES, BARS, BN_CASES, BN_VARIANTS, DETERMINISM_SHAPE, DX_REL_L2, EPS, EVAL_CASES, IN_CASES, SLOPE,
                           STAT_SHAPES, assert_forms_covered, bn_eval_ref, build_case, build_eval_case, case_id, elementwise_violations,
                           forms, norm_ref, rel_l2, sum_violations)

pytestmark = pytest.mark.gpu

SENTINEL = 1.2345e30


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def dev(t):
    return None if t is None else t.cuda().contiguous()


def leaf(t):
    return None if t is None else dev(t).requires_grad_(True)


@contextlib.contextmanager
def sentinel_outputs():
    """Inside, every tensor that torch.empty / torch.empty_like hands out on the GPU (the operators' y, dx, dres, statistics and
    affine gradients) starts as the sentinel instead of as whatever the allocator had there."""
    real = torch.empty, torch.empty_like

    def filled(fn):
        def make(*a, **k):
            t = fn(*a, **k)
            if t.is_cuda and t.is_floating_point():
                t.fill_(SENTINEL)
            return t
        return make
    torch.empty, torch.empty_like = filled(real[0]), filled(real[1])
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real


def report(case, name, got, ref, ref32):
    e_ref, e_hip = rel_l2(ref32, ref), rel_l2(got, ref)
    print("NORM_ERR %-34s %-11s e_ref %.3e e_hip %.3e ratio %.3f" % (case, name, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf")))


def check_elementwise(case, name, got, ref, ref32, c, bar=None):
    report(case, name, got, ref[name], ref32[name])
    assert got.shape == ref[name].shape
    g = got.detach().cpu()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) < 1e29, "%s %s: an element was never stored" % (case, name)
    n, worst = elementwise_violations(g, ref[name], c["spikes"], c["rtol_only"], *(bar or BARS[name]))
    assert n == 0, "%s %s: %d elements outside the bar, worst excess %.3e" % (case, name, n, worst)
    if name == "dx":
        assert rel_l2(g, ref[name]) < DX_REL_L2, (case, rel_l2(g, ref[name]))


def check_stat(case, name, got, ref, ref32, rtol, atol):
    report(case, name, got, ref[name], ref32[name])
    g, r = got.detach().cpu().double().reshape(-1), ref[name].reshape(-1)
    bad = ~((g - r).abs() <= rtol * r.abs() + atol)
    assert not bool(bad.any()), "%s %s: %d rows outside rtol %g atol %g, worst %.3e" % (case, name, int(bad.sum()), rtol, atol,
                                                                                        float(((g - r).abs() / r.abs()).max()))


def check_sum(case, name, got, ref, ref32, abs_terms):
    report(case, name, got, ref[name], ref32[name])
    n, worst = sum_violations(got, ref[name], abs_terms)
    assert n == 0, "%s %s: %d sums outside gamma sum|terms| + 2 ulp, worst at %.2f of the bar" % (case, name, n, worst)


def check_forward_stats(case, stats, rm, rv, ref, ref32):
    check_stat(case, "save_mean", stats[0], ref, ref32, 1e-5, 1e-6)
    n, worst = sum_violations(stats[0], ref["save_mean"], ref["abs_mean"])
    assert n == 0, "%s save_mean: %d rows outside the summation bound, worst at %.2f of it" % (case, n, worst)
    check_stat(case, "save_invstd", stats[1], ref, ref32, 1e-4, 0.0)
    if rm is not None:
        check_stat(case, "rmean", rm, ref, ref32, 1e-5, 1e-6)
        check_stat(case, "rvar", rv, ref, ref32, 1e-4, 0.0)


def refs(c, act, res, instance=False, momentum=0.1, running=True):
    kw = dict(instance=instance, momentum=momentum)
    if running and not instance:
        kw.update(rmean=c["rmean"], rvar=c["rvar"])
    return tuple(norm_ref(c["x"], c["gamma"], c["beta"], c["res"] if res else None, act, c["cot"], dtype=dt, **kw)
                 for dt in (torch.float64, torch.float32))


def run_batchnorm(fa, case, c, act, res, momentum=0.1, running=True, noncontig=False, backward=True):
    ref, ref32 = refs(c, act, res, momentum=momentum, running=running)
    gd, bd, rd = leaf(c["gamma"]), leaf(c["beta"]), leaf(c["res"] if res else None)
    rm, rv = (dev(c["rmean"]), dev(c["rvar"])) if running else (None, None)
    W = c["x"].shape[3]
    if noncontig:                                   # a slice of a wider tensor: ops._c must make it contiguous
        wide = torch.full(c["x"].shape[:3] + (W + 3,), 7.0)
        wide[..., 2:2 + W] = c["x"]
        xd = leaf(wide)
        xin = xd[..., 2:2 + W]
        assert not xin.is_contiguous()
    else:
        xd = xin = leaf(c["x"])
    with sentinel_outputs():
        y, stats = fa.ops._BatchNormTrain.apply(xin, gd, bd, rd, rm, rv, float(momentum), EPS, fa.ops.act_code(act), SLOPE, None)
        torch.cuda.synchronize()
        check_elementwise(case, "y", y, ref, ref32, c)
        check_forward_stats(case, stats, rm, rv, ref, ref32)
        if not backward:
            return
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    dx = xd.grad
    if noncontig:
        assert float(dx[..., :2].abs().max()) == 0.0 and float(dx[..., 2 + W:].abs().max()) == 0.0
        dx = dx[..., 2:2 + W]
    check_elementwise(case, "dx", dx, ref, ref32, c)
    if gd is not None:
        check_sum(case, "dgamma", gd.grad, ref, ref32, ref["abs_dgamma"])
        check_sum(case, "dbeta", bd.grad, ref, ref32, ref["abs_dbeta"])
    if res:
        check_elementwise(case, "dres", rd.grad, ref, ref32, c)


@pytest.mark.parametrize("shape,act,res", BN_CASES, ids=[case_id(*c) for c in BN_CASES])
def test_batchnorm_train_forms(fa, shape, act, res):
    c = build_case(shape, act, res, BN_CASES.index((shape, act, res)))
    run_batchnorm(fa, "bn_" + case_id(shape, act, res), c, act, res)


@pytest.mark.parametrize("what,shape,act,res", BN_VARIANTS, ids=[case_id(s, a, r, w) for (w, s, a, r) in BN_VARIANTS])
def test_batchnorm_train_variants(fa, what, shape, act, res):
    """gamma = beta = None; no running statistics; another momentum; a non-contiguous x -- on a small-row and a streaming shape."""
    c = build_case(shape, act, res, 3000 + BN_VARIANTS.index((what, shape, act, res)), affine=what != "no_affine")
    run_batchnorm(fa, "bn_" + case_id(shape, act, res, what), c, act, res, momentum=0.3 if what == "momentum" else 0.1,
                  running=what != "no_running", noncontig=what == "noncontig")


def test_every_kernel_form_is_reached():
    """The dispatch conditions (H*W % 4, L against 4096 / 8192 / 16384, the split S), recomputed from the shapes: every kernel of
    norm.hip -- both HAS_Y instantiations, every K -- plus bn_eval_fwd / bn_eval_bwd is launched by a case of this file."""
    assert_forms_covered()
    assert forms(DETERMINISM_SHAPE, "lrelu", True) >= {"norm_bwd_reduce_kernel<true>", "norm_bwd_dx_kernel<true>", "streaming, S > 1"}
    assert {"norm_bwd_small_kernel<4>"} <= forms(ACC_SHAPES[0], None, False) and {"norm_bwd_dx_kernel<false>"} <= forms(ACC_SHAPES[1], None, False)
    assert {"norm_bwd_dx_generic_kernel", "generic, S > 1"} <= forms(ACC_SHAPES[2], None, False)
    assert {"norm_fwd_small_kernel<16>"} <= forms(STAT_SHAPES[0], None, False) and {"norm_stats_kernel"} <= forms(STAT_SHAPES[1], None, False)


@pytest.mark.parametrize("shape", ACC_SHAPES, ids=[case_id(s) for s in ACC_SHAPES])
def test_batchnorm_bwd_accumulate_affine(fa, shape):
    """faoctasr_batchnorm_train_bwd through the C ABI: accumulate_affine = 1 adds the gradient to what dgamma / dbeta hold,
    accumulate_affine = 0 overwrites it -- small-row, streaming and generic form."""
    from faoctasr._lib import call, ptr, stream_ptr
    N, C, H, W = shape
    case = "acc_" + case_id(shape)
    c = build_case(shape, None, False, 4000 + ACC_SHAPES.index(shape))
    ref, ref32 = refs(c, None, False)
    x, cot, gamma, beta = dev(c["x"]), dev(c["cot"]), dev(c["gamma"]), dev(c["beta"])
    mean, invstd = dev(ref["save_mean"].float()), dev(ref["save_invstd"].float())
    ws = torch.empty(fa._lib.load().faoctasr_bn_workspace_floats(C), device="cuda")
    pre_g, pre_b = torch.arange(C, dtype=torch.float32) * 3.25 - 5.0, torch.arange(C, dtype=torch.float32) * -1.5 + 700.0
    for accumulate in (1, 0):
        dx = torch.full_like(x, SENTINEL)
        dgamma, dbeta = dev(pre_g), dev(pre_b)
        call("batchnorm_train_bwd", ptr(x), ptr(cot), None, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(dx), ptr(dgamma), ptr(dbeta),
             None, N, C, H * W, 0, SLOPE, accumulate, ptr(ws), stream_ptr())
        torch.cuda.synchronize()
        tag = "%s_%d" % (case, accumulate)
        check_elementwise(tag, "dx", dx, ref, ref32, c)
        want = {"dgamma": ref["dgamma"] + pre_g.double() * accumulate, "dbeta": ref["dbeta"] + pre_b.double() * accumulate}
        want32 = {"dgamma": ref32["dgamma"] + pre_g * accumulate, "dbeta": ref32["dbeta"] + pre_b * accumulate}
        check_sum(tag, "dgamma", dgamma, want, want32, ref["abs_dgamma"])
        check_sum(tag, "dbeta", dbeta, want, want32, ref["abs_dbeta"])


@pytest.mark.parametrize("shape,act,affine", IN_CASES, ids=[case_id(s, a, what=None if f else "no_affine") for (s, a, f) in IN_CASES])
def test_instancenorm_forms(fa, shape, act, affine):
    case = "in_" + case_id(shape, act, what=None if affine else "no_affine")
    c = build_case(shape, act, False, 1000 + IN_CASES.index((shape, act, affine)), instance=True, affine=affine)
    ref, ref32 = refs(c, act, False, instance=True)
    xd, gd, bd = leaf(c["x"]), leaf(c["gamma"]), leaf(c["beta"])
    with sentinel_outputs():
        y = fa.ops.instance_norm(xd, gd, bd, EPS, act, SLOPE)
        torch.cuda.synchronize()
        check_elementwise(case, "y", y, ref, ref32, c)
        stats = y.grad_fn.saved_tensors[2]
        assert stats.shape == (2, shape[0] * shape[1])
        check_forward_stats(case, stats, None, None, ref, ref32)
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    check_elementwise(case, "dx", xd.grad, ref, ref32, c)
    if affine:
        check_sum(case, "dgamma", gd.grad, ref, ref32, ref["abs_dgamma"])
        check_sum(case, "dbeta", bd.grad, ref, ref32, ref["abs_dbeta"])


@pytest.mark.parametrize("shape,act,affine", EVAL_CASES, ids=[case_id(s, a, what=None if f else "no_affine") for (s, a, f) in EVAL_CASES])
def test_batchnorm_eval(fa, shape, act, affine):
    case = "eval_" + case_id(shape, act, what=None if affine else "no_affine")
    c = build_eval_case(shape, act, affine, 2000 + EVAL_CASES.index((shape, act, affine)))
    ref, ref32 = (bn_eval_ref(c["x"], c["gamma"], c["beta"], c["rmean"], c["rvar"], act, c["cot"], dtype=dt) for dt in (torch.float64, torch.float32))
    xd = leaf(c["x"])
    rm, rv = dev(c["rmean"]), dev(c["rvar"])
    with sentinel_outputs():
        y = fa.ops.batchnorm_eval(xd, dev(c["gamma"]), dev(c["beta"]), rm, rv, EPS, act, SLOPE)
        torch.cuda.synchronize()
        check_elementwise(case, "y", y, ref, ref32, c)
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    check_elementwise(case, "dx", xd.grad, ref, ref32, c)
    assert torch.equal(rm.cpu(), c["rmean"]) and torch.equal(rv.cpu(), c["rvar"])       # inference mode leaves them alone


@pytest.mark.parametrize("shape", STAT_SHAPES, ids=[case_id(s) for s in STAT_SHAPES])
def test_statistics_of_a_large_mean(fa, shape):
    """x = 0.01 randn + 100: the mean squared is 1e8 times the variance.  The statistics are accumulated around the row's first
    element, and the forward adds what the roundings of the mean and of beta - mean * gamma * invstd lose back to the output
    (norm.hip offset_tail), so save_invstd and y hold the bars they hold everywhere else.  Before that correction y was up to
    3.5e-4 from float64 here (relative L2 1.3e-4 and 2.1e-4; 30647 and 44276 elements outside the bar on an MI355X)."""
    c = build_case(shape, None, False, 5000 + STAT_SHAPES.index(shape), spikes=False, x_scale=0.01, x_offset=100.0)
    run_batchnorm(fa, "stat_" + case_id(shape), c, None, False, backward=False)


@pytest.mark.parametrize("act,res", [("relu", False), ("lrelu", True)])
def test_streaming_backward_is_deterministic(fa, act, res):
    """The S partials of a row are combined in a fixed order and the affine gradients are plain stores: two identical calls give
    identical bits (both HAS_Y forms of the streaming backward)."""
    c = build_case(DETERMINISM_SHAPE, act, res, 6000)
    outs = []
    for _ in range(2):
        xd, gd, bd, rd = leaf(c["x"]), leaf(c["gamma"]), leaf(c["beta"]), leaf(c["res"] if res else None)
        fa.ops.batchnorm_train(xd, gd, bd, None, None, 0.1, EPS, act, SLOPE, rd).backward(dev(c["cot"]))
        torch.cuda.synchronize()
        outs.append((xd.grad, gd.grad, bd.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
