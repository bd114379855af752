"""Every pointwise kernel of csrc/pointwise.hip on the GPU at the sizes where its code takes another branch -- float4 body and
scalar tail, n < 4, a second grid pass, channel_sum's float4 / scalar / split / accumulate forms, the reflection fold with both
borders on one pixel, loss_final over more than 256 partials, mean_mix rows on either side of the block, the NULL-band and
NULL-gradient forms, both AdamW kernels -- against the float64 restatement of tests/test_pointwise_cpu.py (pinned there to torch
and the oracle in float64).  The case tables, the input builders, the bars and their derivation live in that file; its
test_every_form_is_reached ties the tables to the constants of the source.

Operators are reached through faoctasr.ops / ParamArena.step where a public path exists and through the C ABI where the op is an
internal entry point (channel_sum, reflect_pad_bwd, fill, freq_mix_fwd / _bwd, the NULL-band Haar forms, adamw_step with an n
that is no multiple of 4 -- a ParamArena pads to 4 -- and adamw_step_dev).  Every output is allocated under the sentinel fill
(test_gpu_norm.sentinel_outputs) or pre-filled with it, so an element that is never stored fails its comparison.

``POINTWISE_ERR <case> <array> e_ref e_hip ratio ulp`` lines record the relative L2 error of the kernels (e_hip) and of the
restatement run in float32 on the CPU (e_ref) against float64, and the kernels' worst error in fp32 ulps of the reference;
profiles/pointwise_error.txt keeps an MI355X run's.  Reported, not asserted."""
import pytest
import torch

import test_pointwise_cpu as P
from test_gpu_norm import SENTINEL, dev, leaf, sentinel_outputs
from test_norm_cpu import rel_l2

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def ids(op, table):
    return [P.ident(op, c) for c in table]


def filled(*shape):
    return torch.full(shape, SENTINEL, dtype=F32, device="cuda")


def report(case, name, got, ref, ref32):
    e_ref, e_hip = rel_l2(ref32, ref), rel_l2(got, ref)
    print("POINTWISE_ERR %-44s %-9s e_ref %.3e e_hip %.3e ratio %.3f ulp %.2f"
          % (case, name, e_ref, e_hip, e_hip / e_ref if e_ref else float("inf") if e_hip else 1.0, P.worst_ulps(got, ref)))


def check(case, got, ref, ref32, bars, names=None):
    torch.cuda.synchronize()
    for name in names or bars:
        g = got[name].detach().cpu()
        report(case, name, g, ref[name], ref32[name])
        assert bool(torch.isfinite(g).all()) and (g.numel() == 0 or float(g.abs().max()) < 1e29), "%s %s: an element was never stored" % (case, name)
    P.assert_bars(case, got, ref, bars, names)


def call(fa, name, *args):
    fa._lib.call(name, *[fa._lib.ptr(a) if torch.is_tensor(a) else a for a in args], fa._lib.stream_ptr())


# ----------------------------------------------------------------------------------------
# activations, cat + activation, axpby / add / fill
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.ACT_CASES, ids=ids("act", P.ACT_CASES))
def test_activation(fa, case):
    n, act, slope = case
    c = P.build_act(case)
    ref, ref32 = P.act_ref(c, act, slope), P.act_ref(c, act, slope, F32)
    xd = leaf(c["x"])
    with sentinel_outputs():
        y = fa.ops.activation(xd, act, slope)
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    check(P.ident("act", case), {"y": y, "dx": xd.grad}, ref, ref32, P.act_bars(act))


@pytest.mark.parametrize("case", P.CAT2_CASES, ids=ids("cat2", P.CAT2_CASES))
def test_cat2_act(fa, case):
    shape, act, needs = case
    c = P.build_cat2(case)
    ref, ref32 = P.cat2_ref(c, act, P.SLOPE), P.cat2_ref(c, act, P.SLOPE, F32)
    ad, bd = (leaf(c["a"]) if "a" in needs else dev(c["a"])), (leaf(c["b"]) if "b" in needs else dev(c["b"]))
    with sentinel_outputs():
        y = fa.ops.cat2_act(ad, bd, act, P.SLOPE)
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    got = {"y": y, "da": ad.grad, "db": bd.grad}
    assert (ad.grad is None) == ("a" not in needs) and (bd.grad is None) == ("b" not in needs)
    check(P.ident("cat2", case), got, ref, ref32, P.cat2_bars(act), ["y"] + ["d" + k for k in needs])


@pytest.mark.parametrize("case", P.AXPBY_CASES, ids=ids("axpby", P.AXPBY_CASES))
def test_axpby(fa, case):
    n, alpha, beta, inplace = case
    c = P.build_axpby(case)
    ref, ref32 = P.axpby_ref(c, alpha, beta), P.axpby_ref(c, alpha, beta, F32)
    tag = P.ident("axpby", case)
    if inplace:                                          # y is a, as _FreqSplit.backward accumulates into dx
        buf, b = filled(n + 8), dev(c["b"])
        a = buf[4:4 + n]
        a.copy_(c["a"])
        call(fa, "axpby", a, b, a, n, alpha, beta)
        check(tag, {"y": a}, ref, ref32, P.AXPBY_BARS, ["y"])
        assert bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all()) and torch.equal(b.cpu(), c["b"])
        return
    ad, bd = leaf(c["a"]), leaf(c["b"])
    with sentinel_outputs():
        y = fa.ops.axpby(ad, bd, alpha, beta)
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    check(tag, {"y": y, "da": ad.grad, "db": bd.grad}, ref, ref32, P.AXPBY_BARS)
    if (alpha, beta) == (1.0, 1.0):
        a2, b2 = leaf(c["a"]), leaf(c["b"])
        with sentinel_outputs():
            y2 = fa.ops.add(a2, b2)
            y2.backward(dev(c["cot"]))
            torch.cuda.synchronize()
        check(tag + "_add", {"y": y2}, ref, ref32, P.AXPBY_BARS, ["y"])
        assert torch.equal(y2, y) and torch.equal(a2.grad.cpu(), c["cot"]) and torch.equal(b2.grad.cpu(), c["cot"])


@pytest.mark.parametrize("n", P.FILL_CASES)
def test_fill(fa, n):
    buf = filled(n + 8)
    call(fa, "fill", buf[4:4 + n], n, -3.25)
    torch.cuda.synchronize()
    assert bool((buf[4:4 + n] == -3.25).all()), "fill_%d: an element was not stored" % n
    assert bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all()), "fill_%d wrote outside its range" % n


# ----------------------------------------------------------------------------------------
# per-channel sum, reflection fold
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CSUM_CASES, ids=ids("csum", P.CSUM_CASES))
def test_channel_sum(fa, case):
    (N, C, H, W), acc = case
    c = P.build_csum(case)
    ref, ref32 = P.csum_ref(c, acc), P.csum_ref(c, acc, F32)
    dy = dev(c["dy"])
    db = dev(c["prior"]) if acc else filled(C)           # accumulate = 0 overwrites whatever db held
    call(fa, "channel_sum", dy, db, N, C, H * W, acc)
    check(P.ident("csum", case), {"db": db}, ref, ref32, P.CSUM_BARS)
    if acc:                                              # accumulate = 1 is accumulate = 0 plus the prior contents, within the bound
        db0 = filled(C)
        call(fa, "channel_sum", dy, db0, N, C, H * W, 0)
        torch.cuda.synchronize()
        n, worst = P.sum_violations(db, db0.cpu().double() + c["prior"].double(), 2 * ref["abs_db"])
        assert n == 0, "%s: accumulate = 1 differs from accumulate = 0 + prior at %.2f of the bar" % (P.ident("csum", case), worst)


@pytest.mark.parametrize("case", P.REFLECT_CASES, ids=ids("reflect", P.REFLECT_CASES))
def test_reflect_pad_bwd(fa, case):
    NC, H, W, p = case
    c = P.build_reflect(case)
    ref, ref32 = P.reflect_fold_ref(c, p), P.reflect_fold_ref(c, p, F32)
    dx = filled(NC, H, W)
    call(fa, "reflect_pad_bwd", dev(c["dxp"]), dx, NC, H, W, p)
    check(P.ident("reflect", case), {"dx": dx}, ref, ref32, P.REFLECT_BARS)


# ----------------------------------------------------------------------------------------
# Haar analysis / synthesis, discriminator front ends, frequency-split mixing
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.HAAR_CASES, ids=ids("haar", P.HAAR_CASES))
def test_haar(fa, case):
    shape, bands = case
    N, C, H, W = shape
    c = P.build_haar(case)
    tag = P.ident("haar", case)
    l_, h_ = (None if bands == "hi only" else c["ll"]), (None if bands == "ll only" else c["hi"])
    fwd, fwd32 = P.haar_fwd_ref(c["x"]), P.haar_fwd_ref(c["x"], F32)
    inv, inv32 = P.haar_inv_ref(l_, h_, shape), P.haar_inv_ref(l_, h_, shape, F32)
    out_names = [k for k, t in (("ll", l_), ("hi", h_)) if t is not None]
    if bands == "both bands":                            # the public pair, forward and backward
        xd, ld, hd = leaf(c["x"]), leaf(c["ll"]), leaf(c["hi"])
        with sentinel_outputs():
            ll, hi = fa.ops.haar_afb2d(xd)
            torch.autograd.backward([ll, hi], [dev(c["ll"]), dev(c["hi"])])
            x = fa.ops.haar_sfb2d(ld, hd)
            x.backward(dev(c["x"]))
            torch.cuda.synchronize()
        check(tag, {"ll": ll, "hi": hi}, fwd, fwd32, P.HAAR_BARS, out_names)
        check(tag + "_afb_bwd", {"x": xd.grad}, inv, inv32, P.HAAR_BARS, ["x"])
        check(tag + "_sfb", {"x": x}, inv, inv32, P.HAAR_BARS, ["x"])
        check(tag + "_sfb_bwd", {"ll": ld.grad, "hi": hd.grad}, fwd, fwd32, P.HAAR_BARS, out_names)
    # the C ABI with the absent band NULL (both present: the same kernels as above, once more)
    got = {"ll": filled(N, C, H // 2, W // 2) if l_ is not None else None, "hi": filled(N, C, 3, H // 2, W // 2) if h_ is not None else None,
           "x": filled(N, C, H, W)}
    call(fa, "haar_dwt2d_fwd", dev(c["x"]), got["ll"], got["hi"], N * C, H, W)
    call(fa, "haar_dwt2d_bwd", None if l_ is None else dev(l_), None if h_ is None else dev(h_), got["x"], N * C, H, W)
    check(tag + "_abi", got, fwd, fwd32, P.HAAR_BARS, out_names)
    check(tag + "_abi", got, inv, inv32, P.HAAR_BARS, ["x"])
    # <A x, c> = <x, A^T c> between the two kernels' outputs, within what their bars allow each side
    lhs, rhs, slack = 0.0, float((c["x"].double() * got["x"].cpu().double()).sum()), 0.0
    slack += float(((3 * P.U * inv["abs_x"] + P.ulp32(inv["x"])) * c["x"].double().abs()).sum())
    for k, cot in (("ll", l_), ("hi", h_)):
        if cot is not None:
            lhs += float((got[k].cpu().double() * cot.double()).sum())
            slack += float(((3 * P.U * fwd["abs_" + k] + P.ulp32(fwd[k])) * cot.double().abs()).sum())
    assert abs(lhs - rhs) <= slack, "%s: <A x, c> = %.9g but <x, A^T c> = %.9g (allowed %.3g)" % (tag, lhs, rhs, slack)


@pytest.mark.parametrize("case", P.DFRONT_CASES, ids=ids("dfront", P.DFRONT_CASES))
def test_haar_dfront(fa, case):
    (N, H, W), mode = case
    c = P.build_dfront(case)
    ref, ref32 = P.dfront_ref(c, mode), P.dfront_ref(c, mode, F32)
    xd = leaf(c["x"])
    with sentinel_outputs():
        y = fa.ops.haar_dfront(xd, mode)
        y.backward(dev(c["cot"]))
        torch.cuda.synchronize()
    check(P.ident("dfront", case), {"y": y, "dx": xd.grad}, ref, ref32, P.dfront_bars(mode))


@pytest.mark.parametrize("case", P.FREQ_CASES, ids=ids("freq", P.FREQ_CASES))
def test_freq_mix(fa, case):
    n, grads = case
    c = P.build_freq(case)
    ref, ref32 = P.freq_mix_ref(c, grads), P.freq_mix_ref(c, grads, F32)
    x, hp, lp = dev(c["x"]), dev(c["lo_hp"]), dev(c["lo_lp"])
    got = {k: filled(n) for k in ("hf", "lf", "s_hp", "s_lp", "dx_direct")}
    call(fa, "freq_mix_fwd", x, hp, lp, got["hf"], got["lf"], n)
    call(fa, "freq_mix_bwd", x, hp, lp, None if grads == "g_lf only" else dev(c["g_hf"]), None if grads == "g_hf only" else dev(c["g_lf"]),
         got["s_hp"], got["s_lp"], got["dx_direct"], n)
    check(P.ident("freq", case), got, ref, ref32, P.FREQ_BARS)
    # the ties: sgn(0) = 0, as torch's abs
    assert float(got["s_hp"].cpu()[c["tie_hp"]].abs().sum()) == 0.0 and float(got["s_lp"].cpu()[c["tie_lp"]].abs().sum()) == 0.0


# ----------------------------------------------------------------------------------------
# losses, mean_mix, AdamW
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.LOSS_CASES, ids=ids("loss", P.LOSS_CASES))
def test_losses(fa, case):
    kind, n = case
    c = P.build_loss(case)
    ref, ref32 = P.loss_ref(c, kind), P.loss_ref(c, kind, F32)
    fn = {"mse": fa.ops.mse_loss, "l1": fa.ops.l1_loss, "bce": fa.ops.bce_with_logits}[kind]
    ad, bd = leaf(c["a"]), leaf(c["b"])
    with sentinel_outputs():
        val = fn(ad, bd, P.LOSS_WEIGHT)
        val.backward(dev(c["g"]))
        again = fn(ad.detach(), bd.detach(), P.LOSS_WEIGHT)
        torch.cuda.synchronize()
    check(P.ident("loss", case), {"value": val, "da": ad.grad, "db": bd.grad}, ref, ref32, P.loss_bars(kind))
    assert torch.equal(val, again), "loss_fwd has no atomics: two runs must agree to the bit"
    if kind == "l1":
        assert float(ad.grad.cpu()[c["tie"]].abs().sum()) == 0.0 and float(bd.grad.cpu()[c["tie"]].abs().sum()) == 0.0


@pytest.mark.parametrize("case", P.MEAN_MIX_CASES, ids=ids("mean_mix", P.MEAN_MIX_CASES))
def test_mean_mix(fa, case):
    (N, La, Lb), (wa, wb) = case
    c = P.build_mean_mix(case)
    ref, ref32 = P.mean_mix_ref(c, wa, wb), P.mean_mix_ref(c, wa, wb, F32)
    ad, bd = leaf(c["a"]), leaf(c["b"])
    with sentinel_outputs():
        out = fa.ops.mean_mix(ad, bd, wa, wb)
        out.backward(dev(c["g"]))
        again = fa.ops.mean_mix(ad.detach(), bd.detach(), wa, wb)
        torch.cuda.synchronize()
    check(P.ident("mean_mix", case), {"out": out, "da": ad.grad, "db": bd.grad}, ref, ref32, P.MEAN_MIX_BARS)
    assert torch.equal(out, again), "mean_mix_fwd has no atomics: two runs must agree to the bit"


def adamw_report(case, steps_got, steps_ref, steps_ref32):
    for i, (g, r, r32) in enumerate(zip(steps_got, steps_ref, steps_ref32)):
        for j, name in enumerate(("p", "m", "v")):
            report("%s_step%d" % (case, i), name, g[j], r[j], r32[j])


@pytest.mark.parametrize("case", P.ADAMW_CASES, ids=ids("adamw", P.ADAMW_CASES))
def test_adamw(fa, case):
    """ParamArena.step in its eager (host scalars, adamw_kernel) and captured-graph (device scalars, adamw_dev_kernel) forms on
    the arena's padded length, and both entry points through the C ABI on the case's own n (the scalar tail).  The device-scalar
    form equals the host-scalar form to the bit; both meet the bars against float64."""
    n, start, wd, gs = case
    c = P.build_adamw(case)
    tag = P.ident("adamw", case)
    ref, ref32, ref_r = P.adamw_run(c, case), P.adamw_run(c, case, F32, True), P.adamw_run(c, case, round_scalars=True)
    runs = {}
    # through the arena
    for form in ("eager", "graph"):
        w = torch.nn.Parameter(dev(c["p"]).clone())
        arena = fa.ParamArena([("w", w)], lr=P.ADAMW_LR, betas=P.ADAMW_BETAS, eps=P.ADAMW_EPS, weight_decay=wd)
        pad = arena.numel - n
        assert 0 <= pad < 4 and w.data_ptr() == arena.flat.data_ptr()
        arena.exp_avg[:n].copy_(c["m"])
        arena.exp_avg_sq[:n].copy_(c["v"])
        arena.step_count = c["first_step"] - 1
        steps = []
        for i, g in enumerate(c["grads"]):
            arena.grad[:n].copy_(g)
            if form == "eager":
                arena.step(gs)
            else:
                hyper = torch.tensor(arena.hyper_values(c["first_step"] + i, gs), dtype=F32, device="cuda")
                arena.step(hyper=hyper)
            torch.cuda.synchronize()
            steps.append((w.detach().cpu().clone(), arena.exp_avg[:n].cpu(), arena.exp_avg_sq[:n].cpu()))
            for t in (arena.flat, arena.exp_avg, arena.exp_avg_sq):
                assert float(t[n:].abs().sum()) == 0.0 if pad else True, "%s: the arena's padding moved" % tag
        runs["arena_" + form] = steps
    # through the C ABI, n as it is
    hyper_of = arena.hyper_values
    for form in ("host", "dev"):
        bufs = [filled(n + 4) for _ in range(3)]
        for b, src in zip(bufs, (c["p"], c["m"], c["v"])):
            b[:n].copy_(src)
        p, m, v = (b[:n] for b in bufs)
        steps = []
        for i, g in enumerate(c["grads"]):
            gd = dev(g)
            if form == "host":
                call(fa, "adamw_step", p, gd, m, v, n, P.ADAMW_LR, P.ADAMW_BETAS[0], P.ADAMW_BETAS[1], P.ADAMW_EPS, wd, c["first_step"] + i, gs)
            else:
                call(fa, "adamw_step_dev", p, gd, m, v, n, torch.tensor(hyper_of(c["first_step"] + i, gs), dtype=F32, device="cuda"))
            torch.cuda.synchronize()
            steps.append((p.cpu(), m.cpu(), v.cpu()))
            assert torch.equal(gd.cpu(), g), "%s: the gradient was written" % tag
        for b in bufs:
            assert bool((b[n:] == SENTINEL).all()), "%s: adamw_%s wrote past n" % (tag, form)
        runs["abi_" + form] = steps
    adamw_report(tag, runs["abi_host"], ref, ref32)
    for name, steps in runs.items():
        P.adamw_assert(tag + "_" + name, steps, ref, ref_r)
    # the two kernels agree to the bit, and so do the float4 body (the arena's padded length) and the scalar tail (n as it is):
    # adamw_elem writes its multiply-adds out.  Left to the compiler's contraction, adamw_kernel's tail rounded v differently from
    # its body and from adamw_dev_kernel's tail (n = 3: m, v and p differed; n = 2098183: v of a tail element)
    for a, b in (("abi_host", "abi_dev"), ("arena_eager", "arena_graph"), ("abi_host", "arena_eager")):
        for i, (sa, sb) in enumerate(zip(runs[a], runs[b])):
            for name, ta, tb in zip("pmv", sa, sb):
                assert torch.equal(ta, tb), "%s step %d %s: %s and %s differ in bits" % (tag, i, name, a, b)


# ----------------------------------------------------------------------------------------
# the host-side checks, with device operands: refused before anything is allocated or launched
# ----------------------------------------------------------------------------------------
def test_mismatched_operands_and_negative_slopes_launch_nothing(fa, monkeypatch):
    P.refuse_launches(monkeypatch, fa.ops)
    allocated = []
    real = torch.empty, torch.empty_like

    def counted(fn):
        def make(*a, **k):
            allocated.append((a, k))
            return fn(*a, **k)
        return make
    monkeypatch.setattr(torch, "empty", counted(real[0]))
    monkeypatch.setattr(torch, "empty_like", counted(real[1]))
    g = torch.Generator().manual_seed(5)
    for what, fn, pattern in P.mismatched_calls(fa.ops, lambda *s: torch.randn(*s, generator=g).cuda().requires_grad_(True)):
        with pytest.raises(fa._lib.KernelError, match=pattern):
            fn()
        assert not allocated, "%s allocated an output before it refused the call" % what


def test_haar_dfront_bwd_rejects_odd_sizes(fa):
    for H, W in ((5, 6), (6, 5)):
        dy, dx = dev(torch.ones(1, 1, H // 2, W // 2)), filled(1, 1, H, W)
        for name, first, second in (("haar_dfront_fwd", dx, filled(1, 1, H // 2, W // 2)), ("haar_dfront_bwd", dy, dx)):
            with pytest.raises(fa._lib.KernelError, match="odd size"):
                call(fa, name, first, second, 1, H, W, 0)
            torch.cuda.synchronize()
            assert bool((second == SENTINEL).all()), "%s stored something for an odd size" % name
