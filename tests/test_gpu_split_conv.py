"""The split-precision convolutions on the GPU: the wide gather kernel (csrc/igemm_bf16x3.hip, route 4), the f16x2 narrow-map kernel
(csrc/igemm_nm_x2.hip, route 8) and the split weight gradient (csrc/wgrad_x3.hip, route 15), form by form, against the float64
restatements of tests/test_split_conv_cpu.py.  The case tables, the input builders, the bars and their derivation, and the map from a
case to the forms it reaches live in that file; its test_every_form_is_reached ties the tables to the constants of the sources.

Every case is called through the C ABI with the hand-over ``ops`` makes (absmax_bits, conv_set_scales, conv_set_workspace,
conv_set_residual, wpack_state 1 and then 2 on the same image), in both arithmetics and both data modes, on buffers of this file's
own making: operands are NaN in GUARD elements on either side, outputs are the sentinel (test_gpu_norm.SENTINEL) and sit inside
sentinel bands, as do the packed image (sized exactly by faoctasr_conv_wpack_floats), the workspace (sized exactly by
faoctasr_conv_gather_workspace_floats / faoctasr_conv_wgrad_workspace_floats) and the absmax slots.

``SPLIT_ERR <case> <array> e_split e_hip ratio ulp`` lines record the relative L2 distance from float64 of the emulated split
operands (e_split) and of the kernels (e_hip), and the kernels' worst distance from the emulation in fp32 ulps;
profiles/split_conv_error.txt keeps an MI355X run's.  Reported, not asserted."""
import functools

import pytest
import torch

import test_split_conv_cpu as S
from test_gpu_norm import SENTINEL, dev
from test_norm_cpu import rel_l2
from test_pointwise_cpu import worst_ulps

pytestmark = pytest.mark.gpu
F32 = torch.float32
GUARD, BAND = 64, 1024                          # NaN elements around an operand; sentinel elements around a buffer the kernels write
BY = {c.name: c for c in S.ALL_CASES}


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Operand:
    """A read-only tensor between two NaN guards; ``misaligned``: its first element sits 4 bytes past a 16-byte boundary."""

    def __init__(self, t, misaligned=False):
        self.host, self.off = t.contiguous(), GUARD + (1 if misaligned else 0)
        buf = torch.full((t.numel() + 2 * GUARD + 4,), float("nan"), dtype=F32)
        buf[self.off:self.off + t.numel()] = t.reshape(-1)
        self.buf = buf.cuda()
        self.ptr = self.buf.data_ptr() + 4 * self.off
        assert self.ptr % 16 == (4 if misaligned else 0)

    def view(self):
        return self.buf[self.off:self.off + self.host.numel()]

    def unchanged(self):
        return torch.equal(bits(self.view()), bits(self.host.reshape(-1)))


class Banded:
    """A buffer the kernels may write, sentinel-filled (or holding ``init``), between two sentinel bands."""

    def __init__(self, n, init=None, misaligned=False, zero=False):
        self.n, self.off = n, BAND + (1 if misaligned else 0)
        self.buf = torch.full((n + 2 * BAND + 4,), SENTINEL, dtype=F32, device="cuda")
        if init is not None:
            self.buf[self.off:self.off + n] = dev(init.reshape(-1))
        elif zero:
            self.buf[self.off:self.off + n] = 0
        self.ptr = (self.buf.data_ptr() + 4 * self.off) if n > 0 else None
        assert self.ptr is None or self.ptr % 16 == (4 if misaligned else 0)

    def live(self):
        return self.buf[self.off:self.off + self.n]

    def intact(self):
        h = self.buf.cpu()
        return bool((h[:self.off] == SENTINEL).all()) and bool((h[self.off + self.n:] == SENTINEL).all())

    def refill(self):
        self.buf[self.off:self.off + self.n] = SENTINEL


@functools.lru_cache(maxsize=None)
def references(c, mode, eff):
    """(conv_ref, split_ref) of a case's data at the arithmetic its route really uses ("f32" off the split routes); computed once."""
    d = S.build(c, mode)
    integer = mode == "integer"
    return S.conv_ref(c.kind, c, d, integer), S.split_ref(c.kind, c, d, eff, integer=integer)


def run(fa, c, arith, d, calls=2, residual=True):
    """Calls the entry point of ``c`` ``calls`` times (wpack_state 1, then 2) and checks every buffer.  Returns the outputs on the host."""
    from faoctasr._lib import call, stream_ptr
    lib, st = fa._lib.load(), stream_ptr()
    prec = S.ARITH[arith] | (S.NO_SPLIT_K if c.nosplit else 0)
    dims, wgrad = S.abi_dims(c), c.kind in S.WGRAD
    N, C, H, W, M, KH, KW, s, p = dims
    so = S.shapes(c)[2]
    nout = int(torch.Size(so).numel())
    a, b = Operand(d["a"], "x" in c.align), Operand(d["b"])
    bias = Operand(d["bias"]) if d["bias"] is not None else None
    res = Operand(d["res"], "r" in c.align) if d["res"] is not None and residual else None
    out = Banded(nout, init=d["dw0"], misaligned="y" in c.align)
    watched = [("out", out)]
    slots = []
    if arith == "f16x2":
        for o in (a, b) if wgrad else (a,):
            slot = Banded(S.SLOT_WORDS, zero=True)
            call("absmax_bits", o.ptr, o.host.numel(), slot.ptr, st)
            slots.append(slot)
            watched.append(("absmax slot", slot))
    if wgrad:
        wp = None
        need = lib.faoctasr_conv_wgrad_workspace_floats(*((C, M) if c.kind == "conv2d_wgrad" else (M, C)), KH, KW, s)
    else:
        wp = Banded(lib.faoctasr_conv_wpack_floats(S.KIND_ID[c.kind], C, M, KH, KW, s, p, S.ARITH[arith]))
        watched.append(("packed image", wp))
        need = lib.faoctasr_conv_gather_workspace_floats(*S.probe_args(c)) if arith == "f16x2" else 0
    if c.ws == "short":                 # one float less than the launch needs (the weight gradients' own count is an upper bound)
        need = (S.wx3_slices(c, None, S.read_constants())[0] * nout if wgrad else need) - 1
    ws = Banded(max(need, 0)) if need > 0 and c.ws != "none" else None
    if ws is not None:
        watched.append(("workspace", ws))
    act, bp = S.ACT_ID[c.act], bias.ptr if bias else None
    outs = []
    for i in range(calls):
        if i:
            if d["dw0"] is None:
                out.refill()
            else:
                out.live().copy_(d["dw0"].reshape(-1))
        state = 0 if wp is None or wp.n == 0 else 1 + min(i, 1)
        if slots:
            call("conv_set_scales", slots[0].ptr, slots[1].ptr if len(slots) > 1 else None)
        if ws is not None:
            call("conv_set_workspace", ws.ptr, ws.n)
        if res is not None:
            call("conv_set_residual", res.ptr)
        wpp = wp.ptr if wp is not None else None
        if c.kind == "conv2d_fwd":
            call(c.kind, a.ptr, b.ptr, bp, out.ptr, *dims, c.reflect, act, c.slope, wpp, state, prec, st)
        elif c.kind == "conv2d_dgrad":
            call(c.kind, a.ptr, b.ptr, out.ptr, *dims, wpp, state, prec, st)
        elif c.kind == "conv_transpose2d_fwd":
            call(c.kind, a.ptr, b.ptr, bp, out.ptr, *dims, c.out_pad, act, c.slope, wpp, state, prec, st)
        elif c.kind == "conv_transpose2d_dgrad":
            call(c.kind, a.ptr, b.ptr, out.ptr, *dims, c.out_pad, wpp, state, prec, st)
        elif c.kind == "conv2d_wgrad":
            call(c.kind, a.ptr, b.ptr, out.ptr, *dims, c.reflect, c.acc, prec, st)
        else:
            call(c.kind, a.ptr, b.ptr, out.ptr, *dims, c.out_pad, c.acc, prec, st)
        r = lib.faoctasr_last_route()
        torch.cuda.synchronize()
        want = S.route(c, arith)
        assert r == want if want is not None else r not in (S.ROUTE_X3, S.ROUTE_NX2, S.ROUTE_WX3), "%s: route %d, predicted %s" % (c.name, r, want)
        got = out.live().cpu().view(so)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 1e29, "%s: an output element was never stored (call %d)" % (c.name, i)
        for name, buf in watched:
            assert buf.intact(), "%s: a store outside the %s (call %d)" % (c.name, name, i)
        for name, o in (("a", a), ("b", b), ("bias", bias), ("res", res)):
            assert o is None or o.unchanged(), "%s: operand %s was written (call %d)" % (c.name, name, i)
        for slot in slots:
            words = slot.live().cpu().view(torch.int32)
            used = torch.zeros(S.SLOT_WORDS, dtype=torch.bool)
            used[::S.SLOT_STRIDE] = True
            assert int(used.sum()) == S.SLOT_PARTS and bool((words[~used] == 0).all()), "%s: an unused word of an absmax slot is set" % c.name
        outs.append(got.clone())
    return outs


def report(tag, got, ref, sp):
    e_split, e_hip = rel_l2(sp["out"], ref), rel_l2(got, ref)
    print("SPLIT_ERR %-44s e_split %.3e e_hip %.3e ratio %.3f ulp %.2f"
          % (tag, e_split, e_hip, e_hip / e_split if e_split else float("inf") if e_hip else 1.0, worst_ulps(got, sp["out"])))


def judge(c, arith, mode, got, tag, first=True):
    eff = arith if S.route(c, arith) is not None else "f32"
    ref, sp = references(c, mode, eff)
    if first:
        report(tag, got, ref, sp)
    if mode == "integer":
        n = S.exact_violations(got, ref)
        assert n == 0, "%s: %d of %d elements differ from the exact integer result" % (tag, n, got.numel())
    else:
        n, worst = S.violations(got, S.bar(c, sp, eff), sp["out"])
        assert n == 0, "%s: %d elements outside gamma_n |terms| + 1 ulp, worst at %.3g of the bar" % (tag, n, worst)
        assert rel_l2(got, ref) < S.AGGREGATE[arith], tag


def deterministic(c, arith, mode):
    """Two calls must agree to the bit: always on integers (exact), and wherever no fp32 atomics order the sum."""
    if mode == "integer" or S.route(c, arith) == S.ROUTE_NX2:
        return True
    if c.kind in S.WGRAD:
        return S.route(c, arith) == S.ROUTE_WX3 and c.ws == "exact"
    return S.route(c, arith) == S.ROUTE_X3 and S.x3_plan(c, S.gather_geom(c), S.read_constants())["ksplit"] == 1


def check_case(fa, c, arith, mode):
    tag = "%s_%s%s" % (c.name, arith, "_int" if mode == "integer" else "")
    outs = run(fa, c, arith, S.build(c, mode))
    for i, got in enumerate(outs):
        judge(c, arith, mode, got, tag, first=i == 0)
    if deterministic(c, arith, mode):
        assert torch.equal(bits(outs[0]), bits(outs[1])), "%s: the call on the packed image (wpack_state 2) differs in bits from the packing call" % tag


CASE_MODES = [(c, m) for c in S.ALL_CASES for m in S.modes(c)]


@pytest.mark.parametrize("arith", list(S.ARITH))
@pytest.mark.parametrize("c,mode", [(c, m) for c, m in CASE_MODES if c in S.WIDE_CASES], ids=lambda v: v if isinstance(v, str) else v.name)
def test_wide_split_kernel(fa, c, mode, arith):
    check_case(fa, c, arith, mode)


@pytest.mark.parametrize("arith", list(S.ARITH))
@pytest.mark.parametrize("c,mode", [(c, m) for c, m in CASE_MODES if c in S.NARROW_CASES], ids=lambda v: v if isinstance(v, str) else v.name)
def test_narrow_f16x2_kernel(fa, c, mode, arith):
    """At bf16x3 these shapes run on the exact-f32 narrow kernels and are held to the f32 bar."""
    check_case(fa, c, arith, mode)


@pytest.mark.parametrize("arith", list(S.ARITH))
@pytest.mark.parametrize("c,mode", [(c, m) for c, m in CASE_MODES if c in S.WGRAD_CASES], ids=lambda v: v if isinstance(v, str) else v.name)
def test_split_weight_gradient(fa, c, mode, arith):
    check_case(fa, c, arith, mode)


@pytest.mark.parametrize("arith", list(S.ARITH))
def test_misaligned_calls_equal_the_aligned_call(fa, arith):
    """x, y, the residual 4 bytes past a 16-byte boundary (single-pixel items, dword stores, 16-byte residual loads from a misaligned
    address): the same bits as the aligned call, at an interior and at a tail shape."""
    for base in (BY["align_xyr"], BY["align_r_tail"]):
        d = S.build(base, "random")
        want = run(fa, base._replace(align=""), arith, d, calls=1)[0]
        for align in ("x", "y", "r", "xy", "xyr"):
            got = run(fa, base._replace(align=align), arith, d, calls=1)[0]
            assert torch.equal(bits(got), bits(want)), (base.name, arith, align)


def test_narrow_split_k_variants_agree(fa):
    """Route 8 on one set of data: split through the workspace (2 .. 8 slices) within the bar of the unsplit result; without a workspace,
    with one a float too small and under NO_SPLIT_K the grid is not split and the three give the same bits."""
    base = BY["nx_splitk_no_ws"]
    d = S.build(base, "random")
    unsplit = [run(fa, base._replace(ws=ws, nosplit=ns), "f16x2", d)[0] for ws, ns in (("none", False), ("short", False), ("exact", True))]
    assert torch.equal(bits(unsplit[0]), bits(unsplit[1])) and torch.equal(bits(unsplit[0]), bits(unsplit[2]))
    split = run(fa, base._replace(ws="exact"), "f16x2", d)[0]
    assert S.nx2_plan(base._replace(ws="exact"), S.gather_geom(base), S.read_constants())[1] > 1
    sp = S.split_ref(base.kind, base, d, "f16x2")
    assert S.violations(split, S.bar(base, sp, "f16x2"), sp["out"])[0] == 0


@pytest.mark.parametrize("arith", list(S.ARITH))
def test_a_residual_is_applied_exactly_once(fa, arith):
    """The call after one with a residual, made without one, does not see it (integer data: the exact result without the residual)."""
    for name in ("align_r_tail", "dgrad_s1") + (("nx_pix65",) if arith == "f16x2" else ()):
        c = BY[name]
        d = S.build(c, "integer")
        with_res = run(fa, c, arith, d, calls=1)[0]
        without = run(fa, c, arith, d, calls=1, residual=False)[0]
        plain = dict(d, res=None)
        assert S.exact_violations(with_res, S.conv_ref(c.kind, c, d, True)) == 0, name
        assert S.exact_violations(without, S.conv_ref(c.kind, c, plain, True)) == 0, name


@pytest.mark.parametrize("arith", list(S.ARITH))
def test_a_refused_call_consumes_the_hand_over(fa, arith):
    """A call refused for a null pointer or a bad shape takes the residual, the scales and the workspace with it: the good call after it
    behaves as if nothing had been handed over.  At f16x2 the good call is a route-8 layer that splits K only when it has a workspace
    (nx_splitk_256: 4 slices), on random data, so a workspace that survived the refusal would be written and would change the bits of
    the result, as a surviving residual would; at bf16x3 (route 4, which uses no workspace) the residual alone is at stake."""
    from faoctasr._lib import KernelError, call, stream_ptr
    lib, st = fa._lib.load(), stream_ptr()
    c = (BY["nx_splitk_256"] if arith == "f16x2" else BY["align_r_tail"])._replace(ws="none")
    d = S.build(c, "random")
    dims = S.abi_dims(c)
    need = lib.faoctasr_conv_gather_workspace_floats(*S.probe_args(c)) if arith == "f16x2" else 1 << 16
    assert need > 0
    clean = run(fa, c, arith, d, calls=1, residual=False)[0]                   # no workspace, no residual
    leaked = run(fa, c._replace(ws="exact"), arith, d, calls=1)[0]             # what a surviving hand-over would give
    assert not torch.equal(bits(clean), bits(leaked))
    if arith == "f16x2":
        assert S.nx2_plan(c, S.gather_geom(c), S.read_constants())[1] > 1
        assert not torch.equal(bits(clean), bits(run(fa, c._replace(ws="exact"), arith, d, calls=1, residual=False)[0])), "split and unsplit sums coincide"

    def hand_over_and_refuse(refusal):
        x, w, res = Operand(d["a"]), Operand(d["b"]), Operand(d["res"])
        y, ws, slot = Banded(clean.numel()), Banded(need), Banded(S.SLOT_WORDS, zero=True)
        call("absmax_bits", x.ptr, x.host.numel(), slot.ptr, st)
        call("conv_set_scales", slot.ptr, None)
        call("conv_set_workspace", ws.ptr, ws.n)
        call("conv_set_residual", res.ptr)
        bad = (None,) + dims if refusal == "null pointer" else (x.ptr,) + (dims[0], 0) + dims[2:]
        with pytest.raises(KernelError, match=refusal):
            call("conv2d_fwd", bad[0], w.ptr, None, y.ptr, *bad[1:], 0, 0, 0.2, None, 0, S.ARITH[arith], st)
        torch.cuda.synchronize()
        assert bool((y.buf == SENTINEL).all()) and bool((ws.buf == SENTINEL).all())
        return x, w, res, y, ws, slot

    for refusal in ("null pointer", "bad shape"):
        # residual and workspace: the next good call (its own scales, nothing else handed over) is the clean one, bit for bit
        kept = hand_over_and_refuse(refusal)
        got = run(fa, c, arith, d, calls=1, residual=False)[0]
        assert torch.equal(bits(got), bits(clean)), "%s: the call after the refused one saw its residual or its workspace" % refusal
        assert bool((kept[4].buf == SENTINEL).all()), "%s: the workspace of the refused call was used by a later one" % refusal
        if arith == "f16x2":            # scales: the split routes refuse the next call for want of them
            x, w, res, y, ws, slot = hand_over_and_refuse(refusal)
            wp = Banded(lib.faoctasr_conv_wpack_floats(0, dims[1], dims[4], c.k, c.k, c.s, c.p, 3))
            with pytest.raises(KernelError, match="absmax slot"):
                call("conv2d_fwd", x.ptr, w.ptr, None, y.ptr, *dims, 0, 0, 0.2, wp.ptr, 1, 3, st)
            torch.cuda.synchronize()
            assert bool((y.buf == SENTINEL).all()) and bool((ws.buf == SENTINEL).all())


@pytest.mark.parametrize("arith", list(S.ARITH))
def test_scale_invariance(fa, arith):
    """x 2^-30 and w 2^20 (dy for a weight gradient): the unscaled result times 2^-10 to the bit, at a tail shape of route 4, on
    route 8 and on route 15 (power-of-two scales move exponents only: every half, product and partial sum scales with them)."""
    for name in ("W36", "align_r_tail", "nx_pix65", "wx_roll_N3", "wx_row_k4_s2"):
        c = BY[name]._replace(bias=False, res=False, acc=0, align="")
        if S.route(c, arith) is None:
            continue
        assert deterministic(c, arith, "random"), name
        d0 = {k: (v if k in "ab" else None) for k, v in S.build(c, "random").items()}
        d1 = dict(d0, a=d0["a"] * 2.0 ** -30, b=d0["b"] * 2.0 ** 20)
        got0, got1 = run(fa, c, arith, d0, calls=1)[0], run(fa, c, arith, d1, calls=1)[0]
        assert float(got0.abs().max()) > 0 and torch.equal(bits(got1), bits(got0 * 2.0 ** -10)), (name, arith)
