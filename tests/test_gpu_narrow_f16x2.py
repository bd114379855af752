"""The discriminators' narrow-map convolutions (an output phase narrower than 24 pixels) at precision 3 on the f16x2 narrow-map kernel
(csrc/igemm_nm_x2.hip): accuracy beside the exact-f32 kernels against fp64, the route, bit-reproducible split-K (no atomics), tiny
magnitudes, and the shapes it leaves to the exact-f32 narrow kernel."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROUTE_NARROW = 6
ROUTE_NARROW_X2 = 8

# (N, C, H, W, M, k, s, p, bias, act): the PatchGAN layers of model.py at 256^2 (net: 32^2 -> 16^2 -> 8^2 -> 7^2), the half-size
# Haar-band branch's last ones, and the 3x3 narrow layer of the batched-pack test
NARROW_CASES = [
    (4, 256, 32, 32, 512, 4, 2, 1, True, None),
    (4, 512, 16, 16, 512, 4, 2, 1, False, None),
    (4, 512, 8, 8, 512, 4, 1, 1, True, "lrelu"),
    (8, 512, 4, 4, 512, 4, 1, 1, False, None),
    (2, 256, 16, 16, 256, 3, 1, 1, True, "lrelu"),
]


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def dev(t):
    return t.cuda().contiguous()


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _route(fa):
    return fa._lib.load().faoctasr_last_route()


def _ref(x, w, b, s, p, act, cot):
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xr, wr, None if b is None else b.double(), stride=s, padding=p)
    if act == "lrelu":
        ref = F.leaky_relu(ref, 0.2)
    ref.backward(cot.double())
    return ref.detach(), xr.grad, wr.grad


def _data(case, seed, cot_scale=1.0):
    N, C, H, W, M, k, s, p, bias, act = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(M, C, k, k, generator=g) * 0.05
    b = torch.randn(M, generator=g) if bias else None
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cot = 1e-4 * torch.randn(N, M, OH, OW, generator=g) * torch.exp(1.5 * torch.randn(N, M, OH, OW, generator=g)) * cot_scale
    return x, w, b, cot


def _run(fa, prec, case, x, w, b, cot):
    N, C, H, W, M, k, s, p, bias, act = case
    fa.ops.conv_precision = prec
    try:
        xd, wd = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
        out = fa.ops.conv2d(xd, wd, dev(b) if b is not None else None, s, p, False, act, 0.2)
        out.backward(dev(cot))
        torch.cuda.synchronize()
    finally:
        fa.ops.conv_precision = 0
    return out.detach(), xd.grad, wd.grad


@pytest.mark.parametrize("case", NARROW_CASES)
def test_narrow_f16x2_accuracy_beside_f32(fa, case):
    """Forward, input gradient and weight gradient against fp64, f16x2 beside the exact-f32 direct kernels on the same data, with a
    heavy-tailed ~1e-4 cotangent (as test_gpu_ops.py::test_conv2d_f16x2)."""
    x, w, b, cot = _data(case, 99)
    N, C, H, W, M, k, s, p, bias, act = case
    ref = _ref(x, w, b, s, p, act, cot)
    err = {}
    for prec in (1, 3):
        out = _run(fa, prec, case, x, w, b, cot)
        err[prec] = [rel_l2(o, r) for o, r in zip(out, ref)]
    for what, e32, e16 in zip(("y", "dx", "dw"), err[1], err[3]):
        print("narrow f16x2-vs-f32 %s %s f32 %.3e f16x2 %.3e ratio %.2f" % (case, what, e32, e16, e16 / e32))
        assert e16 <= 2.0 * e32 + 5e-8, (case, what, e32, e16)


def _dgrad_direct(fa, dy, w, case):
    """conv2d_dgrad at precision 3 through the C ABI, with the hand-over the autograd path makes (slot, workspace, image state 1)."""
    from faoctasr._lib import call, ptr, stream_ptr
    N, C, H, W, M, k, s, p, bias, act = case
    dims = (N, C, H, W, M, k, k, s, p)
    wp = torch.empty(fa._lib.load().faoctasr_conv_wpack_floats(1, C, M, k, k, s, p, 3), device="cuda")
    dx = torch.empty(N, C, H, W, device="cuda")
    slot = fa.ops.absmax_slot(dy)
    fa.ops._gather_workspace(dy.device, 1, dims)
    call("conv_set_scales", ptr(slot), None)
    call("conv2d_dgrad", ptr(dy), ptr(w), ptr(dx), *dims, ptr(wp), 1, 3, stream_ptr())
    assert _route(fa) == ROUTE_NARROW_X2, case
    return dx


@pytest.mark.parametrize("case", NARROW_CASES)
def test_narrow_f16x2_route_and_bit_reproducible(fa, case):
    """Forward and input gradient take the narrow f16x2 kernel; two calls give bit-identical results with split-K (the default for
    these small grids: partials in a workspace, summed in a fixed order) and without it (reproducible_forward)."""
    x, w, b, cot = _data(case, 7)
    N, C, H, W, M, k, s, p, bias, act = case
    xd, wd, bd, cd = dev(x), dev(w), dev(b) if b is not None else None, dev(cot)
    fa.ops.conv_precision = 3
    try:
        outs = {}
        for repro in (False, True):
            fa.ops.reproducible_forward = repro
            try:
                ys = []
                for _ in range(2):
                    with torch.no_grad():
                        ys.append(fa.ops.conv2d(xd, wd, bd, s, p, False, act, 0.2))
                    assert _route(fa) == ROUTE_NARROW_X2, case
            finally:
                fa.ops.reproducible_forward = False
            assert torch.equal(ys[0], ys[1]), (case, repro)
            outs[repro] = ys[0]
        assert rel_l2(outs[False], outs[True]) < 1e-6
        # input gradient: called on this thread (the route is per calling thread; autograd runs backward on its own)
        dxs = [_dgrad_direct(fa, cd, wd, case) for _ in range(2)]
        xg = xd.clone().requires_grad_(True)
        (dx_ops,) = torch.autograd.grad(fa.ops.conv2d(xg, wd, bd, s, p, False, None, 0.2), xg, cd)
        torch.cuda.synchronize()
        assert torch.equal(dxs[0], dxs[1]), case
        assert torch.equal(dx_ops, dxs[0]), case
    finally:
        fa.ops.conv_precision = 0


def test_narrow_f16x2_tiny_cotangent(fa):
    """A cotangent 1e-25 times smaller (fp16 could not hold any of it unscaled): the input gradient matches the exact-f32 kernel's, not zero."""
    case = NARROW_CASES[1]
    x, w, b, cot = _data(case, 11, cot_scale=1e-25)
    N, C, H, W, M, k, s, p, bias, act = case
    ref = _ref(x, w, b, s, p, act, cot)
    r32 = _run(fa, 1, case, x, w, b, cot)
    r16 = _run(fa, 3, case, x, w, b, cot)
    assert float(r16[1].abs().max()) > 0
    e32, e16 = rel_l2(r32[1], ref[1]), rel_l2(r16[1], ref[1])
    assert e16 <= 2.0 * e32 + 5e-8, (e32, e16)
    assert rel_l2(r16[1], r32[1]) < 1e-5


@pytest.mark.parametrize("case", [(2, 24, 16, 16, 64, 4, 2, 1, True, None),       # channels not a multiple of 16
                                  (2, 512, 2, 2, 512, 4, 2, 1, False, None),      # a single output pixel
                                  (2, 48, 9, 9, 96, 3, 1, 1, True, "lrelu")])     # 3 channel groups x 9 taps: not whole chunks
def test_narrow_f16x2_fallbacks(fa, case):
    """Shapes outside the narrow f16x2 kernel run correctly on another route (channel counts it does not take) or on it (a single-pixel map)."""
    x, w, b, cot = _data(case, 3)
    N, C, H, W, M, k, s, p, bias, act = case
    ref = _ref(x, w, b, s, p, act, cot)
    out = _run(fa, 3, case, x, w, b, cot)
    for o, r in zip(out, ref):
        assert rel_l2(o, r) < 2e-6, case
    fa.ops.conv_precision = 3
    try:
        with torch.no_grad():
            fa.ops.conv2d(dev(x), dev(w), dev(b) if b is not None else None, s, p, False, act, 0.2)
        r = _route(fa)
    finally:
        fa.ops.conv_precision = 0
    if C % 16 or (C // 16) * k * k % 4:
        assert r != ROUTE_NARROW_X2, (case, r)
