"""The stride-1 3x3 split-operand weight gradient (csrc/wgrad_x3.hip, route 15) with its rolling input window: a block walks its tiles
down a 32-pixel column strip and stages only the two new input rows of a tile that lies below its predecessor, into a ring of 8 row
slots in LDS.  The shapes are the smallest that reach each way the window can go wrong (a stale or misplaced row is an O(1) error);
the slice counts follow from the launcher's slices = min(256 / (gx gy), ntiles / 4)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# N, C, H, W, M
SHAPES = [
    (4, 64, 2, 32, 64),       # tiles_y = 1: every tile starts a column, both halo rows lie outside the image
    (3, 64, 12, 32, 64),      # 18 tiles in 4 slices of 5, 5, 5, 3: an image change inside a slice, ragged last slice
    (2, 64, 12, 64, 64),      # tiles_x = 2, 6 slices of 4: a column change inside a slice
    (8, 256, 32, 32, 256),    # 8 tiles per block down one column: the ring wraps; gx gy = 16
    (2, 64, 64, 64, 128),     # gx != gy, columns of 32 tiles cut into runs of 4
]


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _data(shape):
    """x ~ N(0, 1) and the heavy-tailed ~1e-4 cotangent of test_conv2d_f16x2; dW in fp64 and in fp32 on the CPU (computed once)."""
    N, C, H, W, M = shape
    g = torch.Generator().manual_seed(4242 + sum(shape))
    x = torch.randn(N, C, H, W, generator=g)
    dy = 1e-4 * torch.randn(N, M, H, W, generator=g) * torch.exp(1.5 * torch.randn(N, M, H, W, generator=g))
    ref = {}
    for dt in (torch.float64, torch.float32):
        w = torch.zeros(M, C, 3, 3, dtype=dt, requires_grad=True)
        F.conv2d(x.to(dt), w, None, stride=1, padding=1).backward(dy.to(dt))
        ref[dt] = w.grad
    return x, dy, ref[torch.float64], ref[torch.float32]


class _Runner:
    """conv2d_wgrad through the C ABI on one shape's data, as test_split_wgrad_two_pass_reduction_is_reproducible calls it."""

    def __init__(self, fa, shape):
        from faoctasr._lib import call, ptr, stream_ptr
        self.fa, self.shape = fa, shape
        self.call, self.ptr, self.stream_ptr = call, ptr, stream_ptr
        N, C, H, W, M = shape
        x, dy, self.dw64, self.dw32 = _data(shape)
        self.x, self.dy = x.cuda().contiguous(), dy.cuda().contiguous()
        self.sx, self.sdy = torch.zeros(fa.ops.SLOT_WORDS, device="cuda"), torch.zeros(fa.ops.SLOT_WORDS, device="cuda")
        call("absmax_bits", ptr(self.x), self.x.numel(), ptr(self.sx), stream_ptr())
        call("absmax_bits", ptr(self.dy), self.dy.numel(), ptr(self.sdy), stream_ptr())
        need = fa._lib.load().faoctasr_conv_wgrad_workspace_floats(C, M, 3, 3, 1)
        assert need > 0
        self.ws = torch.empty(need, device="cuda")

    def run(self, precision, workspace=True, dw=None):
        N, C, H, W, M = self.shape
        dw = torch.zeros(M, C, 3, 3, device="cuda") if dw is None else dw.clone()
        if precision == 3:
            self.call("conv_set_scales", self.ptr(self.sx), self.ptr(self.sdy))
        if workspace and precision != 1:
            self.call("conv_set_workspace", self.ptr(self.ws), self.ws.numel())
        self.call("conv2d_wgrad", self.ptr(self.x), self.ptr(self.dy), self.ptr(dw), N, C, H, W, M, 3, 3, 1, 1, 0, 1, precision, self.stream_ptr())
        if precision != 1:
            assert self.fa._lib.load().faoctasr_last_route() == 15, self.shape
        torch.cuda.synchronize()
        return dw


@pytest.mark.parametrize("shape", SHAPES)
def test_rolling_wgrad_bf16x3(fa, shape):
    """precision 2: relative L2 error < 3e-5 against the fp32 CPU result (the bar of test_conv2d_bf16x3), with and without a workspace."""
    r = _Runner(fa, shape)
    for workspace in (True, False):
        e = rel_l2(r.run(2, workspace), r.dw32)
        print("rolling bf16x3 %s workspace=%s rel_l2 %.3e" % (shape, workspace, e))
        assert e < 3e-5, (shape, workspace, e)


@pytest.mark.parametrize("shape", SHAPES)
def test_rolling_wgrad_f16x2(fa, shape):
    """precision 3 against an fp64 convolution, beside the exact-f32 kernels on the same data: error <= 2x theirs + 5e-8 and < 2e-6
    (the bars of test_conv2d_f16x2)."""
    r = _Runner(fa, shape)
    e32 = rel_l2(r.run(1), r.dw64)
    for workspace in (True, False):
        e16 = rel_l2(r.run(3, workspace), r.dw64)
        print("rolling f16x2 %s workspace=%s f32 %.3e f16x2 %.3e ratio %.2f" % (shape, workspace, e32, e16, e16 / e32))
        assert e16 <= 2.0 * e32 + 5e-8, (shape, workspace, e32, e16)
        assert e16 < 2e-6, (shape, workspace, e16)


@pytest.mark.parametrize("shape", SHAPES)
def test_rolling_wgrad_reproducible_and_accumulates(fa, shape):
    """With a workspace two runs give the same bits; the atomics form (no workspace) agrees to summation-order noise (2e-6); and a
    non-zero dW is added to, not overwritten: the second pass adds each element's slice sum to dW once, so dW0 + (run into zeros) is
    what a run into dW0 must give, bit for bit."""
    r = _Runner(fa, shape)
    a, b = r.run(3), r.run(3)
    assert torch.equal(a, b)
    atomics = r.run(3, workspace=False)
    e = rel_l2(atomics, a)
    print("rolling f16x2 %s atomics vs two-pass rel_l2 %.3e" % (shape, e))
    assert e < 2e-6, (shape, e)
    g = torch.Generator().manual_seed(7)
    dw0 = (torch.randn(a.shape, generator=g) * float(a.abs().mean())).cuda()
    assert torch.equal(r.run(3, dw=dw0), dw0 + a)
    # atomics form: at most 256 slices each add their partial into dW0 + ..., one fp32 rounding (2^-24 relative) per add, on top of
    # the 2e-6 allowed between the two forms above
    assert rel_l2(r.run(3, workspace=False, dw=dw0), dw0 + a) < 2e-6 + 256 * 2.0 ** -24
