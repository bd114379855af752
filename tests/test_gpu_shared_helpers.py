"""What the helpers shared across the kernel files (csrc/common.h, csrc/filterbank_dev.h) must keep.

The single-block finish kernels add a loss's block partials in a documented order: thread t adds partials t, t + 256, ... one
after the other in double, then ``red[:o] += red[o:2 o]`` for o = 128 .. 1 adds the threads.  ``dtcwt_loss_final`` and
``cwssim_final`` are fed partials from the caller's side, built so that the order of the additions shows after the cast to
float32, and compared exactly with a NumPy restatement of that order.

The 2-D and the 1-D filter bank share one extension map and one tap order: with the H-axis pair lo = (1, 0), hi = (0, 1) on
six rows (no extension along H, base 0) the four bands of ``afb2d`` are the even and the odd rows of ``afb1d`` of every row,
bit for bit, in all five padding modes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def partials(n, seed):
    """n float32 values whose sum cancels: N(0, 1) * 10^U(-6, 6) with its negatives (and one value of order 1e-9 for odd n), shuffled."""
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal(n // 2) * 10.0 ** rng.uniform(-6.0, 6.0, n // 2)).astype(np.float32)
    v = np.concatenate([h, -h, np.full(n % 2, 1.5e-9, np.float32)])
    rng.shuffle(v)
    assert v.size == n and v.dtype == np.float32
    return v


def documented_sum(p):
    """Thread t adds p[t::256] sequentially in float64, then the fixed tree over the 256 threads."""
    red = np.zeros(256, np.float64)
    for t in range(256):
        a = 0.0
        for v in p[t::256]:
            a += float(v)
        red[t] = a
    o = 128
    while o:
        red[:o] += red[o:2 * o]
        o >>= 1
    return float(red[0])


def sequential_sum(p):
    a = 0.0
    for v in p:
        a += float(v)
    return a


def test_dtcwt_loss_final_adds_in_the_documented_order(fa):
    sizes, scales = (1000, 77), (0.75, 1.5)
    parts = [partials(n, 11 + j) for j, n in enumerate(sizes)]

    def total(level_sum):
        t = 0.0
        for p, s in zip(parts, scales):
            t += level_sum(p) * s
        return np.float32(t)

    want = total(documented_sum)
    assert want != total(sequential_sum)                     # the fixture shows the order
    ws = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.full((), float("nan"), device="cuda")
    J = len(sizes)
    fa._lib.call("dtcwt_loss_final", ws.data_ptr(), ctypes.cast((ctypes.c_long * J)(*sizes), ctypes.c_void_p),
                 ctypes.cast((ctypes.c_double * J)(*scales), ctypes.c_void_p), J, out.data_ptr(), fa._lib.stream_ptr())
    got = np.float32(out.item())
    print("dtcwt_loss_final: got %r, documented order %r, sequential %r" % (got, want, total(sequential_sum)))
    assert got == want


def test_cwssim_final_adds_in_the_documented_order(fa):
    N, planes, h, w, win = 2, 12, 119, 391, 7                # 113 x 385 positions: 8 x 7 tiles a plane, 6 planes an image
    floats = fa._lib.load().faoctasr_cwssim_workspace_floats(planes, h, w, win)     # as ops.py sizes the workspace
    per_image = floats // N
    assert floats == N * per_image and per_image > 256 and per_image % 256
    parts = [partials(per_image, 21 + n) for n in range(N)]
    count = float(planes // N) * float(h - win + 1) * float(w - win + 1)

    def images(image_sum):
        return [image_sum(p) / count for p in parts]

    m = images(documented_sum)
    want_image = np.array(m, np.float64).astype(np.float32)
    want_mean = np.float32((0.0 + m[0] + m[1]) / float(N))
    seq = images(sequential_sum)
    assert all(np.float32(a) != np.float32(b) for a, b in zip(m, seq))              # the fixture shows the order
    assert want_mean != np.float32((0.0 + seq[0] + seq[1]) / float(N))
    ws = torch.from_numpy(np.concatenate(parts)).cuda()
    out_image = torch.full((N,), float("nan"), device="cuda")
    out_mean = torch.full((), float("nan"), device="cuda")
    fa._lib.call("cwssim_final", ws.data_ptr(), N, planes, h, w, win, out_image.data_ptr(), out_mean.data_ptr(), fa._lib.stream_ptr())
    got_image, got_mean = out_image.cpu().numpy(), np.float32(out_mean.item())
    print("cwssim_final: got %r %r, documented order %r %r" % (got_image, got_mean, want_image, want_mean))
    assert np.array_equal(got_image, want_image) and got_mean == want_mean


@pytest.mark.parametrize("mode", [0, 1, 2, 4, 6], ids=["zero", "symmetric", "periodization", "reflect", "periodic"])
@pytest.mark.parametrize("W", [37, 150])
def test_2d_bank_rows_are_the_1d_bank(fa, W, mode):
    """db4 along W; 150 columns give 78 (75) outputs, three 32-wide analysis tiles with a remainder; 37 is odd (periodization's
    Ne = N + 1).  Both kernels form fmaf(f[k], v, acc) for k ascending, and the H pass adds exact zeros."""
    d4 = fa.daubechies(4)
    lo_w, hi_w = list(d4.dec_lo)[::-1], list(d4.dec_hi)[::-1]
    x = torch.randn((1, 2, 6, W), generator=torch.Generator().manual_seed(W)).cuda()
    ll, hi = fa.ops.afb2d(x, lo_w, hi_w, [1.0, 0.0], [0.0, 1.0], mode)
    lo1, hi1 = fa.ops.afb1d(x.reshape(1, 12, W), lo_w, hi_w, mode)
    O = lo1.shape[-1]
    lo1, hi1 = lo1.reshape(1, 2, 3, 2, O), hi1.reshape(1, 2, 3, 2, O)               # (.., row pair, even / odd row, O)
    assert ll.shape == (1, 2, 3, O) and hi.shape == (1, 2, 3, 3, O) and torch.isfinite(lo1).all() and torch.isfinite(hi1).all()
    assert torch.equal(ll, lo1[:, :, :, 0])                  # (w lo, h lo): even rows of the lowpass
    assert torch.equal(hi[:, :, 0], lo1[:, :, :, 1])         # (w lo, h hi): odd rows of the lowpass
    assert torch.equal(hi[:, :, 1], hi1[:, :, :, 0])         # (w hi, h lo): even rows of the highpass
    assert torch.equal(hi[:, :, 2], hi1[:, :, :, 1])         # (w hi, h hi): odd rows of the highpass
