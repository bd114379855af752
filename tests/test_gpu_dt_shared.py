"""The transform (dtcwt.hip), the scattering layers (scat.hip) and the magnitude loss (dtcwt_loss.hip) run the same tile bodies
(csrc/dtcwt_dev.h), so where two families compute the same lowpass they compute the same filter sums in the same order: the
results are equal bit for bit, on an input with a remainder tile in both axes.  The entry points are driven as ops.py drives
them (the third filter NULL for a two-filter bank), on tensors allocated here; the taps are bank "a" of the dual-tree fixtures and
the three-filter fixture bank."""
import pytest
import torch

from test_dtcwt_cpu import bufs as bufs_a
from test_rot_cpu import bufs as bufs_rot

pytestmark = pytest.mark.gpu

N, C = 1, 2
MODES = {"symmetric": 1, "zero": 0}


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    faoctasr._lib.load()
    return faoctasr


def host(b, names):
    return tuple(tuple(b[n].float().tolist()) for n in names)


def image(seed, H, W):
    return torch.randn((N, C, H, W), generator=torch.Generator().manual_seed(seed)).cuda()


def transform_ll(fa, x, taps, level1, mode=1):
    """ll of one launch of the transform, the bandpass computed beside it as the modules do."""
    _, _, H, W = x.shape
    lh, lw = (H, W) if level1 else (H // 2, W // 2)
    ll = torch.full((N, C, lh, lw), float("nan"), device="cuda")
    hi = torch.empty((N, C, 6, lh // 2, lw // 2, 2), device="cuda")
    st, vec = fa.ops._dtcwt_high_strides(hi, "ncohwr")
    head = (x.data_ptr(),) + x.stride()[:3] + (ll.data_ptr(), hi.data_ptr()) + st + (vec, N, C, H, W)
    if level1:
        fa._lib.call("dtcwt_fwd_j1", *head, *fa.ops._taps1_args(taps), mode, fa._lib.stream_ptr())
    else:
        fa._lib.call("dtcwt_fwd_j2", *head, *fa.ops._taps2_args(taps), fa._lib.stream_ptr())
    return ll


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("bank", ["two_filter", "bp"])
def test_scat_level1_lowpass_is_the_transforms(fa, bank, mode):
    """``scat_fwd_j1`` without pooling writes ll itself: 20 x 72 is the 16 x 64 tile and a remainder in both axes."""
    taps = host(bufs_a("a"), ("h0o", "h1o")) if bank == "two_filter" else host(bufs_rot(), ("h0o", "h1o", "h2o"))
    H, W = 20, 72
    x = image(1, H, W)
    low = torch.full((N, C, H, W), float("nan"), device="cuda")
    mag = torch.empty((N, 6, C, H // 2, W // 2), device="cuda")
    fa._lib.call("scat_fwd_j1", x.data_ptr(), *x.stride()[:3], *fa.ops._scat_low(low), 0, *fa.ops._scat_mag(mag, False),
                 None, 0, 1e-2, 1e-4, N, C, H, W, *fa.ops._taps1_args(taps), MODES[mode], fa._lib.stream_ptr())
    want = transform_ll(fa, x, taps, True, MODES[mode])
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and torch.equal(low, want)


@pytest.mark.parametrize("level1", [True, False], ids=["level1_20x72", "level2_20x136"])
def test_loss_lowpasses_are_the_transforms(fa, level1):
    """``dtcwt_loss_fwd_j1`` / ``_j2`` write the lowpass of both images for the next level; the level >= 2 tile is 16 x 128 of the
    input."""
    b = bufs_a("a")
    taps = host(b, ("h0o", "h1o")) if level1 else host(b, ("h0a", "h0b", "h1a", "h1b"))
    H, W = (20, 72) if level1 else (20, 136)
    x, y = image(2, H, W), image(3, H, W)
    lh, lw = (H, W) if level1 else (H // 2, W // 2)
    llx, lly = (torch.full((N, C, lh, lw), float("nan"), device="cuda") for _ in range(2))
    floats = fa._lib.load().faoctasr_dtcwt_loss_workspace_floats(N, C, H, W, int(level1))
    assert floats > 0
    part = torch.empty(floats, device="cuda")
    head = (x.data_ptr(),) + x.stride()[:3] + (y.data_ptr(),) + y.stride()[:3] + (llx.data_ptr(), lly.data_ptr(), None, None, part.data_ptr(),
                                                                                  1.0, 1e-4, N, C, H, W)
    if level1:
        fa._lib.call("dtcwt_loss_fwd_j1", *head, *fa.ops._taps1_args(taps)[:4], 1, fa._lib.stream_ptr())       # the loss takes two filters
    else:
        fa._lib.call("dtcwt_loss_fwd_j2", *head, *(fa.ops._tap_array(t) for t in taps), len(taps[0]), fa._lib.stream_ptr())
    wx, wy = transform_ll(fa, x, taps, level1), transform_ll(fa, y, taps, level1)
    torch.cuda.synchronize()
    assert torch.isfinite(wx).all() and torch.isfinite(wy).all() and not torch.equal(wx, wy)
    assert torch.equal(llx, wx) and torch.equal(lly, wy)
