"""Host-side checks of the total-variation loss (reference model.py:17-33): the float64 restatement of the formula and the
closed-form gradient the stencil kernel implements -- both pinned to the fixture the reference itself produced
(tests/golden/golden_tv.npz, written by tools/gen_golden_tv.py) -- the module's unchanged CPU path, the public names and the
C ABI's argument checks."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_tv.npz")
NEW_SYMBOLS = ("faoctasr_tv_loss_workspace_floats", "faoctasr_tv_loss_fwd", "faoctasr_tv_loss_bwd")


def restatement(x, weight=1.0, dtype=torch.float64):
    """The reference's formula with stock ops on the CPU in ``dtype``: (loss, dloss/dx) as float64."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    b, c, h, w = x.shape
    h_tv = ((x[:, :, 1:, :] - x[:, :, :h - 1, :]) ** 2).sum()
    w_tv = ((x[:, :, :, 1:] - x[:, :, :, :w - 1]) ** 2).sum()
    loss = weight * 2 * (h_tv / (c * (h - 1) * w) + w_tv / (c * h * (w - 1))) / b
    g, = torch.autograd.grad(loss, x)
    return loss.detach().double(), g.double()


def closed_form_gradient(x, weight=1.0):
    """dx[i,j] = s (2/count_h ((x[i,j]-x[i-1,j]) [i>0] - (x[i+1,j]-x[i,j]) [i<H-1]) + 2/count_w (the same along j)), s = weight 2 / B,
    in float64: what ``faoctasr_tv_loss_bwd`` computes for an upstream gradient of 1."""
    x = x.detach().cpu().double()
    b, c, h, w = x.shape
    dv, dh = x[:, :, 1:, :] - x[:, :, :-1, :], x[:, :, :, 1:] - x[:, :, :, :-1]
    a, bb = torch.zeros_like(x), torch.zeros_like(x)
    a[:, :, 1:, :] += dv
    a[:, :, :-1, :] -= dv
    bb[:, :, :, 1:] += dh
    bb[:, :, :, :-1] -= dh
    return weight * 2 / b * (2 / (c * (h - 1) * w) * a + 2 / (c * h * (w - 1)) * bb)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def fixture_rows():
    g = np.load(GOLD)
    for shape in g["shapes"]:
        tag = "%dx%dx%dx%d" % tuple(shape)
        x = torch.from_numpy(g["x_" + tag])
        for w in g["weights"]:
            yield tag, tuple(int(v) for v in shape), float(w), x, float(g["loss_w%g_%s" % (w, tag)]), torch.from_numpy(g["g_w%g_%s" % (w, tag)])


@pytest.fixture(scope="module")
def lib():
    import faoctasr
    return faoctasr._lib.load()


def test_fixture_contents():
    g = np.load(GOLD)
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    assert shapes == [(1, 1, 64, 64), (2, 1, 48, 80), (2, 3, 31, 50), (1, 1, 2, 2)]
    assert list(g["weights"]) == [1.0, 0.5]
    assert os.path.getsize(GOLD) < 512 * 1024
    for tag, shape, w, x, loss, grad in fixture_rows():
        assert tuple(x.shape) == shape and x.dtype == torch.float32 and grad.dtype == torch.float32
        assert float(x.abs().max()) < 1.0               # tanh(randn)


def test_restatement_reproduces_the_reference_fixture():
    """float64 restatement against the reference's fp32 CPU result: the fixture's own fp32 rounding is the only difference.
    Loss within 4 fp32 ulps of |loss| (measured 0.29 - 1.02 ulp), gradient within 4 * 2^-23 in relative L2 (measured 4.7e-8 - 7.4e-8)."""
    for tag, shape, w, x, loss, grad in fixture_rows():
        l64, g64 = restatement(x, w)
        e_loss, e_g = abs(float(l64) - loss), rel_l2(grad, g64)
        print("fixture vs fp64 restatement %s weight %g: loss %.3e (%.2f ulp)  gradient %.3e" % (tag, w, e_loss, e_loss / (abs(float(l64)) * 2.0 ** -23), e_g))
        assert e_loss <= 4 * abs(float(l64)) * 2.0 ** -23, (tag, w, e_loss)
        assert e_g <= 4 * 2.0 ** -23, (tag, w, e_g)


def test_closed_form_gradient_matches_autograd():
    """The stencil of the backward kernel against autograd of the restatement, in float64: fixture shapes and the edge sizes
    (H or W of 2, odd W, W not a multiple of 4)."""
    for tag, shape, w, x, loss, grad in fixture_rows():
        _, g64 = restatement(x, w)
        assert rel_l2(closed_form_gradient(x, w), g64) < 1e-14, (tag, w)
    torch.manual_seed(3)
    for shape in ((1, 1, 2, 2), (1, 1, 2, 257), (1, 1, 130, 2), (3, 2, 7, 5), (2, 1, 9, 12)):
        x = torch.tanh(torch.randn(*shape))
        _, g64 = restatement(x, 0.5)
        assert rel_l2(closed_form_gradient(x, 0.5), g64) < 1e-14, shape


def test_module_on_cpu_tensors_still_equals_the_fixture():
    """``TVLoss`` on CPU tensors keeps the reference's composition of stock ops: bit-equal to the reference's fp32 result."""
    import faoctasr
    for tag, shape, w, x, loss, grad in fixture_rows():
        crit = faoctasr.TVLoss(TVLoss_weight=w)
        assert crit.TVLoss_weight == w
        xr = x.clone().requires_grad_(True)
        out = crit(xr)
        out.backward()
        assert float(out.detach()) == loss, (tag, w, float(out.detach()), loss)
        assert torch.equal(xr.grad, grad), (tag, w)
    assert faoctasr.TVLoss().TVLoss_weight == 1
    # other dtypes and degenerate sizes stay on the composition as well
    x64 = torch.rand(1, 1, 5, 6, dtype=torch.float64)
    assert faoctasr.TVLoss()(x64).dtype == torch.float64


def test_new_symbols_in_header_and_library(lib):
    import faoctasr
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in faoctasr._lib.declared_symbols(), s
        assert hasattr(lib, s), s
    assert lib.faoctasr_version() >= 420


def test_ops_tv_loss_exists_and_has_no_cpu_fallback():
    import faoctasr
    assert callable(faoctasr.ops.tv_loss)
    with pytest.raises(faoctasr.KernelError):
        faoctasr.ops.tv_loss(torch.rand(1, 1, 8, 8))


def test_train_step_accepts_the_tv_term():
    import faoctasr
    sig = inspect.signature(faoctasr.TrainStep.__init__)
    assert sig.parameters["tv_weight"].default == 0.0


def test_workspace_query(lib):
    """Two partial sums per 256-thread block; the scalar path's block count (one thread per 8 rows of one column) bounds it."""
    assert lib.faoctasr_tv_loss_workspace_floats(8, 1, 256, 256) == 2 * (8 * 32 * 256 // 256)
    assert lib.faoctasr_tv_loss_workspace_floats(1, 1, 2, 2) == 2
    assert lib.faoctasr_tv_loss_workspace_floats(3, 2, 63, 50) > lib.faoctasr_tv_loss_workspace_floats(3, 1, 63, 50)


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.faoctasr_tv_loss_workspace_floats(1, 1, 1, 64) < 0
    assert b"H" in lib.faoctasr_last_error()
    for H, W in ((1, 64), (64, 1)):
        rc = lib.faoctasr_tv_loss_fwd(p, p, p, 1, 1, H, W, 1.0, None)
        assert rc == -1 and b"tv_loss_fwd" in lib.faoctasr_last_error()
        rc = lib.faoctasr_tv_loss_bwd(p, p, p, 1, 1, H, W, 1.0, None)
        assert rc == -1 and b"tv_loss_bwd" in lib.faoctasr_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        rc = lib.faoctasr_tv_loss_fwd(*args, 1, 1, 64, 64, 1.0, None)
        assert rc == -1 and b"null" in lib.faoctasr_last_error()
        rc = lib.faoctasr_tv_loss_bwd(*args, 1, 1, 64, 64, 1.0, None)
        assert rc == -1 and b"null" in lib.faoctasr_last_error()
