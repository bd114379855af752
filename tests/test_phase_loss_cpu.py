"""Host-side checks of the spectral phase-consistency loss (reference model.py:36-58): the public names, the C ABI's argument
checks, and the float64 ``torch.fft`` restatement of the formula that the GPU tests lean on -- pinned here to the fixture the
reference itself produced (tests/golden/golden_phase.npz, written by tools/gen_golden_phase.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_phase.npz")
NEW_SYMBOLS = ("faoctasr_dft_tables", "faoctasr_phase_loss_workspace_floats", "faoctasr_phase_loss_fwd", "faoctasr_phase_loss_bwd")


def restatement(x, y, radius=5.0, dtype=torch.float64):
    """The reference's formula with stock ops in ``dtype``, per sample and averaged over the batch: (loss, dloss/dx, dloss/dy).
    The mask is built in double and rounded once, as the reference does."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    B, C, H, W = x.shape
    i = torch.arange(H, dtype=torch.float64)[:, None] - H // 2
    j = torch.arange(W, dtype=torch.float64)[None, :] - W // 2
    m = (1 - torch.exp(-0.5 * (i * i + j * j) / radius ** 2)).to(dtype)
    total = 0
    for b in range(B):
        ax = (m * torch.log(torch.abs(torch.fft.fftshift(torch.fft.fft2(x[b]), dim=(-2, -1))))).flatten()
        ay = (m * torch.log(torch.abs(torch.fft.fftshift(torch.fft.fft2(y[b]), dim=(-2, -1))))).flatten()
        total = total - torch.cosine_similarity(ax, ay, dim=0)
    loss = total / B
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach().double(), gx.double(), gy.double()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def lib():
    import faoctasr
    return faoctasr._lib.load()


def test_public_names_exist():
    import faoctasr
    assert callable(faoctasr.ops.phase_loss)
    crit = faoctasr.phase_consistency_loss()               # no-argument constructor, as at the reference's train.py:94
    assert isinstance(crit, torch.nn.Module) and crit.radius == 5
    assert "phase_consistency_loss" in faoctasr.__all__
    assert faoctasr.model.phase_consistency_loss is faoctasr.phase_consistency_loss


def test_new_symbols_in_header_and_library(lib):
    import faoctasr
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in faoctasr._lib.declared_symbols(), s
        assert hasattr(lib, s), s
    assert lib.faoctasr_version() >= 410


def test_workspace_query(lib):
    n = lib.faoctasr_phase_loss_workspace_floats(8, 1, 256, 256)
    # at least the spectrum planes of both images (Re and -Im) and the row-pass buffer
    assert n >= 2 * 8 * 2 * 256 * 256
    assert lib.faoctasr_phase_loss_workspace_floats(1, 1, 2, 2) > 0
    assert lib.faoctasr_phase_loss_workspace_floats(3, 2, 63, 50) > lib.faoctasr_phase_loss_workspace_floats(3, 1, 63, 50)


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.faoctasr_phase_loss_workspace_floats(1, 1, 1, 64) < 0
    assert b"H" in lib.faoctasr_last_error()
    rc = lib.faoctasr_phase_loss_fwd(p, p, p, p, 5.0, p, p, p, 1, 1, 1, 64, None)            # H < 2
    assert rc == -1 and b"phase_loss_fwd" in lib.faoctasr_last_error()
    rc = lib.faoctasr_phase_loss_fwd(p, p, p, p, 5.0, p, p, p, 1, 1, 64, 1, None)            # W < 2
    assert rc == -1 and b"phase_loss_fwd" in lib.faoctasr_last_error()
    for radius in (0.0, -1.0, float("nan")):
        rc = lib.faoctasr_phase_loss_fwd(p, p, p, p, radius, p, p, p, 1, 1, 64, 64, None)
        assert rc == -1 and b"radius" in lib.faoctasr_last_error()
        rc = lib.faoctasr_phase_loss_bwd(p, p, p, radius, p, p, p, 1, 1, 64, 64, None)
        assert rc == -1 and b"radius" in lib.faoctasr_last_error()
    rc = lib.faoctasr_phase_loss_fwd(None, p, p, p, 5.0, p, p, p, 1, 1, 64, 64, None)
    assert rc == -1 and b"null" in lib.faoctasr_last_error()
    rc = lib.faoctasr_phase_loss_bwd(p, p, p, 5.0, p, p, p, 1, 1, 1, 64, None)
    assert rc == -1 and b"phase_loss_bwd" in lib.faoctasr_last_error()
    assert lib.faoctasr_dft_tables(None, 8, None) == -1
    assert lib.faoctasr_dft_tables(p, 0, None) == -1


def test_no_cpu_fallback():
    import faoctasr
    x = torch.rand(1, 1, 8, 8)
    with pytest.raises(faoctasr.KernelError):
        faoctasr.ops.phase_loss(x, x)
    with pytest.raises(faoctasr.KernelError):
        faoctasr.phase_consistency_loss()(x, x)


def test_restatement_reproduces_the_reference_fixture():
    """float64 restatement against the reference's fp32 CPU result.  The fixture's own rounding is the only difference: the
    loss within 4 fp32 ulps at |loss| ~ 1 (measured 1.2e-7 - 2.0e-7), each gradient within 2e-5 relative L2 (measured ~3e-6: the
    two terms of dloss/da nearly cancel at cosine similarity 0.99)."""
    g = np.load(GOLD)
    assert [tuple(s) for s in g["shapes"]] == [(64, 64), (48, 80), (31, 50)]
    for H, W in g["shapes"]:
        tag = "%dx%d" % (H, W)
        x, y = torch.from_numpy(g["x_" + tag]), torch.from_numpy(g["y_" + tag])
        assert x.shape == (1, 1, H, W) and x.dtype == torch.float32
        loss, gx, gy = restatement(x, y)
        e_loss = abs(float(loss) - float(g["loss_" + tag]))
        e_gx, e_gy = rel_l2(torch.from_numpy(g["gx_" + tag]), gx), rel_l2(torch.from_numpy(g["gy_" + tag]), gy)
        print("fixture vs fp64 restatement %s: loss %.3e  gx %.3e  gy %.3e" % (tag, e_loss, e_gx, e_gy))
        assert e_loss <= 4.8e-7, (tag, e_loss)
        assert e_gx <= 2e-5 and e_gy <= 2e-5, (tag, e_gx, e_gy)


def test_dropping_the_fftshift_and_the_real_gemm_form():
    """The two facts the kernels rest on, in float64: (1) the mask evaluated at the centred frequency of each UNSHIFTED bin,
    u_c = ((u + H//2) mod H) - H//2, gives the reference's loss without moving data, even and odd sizes; (2) the DFT of a real
    image is Re = C X C - S X S, Im = -(S X C + C X S) with the symmetric cos / sin tables."""
    torch.manual_seed(5)
    for H, W in ((64, 64), (96, 128), (63, 50), (31, 2)):
        x = torch.tanh(torch.randn(2, 1, H, W))
        y = torch.tanh(x + 0.3 * torch.randn(2, 1, H, W))
        want, _, _ = restatement(x, y)

        def tables(n):
            k = torch.arange(n)
            a = 2 * torch.pi * ((k[:, None] * k[None, :]) % n).double() / n
            return torch.cos(a), torch.sin(a)
        (CH, SH), (CW, SW) = tables(H), tables(W)
        uc = ((torch.arange(H) + H // 2) % H - H // 2).double()[:, None]
        vc = ((torch.arange(W) + W // 2) % W - W // 2).double()[None, :]
        m = 1 - torch.exp(-0.5 * (uc * uc + vc * vc) / 25.0)

        def amp(t):
            t = t.double()[:, 0]
            p, q = t @ CW, t @ SW
            re, im = CH @ p - SH @ q, -(SH @ p + CH @ q)
            f = torch.fft.fft2(t)
            assert torch.allclose(re, f.real, atol=1e-9) and torch.allclose(im, f.imag, atol=1e-9)
            return (m * 0.5 * torch.log(re * re + im * im)).flatten(1)
        ax, ay = amp(x), amp(y)
        got = (-(ax * ay).sum(1) / (ax.norm(dim=1) * ay.norm(dim=1))).mean()
        assert abs(float(got) - float(want)) < 1e-12, (H, W, float(got), float(want))


def test_train_step_accepts_the_phase_term():
    import faoctasr
    sig = inspect.signature(faoctasr.TrainStep.__init__)
    assert sig.parameters["phase_weight"].default == 0.0
    assert sig.parameters["phase_radius"].default == 5.0
