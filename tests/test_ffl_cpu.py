"""Host-side checks of the focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021): the float64 restatement of the definition that
the GPU tests lean on, pinned to the fixture (tests/golden/golden_ffl.npz, written by tools/gen_golden_ffl.py); the two
identities the kernels rest on; the public names, the host-side refusals and the C ABI's argument checks."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_ffl.npz")
NEW_SYMBOLS = ("faoctasr_ffl_workspace_floats", "faoctasr_ffl_fwd", "faoctasr_ffl_bwd")
SETTINGS = ((1.0, False, False), (0.5, True, False), (2.0, False, True), (0.0, False, False))
SHAPES = ((1, 1, 2, 2), (1, 1, 2, 3), (3, 1, 63, 50), (2, 1, 65, 70), (2, 2, 96, 64), (3, 1, 16, 16))


def restatement(x, y, alpha=1.0, log_matrix=False, batch_matrix=False, dtype=torch.float64):
    """The literal definition with ``torch.fft`` on the CPU in ``dtype``: (loss, dL/dx, dL/dy)."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    D = torch.fft.fft2(x, norm="ortho") - torch.fft.fft2(y, norm="ortho")
    q = D.real ** 2 + D.imag ** 2
    with torch.no_grad():
        w = torch.sqrt(q) ** alpha
        if log_matrix:
            w = torch.log(w + 1)
        w = w / (w.max() if batch_matrix else w.amax(dim=(-2, -1), keepdim=True))
        w[torch.isnan(w)] = 0
        w = torch.clamp(w, 0, 1)
    loss = (w * q).mean()
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach().double(), gx.double(), gy.double()


def factorised(x, y, alpha, log_matrix, batch_matrix):
    """What the kernels compute, in float64: ONE transform of x - y, the loss as (sum phi(q) q) / phi(M) per plane, the
    gradient as (2 / count) Re ifft2(w D) and its negation.  A plane (batch) with M = 0 has weight 0."""
    d = (x.double() - y.double())
    D = torch.fft.fft2(d, norm="ortho")
    q = D.real ** 2 + D.imag ** 2

    def phi(t):
        w = torch.ones_like(t) if alpha == 0 else t ** (alpha / 2)
        return torch.log(w + 1) if log_matrix else w
    M = q.amax(dim=(-2, -1), keepdim=True)
    if batch_matrix:
        M = M.max().expand_as(M)
    pm = phi(M)
    inv = torch.where(pm > 0, 1 / pm, torch.zeros_like(pm))
    loss = ((phi(q) * q).sum(dim=(-2, -1), keepdim=True) * inv).sum() / q.numel()
    gx = 2.0 / q.numel() * torch.fft.ifft2(phi(q) * inv * D, norm="ortho").real
    return loss, gx, -gx


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tag_of(shape, setting):
    return "%s_a%g_l%d_b%d" % ("x".join(str(s) for s in shape), setting[0], setting[1], setting[2])


def case_inputs(g, shape):
    case = "x".join(str(s) for s in shape)
    return torch.from_numpy(g["x_" + case]), torch.from_numpy(g["y_" + case])


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


@pytest.fixture(scope="module")
def lib(fa):
    return fa._lib.load()


def test_restatement_reproduces_the_fixture():
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < (1 << 20)
    assert [tuple(s) for s in g["shapes"]] == list(SHAPES)
    assert [(a, bool(l), bool(b)) for a, l, b in g["settings"]] == list(SETTINGS)
    for shape in SHAPES:
        x, y = case_inputs(g, shape)
        assert tuple(x.shape) == shape and x.dtype == torch.float32
        for st in SETTINGS:
            t = tag_of(shape, st)
            loss, gx, gy = restatement(x, y, *st)
            assert abs(float(loss) - float(g["loss64_" + t])) <= 1e-12 * abs(float(g["loss64_" + t])), t
            assert abs(float(gx.norm()) - float(g["gnorm64_" + t])) <= 1e-12 * float(g["gnorm64_" + t]), t
            if "gx64_" + t in g:
                assert rel_l2(gx, torch.from_numpy(g["gx64_" + t])) <= 1e-12, t
            # the fp32 run of the same definition is the GPU tests' yardstick.  Its last bits depend on the host's FFT code path, so
            # the file's figures are held to the class of an fp32 error, and so is this host's run -- not to each other's bits
            l32, gx32, _ = restatement(x, y, *st, dtype=torch.float32)
            assert abs(float(g["loss32_" + t]) - float(loss)) <= 1e-6 * abs(float(loss)) and 1e-8 < float(g["gerr32_" + t]) < 1e-6, t
            assert abs(float(l32) - float(loss)) <= 1e-6 * abs(float(loss)) and rel_l2(gx32, gx) < 1e-6, t


def test_one_transform_one_pass_and_the_ifft_gradient():
    """The identities the kernels rest on, against autograd of the literal definition in float64, to 1e-12: F(x) - F(y) =
    F(x - y); sum w q = (sum phi(q) q) / phi(M); dL/dx = (2 / count) Re ifft2(w D); dL/dy = -dL/dx exactly."""
    g = np.load(GOLD)
    for shape in SHAPES:
        x, y = case_inputs(g, shape)
        for st in SETTINGS:
            want, wx, wy = restatement(x, y, *st)
            got, gx, gy = factorised(x, y, *st)
            assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (shape, st)
            assert rel_l2(gx, wx) <= 1e-12 and rel_l2(gy, wy) <= 1e-12, (shape, st)
            assert torch.equal(wy, -wx) and torch.equal(gy, -gx)


def test_alpha_zero_is_the_mean_squared_error():
    g = np.load(GOLD)
    for shape in SHAPES:
        x, y = case_inputs(g, shape)
        mse = ((x.double() - y.double()) ** 2).mean()
        for log_matrix in (False, True):
            loss, gx, _ = restatement(x, y, 0.0, log_matrix, False)
            assert abs(float(loss) - float(mse)) <= 1e-12 * float(mse)
            assert rel_l2(gx, 2 * (x.double() - y.double()) / x.numel()) <= 1e-12


def test_identical_sample_has_zero_weight_and_zero_gradient():
    g = np.load(GOLD)
    x, y = case_inputs(g, (3, 1, 16, 16))
    assert torch.equal(x[1], y[1]) and not torch.equal(x[0], y[0])
    for st in SETTINGS:
        loss, gx, gy = restatement(x, y, *st)
        assert torch.isfinite(loss) and float(loss) > 0
        assert not gx[1].any() and not gy[1].any() and gx[0].any()
    same, gx, gy = restatement(x, x.clone())
    assert float(same) == 0 and not gx.any() and not gy.any()


def test_public_names_exist(fa):
    assert callable(fa.ops.focal_frequency_loss)
    assert "FocalFrequencyLoss" in fa.__all__ and fa.model.FocalFrequencyLoss is fa.FocalFrequencyLoss
    sig = inspect.signature(fa.ops.focal_frequency_loss)
    assert list(sig.parameters) == ["x", "y", "alpha", "log_matrix", "batch_matrix"]
    assert [sig.parameters[k].default for k in ("alpha", "log_matrix", "batch_matrix")] == [1.0, False, False]


def test_module_signature_defaults_and_repr(fa):
    sig = inspect.signature(fa.FocalFrequencyLoss.__init__)
    assert list(sig.parameters) == ["self", "loss_weight", "alpha", "log_matrix", "batch_matrix"]
    assert [sig.parameters[k].default for k in ("loss_weight", "alpha", "log_matrix", "batch_matrix")] == [1.0, 1.0, False, False]
    assert list(inspect.signature(fa.FocalFrequencyLoss.forward).parameters) == ["self", "pred", "target"]
    m = fa.FocalFrequencyLoss()
    assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(m.buffers())
    assert (m.loss_weight, m.alpha, m.log_matrix, m.batch_matrix) == (1.0, 1.0, False, False)
    assert repr(m) == "FocalFrequencyLoss(loss_weight=1, alpha=1, log_matrix=False, batch_matrix=False)"
    m = fa.FocalFrequencyLoss(loss_weight=0.25, alpha=0.5, log_matrix=True, batch_matrix=True)
    assert m.extra_repr() == "loss_weight=0.25, alpha=0.5, log_matrix=True, batch_matrix=True"
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            fa.FocalFrequencyLoss(alpha=bad)


def test_host_side_refusals(fa):
    """Each refusal comes before any device call: none of these needs a GPU, and there is no CPU fallback."""
    x = torch.rand(1, 1, 8, 8)
    f = fa.ops.focal_frequency_loss
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            f(x, x, alpha=bad)
    with pytest.raises(fa.KernelError, match="shape"):
        f(x[0], x[0])                                            # not 4-D
    with pytest.raises(fa.KernelError, match="shape"):
        f(x, torch.rand(1, 1, 8, 9))                             # unequal shapes
    with pytest.raises(fa.KernelError, match="shape"):
        f(x, None)
    with pytest.raises(fa.KernelError, match="fp32"):
        f(x.double(), x.double())
    with pytest.raises(fa.KernelError, match="fp32"):
        f(x, x.half())
    with pytest.raises(fa.KernelError, match="GPU"):
        f(x, x)                                                  # CPU tensors
    with pytest.raises(fa.KernelError, match="GPU"):
        fa.FocalFrequencyLoss()(x, x)


def test_new_symbols_in_header_and_library(fa, lib):
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in fa._lib.declared_symbols(), s
        assert hasattr(lib, s), s
    assert lib.faoctasr_version() >= 430


def test_workspace_query(lib):
    n = lib.faoctasr_ffl_workspace_floats(8, 1, 256, 256)
    assert n >= 4 * 8 * 256 * 256                     # at least the row-pass buffer of both images
    # ... and no spectrum planes of its own: those belong to the caller, and only when a backward will follow
    assert n < lib.faoctasr_phase_loss_workspace_floats(8, 1, 256, 256) - 3 * 8 * 256 * 256
    assert lib.faoctasr_ffl_workspace_floats(1, 1, 2, 2) > 0
    assert lib.faoctasr_ffl_workspace_floats(3, 2, 63, 50) > lib.faoctasr_ffl_workspace_floats(3, 1, 63, 50)
    assert lib.faoctasr_ffl_workspace_floats(1, 1, 1, 64) < 0 and b"H" in lib.faoctasr_last_error()


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    fwd = lambda *a: lib.faoctasr_ffl_fwd(*a)
    bwd = lambda *a: lib.faoctasr_ffl_bwd(*a)
    for H, W in ((1, 64), (64, 1)):
        assert fwd(p, p, p, p, 1.0, 0, 0, p, p, p, 1, 1, H, W, None) == -1 and b"ffl_fwd" in lib.faoctasr_last_error()
        assert bwd(p, p, p, p, 1.0, 0, p, p, p, 1, 1, H, W, None) == -1 and b"ffl_bwd" in lib.faoctasr_last_error()
    for alpha in (-1.0, float("nan"), float("inf")):
        assert fwd(p, p, p, p, alpha, 0, 0, p, p, p, 1, 1, 64, 64, None) == -1 and b"alpha" in lib.faoctasr_last_error()
        assert bwd(p, p, p, p, alpha, 0, p, p, p, 1, 1, 64, 64, None) == -1 and b"alpha" in lib.faoctasr_last_error()
    for k in (0, 1, 2, 3, 7, 9):                                  # x, y, tabH, tabW, loss, workspace; `planes` (8) may be null
        a = [p, p, p, p, 1.0, 0, 0, p, p, p, 1, 1, 64, 64, None]
        a[k] = None
        assert fwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    for k in (0, 1, 2, 3, 8):                                     # g, planes, tabH, tabW, workspace; dx (6), dy (7) may be null
        a = [p, p, p, p, 1.0, 0, p, p, p, 1, 1, 64, 64, None]
        a[k] = None
        assert bwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    assert fwd(p, p, p, p, 1.0, 0, 0, p, p, p + 4, 1, 1, 64, 64, None) == -1 and b"aligned" in lib.faoctasr_last_error()
    assert bwd(p, p, p, p, 1.0, 0, p, p, p + 4, 1, 1, 64, 64, None) == -1 and b"aligned" in lib.faoctasr_last_error()
    # the size limits of the phase loss
    assert fwd(p, p, p, p, 1.0, 0, 0, p, p, p, 1, 1, 8193, 64, None) == -2 and b"8192" in lib.faoctasr_last_error()
    assert fwd(p, p, p, p, 1.0, 0, 0, p, p, p, 65536, 1, 2, 2, None) == -2 and b"65535" in lib.faoctasr_last_error()
    # neither gradient wanted: nothing to do, and nothing is launched
    assert bwd(p, p, p, p, 1.0, 0, None, None, p, 1, 1, 64, 64, None) == 0


def test_train_step_arguments(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor).  Weight 0 builds no module;
    a bad ``ffl_alpha`` or ``ffl_weight`` raises before a device is touched."""
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("ffl_weight", "ffl_alpha", "ffl_log_matrix", "ffl_batch_matrix")] == [0.0, 1.0, False, False]
    built = []
    real = fa.train.FocalFrequencyLoss

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "FocalFrequencyLoss", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.ffl_weight == 0.0 and ts.ffl is None and not built
    ts = fa.TrainStep(*nets, device="cpu", ffl_weight=0.5, ffl_alpha=0.5, ffl_log_matrix=True, ffl_batch_matrix=True)
    assert built == [dict(alpha=0.5, log_matrix=True, batch_matrix=True)]
    assert ts.ffl_weight == 0.5 and (ts.ffl.loss_weight, ts.ffl.alpha, ts.ffl.log_matrix, ts.ffl.batch_matrix) == (1.0, 0.5, True, True)
    assert ts.msssim is None and ts.cwssim is None and ts.cwt_loss is None
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            fa.TrainStep(*nets, device="cpu", ffl_weight=0.5, ffl_alpha=bad)
    for bad in (-0.5, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="ffl_weight"):
            fa.TrainStep(*nets, device="cpu", ffl_weight=bad)


def test_train_step_terms_call_the_module(fa):
    """``_extension_terms`` names ``loss_ffl``; with the module replaced by a stub no kernel runs (``generator_loss``:
    tests/test_train_terms_cpu.py)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu", ffl_weight=0.5)
    ts.ffl = lambda rec, real: (rec * real).mean()
    rec, real = torch.full((1, 1, 4, 4), 0.5), torch.full((1, 1, 4, 4), 0.5)
    t = ts._extension_terms(rec, real)
    assert list(t) == ["loss_ffl"] and float(t["loss_ffl"]) == 0.5 * 0.25
    assert fa.TrainStep(*nets, device="cpu")._extension_terms(rec, real) == {}
    assert "if self.phase_weight or self.ffl_weight:" in inspect.getsource(fa.TrainStep.step)
