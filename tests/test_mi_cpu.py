"""Host-side checks of the differentiable mutual information: the float64 / float32 torch restatement of the definition that the
GPU tests lean on, pinned to the fixture (tests/golden/golden_mi.npz, written by tools/gen_golden_mi.py); the closed-form
gradient the backward kernel implements, written out here and held to autograd; the public names, the host-side refusals,
the C ABI's argument checks and the ``TrainStep(mi_weight=...)`` plumbing."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_mi.npz")
NEW_SYMBOLS = ("faoctasr_mi_workspace_floats", "faoctasr_mi_fwd", "faoctasr_mi_bwd")
SETTINGS = ((32, 1.0), (64, 0.5), (24, 1.0), (40, 0.75))
SHAPES = ((2, 1, 7, 9), (1, 1, 33, 31), (3, 1, 63, 50), (2, 2, 96, 64))
GUARD = 0.03                     # nats: the smallest float64 MI of a plane any comparison may rest on


def restatement(x, y, bins=32, sigma_ratio=1.0, normalized=False, dtype=torch.float64, value_range=(-1.0, 1.0), eps=1e-6):
    """The literal definition with softmax, bmm and autograd on the CPU in ``dtype``: (score, dS/dx, dS/dy, per-plane MI)."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    y = y.detach().cpu().to(dtype).requires_grad_(True)
    N, C, H, W = x.shape
    lo, hi = value_range
    d = (hi - lo) / bins
    c = lo + (torch.arange(bins, dtype=dtype) + 0.5) * d
    sigma = sigma_ratio * d

    def weights(v):
        return torch.softmax(-(v.reshape(N * C, H * W, 1) - c) ** 2 / (2 * sigma ** 2), dim=-1)

    P = torch.bmm(weights(x).transpose(1, 2), weights(y)) / (H * W)
    pa, pb = P.sum(2), P.sum(1)
    Ha = -(pa * torch.log(pa + eps)).sum(1)
    Hb = -(pb * torch.log(pb + eps)).sum(1)
    Hab = -(P * torch.log(P + eps)).sum((1, 2))
    mi = Ha + Hb - Hab
    score = ((Ha + Hb) / Hab if normalized else mi).mean()
    gx, gy = torch.autograd.grad(score, (x, y))
    return score.detach().double(), gx.double(), gy.double(), mi.detach().double()


def closed_form(x, y, bins, sigma_ratio, normalized, value_range=(-1.0, 1.0), eps=1e-6):
    """What the kernels compute, in float64 and without autograd: the score and both gradients from x, y and one K x K table G
    per plane.  A = log(P + eps) + P / (P + eps), u = -(log(pa + eps) + pa / (pa + eps)), v likewise from pb; MI: G = A + u_i +
    v_j; NMI: G = (u_i + v_j) / Hab + (Ha + Hb) / Hab^2 A; dS/dx_p = 1 / (planes n_pix sigma^2) sum_k Wa[p,k] (c_k - xbar_p)
    sum_j G_kj Wb[p,j] with xbar_p = sum_k Wa[p,k] c_k, and dS/dy_p the same with G^T and the roles swapped."""
    x, y = x.double(), y.double()
    N, C, H, W = x.shape
    planes, n_pix = N * C, H * W
    lo, hi = value_range
    d = (hi - lo) / bins
    c = lo + (torch.arange(bins, dtype=torch.float64) + 0.5) * d
    sigma = sigma_ratio * d

    def weights(v):
        z = -(v.reshape(planes, n_pix, 1) - c) ** 2 / (2 * sigma ** 2)
        e = torch.exp(z - z.amax(-1, keepdim=True))
        return e / e.sum(-1, keepdim=True)

    Wa, Wb = weights(x), weights(y)
    P = torch.einsum("qpi,qpj->qij", Wa, Wb) / n_pix
    pa, pb = P.sum(2), P.sum(1)
    Ha, Hb, Hab = -(pa * torch.log(pa + eps)).sum(1), -(pb * torch.log(pb + eps)).sum(1), -(P * torch.log(P + eps)).sum((1, 2))
    A = torch.log(P + eps) + P / (P + eps)
    u = -(torch.log(pa + eps) + pa / (pa + eps))
    v = -(torch.log(pb + eps) + pb / (pb + eps))
    uv = u[:, :, None] + v[:, None, :]
    if normalized:
        score = (Ha + Hb) / Hab
        G = uv / Hab[:, None, None] + ((Ha + Hb) / Hab ** 2)[:, None, None] * A
    else:
        score = Ha + Hb - Hab
        G = A + uv
    f = 1.0 / (planes * n_pix * sigma ** 2)
    xbar, ybar = (Wa * c).sum(-1, keepdim=True), (Wb * c).sum(-1, keepdim=True)
    gx = f * (Wa * (c - xbar) * torch.einsum("qkj,qpj->qpk", G, Wb)).sum(-1)
    gy = f * (Wb * (c - ybar) * torch.einsum("qkj,qpk->qpj", G, Wa)).sum(-1)
    return score.mean(), gx.reshape(x.shape), gy.reshape(x.shape)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tag_of(shape, bins, sigma_ratio, normalized):
    return "%s_k%d_s%g_n%d" % ("x".join(str(s) for s in shape), bins, sigma_ratio, int(normalized))


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


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_restatement_reproduces_the_fixture(gold):
    g = gold
    assert os.path.getsize(GOLD) < (1 << 20)
    assert [tuple(s) for s in g["shapes"]] == list(SHAPES)
    assert [(int(k), float(s)) for k, s in g["settings"]] == list(SETTINGS)
    for shape in SHAPES:
        x, y = case_inputs(g, shape)
        assert tuple(x.shape) == shape and x.dtype == torch.float32
        assert float(x.min()) >= -1 and float(x.max()) <= 1 and float(y.min()) >= -1 and float(y.max()) <= 1
        for bins, sr in SETTINGS:
            for normalized in (False, True):
                t = tag_of(shape, bins, sr, normalized)
                s, gx, gy, mi = restatement(x, y, bins, sr, normalized)
                assert abs(float(s) - float(g["score64_" + t])) <= 1e-12 * abs(float(s)), t
                assert abs(float(mi.min()) - float(g["mi_min_" + t])) <= 1e-11, t
                assert abs(float(gx.norm()) - float(g["gxnorm64_" + t])) <= 1e-11 * float(gx.norm()), t
                assert abs(float(gy.norm()) - float(g["gynorm64_" + t])) <= 1e-11 * float(gy.norm()), t
                if "gx64_" + t in g:
                    assert rel_l2(gx, torch.from_numpy(g["gx64_" + t])) <= 1e-11, t
                    assert rel_l2(gy, torch.from_numpy(g["gy64_" + t])) <= 1e-11, t
                # the fp32 run of the same definition is the GPU tests' yardstick.  Its last bits depend on the host's matmul code
                # path, so this host's run is held to the class of an fp32 error, not to the file's bits
                s32, gx32, gy32, _ = restatement(x, y, bins, sr, normalized, dtype=torch.float32)
                assert abs(float(s32) - float(s)) <= 1e-5 * abs(float(s)), t
                assert rel_l2(gx32, gx) < 5e-6 and rel_l2(gy32, gy) < 5e-6, t


def test_fixture_guard_and_reference_errors_are_sane(gold):
    """MI is a difference of entropies: every plane the comparisons rest on carries at least GUARD nats, and the fp32 reference's
    own errors -- the yardstick of the GPU bars -- are of the size of an fp32 error, neither accidentally tiny nor large.  This
    fixture's gradient e_ref span 3.0e-7 to 1.4e-6 and its largest relative score error is 3.1e-6 (tools/gen_golden_mi.py prints
    them); another draw of the same recipe gave 3.4e-7 to 2.6e-6, so the class is bounded here, not the draw."""
    g = gold
    r, lo_e, hi_e = 0.0, 1.0, 0.0
    for shape in SHAPES:
        for bins, sr in SETTINGS:
            for normalized in (False, True):
                t = tag_of(shape, bins, sr, normalized)
                assert float(g["mi_min_" + t]) >= GUARD, t
                assert float(g["mi_min_" + t]) <= math.log(bins)
                for k in ("gxerr32_", "gyerr32_"):
                    lo_e, hi_e = min(lo_e, float(g[k + t])), max(hi_e, float(g[k + t]))
                r = max(r, abs(float(g["score32_" + t]) - float(g["score64_" + t])) / abs(float(g["score64_" + t])))
                assert float(g["gxnorm64_" + t]) > 0 and float(g["gynorm64_" + t]) > 0
    assert 1e-7 < lo_e and hi_e < 5e-6, (lo_e, hi_e)
    assert 1e-7 < r < 1e-5, r


def test_closed_form_gradient_matches_autograd(gold):
    """The formula the backward kernel implements, against autograd of the literal definition in float64."""
    for shape in SHAPES[:3]:
        x, y = case_inputs(gold, shape)
        for bins, sr in SETTINGS:
            for normalized in (False, True):
                want, wx, wy, _ = restatement(x, y, bins, sr, normalized)
                got, gx, gy = closed_form(x, y, bins, sr, normalized)
                assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (shape, bins, normalized)
                assert rel_l2(gx, wx) <= 1e-11 and rel_l2(gy, wy) <= 1e-11, (shape, bins, normalized, rel_l2(gx, wx), rel_l2(gy, wy))


def test_symmetry_and_invariance_of_the_definition(gold):
    """S(x, y) = S(y, x) with swapped gradients; an invertible map of one image's intensities (here the flip v -> -v, which maps
    the bin centres onto themselves) leaves the score unchanged -- what a pixelwise distance cannot offer."""
    x, y = case_inputs(gold, (3, 1, 63, 50))
    s, gx, gy, _ = restatement(x, y)
    t, hx, hy, _ = restatement(y, x)
    assert abs(float(s) - float(t)) <= 1e-13 and rel_l2(hx, gy) <= 1e-12 and rel_l2(hy, gx) <= 1e-12
    f, _, _, _ = restatement(x, -y)
    assert abs(float(f) - float(s)) <= 1e-12
    assert float((x - y).abs().mean()) > 0.05 and float((x + y).abs().mean()) > 0.05


def test_public_names_exist(fa):
    assert callable(fa.ops.mutual_information)
    assert "MutualInformationLoss" in fa.__all__ and fa.model.MutualInformationLoss is fa.MutualInformationLoss
    sig = inspect.signature(fa.ops.mutual_information)
    assert list(sig.parameters) == ["x", "y", "bins", "value_range", "sigma_ratio", "eps", "normalized", "per_image"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [32, (-1.0, 1.0), 1.0, 1e-6, False, False]


def test_module_signature_defaults_and_repr(fa):
    sig = inspect.signature(fa.MutualInformationLoss.__init__)
    assert list(sig.parameters) == ["self", "bins", "value_range", "sigma_ratio", "eps", "normalized", "per_image"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [32, (-1.0, 1.0), 1.0, 1e-6, False, False]
    assert list(inspect.signature(fa.MutualInformationLoss.forward).parameters) == ["self", "x", "y"]
    m = fa.MutualInformationLoss()
    assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(m.buffers())
    assert repr(m) == "MutualInformationLoss(bins=32, value_range=(-1, 1), sigma_ratio=1, eps=1e-06, normalized=False, per_image=False)"
    assert m.upper == math.log(32)
    m = fa.MutualInformationLoss(bins=40, value_range=(0, 2.5), sigma_ratio=0.75, eps=1e-5, normalized=True, per_image=True)
    assert m.extra_repr() == "bins=40, value_range=(0, 2.5), sigma_ratio=0.75, eps=1e-05, normalized=True, per_image=True"
    assert m.upper == 2.0
    for bad in (1, 65, 0, -3, 32.0, True, "32", None):
        with pytest.raises(ValueError, match="bins"):
            fa.MutualInformationLoss(bins=bad)
    for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0), 1.0, (0, 1, 2), None):
        with pytest.raises(ValueError, match="value_range"):
            fa.MutualInformationLoss(value_range=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_ratio"):
            fa.MutualInformationLoss(sigma_ratio=bad)
        with pytest.raises(ValueError, match="eps"):
            fa.MutualInformationLoss(eps=bad)


def test_host_side_refusals(fa):
    """Each refusal comes before any device call: none of these needs a GPU, and there is no CPU fallback."""
    x = torch.rand(1, 1, 8, 8)
    f = fa.ops.mutual_information
    for bad in (1, 65, 16.0):
        with pytest.raises(ValueError, match="bins"):
            f(x, x, bins=bad)
    with pytest.raises(ValueError, match="value_range"):
        f(x, x, value_range=(1.0, 0.0))
    with pytest.raises(ValueError, match="sigma_ratio"):
        f(x, x, sigma_ratio=0.0)
    with pytest.raises(ValueError, match="eps"):
        f(x, x, eps=0.0)
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
        fa.MutualInformationLoss()(x, x)


def test_new_symbols_in_header_and_library(fa, lib):
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in fa._lib.declared_symbols(), s
        assert hasattr(lib, s), s
    assert lib.faoctasr_version() >= 440


def test_workspace_query(lib):
    """One K x K partial per 2048 pixels and plane plus the planes' scores -- nothing of size pixels x bins."""
    ws = lib.faoctasr_mi_workspace_floats
    assert ws(8, 1, 256, 256, 32) == 2 * 8 + 8 * 32 * 32 * 32
    assert ws(8, 1, 256, 256, 64) == 2 * 8 + 8 * 32 * 64 * 64
    assert ws(8, 1, 256, 256, 64) < 8 * 256 * 256 * 64 // 16
    assert ws(2, 1, 7, 9, 24) == 2 * 2 + 2 * 24 * 24
    assert ws(3, 2, 63, 50, 40) == 2 * ws(3, 1, 63, 50, 40)
    assert ws(1, 1, 1, 2049, 2) == 2 + 2 * 4
    for bad in ((0, 1, 8, 8, 32), (1, 0, 8, 8, 32), (1, 1, 0, 8, 32), (1, 1, 8, 8, 1), (1, 1, 8, 8, 65), (65536, 1, 8, 8, 32)):
        assert ws(*bad) < 0 and b"mi_workspace_floats" in lib.faoctasr_last_error(), bad


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    fwd = lambda *a: lib.faoctasr_mi_fwd(*a)
    bwd = lambda *a: lib.faoctasr_mi_bwd(*a)
    good_f = [p, p, p, p, p, 1, 1, 8, 8, 32, -1.0, 1.0, 1.0, 1e-6, 0, 0, None]
    good_b = [p, p, p, p, p, p, 1, 1, 8, 8, 32, -1.0, 1.0, 1.0, 0, None]
    for k in (0, 1, 2, 4):                                        # x, y, out, workspace; `table` (3) may be null
        a = list(good_f)
        a[k] = None
        assert fwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    for k in (0, 1, 2, 3):                                        # g, x, y, table; dx (4), dy (5) may be null
        a = list(good_b)
        a[k] = None
        assert bwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    a = list(good_f)
    a[4] = p + 4
    assert fwd(*a) == -1 and b"aligned" in lib.faoctasr_last_error()
    for idx_f, idx_b, vals, word in ((9, 10, (1, 65, 0, -1), b"bins"), (12, 13, (0.0, -1.0, float("nan"), float("inf")), b"sigma_ratio"),
                                     (11, 12, (-1.0, -2.0, float("nan"), float("inf")), b"range"), (7, 8, (0, -1), b"shape"),
                                     (5, 6, (0, 65536), b"shape")):
        for v in vals:
            a, b = list(good_f), list(good_b)
            a[idx_f], b[idx_b] = v, v
            assert fwd(*a) == -1 and b"mi_fwd" in lib.faoctasr_last_error() and word in lib.faoctasr_last_error(), (word, v)
            assert bwd(*b) == -1 and b"mi_bwd" in lib.faoctasr_last_error() and word in lib.faoctasr_last_error(), (word, v)
    for v in (0.0, -1e-6, float("nan"), float("inf")):
        a = list(good_f)
        a[13] = v
        assert fwd(*a) == -1 and b"eps" in lib.faoctasr_last_error(), v
    # neither gradient wanted: nothing to do, and nothing is launched
    b = list(good_b)
    b[4] = b[5] = None
    assert bwd(*b) == 0


def test_train_step_arguments(fa, monkeypatch):
    """Argument plumbing of ``TrainStep.__init__`` (on the CPU: no kernel runs in a constructor).  Weight 0 builds no module;
    a bad ``mi_bins``, ``mi_sigma_ratio`` or ``mi_weight`` raises before a device is touched."""
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("mi_weight", "mi_bins", "mi_sigma_ratio", "mi_normalized")] == [0.0, 32, 1.0, False]
    built = []
    real = fa.train.MutualInformationLoss

    def record(**kw):
        built.append(kw)
        return real(**kw)
    monkeypatch.setattr(fa.train, "MutualInformationLoss", record)
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert ts.mi_weight == 0.0 and ts.mi is None and not built
    ts = fa.TrainStep(*nets, device="cpu", mi_weight=0.5, mi_bins=40, mi_sigma_ratio=0.75, mi_normalized=True)
    assert built == [dict(bins=40, sigma_ratio=0.75, normalized=True)]
    assert ts.mi_weight == 0.5 and (ts.mi.bins, ts.mi.sigma_ratio, ts.mi.normalized, ts.mi.per_image, ts.mi.upper) == (40, 0.75, True, False, 2.0)
    assert ts.ffl is None and ts.msssim is None and ts.cwssim is None
    for bad in (1, 65, 32.5):
        with pytest.raises(ValueError, match="bins"):
            fa.TrainStep(*nets, device="cpu", mi_weight=0.5, mi_bins=bad)
    for bad in (0.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_ratio"):
            fa.TrainStep(*nets, device="cpu", mi_weight=0.5, mi_sigma_ratio=bad)
    for bad in (-0.5, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="mi_weight"):
            fa.TrainStep(*nets, device="cpu", mi_weight=bad)


def test_train_step_terms_call_the_module(fa):
    """At weight 0 ``_extension_terms`` does not know the term (where the term lives, with which operands and as ``upper - score``:
    tests/test_train_terms_cpu.py; the GPU step test covers the placement by value)."""
    nets = (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))
    ts = fa.TrainStep(*nets, device="cpu")
    assert "loss_mi" not in ts._extension_terms(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
