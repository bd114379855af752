"""Host-side checks of the spectral-profile loss (after Durall, Keuper, Keuper, CVPR 2020): ``radial_bins`` against Python integers;
the float64 ``torch.fft`` + ``index_add_`` restatement the GPU tests lean on, pinned to the fixture (tests/golden/golden_sprof.npz,
written by tools/gen_golden_sprof.py from explicit DFT matrices and a loop over the rings); the half-spectrum identity and the
gather list the kernels rest on; the sixteenth record of ``train.OPT_IN_TERMS`` by behaviour (stubs as in
tests/test_train_terms_cpu.py, restated here); the public names, the host-side refusals and the C ABI's argument checks."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_sprof.npz")
NEW_SYMBOLS = ("faoctasr_sprof_workspace_floats", "faoctasr_sprof_profile_fwd", "faoctasr_sprof_loss_fwd", "faoctasr_sprof_bwd")
SHAPES = ((1, 1, 2, 3), (2, 1, 8, 8), (1, 2, 37, 53), (2, 1, 64, 64), (1, 1, 65, 63), (2, 1, 72, 136))
SETTINGS = ((False, 0), (False, 1), (True, 0), (True, 1))               # (batch_profile, k_min)
GRADIENTS = {(2, 1, 8, 8): SETTINGS, (1, 2, 37, 53): ((False, 1), (True, 1))}
SMALL = ((2, 2), (2, 64), (3, 5), (4, 4), (5, 7), (6, 6), (37, 53), (64, 64), (65, 63), (72, 136))
LARGE = ((192, 192), (256, 256), (512, 512), (1024, 1024), (1024, 2), (1023, 1024), (100, 1000))
EPS = 1e-8


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


def brute_force(H, W):
    """bin (rows of Python ints) and counts straight from the definition: the largest k with k^2 H^2 W^2 <= M^2 (u_c^2 W^2 + v_c^2 H^2)."""
    M, den = min(H, W), H * H * W * W
    rows, cnt = [], {}
    for u in range(H):
        uc = (u + H // 2) % H - H // 2
        row = []
        for v in range(W):
            vc = (v + W // 2) % W - W // 2
            num, k = M * M * (uc * uc * W * W + vc * vc * H * H), 0
            while (k + 1) * (k + 1) * den <= num:
                k += 1
            row.append(k)
            cnt[k] = cnt.get(k, 0) + 1
        rows.append(row)
    return rows, cnt


def k_formula(H, W):
    M = min(H, W)
    K = 1 + int(math.floor(M * math.sqrt((H // 2) ** 2 / H ** 2 + (W // 2) ** 2 / W ** 2)))
    # the floating formula of the issue, settled in integers where it sits on an integer
    num, den = M * M * ((H // 2) ** 2 * W * W + (W // 2) ** 2 * H * H), H * H * W * W
    exact = 1 + math.isqrt(num // den)
    assert abs(K - exact) <= 1
    return exact


def point_symmetric(b):
    return torch.equal(b, b.flip(0, 1).roll((1, 1), (0, 1)))


@pytest.mark.parametrize("H,W", SMALL)
def test_radial_bins_against_python_integers(fa, H, W):
    b, c = fa.radial_bins(H, W)
    assert b.dtype == torch.int64 and c.dtype == torch.int64 and tuple(b.shape) == (H, W) and not b.is_cuda
    rows, cnt = brute_force(H, W)
    assert b.tolist() == rows
    K = k_formula(H, W)
    assert c.numel() == K and c.tolist() == [cnt[k] for k in range(K)]
    assert int(c.sum()) == H * W and int(c.min()) >= 1
    assert point_symmetric(b)
    if H == W:
        uc = (torch.arange(H) + H // 2) % H - H // 2
        assert b.tolist() == [[math.isqrt(int(u) ** 2 + int(v) ** 2) for v in uc] for u in uc]
        assert int(c[0]) == 1                                      # a square plane: ring 0 is the DC bin alone
    assert int(b[0, 0]) == 0


@pytest.mark.parametrize("H,W", LARGE)
def test_radial_bins_at_the_large_shapes(fa, H, W):
    """The defining inequality in int64 at every position, the K formula, no empty ring, the point symmetry."""
    b, c = fa.radial_bins(H, W)
    M, den = min(H, W), H * H * W * W
    uc = ((torch.arange(H) + H // 2) % H - H // 2)[:, None]
    vc = ((torch.arange(W) + W // 2) % W - W // 2)[None, :]
    num = M * M * (uc * uc * (W * W) + vc * vc * (H * H))
    assert bool(((b * b * den <= num) & ((b + 1) * (b + 1) * den > num)).all())
    assert c.numel() == k_formula(H, W) == int(b.max()) + 1
    assert torch.equal(c, torch.bincount(b.flatten())) and int(c.min()) >= 1 and int(c.sum()) == H * W
    assert point_symmetric(b)
    assert (H, W) != (256, 256) or c.numel() == 182


def test_radial_bins_known_values_and_refusals(fa):
    assert fa.radial_bins(256, 256)[1].numel() == 182 and fa.radial_bins(37, 53)[1].numel() == 26
    assert fa.radial_bins(2, 3)[1].numel() == 2
    assert fa.radial_bins is fa.ops.radial_bins and "radial_bins" in fa.__all__
    for bad in ((1, 8), (8, 1), (1025, 8), (8, 1025), (8.0, 8), (True, 8), ("8", 8)):
        with pytest.raises(ValueError, match="radial_bins"):
            fa.radial_bins(*bad)


def restatement(fa, x, y, batch, k_min, eps=EPS, dtype=torch.float64):
    """The definition with ``torch.fft.fft2`` and ``index_add_`` on the CPU in ``dtype``: (loss, per-image or None, dL/dx, dL/dy, A_x, A_y)."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(True)
    N, C, H, W = x.shape
    bins, cnt = fa.radial_bins(H, W)

    def profile(t):
        Fq = torch.fft.fft2(t)
        q = ((Fq.real ** 2 + Fq.imag ** 2) / (H * W)).reshape(N, C, H * W)
        return torch.zeros(N, C, cnt.numel(), dtype=dtype).index_add_(2, bins.flatten(), q) / cnt.to(dtype)
    Ax, Ay = profile(x), profile(y)
    ax, ay = torch.log(Ax + eps), torch.log(Ay + eps)
    if batch:
        loss, per = ((ax.mean((0, 1)) - ay.mean((0, 1)))[k_min:] ** 2).mean(), None
    else:
        per = ((ax - ay)[..., k_min:] ** 2).mean((1, 2))
        loss = per.mean()
    gx, gy = torch.autograd.grad(loss, (x, y))
    return loss.detach().double(), None if per is None else per.detach().double(), gx.double(), gy.double(), Ax.detach().double(), Ay.detach().double()


def half_spectrum(fa, x, y, batch, k_min, eps=EPS):
    """What the kernels compute, in float64: the half tables W x 2Wh, the column weights m_v, the gather along the CSR list, the
    coefficient table, and the backward through the transposed half tables.  (loss, dL/dx, dL/dy, A_x, A_y)."""
    x, y = x.double(), y.double()
    N, C, H, W = x.shape
    K, Wh, off, idx, cnt, binmap = fa.ops.sprof_host_geometry(H, W)
    tab = lambda n: (torch.cos(2 * math.pi * ((torch.arange(n)[:, None] * torch.arange(n)[None, :]) % n).double() / n),
                     torch.sin(2 * math.pi * ((torch.arange(n)[:, None] * torch.arange(n)[None, :]) % n).double() / n))
    (CH, SH), (CW, SW) = tab(H), tab(W)
    CWh, SWh = CW[:, :Wh], SW[:, :Wh]
    m = torch.full((Wh,), 2.0, dtype=torch.float64)
    m[0] = 1
    if W % 2 == 0:
        m[W // 2] = 1
    cntd = cnt.double()

    def forward(t):
        P, Q = t @ CWh, t @ SWh
        Re, J = CH @ P - SH @ Q, SH @ P + CH @ Q
        pw = (m * (Re * Re + J * J) / (H * W)).reshape(N, C, H * Wh)
        A = torch.stack([pw[..., idx[off[k]:off[k + 1]].long()].sum(-1) for k in range(K)], -1) / cntd
        return Re, J, A
    Rx, Jx, Ax = forward(x)
    Ry, Jy, Ay = forward(y)
    d = torch.log(Ax + eps) - torch.log(Ay + eps)
    keep = (torch.arange(K) >= k_min).double()
    if batch:
        dm = d.mean((0, 1))
        loss = (dm * dm * keep).sum() / (K - k_min)
        da = (2 * dm * keep / ((K - k_min) * N * C)).expand(N, C, K)
    else:
        loss = (d * d * keep).sum() / (N * C * (K - k_min))
        da = 2 * d * keep / (N * C * (K - k_min))

    def backward(Re, J, coef):
        w = (2.0 / (H * W)) * m * coef[..., binmap.long()]                      # (N, C, H, Wh)
        dRe, dJ = w * Re, w * J
        T1, T2 = CH @ dRe + SH @ dJ, CH @ dJ - SH @ dRe
        return T1 @ CWh.t() + T2 @ SWh.t()
    return loss, backward(Rx, Jx, da / (Ax + eps) / cntd), backward(Ry, Jy, -da / (Ay + eps) / cntd), Ax, Ay


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tag_of(shape, setting):
    return "%s_b%d_k%d" % ("x".join(str(s) for s in shape), setting[0], setting[1])


def case_inputs(g, shape):
    case = "x".join(str(s) for s in shape)
    return torch.from_numpy(g["x_" + case]), torch.from_numpy(g["y_" + case])


def test_restatement_reproduces_the_fixture(fa, gold):
    g = gold
    assert os.path.getsize(GOLD) < (1 << 20)
    assert [tuple(s) for s in g["shapes"]] == list(SHAPES)
    assert [(bool(b), int(k)) for b, k in g["settings"]] == list(SETTINGS) and float(g["eps"]) == EPS
    for shape in SHAPES:
        x, y = case_inputs(g, shape)
        case = "x".join(str(s) for s in shape)
        assert tuple(x.shape) == shape and x.dtype == torch.float32
        assert g["cnt_" + case].tolist() == fa.radial_bins(*shape[-2:])[1].tolist()
        for st in SETTINGS:
            t = tag_of(shape, st)
            loss, per, gx, gy, Ax, Ay = restatement(fa, x, y, *st)
            assert abs(float(loss) - float(g["loss64_" + t])) <= 1e-12 * abs(float(g["loss64_" + t])), t
            assert rel_l2(Ax, torch.from_numpy(g["Ax_" + case])) <= 1e-12 and rel_l2(Ay, torch.from_numpy(g["Ay_" + case])) <= 1e-12, t
            assert (per is None) == st[0] and (per is None or rel_l2(per, torch.from_numpy(g["per64_" + t])) <= 1e-12), t
            assert ("gx64_" + t in g) == (st in GRADIENTS.get(shape, ())), t
            if "gx64_" + t in g:
                assert rel_l2(gx, torch.from_numpy(g["gx64_" + t])) <= 1e-12 and rel_l2(gy, torch.from_numpy(g["gy64_" + t])) <= 1e-12, t
            # the fp32 run of the same definition is the GPU tests' yardstick.  Its last bits depend on the host's FFT code path, so
            # the file's figures are held to the class of an fp32 error, and so is this host's run -- not to each other's bits
            l32, _, gx32, gy32, A32, _ = restatement(fa, x, y, *st, dtype=torch.float32)
            assert abs(float(g["loss32_" + t]) - float(loss)) <= 1e-6 * abs(float(loss)), t
            assert 1e-8 < float(g["gxerr32_" + t]) < 3e-6 and 1e-8 < float(g["gyerr32_" + t]) < 3e-6, t
            assert abs(float(l32) - float(loss)) <= 1e-6 * abs(float(loss)) and rel_l2(gx32, gx) < 3e-6 and rel_l2(gy32, gy) < 3e-6, t
        assert 1e-9 < float(g["Axerr32_" + case]) < 1e-6 and 1e-9 < float(g["Ayerr32_" + case]) < 1e-6


def test_fixture_inputs_follow_the_recipe(gold):
    """seed 0, float64: x = 2 smooth(randn, 2) + 0.25 randn, y0 = x + 0.3 randn, y = 0.7 smooth(y0, 1) + 0.3 y0, rounded to fp32."""
    def smooth(t, r):
        return sum(torch.roll(t, (dy, dx), (-2, -1)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / (2 * r + 1) ** 2
    for shape in SHAPES:
        g = torch.Generator().manual_seed(0)
        rn = lambda: torch.randn(*shape, generator=g, dtype=torch.float64)
        x = 2 * smooth(rn(), 2) + 0.25 * rn()
        y0 = x + 0.3 * rn()
        y = 0.7 * smooth(y0, 1) + 0.3 * y0
        fx, fy = case_inputs(gold, shape)
        assert float((fx.double() - x).abs().max()) <= 1e-6 and float((fy.double() - y).abs().max()) <= 1e-6


def test_conditioning_guard_parseval_and_identical_inputs(fa, gold):
    """min over k >= 1 of A[k] / mean(x^2) >= 2^-8 for both images of every case (1 / (A + eps) amplifies rounding);
    sum_k cnt_k A[k] = sum x^2; L(x, x) = 0 with zero gradients."""
    for shape in SHAPES:
        x, y = case_inputs(gold, shape)
        cnt = fa.radial_bins(*shape[-2:])[1].double()
        _, _, _, _, Ax, Ay = restatement(fa, x, y, False, 1)
        for img, A in ((x, Ax), (y, Ay)):
            e = (img.double() ** 2).sum((-2, -1))
            assert float(((A * cnt).sum(-1) - e).abs().max()) <= 1e-12 * float(e.max())
            assert float((A[..., 1:] / (img.double() ** 2).mean((-2, -1))[..., None]).min()) >= 2.0 ** -8
        for st in SETTINGS:
            same, _, gx, gy, _, _ = restatement(fa, x, x.clone(), *st)
            assert float(same) == 0 and not gx.any() and not gy.any()


def test_half_spectrum_form_and_gather_list(fa, gold):
    """The identities the kernels rest on, against autograd of the full-plane definition in float64: the half tables with the
    column weights give the same profile, the CSR gather is the ring sum, and the adjoint through the transposed half tables is the
    gradient.  The list itself: sorted by (bin, position), every half-plane position once, the weighted counts are the full counts."""
    for shape in SHAPES:
        x, y = case_inputs(gold, shape)
        H, W = shape[-2:]
        K, Wh, off, idx, cnt, binmap = fa.ops.sprof_host_geometry(H, W)
        bins, cnt64 = fa.radial_bins(H, W)
        assert Wh == W // 2 + 1 and K == cnt64.numel() and cnt.dtype == torch.int32 and cnt.tolist() == cnt64.tolist()
        assert off.dtype == torch.int32 and idx.dtype == torch.int32 and binmap.dtype == torch.int16
        assert tuple(binmap.shape) == (H, Wh) and torch.equal(binmap.long(), bins[:, :Wh])
        assert int(off[0]) == 0 and int(off[-1]) == H * Wh and sorted(idx.tolist()) == list(range(H * Wh))
        flat = binmap.flatten().long()
        m = torch.full((Wh,), 2, dtype=torch.int64)
        m[0] = 1
        if W % 2 == 0:
            m[W // 2] = 1
        for k in range(K):
            seg = idx[off[k]:off[k + 1]].long()
            assert seg.numel() >= 1 and bool((flat[seg] == k).all()) and bool((seg[1:] > seg[:-1]).all())
            assert int(m[seg % Wh].sum()) == int(cnt[k])
        for st in SETTINGS:
            want, _, wx, wy, Ax, Ay = restatement(fa, x, y, *st)
            got, gx, gy, Bx, By = half_spectrum(fa, x, y, *st)
            assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (shape, st)
            assert rel_l2(Bx, Ax) <= 1e-12 and rel_l2(By, Ay) <= 1e-12
            assert rel_l2(gx, wx) <= 1e-11 and rel_l2(gy, wy) <= 1e-11, (shape, st)
    full = fa.ops.sprof_host_geometry(8, 6, full=True)
    assert full[1] == 6 and tuple(full[5].shape) == (8, 6) and int(full[2][-1]) == 48


def test_translation_invariance_and_pure_tone(fa):
    """Phase-blind: a circular shift leaves the profile alone; cos(2 pi (3 i/H + 5 j/W)) at 64 x 64 puts HW/2 into ring 5."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 1, 37, 53, generator=g)
    A = restatement(fa, x, x, False, 0)[4]
    B = restatement(fa, torch.roll(x, (3, 5), (-2, -1)), x, False, 0)[4]
    assert rel_l2(B, A) <= 1e-12
    H = W = 64
    i, j = torch.arange(H, dtype=torch.float64)[:, None], torch.arange(W, dtype=torch.float64)[None, :]
    tone = torch.cos(2 * math.pi * (3 * i / H + 5 * j / W))[None, None]
    A = restatement(fa, tone, tone, False, 0)[4][0, 0]
    cnt = fa.radial_bins(H, W)[1]
    assert math.isqrt(3 * 3 + 5 * 5) == 5
    assert abs(float(A[5]) - H * W / 2 / int(cnt[5])) <= 1e-10 and float(A.sum() - A[5]) <= 1e-20


def test_generator_script_is_independent_of_package_and_tests():
    with open(os.path.join(ROOT, "tools", "gen_golden_sprof.py")) as f:
        src = f.read()
    imports = re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, re.M)
    assert sorted(set(imports)) == ["math", "numpy", "os", "torch"]
    assert "faoctasr" not in src and "radial_bins" not in src and "torch.fft.fft2" in src and "CH @ x @ CW" in src


def test_public_names_and_signatures(fa):
    assert callable(fa.ops.spectral_profile) and callable(fa.ops.spectral_profile_loss)
    assert "SpectralProfileLoss" in fa.__all__ and fa.model.SpectralProfileLoss is fa.SpectralProfileLoss
    sig = inspect.signature(fa.ops.spectral_profile_loss)
    assert list(sig.parameters)[:6] == ["x", "y", "eps", "k_min", "batch_profile", "per_image"]
    assert [sig.parameters[k].default for k in ("eps", "k_min", "batch_profile", "per_image")] == [1e-8, 1, False, False]
    assert list(inspect.signature(fa.ops.spectral_profile).parameters)[:1] == ["x"]
    sig = inspect.signature(fa.SpectralProfileLoss.__init__)
    assert list(sig.parameters) == ["self", "eps", "k_min", "batch_profile"]
    assert [sig.parameters[k].default for k in ("eps", "k_min", "batch_profile")] == [1e-8, 1, False]
    assert list(inspect.signature(fa.SpectralProfileLoss.forward).parameters) == ["self", "x", "y"]
    assert list(inspect.signature(fa.SpectralProfileLoss.index).parameters) == ["self", "a", "b", "per_image"]
    m = fa.SpectralProfileLoss()
    assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(m.buffers())
    assert repr(m) == "SpectralProfileLoss(eps=1e-08, k_min=1, batch_profile=False)"
    assert fa.SpectralProfileLoss(eps=1e-6, k_min=0, batch_profile=True).extra_repr() == "eps=1e-06, k_min=0, batch_profile=True"


def test_host_side_refusals(fa):
    """Each refusal comes before any device call: none of these needs a GPU, and there is no CPU fallback."""
    x = torch.rand(1, 1, 8, 8)
    f = fa.ops.spectral_profile_loss
    for bad in (0.0, -1e-8, float("nan"), float("inf"), "1e-8", None, True):
        with pytest.raises(ValueError, match="eps"):
            f(x, x, eps=bad)
        with pytest.raises(ValueError, match="eps"):
            fa.SpectralProfileLoss(eps=bad)
    for bad in (-1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="k_min"):
            f(x, x, k_min=bad)
        with pytest.raises(ValueError, match="k_min"):
            fa.SpectralProfileLoss(k_min=bad)
    with pytest.raises(ValueError, match="per_image"):
        f(x, x, batch_profile=True, per_image=True)
    with pytest.raises(fa.KernelError, match=r"\(N,C,H,W\)"):
        f(x[0], x[0])
    with pytest.raises(fa.KernelError, match=r"\(N,C,H,W\)"):
        f(x, None)
    with pytest.raises(fa.KernelError, match="fp32"):
        f(x.double(), x.double())
    with pytest.raises(fa.KernelError, match="fp32"):
        f(x, x.half())
    with pytest.raises(fa.KernelError, match="GPU"):
        f(x, x)
    with pytest.raises(fa.KernelError, match="GPU"):
        fa.SpectralProfileLoss()(x, x)
    with pytest.raises(fa.KernelError, match="GPU"):
        fa.SpectralProfileLoss().index(x, x, True)
    with pytest.raises(fa.KernelError, match="GPU"):
        fa.ops.spectral_profile(x)
    with pytest.raises(fa.KernelError, match="fp32"):
        fa.ops.spectral_profile(x.double())


def test_new_symbols_in_header_and_library(fa, lib):
    with open(os.path.join(ROOT, "include", "faoctasr.h")) as f:
        declared = set(re.findall(r"\b(faoctasr_[a-z0-9_]+)\s*\(", f.read()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in fa._lib.declared_symbols(), s
        assert hasattr(lib, s), s


def test_workspace_query(lib):
    K = 182
    n2 = lib.faoctasr_sprof_workspace_floats(2, 8, 1, 256, 256, 129, K)
    n1 = lib.faoctasr_sprof_workspace_floats(1, 8, 1, 256, 256, 129, K)
    assert n2 >= 2 * 8 * 256 * 3 * 129 and n1 >= 8 * 256 * 3 * 129 and n1 < n2
    # half the row-pass buffer of the full-spectrum losses (plus the power plane): below the focal frequency loss's workspace
    assert n2 < lib.faoctasr_ffl_workspace_floats(8, 1, 256, 256)
    assert lib.faoctasr_sprof_workspace_floats(2, 8, 1, 256, 256, 256, K) > n2            # the measuring switch: the full plane
    assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, 2, 3, 2, 2) > 0
    assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, 1, 64, 33, 2) < 0 and b"H" in lib.faoctasr_last_error()
    assert lib.faoctasr_sprof_workspace_floats(3, 1, 1, 8, 8, 5, 6) < 0 and b"sides" in lib.faoctasr_last_error()
    assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, 8, 8, 4, 6) < 0 and b"Wh" in lib.faoctasr_last_error()
    assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, 8, 8, 5, 7) < 0 and b"radial bins" in lib.faoctasr_last_error()
    assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, 1025, 8, 5, 6) < 0 and b"1024" in lib.faoctasr_last_error()


def test_library_counts_the_rings_like_radial_bins(fa, lib):
    for H, W in SMALL + LARGE:
        K = fa.radial_bins(H, W)[1].numel()
        assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, H, W, W // 2 + 1, K) > 0, (H, W)
        assert lib.faoctasr_sprof_workspace_floats(1, 1, 1, H, W, W // 2 + 1, K + 1) < 0, (H, W)


def test_bad_arguments_are_refused_with_a_message(lib):
    """The argument checks come before any launch, so they need no device: pointers are never dereferenced on the host."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    prof = lambda *a: lib.faoctasr_sprof_profile_fwd(*a)
    fwd = lambda *a: lib.faoctasr_sprof_loss_fwd(*a)
    bwd = lambda *a: lib.faoctasr_sprof_bwd(*a)
    P = lambda H=64, W=64, Wh=33, K=46: [p, p, p, p, p, p, p, p, p, 1, 1, H, W, Wh, K, None]
    L = lambda H=64, W=64, Wh=33, K=46, eps=1e-8, k_min=1, batch=0, per=0: [p, p, p, p, p, p, p, eps, k_min, batch, per, p, p, p, p, p, p, 1, 1, H, W, Wh, K, None]
    B = lambda H=64, W=64, Wh=33, K=46: [p, 0, None, p, p, p, p, p, p, p, p, p, 1, 1, H, W, Wh, K, None]
    for H, W in ((1, 64), (64, 1)):
        for f, a, name in ((prof, P, b"sprof_profile_fwd"), (fwd, L, b"sprof_loss_fwd"), (bwd, B, b"sprof_bwd")):
            assert f(*a(H=H, W=W)) == -1 and name in lib.faoctasr_last_error()
    for f, a in ((prof, P), (fwd, L), (bwd, B)):
        assert f(*a(H=1025)) == -2 and b"1024" in lib.faoctasr_last_error()
        assert f(*a(Wh=32)) == -1 and b"Wh" in lib.faoctasr_last_error()
        assert f(*a(K=45)) == -1 and b"radial bins" in lib.faoctasr_last_error()
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(*L(eps=eps)) == -1 and b"eps" in lib.faoctasr_last_error()
    for k_min in (-1, 46):
        assert fwd(*L(k_min=k_min)) == -1 and b"k_min" in lib.faoctasr_last_error()
    assert fwd(*L(batch=1, per=1)) == -1 and b"per_image" in lib.faoctasr_last_error()
    for k in (0, 1, 2, 3, 4, 5, 6, 8):                            # x, tabH, halfW, csr_off, csr_idx, cnt, A, workspace; `save` (7) may be null
        a = P()
        a[k] = None
        assert prof(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    for k in (0, 1, 2, 3, 4, 5, 6, 11, 13, 16):                   # loss_per_image (12), save_x (14), save_y (15) may be null
        a = L()
        a[k] = None
        assert fwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    a = L(per=1)
    a[12] = None
    assert fwd(*a) == -1 and b"per_image" in lib.faoctasr_last_error()
    for k in (5, 6, 7, 8, 11):                                    # tabH, halfW, binmap, cnt, workspace
        a = B()
        a[k] = None
        assert bwd(*a) == -1 and b"null" in lib.faoctasr_last_error(), k
    a = B()
    a[2] = p                                                      # both g and gA
    assert bwd(*a) == -1 and b"exactly one" in lib.faoctasr_last_error()
    a[0] = None
    assert bwd(*a) == -1 and b"one input" in lib.faoctasr_last_error()          # the profile has no dy
    a = B()
    a[3] = None                                                   # dx wanted, nothing saved for x
    assert bwd(*a) == -1 and b"saved nothing" in lib.faoctasr_last_error()
    a = B()
    a[9] = a[10] = None                                           # neither gradient wanted: nothing to do, and nothing is launched
    assert bwd(*a) == 0


# ---- the sixteenth record of train.OPT_IN_TERMS, by behaviour (the stubs of tests/test_train_terms_cpu.py, restated) --------------
W_ = 0.3
OLDER = ("ssim", "whf", "phase", "cwt", "cwssim", "msssim", "haarpsi", "gmsd", "vessel", "vif", "cldice", "ffl", "tv", "mi", "lncc")


@pytest.fixture(scope="module")
def nets(fa):
    return (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))


class Stub:
    """Stands in for the term's module: records the operands of every call, returns the next chosen value."""

    def __init__(self, values):
        self.values, self.calls = list(values), []

    def __call__(self, *args):
        self.calls.append(args)
        return torch.tensor(self.values[(len(self.calls) - 1) % len(self.values)], dtype=torch.float32)


@pytest.fixture
def plain_losses(fa, monkeypatch):
    monkeypatch.setattr(fa.ops, "mse_loss", lambda a, b, weight=1.0: weight * ((a - b) ** 2).mean())
    monkeypatch.setattr(fa.ops, "l1_loss", lambda a, b, weight=1.0: weight * (a - b).abs().mean())
    monkeypatch.setattr(fa.ops, "bce_with_logits", lambda i, t, weight=1.0: weight * F.binary_cross_entropy_with_logits(i, t))


def batch():
    g = torch.Generator().manual_seed(5)
    img = lambda: torch.rand(1, 1, 4, 4, generator=g) * 2 - 1
    real_A, real_B = img(), img()
    o = {k: img() for k in ("fake_A", "fake_B", "recovered_A", "recovered_B", "idt_A", "idt_B", "pred_fake_A", "pred_fake_B",
                            "hf_feature_A", "hf_feature_recovered_A", "hf_feature_B", "hf_feature_recovered_B")}
    return o, real_A, real_B


def left_to_right(values, start):
    acc = start
    for v in values:
        acc = f32(acc + v)
    return acc


def test_table_record(fa):
    t = fa.train.OPT_IN_TERMS
    assert len(t) == 16 and [r.name for r in t] == list(OLDER) + ["sprof"]
    assert (t[-1].side, t[-1].attr, t[-1].check) == ("domain", "sprof", "number")
    assert [r.side for r in t].count("domain") == 1
    sig = inspect.signature(fa.TrainStep.__init__)
    assert [sig.parameters[k].default for k in ("sprof_weight", "sprof_eps", "sprof_k_min", "sprof_batch")] == [0.0, 1e-8, 1, True]
    names = list(sig.parameters)                     # keyword-only in practice; the tests of earlier terms pin the keywords from ffl_weight on
    at = names.index("cldice_iters")
    assert names[at + 1:at + 6] == ["sprof_weight", "sprof_eps", "sprof_k_min", "sprof_batch", "ffl_weight"]


def test_generator_loss_formula_and_operands(fa, nets, plain_losses):
    """``loss_sprof = w * (S(fake_B, real_B) + S(fake_A, real_A))`` in fp32, the B-domain pair on the left, operands by identity."""
    vA, vB = 0.7, 0.9
    ts = fa.TrainStep(*nets, device="cpu", sprof_weight=W_)
    assert isinstance(ts.sprof, fa.SpectralProfileLoss) and (ts.sprof.eps, ts.sprof.k_min, ts.sprof.batch_profile) == (1e-8, 1, True)
    o, real_A, real_B = batch()
    stub = ts.sprof = Stub((vA, vB))
    L = ts.generator_loss(o, real_A, real_B)
    want, halves = f32(W_) * (f32(vA) + f32(vB)), f32(W_) * f32(vA) + f32(W_) * f32(vB)
    assert want != halves                                           # the stub values tell the two forms apart
    assert L["loss_sprof"].dtype == torch.float32 and L["loss_sprof"].item() == want.item()
    assert len(stub.calls) == 2 and all(len(c) == 2 for c in stub.calls)
    assert stub.calls[0][0] is o["fake_B"] and stub.calls[0][1] is real_B
    assert stub.calls[1][0] is o["fake_A"] and stub.calls[1][1] is real_A
    assert [k for k in L if k.startswith("loss_") and k[5:] in OLDER + ("sprof",)] == ["loss_sprof"]
    base = left_to_right([f32(L[k].item()) for k in ("loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")], f32(L["loss_GAN_A2B"].item()))
    assert L["_root"].item() == f32(base + want).item() and L["loss_G"] is L["_root"]


def test_pair_terms_domain(fa, nets):
    """``_pair_terms("domain", fake, real)``: ``w * S`` of that pair, the fake first; the cycle and fake sides know nothing of it."""
    ts = fa.TrainStep(*nets, device="cpu", sprof_weight=W_)
    o, real_A, real_B = batch()
    stub = ts.sprof = Stub((0.7,))
    t = ts._pair_terms("domain", o["fake_B"], real_B)
    assert list(t) == ["loss_sprof"] and t["loss_sprof"].item() == (f32(W_) * f32(0.7)).item()
    assert len(stub.calls) == 1 and stub.calls[0][0] is o["fake_B"] and stub.calls[0][1] is real_B
    assert ts._extension_terms(o["recovered_B"], real_B) == {} and ts._fake_terms(o["fake_A"], real_B) == {} and len(stub.calls) == 1
    src = inspect.getsource(fa.TrainStep._generators_two_chains)
    assert '_pair_terms("domain", o["fake_B"], real_B)' in src and '_pair_terms("domain", o["fake_A"], real_A)' in src
    assert "if self.sprof_weight:" in inspect.getsource(fa.TrainStep.step)


def test_key_sits_last(fa, nets, plain_losses, monkeypatch):
    ts = fa.TrainStep(*nets, device="cpu", lncc_weight=W_, tv_weight=W_, sprof_weight=W_)
    o, real_A, real_B = batch()
    ts.lncc, ts.sprof = Stub((0.1, 0.2)), Stub((0.7, 0.9))
    monkeypatch.setattr(fa.ops, "tv_loss", Stub((0.3, 0.4)))
    L = ts.generator_loss(o, real_A, real_B)
    assert list(L) == ["loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt", "loss_tv", "loss_lncc", "loss_sprof", "_root", "loss_G"]
    summed = [k for k in L if k not in ("_root", "loss_G")]
    assert L["_root"].item() == left_to_right([f32(L[k].item()) for k in summed[1:]], f32(L[summed[0]].item())).item()


def test_absent_with_all_weights_off(fa, nets, plain_losses, monkeypatch):
    built = []
    monkeypatch.setattr(fa.train, "SpectralProfileLoss", lambda **kw: built.append(kw))
    ts = fa.TrainStep(*nets, device="cpu")
    o, real_A, real_B = batch()
    assert ts.sprof_weight == 0.0 and ts.sprof is None and not built
    assert list(ts.generator_loss(o, real_A, real_B)) == ["loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt", "_root", "loss_G"]
    assert ts._pair_terms("domain", o["fake_B"], real_B) == {}
    fa.TrainStep(*nets, device="cpu", sprof_weight=0.5, sprof_eps=1e-6, sprof_k_min=2, sprof_batch=False)
    assert built == [dict(eps=1e-6, k_min=2, batch_profile=False)]


def test_weight_validation(fa, nets):
    for bad in (-1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="sprof_weight must be a finite number >= 0, got %s" % repr(bad).replace("'", ".")):
            fa.TrainStep(*nets, device="cpu", sprof_weight=bad)
    for kw in (dict(sprof_eps=0.0), dict(sprof_eps=float("nan")), dict(sprof_k_min=-1), dict(sprof_k_min=1.5)):
        with pytest.raises(ValueError, match="eps|k_min"):
            fa.TrainStep(*nets, device="cpu", sprof_weight=0.5, **kw)
