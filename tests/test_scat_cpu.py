"""The DTCWT scattering layers without a GPU: a plain-torch restatement of ``ScatLayer`` / ``ScatLayerj2`` and of their backward
passes, written from the mathematics (a dual-tree level from tests/test_dtcwt_cpu.py, z -> sqrt(|z|^2 + b^2) - b with the unit
phasor z / r kept for the way back, the 2x2 mean of the lowpass and its adjoint a quarter of the nearest upsampling), pinned to
the reference's own float64 results (tests/golden/golden_scat_*.npz, tools/gen_golden_scat.py), and the host logic of ``ops`` and
``wavelets`` (everything that raises before an entry point is reached).

Bound.  Restatement against the fixtures' float64 arrays: relative L2 <= 1e-12 -- both sides are float64 sums of a few hundred
terms followed by pointwise operations of condition number about 1 (b > 0 keeps r away from zero), about 1e-14 of rounding."""
import glob
import os

import numpy as np
import pytest
import torch
from torch.autograd import Function

from test_dtcwt_cpu import decode, fwd_j1, fwd_j2, inv_j1, inv_j2, rel_l2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BANKS = ("a", "b", "c")
BUFS = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")
MAGBIAS = 1e-2
J1_MODES = ("symmetric", "zero")
J1_SHAPES = (((2, 3, 16, 24), False), ((2, 3, 16, 24), True), ((1, 2, 13, 19), False), ((1, 1, 2, 2), False))
J2_SHAPES = (((2, 3, 16, 24), False), ((2, 3, 16, 24), True), ((1, 2, 13, 19), False), ((1, 1, 8, 8), False))
_gold = {}


def gold(bank):
    if bank not in _gold:
        with np.load(os.path.join(GOLDEN, "golden_scat_%s.npz" % bank)) as z:
            _gold[bank] = {k: z[k] for k in z.files}
    return _gold[bank]


def fixture_cases():
    """(case id, bank, order, mode, shape, combine_colour)"""
    out = []
    for b in BANKS:
        out += [("j1_%s_%dx%dx%dx%d%s" % ((m,) + s + ("_cc" if cc else "",)), b, 1, m, s, cc) for m in J1_MODES for s, cc in J1_SHAPES]
        out += [("j2_symmetric_%dx%dx%dx%d%s" % (s + ("_cc" if cc else "",)), b, 2, "symmetric", s, cc) for s, cc in J2_SHAPES]
    return out


def case_name(case):
    return "%s_%s" % (case[1], case[0])


def bufs(bank, dtype=torch.float64):
    """The six registered tap parameters of a bank pair as flat tensors (taps reversed, as prep_filt stores them)."""
    g = gold(bank)
    return {n: torch.from_numpy(g["buf_" + n]).reshape(-1).to(dtype) for n in BUFS}


def tuples(bank):
    """(biort, qshift) in the order the constructors take them."""
    w = {k: v.flip(0).tolist() for k, v in bufs(bank).items()}
    return (w["h0o"], w["h1o"]), (w["h0a"], w["h0b"], w["h1a"], w["h1b"])


# ------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------
def pool(ll):
    return (ll[..., 0::2, 0::2] + ll[..., 0::2, 1::2] + ll[..., 1::2, 0::2] + ll[..., 1::2, 1::2]) * 0.25


def unpool(d):
    """The adjoint of ``pool``."""
    return d.repeat_interleave(2, -2).repeat_interleave(2, -1) * 0.25


def smooth_mag(h, bias, colour):
    """h (N, C, 6, h, w, 2) -> the magnitudes (N, C or 1, 6, h, w) and the unit phasors (N, C, 6, h, w, 2)."""
    s = h[..., 0] ** 2 + h[..., 1] ** 2
    if colour:
        s = s.sum(1, keepdim=True)
    r = torch.sqrt(s + bias * bias)
    return r - bias, h / r.unsqueeze(-1)


class RScat1(Function):
    """One scattering order at one scale on an even-sided x: Z (N, 7, C, h, w), or (N, 9, h, w) for the colour form."""

    @staticmethod
    def forward(ctx, x, b, sym, bias, colour):
        ll, h = fwd_j1(x, b["h0o"], b["h1o"], sym)
        mag, phase = smooth_mag(h, bias, colour)
        ctx.cfg = (b, sym, colour)
        ctx.save_for_backward(phase)
        if colour:
            return torch.cat((pool(ll), mag[:, 0]), 1)
        return torch.cat((pool(ll)[:, None], mag.transpose(1, 2)), 1)

    @staticmethod
    def backward(ctx, dZ):
        b, sym, colour = ctx.cfg
        phase, = ctx.saved_tensors
        dlow, dmag = (dZ[:, :3], dZ[:, 3:][:, None]) if colour else (dZ[:, 0], dZ[:, 1:].transpose(1, 2))
        return inv_j1(unpool(dlow), dmag.unsqueeze(-1) * phase, b["h0o"], b["h1o"], sym), None, None, None, None


class RScat2(Function):
    """Second-order scattering over two scales on an x whose sides are multiples of 8: Z (N, 49, C, h, w) or (N, 51, h, w)."""

    @staticmethod
    def forward(ctx, x, b, bias, colour):
        N, C = x.shape[:2]
        q = (b["h0a"], b["h0b"], b["h1a"], b["h1b"])
        s0, h = fwd_j1(x, b["h0o"], b["h1o"], True)
        m1, p1 = smooth_mag(h, bias, colour)                                     # (N, C1, 6, h2, w2)
        C1 = m1.shape[1]
        ll2, h = fwd_j2(s0, *q)
        m2, p2 = smooth_mag(h, bias, colour)                                     # (N, C1, 6, h4, w4)
        u = m1.transpose(1, 2).reshape(N, 6 * C1, m1.shape[3], m1.shape[4])      # channel o1 C1 + c
        l1, h = fwd_j1(u, b["h0o"], b["h1o"], True)
        m21, p21 = smooth_mag(h, bias, False)                                    # (N, 6 C1, 6 (o2), h4, w4)
        hw = m21.shape[3:]
        s2 = m21.reshape((N, 6, C1, 6) + hw).permute(0, 3, 1, 2, 4, 5).reshape((N, 36, C1) + hw)      # index 6 o2 + o1
        ctx.cfg = (b, colour, C1)
        ctx.save_for_backward(p1, p2, p21)
        if colour:
            return torch.cat((pool(ll2), pool(l1), m2[:, 0], s2[:, :, 0]), 1)
        return torch.cat((pool(ll2)[:, None], pool(l1).reshape((N, 6, C) + hw), m2.transpose(1, 2), s2), 1)

    @staticmethod
    def backward(ctx, dZ):
        b, colour, C1 = ctx.cfg
        p1, p2, p21 = ctx.saved_tensors
        N, hw = dZ.shape[0], tuple(dZ.shape[-2:])
        if colour:
            d_s0, d_s1, d_m2, d_s2 = dZ[:, :3], dZ[:, 3:9], dZ[:, 9:15][:, None], dZ[:, 15:][:, :, None]
        else:
            d_s0, d_s1, d_m2, d_s2 = dZ[:, 0], dZ[:, 1:7].reshape((N, 6 * C1) + hw), dZ[:, 7:13].transpose(1, 2), dZ[:, 13:]
        d_m21 = d_s2.reshape((N, 6, 6, C1) + hw).permute(0, 2, 3, 1, 4, 5).reshape((N, 6 * C1, 6) + hw)
        du = inv_j1(unpool(d_s1), d_m21.unsqueeze(-1) * p21, b["h0o"], b["h1o"], True)
        d_m1 = du.reshape((N, 6, C1) + tuple(du.shape[-2:])).transpose(1, 2)
        ds0 = inv_j2(unpool(d_s0), d_m2.unsqueeze(-1) * p2, b["h0b"], b["h0a"], b["h1b"], b["h1a"])     # the trees swapped
        return inv_j1(ds0, d_m1.unsqueeze(-1) * p1, b["h0o"], b["h1o"], True), None, None, None


def layer1(x, b, mode, colour=False, bias=MAGBIAS):
    """``ScatLayer``: (N, 7C, h, w) or (N, 9, h, w); an odd side repeats its last row / column."""
    if x.shape[2] % 2:
        x = torch.cat((x, x[:, :, -1:]), 2)
    if x.shape[3] % 2:
        x = torch.cat((x, x[:, :, :, -1:]), 3)
    Z = RScat1.apply(x, b, mode == "symmetric", bias, colour)
    return Z if colour else Z.reshape(Z.shape[0], -1, Z.shape[3], Z.shape[4])


def layer2(x, b, colour=False, bias=MAGBIAS):
    """``ScatLayerj2``: (N, 49C, h, w) or (N, 51, h, w); a side is brought to a multiple of 8 by its own first and last rows."""
    for dim in (2, 3):
        rem = x.shape[dim] % 8
        if rem:
            n, before, after = x.shape[dim], (8 - rem) // 2, (9 - rem) // 2
            x = torch.cat((x.narrow(dim, 0, before), x, x.narrow(dim, n - after, after)), dim)
    Z = RScat2.apply(x, b, bias, colour)
    return Z if colour else Z.reshape(Z.shape[0], -1, Z.shape[3], Z.shape[4])


def restate(x, b, order, mode, colour, cot, dtype):
    """{"Z", "xgrad"} of a layer from the restatement in ``dtype``."""
    b = {k: v.to(dtype) for k, v in b.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    Z = layer1(x, b, mode, colour) if order == 1 else layer2(x, b, colour)
    Z.backward(cot.to(dtype))
    return {"Z": Z.detach(), "xgrad": x.grad}


def fixture_inputs(case):
    cid, bank, order, mode, shape, colour = case
    g = gold(bank)
    return torch.from_numpy(g["x_%dx%dx%dx%d" % shape]), decode(g[cid + "/cot"])


_restated = {}


def restate_case(case):
    """The float64 restatement of a fixture case, computed once and shared (do not modify the arrays)."""
    key = case_name(case)
    if key not in _restated:
        x, cot = fixture_inputs(case)
        _restated[key] = restate(x, bufs(case[1]), case[2], case[3], case[5], cot, torch.float64)
    return _restated[key]


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_fixture_files_are_small():
    files = glob.glob(os.path.join(GOLDEN, "golden_scat_*.npz"))
    assert len(files) == 3 and all(os.path.getsize(f) < 1 << 20 for f in files)


@pytest.mark.parametrize("case", fixture_cases(), ids=case_name)
def test_restatement_matches_reference(case):
    g, ref = gold(case[1]), restate_case(case)
    for k, v in ref.items():
        want = g[case[0] + "/" + k]
        assert tuple(v.shape) == want.shape, (k, tuple(v.shape), want.shape)
        assert rel_l2(v, want) <= 1e-12, (k, rel_l2(v, want))


def test_fp32_reference_error_is_meaningful():
    """The fp32 reference sits 1e-8 .. 1e-6 from the fp64 one on every array: e_ref of the GPU test's bar is neither zero nor
    large."""
    for case in fixture_cases():
        g = gold(case[1])
        for k in ("Z", "xgrad"):
            e = rel_l2(g[case[0] + "/f32/" + k], g[case[0] + "/" + k])
            assert 1e-9 < e < 2e-6, (case_name(case), k, e)


def test_restated_backward_is_the_gradient():
    """The written-out backward passes against finite differences of the restated forward, in float64."""
    b = bufs("a")
    g = torch.Generator().manual_seed(4)
    for fn, shape in ((lambda t: layer1(t, b, "symmetric"), (1, 2, 4, 6)), (lambda t: layer1(t, b, "zero", True), (1, 3, 4, 4)),
                      (lambda t: layer2(t, b), (1, 1, 8, 8)), (lambda t: layer2(t, b, True), (1, 3, 8, 8))):
        x = torch.randn(*shape, generator=g, dtype=torch.float64).requires_grad_(True)
        Z = fn(x)
        c = torch.randn(Z.shape, generator=g, dtype=torch.float64)
        Z.backward(c)
        d = torch.randn(*shape, generator=g, dtype=torch.float64)
        eps = 1e-6
        with torch.no_grad():
            fd = float(((fn(x + eps * d) - fn(x - eps * d)) * c).sum()) / (2 * eps)
        an = float((x.grad * d).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(fd), abs(an)), (shape, fd, an)


# ------------------------------------------------------------------------------------------------------------------------
# host logic: nothing below reaches an entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


def test_exports(fa):
    assert fa.ScatLayer is fa.wavelets.ScatLayer and fa.ScatLayerj2 is fa.wavelets.ScatLayerj2
    assert "ScatLayer" in fa.__all__ and "ScatLayerj2" in fa.__all__
    for n in ("scat_fwd_j1", "scat_fwd_j2", "scat_bwd_j1", "scat_bwd_j2"):
        assert "faoctasr_" + n in fa._lib.declared_symbols()


@pytest.mark.parametrize("bank", BANKS)
def test_modules_register_the_reference_parameters(fa, bank):
    import inspect
    fb, fq = tuples(bank)
    one, two = fa.ScatLayer(biort=fb), fa.ScatLayerj2(biort=fb, qshift=fq)
    b = bufs(bank)
    assert list(one.state_dict()) == ["h0o", "h1o"] and list(two.state_dict()) == list(BUFS)         # the reference's listing
    assert [n for n, _ in one.named_parameters()] == ["h0o", "h1o"] and [n for n, _ in two.named_parameters()] == list(BUFS)
    assert not list(one.buffers()) and not list(two.buffers())
    for mod in (one, two):
        for n, p in mod.named_parameters():
            assert isinstance(p, torch.nn.Parameter) and not p.requires_grad
            assert p.dtype == torch.float32 and tuple(p.shape) == (1, 1, len(b[n]), 1)
            assert torch.equal(p.reshape(-1), b[n].float())
    sig = inspect.signature(fa.ScatLayer.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("biort", "near_sym_a"), ("mode", "symmetric"), ("magbias", 1e-2), ("combine_colour", False)]
    sig = inspect.signature(fa.ScatLayerj2.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("biort", "near_sym_a"), ("qshift", "qshift_a"), ("mode", "symmetric"), ("magbias", 1e-2), ("combine_colour", False)]
    assert (one.mode, one.mode_str, one.magbias, one.combine_colour) == (1, "symmetric", 1e-2, False)


def test_closed_form_bank_and_extra_repr(fa):
    one = fa.ScatLayer()
    assert torch.equal(one.h0o.reshape(-1), bufs("a")["h0o"].float()) and torch.equal(one.h1o.reshape(-1), bufs("a")["h1o"].float())
    assert one.extra_repr() == "biort='near_sym_a', mode='symmetric', magbias=0.01"
    two = fa.ScatLayerj2(biort="legall", qshift=tuples("c")[1], mode="zero", magbias=0.5)
    assert two.extra_repr() == "biort='legall', mode='zero', magbias=0.5" and two.mode == 0
    assert torch.equal(two.h1o.reshape(-1), bufs("c")["h1o"].float())
    assert repr(one).startswith("ScatLayer(biort='near_sym_a'")


def test_state_dict_round_trip(fa):
    fb, fq = tuples("b")
    src, dst = fa.ScatLayerj2(biort=fb, qshift=fq), fa.ScatLayerj2(biort="legall", qshift=tuples("a")[1])
    with pytest.raises(RuntimeError, match="size mismatch"):
        dst.load_state_dict(src.state_dict())
    dst = fa.ScatLayerj2(biort=fb, qshift=[[0.0] * 16] * 4)
    dst.load_state_dict(src.state_dict())
    assert all(torch.equal(getattr(dst, n), getattr(src, n)) for n in BUFS)
    assert dst._taps["h0a"] == src._taps["h0a"]


def test_three_filter_variants_are_refused(fa):
    with pytest.raises(NotImplementedError, match="near_sym_b_bp.*third filter"):
        fa.ScatLayer(biort="near_sym_b_bp")
    with pytest.raises(NotImplementedError, match="near_sym_b_bp.*third filter"):
        fa.ScatLayerj2(biort="near_sym_b_bp", qshift="qshift_b_bp")
    with pytest.raises(NotImplementedError, match="qshift_b_bp.*third filter"):
        fa.ScatLayerj2(biort="legall", qshift="qshift_b_bp")


def test_names_without_a_provider(fa, monkeypatch):
    monkeypatch.setattr(fa.wavelets, "_DTCWT_PROVIDERS", ("no_such_module_for_dtcwt.coeffs",))
    with pytest.raises(NotImplementedError, match="antonini.*2-tuple"):
        fa.ScatLayer(biort="antonini")
    with pytest.raises(NotImplementedError, match="qshift_a.*4-tuple"):
        fa.ScatLayerj2()
    with pytest.raises(NotImplementedError, match="near_sym_b.*2-tuple"):
        fa.ScatLayerj2(biort="near_sym_b", qshift=tuples("b")[1])


def test_j2_runs_in_symmetric_mode_only(fa):
    fb, fq = tuples("a")
    layer = fa.ScatLayerj2(biort=fb, qshift=fq, mode="zero")
    with pytest.raises(NotImplementedError, match="symmetric"):
        layer(torch.zeros(1, 1, 8, 8))
    with pytest.raises(NotImplementedError, match="symmetric"):
        fa.ops.scat_layer_j2(torch.zeros(1, 1, 8, 8), fb[0], fb[1], *fq, mode=0)
    with pytest.raises(ValueError, match="Unkown pad type"):
        fa.ScatLayer(mode="nope")


def test_every_refusal_is_raised_on_the_host(fa):
    """CPU tensors throughout: the device check comes last, so each named check fires before it -- and before any launch."""
    fb, fq = tuples("a")
    ops, x = fa.ops, torch.zeros(1, 3, 8, 8)
    o3, o5, e10 = [0.25, 0.5, 0.25], [0.1] * 5, [0.1] * 10
    with pytest.raises(ValueError, match="odd"):
        ops.scat_layer_j1(x, [0.5] * 4, o3)
    with pytest.raises(ValueError, match="odd"):
        ops.scat_layer_j1(x, o5, [0.1] * 21)
    with pytest.raises(ValueError, match="even"):
        ops.scat_layer_j2(x, o5, o3, *([[0.1] * 22] * 4))
    with pytest.raises(ValueError, match="same length"):
        ops.scat_layer_j2(x, o5, o3, e10, e10, [0.1] * 8, e10)
    with pytest.raises(ValueError, match="odd"):
        fa.ScatLayer(biort=([0.5] * 4, o3))
    with pytest.raises(ValueError, match="2-tuple"):
        fa.ScatLayer(biort=fb + fb)
    with pytest.raises(ValueError, match="4-tuple"):
        fa.ScatLayerj2(biort=fb, qshift=fq[:3])
    with pytest.raises(ValueError, match="4 dimensions"):
        ops.scat_layer_j1(torch.zeros(8, 8), o5, o3)
    with pytest.raises(ValueError, match="4 dimensions"):
        fa.ScatLayer()(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="3 channels"):
        ops.scat_layer_j1(torch.zeros(1, 2, 8, 8), o5, o3, 1, 1e-2, True)
    with pytest.raises(ValueError, match="3 channels"):
        fa.ScatLayer(combine_colour=True)(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="3 channels"):
        fa.ScatLayerj2(biort=fb, qshift=fq, combine_colour=True)(torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError, match="multiple of 2"):
        ops.scat_layer_j1(torch.zeros(1, 1, 7, 8), o5, o3)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.scat_layer_j2(torch.zeros(1, 1, 8, 12), o5, o3, e10, e10, e10, e10)
    with pytest.raises(ValueError, match="Unkown pad type"):
        ops.scat_layer_j1(x, o5, o3, 7)
    with pytest.raises(ValueError, match="float32"):
        ops.scat_layer_j1(x.double(), o5, o3)
    with pytest.raises(ValueError, match="float32"):
        fa.ScatLayerj2(biort=fb, qshift=fq)(x.double())
    with pytest.raises(ValueError, match="device"):
        ops.scat_layer_j1(x, o5, o3)
    with pytest.raises(ValueError, match="device"):
        fa.ScatLayerj2(biort=fb, qshift=fq, combine_colour=True)(x)


def test_output_shape_table(fa):
    """ops.scat_sizes for even and odd sides against the restatement's shapes."""
    b = bufs("c")
    for H, W in ((16, 24), (13, 19), (2, 2), (8, 8), (9, 30), (17, 7)):
        for C, colour in ((2, False), (3, True)):
            x = torch.zeros(1, C, H, W, dtype=torch.float64)
            (ph, pw), (oh, ow) = fa.ops.scat_sizes(H, W, 1)
            assert (ph, pw) == (H + H % 2, W + W % 2)
            assert tuple(layer1(x, b, "zero", colour).shape) == (1, 9 if colour else 7 * C, oh, ow)
            (ph, pw), (oh, ow) = fa.ops.scat_sizes(H, W, 2)
            assert ph % 8 == 0 and pw % 8 == 0 and 0 <= ph - H < 8 and 0 <= pw - W < 8
            if min(H, W) >= 4:                                       # the pad takes up to 4 of the side's own rows
                assert tuple(layer2(x, b, colour).shape) == (1, 51 if colour else 49 * C, oh, ow)
