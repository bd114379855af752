"""What ``TrainStep`` does with its fifteen opt-in loss terms, by behaviour (CPU only: every kernel-backed piece is replaced by a stub).

``generator_loss`` runs on the CPU once ``ops.mse_loss`` / ``ops.l1_loss`` / ``ops.bce_with_logits`` are plain torch forms, the term's
module (or its ``ops`` function) is a stub that records its operands and returns chosen fp32 scalars, and ``o`` already holds the
discriminators' predictions.  Per term: the formula bit for bit, the operands by identity and in order; then the key order and the
running total with all fifteen on, nothing at all with all fifteen off, and which weights the constructor refuses.

The expected values are restated here in numpy float32, from the rule the term is documented with (``TERMS`` below), never from the
code under test.  Stub values are chosen so that ``w * (share_A + share_B)`` and ``w * share_A + w * share_B`` differ in fp32 (each
test asserts that they do): a step that summed the chains' halves where the single-stream form is asked for would fail.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

f32 = np.float32

# name, pair, share of one pair as a function of the stub's value S (and the stub's upper bound U), where the stub goes, stub values (A, B)
ONE_MINUS, PLAIN, ONE_PLUS, UPPER_MINUS = (lambda S, U: f32(1) - S), (lambda S, U: S), (lambda S, U: f32(1) + S), (lambda S, U: U - S)
TERMS = [
    ("ssim", "cycle", ONE_MINUS, "ops.ssim", (0.1, 0.2)),
    ("whf", "cycle", None, "dwt_loss", None),
    ("phase", "cycle", ONE_PLUS, "ops.phase_loss", (0.3, 0.4)),
    ("cwt", "cycle", PLAIN, "cwt_loss", (0.7, 0.9)),
    ("cwssim", "cycle", ONE_MINUS, "cwssim", (0.1, 0.2)),
    ("msssim", "cycle", ONE_MINUS, "msssim", (0.1, 0.2)),
    ("haarpsi", "cycle", ONE_MINUS, "haarpsi", (0.1, 0.2)),
    ("gmsd", "cycle", PLAIN, "gmsd", (0.7, 0.9)),
    ("vessel", "cycle", ONE_MINUS, "vessel", (0.1, 0.2)),
    ("vif", "cycle", ONE_MINUS, "vif", (0.1, 0.2)),
    ("cldice", "cycle", PLAIN, "cldice", (0.7, 0.9)),
    ("ffl", "cycle", PLAIN, "ffl", (0.7, 0.9)),
    ("tv", "fake", PLAIN, "ops.tv_loss", (0.7, 0.9)),
    ("mi", "fake", UPPER_MINUS, "mi", (0.1, 0.2)),
    ("lncc", "fake", ONE_MINUS, "lncc", (0.1, 0.2)),
]
NAMES = [t[0] for t in TERMS]
CYCLE = [t[0] for t in TERMS if t[1] == "cycle"]
FAKE = [t[0] for t in TERMS if t[1] == "fake"]
MODULE_ATTRS = [t[3] for t in TERMS if not t[3].startswith("ops.")]
W = 0.3
UPPER = math.log(32)
WHF_BANDS = {"recovered_A": (0.7, 0.9), "recovered_B": (0.3, 0.2)}      # |band| per level; the real images' bands are 0
# the constructor's rule: these weights must be finite numbers >= 0, the last two may not be bools either; the others are not checked
# ``cwssim_levels`` >= 2 needs q-shift tap tables, which are data of other packages (wavelets.dtcwt_qshift): one level builds without
BUILD_KW = dict(cwssim_levels=1)
CHECKED, CHECKED_NO_BOOL = {"ffl", "mi", "gmsd", "vessel", "lncc"}, {"vif", "cldice"}


@pytest.fixture(scope="module")
def fa():
    import faoctasr
    return faoctasr


@pytest.fixture(scope="module")
def nets(fa):
    return (fa.NetworkA2B(), fa.NetworkB2A(), fa.FS_DiscriminatorA(1), fa.FS_DiscriminatorB(1))


class Stub:
    """Stands in for a term's module or ``ops`` function: records the operands of every call, returns the next chosen value."""

    def __init__(self, values, upper=UPPER):
        self.values, self.calls, self.upper = list(values), [], upper

    def __call__(self, *args):
        self.calls.append(args)
        return torch.tensor(self.values[(len(self.calls) - 1) % len(self.values)], dtype=torch.float32)


class Bands:
    """Stands in for ``DWTForward``: (yl, yh) with the chosen high-frequency bands of that very image, one tensor per level."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def __call__(self, img):
        self.calls.append((img,))
        return None, self.table[id(img)]


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


def install(fa, monkeypatch, ts, name, values, o, real_A, real_B):
    """Put the stub where the term looks for its value; returns it (for ``whf``: the stub ``dwt_loss``)."""
    where = TERMS[NAMES.index(name)][3]
    if name == "whf":
        table = {id(o[k]): [torch.tensor([v]) for v in vs] for k, vs in WHF_BANDS.items()}
        for real in (real_A, real_B):
            table[id(real)] = [torch.zeros(1), torch.zeros(1)]
        ts.dwt_loss = Bands(table)
        return ts.dwt_loss
    stub = Stub(values)
    if where.startswith("ops."):
        monkeypatch.setattr(fa.ops, where[4:], stub)
    else:
        setattr(ts, where, stub)
    return stub


def pairs_of(side, o, real_A, real_B):
    return ([(o["recovered_A"], real_A), (o["recovered_B"], real_B)] if side == "cycle" else [(o["fake_B"], real_A), (o["fake_A"], real_B)])


def check_operands(name, calls, pairs, ts):
    assert len(calls) == len(pairs)
    for got, (x, y) in zip(calls, pairs):
        assert got[0] is x
        if name == "tv":
            assert len(got) == 1                                    # the fake alone
        else:
            assert got[1] is y
        if name == "phase":
            assert got[2] == ts.phase_radius
        assert len(got) == {"tv": 1, "phase": 3}.get(name, 2)


def whf_levels(key):
    """The weighted L1 of each level of one pair, as the plain ``l1_loss`` above forms it: fp32(w) * |band|."""
    return [f32(W) * f32(v) for v in WHF_BANDS[key]]


def left_to_right(values, start=f32(0)):
    acc = start
    for v in values:
        acc = f32(acc + v)
    return acc


@pytest.mark.parametrize("name", [n for n in NAMES if n != "whf"])
def test_generator_loss_formula_and_operands(fa, nets, monkeypatch, plain_losses, name):
    """``L["loss_<name>"]`` is the fp32 value of ``w * (share_A + share_B)``, the A pair on the left, and ``_root`` carries it."""
    _, side, share, _, (vA, vB) = TERMS[NAMES.index(name)]
    ts = fa.TrainStep(*nets, device="cpu", **BUILD_KW, **{name + "_weight": W})
    o, real_A, real_B = batch()
    stub = install(fa, monkeypatch, ts, name, (vA, vB), o, real_A, real_B)
    L = ts.generator_loss(o, real_A, real_B)
    sA, sB = share(f32(vA), f32(UPPER)), share(f32(vB), f32(UPPER))
    want, halves = f32(W) * (sA + sB), f32(W) * sA + f32(W) * sB
    assert want != halves                                           # the stub values tell the two forms apart
    assert L["loss_" + name].dtype == torch.float32 and L["loss_" + name].item() == want.item()
    check_operands(name, stub.calls, pairs_of(side, o, real_A, real_B), ts)
    assert [k for k in L if k[5:] in NAMES] == ["loss_" + name]
    base = left_to_right([f32(L[k].item()) for k in ("loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt")], f32(L["loss_GAN_A2B"].item()))
    assert L["_root"].item() == f32(base + want).item() and L["loss_G"] is L["_root"]


def test_generator_loss_whf_is_one_running_sum(fa, nets, monkeypatch, plain_losses):
    """``whf``: the weight goes inside ``l1_loss`` and the levels of both pairs are one chain of additions, 0 + A1 + A2 + B1 + B2."""
    ts = fa.TrainStep(*nets, device="cpu", whf_weight=W, dwt_levels=2)
    o, real_A, real_B = batch()
    stub = install(fa, monkeypatch, ts, "whf", None, o, real_A, real_B)
    L = ts.generator_loss(o, real_A, real_B)
    A, B = whf_levels("recovered_A"), whf_levels("recovered_B")
    want, halves = left_to_right(A + B), f32(left_to_right(A) + left_to_right(B))
    assert want != halves
    assert L["loss_whf"].item() == want.item()
    assert len(stub.calls) == 4 and all(got[0] is img for got, img in zip(stub.calls, (o["recovered_A"], real_A, o["recovered_B"], real_B)))
    del stub.calls[:]
    for key, levels in (("recovered_A", A), ("recovered_B", B)):    # per pair: 0 + X1 + X2
        t = ts._extension_terms(o[key], real_A if key == "recovered_A" else real_B)
        assert list(t) == ["loss_whf"] and t["loss_whf"].item() == left_to_right(levels).item()


@pytest.mark.parametrize("name", [n for n in CYCLE if n != "whf"])
def test_extension_terms_formula_and_operands(fa, nets, monkeypatch, name):
    """``_extension_terms(rec, real)``: ``w * share`` of that pair, the reconstruction first."""
    _, _, share, _, (vA, _) = TERMS[NAMES.index(name)]
    ts = fa.TrainStep(*nets, device="cpu", **BUILD_KW, **{name + "_weight": W})
    o, real_A, real_B = batch()
    stub = install(fa, monkeypatch, ts, name, (vA,), o, real_A, real_B)
    t = ts._extension_terms(o["recovered_B"], real_B)
    assert list(t) == ["loss_" + name] and t["loss_" + name].item() == (f32(W) * share(f32(vA), f32(UPPER))).item()
    check_operands(name, stub.calls, [(o["recovered_B"], real_B)], ts)


@pytest.mark.parametrize("name", FAKE)
def test_fake_side_terms_formula_and_operands(fa, nets, monkeypatch, name):
    """``_fake_terms(fake, source)``: ``w * share`` of a chain's fake and the image it was made from; the cycle terms know nothing of it."""
    _, _, share, _, (vA, _) = TERMS[NAMES.index(name)]
    ts = fa.TrainStep(*nets, device="cpu", **BUILD_KW, **{name + "_weight": W})
    o, real_A, real_B = batch()
    stub = install(fa, monkeypatch, ts, name, (vA,), o, real_A, real_B)
    t = ts._fake_terms(o["fake_A"], real_B)
    assert list(t) == ["loss_" + name] and t["loss_" + name].item() == (f32(W) * share(f32(vA), f32(UPPER))).item()
    check_operands(name, stub.calls, [(o["fake_A"], real_B)], ts)
    assert ts._extension_terms(o["recovered_B"], real_B) == {} and len(stub.calls) == 1


def all_on(fa, nets, monkeypatch):
    ts = fa.TrainStep(*nets, device="cpu", dwt_levels=2, **BUILD_KW, **{n + "_weight": W + 0.05 * i for i, n in enumerate(NAMES)})
    o, real_A, real_B = batch()
    for i, n in enumerate(NAMES):
        install(fa, monkeypatch, ts, n, (0.11 + 0.03 * i, 0.23 + 0.02 * i), o, real_A, real_B)
    return ts, o, real_A, real_B


def test_all_terms_on_key_order_and_total(fa, nets, monkeypatch, plain_losses):
    """Every opt-in key between ``loss_idt`` and ``_root`` in table order; ``_root`` is the left-to-right fp32 sum of the base terms and
    the opt-in terms in that order."""
    ts, o, real_A, real_B = all_on(fa, nets, monkeypatch)
    L = ts.generator_loss(o, real_A, real_B)
    assert list(L) == ["loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt"] + ["loss_" + n for n in NAMES] + ["_root", "loss_G"]
    summed = [k for k in L if k not in ("_root", "loss_G")]
    want = left_to_right([f32(L[k].item()) for k in summed[1:]], f32(L[summed[0]].item()))
    assert L["_root"].item() == want.item()
    assert all(math.isfinite(L[k].item()) and L[k].item() > 0 for k in L)
    assert list(ts._extension_terms(o["recovered_A"], real_A)) == ["loss_" + n for n in CYCLE]


def test_all_terms_on_fake_side_keys(fa, nets, monkeypatch, plain_losses):
    ts, o, real_A, real_B = all_on(fa, nets, monkeypatch)
    assert list(ts._fake_terms(o["fake_B"], real_A)) == ["loss_tv", "loss_mi", "loss_lncc"]


def test_all_terms_off(fa, nets, plain_losses):
    """The default step: no opt-in key, no module."""
    ts = fa.TrainStep(*nets, device="cpu")
    o, real_A, real_B = batch()
    assert list(ts.generator_loss(o, real_A, real_B)) == ["loss_GAN_A2B", "loss_GAN_B2A", "loss_cycle_ABA", "loss_cycle_BAB", "loss_idt", "_root", "loss_G"]
    assert ts._extension_terms(o["recovered_A"], real_A) == {}
    assert all(getattr(ts, n + "_weight") == 0.0 for n in NAMES)
    assert all(getattr(ts, a) is None for a in MODULE_ATTRS) and len(MODULE_ATTRS) == 12


def test_all_terms_off_fake_side(fa, nets):
    ts = fa.TrainStep(*nets, device="cpu")
    o, real_A, _ = batch()
    assert ts._fake_terms(o["fake_B"], real_A) == {}


@pytest.mark.parametrize("name", NAMES)
def test_weight_validation(fa, nets, name):
    """-1, nan, inf, a string, None and True per weight: refused with the one message where the weight is checked, taken as given
    where it is not (the weights older than the check)."""
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        refused = (name in CHECKED and bad is not True) or name in CHECKED_NO_BOOL
        if refused:
            with pytest.raises(ValueError, match="%s_weight must be a finite number >= 0, got %s" % (name, repr(bad).replace("'", "."))):
                fa.TrainStep(*nets, device="cpu", **BUILD_KW, **{name + "_weight": bad})
        else:
            ts = fa.TrainStep(*nets, device="cpu", **BUILD_KW, **{name + "_weight": bad})
            got = getattr(ts, name + "_weight")
            assert got is bad or got == bad
            attr = TERMS[NAMES.index(name)][3]
            if not attr.startswith("ops."):
                assert (getattr(ts, attr) is not None) == bool(bad)
