"""2-D and 1-D DWT / IDWT modules on fused HIP kernels, behind the interface of the reference's vendored pytorch_wavelets
(pytorch_wavelets/pytorch_wavelets/dwt/transform2d.py:7-148, lowlevel.py:91-172,226-271,312-365,647-694).

Two paths.  The Haar modules (``wave='haar'`` / ``'db1'``, or 2-tap Haar arrays) run the 2x2 block kernels the OCTA networks use
and keep their scope: even H and W, the modes in which the 2-tap bank needs no padding; anything else raises
``NotImplementedError``.  Every other filter bank runs the general kernels of csrc/dwt.hip: any even number of taps from 2 to
16, per axis, any image size, the modes 'zero', 'symmetric', 'reflect', 'periodic' and 'periodization' ('per').

``wave`` takes the reference's three forms, of which the name is resolved for Haar only -- the reference looks names up in
PyWavelets, whose tables are not part of this package:
  * a 2-tuple ``(lo, hi)`` or 4-tuple ``(lo_col, hi_col, lo_row, hi_row)`` of tap sequences: ``dec_lo, dec_hi`` for
    ``DWTForward``, ``rec_lo, rec_hi`` for ``DWTInverse``;
  * any object with ``dec_lo, dec_hi, rec_lo, rec_hi`` (a ``pywt.Wavelet``, or ``daubechies(N)`` below).
An odd number of taps raises ``ValueError`` (pad with a zero tap, as PyWavelets does for biorthogonal pairs), and so does a
side below ``L/2 + 1``: one fold or wrap then covers the padding.  ``'constant'`` and ``'replicate'`` are not built.

The backward passes are the reference's own definitions, so that a drop-in user gets its training trajectory: AFB2D's is the
synthesis bank on the analysis taps plus a crop, SFB2D's the analysis bank on the synthesis taps with the mode's padding.  That
is the adjoint of the forward for 'zero' at any size and for 'periodization' at even sizes; for 'symmetric', 'reflect',
'periodic' and odd-sized 'periodization' it is NOT the adjoint (the folded samples' contributions are dropped).
"""
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import ops

_S = 1.0 / math.sqrt(2.0)
_MODES = {"zero": 0, "symmetric": 1, "per": 2, "periodization": 2, "constant": 3, "reflect": 4, "replicate": 5, "periodic": 6}
_NATIVE_MODES = (0, 1, 4, 6)


def mode_to_int(mode):
    """lowlevel.py:274-290."""
    if mode not in _MODES:
        raise ValueError("Unkown pad type: {}".format(mode))
    return _MODES[mode]


def int_to_mode(mode):
    """lowlevel.py:293-309."""
    for k, v in (("zero", 0), ("symmetric", 1), ("periodization", 2), ("constant", 3), ("reflect", 4), ("replicate", 5), ("periodic", 6)):
        if v == mode:
            return k
    raise ValueError("Unkown pad type: {}".format(mode))


class _Bank:
    def __init__(self, dec_lo, dec_hi, rec_lo, rec_hi, name):
        self.dec_lo, self.dec_hi, self.rec_lo, self.rec_hi, self.name = dec_lo, dec_hi, rec_lo, rec_hi, name
        self.dec_len = self.rec_len = len(dec_lo)

    def __repr__(self):
        return "<filter bank %s, %d taps>" % (self.name, self.dec_len)


_daubechies = {}


def daubechies(N):
    """The orthogonal Daubechies bank with N vanishing moments (2N taps), N = 1..8, as an object with ``dec_lo, dec_hi, rec_lo,
    rec_hi`` lists in PyWavelets' convention: ``rec_lo`` minimum phase, ``dec_lo = rec_lo[::-1]``,
    ``dec_hi[k] = (-1)**(k+1) * dec_lo[L-1-k]``, ``rec_hi = dec_hi[::-1]``.  Computed once, in float64, by spectral factorisation:
    |H(w)|^2 = 2 cos^2N(w/2) P(sin^2(w/2)), P(y) = sum_{k<N} C(N-1+k, k) y^k; with y = (2 - z - 1/z) / 4 every root of P gives a
    pair z, 1/z, of which the one inside the unit circle is kept, next to N zeros at z = -1; the taps are scaled to sum sqrt(2)."""
    N = int(N)
    if not 1 <= N <= 8:
        raise ValueError("daubechies(N) is built for N = 1..8, got %d" % N)
    if N not in _daubechies:
        roots = [-1.0] * N
        if N > 1:
            p = [float(math.comb(N - 1 + k, k)) for k in range(N)]
            for y in np.roots(p[::-1]):
                b = 2.0 - 4.0 * y                                   # z + 1/z = b
                d = np.sqrt(complex(b * b - 4.0))
                z = (b + d) / 2.0
                roots.append(z if abs(z) < 1.0 else (b - d) / 2.0)
        h = np.real(np.poly(np.array(roots, dtype=np.complex128)))
        rec_lo = h * (math.sqrt(2.0) / h.sum())
        dec_lo = rec_lo[::-1]
        L = 2 * N
        dec_hi = np.array([(-1.0) ** (k + 1) * dec_lo[L - 1 - k] for k in range(L)])
        _daubechies[N] = tuple(tuple(float(v) for v in a) for a in (dec_lo, dec_hi, rec_lo, dec_hi[::-1]))
    d = _daubechies[N]
    return _Bank(list(d[0]), list(d[1]), list(d[2]), list(d[3]), "db%d" % N)


def _tap_arrays(wave, analysis):
    """A wavelet object or a tuple of 2 or 4 tap sequences -> [lo_col, hi_col, lo_row, hi_row] as float64 arrays in the order given."""
    if all(hasattr(wave, a) for a in ("dec_lo", "dec_hi", "rec_lo", "rec_hi")):
        wave = (wave.dec_lo, wave.dec_hi) if analysis else (wave.rec_lo, wave.rec_hi)
    if len(wave) not in (2, 4):
        raise ValueError("wave must be a name, a wavelet object, or a tuple of 2 or 4 tap sequences; got %d sequences" % len(wave))
    taps = [np.asarray(torch.as_tensor(w).detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float64).ravel() for w in wave]
    return taps + taps if len(taps) == 2 else taps


def _named(wave):
    if wave not in ("haar", "db1"):
        raise NotImplementedError("wavelet names are resolved for 'haar' / 'db1' only (the reference looks them up in PyWavelets, "
                                  "whose tables are not part of this package); got %r.  Pass the taps instead: a (lo, hi) or "
                                  "(lo_col, hi_col, lo_row, hi_row) tuple, an object with dec_lo/dec_hi/rec_lo/rec_hi such as a "
                                  "pywt.Wavelet, or faoctasr.daubechies(N)" % (wave,))
    return daubechies(1)


def _check_taps(taps):
    for lo, hi in (taps[:2], taps[2:]):
        if len(lo) != len(hi):
            raise ValueError("lowpass and highpass filters must have the same length, got %d and %d" % (len(lo), len(hi)))
        if len(lo) % 2 or not 2 <= len(lo) <= ops.DWT_MAX_TAPS:
            raise ValueError("filter length %d: the filter banks take an even number of taps, 2 to %d (pad an odd-length filter with a "
                             "zero tap, as PyWavelets does for biorthogonal pairs)" % (len(lo), ops.DWT_MAX_TAPS))
    return taps


def _resolve(wave, analysis):
    """``wave`` -> (is_haar, (lo_col, hi_col, lo_row, hi_row)) as float64 arrays in the order given (transform2d.py:22-33,91-102)."""
    if isinstance(wave, str):
        _named(wave)
        return True, None
    taps = _tap_arrays(wave, analysis)
    if all(len(t) == 2 and abs(abs(t[0]) - _S) <= 1e-6 and abs(abs(t[1]) - _S) <= 1e-6 for t in taps):
        return True, None
    return False, _check_taps(taps)


def _check_geometry(x, mode):
    if mode not in _NATIVE_MODES:
        raise NotImplementedError("padding mode %r is outside the built Haar path" % int_to_mode(mode))
    if x.shape[-1] % 2 or x.shape[-2] % 2:
        raise NotImplementedError("odd sizes need boundary padding; the OCTA path only transforms even sizes")


def _is_haar(*filters):
    """Four 2-tap filters holding the Haar values (read through ``ops.host_taps``: once per tensor, then cached)."""
    if not all(f.numel() == 2 for f in filters):
        return False
    return all(abs(abs(v) - _S) <= 1e-6 for f in filters for v in ops.host_taps(f))


class AFB2D(Function):
    """lowlevel.py:312-365: one analysis level; ``apply(x, h0_row, h1_row, h0_col, h1_col, mode_int) -> (low, highs)``.
    As in the reference the first filter pair runs along W and the second along H (``DWTForward`` hands its ``*_col`` buffers to
    the first pair).  Four 2-tap filters holding the Haar values select the Haar block kernel; anything else runs the general bank
    on the tensors' values (read once per tensor and cached, ``ops.host_taps``).  The backward is the reference's (see the module
    docstring)."""

    @staticmethod
    def forward(ctx, x, h0_row, h1_row, h0_col, h1_col, mode):
        ctx.general = not _is_haar(h0_row, h1_row, h0_col, h1_col)
        if ctx.general:
            return ops._AFB2D.forward(ctx, x, ops.dwt_bank(h0_row, h1_row, h0_col, h1_col), mode)
        _check_geometry(x, mode)
        ll, hi = ops._HaarAFB2D.forward(ctx, x)
        return ll, hi

    @staticmethod
    def backward(ctx, low, highs):
        if ctx.general:
            return ops._AFB2D.backward(ctx, low, highs)[0], None, None, None, None, None
        return ops._HaarAFB2D.backward(ctx, low, highs), None, None, None, None, None


class SFB2D(Function):
    """lowlevel.py:647-694: one synthesis level; ``apply(low, highs, g0_row, g1_row, g0_col, g1_col, mode_int) -> y``.
    The first filter pair runs along W, the second along H; four 2-tap Haar filters select the Haar block kernel."""

    @staticmethod
    def forward(ctx, low, highs, g0_row, g1_row, g0_col, g1_col, mode):
        ctx.general = not _is_haar(g0_row, g1_row, g0_col, g1_col)
        if ctx.general:
            return ops._SFB2D.forward(ctx, low, highs, ops.dwt_bank(g0_row, g1_row, g0_col, g1_col), mode)
        if mode not in _NATIVE_MODES:
            raise NotImplementedError("padding mode %r is outside the built Haar path" % int_to_mode(mode))
        return ops._HaarSFB2D.forward(ctx, low, highs)

    @staticmethod
    def backward(ctx, dy):
        if ctx.general:
            dl, dh = ops._SFB2D.backward(ctx, dy)[:2]
        else:
            dl, dh = ops._HaarSFB2D.backward(ctx, dy)
        return dl, dh, None, None, None, None, None


def _register(module, names, taps, reverse):
    for name, t, col in zip(names, taps, (True, True, False, False)):
        t = torch.tensor(np.ascontiguousarray(t[::-1] if reverse else t), dtype=torch.get_default_dtype())
        module.register_buffer(name, t.reshape(1, 1, -1, 1) if col else t.reshape(1, 1, 1, -1))
    _record(module, names)


def _record(module, names):
    module._taps = {n: tuple(getattr(module, n).reshape(-1).tolist()) for n in names}
    module._tap_versions = {n: getattr(module, n)._version for n in names}


def _prime(module, names):
    """The buffers of a module take the taps it registered as their host record (``ops.prime_taps``), so that no call reads a
    device buffer back -- unless the buffer was written since (``load_state_dict``), which its version counter shows."""
    for n in names:
        buf = getattr(module, n)
        if buf._version == module._tap_versions.get(n) or buf._version == 0:      # 0: a fresh copy made by .to() / .cuda()
            ops.prime_taps(buf, module._taps[n])


class _TapModule(nn.Module):
    _tap_names = ()

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        _record(self, self._tap_names)              # loaded taps replace the registered ones as the host record


class DWTForward(_TapModule):
    """transform2d.py:7-74.  forward(x) -> (yl, [yh_0 .. yh_{J-1}]), yh_j of shape (N, C, 3, H_j, W_j) with band order LH, HL, HH and
    H_j = (H_{j-1} + L - 1) // 2 (``(H_{j-1} + 1) // 2`` for periodization); buffers h0_col, h1_col, h0_row, h1_row as registered by
    the reference (the decomposition taps reversed, shapes (1,1,L,1) and (1,1,1,L)).  ``wave``: see the module docstring."""

    _tap_names = ("h0_col", "h1_col", "h0_row", "h1_row")

    def __init__(self, J=1, wave="db1", mode="zero"):
        super().__init__()
        self._haar, taps = _resolve(wave, analysis=True)
        if self._haar:
            # prep_filt_afb2d reverses the decomposition taps (lowlevel.py:925-953): dec_lo [s,s], dec_hi [-s,s] -> [s,-s]
            self.register_buffer("h0_col", torch.tensor([_S, _S]).reshape(1, 1, 2, 1))
            self.register_buffer("h1_col", torch.tensor([_S, -_S]).reshape(1, 1, 2, 1))
            self.register_buffer("h0_row", torch.tensor([_S, _S]).reshape(1, 1, 1, 2))
            self.register_buffer("h1_row", torch.tensor([_S, -_S]).reshape(1, 1, 1, 2))
            _record(self, ("h0_col", "h1_col", "h0_row", "h1_row"))
        else:
            _register(self, ("h0_col", "h1_col", "h0_row", "h1_row"), taps, reverse=True)
        self.J = J
        self.mode = mode

    def forward(self, x):
        yh = []
        ll = x
        mode = mode_to_int(self.mode)
        _prime(self, ("h0_col", "h1_col", "h0_row", "h1_row"))
        for _ in range(self.J):
            ll, high = AFB2D.apply(ll, self.h0_col, self.h1_col, self.h0_row, self.h1_row, mode)
            yh.append(high)
        return ll, yh


class DWTInverse(_TapModule):
    """transform2d.py:77-148.  forward((yl, yh)) -> x; a ``None`` entry in yh stands for zero bands.  A level returns
    ``2 n - L + 2`` samples per side (``2 n`` for periodization), so an odd-sized input comes back one sample longer; a surplus
    row or column of the running lowpass is dropped between levels, as in the reference.  Buffers g0_col, g1_col, g0_row, g1_row
    hold the synthesis taps as given."""

    _tap_names = ("g0_col", "g1_col", "g0_row", "g1_row")

    def __init__(self, wave="db1", mode="zero"):
        super().__init__()
        self._haar, taps = _resolve(wave, analysis=False)
        if self._haar:
            self.register_buffer("g0_col", torch.tensor([_S, _S]).reshape(1, 1, 2, 1))
            self.register_buffer("g1_col", torch.tensor([_S, -_S]).reshape(1, 1, 2, 1))
            self.register_buffer("g0_row", torch.tensor([_S, _S]).reshape(1, 1, 1, 2))
            self.register_buffer("g1_row", torch.tensor([_S, -_S]).reshape(1, 1, 1, 2))
            _record(self, ("g0_col", "g1_col", "g0_row", "g1_row"))
        else:
            _register(self, ("g0_col", "g1_col", "g0_row", "g1_row"), taps, reverse=False)
        self.mode = mode

    def forward(self, coeffs):
        yl, yh = coeffs
        ll = yl
        mode = mode_to_int(self.mode)
        general = not self._haar
        _prime(self, ("g0_col", "g1_col", "g0_row", "g1_row"))
        for h in yh[::-1]:
            if h is None and not general:
                h = torch.zeros(ll.shape[0], ll.shape[1], 3, ll.shape[-2], ll.shape[-1], device=ll.device, dtype=ll.dtype)
            if h is not None:
                if ll.shape[-2] > h.shape[-2]:
                    ll = ll[..., :-1, :]
                if ll.shape[-1] > h.shape[-1]:
                    ll = ll[..., :-1]
            if general:                             # a missing level goes to the kernel as a null pointer: no zero tensor
                ll = ops.sfb2d(ll, h, self.g0_col, self.g1_col, self.g0_row, self.g1_row, mode)
            else:
                ll = SFB2D.apply(ll, h, self.g0_col, self.g1_col, self.g0_row, self.g1_row, mode)
        return ll


# ----------------------------------------------------------------------------------------
# the 1-D transform over rows: transform1d.py:7-115, lowlevel.py:368-424, 697-743 -> csrc/dwt1d.hip
# ----------------------------------------------------------------------------------------
class AFB1D(Function):
    """lowlevel.py:368-424: one 1-D analysis level; ``apply(x, h0, h1, mode_int) -> (x0, x1)`` for x of shape (N, C, L) and the
    filters as ``DWT1DForward`` registers them.  The backward is the reference's: the synthesis bank on the analysis taps,
    cropped to the input's length."""

    @staticmethod
    def forward(ctx, x, h0, h1, mode):
        return ops._DWT1DAnalysis.forward(ctx, x, ops.dwt1d_bank(h0, h1), int(mode), 1, None)

    @staticmethod
    def backward(ctx, dx0, dx1):
        return ops._DWT1DAnalysis.backward(ctx, dx0, dx1)[0], None, None, None


class SFB1D(Function):
    """lowlevel.py:697-743: one 1-D synthesis level; ``apply(low, high, g0, g1, mode_int) -> y``.  The backward is the analysis
    bank on the synthesis taps with the mode's padding."""

    @staticmethod
    def forward(ctx, low, high, g0, g1, mode):
        return ops._DWT1DSynthesis.forward(ctx, low, ops.dwt1d_bank(g0, g1), int(mode), None, high)

    @staticmethod
    def backward(ctx, dy):
        g = ops._DWT1DSynthesis.backward(ctx, dy)
        return g[0], g[4], None, None, None


def _taps_1d(wave, analysis):
    """``wave`` -> (lo, hi) float64 arrays in the order given; Haar is an ordinary 2-tap bank here."""
    if isinstance(wave, str):
        wave = _named(wave)
    elif not all(hasattr(wave, a) for a in ("dec_lo", "dec_hi", "rec_lo", "rec_hi")) and len(wave) != 2:
        raise ValueError("wave must be a name, a wavelet object, or a (lo, hi) pair of tap sequences; got %d sequences" % len(wave))
    return _check_taps(_tap_arrays(wave, analysis))[:2]


def _register_1d(module, taps, reverse):
    for name, t in zip(module._tap_names, taps):
        t = torch.tensor(np.ascontiguousarray(t[::-1] if reverse else t), dtype=torch.get_default_dtype())
        module.register_buffer(name, t.reshape(1, 1, -1))
    _record(module, module._tap_names)


class DWT1DForward(_TapModule):
    """transform1d.py:7-60.  forward(x) -> (yl, [yh_0 .. yh_{J-1}]) for x of shape (N, C, L): yh_j of shape (N, C, L_j) with
    L_j = (L_{j-1} + taps - 1) // 2 (``(L_{j-1} + 1) // 2`` for periodization), contiguous.  Buffers h0, h1 of shape (1, 1, taps) as
    ``prep_filt_afb1d`` registers them (the decomposition taps reversed).  ``wave``: a (lo, hi) pair, an object with
    ``dec_lo .. rec_hi``, ``daubechies(N)``, or 'haar' / 'db1'.  All J levels of a row run in ONE launch (rows up to
    ``DWT1D_FUSED_MAX`` samples; a launch per level beyond), J <= 8; every level's input needs L/2 + 1 samples."""

    _tap_names = ("h0", "h1")

    def __init__(self, J=1, wave="db1", mode="zero"):
        super().__init__()
        _register_1d(self, _taps_1d(wave, analysis=True), reverse=True)
        self.J = J
        self.mode = mode

    def forward(self, x):
        if x.dim() != 3:
            raise ValueError("Can only handle 3d inputs (N, C, L), got %d dimensions" % x.dim())
        _prime(self, self._tap_names)
        return ops.dwt1d_analysis(x, self.h0, self.h1, mode_to_int(self.mode), self.J)


class DWT1DInverse(_TapModule):
    """transform1d.py:63-115.  forward((yl, yh)) -> x; a ``None`` entry in yh stands for a zero band.  A level returns
    ``2 n - taps + 2`` samples (``2 n`` for periodization), so an odd-length input comes back one sample longer; a surplus last
    sample of the running lowpass is dropped between levels, as in the reference, and a lowpass whose length still differs from
    its level's highpass raises ``ValueError``.  Buffers g0, g1 of shape (1, 1, taps) hold the synthesis taps as given.  One
    launch for all levels (results up to ``DWT1D_FUSED_MAX`` samples a row)."""

    _tap_names = ("g0", "g1")

    def __init__(self, wave="db1", mode="zero"):
        super().__init__()
        _register_1d(self, _taps_1d(wave, analysis=False), reverse=False)
        self.mode = mode

    def forward(self, coeffs):
        yl, yh = coeffs
        if yl.dim() != 3:
            raise ValueError("Can only handle 3d inputs (N, C, L), got %d dimensions" % yl.dim())
        _prime(self, self._tap_names)
        return ops.dwt1d_synthesis(yl, list(yh), self.g0, self.g1, mode_to_int(self.mode))


# ----------------------------------------------------------------------------------------
# the stationary (undecimated, a-trous) transform: transform2d.py:151-212, lowlevel.py:175-223, 475-521 -> csrc/swt.hip
# ----------------------------------------------------------------------------------------
_SWT_MODES = {"zero": 0, "symmetric": 1, "reflect": 4, "periodic": 6, "periodization": 6, "per": 6}


def swt_mode_to_int(mode):
    """The extensions of the stationary transform.  'periodization' / 'per' stand for 'periodic': it is ``SWTForward``'s default
    in the reference, whose own pad refuses it, and PyWavelets' ``swt2`` is periodic."""
    if mode not in _SWT_MODES:
        raise ValueError("Unkown pad type: {}".format(mode))
    return _SWT_MODES[mode]


def _swt_taps(wave, analysis):
    """``wave`` -> (lo_col, hi_col, lo_row, hi_row) float64 arrays in wavelet order; Haar is an ordinary 2-tap bank here."""
    return _check_taps(_tap_arrays(_named(wave) if isinstance(wave, str) else wave, analysis))


class SWTForward(_TapModule):
    """transform2d.py:151-212 as documented there: forward(x) -> a list of J contiguous (N, C, 4, H, W) tensors, bands (ll, lh, hl, hh)
    = (W lo, H lo), (W lo, H hi), (W hi, H lo), (W hi, H hi), level j computed at dilation 2^j from band 0 of level j - 1.  Buffers
    h0_col, h1_col, h0_row, h1_row in the ``prep_filt_afb2d`` form (the decomposition taps reversed, shapes (1,1,L,1) and
    (1,1,1,L)); as ``afb2d_atrous`` uses them the *_col pair filters along H and the *_row pair along W, so a 4-tuple ``wave`` is
    (col lo, col hi, row lo, row hi).  Modes 'zero', 'symmetric', 'reflect', 'periodic' (= 'periodization', 'per'); J <= 4; every
    side at least L 2^(J-1) / 2 + 1, else ``ValueError``.  The backward is the exact adjoint in every mode (the reference
    differentiates through its pad)."""

    _tap_names = ("h0_col", "h1_col", "h0_row", "h1_row")

    def __init__(self, J=1, wave="db1", mode="periodization"):
        super().__init__()
        swt_mode_to_int(mode)
        if not 1 <= int(J) <= ops.SWT_MAX_LEVELS:
            raise ValueError("SWTForward runs J = 1..%d levels, got %r" % (ops.SWT_MAX_LEVELS, J))
        _register(self, self._tap_names, _swt_taps(wave, analysis=True), reverse=True)
        self.J = int(J)
        self.mode = mode

    def forward(self, x):
        _prime(self, self._tap_names)
        h = [ops.host_taps(getattr(self, n))[::-1] for n in self._tap_names]           # back to wavelet order
        return list(ops.swt_analysis(x, h[0], h[1], h[2], h[3], swt_mode_to_int(self.mode), self.J))


class SWTInverse(_TapModule):
    """The periodic inverse of ``SWTForward`` (PyWavelets' ``iswt2``; the reference's ``SWTInverse`` calls the decimated bank and
    does not run): forward(coeffs) -> x for the list of (N, C, 4, H, W) tensors, coarse to fine, per level and axis
    y[m] = 1/2 sum_k g0[k] lo[(m - k d + (L/2 - 1) d) mod N] + g1[k] hi[same], d = 2^level, H first, then W.  The coarsest level's
    band 0 and bands 1..3 of every level are used; the finer levels' band 0 is ignored.  Buffers g0_col, g1_col, g0_row, g1_row
    hold the synthesis taps as given (``DWTInverse``'s form).  Any mode but the periodic ones raises ``ValueError``."""

    _tap_names = ("g0_col", "g1_col", "g0_row", "g1_row")

    def __init__(self, wave="db1", mode="periodization"):
        super().__init__()
        if swt_mode_to_int(mode) != 6:
            raise ValueError("SWTInverse is built for the periodic extension only ('periodic', 'periodization', 'per'), got %r" % (mode,))
        _register(self, self._tap_names, _swt_taps(wave, analysis=False), reverse=False)
        self.mode = mode

    def forward(self, coeffs):
        _prime(self, self._tap_names)
        g = [ops.host_taps(getattr(self, n)) for n in self._tap_names]
        return ops.swt_synthesis(list(coeffs), g[0], g[1], g[2], g[3])


# ----------------------------------------------------------------------------------------
# the dual-tree complex wavelet transform: dtcwt/transform2d.py:20-254, transform_funcs.py -> csrc/dtcwt.hip
# ----------------------------------------------------------------------------------------
_DTCWT_PROVIDERS = ("pytorch_wavelets.dtcwt.coeffs", "dtcwt.coeffs")
#: the two level-1 banks with closed rational forms (Kingsbury's LeGall 5,3 and near-symmetric 5,7 pairs): (h0o, g0o, h1o, g1o)
_BIORT_CLOSED = {
    "legall": (([-1, 2, 6, 2, -1], 8), ([1, 2, 1], 4), ([-1, 2, -1], 4), ([-1, -2, 6, -2, -1], 8)),
    "near_sym_a": (([-1, 5, 12, 5, -1], 20), ([-3, -15, 73, 170, 73, -15, -3], 280), ([3, -15, -73, 170, -73, -15, 3], 280),
                   ([-1, -5, 12, -5, -1], 20)),
}


def _dtcwt_provider(kind, name):
    import importlib
    for mod in _DTCWT_PROVIDERS:
        try:
            fn = getattr(importlib.import_module(mod), kind)
        except (ImportError, AttributeError):
            continue
        return tuple(np.asarray(v, dtype=np.float64).ravel() for v in fn(name))
    form = "a 2-tuple (h0o, h1o) -- (g0o, g1o) for the inverse" if kind == "biort" else \
        "a 4-tuple (h0a, h0b, h1a, h1b) -- (g0a, g0b, g1a, g1b) for the inverse"
    raise NotImplementedError("the %s name %r is not resolved: the tap tables are data of the dtcwt / pytorch_wavelets packages and not "
                              "part of this one (only 'legall' and 'near_sym_a' are built here, from their closed forms), and neither "
                              "%s is importable.  Pass the taps instead: %s of tap sequences"
                              % (kind, name, " nor ".join(_DTCWT_PROVIDERS), form))


def dtcwt_biort(name):
    """(h0o, g0o, h1o, g1o) of a level-1 bank, the reference's ``coeffs.biort`` order, as float64 arrays."""
    if name in _BIORT_CLOSED:
        return tuple(np.asarray(num, dtype=np.float64) / den for num, den in _BIORT_CLOSED[name])
    return _dtcwt_provider("biort", name)[:4]


def dtcwt_qshift(name):
    """(h0a, h0b, g0a, g0b, h1a, h1b, g1a, g1b) of a q-shift bank, the reference's ``coeffs.qshift`` order; provider only."""
    return _dtcwt_provider("qshift", name)[:8]


def dtcwt_biort_bp(name):
    """(h0o, g0o, h1o, g1o, h2o, g2o) of a three-filter level-1 bank ('near_sym_b_bp'), the reference's ``coeffs.biort`` order;
    provider only.  ``ScatLayer(biort=(b[0], b[2], b[4]))`` builds the layer the reference names 'near_sym_b_bp'."""
    taps = _dtcwt_provider("biort", name)
    if len(taps) != 6:
        raise ValueError("%r is no three-filter level-1 bank: its table lists %d filters, not 6" % (name, len(taps)))
    return taps


def dtcwt_qshift_bp(name):
    """(h0a, h0b, g0a, g0b, h1a, h1b, g1a, g1b, h2a, h2b, g2a, g2b) of a three-filter q-shift bank ('qshift_b_bp'), the
    reference's ``coeffs.qshift`` order; provider only.  The analysis 6-tuple is ``(q[0], q[1], q[4], q[5], q[8], q[9])``."""
    taps = _dtcwt_provider("qshift", name)
    if len(taps) != 12:
        raise ValueError("%r is no three-filter q-shift bank: its table lists %d filters, not 12" % (name, len(taps)))
    return taps


def _dtcwt_taps(biort, qshift, analysis, three=True):
    """The taps of a bank as float64 arrays, level 1 first: 2 (+ 4) of a two-filter bank, 3 (+ 6) of a three-filter one (the
    rotationally symmetric banks, given as tuples; ``three`` False refuses them)."""
    if isinstance(biort, str):
        b = dtcwt_biort(biort)
        biort = (b[0], b[2]) if analysis else (b[1], b[3])
    elif len(biort) != 2 and not (three and len(biort) == 3):
        raise ValueError("biort must be a name or a 2-tuple of tap sequences (lowpass, highpass)%s; got %d sequences"
                         % (", or a 3-tuple (lowpass, highpass, bandpass) of a three-filter bank" if three else "", len(biort)))
    if qshift is None:                      # a level-1 bank alone (ScatLayer)
        qshift = ()
    elif isinstance(qshift, str):
        q = dtcwt_qshift(qshift)
        qshift = (q[0], q[1], q[4], q[5]) if analysis else (q[2], q[3], q[6], q[7])
    elif len(qshift) != 4 and not (three and len(qshift) == 6):
        raise ValueError("qshift must be a name or a 4-tuple of tap sequences (tree a low, tree b low, tree a high, tree b high)%s; got "
                         "%d sequences" % (", or a 6-tuple with the bandpass pair of a three-filter bank" if three else "", len(qshift)))
    if qshift and (len(biort) == 3) != (len(qshift) == 6):
        raise ValueError("a three-filter biort (3 tap sequences) goes with a three-filter qshift (6 tap sequences) and a two-filter "
                         "one with a two-filter one; got %d and %d sequences" % (len(biort), len(qshift)))
    taps = [np.asarray(torch.as_tensor(t).detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64).ravel()
            for t in tuple(biort) + tuple(qshift)]
    ops._dtcwt_taps1(*taps[:len(biort)])
    if qshift:
        ops._dtcwt_taps2(*taps[len(biort):])
    return taps


def _bp_names(names, taps, order):
    """The tap names of a module whose bank may carry third filters: ``names`` as they stand for 2 / 6 taps; for 3 / 9 the
    names of ``taps``' order (level 1, then the q-shift pairs) and the order the module registers them in (``order``: the
    reference's, which a state dict follows).  Returns (names in registration order, taps in that order)."""
    if len(taps) == len(names):
        return names, taps
    p = names[0][0]                         # 'h' or 'g'
    given = (p + "0o", p + "1o", p + "2o", p + "0a", p + "0b", p + "1a", p + "1b", p + "2a", p + "2b")[:len(taps)]
    by_name = dict(zip(given, taps))
    reg = tuple(n for n in order if n in by_name)
    return reg, [by_name[n] for n in reg]


def _register_dtcwt(module, taps):
    """prep_filt (dtcwt/lowlevel.py:58-67): shape (1, 1, L, 1), the taps reversed; ``taps`` in the order of ``module._tap_names``."""
    for name, t in zip(module._tap_names, taps):
        module.register_buffer(name, torch.tensor(np.ascontiguousarray(t[::-1]), dtype=torch.get_default_dtype()).reshape(1, 1, -1, 1))
    _record(module, module._tap_names)


def _per_level(value, J, what):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != J:
            raise ValueError("%s lists one entry per level: %d entries for J = %d" % (what, len(value), J))
        return [bool(v) for v in value]
    return [bool(value)] * J


def _missing(t):
    return t is None or t.dim() == 0 or t.numel() == 0


class DTCWTForward(_TapModule):
    """dtcwt/transform2d.py:20-147.  forward(x) -> (yl, yh) for x of shape (N, C, H, W): yh[j] the six complex bandpass orientations
    (15, 45, 75, 105, 135, 165 degrees) of level j, shape (N, C, 6, H_j, W_j, 2) or as ``o_dim`` / ``ri_dim`` place the orientation
    and real/imaginary axes; yl the last lowpass (twice the last bandpass a side), or with ``include_scale`` the list of every
    level's lowpass (a 0-d zero where not asked for).  A level in ``skip_hps`` computes its lowpass only and returns a 0-d zero.
    ``biort``: 'legall' or 'near_sym_a' (built from their closed forms), another name if ``pytorch_wavelets.dtcwt.coeffs`` or
    ``dtcwt.coeffs`` is importable, or a 2-tuple (h0o, h1o) of odd length 3..19; ``qshift``: a provider's name or a 4-tuple
    (h0a, h0b, h1a, h1b) of one even length 4..``ops.DTCWT_MAX_TAPS``.  A 3-tuple (h0o, h1o, h2o) with a 6-tuple (h0a, h0b, h1a, h1b,
    h2a, h2b) is a rotationally symmetric three-filter bank (the reference's near_sym_b_bp / qshift_b_bp, whose names stay refused
    for want of their tables): the diagonal bands take the bandpass filters h2 on both axes, the buffers ``h2o, h2a, h2b`` follow the
    six, ``bandpass_diag`` is True and the launches pass the third filter to the entry points of csrc/dtcwt.hip.  ``mode`` acts on level 1 only: 'symmetric', or zero padding
    for any other name; the later levels always extend symmetrically.  An odd side has its last row / column repeated; a lowpass
    side that is no multiple of 4 has its first and last row / column repeated before the next level (torch ops outside the
    kernels -- the sizes 192, 256, 512 never take them up to J = 3).  Otherwise a forward is J launches of csrc/dtcwt.hip."""

    _tap_names = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")

    def __init__(self, biort="near_sym_a", qshift="qshift_a", J=3, skip_hps=False, include_scale=False, o_dim=2, ri_dim=-1,
                 mode="symmetric"):
        super().__init__()
        if o_dim == ri_dim:
            raise ValueError("Orientations and real/imaginary parts must be in different dimensions.")
        ops.dtcwt_layout(o_dim, ri_dim)
        self.biort, self.qshift, self.J, self.o_dim, self.ri_dim, self.mode = biort, qshift, J, o_dim, ri_dim, mode
        self._tap_names, taps = _bp_names(self._tap_names, _dtcwt_taps(biort, qshift, analysis=True), self._tap_names + ("h2o", "h2a", "h2b"))
        self.bandpass_diag = len(taps) == 9     # a three-filter bank: the diagonal bands on a bandpass filter of their own
        _register_dtcwt(self, taps)
        self.skip_hps = _per_level(skip_hps, J, "skip_hps")
        self.include_scale = _per_level(include_scale, J, "include_scale")

    def forward(self, x):
        if self.J == 0:
            return x, None
        if x.dim() != 4:
            raise ValueError("the transform takes inputs of 4 dimensions (N, C, H, W), got %d" % x.dim())
        mode = mode_to_int(self.mode)
        _prime(self, self._tap_names)
        if x.shape[2] % 2:
            x = torch.cat((x, x[:, :, -1:]), dim=2)
        if x.shape[3] % 2:
            x = torch.cat((x, x[:, :, :, -1:]), dim=3)
        bp = self.bandpass_diag
        low, h = ops.dtcwt_fwd_j1(x, self.h0o, self.h1o, self.skip_hps[0], self.o_dim, self.ri_dim, mode, self.h2o if bp else None)
        highs, scales = [h], [low if self.include_scale[0] else None]
        for j in range(1, self.J):
            if low.shape[2] % 4:
                low = torch.cat((low[:, :, 0:1], low, low[:, :, -1:]), dim=2)
            if low.shape[3] % 4:
                low = torch.cat((low[:, :, :, 0:1], low, low[:, :, :, -1:]), dim=3)
            low, h = ops.dtcwt_fwd_j2(low, self.h0a, self.h0b, self.h1a, self.h1b, self.skip_hps[j], self.o_dim, self.ri_dim,
                                      self.h2a if bp else None, self.h2b if bp else None)
            highs.append(h)
            scales.append(low if self.include_scale[j] else None)
        if True in self.include_scale:
            return [s if s is not None else x.new_zeros([]) for s in scales], highs
        return low, highs


class DTCWTInverse(_TapModule):
    """dtcwt/transform2d.py:150-254.  forward((yl, yh)) -> x.  ``None``, a 0-d or an empty tensor for a bandpass level -- or for the
    lowpass, where the coarsest bandpass is given -- stands for zeros and costs nothing: its path is not computed.  A lowpass that
    is not twice its level's bandpass loses its first and last row / column (the forward's pad).  The bandpass tensors are read
    in place through their strides, whatever ``o_dim`` / ``ri_dim`` and whatever view.  Unlike the reference, a missing level-1
    bandpass keeps ``mode`` (the reference then extends symmetrically even for 'zero')."""

    _tap_names = ("g0o", "g1o", "g0a", "g0b", "g1a", "g1b")

    def __init__(self, biort="near_sym_a", qshift="qshift_a", o_dim=2, ri_dim=-1, mode="symmetric"):
        super().__init__()
        if o_dim == ri_dim:
            raise ValueError("Orientations and real/imaginary parts must be in different dimensions.")
        self._names = ops.dtcwt_layout(o_dim, ri_dim)
        self.biort, self.qshift, self.o_dim, self.ri_dim, self.mode = biort, qshift, o_dim, ri_dim, mode
        self._tap_names, taps = _bp_names(self._tap_names, _dtcwt_taps(biort, qshift, analysis=False), self._tap_names + ("g2o", "g2a", "g2b"))
        self.bandpass_diag = len(taps) == 9
        _register_dtcwt(self, taps)

    def _fit(self, low, h):
        if _missing(low) or _missing(h) or h.dim() != 6:
            return low
        size = dict(zip(self._names, h.shape))
        if low.shape[2] != 2 * size["h"]:
            low = low[:, :, 1:-1]
        if low.shape[3] != 2 * size["w"]:
            low = low[:, :, :, 1:-1]
        return low

    def forward(self, coeffs):
        low, highs = coeffs
        mode = mode_to_int(self.mode)
        _prime(self, self._tap_names)
        low = None if _missing(low) else low
        bp = self.bandpass_diag
        for h in list(highs)[:0:-1]:
            h = None if _missing(h) else h
            low = ops.dtcwt_inv_j2(self._fit(low, h), h, self.g0a, self.g0b, self.g1a, self.g1b, self.o_dim, self.ri_dim,
                                   self.g2a if bp else None, self.g2b if bp else None)
        h = None if _missing(highs[0]) else highs[0]
        return ops.dtcwt_inv_j1(self._fit(low, h), h, self.g0o, self.g1o, self.o_dim, self.ri_dim, mode, self.g2o if bp else None)


# ----------------------------------------------------------------------------------------
# DTCWT scattering layers: scatternet/layers.py -> csrc/scat.hip
# ----------------------------------------------------------------------------------------
def _register_scat(module, taps):
    """prep_filt as ``_register_dtcwt``, but as the reference's scattering layers hold their taps: frozen parameters."""
    for name, t in zip(module._tap_names, taps):
        t = torch.tensor(np.ascontiguousarray(t[::-1]), dtype=torch.get_default_dtype()).reshape(1, 1, -1, 1)
        setattr(module, name, nn.Parameter(t, requires_grad=False))
    _record(module, module._tap_names)


def _refuse_bp(biort, qshift):
    for name in (biort, qshift):
        if isinstance(name, str) and name.endswith("_bp"):
            raise NotImplementedError("%r: the name is not resolved.  The rotationally symmetric three-filter variants (near_sym_b_bp / "
                                      "qshift_b_bp) run on the third filter path of csrc/dtcwt.hip and csrc/scat.hip, but their tap "
                                      "tables are not this package's data: pass the taps, a 3-tuple (h0o, h1o, h2o) as biort and a "
                                      "6-tuple (h0a, h0b, h1a, h1b, h2a, h2b) as qshift (wavelets.dtcwt_biort_bp / dtcwt_qshift_bp read "
                                      "them from an installed provider).  DTCWTMagnitudeLoss takes two-filter banks only" % name)


#: the reference's registration order of a three-filter scattering layer's parameters (scatternet/layers.py)
_SCAT_BP_ORDER = ("h0o", "h1o", "h2o", "h0a", "h0b", "h1a", "h1b", "h2a", "h2b")


def _scat_taps(biort, qshift):
    _refuse_bp(biort, qshift)
    return _dtcwt_taps(biort, qshift, analysis=True)


class ScatLayer(_TapModule):
    """scatternet/layers.py:11-79.  One order of scattering at one scale: forward(x) for x of shape (N, C, H, W) returns
    (N, 7C, H/2, W/2) -- the C lowpass channels (the level-1 lowpass averaged 2x2), then for each of the six orientations the C
    magnitudes ``sqrt(re^2 + im^2 + magbias^2) - magbias``.  ``combine_colour`` (C == 3): the magnitude runs over the three channels
    as well, (N, 9, H/2, W/2).  ``biort`` as ``DTCWTForward`` takes it; ``mode`` 'symmetric', or zero padding for any other name.  An
    odd side has its last row / column repeated (a torch op).  The forward is one launch of csrc/scat.hip and so is the backward;
    under ``torch.no_grad()`` (or for an input that needs no gradient) no phasors are stored."""

    _tap_names = ("h0o", "h1o")

    def __init__(self, biort="near_sym_a", mode="symmetric", magbias=1e-2, combine_colour=False):
        super().__init__()
        self.biort, self.mode_str, self.mode, self.magbias, self.combine_colour = biort, mode, mode_to_int(mode), magbias, combine_colour
        self._tap_names, taps = _bp_names(self._tap_names, _scat_taps(biort, None), _SCAT_BP_ORDER)
        self.bandpass_diag = len(taps) == 3     # a three-filter bank (the reference's biort='near_sym_b_bp')
        _register_scat(self, taps)

    def forward(self, x):
        if x.dim() != 4:
            raise ValueError("a scattering layer takes inputs of 4 dimensions (N, C, H, W), got %d" % x.dim())
        if self.combine_colour and x.shape[1] != 3:
            raise ValueError("combine_colour takes 3 channels, got %d" % x.shape[1])
        _prime(self, self._tap_names)
        if x.shape[2] % 2:
            x = torch.cat((x, x[:, :, -1:]), dim=2)
        if x.shape[3] % 2:
            x = torch.cat((x, x[:, :, :, -1:]), dim=3)
        Z = ops.scat_layer_j1(x, self.h0o, self.h1o, self.mode, self.magbias, self.combine_colour, self.h2o if self.bandpass_diag else None)
        return Z if self.combine_colour else Z.view(Z.shape[0], 7 * Z.shape[2], Z.shape[3], Z.shape[4])

    def extra_repr(self):
        return "biort='{}', mode='{}', magbias={}".format(self.biort, self.mode_str, self.magbias)


class ScatLayerj2(_TapModule):
    """scatternet/layers.py:82-172.  Second-order scattering over two scales with the level-1 and the q-shift filters: forward(x)
    returns (N, 49C, H/4, W/4) -- per channel group the lowpass, the six level-1 and the six level-2 first-order magnitudes and the
    36 second-order ones (index 6 o2 + o1) --, or (N, 51, H/4, W/4) = 3 + 6 + 6 + 36 with ``combine_colour``.  A side that is no
    multiple of 8 is extended by its own leading and trailing rows / columns (torch ops, as the reference pads).  Only
    ``mode='symmetric'`` runs: any other raises ``NotImplementedError`` in ``forward``, as the reference's q-shift filters do.  The
    forward is three launches of csrc/scat.hip that write the result in place, the backward three."""

    _tap_names = ("h0o", "h1o", "h0a", "h0b", "h1a", "h1b")

    def __init__(self, biort="near_sym_a", qshift="qshift_a", mode="symmetric", magbias=1e-2, combine_colour=False):
        super().__init__()
        self.biort, self.qshift, self.mode_str, self.mode = biort, qshift, mode, mode_to_int(mode)
        self.magbias, self.combine_colour = magbias, combine_colour
        self._tap_names, taps = _bp_names(self._tap_names, _scat_taps(biort, qshift), _SCAT_BP_ORDER)
        self.bandpass_diag = len(taps) == 9
        _register_scat(self, taps)

    def forward(self, x):
        if self.mode != 1:
            raise NotImplementedError("ScatLayerj2 runs with mode='symmetric' only (the q-shift level has no other extension), got %r"
                                      % self.mode_str)
        if x.dim() != 4:
            raise ValueError("a scattering layer takes inputs of 4 dimensions (N, C, H, W), got %d" % x.dim())
        if self.combine_colour and x.shape[1] != 3:
            raise ValueError("combine_colour takes 3 channels, got %d" % x.shape[1])
        _prime(self, self._tap_names)
        for dim in (2, 3):
            rem = x.shape[dim] % 8
            if rem:
                before, after = (8 - rem) // 2, (9 - rem) // 2
                n = x.shape[dim]
                x = torch.cat((x.narrow(dim, 0, before), x, x.narrow(dim, n - after, after)), dim=dim)
        third = (self.h2o, self.h2a, self.h2b) if self.bandpass_diag else (None,) * 3
        Z = ops.scat_layer_j2(x, self.h0o, self.h1o, self.h0a, self.h0b, self.h1a, self.h1b, self.mode, self.magbias, self.combine_colour,
                              *third)
        return Z if self.combine_colour else Z.view(Z.shape[0], 49 * Z.shape[2], Z.shape[3], Z.shape[4])

    def extra_repr(self):
        return "biort='{}', mode='{}', magbias={}".format(self.biort, self.mode_str, self.magbias)


# ----------------------------------------------------------------------------------------
# DTCWT magnitude loss -> csrc/dtcwt_loss.hip
# ----------------------------------------------------------------------------------------
class DTCWTMagnitudeLoss(_TapModule):
    """forward(x, y) -> ``sum_j w_j * mean |r_j(x) - r_j(y)|`` over the six complex orientations of the levels j = 1..J of
    ``DTCWTForward(biort, qshift, J, mode)``, with the scattering layers' smoothed magnitude ``r = sqrt(re^2 + im^2 + magbias^2)``
    (its bias cancels in the difference); a level's mean runs over its N * C * 6 * h_j * w_j coefficients and there is no lowpass
    term.  A 0-d tensor with gradients to both images.  The six orientations keep +45 and -45 degrees apart and the magnitudes are
    nearly shift-invariant, so the comparison tolerates a sub-pixel misregistration that a decimated real transform penalises.

    ``biort`` / ``qshift`` / ``mode`` as ``DTCWTForward`` takes them, registered under the same buffer names; ``qshift`` is resolved
    only when J >= 2.  ``level_weights``: one weight per level (default all 1).  The three-filter ``*_bp`` banks are refused.  With H
    and W multiples of 2^J a forward is J + 1 launches of csrc/dtcwt_loss.hip that store no band, and the backward J launches of
    the transform's adjoint per image that needs a gradient; any other size takes the composition of the per-level ops with
    ``DTCWTForward``'s padding and torch ops (``ops.dtcwt_mag_loss``) -- the sizes 192, 256, 512 never do up to J = 3."""

    def __init__(self, biort="near_sym_a", qshift="qshift_a", J=3, mode="symmetric", magbias=1e-2, level_weights=None):
        super().__init__()
        if int(J) != J or J < 1:
            raise ValueError("the magnitude loss takes J >= 1 levels, got %r" % (J,))
        if not magbias > 0:
            raise ValueError("magbias must be positive (the magnitude's gradient is z / r), got %r" % (magbias,))
        if level_weights is not None and len(level_weights) != J:
            raise ValueError("level_weights lists one weight per level: %d entries for J = %d" % (len(level_weights), J))
        self.biort, self.qshift, self.J, self.mode, self.magbias = biort, qshift, int(J), mode, float(magbias)
        self.level_weights = None if level_weights is None else tuple(float(w) for w in level_weights)
        self._tap_names = DTCWTForward._tap_names if self.J >= 2 else DTCWTForward._tap_names[:2]
        _refuse_bp(biort, qshift)
        _register_dtcwt(self, _dtcwt_taps(biort, qshift if self.J >= 2 else None, analysis=True, three=False))

    def forward(self, x, y):
        mode = mode_to_int(self.mode)
        _prime(self, self._tap_names)
        q = (self.h0a, self.h0b, self.h1a, self.h1b) if self.J >= 2 else None
        return ops.dtcwt_mag_loss(x, y, self.h0o, self.h1o, q, self.J, mode, self.magbias, self.level_weights)

    def extra_repr(self):
        return "biort='{}', J={}, mode='{}', magbias={}".format(self.biort, self.J, self.mode, self.magbias)


# ----------------------------------------------------------------------------------------
# complex-wavelet structural similarity -> csrc/cwssim.hip
# ----------------------------------------------------------------------------------------
class CWSSIM(_TapModule):
    """forward(x, y) -> the complex-wavelet structural similarity (CW-SSIM; Wang & Simoncelli 2005, Sampat et al. 2009) of two
    images (N, C, H, W) over the levels j = 1..J of ``DTCWTForward(biort, qshift, J, mode)``: ``S = sum_j w_j S_j / sum_j w_j``, S_j
    the mean over n, c, the six orientations and every valid position p of a ``win x win`` box window of

        S_p = (2 |z_p| + K) / (E_p + K),   z_p = sum_W cx conj(cy),   E_p = sum_W |cx|^2 + sum_W |cy|^2.

    0 < S <= 1 and S(x, x) = 1; the module returns the index, as ``ssim`` does, and the loss is ``1 - S``.  A small translation
    turns every coefficient of a window by nearly the same phase and leaves |z_p| nearly unchanged, and unlike a magnitude
    comparison the index keeps the relative phase inside a window: it tells a vessel from a blur of the same energy.  A 0-d
    tensor, or ``(N,)`` with ``per_image``; gradients to both images.

    ``biort`` / ``qshift`` / ``mode`` as ``DTCWTForward`` takes them, registered under the same buffer names and in the same order,
    three-filter banks (a 3-tuple with a 6-tuple) included; ``qshift`` is resolved only when J >= 2, and the ``*_bp`` names stay
    refused for want of their tables.  ``level_weights``: one weight per level (default all 1).  ``1 <= win <= 11``; every level's
    bands must hold a window.  fp32, box window, no double backward (``ops.cw_ssim``)."""

    def __init__(self, biort="near_sym_a", qshift="qshift_a", J=3, mode="symmetric", win=7, K=1e-2, level_weights=None, per_image=False):
        super().__init__()
        if int(J) != J or J < 1:
            raise ValueError("the index takes J >= 1 levels, got %r" % (J,))
        ops._cwssim_check_scalars(win, K)
        if level_weights is not None and len(level_weights) != J:
            raise ValueError("level_weights lists one weight per level: %d entries for J = %d" % (len(level_weights), J))
        if level_weights is not None and not sum(float(w) for w in level_weights) > 0:
            raise ValueError("level_weights must have a positive sum (the index is their weighted mean), got %r" % (level_weights,))
        self.biort, self.qshift, self.J, self.mode, self.win, self.K = biort, qshift, int(J), mode, int(win), float(K)
        self.level_weights = None if level_weights is None else tuple(float(w) for w in level_weights)
        self.per_image = bool(per_image)
        _refuse_bp(biort, qshift)
        names = DTCWTForward._tap_names if self.J >= 2 else DTCWTForward._tap_names[:2]
        self._tap_names, taps = _bp_names(names, _dtcwt_taps(biort, qshift if self.J >= 2 else None, analysis=True),
                                          DTCWTForward._tap_names + ("h2o", "h2a", "h2b"))
        self.bandpass_diag = "h2o" in self._tap_names
        _register_dtcwt(self, taps)

    def index(self, x, y, per_image):
        """The index with ``per_image`` as given instead of the module's."""
        mode = mode_to_int(self.mode)
        _prime(self, self._tap_names)
        bp = self.bandpass_diag
        q = (self.h0a, self.h0b, self.h1a, self.h1b) if self.J >= 2 else None
        return ops.cw_ssim(x, y, self.h0o, self.h1o, q, self.J, mode, self.win, self.K, self.level_weights, per_image,
                           self.h2o if bp else None, (self.h2a, self.h2b) if bp and self.J >= 2 else None)

    def forward(self, x, y):
        return self.index(x, y, self.per_image)

    def extra_repr(self):
        return "biort='{}', J={}, mode='{}', win={}, K={}, per_image={}".format(self.biort, self.J, self.mode, self.win, self.K, self.per_image)
