"""SSIM behind the reference's ``ssim.py`` interface (ssim.py:7-73) on one fused separable HIP kernel, and multi-scale SSIM on the
same window behind the same interface (csrc/msssim.hip), and HaarPSI (csrc/haarpsi.hip) and the local normalised cross-correlation (csrc/lncc.hip) behind the same ``forward`` / ``index`` pair,
and GMSD and multi-scale GMSD (csrc/gmsd.hip) behind it too, and the Hessian vesselness
filter with its Dice index (csrc/vessel.hip), the pixel-domain visual information fidelity (csrc/vif.hip), and the soft skeleton
with soft-clDice (csrc/cldice.hip)."""
from math import exp

import torch

from . import ops


def gaussian(window_size, sigma):
    """ssim.py:7-9."""
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    return gauss / gauss.sum()


def create_window(window_size, channel):
    """ssim.py:11-15 (the kernel uses the separable 1-D taps; this 2-D window is kept for API parity)."""
    w1 = gaussian(window_size, 1.5).unsqueeze(1)
    w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, window_size, window_size).contiguous()


def _check(window_size):
    if window_size != 11:
        raise NotImplementedError("the fused kernel is built for the reference's 11-tap, sigma 1.5 window (ssim.py:40)")


def ssim(img1, img2, window_size=11, size_average=True):
    """ssim.py:65-73."""
    _check(window_size)
    return ops.ssim(img1, img2, size_average)


class SSIM(torch.nn.Module):
    """ssim.py:39-63."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        _check(window_size)
        self.window_size, self.size_average, self.channel = window_size, size_average, 1
        self.window = create_window(window_size, self.channel)

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average`` (what ``Registered`` and ``evaluate_pairs_with`` call)."""
        return ops.ssim(img1, img2, not per_image)

    def forward(self, img1, img2):
        return ops.ssim(img1, img2, self.size_average)


def ms_ssim(img1, img2, window_size=11, size_average=True, levels=5, weights=None, data_range=1.0):
    """Multi-scale SSIM with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with ``size_average=False`` (``ops.ms_ssim``)."""
    _check(window_size)
    return ops.ms_ssim(img1, img2, levels, weights, data_range, not size_average)


class MSSSIM(torch.nn.Module):
    """forward(img1, img2) -> multi-scale SSIM (Wang, Simoncelli & Bovik 2003) with ``SSIM``'s interface: the contrast-structure
    factor of ssim.py:17-32 at ``levels`` dyadic scales (scale j + 1 = ``avg_pool2d(scale j, 2)``) and the luminance factor at the
    coarsest, ``MS[n] = prod_j max(F_j[n], 0)^w_j``.  ``weights`` defaults to the first ``levels`` of (0.0448, 0.2856, 0.3001, 0.2363,
    0.1333), not renormalised; ``data_range`` L sets C1 = (0.01 L)^2, C2 = (0.03 L)^2.  ``levels=1, weights=(1,)`` is ``SSIM``.  The
    mean over the batch, or ``(N,)`` with ``size_average=False``; the loss is ``1 - MS``.  Every side must be at least
    ``2^(levels - 1)``; fp32, 11-tap window only, no double backward."""

    def __init__(self, window_size=11, size_average=True, levels=5, weights=None, data_range=1.0):
        super().__init__()
        _check(window_size)
        ops._msssim_check_scalars(levels, weights, data_range)
        self.window_size, self.size_average = window_size, size_average
        self.levels, self.data_range = int(levels), float(data_range)
        self.weights = None if weights is None else tuple(float(w) for w in weights)

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.ms_ssim(img1, img2, self.levels, self.weights, self.data_range, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "levels={}, weights={}, data_range={}, size_average={}".format(self.levels, self.weights, self.data_range, self.size_average)


def haarpsi(img1, img2, c=30.0, alpha=4.2, value_range=(-1., 1.), size_average=True):
    """HaarPSI with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with ``size_average=False`` (``ops.haarpsi``)."""
    return ops.haarpsi(img1, img2, c, alpha, value_range, not size_average)


class HaarPSI(torch.nn.Module):
    """forward(img1, img2) -> the Haar wavelet-based perceptual similarity index (Reisenhofer, Bosse, Kutyniok & Wiegand 2018) with
    ``SSIM``'s interface: the images are mapped from ``value_range`` to 0..255 and halved by a 2 x 2 mean; the similarity of the Haar
    coefficient magnitudes at the scales 2 and 4, ``1/2 sum_k (2 a_k b_k + c) / (a_k^2 + b_k^2 + c)``, goes through a logistic of
    slope ``alpha`` and is averaged with the scale-8 edge strength of the stronger image as weight; the score is the squared
    inverse logistic of that average.  Channels are independent grey planes pooled inside an image (no YIQ chroma term).  The mean
    over the batch, or ``(N,)`` with ``size_average=False``; the loss is ``1 - HaarPSI``.  Every side must be at least 2; fp32, no
    double backward (csrc/haarpsi.hip)."""

    def __init__(self, c=30.0, alpha=4.2, value_range=(-1., 1.), size_average=True):
        super().__init__()
        self.c, self.alpha, lo, hi = ops._haarpsi_check_scalars(c, alpha, value_range)
        self.value_range, self.size_average = (lo, hi), size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.haarpsi(img1, img2, self.c, self.alpha, self.value_range, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "c={}, alpha={}, value_range={}, size_average={}".format(self.c, self.alpha, self.value_range, self.size_average)


def lncc(img1, img2, win=9, eps=1e-5, size_average=True):
    """Local normalised cross-correlation with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with ``size_average=False``
    (``ops.lncc``)."""
    return ops.lncc(img1, img2, win, eps, not size_average)


class LNCC(torch.nn.Module):
    """forward(img1, img2) -> the local normalised cross-correlation with ``SSIM``'s interface: the squared correlation coefficient of
    the two images inside a sliding ``win x win`` box (zero padding, divisor ``win^2``), ``u^2 / (va vb + eps)`` with ``u`` the
    windowed covariance sum and ``va``, ``vb`` the windowed variance sums, averaged over the positions and channels of an image.  It
    does not change under an affine intensity map of either image inside the window, which makes it the spatial complement of the
    mutual information for pairs of different contrast.  The mean over the batch, or ``(N,)`` with ``size_average=False``; the loss
    is ``1 - LNCC``.  ``win`` odd in 3..15; fp32, no double backward (csrc/lncc.hip)."""

    def __init__(self, win=9, eps=1e-5, size_average=True):
        super().__init__()
        self.win, self.eps = ops._lncc_check_scalars(win, eps)
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.lncc(img1, img2, self.win, self.eps, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "win={}, eps={}, size_average={}".format(self.win, self.eps, self.size_average)


def gmsd(img1, img2, c=0.0026, value_range=(-1., 1.), size_average=True):
    """The gradient magnitude similarity deviation with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with
    ``size_average=False`` (``ops.gmsd``).  A distortion: 0 for identical images."""
    return ops.gmsd(img1, img2, c, value_range, not size_average)


def ms_gmsd(img1, img2, weights=None, c=0.0026, value_range=(-1., 1.), size_average=True):
    """The multi-scale gradient magnitude similarity deviation with ``ssim``'s interface (``ops.ms_gmsd``)."""
    return ops.ms_gmsd(img1, img2, weights, c, value_range, not size_average)


class GMSD(torch.nn.Module):
    """forward(img1, img2) -> the gradient magnitude similarity deviation (Xue, Zhang, Mou & Bovik 2014) with ``SSIM``'s interface.  The
    images, mapped by ``u = (x - lo) / (hi - lo)`` for ``value_range = (lo, hi)``, are pooled once by ``avg_pool2d(., 2)``; with ``ma``,
    ``mb`` the Prewitt gradient magnitudes (zero padding 1, no epsilon) of the pooled pair, ``g_p = (2 ma mb + c) / (ma^2 + mb^2 + c)``
    and ``GMSD[n]`` is the population standard deviation of ``g_p`` over the channels and positions of image n: it measures how
    unevenly quality is spread over the image, where every mean-pooled index averages a local failure away.  A distortion: 0 for
    identical images, larger is worse, and the value itself is the loss.  The mean over the batch, or ``(N,)`` with
    ``size_average=False``.  Every side at least 2; fp32, grey planes only, no double backward (csrc/gmsd.hip)."""

    def __init__(self, c=0.0026, value_range=(-1., 1.), size_average=True):
        super().__init__()
        self.c, lo, hi, _ = ops._gmsd_check_scalars(c, value_range)
        self.value_range = (lo, hi)
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.gmsd(img1, img2, self.c, self.value_range, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "c={}, value_range={}, size_average={}".format(self.c, self.value_range, self.size_average)


class MSGMSD(torch.nn.Module):
    """forward(img1, img2) -> the multi-scale gradient magnitude similarity deviation (Zhang, Shen, Wang & Li 2017) with ``SSIM``'s
    interface: ``sqrt(sum_j w_j V_j[n])`` with ``V_j`` the population variance of ``GMSD``'s similarity map at scale j, scale 1 the
    mapped input itself and scale j + 1 = ``avg_pool2d(scale j, 2)``.  ``weights`` defaults to (0.096, 0.596, 0.289, 0.019); 1..5
    weights, each finite and >= 0, not all zero; every side at least ``2^(M - 1)``.  A distortion: 0 for identical images; the value
    itself is the loss.  The mean over the batch, or ``(N,)`` with ``size_average=False``.  fp32, no double backward (csrc/gmsd.hip)."""

    def __init__(self, weights=None, c=0.0026, value_range=(-1., 1.), size_average=True):
        super().__init__()
        self.c, lo, hi, self.weights = ops._gmsd_check_scalars(c, value_range, ops.MSGMSD_WEIGHTS if weights is None else weights)
        self.value_range = (lo, hi)
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.ms_gmsd(img1, img2, self.weights, self.c, self.value_range, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "weights={}, c={}, value_range={}, size_average={}".format(self.weights, self.c, self.value_range, self.size_average)


def vessel_dice(img1, img2, sigmas=ops.VESSEL_SIGMAS, weights=None, beta=0.5, c=0.1, eps=1e-6, value_range=(-1., 1.), bright=True, size_average=True):
    """The vessel Dice index with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with ``size_average=False``
    (``ops.vessel_dice``).  An index: 1 for identical images."""
    return ops.vessel_dice(img1, img2, sigmas, weights, beta, c, eps, value_range, bright, not size_average)


class Vesselness(torch.nn.Module):
    """forward(x) -> the multi-scale Hessian vesselness of ``x`` ``(N, C, H, W)``, the shape of ``x`` (``ops.vesselness``): Frangi's 2-D
    ridge measure with the eigenvalues ordered by value, which extends it continuously over Frangi's cut at a non-negative trace, summed
    over 1 to 3 scales with weights instead of maximised.  Differentiable; fp32, grey planes, zero padding (csrc/vessel.hip)."""

    def __init__(self, sigmas=ops.VESSEL_SIGMAS, weights=None, beta=0.5, c=0.1, value_range=(-1., 1.), bright=True):
        super().__init__()
        ops._vessel_check_scalars(sigmas, weights, beta, c, value_range)
        self.sigmas = tuple(float(v) for v in sigmas)
        self.weights = None if weights is None else tuple(float(v) for v in weights)
        self.beta, self.c = float(beta), float(c)
        self.value_range = (float(value_range[0]), float(value_range[1]))
        self.bright = bool(bright)

    def forward(self, x):
        return ops.vesselness(x, self.sigmas, self.weights, self.beta, self.c, self.value_range, self.bright)

    def extra_repr(self):
        return "sigmas={}, weights={}, beta={}, c={}, value_range={}, bright={}".format(self.sigmas, self.weights, self.beta, self.c, self.value_range,
                                                                                       self.bright)


class VesselDice(torch.nn.Module):
    """forward(img1, img2) -> the continuous Dice overlap of the two images' vessel maps with ``SSIM``'s interface:
    ``S[n] = (2 mean(A B) + eps) / (mean(A^2) + mean(B^2) + eps)`` with ``A``, ``B`` the ``Vesselness`` responses and the means over the
    channels and positions of image n.  An index: 1 for identical images and for two vessel-free images, so the loss is
    ``1 - VesselDice()(a, b)``.  The mean over the batch, or ``(N,)`` with ``size_average=False``.  fp32, grey planes, zero padding, no
    double backward (csrc/vessel.hip)."""

    def __init__(self, sigmas=ops.VESSEL_SIGMAS, weights=None, beta=0.5, c=0.1, eps=1e-6, value_range=(-1., 1.), bright=True, size_average=True):
        super().__init__()
        ops._vessel_check_scalars(sigmas, weights, beta, c, value_range, eps)
        self.sigmas = tuple(float(v) for v in sigmas)
        self.weights = None if weights is None else tuple(float(v) for v in weights)
        self.beta, self.c, self.eps = float(beta), float(c), float(eps)
        self.value_range = (float(value_range[0]), float(value_range[1]))
        self.bright = bool(bright)
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.vessel_dice(img1, img2, self.sigmas, self.weights, self.beta, self.c, self.eps, self.value_range, self.bright, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "sigmas={}, weights={}, beta={}, c={}, eps={}, value_range={}, bright={}, size_average={}".format(
            self.sigmas, self.weights, self.beta, self.c, self.eps, self.value_range, self.bright, self.size_average)


def vif(img1, img2, sigma_n_sq=2.0, value_range=(-1., 1.), size_average=True):
    """The pixel-domain visual information fidelity of ``img1`` (the image under test) against ``img2`` (the reference) with ``ssim``'s
    interface: the mean over the batch, or ``(N,)`` with ``size_average=False`` (``ops.vif``).  Not symmetric in its arguments."""
    return ops.vif(img1, img2, sigma_n_sq, value_range, not size_average)


class VIF(torch.nn.Module):
    """forward(img1, img2) -> the visual information fidelity in the pixel domain (VIFp; Sheikh & Bovik 2006) of ``img1``, the image under
    test, against ``img2``, the reference, with ``SSIM``'s interface: the Gaussian-channel information ``img1`` keeps about ``img2`` over
    the information ``img2`` itself carries, against the visual-noise floor ``sigma_n_sq`` (in 0..255 units of ``value_range``), at four
    scales.  NOT symmetric: an image that adds contrast the reference lacks can score above 1, a blurred one scores below 1; 1 up to
    rounding for identical images, so the loss is ``1 - VIF()(x, ref)``.  The mean over the batch, or ``(N,)`` with ``size_average=False``.
    fp32, grey planes, sides >= 41, no double backward (csrc/vif.hip)."""

    def __init__(self, sigma_n_sq=2.0, value_range=(-1., 1.), size_average=True):
        super().__init__()
        ops._vif_check_scalars(sigma_n_sq, value_range)
        self.sigma_n_sq = float(sigma_n_sq)
        self.value_range = (float(value_range[0]), float(value_range[1]))
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.vif(img1, img2, self.sigma_n_sq, self.value_range, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "sigma_n_sq={}, value_range={}, size_average={}".format(self.sigma_n_sq, self.value_range, self.size_average)


def cldice(img1, img2, iters=3, smooth=1.0, value_range=(-1., 1.), bright=True, size_average=True):
    """The soft-clDice index with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with ``size_average=False``
    (``ops.cldice``).  An index: the loss is ``1 - cldice(...)``."""
    return ops.cldice(img1, img2, iters, smooth, value_range, bright, not size_average)


class SoftSkeleton(torch.nn.Module):
    """forward(x) -> the soft skeleton of ``x`` ``(N, C, H, W)``, the shape of ``x`` (``ops.soft_skeleton``): ``iters`` rounds of min pooling
    over the 5-point cross, each followed by a 3 x 3 max pooling, keep what an opening removes (Shit et al., CVPR 2021).  ``iters`` in
    1..10.  Differentiable, with the tie rule of ``ops.soft_skeleton``; fp32, grey planes (csrc/cldice.hip)."""

    def __init__(self, iters=3, value_range=(-1., 1.), bright=True):
        super().__init__()
        ops._cldice_check_scalars(iters, value_range)
        self.iters = iters
        self.value_range = (float(value_range[0]), float(value_range[1]))
        self.bright = bool(bright)

    def forward(self, x):
        return ops.soft_skeleton(x, self.iters, self.value_range, self.bright)

    def extra_repr(self):
        return "iters={}, value_range={}, bright={}".format(self.iters, self.value_range, self.bright)


class SoftClDice(torch.nn.Module):
    """The soft centre-line Dice (soft-clDice; Shit et al., CVPR 2021) of two images: per image, the harmonic mean of
    ``Tprec = (sum skel(img1) u2 + smooth) / (sum skel(img1) + smooth)`` and ``Tsens = (sum skel(img2) u1 + smooth) / (sum skel(img2) + smooth)``,
    ``skel`` the ``SoftSkeleton`` and ``u`` the image mapped to [0, 1].  It rewards connected centre lines, not overlapping area: a
    capillary broken for a few pixels loses its skeleton there.  ``index(img1, img2, per_image)`` is the index ``S``; ``forward`` is the
    LOSS ``1 - S``, the mean over the batch or ``(N,)`` with ``size_average=False``.  ``iters`` in 1..10; fp32, grey planes, no double
    backward; on plateaus the gradient follows the tie rule of ``ops.cldice`` (csrc/cldice.hip)."""

    def __init__(self, iters=3, smooth=1.0, value_range=(-1., 1.), bright=True, size_average=True):
        super().__init__()
        ops._cldice_check_scalars(iters, value_range, smooth)
        self.iters = iters
        self.smooth = float(smooth)
        self.value_range = (float(value_range[0]), float(value_range[1]))
        self.bright = bool(bright)
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index ``S`` with ``per_image`` as given instead of ``not size_average``."""
        return ops.cldice(img1, img2, self.iters, self.smooth, self.value_range, self.bright, per_image)

    def forward(self, img1, img2):
        return 1 - self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "iters={}, smooth={}, value_range={}, bright={}, size_average={}".format(self.iters, self.smooth, self.value_range, self.bright,
                                                                                    self.size_average)


def frc(img1, img2, k_min=1, k_max=None, eps=1e-16, size_average=True):
    """The Fourier ring correlation index with ``ssim``'s interface: the mean over the batch, or ``(N,)`` with ``size_average=False``
    (``ops.frc``).  An index: the loss is ``1 - frc(...)``."""
    return ops.frc(img1, img2, k_min, k_max, eps, not size_average)


class FRC(torch.nn.Module):
    """forward(img1, img2) -> the Fourier ring correlation index (Saxton & Baumeister 1982; van Heel & Schatz 2005) with ``SSIM``'s
    interface: the correlation of the two spectra ring by ring, ``r_k = Nk / sqrt(Xk Yk + eps)`` from the ring means of
    ``Re(F conj G)``, ``|F|^2`` and ``|G|^2`` over the rings of ``radial_bins(H, W)``, averaged over the channels and the rings
    ``k_min..k_max`` of an image (``k_min = 1`` drops DC; ``k_max = None`` is the Nyquist ring ``min(H, W) // 2``).  It keeps phase
    and does not change under a gain on either image.  1 for identical images; the mean over the batch, or ``(N,)`` with
    ``size_average=False``; the loss is ``1 - FRC()(x, y)``, with gradients to both images.  A ring where either image has no power
    contributes 0.  fp32, sides 2..1024, no double backward (csrc/spectral.hip)."""

    def __init__(self, k_min=1, k_max=None, eps=1e-16, size_average=True):
        super().__init__()
        self.k_min, self.k_max, self.eps = ops.check_frc_params(k_min, k_max, eps)
        self.size_average = size_average

    def index(self, img1, img2, per_image):
        """The index with ``per_image`` as given instead of ``not size_average``."""
        return ops.frc(img1, img2, self.k_min, self.k_max, self.eps, per_image)

    def forward(self, img1, img2):
        return self.index(img1, img2, not self.size_average)

    def extra_repr(self):
        return "k_min={}, k_max={}, eps={}, size_average={}".format(self.k_min, self.k_max, self.eps, self.size_average)


class FRCResolution(torch.nn.Module):
    """The resolution read off the Fourier ring correlation curve: the fractional ring ``k*`` at which the curve of ``(img1, img2)``
    falls through ``threshold`` (a float in (0, 1), 1/7 after Nieuwenhuizen et al. 2013, or ``"half-bit"`` after van Heel & Schatz
    2005), after a moving average over ``smooth`` rings, searched in ``k_min..k_max`` (``ops.frc_cutoff``).
    ``index(img1, img2, per_image)`` is the cutoff frequency ``k* / min(H, W)`` in cycles per pixel, averaged over the channels:
    higher is better, so its batch mean in ``evaluate_pairs_with`` is meaningful; ``(N,)`` float64 with ``per_image``, else the
    batch mean.  ``curve(img1, img2)`` is the curve (N, C, K) and ``resolution(img1, img2)`` the resolution ``min(H, W) / k*`` in
    pixels, float64 (N, C) (inf where ``k* = 0``).  ``forward`` is ``index`` with the batch mean.  An evaluation read-out: no gradient."""

    def __init__(self, threshold=1 / 7, smooth=1, k_min=1, k_max=None, eps=1e-16):
        super().__init__()
        self.k_min, self.k_max, self.eps = ops.check_frc_params(k_min, k_max, eps)
        self.threshold, self.smooth = ops.check_frc_readout(threshold, smooth)

    def curve(self, img1, img2):
        return ops.frc_curve(img1, img2, self.eps)

    def cutoff(self, img1, img2):
        """``k*``, float64 (N, C)."""
        H, W = img1.shape[-2:]
        return ops.frc_cutoff(self.curve(img1, img2), H, W, self.threshold, self.smooth, self.k_min, self.k_max)

    def index(self, img1, img2, per_image):
        f = (self.cutoff(img1, img2) / min(img1.shape[-2:])).mean(1)
        return f if per_image else f.mean()

    def resolution(self, img1, img2):
        return min(img1.shape[-2:]) / self.cutoff(img1, img2)

    def forward(self, img1, img2):
        return self.index(img1, img2, False)

    def extra_repr(self):
        return "threshold={}, smooth={}, k_min={}, k_max={}, eps={}".format(self.threshold, self.smooth, self.k_min, self.k_max, self.eps)


class Registered(torch.nn.Module):
    """An index behind a sub-pixel registration: ``d = ops.phase_correlation(img1, img2, upsample, max_shift, k_max)`` (a constant:
    taken without gradient), ``img2' = ops.fourier_shift(img2, -d)``, both cropped by the static margin ``max_shift + 1`` on all four
    sides (the wrapped-around border never reaches the index, and no shape depends on data: capturable), then ``index.forward`` /
    ``index.index`` on the crops.  Every full-reference index here assumes registered pairs; this is the wrapper for pairs that are
    off by a pixel or so.  Gradients flow to ``img1`` and, through the shift's adjoint, to ``img2``.  ``index``: any module with
    ``forward(a, b)`` and ``index(a, b, per_image)``.  Sides must exceed ``2 (max_shift + 1)``."""

    def __init__(self, index, max_shift=8, upsample=10, k_max=None):
        super().__init__()
        if isinstance(max_shift, bool) or not isinstance(max_shift, int) or max_shift < 0:
            raise ValueError("Registered: max_shift must be an int >= 0, got %r" % (max_shift,))
        if isinstance(upsample, bool) or not isinstance(upsample, int) or not 1 <= upsample <= ops.PCORR_MAX_UPSAMPLE:
            raise ValueError("Registered: upsample must be an int in 1..%d, got %r" % (ops.PCORR_MAX_UPSAMPLE, upsample))
        if k_max is not None and (isinstance(k_max, bool) or not isinstance(k_max, int) or k_max < 0):
            raise ValueError("Registered: k_max must be None or an int >= 0, got %r" % (k_max,))
        self.wrapped = index
        self.max_shift, self.upsample, self.k_max = max_shift, upsample, k_max

    def shift(self, img1, img2):
        """``(shift (N, 2), peak (N,))`` of ``ops.phase_correlation`` with this module's settings."""
        m = self.max_shift + 1
        if img1.dim() != 4 or min(img1.shape[-2:]) <= 2 * m:
            raise ValueError("Registered: sides must exceed 2 (max_shift + 1) = %d, got %s" % (2 * m, tuple(img1.shape)))
        return ops.phase_correlation(img1, img2, self.upsample, self.max_shift, self.k_max)

    def register(self, img1, img2):
        """The registered, cropped pair the wrapped index sees."""
        d, _ = self.shift(img1, img2)
        m = self.max_shift + 1
        moved = ops.fourier_shift(img2, -d)
        return img1[..., m:-m, m:-m].contiguous(), moved[..., m:-m, m:-m].contiguous()

    def index(self, img1, img2, per_image=False):
        return self.wrapped.index(*self.register(img1, img2), per_image)

    def forward(self, img1, img2):
        return self.wrapped(*self.register(img1, img2))

    def extra_repr(self):
        return "max_shift={}, upsample={}, k_max={}".format(self.max_shift, self.upsample, self.k_max)


class RegistrationShift(torch.nn.Module):
    """The length in pixels of the translation between two images (``ops.phase_correlation``), with an index's interface so that an
    evaluation can report how far apart its pairs were: ``index(img1, img2, per_image)`` is ``|d|``, ``(N,)`` or the batch mean;
    ``forward`` the batch mean.  No gradient."""

    def __init__(self, max_shift=8, upsample=10, k_max=None):
        super().__init__()
        checked = Registered(None, max_shift, upsample, k_max)
        self.max_shift, self.upsample, self.k_max = checked.max_shift, checked.upsample, checked.k_max

    def index(self, img1, img2, per_image=False):
        d, _ = ops.phase_correlation(img1, img2, self.upsample, min(self.max_shift, min(img1.shape[-2:]) // 2), self.k_max)
        n = d.square().sum(1).sqrt()
        return n if per_image else n.mean()

    def forward(self, img1, img2):
        return self.index(img1, img2, False)

    def extra_repr(self):
        return "max_shift={}, upsample={}, k_max={}".format(self.max_shift, self.upsample, self.k_max)
