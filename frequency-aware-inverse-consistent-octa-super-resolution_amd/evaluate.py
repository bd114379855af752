"""Inference / evaluation path of the reference (utils.py:182-242 `eval`, `eval_6m`), on the device.

``super_resolve`` is the reference's inference recipe (utils.py:202-205): frequency split with radii (10, 8), generator forward
in eval mode.  `model.eval()` turns every BatchNorm2d into a per-channel affine map; the forward folds it into the preceding
convolution's weights (``faoctasr_bn_fold``), so the inference generator is convolutions + activations only.
``image_metrics`` / ``evaluate_pairs`` score outputs with the four skimage metrics of utils.py:209-212 -- PSNR, SSIM (7x7 uniform
window), MSE, NMI (100 x 100 joint histogram) -- computed by HIP kernels (``faoctasr_eval_metrics``); the reference copies every
image to the host for skimage.  Only the N x 4 results travel.  Dataset / PNG IO is out of scope: the caller supplies tensors.
"""
import torch

from . import _lib, ops
from ._lib import call, ptr, stream_ptr


@torch.no_grad()
def super_resolve(model, lr_img, r_hp=10, r_lp=8):
    """lr_img (B,1,H,W) in [-1,1] -> super-resolved (B,1,H,W).  Leaves the model in eval mode, as utils.eval does."""
    model.eval()
    hf, lf = ops.freq_split(lr_img, r_hp, r_lp)
    return model(lf, hf)[2]


@torch.no_grad()
def image_metrics(y, gt, data_range=2.0, bins=100, cw_ssim=None):
    """y, gt: (N,1,H,W) or (N,H,W) device tensors -> float64 tensor (N,4) on the device: PSNR, SSIM, MSE, NMI per image pair
    (skimage.metrics.peak_signal_noise_ratio(data_range=2) / structural_similarity / mean_squared_error /
    normalized_mutual_information with their defaults, utils.py:209-212).  ``cw_ssim``: a ``wavelets.CWSSIM`` module; the result
    is then (N,5), the fifth column the module's per-image complex-wavelet index, which unlike SSIM hardly moves under a
    one-pixel misregistration of the pair.  Every sum has a fixed order: two calls on the same images agree bit for bit."""
    y, gt = ops._c(y), ops._c(gt)
    if y.shape != gt.shape:
        raise _lib.KernelError("image_metrics: shapes differ: %s vs %s" % (tuple(y.shape), tuple(gt.shape)))
    if y.dim() == 4:
        if y.shape[1] != 1:
            raise _lib.KernelError("image_metrics: single-channel images expected")
        N, _, H, W = y.shape
    else:
        N, H, W = y.shape
    out = torch.empty((N, 4), dtype=torch.float64, device=y.device)
    nbytes = _lib.load().faoctasr_eval_workspace_bytes(N, bins)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=y.device)
    call("eval_metrics", ptr(y), ptr(gt), out.data_ptr(), ws.data_ptr(), N, H, W, float(data_range), int(bins), stream_ptr())
    if cw_ssim is not None:
        out = torch.cat((out, cw_ssim.index(y.reshape(N, 1, H, W), gt.reshape(N, 1, H, W), True).double().reshape(N, 1)), dim=1)
    return out


def evaluate_pairs_with(model, pairs, cw_ssim=None, **indices):
    """``evaluate_pairs`` with any number of further full-reference indices: every keyword names a module with
    ``index(a, b, per_image)`` (``ssim.MSSSIM``, ``ssim.HaarPSI``) and adds a key of that name, in keyword order, behind the four
    metrics and "cw_ssim": the mean of the module's per-image index of ``(super_resolve(lr), hr)``.  A keyword given as None adds
    nothing.  ``evaluate_pairs_with(model, pairs, haarpsi=HaarPSI())`` returns the keys psnr, ssim, mse, nmi, haarpsi.  The keyword is
    the key: any name is taken, so a value that is no index module (no callable ``index``, or a string or sequence, whose ``index``
    is something else) and a name that is already a key raise ``TypeError`` / ``ValueError`` before anything runs."""
    indices = {k: mod for k, mod in indices.items() if mod is not None}
    for k, mod in indices.items():
        if isinstance(mod, (str, bytes, list, tuple)) or not callable(getattr(mod, "index", None)):
            raise TypeError("%s must be a module with index(a, b, per_image), got %r" % (k, mod))
        if k in ("psnr", "ssim", "mse", "nmi", "cw_ssim"):
            raise ValueError("%r is a key of the result already" % k)
    keys = ("psnr", "ssim", "mse", "nmi") + (("cw_ssim",) if cw_ssim is not None else ()) + tuple(indices)
    acc, n = None, 0
    for lr, hr in pairs:
        sr = super_resolve(model, lr)
        m = image_metrics(sr, hr, cw_ssim=cw_ssim).sum(0)
        for mod in indices.values():
            with torch.no_grad():
                m = torch.cat((m, mod.index(sr, hr, True).double().sum(0, keepdim=True)))
        acc = m if acc is None else acc + m
        n += lr.shape[0]
    if acc is None:
        return dict.fromkeys(keys, 0.0)
    vals = (acc / n).tolist()
    return dict(zip(keys, vals))


def evaluate_pairs(model, pairs, cw_ssim=None, ms_ssim=None):
    """pairs: iterable of (lr (B,1,H,W), hr (B,1,H,W)) device tensors.  Returns mean PSNR / SSIM / MSE / NMI like the print at
    utils.py:214,242; one host read at the end.  With a ``wavelets.CWSSIM`` module as ``cw_ssim`` also the key "cw_ssim"; with an
    ``ssim.MSSSIM`` module as ``ms_ssim`` also the key "ms_ssim", the mean of the module's per-image multi-scale index of
    ``(super_resolve(lr), hr)``.  Further indices (``ssim.HaarPSI``): ``evaluate_pairs_with``."""
    return evaluate_pairs_with(model, pairs, cw_ssim=cw_ssim, ms_ssim=ms_ssim)
