"""PSNR and SSIM as the reference's evaluation computes them (test.py:118-119): `psnr` is utils/image_utils.py:17-19
(a per-channel MSE, 20 log10(1 / sqrt(mse)) per channel, shape [C,1]; the caller takes the mean), `ssim` is
utils/loss_utils.py:23-63 (11 x 11 Gaussian window, sigma 1.5, zero padding, per channel, mean of the map).  Same
signatures.  Two fp32 device images of shape [3,H,W] (what the evaluation passes) run ONE fused kernel
(dgs_image_metrics: both metrics from one pass over the two images) -- `psnr_ssim` returns both from that one launch.
Everything else the reference's signatures accept -- CPU tensors, batches, other channel counts, another window,
size_average=False -- runs the torch expressions below on whatever device the tensors live on.
tests/golden/metrics_golden.npz pins both paths against the reference's own functions.

LPIPS, the third number the reference reports, is `lpips(x, y, weights)` (deblurgs_amd/lpips.py, re-exported here): the
operator is part of this package (dgs_lpips_alex), its network weights are the caller's.
"""
import ctypes
from math import exp

import torch
import torch.nn.functional as F

from . import _lib
from .lpips import lpips, lpips_layers  # noqa: F401  (the third metric of test.py:118-120)


def _gaussian(window_size, sigma):
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                         dtype=torch.float32)
    return gauss / gauss.sum()


def _window(window_size, channel):
    w1 = _gaussian(window_size, 1.5).unsqueeze(1)
    return w1.mm(w1.t()).float()[None, None].expand(channel, 1, window_size, window_size).contiguous()


def _ssim_torch(img1, img2, window_size, size_average):
    channel = img1.size(-3)
    window = _window(window_size, channel).to(img1.device).type_as(img1)
    pad = window_size // 2
    conv = lambda x: F.conv2d(x, window, padding=pad, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    if size_average:
        return ssim_map.mean()
    return ssim_map.mean(1).mean(1).mean(1)


def _psnr_torch(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def _fused_ok(a, b, window_size=11, size_average=True):
    return (a.device.type == "cuda" and b.device == a.device and a.dtype == torch.float32 and b.dtype == torch.float32
            and a.dim() == 3 and a.shape[0] == 3 and a.shape == b.shape and window_size == 11 and size_average)


def psnr_ssim(a, b):
    """Both metrics of two [3,H,W] fp32 device images from one launch: a device tensor [5] = (mean over the channels of
    the per-channel PSNR in dB, SSIM, the three per-channel PSNRs).  No host synchronisation."""
    if not _fused_ok(a, b):
        raise RuntimeError("psnr_ssim needs two [3,H,W] float32 tensors on the same HIP device")
    a, b = a.contiguous(), b.contiguous()
    L = _lib.lib()
    H, W = int(a.shape[1]), int(a.shape[2])
    tmp = torch.empty(L.dgs_image_metrics_tmp_bytes(W, H), dtype=torch.uint8, device=a.device)
    out = torch.empty(5, dtype=torch.float32, device=a.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
    _lib.check(L.dgs_image_metrics(a.data_ptr(), b.data_ptr(), W, H, tmp.data_ptr(), out.data_ptr(), st),
               "dgs_image_metrics")
    return out


def psnr(img1, img2):
    """[C,H,W] x 2 -> [C,1] dB per channel (utils/image_utils.py:17-19); the reference's callers take `.mean()`."""
    if _fused_ok(img1, img2):
        return psnr_ssim(img1, img2)[2:5].reshape(3, 1)
    return _psnr_torch(img1, img2)


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py:39-63.  [3,H,W] fp32 device images, the default window and size_average: the fused kernel."""
    if _fused_ok(img1, img2, window_size, size_average):
        return psnr_ssim(img1, img2)[1]
    return _ssim_torch(img1, img2, window_size, size_average)
