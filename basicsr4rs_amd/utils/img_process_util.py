"""``filter2D`` and ``USMSharp`` (basicsr/utils/img_process_util.py:7-31, 63-83) on the HIP kernels of
csrc/degrade.hip.  The numpy ``usm_sharp`` (cv2) is not provided."""
import torch

from ..ops import degrade as D


def filter2D(img, kernel):
    """Reflect-padded correlation of ``img`` (b, c, h, w) with ``kernel`` (b, k, k) per sample, or (1, k, k) shared."""
    if kernel.size(-1) % 2 == 0:
        raise ValueError('Wrong kernel size')
    return D.filter2d(img, kernel)


class USMSharp(torch.nn.Module):
    """Unsharp masking.  The buffer ``kernel`` [1, radius, radius] is the reference's (the outer product of the 1-D
    Gaussian of ``cv2.getGaussianKernel(radius, sigma)``), kept so that state dicts match; the forward runs the two
    1-D passes of its factor ``taps`` instead of the dense radius x radius convolution."""

    def __init__(self, radius=50, sigma=0):
        super().__init__()
        if radius % 2 == 0:
            radius += 1
        self.radius = radius
        taps = D.gaussian_taps(radius, sigma)
        self.register_buffer('kernel', torch.outer(taps, taps).float().unsqueeze_(0))
        self.register_buffer('taps', taps.float(), persistent=False)

    def forward(self, img, weight=0.5, threshold=10):
        return D.usm_sharp(img, self.taps, weight, threshold)
