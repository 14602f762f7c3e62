"""``DiffJPEG`` (basicsr/utils/diffjpeg.py:449-491) as one HIP kernel (csrc/degrade.hip: jpeg_kernel).  Forward only."""
import torch

from ..ops import degrade as D


def quality_to_factor(quality):
    """The quantisation-table factor of a JPEG quality (diffjpeg.py:32-45)."""
    if quality < 50:
        quality = 5000. / quality
    else:
        quality = 200. - quality * 2
    return quality / 100.


class DiffJPEG(torch.nn.Module):
    """``forward(x, quality)``: x [B, 3, H, W] in [0, 1] (the clamp is the caller's, as in the reference); quality a
    Python number or a [B] device tensor.  The tensor is only read: the reference overwrites it with the factors,
    this module does not.  ``differentiable=True`` uses the rounding r + (v - r)^3 in the forward; there is no
    backward."""

    def __init__(self, differentiable=True):
        super().__init__()
        self.differentiable = bool(differentiable)

    def forward(self, x, quality):
        return D.jpeg(x, quality, self.differentiable)
