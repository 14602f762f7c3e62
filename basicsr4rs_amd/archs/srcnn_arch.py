"""SRCNN (basicsr/archs/srcnn_arch.py of the remote-sensing fork) on the HIP engine.

Bicubic upsampling of the LR image (align_corners=True) fused with the NCHW -> NHWC layout change,
then 9x9 (num_in_ch -> 64) + ReLU, 5x5 (64 -> 32) + ReLU, 5x5 (32 -> num_out_ch) on the k x k
convolution kernels (ops/convk.py); the output goes back to fp32 NCHW.  The module tree is the
reference's (``conv1`` / ``conv2`` / ``conv3``, plain ``nn.Conv2d`` with the default init), so its
state_dict loads here with ``strict_load_g``.
"""
from torch import nn as nn

from .. import _lib
from ..ops import conv as C
from ..ops import convk as K
from ..utils.registry import ARCH_REGISTRY


@ARCH_REGISTRY.register()
class SRCNN(nn.Module):

    def __init__(self, num_in_ch, num_out_ch, upscale=4):
        super().__init__()
        self.upscale = upscale
        self.num_in_ch, self.num_out_ch = num_in_ch, num_out_ch
        self.conv1 = nn.Conv2d(num_in_ch, 64, kernel_size=9, padding=4)
        self.conv2 = nn.Conv2d(64, 32, kernel_size=5, padding=2)
        self.conv3 = nn.Conv2d(32, num_out_ch, kernel_size=5, padding=2)

    def forward(self, x):
        h = K.bicubic_up(x, self.upscale, C.feature_dtype())
        h = K.convk(h, self.conv1, act=_lib.ACT_RELU)
        h = K.convk(h, self.conv2, act=_lib.ACT_RELU)
        h = K.convk(h, self.conv3)
        return C.to_nchw(h, self.num_out_ch)
