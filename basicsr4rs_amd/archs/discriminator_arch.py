"""VGG-style discriminator of SRGAN / ESRGAN (basicsr/archs/discriminator_arch.py:8-87) on the HIP engine.

The parameter modules are the reference's (``conv0_0`` ... ``conv4_1`` / ``conv5_1``, ``bn0_1`` ..., ``linear1``,
``linear2``), so the state-dict keys, shapes and default init are the reference's and a ``net_d_*.pth`` loads
strictly.  Forward: NCHW fp32 image -> NHWC (3 channels padded to 8) -> 3x3 convs (ops/conv.py; the LeakyReLU of
``conv0_0`` in its epilogue) and 4x4 stride-2 convs (ops/gan.py), BatchNorm + LeakyReLU(0.2) fused in one pass
after every conv but the first, then the two head linears on the flattened NHWC map (``linear1`` reads the
reference's NCHW-flatten weight through the kernel's index permutation).  Output [N, 1] fp32.
"""
from torch import nn as nn

from .. import _lib
from ..ops import conv as C
from ..ops import gan as G
from ..utils.registry import ARCH_REGISTRY


@ARCH_REGISTRY.register()
class VGGStyleDiscriminator(nn.Module):
    """VGG style discriminator with input size 128 x 128 or 256 x 256.

    Args:
        num_in_ch (int): Channel number of inputs.
        num_feat (int): Channel number of base intermediate features (a multiple of 8).
        input_size (int): 128 or 256.
    """

    def __init__(self, num_in_ch, num_feat, input_size=128):
        super().__init__()
        self.input_size = input_size
        assert self.input_size == 128 or self.input_size == 256, (
            f'input size must be 128 or 256, but received {input_size}')
        if num_feat % 8 or num_feat * 8 > 512:
            raise ValueError(f'VGGStyleDiscriminator: num_feat must be a multiple of 8 up to 64, got {num_feat}')
        self.num_in_ch = num_in_ch
        self.stages = 5 if input_size == 128 else 6
        mult = (1, 2, 4, 8, 8, 8)
        self.conv0_0 = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1, bias=True)
        self.conv0_1 = nn.Conv2d(num_feat, num_feat, 4, 2, 1, bias=False)
        self.bn0_1 = nn.BatchNorm2d(num_feat, affine=True)
        for s in range(1, self.stages):
            cin, cout = num_feat * mult[s - 1], num_feat * mult[s]
            setattr(self, f'conv{s}_0', nn.Conv2d(cin, cout, 3, 1, 1, bias=False))
            setattr(self, f'bn{s}_0', nn.BatchNorm2d(cout, affine=True))
            setattr(self, f'conv{s}_1', nn.Conv2d(cout, cout, 4, 2, 1, bias=False))
            setattr(self, f'bn{s}_1', nn.BatchNorm2d(cout, affine=True))
        self.linear1 = nn.Linear(num_feat * 8 * 4 * 4, 100)
        self.linear2 = nn.Linear(100, 1)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.num_in_ch:
            raise ValueError(f'VGGStyleDiscriminator takes NCHW images with {self.num_in_ch} channels, got {tuple(x.shape)}')
        assert x.size(2) == self.input_size and x.size(3) == self.input_size, (
            f'Input size must be identical to input_size, but received {x.size()}.')
        lrelu = _lib.ACT_LRELU
        feat = C.to_nhwc(x, C.pad8(self.num_in_ch), C.feature_dtype())
        feat = C.conv3x3(feat, self.conv0_0, act=lrelu, slope=0.2)
        feat = G.batch_norm_act(G.conv4s2(feat, self.conv0_1), self.bn0_1, lrelu, 0.2)
        for s in range(1, self.stages):
            feat = G.batch_norm_act(C.conv3x3(feat, getattr(self, f'conv{s}_0')), getattr(self, f'bn{s}_0'), lrelu, 0.2)
            feat = G.batch_norm_act(G.conv4s2(feat, getattr(self, f'conv{s}_1')), getattr(self, f'bn{s}_1'), lrelu, 0.2)
        # spatial size (4, 4): the NHWC map flattened; linear1 permutes to the reference's NCHW flatten
        n, h, w, c = feat.shape
        feat = G.linear(feat.reshape(n, h * w * c), self.linear1, lrelu, 0.2, spatial=h * w)
        return G.linear(feat, self.linear2)
