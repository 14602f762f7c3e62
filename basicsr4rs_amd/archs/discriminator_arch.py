"""Discriminators of SRGAN / ESRGAN / Real-ESRGAN (basicsr/archs/discriminator_arch.py) on the HIP engine.

VGGStyleDiscriminator (discriminator_arch.py:8-87):

The parameter modules are the reference's (``conv0_0`` ... ``conv4_1`` / ``conv5_1``, ``bn0_1`` ..., ``linear1``,
``linear2``), so the state-dict keys, shapes and default init are the reference's and a ``net_d_*.pth`` loads
strictly.  Forward: NCHW fp32 image -> NHWC (3 channels padded to 8) -> 3x3 convs (ops/conv.py; the LeakyReLU of
``conv0_0`` in its epilogue) and 4x4 stride-2 convs (ops/gan.py), BatchNorm + LeakyReLU(0.2) fused in one pass
after every conv but the first, then the two head linears on the flattened NHWC map (``linear1`` reads the
reference's NCHW-flatten weight through the kernel's index permutation).  Output [N, 1] fp32.

UNetDiscriminatorSN (discriminator_arch.py:91-150): the parameter modules are the reference's too, ``nn.Conv2d``
wrapped by ``torch.nn.utils.spectral_norm`` (keys ``weight_orig`` / ``weight_u`` / ``weight_v``, their init and load
hooks), but they are never called: the forward reads ``weight_orig``, ``weight_u``, ``weight_v`` and ``bias`` only.
All eight normalised weights come from one grouped launch sequence at the top of the forward
(ops/gan.py:spectral_norm_group), the convs run on them with per-call GEMM images, LeakyReLU(0.2) and the U-Net skips
sit in the conv epilogues, bilinear x2 is its own kernel, and ``conv9`` stores the fp32 NCHW map [N, 1, H, W].
"""
from torch import nn as nn
from torch.nn.utils import spectral_norm

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


@ARCH_REGISTRY.register()
class UNetDiscriminatorSN(nn.Module):
    """U-Net discriminator with spectral normalisation (Real-ESRGAN).

    Args:
        num_in_ch (int): Channel number of inputs.
        num_feat (int): Channel number of base intermediate features (a multiple of 8 up to 64). Default: 64.
        skip_connection (bool): Whether to use the U-Net skip connections. Default: True.
    """

    def __init__(self, num_in_ch, num_feat=64, skip_connection=True):
        super().__init__()
        if num_feat % 8 or num_feat * 8 > 512:
            raise ValueError(f'UNetDiscriminatorSN: num_feat must be a multiple of 8 up to 64, got {num_feat}')
        self.num_in_ch = num_in_ch
        self.skip_connection = skip_connection
        norm = spectral_norm
        self.conv0 = nn.Conv2d(num_in_ch, num_feat, kernel_size=3, stride=1, padding=1)
        self.conv1 = norm(nn.Conv2d(num_feat, num_feat * 2, 4, 2, 1, bias=False))
        self.conv2 = norm(nn.Conv2d(num_feat * 2, num_feat * 4, 4, 2, 1, bias=False))
        self.conv3 = norm(nn.Conv2d(num_feat * 4, num_feat * 8, 4, 2, 1, bias=False))
        self.conv4 = norm(nn.Conv2d(num_feat * 8, num_feat * 4, 3, 1, 1, bias=False))
        self.conv5 = norm(nn.Conv2d(num_feat * 4, num_feat * 2, 3, 1, 1, bias=False))
        self.conv6 = norm(nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1, bias=False))
        self.conv7 = norm(nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=False))
        self.conv8 = norm(nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(num_feat, 1, 3, 1, 1)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.num_in_ch:
            raise ValueError(f'UNetDiscriminatorSN takes NCHW images with {self.num_in_ch} channels, got {tuple(x.shape)}')
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f'UNetDiscriminatorSN: H and W must be multiples of 8, got {tuple(x.shape)}')
        if not x.is_cuda:
            raise NotImplementedError(G._CPU_MESSAGE)
        lrelu = dict(act=_lib.ACT_LRELU, slope=0.2)
        sn = [getattr(self, f'conv{i}') for i in range(1, 9)]
        # the power iterations depend on the weights alone: all eight at the top, one grouped launch sequence
        w = (None, ) + tuple(G.spectral_norm_group(sn, self.training))
        skip = (lambda t: t) if self.skip_connection else (lambda t: None)
        x0 = C.conv3x3(C.to_nhwc(x, C.pad8(self.num_in_ch), C.feature_dtype()), self.conv0, **lrelu)
        x1 = G.conv4s2(x0, self.conv1, weight=w[1], **lrelu)
        x2 = G.conv4s2(x1, self.conv2, weight=w[2], **lrelu)
        x3 = G.conv4s2(x2, self.conv3, weight=w[3], **lrelu)
        # the skip is added after the activation: the res / beta form of the conv epilogue
        x4 = C.conv3x3(G.bilinear_up2(x3), self.conv4, res=skip(x2), weight=w[4], cache=False, **lrelu)
        x5 = C.conv3x3(G.bilinear_up2(x4), self.conv5, res=skip(x1), weight=w[5], cache=False, **lrelu)
        x6 = C.conv3x3(G.bilinear_up2(x5), self.conv6, res=skip(x0), weight=w[6], cache=False, **lrelu)
        out = C.conv3x3(x6, self.conv7, weight=w[7], cache=False, **lrelu)
        out = C.conv3x3(out, self.conv8, weight=w[8], cache=False, **lrelu)
        return C.conv3x3(out, self.conv9, out_nchw=True)
