"""ECBSR (basicsr/archs/ecbsr_arch.py; "Edge-oriented Convolution Block for Real-time Super Resolution on
Mobile Devices") on the HIP engine.

The module tree, parameter names, shapes and default initialisation are the reference's -- every ECB block keeps
its ``conv3x3``, ``conv1x1_3x3`` (``k0 / b0 / k1 / b1``), the three edge branches ``conv1x1_sbx / _sby / _lpl``
(``k0 / b0 / scale / bias`` and the fixed ``mask``, a parameter with ``requires_grad=False``) and ``act.weight`` --
so reference checkpoints load strictly and checkpoints trained here load there.  What differs is how a step runs:
``train()`` and ``eval()`` both go through the collapsed single-conv form of every block, re-collapsed on the
device each step (ops/ecb.py).
"""
import torch
from torch import nn as nn

from ..ops import ecb as E
from ..utils.registry import ARCH_REGISTRY

SEQ_TYPES = ('conv1x1-conv3x3', 'conv1x1-sobelx', 'conv1x1-sobely', 'conv1x1-laplacian')
ACT_TYPES = ('prelu', 'relu', 'linear')
_SOBEL_X = [[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]]
_MASKS = {
    'conv1x1-sobelx': _SOBEL_X,
    'conv1x1-sobely': [list(col) for col in zip(*_SOBEL_X)],
    'conv1x1-laplacian': [[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]],
}


class SeqConv3x3(nn.Module):
    """A 1x1 conv followed by a 3x3 conv (free, or a fixed edge mask times a learnt per-channel scale), the 1x1
    output padded with its own bias.  Holds the parameters only: the arithmetic is the enclosing block's collapse."""

    def __init__(self, seq_type, in_channels, out_channels, depth_multiplier=1):
        super().__init__()
        if seq_type not in SEQ_TYPES:
            raise ValueError(f'SeqConv3x3: seq_type must be one of {SEQ_TYPES}, got {seq_type!r}')
        self.seq_type, self.in_channels, self.out_channels = seq_type, in_channels, out_channels
        if seq_type == 'conv1x1-conv3x3':
            self.mid_planes = int(out_channels * depth_multiplier)
            squeeze = nn.Conv2d(in_channels, self.mid_planes, kernel_size=1)
            self.k0, self.b0 = squeeze.weight, squeeze.bias
            expand = nn.Conv2d(self.mid_planes, out_channels, kernel_size=3)
            self.k1, self.b1 = expand.weight, expand.bias
        else:
            squeeze = nn.Conv2d(in_channels, out_channels, kernel_size=1)
            self.k0, self.b0 = squeeze.weight, squeeze.bias
            self.scale = nn.Parameter(torch.randn(out_channels, 1, 1, 1) * 1e-3)
            self.bias = nn.Parameter(torch.randn(out_channels) * 1e-3)
            mask = torch.tensor(_MASKS[seq_type], dtype=torch.float32).expand(out_channels, 1, 3, 3).contiguous()
            self.mask = nn.Parameter(mask, requires_grad=False)

    def forward(self, x):
        raise NotImplementedError('SeqConv3x3 holds parameters only; the ECB block runs its collapsed form')


class ECB(nn.Module):
    """Edge-oriented convolution block: conv3x3 + four SeqConv3x3 branches (+ identity), then the activation."""

    def __init__(self, in_channels, out_channels, depth_multiplier, act_type='prelu', with_idt=False):
        super().__init__()
        if act_type not in ACT_TYPES:
            raise ValueError(f'ECB: act_type {act_type!r} is not supported on the collapsed HIP path; supported: '
                             f'{", ".join(ACT_TYPES)}')
        self.depth_multiplier = depth_multiplier
        self.in_channels, self.out_channels = in_channels, out_channels
        self.act_type = act_type
        self.with_idt = bool(with_idt and in_channels == out_channels)
        self.conv3x3 = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1)
        self.conv1x1_3x3 = SeqConv3x3('conv1x1-conv3x3', in_channels, out_channels, depth_multiplier)
        self.conv1x1_sbx = SeqConv3x3('conv1x1-sobelx', in_channels, out_channels)
        self.conv1x1_sby = SeqConv3x3('conv1x1-sobely', in_channels, out_channels)
        self.conv1x1_lpl = SeqConv3x3('conv1x1-laplacian', in_channels, out_channels)
        if act_type == 'prelu':
            self.act = nn.PReLU(num_parameters=out_channels)
        elif act_type == 'relu':
            self.act = nn.ReLU(inplace=True)

    def rep_params(self):
        """The collapsed fp32 (rep_weight [Cout, Cin, 3, 3], rep_bias [Cout]), computed on the device."""
        return E.rep_params(self)

    def forward(self, x):
        raise NotImplementedError('an ECB block runs inside ECBSR (ops/ecb.py: one autograd node for the whole net)')


@ARCH_REGISTRY.register()
class ECBSR(nn.Module):

    def __init__(self, num_in_ch, num_out_ch, num_block, num_channel, with_idt, act_type, scale):
        super().__init__()
        if num_in_ch != 1 and num_in_ch != num_out_ch:
            raise ValueError('ECBSR: the shortcut needs num_in_ch == 1 or num_in_ch == num_out_ch')
        self.num_in_ch, self.scale = num_in_ch, scale
        blocks = [ECB(num_in_ch, num_channel, depth_multiplier=2.0, act_type=act_type, with_idt=with_idt)]
        blocks += [ECB(num_channel, num_channel, depth_multiplier=2.0, act_type=act_type, with_idt=with_idt)
                   for _ in range(num_block)]
        blocks.append(ECB(num_channel, num_out_ch * scale * scale, depth_multiplier=2.0, act_type='linear',
                          with_idt=with_idt))
        self.backbone = nn.Sequential(*blocks)
        self.upsampler = nn.PixelShuffle(scale)

    def forward(self, x):
        return E.ecbsr_forward(self, list(self.backbone), x, self.scale)
