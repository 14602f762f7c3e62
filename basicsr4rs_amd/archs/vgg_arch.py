"""VGG feature extractor of the perceptual loss (basicsr/archs/vgg_arch.py) on the HIP engine.

The module tree is defined here (no torchvision): ``vgg_net.<name>`` holds an ``nn.Conv2d(cin, cout, 3, 1, 1)``
per conv layer up to the deepest requested one, so the state-dict keys are ``vgg_net.conv1_1.weight`` ...,
plus the buffers ``mean`` and ``std`` with ``use_input_norm``.  Weights are never downloaded: they are read
from ``pretrain_path``, else ``$BASICSR4RS_VGG_WEIGHTS``, else ``experiments/pretrained_models/vgg19-dcbb9e9d.pth``,
as a torchvision state dict (``features.<i>.weight``) or this module's own keys; ``pretrained=False`` keeps
torch's default init.

Forward: ``range_norm`` and ``use_input_norm`` fold into the one affine of the NCHW -> NHWC head (3 channels
padded to 8), then 3x3 convs with the ReLU fused in the epilogue and the max-pool kernel (ops/perceptual.py).
A tapped ``convX_Y`` is the pre-ReLU map (the reference clones before torchvision's in-place ReLU), so that
conv runs without the fused ReLU and the ReLU is a pass of its own.  Features stay NHWC in the compute
dtype; ``to_nchw=True`` returns NCHW fp32.
"""
import os
from collections import OrderedDict

import torch
from torch import nn as nn

from .. import _lib
from ..ops import conv as C
from ..ops import perceptual as P
from ..utils.registry import ARCH_REGISTRY

VGG_PRETRAIN_PATH = 'experiments/pretrained_models/vgg19-dcbb9e9d.pth'
VGG_WEIGHTS_ENV = 'BASICSR4RS_VGG_WEIGHTS'

# conv layers per stage (between two pools) and the output channels of the stages
_STAGE_CONVS = {'vgg11': (1, 1, 2, 2, 2), 'vgg13': (2, 2, 2, 2, 2), 'vgg16': (2, 2, 3, 3, 3), 'vgg19': (2, 2, 4, 4, 4)}
_STAGE_CHANNELS = (64, 128, 256, 512, 512)


def _names(stage_convs):
    names = []
    for s, n in enumerate(stage_convs, 1):
        for i in range(1, n + 1):
            names += [f'conv{s}_{i}', f'relu{s}_{i}']
        names.append(f'pool{s}')
    return names


# layer names in torchvision's ``features`` order: NAMES[vgg_type][i] is the name of ``features.<i>``
NAMES = {k: _names(v) for k, v in _STAGE_CONVS.items()}


def conv_channels(name):
    """(cin, cout) of conv layer ``convS_I``."""
    s, i = (int(v) for v in name[4:].split('_'))
    cout = _STAGE_CHANNELS[s - 1]
    cin = cout if i > 1 else (3 if s == 1 else _STAGE_CHANNELS[s - 2])
    return cin, cout


def find_weights(pretrain_path=None):
    """The weight file to read and the three places looked at (for the error message)."""
    places = [f'pretrain_path ({pretrain_path})', f'${VGG_WEIGHTS_ENV} ({os.environ.get(VGG_WEIGHTS_ENV) or "unset"})',
              VGG_PRETRAIN_PATH]
    if pretrain_path:
        return (pretrain_path if os.path.exists(pretrain_path) else None), places
    env = os.environ.get(VGG_WEIGHTS_ENV)
    if env:
        return (env if os.path.exists(env) else None), places
    return (VGG_PRETRAIN_PATH if os.path.exists(VGG_PRETRAIN_PATH) else None), places


@ARCH_REGISTRY.register()
class VGGFeatureExtractor(nn.Module):
    """VGG11/13/16/19 up to the deepest layer of ``layer_name_list``; forward returns {name: feature}.

    Reference arguments (vgg_arch.py:78-85) plus ``pretrain_path`` (a weight file) and ``pretrained``
    (False: no file is read, the convs keep torch's default init)."""

    def __init__(self,
                 layer_name_list,
                 vgg_type='vgg19',
                 use_input_norm=True,
                 range_norm=False,
                 requires_grad=False,
                 remove_pooling=False,
                 pooling_stride=2,
                 pretrain_path=None,
                 pretrained=True):
        super().__init__()
        if 'bn' in vgg_type:
            raise NotImplementedError(f'{vgg_type}: the batch-norm VGG variants are not supported')
        if vgg_type not in NAMES:
            raise ValueError(f'unknown vgg_type {vgg_type}; supported: {sorted(NAMES)}')
        if pooling_stride not in (1, 2):
            raise ValueError(f'pooling_stride {pooling_stride} is not supported (1 or 2)')
        self.layer_name_list = list(layer_name_list)
        self.vgg_type = vgg_type
        self.use_input_norm = use_input_norm
        self.range_norm = range_norm
        self.pooling_stride = pooling_stride
        self.names = NAMES[vgg_type]
        for v in self.layer_name_list:
            if v not in self.names:
                raise ValueError(f'{v} is not a layer of {vgg_type}')
        if not self.layer_name_list:
            raise ValueError('layer_name_list is empty')
        max_idx = max(self.names.index(v) for v in self.layer_name_list)
        # the layers that run, in order; only the convs are modules (ReLU and pooling have no state)
        self.layers = [n for n in self.names[:max_idx + 1] if not (remove_pooling and n.startswith('pool'))]
        self.vgg_net = nn.Sequential(
            OrderedDict((n, nn.Conv2d(*conv_channels(n), 3, 1, 1)) for n in self.layers if n.startswith('conv')))
        if pretrained:
            path, places = find_weights(pretrain_path)
            if path is None:
                raise FileNotFoundError('VGGFeatureExtractor: no pretrained weight file (nothing is downloaded); '
                                        'looked at ' + ', '.join(places))
            self.load_vgg_weights(torch.load(path, map_location='cpu', weights_only=True))
        if use_input_norm:
            # for images in [0, 1]
            self.register_buffer('mean', torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer('std', torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        if not requires_grad:
            self.vgg_net.eval()
        else:
            self.vgg_net.train()
        for p in self.parameters():
            p.requires_grad = bool(requires_grad)
        self._affine_cache = None

    def load_vgg_weights(self, state):
        """Copy conv weights from a torchvision VGG state dict (``features.<i>.weight/bias``; classifier keys
        and layers past the truncation ignored) or from this module's own keys."""
        if any(k.startswith('features.') for k in state):
            mapped = {}
            for k, v in state.items():
                part = k.split('.')
                if part[0] != 'features':
                    continue
                idx = int(part[1])
                if idx < len(self.names) and self.names[idx] in self.vgg_net._modules:
                    mapped[f'{self.names[idx]}.{part[2]}'] = v
        else:
            mapped = {k[len('vgg_net.'):]: v for k, v in state.items() if k.startswith('vgg_net.')}
        own = self.vgg_net.state_dict()
        missing = [k for k in own if k not in mapped]
        if missing:
            raise KeyError(f'VGG weight file lacks {missing[:4]}{" ..." if len(missing) > 4 else ""} for {self.vgg_type}')
        for k, t in own.items():
            if tuple(mapped[k].shape) != tuple(t.shape):
                raise ValueError(f'VGG weight {k}: shape {tuple(mapped[k].shape)} in the file, {tuple(t.shape)} expected '
                                 f'(is the file a {self.vgg_type}?)')
        self.vgg_net.load_state_dict({k: mapped[k] for k in own})

    def _affine(self):
        """(shift, scale) of the head, y = (x - shift) * scale, for range_norm then use_input_norm."""
        if not self.use_input_norm:
            if not self.range_norm:
                return None, None
            dev = self.vgg_net.conv1_1.weight.device
            key = (dev, )
            if self._affine_cache is None or self._affine_cache[0] != key:
                self._affine_cache = (key, C.vec([-1.0] * 3, dev), C.vec([0.5] * 3, dev))
            return self._affine_cache[1:]
        key = (self.mean.device, self.mean.data_ptr(), self.mean._version, self.std.data_ptr(), self.std._version)
        if self._affine_cache is None or self._affine_cache[0] != key:
            mean, std = self.mean.detach().reshape(-1).float(), self.std.detach().reshape(-1).float()
            if self.range_norm:  # ((x + 1) / 2 - mean) / std
                shift, scale = 2.0 * mean - 1.0, 0.5 / std
            else:
                shift, scale = mean.clone(), 1.0 / std
            self._affine_cache = (key, shift.contiguous(), scale.contiguous())
        return self._affine_cache[1:]

    def forward(self, x, to_nchw=False):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'VGGFeatureExtractor takes NCHW images with 3 channels, got shape {tuple(x.shape)}')
        shift, scale = self._affine()
        h = C.to_nhwc(x, 8, C.feature_dtype(), shift, scale)
        taps = self.layer_name_list
        output = OrderedDict()
        layers = self.layers
        i = 0
        while i < len(layers):
            name = layers[i]
            if name.startswith('conv'):
                conv = self.vgg_net._modules[name]
                fuse = name not in taps and i + 1 < len(layers) and layers[i + 1].startswith('relu')
                if fuse:
                    h = C.conv3x3(h, conv, act=_lib.ACT_RELU)
                    i += 1
                    name = layers[i]
                else:
                    h = C.conv3x3(h, conv)
            elif name.startswith('relu'):
                h = P.relu(h)
            else:
                h = P.max_pool2(h, self.pooling_stride)
            if name in taps:
                output[name] = C.to_nchw(h, h.shape[-1]) if to_nchw else h
            i += 1
        return output
