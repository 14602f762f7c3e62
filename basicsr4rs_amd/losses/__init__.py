"""Loss registry surface (mirror of basicsr/losses/__init__.py:19-31)."""
from copy import deepcopy

from ..utils.registry import LOSS_REGISTRY
from .basic_loss import CharbonnierLoss, L1Loss, MSELoss, PerceptualLoss, WeightedTVLoss
from .align_loss import EncoderLoss, RegisteredLoss, ShiftConv2d, lanczos_kernel
from .gan_loss import GANLoss, MultiScaleGANLoss

__all__ = ['build_loss', 'L1Loss', 'MSELoss', 'CharbonnierLoss', 'WeightedTVLoss', 'PerceptualLoss', 'GANLoss',
           'MultiScaleGANLoss', 'RegisteredLoss', 'EncoderLoss', 'ShiftConv2d', 'lanczos_kernel']


def build_loss(opt):
    opt = deepcopy(opt)
    loss_type = opt.pop('type')
    return LOSS_REGISTRY.get(loss_type)(**opt)
