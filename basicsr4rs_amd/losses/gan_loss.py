"""GAN losses (mirror of basicsr/losses/gan_loss.py:10-140).

``GANLoss(gan_type)`` with 'vanilla' | 'lsgan' | 'wgan' | 'wgan_softplus' | 'hinge': on the device the mean loss
and its gradient come from one streaming pass (sr_gan_loss of csrc/loss.hip through ops/gan.py); CPU tensors take
the reference's formulas in plain torch, so the host suite can check them.  ``loss_weight`` applies to generators
only.  The gradient penalties of the reference (r1_penalty, g_path_regularize, gradient_penalty_loss) need a
double backward through the HIP ops and are not provided.
"""
import torch
from torch import nn as nn
from torch.nn import functional as F

from ..ops import gan as G
from ..utils.registry import LOSS_REGISTRY


def _torch_gan_loss(gan_type, input, target_is_real, is_disc, real_label_val, fake_label_val):
    """gan_loss.py:89-109 in torch ops (without the loss weight)."""
    if gan_type == 'hinge':
        if is_disc:
            input = -input if target_is_real else input
            return F.relu(1 + input).mean()
        return -input.mean()
    if gan_type == 'wgan':
        return -input.mean() if target_is_real else input.mean()
    if gan_type == 'wgan_softplus':
        return F.softplus(-input).mean() if target_is_real else F.softplus(input).mean()
    target = input.new_ones(input.size()) * (real_label_val if target_is_real else fake_label_val)
    if gan_type == 'vanilla':
        return F.binary_cross_entropy_with_logits(input, target)
    return F.mse_loss(input, target)


@LOSS_REGISTRY.register()
class GANLoss(nn.Module):
    """Define GAN loss.

    Args:
        gan_type (str): 'vanilla', 'lsgan', 'wgan', 'wgan_softplus' or 'hinge'.
        real_label_val (float): The value for real label. Default: 1.0.
        fake_label_val (float): The value for fake label. Default: 0.0.
        loss_weight (float): Loss weight, for generators only (always 1.0 for discriminators). Default: 1.0.
    """

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
        super().__init__()
        if gan_type not in G.GAN_KINDS:
            raise NotImplementedError(f'GAN type {gan_type} is not implemented.')
        self.gan_type = gan_type
        self.loss_weight = loss_weight
        self.real_label_val = real_label_val
        self.fake_label_val = fake_label_val

    def forward(self, input, target_is_real, is_disc=False):
        """input: the prediction (any shape); target_is_real: bool; is_disc: the loss is a discriminator's.
        Returns a 0-dim tensor."""
        if input.is_cuda:
            return G.gan_loss(input, self.gan_type, target_is_real, is_disc, self.real_label_val, self.fake_label_val,
                              self.loss_weight)
        loss = _torch_gan_loss(self.gan_type, input, target_is_real, is_disc, self.real_label_val, self.fake_label_val)
        return loss if is_disc else loss * self.loss_weight


@LOSS_REGISTRY.register()
class MultiScaleGANLoss(GANLoss):
    """GANLoss over a list of predictions, or a list of lists (then the last of each), averaged."""

    def forward(self, input, target_is_real, is_disc=False):
        if isinstance(input, list):
            loss = 0
            for pred_i in input:
                if isinstance(pred_i, list):
                    # only the last layer, in case of multiscale feature matching
                    pred_i = pred_i[-1]
                loss = loss + super().forward(pred_i, target_is_real, is_disc).mean()
            return loss / len(input)
        return super().forward(input, target_is_real, is_disc)
