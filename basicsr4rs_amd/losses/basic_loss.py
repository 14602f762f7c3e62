"""Pixel losses (mirror of basicsr/losses/basic_loss.py:12-143, loss_util.py:6-96).

L1Loss with reduction 'mean'/'sum' and no weight map — the configuration of every SR
train YAML on the hot path (e.g. options/train/EDSR/train_EDSR_Lx4.yml ``pixel_opt``) — is
one fused HIP reduction that also writes the gradient (sr_l1_loss).  Everything else of the
family — MSELoss, CharbonnierLoss, a per-pixel weight map ([N,1,H,W] or [N,C,H,W]),
reduction='none', bf16 predictions, WeightedTVLoss — runs on the streaming kernels of
csrc/loss.hip (sr_pixel_loss): one pass over pred / target that writes the gradient, plus a
weight-sum pass for the weighted mean.  Only a weight map that itself requires grad, or one of
another shape, goes through plain torch ops with the reference's formula.

PerceptualLoss (basic_loss.py:147-253): VGG features of both images (archs/vgg_arch.py), the criterion on
the NHWC feature arrays through sr_pixel_loss, the style term on the Gram matrices of ops/perceptual.py.
"""
import torch
from torch import nn as nn

from .. import _lib
from ..archs.vgg_arch import VGGFeatureExtractor
from ..ops import perceptual as P
from ..utils.registry import LOSS_REGISTRY

_reduction_modes = ['none', 'mean', 'sum']
_REDUCE = {'none': _lib.REDUCE_NONE, 'mean': _lib.REDUCE_MEAN, 'sum': _lib.REDUCE_SUM}
_CPU_MESSAGE = 'basicsr4rs_amd losses run on the MI355X device'


class _L1Fused(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pred, target, loss_weight, mean):
        pred = pred.float().contiguous()
        target = target.float().contiguous()
        # sr_l1_loss reads 16-byte vectors: a contiguous view at an odd storage offset (buf[1:1 + n]) is
        # copied to an aligned buffer; aligned inputs, the hot path, are passed as they are
        if pred.data_ptr() % 16:
            pred = pred.clone()
        if target.data_ptr() % 16:
            target = target.clone()
        lib = _lib.load()
        n = pred.numel()
        ws_bytes = lib.sr_l1_loss_workspace(n)
        ws = torch.empty(ws_bytes // 4 + 1, device=pred.device, dtype=torch.float32)
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        grad = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        _lib.check(
            lib.sr_l1_loss(_lib.ptr(pred), _lib.ptr(target), n, float(loss_weight), int(mean), _lib.ptr(loss),
                           _lib.ptr(grad), _lib.ptr(ws), ws_bytes, _lib.stream()))
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad, ) = ctx.saved_tensors
        return grad * g, None, None, None


class _PixelLossFused(torch.autograd.Function):
    """sr_pixel_loss: the loss (a fp32 scalar, or the elementwise map of reduction 'none' in pred's
    dtype) and d loss / d pred from one pass; d loss / d target is its negation."""

    @staticmethod
    def forward(ctx, pred, target, weight, kind, reduction, loss_weight, eps):
        if pred.dtype not in (torch.float32, torch.bfloat16):
            pred = pred.float()
        if target.dtype != torch.float32 and target.dtype != pred.dtype:
            target = target.float()
        pred, target = pred.contiguous(), target.contiguous()
        if weight is not None:
            weight = weight.detach().float().contiguous()
        lib = _lib.load()
        # without a weight map the layout does not matter: any shape is one row of numel() elements
        N, C, H, W = pred.shape if pred.dim() == 4 else (1, 1, 1, pred.numel())
        ws_bytes = lib.sr_pixel_loss_workspace(pred.numel())
        ws = torch.empty(ws_bytes // 8 + 1, device=pred.device, dtype=torch.float64)
        none = reduction == 'none'
        loss = None if none else torch.empty((), device=pred.device, dtype=torch.float32)
        out = torch.empty_like(pred) if none else None
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        grad = torch.empty_like(pred) if need else None
        _lib.check(
            lib.sr_pixel_loss(kind, _REDUCE[reduction], _lib.dtype_code(pred.dtype), _lib.dtype_code(target.dtype),
                              _lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight),
                              0 if weight is None else weight.size(1), N, C, H, W, float(loss_weight), float(eps),
                              _lib.ptr(loss), _lib.ptr(out), _lib.ptr(grad), _lib.ptr(ws), ws_bytes, _lib.stream()))
        ctx.save_for_backward(grad)
        ctx.target_dtype = target.dtype
        return out if none else loss

    @staticmethod
    def backward(ctx, g):
        (grad, ) = ctx.saved_tensors
        # g: the upstream scalar, or the upstream map of reduction 'none'; the product in pred's dtype
        gp = (grad * g).to(grad.dtype)
        gt = (-gp).to(ctx.target_dtype) if ctx.needs_input_grad[1] else None
        return (gp if ctx.needs_input_grad[0] else None), gt, None, None, None, None, None


def _elementwise(kind, pred, target, eps):
    if kind == _lib.LOSS_L1:
        return (pred - target).abs()
    if kind == _lib.LOSS_MSE:
        return (pred - target)**2
    return torch.sqrt((pred - target)**2 + eps)


def _torch_pixel_loss(kind, pred, target, weight, reduction, loss_weight, eps):
    """The reference's formula (weight_reduce_loss, loss_util.py:26-55) in torch ops on the device
    tensors: a weight map that requires grad, or one the kernel's two layouts do not cover."""
    loss = _elementwise(kind, pred, target, eps)
    if weight is not None:
        assert weight.dim() == loss.dim()
        assert weight.size(1) == 1 or weight.size(1) == loss.size(1)
        loss = loss * weight
    if reduction == 'sum':
        loss = loss.sum()
    elif reduction == 'mean':
        if weight is None:
            loss = loss.mean()
        else:
            loss = loss.sum() / (weight.sum() if weight.size(1) > 1 else weight.sum() * loss.size(1))
    return loss_weight * loss


def _pixel_loss(kind, pred, target, weight, reduction, loss_weight, eps=0.0):
    if not pred.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if weight is None and kind == _lib.LOSS_L1 and reduction in ('mean', 'sum') and not target.requires_grad:
        return _L1Fused.apply(pred, target, loss_weight, reduction == 'mean')
    # sizes are C ints: a tensor that is not 4-D travels as one row of numel() elements
    kernel_ok = pred.shape == target.shape and 0 < pred.numel() < (2**32 - 9 if pred.dim() == 4 else 2**31)
    if weight is not None:
        kernel_ok = (kernel_ok and not weight.requires_grad and pred.dim() == 4 and weight.dim() == 4
                     and weight.size(1) in (1, pred.size(1)) and weight.size(0) == pred.size(0)
                     and weight.shape[2:] == pred.shape[2:])
    if not kernel_ok:
        return _torch_pixel_loss(kind, pred, target, weight, reduction, loss_weight, eps)
    return _PixelLossFused.apply(pred, target, weight, kind, reduction, loss_weight, eps)


def _check_reduction(reduction):
    if reduction not in _reduction_modes:
        raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: {_reduction_modes}')


@LOSS_REGISTRY.register()
class L1Loss(nn.Module):
    """L1 (mean absolute error, MAE) loss (basic_loss.py:27-52)."""

    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, pred, target, weight=None, **kwargs):
        return _pixel_loss(_lib.LOSS_L1, pred, target, weight, self.reduction, self.loss_weight)


@LOSS_REGISTRY.register()
class MSELoss(nn.Module):
    """MSE (L2) loss (basic_loss.py:55-80)."""

    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, pred, target, weight=None, **kwargs):
        return _pixel_loss(_lib.LOSS_MSE, pred, target, weight, self.reduction, self.loss_weight)


@LOSS_REGISTRY.register()
class CharbonnierLoss(nn.Module):
    """Charbonnier loss sqrt((pred - target)^2 + eps), a differentiable variant of L1
    (basic_loss.py:83-114)."""

    def __init__(self, loss_weight=1.0, reduction='mean', eps=1e-12):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.eps = eps

    def forward(self, pred, target, weight=None, **kwargs):
        return _pixel_loss(_lib.LOSS_CHARBONNIER, pred, target, weight, self.reduction, self.loss_weight, self.eps)


@LOSS_REGISTRY.register()
class WeightedTVLoss(L1Loss):
    """Weighted total variation: the weighted L1 of the two shifted slice pairs of the prediction
    (basic_loss.py:117-143); both operands of each pair carry a gradient."""

    def __init__(self, loss_weight=1.0, reduction='mean'):
        if reduction not in ['mean', 'sum']:
            raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: mean | sum')
        super().__init__(loss_weight=loss_weight, reduction=reduction)

    def forward(self, pred, weight=None):
        if weight is None:
            y_weight = None
            x_weight = None
        else:
            y_weight = weight[:, :, :-1, :]
            x_weight = weight[:, :, :, :-1]
        y_diff = super().forward(pred[:, :, :-1, :], pred[:, :, 1:, :], weight=y_weight)
        x_diff = super().forward(pred[:, :, :, :-1], pred[:, :, :, 1:], weight=x_weight)
        return x_diff + y_diff


class _FeatureTerms(torch.autograd.Function):
    """Both terms of one tapped layer from the prediction's feature map xf: the criterion against the
    target's map gf (sr_pixel_loss, which leaves d/dxf) and the Gram matrix of xf.  The backward is the
    Gram GEMM with the criterion's gradient, times its upstream scalar, added in the GEMM's store
    (sr_gram_bwd's beta * res) instead of a separate accumulation pass over the feature map."""

    @staticmethod
    def forward(ctx, xf, gf, kind, reduction):
        ctx.set_materialize_grads(False)
        xf, gf = xf.contiguous(), gf.contiguous()
        lib = _lib.load()
        ws_bytes = lib.sr_pixel_loss_workspace(xf.numel())
        ws = torch.empty(ws_bytes // 8 + 1, device=xf.device, dtype=torch.float64)
        loss = torch.empty((), device=xf.device, dtype=torch.float32)
        grad = torch.empty_like(xf)
        _lib.check(
            lib.sr_pixel_loss(kind, _REDUCE[reduction], _lib.dtype_code(xf.dtype), _lib.dtype_code(gf.dtype),
                              _lib.ptr(xf), _lib.ptr(gf), None, 0, 1, 1, 1, xf.numel(), 1.0, 0.0, _lib.ptr(loss), None,
                              _lib.ptr(grad), _lib.ptr(ws), ws_bytes, _lib.stream()))
        ctx.scale = P.gram_scale(xf)
        ctx.save_for_backward(xf, grad)
        return loss, P.gram_fwd_raw(xf, ctx.scale)

    @staticmethod
    def backward(ctx, g_loss, dG):
        xf, grad = ctx.saved_tensors
        res = None if g_loss is None else (grad * g_loss).to(grad.dtype)
        if dG is None:
            return res, None, None, None
        return P.gram_bwd_raw(xf, dG.float().contiguous(), ctx.scale, res=res, beta=1.0), None, None, None


@LOSS_REGISTRY.register()
class PerceptualLoss(nn.Module):
    """Perceptual loss with the style loss (basic_loss.py:147-253).

    ``layer_weights``: {VGG layer name: weight}; ``criterion``: 'l1' | 'l2' | 'fro'.  ``forward(x, gt)``
    returns ``(percep_loss, style_loss)``, each None when its weight is 0.  ``pretrain_path`` / ``pretrained``
    go to the VGGFeatureExtractor: the weights come from a file, nothing is downloaded."""

    def __init__(self,
                 layer_weights,
                 vgg_type='vgg19',
                 use_input_norm=True,
                 range_norm=False,
                 perceptual_weight=1.0,
                 style_weight=0.,
                 criterion='l1',
                 pretrain_path=None,
                 pretrained=True):
        super().__init__()
        self.perceptual_weight = perceptual_weight
        self.style_weight = style_weight
        self.layer_weights = layer_weights
        self.criterion_type = criterion
        if criterion == 'l1':
            self._kind, self._reduction = _lib.LOSS_L1, 'mean'
        elif criterion == 'l2':
            self._kind, self._reduction = _lib.LOSS_MSE, 'mean'
        elif criterion == 'fro':
            self._kind, self._reduction = _lib.LOSS_MSE, 'sum'  # the square root follows
        else:
            raise NotImplementedError(f'{criterion} criterion has not been supported.')
        self.vgg = VGGFeatureExtractor(layer_name_list=list(layer_weights.keys()), vgg_type=vgg_type,
                                       use_input_norm=use_input_norm, range_norm=range_norm,
                                       pretrain_path=pretrain_path, pretrained=pretrained)

    def _finish(self, v):
        return v.sqrt() if self.criterion_type == 'fro' else v

    def _criterion(self, a, b):
        # without a weight map the layout does not matter: NHWC features and Gram matrices are flat arrays
        return self._finish(_PixelLossFused.apply(a, b, None, self._kind, self._reduction, 1.0, 0.0))

    def forward(self, x, gt):
        if not x.is_cuda or not gt.is_cuda:
            raise NotImplementedError(_CPU_MESSAGE)
        x_features = self.vgg(x)
        with torch.no_grad():
            gt_features = self.vgg(gt.detach())
        want_p, want_s = self.perceptual_weight > 0, self.style_weight > 0
        percep_loss, style_loss = (0 if want_p else None), (0 if want_s else None)
        for k in x_features.keys():
            xf, gf, w = x_features[k], gt_features[k], self.layer_weights[k]
            if want_p and want_s and xf.requires_grad:
                lp, gram_x = _FeatureTerms.apply(xf, gf, self._kind, self._reduction)
                lp = self._finish(lp)
            else:
                lp = self._criterion(xf, gf) if want_p else None
                gram_x = P.gram(xf) if want_s else None
            if want_p:
                percep_loss = percep_loss + lp * w
            if want_s:
                with torch.no_grad():
                    gram_gt = P.gram(gf)
                style_loss = style_loss + self._criterion(gram_x, gram_gt) * w
        if want_p:
            percep_loss = percep_loss * self.perceptual_weight
        if want_s:
            style_loss = style_loss * self.style_weight
        return percep_loss, style_loss
