"""Losses for pairs that are not co-registered (mirror of basicsr/losses/align_loss.py).

``RegisteredLoss`` shifts the prediction by every offset of a sub-pixel grid (separable Lanczos-3 taps), takes the L1
or MSE against the target on the crop the shifts do not disturb, and forwards, per image, only the smallest: the
gradient flows through the winning shift alone.  The reference materialises the [B, S^2, C, H, W] stack of shifted
images and the loss map of the same size; here one call of ``sr_registered_loss`` (csrc/regloss.hip)
evaluates the S^2 losses from LDS tiles, picks the minimum on the device and writes d loss / d pred, and its
workspace holds per-tile partial sums only.  The tap table is built on the host with the reference's torch ops
(``lanczos_kernel``), so it equals the reference's buffer bit for bit; the kernels take it as data.

``ShiftConv2d`` returns the stack itself (plain torch ops; for inspection and tests).  ``EncoderLoss`` is the fused
MSE of the encoder output against ``gt`` or against the bilinearly resized ``lq``.
"""
import math

import torch
from torch import nn as nn
from torch.nn import functional as F

from .. import _lib
from ..ops import degrade
from ..utils.registry import LOSS_REGISTRY
from .basic_loss import _CPU_MESSAGE, _REDUCE, MSELoss

# limits of the kernels (sr_registered_loss): shift values per axis and taps per filter
_S_MAX, _K_MIN, _K_MAX = 9, 7, 13


def lanczos_kernel(dx, a=3, N=None, dtype=None, device=None):
    """1-D Lanczos taps that translate a signal by ``dx`` pixels (a float or a [n, 1] tensor): [n, K] with
    K = 2 (a + max ceil|dx|) + 1, or ``N`` when that is wider.  Tap x is a sin(px) sin(px / a) / px^2 with
    px = pi (x - dx) + 1e-3: not zeroed beyond |x - dx| < a, not normalised, and an integer shift gives a
    near-delta, not a delta -- all as the reference, whose torch ops these are (same values bit for bit)."""
    if not torch.is_tensor(dx):
        dx = torch.tensor(dx, dtype=dtype, device=device)
    device = dx.device if device is None else device
    dtype = dx.dtype if dtype is None else dtype
    D = dx.abs().ceil().int()
    support = 2 * (a + D) + 1
    if N is None or N < support.max():
        N = support
    Z = (N - support) // 2
    lo, hi = (-(a + D + Z)).min(), (a + D + Z + 1).max()
    x = torch.arange(lo, hi, dtype=dtype, device=device).view(1, -1) - dx
    px = (math.pi * x) + 1e-3
    return a * torch.sin(px) * torch.sin(px / a) / px**2


def shift_taps(start, end, step):
    """The [S, K] table of a shift grid: one row of ``lanczos_kernel`` per value of arange(start, end + 1e-3, step)."""
    shift = torch.arange(start, end + 1e-3, step)[:, None]
    return lanczos_kernel(shift, a=3)


class ShiftConv2d(nn.Module):
    """Every shift of x on the last two axes: ``forward(x [B, C, H, W])`` -> [B, S^2, C, H, W], entry sy * S + sx the
    zero-padded cross-correlation of x with the taps of shift sy along H and sx along W.  Buffers ``K_y``
    [S, 1, 1, K, 1] and ``K_x`` [S, 1, 1, 1, K] as the reference.  Plain torch ops, off the hot path."""

    def __init__(self, start, end, step):
        super().__init__()
        self.start, self.end, self.step = float(start), float(end), float(step)
        taps = shift_taps(self.start, self.end, self.step)
        self.register_buffer('K_y', taps[:, None, None, :, None].contiguous())
        self.register_buffer('K_x', taps[:, None, None, None, :].contiguous())

    @property
    def taps(self):
        """[S, K] fp32, a view of ``K_x``."""
        return self.K_x.view(self.K_x.shape[0], self.K_x.shape[-1])

    def forward(self, x):
        B, C, H, W = x.shape
        S, K = self.taps.shape
        r = K // 2
        ys = F.conv2d(x.reshape(B * C, 1, H, W), self.K_y.view(S, 1, K, 1).to(x.dtype), padding=(r, 0))
        xs = F.conv2d(ys.reshape(B * C * S, 1, H, W), self.K_x.view(S, 1, 1, K).to(x.dtype), padding=(0, r))
        return xs.view(B, C, S * S, H, W).transpose(1, 2)


def _torch_registered(shiftconv, pred, target, l1, reduction, loss_weight):
    """The reference's formula in torch ops on the device tensors (the fallback of ``RegisteredLoss``)."""
    r = shiftconv.taps.shape[1] // 2
    shifted = shiftconv(pred)[..., r:-r, r:-r]
    d = shifted - target[:, None, :, r:-r, r:-r]
    table = (d.abs() if l1 else d * d).mean(dim=(-3, -2, -1))
    idx = table.argmin(dim=1)
    picked = table[torch.arange(table.shape[0], device=table.device), idx]
    if reduction == 'mean':
        loss = picked.mean()
    elif reduction == 'sum':
        loss = picked.sum()
    else:
        loss = picked
    return loss_weight * loss, idx.to(torch.int32), table


class _RegisteredFused(torch.autograd.Function):
    """sr_registered_loss: the loss (an fp32 scalar, or [B] for reduction 'none'), the selected shifts and
    d loss / d pred from one call.  A backward that itself needs a graph (double backward) is recomputed through the
    torch composition."""

    @staticmethod
    def forward(ctx, pred, target, shiftconv, l1, reduction, loss_weight, want_table):
        pred_in = pred
        if pred.dtype not in (torch.float32, torch.bfloat16):
            pred = pred.float()
        if target.dtype != torch.float32 and target.dtype != pred.dtype:
            target = target.float()
        pred, target = pred.contiguous(), target.contiguous()
        taps = shiftconv.taps.float().contiguous()  # fp32 buffers as built: the view itself, no copy
        S, K = taps.shape
        B, C, H, W = pred.shape
        lib = _lib.load()
        ws_bytes = lib.sr_registered_loss_workspace(B, C, H, W, S)
        ws = torch.empty(ws_bytes // 8 + 1, device=pred.device, dtype=torch.float64)
        none = reduction == 'none'
        loss = torch.empty((B, ) if none else (), device=pred.device, dtype=torch.float32)
        idx = torch.empty(B, device=pred.device, dtype=torch.int32)
        table = torch.empty(B, S * S, device=pred.device, dtype=torch.float32) if want_table else None
        grad = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        _lib.check(
            lib.sr_registered_loss(_lib.LOSS_L1 if l1 else _lib.LOSS_MSE, _REDUCE[reduction], _lib.dtype_code(pred.dtype),
                                   _lib.dtype_code(target.dtype), _lib.ptr(pred), _lib.ptr(target), _lib.ptr(taps), S, K,
                                   B, C, H, W, float(loss_weight), _lib.ptr(loss), _lib.ptr(idx), _lib.ptr(table),
                                   _lib.ptr(grad), _lib.ptr(ws), ws_bytes, _lib.stream()))
        ctx.save_for_backward(grad, pred_in, target)  # the input itself: a double backward reaches it through it
        ctx.recompute = (shiftconv, l1, reduction, loss_weight)
        ctx.mark_non_differentiable(idx)
        if want_table:
            ctx.mark_non_differentiable(table)
            return loss, idx, table
        return loss, idx

    @staticmethod
    def backward(ctx, g, *unused):
        grad, pred, target = ctx.saved_tensors
        if torch.is_grad_enabled():  # create_graph: a differentiable backward
            with torch.enable_grad():
                loss = _torch_registered(ctx.recompute[0], pred.float(), target.float(), *ctx.recompute[1:])[0]
                gp = torch.autograd.grad(loss, pred, g, create_graph=True)[0]
            return gp, None, None, None, None, None, None
        if g.dim():  # reduction 'none': one upstream element per image
            g = g.view(-1, 1, 1, 1)
        return (grad * g).to(grad.dtype), None, None, None, None, None, None


@LOSS_REGISTRY.register()
class RegisteredLoss(nn.Module):
    """min over the shifts of a sub-pixel grid of L1 / MSE(shifted(y_pred), y), per image (align_loss.py:161-256).

    ``start``, ``end``, ``step``: the grid arange(start, end + 1e-3, step) of S shift values per axis, S^2 shifts.
    ``loss_func``: 'l1', 'l2' or 'mse' (case-insensitive).  ``reduction`` over the batch: 'mean' | 'sum' | 'none'
    ([B]); anything else raises ``NotImplementedError`` at call time, as the reference.  On ties the first shift
    (y index slow) is selected; a NaN entry is selected and gives NaN for that image (``torch.argmin``).

    The loss is scored on the crop [r, H - r) x [r, W - r), r = K // 2.  ``H`` or ``W`` below 2r + 1 raises
    ``ValueError``; the reference returns NaN there (the mean of an empty crop).  ``last_shift``: the int32 [B]
    indices sy * S + sx of the latest call, kept on the device, for logging.

    Runs on ``sr_registered_loss`` for S <= 9, K <= 13 (|shift| <= 3) and B C H W < 2^31, with fp32 or bf16
    predictions; a target that requires grad, a shape outside those limits and a double backward go through torch
    ops with the reference's formula.  CPU tensors are refused."""

    def __init__(self, start, end, step, loss_func, loss_weight=1.0, reduction='mean'):
        super().__init__()
        self._shiftconv2d = ShiftConv2d(start, end, step)
        self.start, self.end, self.step = float(start), float(end), float(step)
        kind = str(loss_func).lower()
        if kind == 'l1':
            self._l1 = True
        elif kind in ('mse', 'l2'):
            self._l1 = False
        else:
            raise ValueError(f"Unsupported loss_func: {loss_func}. Choose from ['l1', 'l2', 'mse']")
        self.loss_func = kind
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.last_shift = None

    def _check(self, y_pred, y):
        if not y_pred.is_cuda or not y.is_cuda:
            raise NotImplementedError(_CPU_MESSAGE)
        if y_pred.dim() != 4 or y_pred.shape != y.shape:
            raise ValueError(f'RegisteredLoss: two [B, C, H, W] tensors of one shape are expected, got '
                             f'{tuple(y_pred.shape)} and {tuple(y.shape)}')
        K = self._shiftconv2d.taps.shape[1]
        if y_pred.shape[2] < K or y_pred.shape[3] < K:
            raise ValueError(f'RegisteredLoss: H and W must be at least 2r + 1 = {K} for this shift grid, got '
                             f'{tuple(y_pred.shape[2:])}')

    def _kernel_ok(self, y_pred, y):
        S, K = self._shiftconv2d.taps.shape
        return (S <= _S_MAX and _K_MIN <= K <= _K_MAX and 0 < y_pred.numel() < 2**31
                and not (y.requires_grad and torch.is_grad_enabled()))

    def _shifted_loss(self, y_pred, y):
        """The [B, S^2] table of the losses of every shift (fp32, no gradient)."""
        self._check(y_pred, y)
        with torch.no_grad():
            if self._kernel_ok(y_pred, y):
                return _RegisteredFused.apply(y_pred, y, self._shiftconv2d, self._l1, 'none', 1.0, True)[2]
            return _torch_registered(self._shiftconv2d, y_pred.float(), y.float(), self._l1, 'none', 1.0)[2]

    def registered_loss(self, y_pred, y):
        if self.reduction not in ('mean', 'sum', 'none'):
            raise NotImplementedError(f"Expected `reduction` values: ['mean'|'sum'|'none']. Got {self.reduction}.")
        self._check(y_pred, y)
        if self._kernel_ok(y_pred, y):
            loss, idx = _RegisteredFused.apply(y_pred, y.detach(), self._shiftconv2d, self._l1, self.reduction,
                                               self.loss_weight, False)
        else:
            loss, idx, _ = _torch_registered(self._shiftconv2d, y_pred.float(), y.float(), self._l1, self.reduction,
                                             self.loss_weight)
        self.last_shift = idx
        return loss

    def forward(self, y_pred, y):
        return self.registered_loss(y_pred, y)


@LOSS_REGISTRY.register()
class EncoderLoss(nn.Module):
    """MSE of the encoder output ``z_start`` against ``gt`` (strategy 'gt') or against ``lq`` resized bilinearly
    (align_corners=False) to z_start's size (strategy 'lq'), on the fused MSE kernel (align_loss.py:259-300).
    ``lq`` is required by both strategies, as in the reference, whose docstring calls it optional."""

    def __init__(self, loss_weight=1.0, strategy='gt', reduction='mean'):
        super().__init__()
        if strategy not in ('gt', 'lq'):
            raise ValueError(f'Unsupported loss strategy {strategy}')
        self.strategy = strategy
        self.mse = MSELoss(loss_weight=loss_weight, reduction=reduction)
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, z_start, gt, lq):
        if self.strategy == 'gt':
            return self.mse(z_start, gt)
        with torch.no_grad():
            lq_up = degrade.resize(lq.float(), size=tuple(z_start.shape[2:]), mode='bilinear')
        return self.mse(z_start, lq_up)
