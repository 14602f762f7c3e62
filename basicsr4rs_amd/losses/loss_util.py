"""The LDL artifact map (mirror of basicsr/losses/loss_util.py:99-145) and the fused ``ldl_opt`` term of
RealESRGANModel (basicsr/models/realesrgan_model.py:211-226) on the kernels of csrc/ldl.hip.

``get_refined_artifact_map(img_gt, img_output, img_ema, ksize)`` returns the weight map ``w`` [N,1,H,W] and is
differentiable with respect to ``img_output`` through all of it -- the mask, the 7x7 window variances and the
per-image variance; the reference does not detach the map.  ``ldl_l1_term`` is ``L1Loss(w * out, w * gt)`` without
the two products: the forward launches leave the loss, one backward launch the whole gradient.

One deliberate divergence: for a constant residual map (V_n == 0) the reference's backward is inf * 0 = NaN; here
the derivative of V_n^(1/5) is defined as 0 for that image, in the kernels and in the torch composition.
"""
import torch
from torch.nn import functional as F

from .. import _lib

_CPU_MESSAGE = 'basicsr4rs_amd losses run on the MI355X device'
_REDUCE = {'mean': _lib.REDUCE_MEAN, 'sum': _lib.REDUCE_SUM}
_KSIZE = 7  # the window the kernels cover


def _prepare(out, gt, ema):
    """The operands as the kernels take them: out fp32 / bf16, gt and ema fp32 or out's dtype, contiguous."""
    if out.dtype not in (torch.float32, torch.bfloat16):
        out = out.float()
    gt, ema = (t if t.dtype in (torch.float32, out.dtype) else t.float() for t in (gt, ema))
    return out.contiguous(), gt.detach().contiguous(), ema.detach().contiguous()


def _forward(out, gt, ema, l1, reduction, loss_weight, want_map):
    """sr_ldl_map_fwd: (w or None, loss or None, planes, stats)."""
    lib = _lib.load()
    N, C, H, W = out.shape
    dev = out.device
    ws_bytes = lib.sr_ldl_map_workspace(N, H, W)
    ws = torch.empty(ws_bytes // 4 + 1, device=dev, dtype=torch.float32)
    planes = torch.empty(4, N, H, W, device=dev, dtype=torch.float32)
    stats = torch.empty(N, 8, device=dev, dtype=torch.float32)
    w = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32) if want_map else None
    loss = torch.empty((), device=dev, dtype=torch.float32) if l1 else None
    _lib.check(
        lib.sr_ldl_map_fwd(_lib.dtype_code(out.dtype), _lib.dtype_code(gt.dtype), _lib.dtype_code(ema.dtype), _lib.ptr(out),
                           _lib.ptr(gt), _lib.ptr(ema), N, C, H, W, _KSIZE, int(l1), _REDUCE.get(reduction, 0),
                           float(loss_weight), _lib.ptr(w), _lib.ptr(planes), _lib.ptr(stats), _lib.ptr(loss), _lib.ptr(ws),
                           ws_bytes, _lib.stream()))
    return w, loss, planes, stats


def _backward(out, gt, planes, stats, dW, upstream, reduction, loss_weight):
    """sr_ldl_map_bwd: d out in out's dtype."""
    lib = _lib.load()
    N, C, H, W = out.shape
    ws_bytes = lib.sr_ldl_map_workspace(N, H, W) if dW is not None else 0
    ws = torch.empty(ws_bytes // 4 + 1, device=out.device, dtype=torch.float32) if dW is not None else None
    dout = torch.empty_like(out)
    _lib.check(
        lib.sr_ldl_map_bwd(_lib.dtype_code(out.dtype), _lib.dtype_code(gt.dtype), _lib.ptr(out), _lib.ptr(gt),
                           _lib.ptr(planes), _lib.ptr(stats), _lib.ptr(dW), _lib.ptr(upstream), N, C, H, W, _KSIZE,
                           _REDUCE.get(reduction, 0), float(loss_weight), _lib.ptr(dout), _lib.ptr(ws), ws_bytes,
                           _lib.stream()))
    return dout


class _ArtifactMap(torch.autograd.Function):
    """w = P_n L m through sr_ldl_map_fwd; the backward takes the upstream map dW through sr_ldl_map_bwd."""

    @staticmethod
    def forward(ctx, out, gt, ema):
        ctx.in_dtype = out.dtype
        out, gt, ema = _prepare(out, gt, ema)
        w, _, planes, stats = _forward(out, gt, ema, False, None, 1.0, True)
        ctx.save_for_backward(out, gt, planes, stats)
        return w

    @staticmethod
    def backward(ctx, dW):
        out, gt, planes, stats = ctx.saved_tensors
        dout = _backward(out, gt, planes, stats, dW.float().contiguous(), None, None, 1.0)
        return dout.to(ctx.in_dtype), None, None


class _LdlL1Fused(torch.autograd.Function):
    """loss = L1Loss(loss_weight, reduction)(w out, w gt) = k sum_n P_n S_n; one backward launch writes d out,
    the upstream scalar read on the device."""

    @staticmethod
    def forward(ctx, out, gt, ema, loss_weight, reduction):
        ctx.in_dtype = out.dtype
        out, gt, ema = _prepare(out, gt, ema)
        _, loss, planes, stats = _forward(out, gt, ema, True, reduction, loss_weight, False)
        ctx.save_for_backward(out, gt, planes, stats)
        ctx.loss_weight, ctx.reduction = loss_weight, reduction
        return loss

    @staticmethod
    def backward(ctx, g):
        out, gt, planes, stats = ctx.saved_tensors
        dout = _backward(out, gt, planes, stats, None, g.float().contiguous(), ctx.reduction, ctx.loss_weight)
        return dout.to(ctx.in_dtype), None, None, None, None


def _torch_artifact_map(img_gt, img_output, img_ema, ksize):
    """The same formula in torch ops on the device tensors: a window other than 7x7, or a layout / dtype the kernels
    do not cover.  The k*k window values of every pixel are gathered (F.unfold), so it is k*k times the residual map in
    memory."""
    r = (img_gt - img_output).abs().sum(1, keepdim=True)
    e = (img_gt - img_ema).abs().sum(1, keepdim=True)
    N, _, H, W = r.shape
    pad = (ksize - 1) // 2
    windows = F.unfold(F.pad(r, (pad, pad, pad, pad), mode='reflect'), ksize)  # [N, k*k, H*W]
    local = windows.var(dim=1, unbiased=True).view(N, 1, H, W)
    V = r.flatten(1).var(dim=1, unbiased=True)
    live = V > 0  # V == 0: P = 0 with a zero derivative instead of the reference's NaN
    P = torch.where(live, V, torch.ones_like(V)).pow(0.2) * live
    return torch.where(r < e, torch.zeros_like(local), P.view(N, 1, 1, 1) * local)


def _kernel_ok(img_gt, img_output, img_ema, ksize):
    o = img_output
    return (ksize == _KSIZE and o.dim() == 4 and img_gt.shape == o.shape and img_ema.shape == o.shape
            and o.dtype in (torch.float32, torch.bfloat16, torch.float16) and o.size(2) >= 4 and o.size(3) >= 4
            and 0 < o.numel() < 2**31 and o.size(0) <= 65535 and not img_gt.requires_grad and not img_ema.requires_grad)


def _check_device(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise NotImplementedError(_CPU_MESSAGE)


def get_refined_artifact_map(img_gt, img_output, img_ema, ksize):
    """The LDL artifact map (loss_util.py:121-145): the weight of every pixel of being an artifact, from the local
    (window) and the global (image) variance of the residual, zero where the EMA network's residual is larger.

    img_gt / img_output / img_ema: [N,C,H,W] on the device; returns [N,1,H,W] (fp32 from the kernels).  ``ksize`` 7
    runs on the HIP kernels; another window, or operands they do not cover (a gradient wanted for ``img_gt`` or
    ``img_ema``, fewer than 4 rows or columns, 2^31 elements or more), on the torch composition of the same formula."""
    _check_device(img_gt, img_output, img_ema)
    if _kernel_ok(img_gt, img_output, img_ema, ksize):
        return _ArtifactMap.apply(img_output, img_gt, img_ema)
    return _torch_artifact_map(img_gt, img_output, img_ema, ksize)


def ldl_l1_term(out, gt, ema, loss_weight=1.0, reduction='mean'):
    """``L1Loss(loss_weight, reduction)(w * out, w * gt)`` with ``w = get_refined_artifact_map(gt, out, ema, 7)``,
    fused: w >= 0, so the term is k * sum_p w r and neither product is materialised."""
    _check_device(out, gt, ema)
    if reduction not in _REDUCE:
        raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: mean | sum')
    if _kernel_ok(gt, out, ema, _KSIZE):
        return _LdlL1Fused.apply(out, gt, ema, loss_weight, reduction)
    w = _torch_artifact_map(gt, out, ema, _KSIZE)
    loss = (w * out - w * gt).abs()
    return loss_weight * (loss.mean() if reduction == 'mean' else loss.sum())
