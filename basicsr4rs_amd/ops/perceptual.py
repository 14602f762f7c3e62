"""Max-pool and Gram-matrix ops of the perceptual / style loss on the HIP kernels of csrc/perceptual.hip.

``max_pool2(x, stride)``: nn.MaxPool2d(2, stride) on an NHWC feature map (torch's first-maximum and NaN
rules); the backward recomputes each window's choice from the saved input, so the forward stores nothing.
``gram(feat, res_grad=None)``: the per-image Gram matrix of basic_loss.py:240-253, fp32 [N, C, C], with
scale 1 / (C H W); its backward is one GEMM per image, and ``res_grad`` (feat's shape and dtype) is added
to the feature gradient in that GEMM's store.  ``relu(x)``: the stand-alone ReLU after a tapped conv.

Every launch runs under a ``ktrace.span`` with the kernel name and its algorithmic FLOPs / bytes.
"""
import torch

from .. import _lib
from ..utils import ktrace
from . import conv as C
from .fused_act import fused_bias_act


def _launch(name, flops, nbytes, fn, args, keep, launches=1):
    if ktrace.active():
        with ktrace.span(name, flops, nbytes, relaunch=lambda a=args, k=keep: fn(*a), launches=launches):
            _lib.check(fn(*args))
    else:
        _lib.check(fn(*args))


def _check_map(x, what):
    if not x.is_cuda:
        raise NotImplementedError('basicsr4rs_amd HIP ops need tensors on the MI355X (cuda) device')
    if x.dim() != 4 or x.shape[-1] % 8:
        raise ValueError(f'{what}: an NHWC map with a multiple of 8 channels is expected, got {tuple(x.shape)}')
    _lib.dtype_code(x.dtype)


def pool_out_size(size, stride):
    return (size - 2) // stride + 1


def maxpool2_fwd_raw(x, stride):
    _check_map(x, 'max_pool2')
    N, H, W, Cc = x.shape
    y = torch.empty(N, pool_out_size(H, stride), pool_out_size(W, stride), Cc, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(x.dtype), _lib.ptr(x), N, H, W, Cc, int(stride), _lib.ptr(y), _lib.stream())
    # 3 comparisons per output; x read once (stride 2; every element up to 4 times from cache with 1), y written
    _launch('maxpool2_fwd_kernel', 3.0 * y.numel(), x.element_size() * (x.numel() + y.numel()), lib.sr_maxpool2_fwd, args,
            (x, y))
    return y


def maxpool2_bwd_raw(x, dy, stride):
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    lib = _lib.load()
    args = (_lib.dtype_code(x.dtype), _lib.ptr(x), _lib.ptr(dy), N, H, W, Cc, int(stride), _lib.ptr(dx), _lib.stream())
    _launch('maxpool2_bwd_kernel', 3.0 * dy.numel(), x.element_size() * (2 * x.numel() + dy.numel()), lib.sr_maxpool2_bwd,
            args, (x, dy, dx))
    return dx


class _MaxPool2(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, stride):
        x = x.contiguous()
        ctx.stride = stride
        ctx.save_for_backward(x)
        return maxpool2_fwd_raw(x, stride)

    @staticmethod
    def backward(ctx, dy):
        (x, ) = ctx.saved_tensors
        return maxpool2_bwd_raw(x, dy.to(x.dtype).contiguous(), ctx.stride), None


def max_pool2(x, stride=2):
    """nn.MaxPool2d(kernel_size=2, stride=stride) of an NHWC map (stride 1 or 2, no padding, floor mode)."""
    if stride not in (1, 2):
        raise ValueError(f'max_pool2: stride {stride} is not supported (1 or 2)')
    _check_map(x, 'max_pool2')
    if x.shape[1] < 2 or x.shape[2] < 2:
        raise ValueError(f'max_pool2: the map {tuple(x.shape)} is smaller than the 2 x 2 window')
    return _MaxPool2.apply(x, stride)


class _Relu(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x):
        y = fused_bias_act(x, None, None, 3, 0, 0.0, 1.0)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y, ) = ctx.saved_tensors
        return C.act_backward(dy.to(y.dtype).contiguous(), y, _lib.ACT_RELU, 0.0, 1.0)


def relu(x):
    """ReLU as a pass of its own (sr_fused_bias_act / sr_act_backward): after a conv whose pre-activation
    map is tapped, where it cannot be fused into the conv's epilogue."""
    return _Relu.apply(x)


def _gram_dims(feat):
    if feat.dim() == 4:
        N, H, W, Cc = feat.shape
        return N, H * W, Cc
    if feat.dim() == 3:
        return tuple(feat.shape)
    raise ValueError(f'gram: an NHWC map or [N, HW, C] is expected, got {tuple(feat.shape)}')


def gram_scale(feat):
    N, HW, Cc = _gram_dims(feat)
    return 1.0 / (Cc * HW)


def gram_fwd_raw(feat, scale):
    """G [N, C, C] fp32 = feat^T feat * scale per image (feat contiguous, NHWC or [N, HW, C])."""
    N, HW, Cc = _gram_dims(feat)
    if not feat.is_cuda:
        raise NotImplementedError('basicsr4rs_amd HIP ops need tensors on the MI355X (cuda) device')
    if Cc % 8 or Cc > 512:
        raise ValueError(f'gram: {Cc} channels (a multiple of 8, at most 512, is supported)')
    lib = _lib.load()
    G = torch.empty(N, Cc, Cc, device=feat.device, dtype=torch.float32)
    ws_bytes = lib.sr_gram_workspace(N, HW, Cc)
    ws = torch.empty(ws_bytes // 4, device=feat.device, dtype=torch.float32) if ws_bytes else None
    args = (_lib.dtype_code(feat.dtype), _lib.ptr(feat), N, HW, Cc, float(scale), _lib.ptr(G), _lib.ptr(ws), ws_bytes,
            _lib.stream())
    # feat read once, G written; with split K the partials written and read once more
    _launch('gram_fwd_kernel', 2.0 * N * HW * Cc * Cc, feat.element_size() * feat.numel() + 4 * G.numel() + 2 * ws_bytes,
            lib.sr_gram_fwd, args, (feat, G, ws), launches=2 if ws_bytes else 1)
    return G


def gram_bwd_raw(feat, dG, alpha, res=None, beta=1.0):
    """alpha * feat (dG + dG^T) + beta * res per image, in feat's dtype and shape."""
    N, HW, Cc = _gram_dims(feat)
    if dG.dtype != torch.float32 or tuple(dG.shape) != (N, Cc, Cc) or not dG.is_contiguous():
        raise ValueError(f'gram backward: dG must be contiguous fp32 {(N, Cc, Cc)}, got {dG.dtype} {tuple(dG.shape)}')
    if res is not None and (res.shape != feat.shape or res.dtype != feat.dtype or not res.is_contiguous()):
        raise ValueError(f'gram backward: res must be like feat ({tuple(feat.shape)} {feat.dtype}), '
                         f'got {tuple(res.shape)} {res.dtype}')
    lib = _lib.load()
    dF = torch.empty_like(feat)
    args = (_lib.dtype_code(feat.dtype), _lib.ptr(feat), _lib.ptr(dG), _lib.ptr(res), N, HW, Cc, float(alpha),
            float(beta), _lib.ptr(dF), _lib.stream())
    nbytes = feat.element_size() * feat.numel() * (2 + (res is not None)) + 4 * dG.numel()
    _launch('gram_bwd_kernel', 2.0 * N * HW * Cc * Cc, nbytes, lib.sr_gram_bwd, args, (feat, dG, res, dF))
    return dF


class _Gram(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feat, res_grad):
        feat = feat.contiguous()
        ctx.scale = gram_scale(feat)
        ctx.save_for_backward(feat, res_grad)
        return gram_fwd_raw(feat, ctx.scale)

    @staticmethod
    def backward(ctx, dG):
        feat, res = ctx.saved_tensors
        return gram_bwd_raw(feat, dG.float().contiguous(), ctx.scale, res=res, beta=1.0), None


def gram(feat, res_grad=None):
    """Gram matrix of an NHWC feature map: [N, C, C] fp32, (feat^T feat) / (C H W) per image.  ``res_grad``
    (feat's shape and dtype, no gradient of its own) is added to d/dfeat in the backward GEMM's store."""
    if res_grad is not None:
        if res_grad.shape != feat.shape or res_grad.dtype != feat.dtype:
            raise ValueError(f'gram: res_grad must be like feat ({tuple(feat.shape)} {feat.dtype})')
        res_grad = res_grad.detach().contiguous()
    return _Gram.apply(feat, res_grad)
