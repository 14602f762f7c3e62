"""k x k convolution (odd k <= 9, narrow channel counts) and bicubic upsampling on the HIP engine
(csrc/convk.hip): the ops of SRCNN (basicsr/archs/srcnn_arch.py: bicubic -> 9x9 -> 5x5 -> 5x5).

``convk(x, conv, act)`` applies an ``nn.Conv2d(cin, cout, k, 1, k // 2)`` parameter module to an NHWC
feature map, like ``conv3x3`` in ops/conv.py: the parameters stay the reference's, their GEMM images
come from ``prepared_images`` (so ``refresh_prepared`` keeps them current after every optimizer
step, also inside a captured step), and the weight gradient lands in the FlatParams gradient views
through ``grad_target`` / ``grad_ready``.  The weight gradient always runs on the current stream: with
``async_wgrad`` of any mode the results are the synchronous ones.

``bicubic_up_hp`` is the ``align_corners=False`` upsampler of L2SSingleModel.feed_data (fp32 NCHW in and
out, optionally into a channel range of a wider tensor).
"""
import torch

from .. import _lib
from ..utils import ktrace
from . import conv as C

KSIZES = (3, 5, 7, 9)
MAX_CH = 64


def _kdesc(dtype, N, H, W, k, cin_p, cin, cout_p, cout, act=_lib.ACT_NONE, alpha=1.0, scale=1.0, accumulate=0):
    d = _lib.ConvKDesc()
    d.dtype = _lib.dtype_code(dtype)
    d.N, d.H, d.W, d.k = N, H, W, k
    d.Cin, d.Cin_real, d.Cout, d.Cout_real = cin_p, cin, cout_p, cout
    d.act, d.alpha, d.scale, d.accumulate = act, alpha, scale, accumulate
    return d


def convk_fwd_raw(x, w_img, bias_g, k, cout_p, cout, act=_lib.ACT_NONE, alpha=1.0):
    """Launch sr_convk_fwd on a prepared GEMM image ``w_img`` [cout_p, k*k*cin_p]; returns y [N, H, W, cout_p]."""
    assert x.is_contiguous() and x.dim() == 4
    N, H, W, cin_p = x.shape
    assert w_img.dtype == x.dtype and tuple(w_img.shape) == (cout_p, k * k * cin_p), (w_img.shape, cout_p, k, cin_p)
    y = torch.empty(N, H, W, cout_p, device=x.device, dtype=x.dtype)
    d = _kdesc(x.dtype, N, H, W, k, cin_p, cin_p, cout_p, cout, act=act, alpha=alpha)
    lib = _lib.load()
    args = (d, _lib.ptr(x), _lib.ptr(w_img), _lib.ptr(bias_g), _lib.ptr(y), _lib.stream())
    if ktrace.active():
        esz, M = x.element_size(), N * H * W
        keep = (x, w_img, bias_g, y)
        with ktrace.span('convk_fwd_kernel', 2.0 * M * k * k * cin_p * cout_p,
                         esz * (M * cin_p + k * k * cin_p * cout_p + M * cout_p),
                         relaunch=lambda a=args, kp=keep: lib.sr_convk_fwd(*a[:-1], _lib.stream())):
            _lib.check(lib.sr_convk_fwd(*args))
    else:
        _lib.check(lib.sr_convk_fwd(*args))
    return y


def convk_wgrad_raw(dy, x, k, cin, cout, scale=1.0, need_bias=True, params=None):
    """Weight / bias gradient of a k x k conv in the nn.Conv2d parameter layout (fp32).  With
    ``params=(weight, bias)`` bound to a FlatParams buffer the kernel accumulates into their gradient
    views, fires the gradient-ready callbacks and returns ``(None, None)`` (as conv_wgrad_raw)."""
    assert dy.is_contiguous() and x.is_contiguous() and dy.dtype == x.dtype
    N, H, W, cin_p = x.shape
    cout_p = dy.shape[-1]
    tw = tb = None
    if params is not None:
        tw = C.grad_target(params[0])
        tb = C.grad_target(params[1]) if need_bias else None
        if tw is None or (need_bias and tb is None):
            tw = tb = None
    direct = tw is not None
    d = _kdesc(x.dtype, N, H, W, k, cin_p, cin, cout_p, cout, scale=scale, accumulate=int(direct))
    lib = _lib.load()
    ws_bytes = lib.sr_convk_wgrad_workspace(d)
    if ws_bytes == 0:
        raise ValueError(f'convk_wgrad: unsupported shape k={k} cin={cin_p} cout={cout_p} N={N} H={H} W={W}')
    ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
    if direct:
        dw, db = tw, tb
    else:
        dw = torch.empty(cout, cin, k, k, device=x.device, dtype=torch.float32)
        db = torch.empty(cout, device=x.device, dtype=torch.float32) if need_bias else None
    args = (d, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(ws), ws_bytes, _lib.ptr(dw), _lib.ptr(db), _lib.stream())
    if ktrace.active():
        # the relaunch closure must not accumulate into the live gradients
        scratch = (torch.empty_like(dw), torch.empty_like(db) if db is not None else None)
        rargs = args[:5] + (_lib.ptr(scratch[0]), _lib.ptr(scratch[1]))
        keep = (dy, x, ws, scratch)
        M = N * H * W
        nbytes = x.element_size() * M * (cin_p + cout_p) + (8 if direct else 4) * (k * k * cin * cout + cout)
        with ktrace.span('convk_wgrad_kernel+reduce', 2.0 * M * k * k * cin_p * cout_p, nbytes,
                         relaunch=lambda a=rargs, kp=keep: lib.sr_convk_wgrad(*a, _lib.stream()), launches=2):
            _lib.check(lib.sr_convk_wgrad(*args))
    else:
        _lib.check(lib.sr_convk_wgrad(*args))
    if direct:
        C.grad_ready(params[0])
        if need_bias:
            C.grad_ready(params[1])
        return None, None
    return dw, db


class _ConvK(torch.autograd.Function):
    """y = act(convk(x) + b) on NHWC maps, act none / ReLU."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        cout, cin, k, _ = weight.shape
        dtype = x.dtype
        cin_p, cout_p = x.shape[-1], C.pad8(cout)
        wf, _, bg = C.prepared_images(weight, bias, dtype, (cout, cin, cout_p, cin_p, 0, k))
        y = convk_fwd_raw(x, wf, bg, k, cout_p, cout, act=act)
        ctx.act, ctx.has_bias = act, bias is not None
        ctx.save_for_backward(x, weight, bias, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, y = ctx.saved_tensors
        cout, cin, k, _ = weight.shape
        dtype = x.dtype
        cin_p, cout_p = x.shape[-1], C.pad8(cout)
        dY = dy.to(dtype).contiguous()
        if ctx.act:
            dY = C.act_backward(dY, y, ctx.act, 0.0, 1.0)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            _, wd, _ = C.prepared_images(weight, bias, dtype, (cout, cin, cout_p, cin_p, 0, k))
            dx = convk_fwd_raw(dY, wd, None, k, cin_p, cin)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = convk_wgrad_raw(dY, x, k, cin, cout, need_bias=ctx.has_bias, params=(weight, bias))
        return dx, dw, db, None


def convk(x, conv, act=_lib.ACT_NONE):
    """Apply an nn.Conv2d(cin, cout, k, 1, k // 2) parameter module (odd k <= 9, at most 64 padded
    channels on either side) to an NHWC feature map [N, H, W, pad8(cin)]."""
    k = conv.kernel_size[0]
    if (tuple(conv.kernel_size) != (k, k) or k not in KSIZES or tuple(conv.stride) != (1, 1)
            or tuple(conv.padding) != (k // 2, k // 2) or tuple(conv.dilation) != (1, 1) or conv.groups != 1):
        raise ValueError(f'convk: needs a k x k conv with odd k in {KSIZES}, stride 1, padding k // 2, no dilation, '
                         f'no groups; got {conv}')
    if act not in (_lib.ACT_NONE, _lib.ACT_RELU):
        raise ValueError('convk: act must be ACT_NONE or ACT_RELU')
    if x.dim() != 4 or x.shape[-1] != C.pad8(conv.in_channels):
        raise ValueError(f'convk: x must be NHWC with {C.pad8(conv.in_channels)} channels, got {tuple(x.shape)}')
    if C.pad8(conv.in_channels) > MAX_CH or C.pad8(conv.out_channels) > MAX_CH:
        raise ValueError(f'convk: at most {MAX_CH} padded channels on either side')
    return _ConvK.apply(x.contiguous(), conv.weight, conv.bias, act)


def bicubic_up(x, scale, dtype, cp=None):
    """F.interpolate(x, scale_factor=scale, mode='bicubic', align_corners=True) of an fp32 NCHW image,
    returned as the NHWC feature map [N, H*scale, W*scale, cp] of ``dtype`` (padded channels zero).
    The gradient with respect to the image is not implemented."""
    if x.requires_grad:
        raise NotImplementedError('bicubic_up: the gradient with respect to the input image is not implemented '
                                  '(pass a tensor that does not require grad)')
    if int(scale) != scale or scale < 1:
        raise ValueError(f'bicubic_up: integer scale >= 1, got {scale}')
    scale = int(scale)
    N, Cc, H, W = x.shape
    cp = cp or C.pad8(Cc)
    xc = x.detach().contiguous().float()
    y = torch.empty(N, H * scale, W * scale, cp, device=x.device, dtype=dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(dtype), _lib.ptr(xc), N, Cc, H, W, scale, cp, _lib.ptr(y), _lib.stream())
    if ktrace.active():
        keep = (xc, y)
        with ktrace.span('bicubic_up_kernel', 32.0 * y.numel() / cp * Cc, 4 * xc.numel() + y.element_size() * y.numel(),
                         relaunch=lambda a=args, kp=keep: lib.sr_bicubic_up(*a[:-1], _lib.stream())):
            _lib.check(lib.sr_bicubic_up(*args))
    else:
        _lib.check(lib.sr_bicubic_up(*args))
    return y


def bicubic_up_hp(x, scale, out=None, c0=0):
    """F.interpolate(x, scale_factor=scale, mode='bicubic') (align_corners=False) of an fp32 NCHW tensor by
    an integer scale, fp32 NCHW out.  With ``out`` [N, Cy, H*scale, W*scale] (fp32, contiguous) the result
    is written into its channels [c0, c0 + C) and the others are left alone (a fused ``torch.cat``).
    The gradient with respect to the image is not implemented."""
    if x.requires_grad:
        raise NotImplementedError('bicubic_up_hp: the gradient with respect to the input image is not implemented '
                                  '(pass a tensor that does not require grad)')
    if int(scale) != scale or scale < 1:
        raise ValueError(f'bicubic_up_hp: integer scale >= 1, got {scale}')
    scale = int(scale)
    N, Cc, H, W = x.shape
    xc = x.detach().contiguous().float()
    if out is None:
        out = torch.empty(N, Cc, H * scale, W * scale, device=x.device, dtype=torch.float32)
        c0 = 0
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 4 or out.device != x.device
          or (out.shape[0], out.shape[2], out.shape[3]) != (N, H * scale, W * scale)):
        raise ValueError(f'bicubic_up_hp: out must be a contiguous fp32 [{N}, Cy, {H * scale}, {W * scale}] tensor on '
                         f'{x.device}, got {out.dtype} {tuple(out.shape)}')
    lib = _lib.load()
    args = (_lib.ptr(xc), N, Cc, H, W, scale, _lib.ptr(out), out.shape[1], int(c0), _lib.stream())
    if ktrace.active():
        keep = (xc, out)
        with ktrace.span('bicubic_up_hp_kernel', 32.0 * xc.numel() * scale * scale, 4 * xc.numel() * (1 + scale * scale),
                         relaunch=lambda a=args, kp=keep: lib.sr_bicubic_up_hp(*a[:-1], _lib.stream())):
            _lib.check(lib.sr_bicubic_up_hp(*args))
    else:
        _lib.check(lib.sr_bicubic_up_hp(*args))
    return out
