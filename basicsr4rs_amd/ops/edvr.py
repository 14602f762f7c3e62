"""Ops of EDVR (basicsr/archs/edvr_arch.py) on the HIP kernels of csrc/edvr.hip.

``conv3s2(x, conv, act, slope)``: an ``nn.Conv2d(cin, cout, 3, 2, 1)`` parameter module on an NHWC feature map, with
the bias and an optional LeakyReLU in the epilogue.  The GEMM images of the weight are cached on the parameter and
rebuilt when its ``_version`` or the parameter epoch (ops/conv.py) changes; the weight and bias gradients land in the
FlatParams gradient views through ``grad_target`` / ``grad_ready`` and are not launched for a frozen parameter.
``pool3s2(x)``: ``cat([MaxPool2d(3, 2, 1)(x), AvgPool2d(3, 2, 1)(x)], channel)`` in one pass.
``tsa_corr(emb, emb_ref, aligned)``: the temporal attention of TSAFusion, the aligned frames weighted by
``sigmoid(<emb, emb_ref>)`` and stored as the ``[B, H, W, T * C]`` map the fusion convs read.
``tsa_modulate(feat, attn, attn_add)``: ``feat * sigmoid(attn) * 2 + attn_add``.
``conv1x1(x, conv, act, slope)``: an ``nn.Conv2d(cin, cout, 1)`` on the conv engine's 1 x 1 GEMM (the fusion and attention
convs of TSAFusion); ``leaky_relu(x, slope)``: the LeakyReLU behind a deformable conv, a pass of its own.
The scaled bilinear x2 of PCD (``upsample(offset) * 2``) is ``bilinear_up2(x, scale)`` of ops/gan.py.

Every launch runs under a ``ktrace.span`` with the kernel name and its algorithmic FLOPs / bytes.
"""
import torch

from .. import _lib
from . import conv as C
from .blocks import channel_reduce
from .fused_act import fused_bias_act
from .gan import _check_map
from .perceptual import _launch


def out_size(n):
    """Output size of a 3 x 3 window with stride 2 and padding 1."""
    return (n - 1) // 2 + 1


# --------------------------------------------------------------------------------------------- conv 3x3 s2


def conv3s2_images(weight, dtype):
    """(wf, wd) GEMM images of a [cout, cin, 3, 3] weight in ``dtype``, cached on the parameter and rebuilt in
    place when the weight's ``_version`` or the parameter epoch moved (as ``conv4s2_images`` of ops/gan.py)."""
    cout, cin = weight.shape[:2]
    cout_p, cin_p = C.pad8(cout), C.pad8(cin)
    skey = (dtype, weight.data_ptr())
    ents = weight.__dict__.setdefault('_sr_prep3s2', {})
    dyn = (weight._version, C._PARAM_EPOCH[0])
    e = ents.get(skey)
    if e is not None and e[0] == dyn:
        return e[1]
    if e is None:
        val = (torch.empty(cout_p, 9 * cin_p, device=weight.device, dtype=dtype),
               torch.empty(9 * cin_p * cout_p, device=weight.device, dtype=dtype))
    else:
        val = e[1]
    lib = _lib.load()
    w = weight.detach()
    args = (_lib.dtype_code(dtype), _lib.ptr(w), cout, cin, cout_p, cin_p, _lib.ptr(val[0]), _lib.ptr(val[1]),
            _lib.stream())
    _launch('conv3s2_prep_kernel', 0.0, 4 * weight.numel() + val[0].element_size() * 2 * cout_p * 9 * cin_p,
            lib.sr_conv3s2_prep, args, (w, val))
    ents[skey] = (dyn, val)
    return val


def conv3s2_fwd_raw(x, wf, bias, cout, act=_lib.ACT_NONE, slope=0.0):
    N, H, W, cin_p = x.shape
    cout_p = C.pad8(cout)
    y = torch.empty(N, out_size(H), out_size(W), cout_p, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(x.dtype), _lib.ptr(x), _lib.ptr(wf), _lib.ptr(bias), N, H, W, cin_p, cout_p, cout, act,
            float(slope), _lib.ptr(y), _lib.stream())
    _launch('conv3s2_fwd_kernel', 2.0 * y.numel() * 9 * cin_p, x.element_size() * (x.numel() + wf.numel() + y.numel()),
            lib.sr_conv3s2_fwd, args, (x, wf, bias, y))
    return y


def conv3s2_dgrad_raw(dy, wd, H, W, cin_p):
    N, Ho, Wo, cout_p = dy.shape
    dx = torch.empty(N, H, W, cin_p, device=dy.device, dtype=dy.dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(dy.dtype), _lib.ptr(dy), _lib.ptr(wd), N, H, W, cin_p, cout_p, _lib.ptr(dx), _lib.stream())
    # 9 tap products per 4 input pixels: the forward's products, none of them a zero
    _launch('conv3s2_dgrad_kernel', 2.0 * dx.numel() * 9 / 4 * cout_p,
            dy.element_size() * (dx.numel() + wd.numel() + dy.numel()), lib.sr_conv3s2_dgrad, args, (dy, wd, dx))
    return dx


def conv3s2_wgrad_raw(dy, x, cin, cout, scale=1.0, param=None):
    """Weight gradient [cout, cin, 3, 3] fp32.  With ``param`` bound to a FlatParams buffer the reduce
    accumulates into its gradient view, fires the gradient-ready callbacks and ``None`` is returned."""
    N, H, W, cin_p = x.shape
    cout_p = dy.shape[-1]
    target = C.grad_target(param) if param is not None else None
    direct = target is not None
    lib = _lib.load()
    ws_bytes = lib.sr_conv3s2_wgrad_workspace(N, H, W, cin_p, cout_p)
    ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
    dw = target if direct else torch.empty(cout, cin, 3, 3, device=x.device, dtype=torch.float32)

    def args(out, acc):
        return (_lib.dtype_code(x.dtype), _lib.ptr(dy), _lib.ptr(x), N, H, W, cin_p, cin, cout_p, cout, float(scale), acc,
                _lib.ptr(out), _lib.ptr(ws), ws_bytes)

    # the relaunch of a trace must not accumulate into the live gradient
    scratch = torch.empty(cout, cin, 3, 3, device=x.device, dtype=torch.float32) if C.ktrace.active() and direct else dw
    M = N * out_size(H) * out_size(W)
    fn = lib.sr_conv3s2_wgrad
    if C.ktrace.active():
        with C.ktrace.span('conv3s2_wgrad_kernel+reduce', 2.0 * M * 9 * cin_p * cout_p,
                           x.element_size() * (x.numel() + dy.numel()) + 2 * ws_bytes + 4 * dw.numel(),
                           relaunch=lambda a=args(scratch, 0), k=(dy, x, ws, scratch): fn(*a, _lib.stream()), launches=2):
            _lib.check(fn(*args(dw, int(direct)), _lib.stream()))
    else:
        _lib.check(fn(*args(dw, int(direct)), _lib.stream()))
    if direct:
        C.grad_ready(param)
        return None
    return dw


def conv3s2_bgrad_raw(dy, cout, param=None):
    """Bias gradient [cout] fp32 by the channel reduce over all N Ho Wo pixels; accumulated into the FlatParams
    gradient view of ``param`` when it has one (``None`` is returned then)."""
    N, Ho, Wo, cout_p = dy.shape
    db = channel_reduce(dy.view(1, N * Ho, Wo, cout_p))[0, :cout]
    target = C.grad_target(param) if param is not None else None
    if target is None:
        return db
    target.add_(db)
    C.grad_ready(param)
    return None


class _Conv3s2(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        cout = weight.shape[0]
        wf, _ = conv3s2_images(weight, x.dtype)
        y = conv3s2_fwd_raw(x, wf, bias.detach() if bias is not None else None, cout, act, slope)
        ctx.cfg = (act, slope)
        ctx.save_for_backward(x, weight, bias, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, y = ctx.saved_tensors
        act, slope = ctx.cfg
        cout, cin = weight.shape[:2]
        dY = dy.to(x.dtype).contiguous()
        if act:
            dY = C.act_backward(dY, y, act, slope, 1.0)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv3s2_dgrad_raw(dY, conv3s2_images(weight, x.dtype)[1], x.shape[1], x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1]:
            dw = conv3s2_wgrad_raw(dY, x, cin, cout, param=weight)
        if bias is not None and ctx.needs_input_grad[2]:
            db = conv3s2_bgrad_raw(dY, cout, param=bias)
        return dx, dw, db, None, None


def conv3s2(x, conv, act=_lib.ACT_NONE, slope=0.1):
    """Apply an nn.Conv2d(cin, cout, 3, 2, 1) parameter module (with or without a bias) to an NHWC feature map
    [N, H, W, pad8(cin)], H and W at least 2 and of either parity; returns [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1,
    pad8(cout)].  ``act``: ACT_NONE or a fused LeakyReLU(slope)."""
    if (tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (2, 2) or tuple(conv.padding) != (1, 1)
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != 'zeros'):
        raise ValueError(f'conv3s2: needs a 3 x 3 conv with stride 2, padding 1, no dilation or groups; got {conv}')
    if act not in (_lib.ACT_NONE, _lib.ACT_LRELU):
        raise ValueError('conv3s2: act must be ACT_NONE or ACT_LRELU')
    _check_map(x, 'conv3s2', C.pad8(conv.in_channels))
    if x.shape[1] < 2 or x.shape[2] < 2:
        raise ValueError(f'conv3s2: H and W must be at least 2, got {tuple(x.shape)}')
    if C.pad8(conv.in_channels) > 512 or C.pad8(conv.out_channels) > 512:
        raise ValueError(f'conv3s2: at most 512 padded channels on either side, got {conv}')
    return _Conv3s2.apply(x.contiguous(), conv.weight, conv.bias, act, slope)


# ------------------------------------------------------------------------------------------- pooling 3x3 s2


def pool3s2_fwd_raw(x):
    N, H, W, Cc = x.shape
    y = torch.empty(N, out_size(H), out_size(W), 2 * Cc, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(x.dtype), _lib.ptr(x), N, H, W, Cc, _lib.ptr(y), _lib.stream())
    # 9 comparisons and 9 adds per output pixel and channel; x read once (9 / 4 times, the rest from cache)
    _launch('pool3s2_fwd_kernel', 9.0 * y.numel(), x.element_size() * (x.numel() + y.numel()), lib.sr_pool3s2_fwd, args,
            (x, y))
    return y


def pool3s2_bwd_raw(x, dy):
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    lib = _lib.load()
    args = (_lib.dtype_code(x.dtype), _lib.ptr(x), _lib.ptr(dy), N, H, W, Cc, _lib.ptr(dx), _lib.stream())
    _launch('pool3s2_bwd_kernel', 9.0 * dy.numel(), x.element_size() * (2 * x.numel() + dy.numel()), lib.sr_pool3s2_bwd,
            args, (x, dy, dx))
    return dx


class _Pool3s2(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return pool3s2_fwd_raw(x)

    @staticmethod
    def backward(ctx, dy):
        (x, ) = ctx.saved_tensors
        return pool3s2_bwd_raw(x, dy.to(x.dtype).contiguous())


def pool3s2(x):
    """``torch.cat([MaxPool2d(3, 2, 1)(x), AvgPool2d(3, 2, 1)(x)], channel)`` of an NHWC map [N, H, W, C] in one
    pass: [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, 2C].  The backward recomputes each window's choice from ``x``."""
    _check_map(x, 'pool3s2')
    return _Pool3s2.apply(x.contiguous())


# --------------------------------------------------------------------------------------- temporal attention


def tsa_corr_fwd_raw(emb, emb_ref, aligned):
    BT, H, W, Cc = emb.shape
    B = emb_ref.shape[0]
    T = BT // B
    out = torch.empty(B, H, W, T * Cc, device=emb.device, dtype=emb.dtype)
    prob = torch.empty(B, T, H, W, device=emb.device, dtype=torch.float32)
    lib = _lib.load()
    args = (_lib.dtype_code(emb.dtype), _lib.ptr(emb), _lib.ptr(emb_ref), _lib.ptr(aligned), B, T, H, W, Cc,
            _lib.ptr(out), _lib.ptr(prob), _lib.stream())
    _launch('tsa_corr_fwd_kernel', 3.0 * emb.numel(),
            emb.element_size() * (2 * emb.numel() + emb_ref.numel() + out.numel()) + 4 * prob.numel(),
            lib.sr_tsa_corr_fwd, args, (emb, emb_ref, aligned, out, prob))
    return out, prob


def tsa_corr_bwd_raw(d_out, emb, emb_ref, aligned, prob):
    BT, H, W, Cc = emb.shape
    B, T = prob.shape[:2]
    d_aligned, d_emb, d_ref = torch.empty_like(aligned), torch.empty_like(emb), torch.empty_like(emb_ref)
    lib = _lib.load()
    args = (_lib.dtype_code(emb.dtype), _lib.ptr(d_out), _lib.ptr(emb), _lib.ptr(emb_ref), _lib.ptr(aligned),
            _lib.ptr(prob), B, T, H, W, Cc, _lib.ptr(d_aligned), _lib.ptr(d_emb), _lib.ptr(d_ref), _lib.stream())
    _launch('tsa_corr_bwd_kernel', 7.0 * emb.numel(),
            emb.element_size() * (5 * emb.numel() + 2 * emb_ref.numel()) + 4 * prob.numel(), lib.sr_tsa_corr_bwd, args,
            (d_out, emb, emb_ref, aligned, prob, d_aligned, d_emb, d_ref))
    return d_aligned, d_emb, d_ref


class _TsaCorr(torch.autograd.Function):

    @staticmethod
    def forward(ctx, emb, emb_ref, aligned):
        out, prob = tsa_corr_fwd_raw(emb, emb_ref, aligned)
        ctx.save_for_backward(emb, emb_ref, aligned, prob)
        ctx.mark_non_differentiable(prob)
        return out, prob

    @staticmethod
    def backward(ctx, d_out, _d_prob):
        emb, emb_ref, aligned, prob = ctx.saved_tensors
        d_aligned, d_emb, d_ref = tsa_corr_bwd_raw(d_out.to(emb.dtype).contiguous(), emb, emb_ref, aligned, prob)
        return d_emb, d_ref, d_aligned


def tsa_corr(emb, emb_ref, aligned):
    """Temporal attention of TSAFusion on NHWC maps: ``emb`` and ``aligned`` [B * T, H, W, C], ``emb_ref``
    [B, H, W, C].  Returns (out [B, H, W, T * C], prob [B, T, H, W] fp32) with prob = sigmoid(sum_c emb * emb_ref) and
    out[..., t * C + c] = aligned[b * T + t, ..., c] * prob[b, t]; ``prob`` carries no gradient."""
    _check_map(emb, 'tsa_corr')
    _check_map(emb_ref, 'tsa_corr', emb.shape[-1])
    if (aligned.shape != emb.shape or aligned.dtype != emb.dtype or emb_ref.dtype != emb.dtype
            or emb.shape[0] % emb_ref.shape[0] or emb_ref.shape[1:] != emb.shape[1:] or emb.shape[-1] > 512):
        raise ValueError(f'tsa_corr: emb / aligned [B * T, H, W, C <= 512] and emb_ref [B, H, W, C] of one dtype are '
                         f'expected, got {tuple(emb.shape)}, {tuple(aligned.shape)}, {tuple(emb_ref.shape)}')
    return _TsaCorr.apply(emb.contiguous(), emb_ref.contiguous(), aligned.contiguous())


def tsa_modulate_fwd_raw(feat, attn, attn_add):
    y = torch.empty_like(feat)
    lib = _lib.load()
    args = (_lib.dtype_code(feat.dtype), _lib.ptr(feat), _lib.ptr(attn), _lib.ptr(attn_add), feat.numel(), _lib.ptr(y),
            _lib.stream())
    _launch('tsa_mod_fwd_kernel', 6.0 * feat.numel(), 4 * feat.element_size() * feat.numel(), lib.sr_tsa_modulate_fwd,
            args, (feat, attn, attn_add, y))
    return y


def tsa_modulate_bwd_raw(dy, feat, attn):
    d_feat, d_attn = torch.empty_like(feat), torch.empty_like(attn)
    lib = _lib.load()
    args = (_lib.dtype_code(feat.dtype), _lib.ptr(dy), _lib.ptr(feat), _lib.ptr(attn), feat.numel(), _lib.ptr(d_feat),
            _lib.ptr(d_attn), _lib.stream())
    _launch('tsa_mod_bwd_kernel', 8.0 * feat.numel(), 5 * feat.element_size() * feat.numel(), lib.sr_tsa_modulate_bwd,
            args, (dy, feat, attn, d_feat, d_attn))
    return d_feat, d_attn


class _TsaModulate(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feat, attn, attn_add):
        ctx.save_for_backward(feat, attn)
        return tsa_modulate_fwd_raw(feat, attn, attn_add)

    @staticmethod
    def backward(ctx, dy):
        feat, attn = ctx.saved_tensors
        dy = dy.to(feat.dtype).contiguous()
        d_feat, d_attn = tsa_modulate_bwd_raw(dy, feat, attn)
        return d_feat, d_attn, dy


def tsa_modulate(feat, attn, attn_add):
    """``feat * sigmoid(attn) * 2 + attn_add`` of three NHWC maps of one shape and dtype, one pass each way."""
    _check_map(feat, 'tsa_modulate')
    if attn.shape != feat.shape or attn_add.shape != feat.shape or attn.dtype != feat.dtype or attn_add.dtype != feat.dtype:
        raise ValueError(f'tsa_modulate: three maps of one shape and dtype are expected, got {tuple(feat.shape)}, '
                         f'{tuple(attn.shape)}, {tuple(attn_add.shape)}')
    return _TsaModulate.apply(feat.contiguous(), attn.contiguous(), attn_add.contiguous())


# ----------------------------------------------------------------------------------- 1 x 1 conv, LeakyReLU


class _Conv1x1(torch.autograd.Function):
    """y = act(conv1x1(x) + b) on NHWC maps through the conv engine's ksize-1 GEMM, act none / LeakyReLU."""

    @staticmethod
    def _shape(x, weight):
        cout, cin = weight.shape[:2]
        return (cout, cin, C.pad8(cout), x.shape[-1], 0, 1)

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        N, H, W, cin_p = x.shape
        shape = _Conv1x1._shape(x, weight)
        cout, cout_p = shape[0], shape[2]
        wf, _, bg = C.prepared_images(weight, bias, x.dtype, shape)
        y = torch.empty(N, H, W, cout_p, device=x.device, dtype=x.dtype)
        C.conv_fwd_raw(x, wf, bg if bias is not None else None, y, N, H, W, cin_p, cout_p, cout, ksize=1, act=act,
                       slope=float(slope))
        ctx.cfg = (act, slope)
        ctx.save_for_backward(x, weight, bias, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, y = ctx.saved_tensors
        act, slope = ctx.cfg
        N, H, W, cin_p = x.shape
        shape = _Conv1x1._shape(x, weight)
        cout, cin, cout_p = shape[:3]
        dY = dy.to(x.dtype).contiguous()
        if act:
            dY = C.act_backward(dY, y, act, slope, 1.0)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wd = C.prepared_images(weight, bias, x.dtype, shape)[1]
            dx = torch.empty_like(x)
            C.conv_fwd_raw(dY, wd, None, dx, N, H, W, cout_p, cin_p, cin_p, ksize=1)
        need_b = bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or need_b:
            dw, db = C.conv_wgrad_raw(dY, x, N, H, W, cin_p, cin, cout_p, cout, ksize=1, need_bias=bias is not None,
                                      params=(weight, bias))
        return dx, dw, db, None, None


def conv1x1(x, conv, act=_lib.ACT_NONE, slope=0.1):
    """Apply an nn.Conv2d(cin, cout, 1) parameter module to an NHWC feature map [N, H, W, pad8(cin)]; ``act``:
    ACT_NONE or a fused LeakyReLU(slope)."""
    if (tuple(conv.kernel_size) != (1, 1) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (0, 0)
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1):
        raise ValueError(f'conv1x1: needs a 1 x 1 conv with stride 1 and no padding, dilation or groups; got {conv}')
    if act not in (_lib.ACT_NONE, _lib.ACT_LRELU):
        raise ValueError('conv1x1: act must be ACT_NONE or ACT_LRELU')
    _check_map(x, 'conv1x1', C.pad8(conv.in_channels))
    return _Conv1x1.apply(x.contiguous(), conv.weight, conv.bias, act, slope)


class _LeakyRelu(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, slope):
        y = fused_bias_act(x, None, None, 3, 0, slope, 1.0)
        ctx.slope = slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y, ) = ctx.saved_tensors
        return C.act_backward(dy.to(y.dtype).contiguous(), y, _lib.ACT_LRELU, ctx.slope, 1.0), None


def leaky_relu(x, slope=0.1):
    """LeakyReLU as a pass of its own (sr_fused_bias_act / sr_act_backward): behind a deformable conv, whose
    kernels have no activation epilogue."""
    return _LeakyRelu.apply(x, float(slope))
