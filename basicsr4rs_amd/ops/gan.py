"""Ops of GAN training on the HIP kernels of csrc/gan.hip, csrc/unet_disc.hip and csrc/loss.hip: the building
blocks of the VGGStyleDiscriminator and the UNetDiscriminatorSN (basicsr/archs/discriminator_arch.py) and the GANLoss
(basicsr/losses/gan_loss.py).

``conv4s2(x, conv)``: an ``nn.Conv2d(cin, cout, 4, 2, 1, bias=False)`` parameter module on an NHWC feature map.
The GEMM images of the weight are cached on the parameter and rebuilt when its ``_version`` or the parameter
epoch (ops/conv.py) changes; the weight gradient lands in the FlatParams gradient view through
``grad_target`` / ``grad_ready`` and is not launched for a weight that does not require grad.
``conv4s2(x, conv, act, slope, weight)`` fuses a LeakyReLU and takes a weight override (per-call images).
``spectral_norm_group(convs, training)``: every spectral-normalised weight of a net from one grouped launch sequence.
``bilinear_up2(x, scale)``: bilinear x2 (align_corners=False) of an NHWC map times an optional scale, forward and
backward.
``batch_norm_act(x, bn, act, slope)``: ``nn.BatchNorm2d`` (affine, tracked running statistics) with an optional
fused LeakyReLU, in the module's training or eval mode; statistics, gamma, beta and their gradients are fp32.
``linear(x, lin, act, slope, spatial)``: a head ``nn.Linear`` on its fp32 parameters; ``spatial`` = H * W of the
NHWC map that ``x`` flattens, so the reference's NCHW-flatten weight is used as it is.
``gan_loss(pred, kind, ...)``: the mean GAN loss of a prediction and its gradient in one pass.

Every launch runs under a ``ktrace.span`` with the kernel name and its algorithmic FLOPs / bytes.
"""
import torch

from .. import _lib
from . import conv as C
from .perceptual import _launch

GAN_KINDS = {'vanilla': 0, 'lsgan': 1, 'wgan': 2, 'wgan_softplus': 3, 'hinge': 4}
_CPU_MESSAGE = 'basicsr4rs_amd HIP ops need tensors on the MI355X (cuda) device'


def _check_map(x, what, channels=None):
    if not x.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if x.dim() != 4 or x.shape[-1] % 8 or (channels is not None and x.shape[-1] != channels):
        want = f'{channels}' if channels is not None else 'a multiple of 8'
        raise ValueError(f'{what}: an NHWC map with {want} channels is expected, got {tuple(x.shape)}')
    _lib.dtype_code(x.dtype)


# --------------------------------------------------------------------------------------------- conv 4x4 s2


def conv4s2_images(weight, dtype):
    """(wf, wd) GEMM images of a [cout, cin, 4, 4] weight in ``dtype``, cached on the parameter and rebuilt in
    place when the weight's ``_version`` or the parameter epoch moved (as ``prepared_images`` of ops/conv.py)."""
    cout, cin = weight.shape[:2]
    cout_p, cin_p = C.pad8(cout), C.pad8(cin)
    skey = (dtype, weight.data_ptr())
    ents = weight.__dict__.setdefault('_sr_prep4', {})
    dyn = (weight._version, C._PARAM_EPOCH[0])
    e = ents.get(skey)
    if e is not None and e[0] == dyn:
        return e[1]
    if e is None:
        val = (torch.empty(cout_p, 16 * cin_p, device=weight.device, dtype=dtype),
               torch.empty(4, cin_p, 4 * cout_p, device=weight.device, dtype=dtype))
    else:
        val = e[1]
    lib = _lib.load()
    w = weight.detach()
    args = (_lib.dtype_code(dtype), _lib.ptr(w), cout, cin, cout_p, cin_p, _lib.ptr(val[0]), _lib.ptr(val[1]),
            _lib.stream())
    n = 2 * cout_p * 16 * cin_p
    _launch('conv4s2_prep_kernel', 0.0, 4 * weight.numel() + val[0].element_size() * n, lib.sr_conv4s2_prep, args,
            (w, val))
    ents[skey] = (dyn, val)
    return val


def conv4s2_fresh_images(weight, dtype):
    """(wf, wd) built for this call alone by one prep launch, nothing cached on ``weight`` (a tensor that is new
    every forward: a spectral-normalised weight)."""
    cout, cin = weight.shape[:2]
    cout_p, cin_p = C.pad8(cout), C.pad8(cin)
    val = (torch.empty(cout_p, 16 * cin_p, device=weight.device, dtype=dtype),
           torch.empty(4, cin_p, 4 * cout_p, device=weight.device, dtype=dtype))
    lib = _lib.load()
    w = weight.detach()
    args = (_lib.dtype_code(dtype), _lib.ptr(w), cout, cin, cout_p, cin_p, _lib.ptr(val[0]), _lib.ptr(val[1]),
            _lib.stream())
    _launch('conv4s2_prep_kernel', 0.0, 4 * weight.numel() + val[0].element_size() * 2 * cout_p * 16 * cin_p,
            lib.sr_conv4s2_prep, args, (w, val))
    return val


def conv4s2_fwd_raw(x, wf, cout_p, act=_lib.ACT_NONE, slope=0.0):
    N, H, W, cin_p = x.shape
    y = torch.empty(N, H // 2, W // 2, cout_p, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    head = (_lib.dtype_code(x.dtype), _lib.ptr(x), _lib.ptr(wf), N, H, W, cin_p, cout_p)
    if act == _lib.ACT_NONE:
        fn, args = lib.sr_conv4s2_fwd, head + (_lib.ptr(y), _lib.stream())
    else:
        fn, args = lib.sr_conv4s2_fwd_act, head + (act, float(slope), _lib.ptr(y), _lib.stream())
    _launch('conv4s2_fwd_kernel', 2.0 * y.numel() * 16 * cin_p, x.element_size() * (x.numel() + wf.numel() + y.numel()),
            fn, args, (x, wf, y))
    return y


def conv4s2_dgrad_raw(dy, wd, H, W, cin_p):
    N, Ho, Wo, cout_p = dy.shape
    dx = torch.empty(N, H, W, cin_p, device=dy.device, dtype=dy.dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(dy.dtype), _lib.ptr(dy), _lib.ptr(wd), N, H, W, cin_p, cout_p, _lib.ptr(dx), _lib.stream())
    # 4 taps per input pixel and parity class: the 16 tap products of the forward, none of them a zero
    _launch('conv4s2_dgrad_kernel', 2.0 * dx.numel() * 4 * cout_p,
            dy.element_size() * (dx.numel() + wd.numel() + dy.numel()), lib.sr_conv4s2_dgrad, args, (dy, wd, dx))
    return dx


def conv4s2_wgrad_raw(dy, x, cin, cout, scale=1.0, param=None):
    """Weight gradient [cout, cin, 4, 4] fp32.  With ``param`` bound to a FlatParams buffer the reduce
    accumulates into its gradient view, fires the gradient-ready callbacks and ``None`` is returned."""
    N, H, W, cin_p = x.shape
    cout_p = dy.shape[-1]
    target = C.grad_target(param) if param is not None else None
    direct = target is not None
    lib = _lib.load()
    ws_bytes = lib.sr_conv4s2_wgrad_workspace(N, H, W, cin_p, cout_p)
    ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
    dw = target if direct else torch.empty(cout, cin, 4, 4, device=x.device, dtype=torch.float32)

    def args(out, acc):
        return (_lib.dtype_code(x.dtype), _lib.ptr(dy), _lib.ptr(x), N, H, W, cin_p, cin, cout_p, cout, float(scale), acc,
                _lib.ptr(out), _lib.ptr(ws), ws_bytes)

    # the relaunch of a trace must not accumulate into the live gradient
    scratch = torch.empty(cout, cin, 4, 4, device=x.device, dtype=torch.float32) if C.ktrace.active() and direct else dw
    M = N * (H // 2) * (W // 2)
    fn = lib.sr_conv4s2_wgrad
    if C.ktrace.active():
        with C.ktrace.span('conv4s2_wgrad_kernel+reduce', 2.0 * M * 16 * cin_p * cout_p,
                           x.element_size() * (x.numel() + dy.numel()) + 2 * ws_bytes + 4 * dw.numel(),
                           relaunch=lambda a=args(scratch, 0), k=(dy, x, ws, scratch): fn(*a, _lib.stream()), launches=2):
            _lib.check(fn(*args(dw, int(direct)), _lib.stream()))
    else:
        _lib.check(fn(*args(dw, int(direct)), _lib.stream()))
    if direct:
        C.grad_ready(param)
        return None
    return dw


class _Conv4s2(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, act=_lib.ACT_NONE, slope=0.2, cache=True):
        cout = weight.shape[0]
        wf, wd = conv4s2_images(weight, x.dtype) if cache else conv4s2_fresh_images(weight, x.dtype)
        y = conv4s2_fwd_raw(x, wf, C.pad8(cout), act, slope)
        ctx.cfg = (act, slope)
        ctx.wd = None if cache else wd
        ctx.save_for_backward(x, weight, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        act, slope = ctx.cfg
        cout, cin = weight.shape[:2]
        dY = dy.to(x.dtype).contiguous()
        if act:
            dY = C.act_backward(dY, y, act, slope, 1.0)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wd = ctx.wd if ctx.wd is not None else conv4s2_images(weight, x.dtype)[1]
            dx = conv4s2_dgrad_raw(dY, wd, x.shape[1], x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1]:
            dw = conv4s2_wgrad_raw(dY, x, cin, cout, param=weight)
        return dx, dw, None, None, None


def conv4s2(x, conv, act=_lib.ACT_NONE, slope=0.2, weight=None):
    """Apply an nn.Conv2d(cin, cout, 4, 2, 1, bias=False) parameter module to an NHWC feature map
    [N, H, W, pad8(cin)] with even H and W; returns [N, H / 2, W / 2, pad8(cout)].  ``act``: ACT_NONE or a fused
    LeakyReLU(slope).  ``weight``: a tensor used in place of ``conv.weight`` (a spectral-normalised weight); its
    GEMM images are then built for this call alone and nothing is cached."""
    if (tuple(conv.kernel_size) != (4, 4) or tuple(conv.stride) != (2, 2) or tuple(conv.padding) != (1, 1)
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.bias is not None
            or conv.padding_mode != 'zeros'):
        raise ValueError(f'conv4s2: needs a 4 x 4 conv with stride 2, padding 1, no dilation, groups or bias; got {conv}')
    if act not in (_lib.ACT_NONE, _lib.ACT_LRELU):
        raise ValueError('conv4s2: act must be ACT_NONE or ACT_LRELU')
    _check_map(x, 'conv4s2', C.pad8(conv.in_channels))
    if x.shape[1] % 2 or x.shape[2] % 2 or x.shape[1] < 2 or x.shape[2] < 2:
        raise ValueError(f'conv4s2: H and W must be even and at least 2, got {tuple(x.shape)}')
    if C.pad8(conv.in_channels) > 512 or C.pad8(conv.out_channels) > 512:
        raise ValueError(f'conv4s2: at most 512 padded channels on either side, got {conv}')
    if weight is None:
        return _Conv4s2.apply(x.contiguous(), conv.weight, act, slope, True)
    if tuple(weight.shape) != (conv.out_channels, conv.in_channels, 4, 4) or weight.dtype != torch.float32:
        raise ValueError(f'conv4s2: the weight override must be fp32 {(conv.out_channels, conv.in_channels, 4, 4)}')
    return _Conv4s2.apply(x.contiguous(), weight.contiguous(), act, slope, False)


# ------------------------------------------------------------------------------------------- spectral norm


def _sn_layout(shapes):
    """Offsets (in floats, multiples of 4) of W, u, v, sigma of every problem in one forward's state buffer."""
    offs, o = [], 0
    for R, K in shapes:
        ow = o
        ou = ow + (R * K + 3) // 4 * 4
        ov = ou + (R + 3) // 4 * 4
        osig = ov + (K + 3) // 4 * 4
        o = osig + 4
        offs.append((ow, ou, ov, osig))
    return offs, o


def _sn_call(fn_name, probs, extra, device):
    """One grouped launch sequence per chunk of at most SN_MAX_PROBLEMS problems."""
    lib = _lib.load()
    fn = getattr(lib, fn_name)
    calls = []
    for c0 in range(0, len(probs), _lib.SN_MAX_PROBLEMS):
        chunk = probs[c0:c0 + _lib.SN_MAX_PROBLEMS]
        arr = (_lib.SnProblem * len(chunk))(*chunk)
        ws_bytes = lib.sr_spectral_norm_workspace(arr, len(chunk))
        ws = torch.empty(ws_bytes // 4, device=device, dtype=torch.float32)
        calls.append((fn, (arr, len(chunk)) + extra + (_lib.ptr(ws), ws_bytes), ws))
    return calls


def _sn_problem(w, u, v, state, off, R, K, out=None, g=None):
    p = _lib.SnProblem()
    base = state.data_ptr()
    p.w, p.u, p.v = w.data_ptr(), (u.data_ptr() if u is not None else None), (v.data_ptr() if v is not None else None)
    p.u_fwd, p.v_fwd, p.sigma = base + 4 * off[1], base + 4 * off[2], base + 4 * off[3]
    p.out = out.data_ptr() if out is not None else None
    p.g = g.data_ptr() if g is not None else None
    p.R, p.K = R, K
    return p


def spectral_norm_fwd_raw(weights, bufs, training, eps=1e-12):
    """One grouped forward over fp32 ``weights`` [cout, ...] with ``bufs`` = [(u, v), ...] (updated in place when
    ``training``).  Returns (outs, state, layout): the normalised weights (views of ``state``), this forward's state
    buffer (W, u, v, sigma of every problem) and ``layout`` = (shapes, offsets) into it (``sn_state``)."""
    shapes = [(w.shape[0], w[0].numel()) for w in weights]
    offs, total = _sn_layout(shapes)
    dev = weights[0].device
    state = torch.empty(total, device=dev, dtype=torch.float32)
    outs = [state[o[0]:o[0] + R * K].view(w.shape) for o, (R, K), w in zip(offs, shapes, weights)]
    probs = [_sn_problem(w, u, v, state, o, R, K, out=out)
             for w, (u, v), o, (R, K), out in zip(weights, bufs, offs, shapes, outs)]
    n_el = sum(R * K for R, K in shapes)
    keep = (weights, bufs, state)
    for fn, args, ws in _sn_call('sr_spectral_norm_fwd', probs, (int(bool(training)), float(eps)), dev):
        # w read by the column, row and scale passes (row and scale in eval), W written; the relaunch of a trace
        # must not move u / v again, so a training call carries none
        relaunch = None if training else (lambda a=args, k=(keep, ws), f=fn: f(*a, _lib.stream()))
        with C.ktrace.span('spectral_norm_fwd_kernels', (5.0 if training else 3.0) * n_el,
                           4.0 * n_el * (4 if training else 3), relaunch=relaunch, launches=5 if training else 4):
            _lib.check(fn(*args, _lib.stream()))
    return outs, state, (shapes, offs)


def sn_state(state, layout, i):
    """(W [R, K], u [R], v [K], sigma [1]) of problem i as views of a forward's state buffer."""
    (R, K), (ow, ou, ov, osig) = layout[0][i], layout[1][i]
    return state[ow:ow + R * K].view(R, K), state[ou:ou + R], state[ov:ov + K], state[osig:osig + 1]


def spectral_norm_bwd_raw(state, layout, gs, outs, accumulate):
    """One grouped backward: ``outs[i]`` (=, or += with ``accumulate``) (gs[i] - <gs[i], W> u v^T) / sigma with the
    W, u, v, sigma of ``state``; problems whose ``gs[i]`` is None are skipped (their ``outs[i]`` may be None)."""
    shapes, offs = layout
    dev = state.device

    def problems(targets):
        return [_sn_problem(state[o[0]:], None, None, state, o, R, K, out=out, g=g)
                for o, (R, K), out, g in zip(offs, shapes, targets, gs)]

    n_el = sum(R * K for (R, K), g in zip(shapes, gs) if g is not None)
    if n_el == 0:
        return
    calls = _sn_call('sr_spectral_norm_bwd', problems(outs), (int(bool(accumulate)), ), dev)
    relaunches = [None] * len(calls)
    if C.ktrace.active():  # the relaunch of a trace must not accumulate into the live gradient
        scratch = [torch.empty_like(g) if g is not None else None for g in gs]
        relaunches = [lambda a=args, k=(ws, scratch, gs, state), f=fn: f(*a, _lib.stream())
                      for fn, args, ws in _sn_call('sr_spectral_norm_bwd', problems(scratch), (0, ), dev)]
    for (fn, args, ws), rl in zip(calls, relaunches):
        # G read by the dot and the apply pass, W by the dot, the target written (read too when accumulating)
        with C.ktrace.span('spectral_norm_bwd_kernels', 6.0 * n_el, 4.0 * n_el * (5 if accumulate else 4), relaunch=rl,
                           launches=2):
            _lib.check(fn(*args, _lib.stream()))


class _SpectralNormGroup(torch.autograd.Function):
    """All spectral-normalised weights of a network from one grouped launch sequence."""

    @staticmethod
    def forward(ctx, training, eps, bufs, *weights):
        ctx.set_materialize_grads(False)
        outs, state, ctx.layout = spectral_norm_fwd_raw([w.detach() for w in weights], bufs, training, eps)
        ctx.save_for_backward(state, *weights)
        ctx.mark_non_differentiable(*[o for o, w in zip(outs, weights) if not w.requires_grad])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        state, *weights = ctx.saved_tensors
        none = (None, None, None)
        need = [ctx.needs_input_grad[3 + i] and grads[i] is not None for i in range(len(weights))]
        if not any(need):
            return none + (None, ) * len(weights)
        gs = [g.float().contiguous() if nd else None for g, nd in zip(grads, need)]
        targets = [C.grad_target(w) if nd else None for w, nd in zip(weights, need)]
        direct = all(t is not None for t, nd in zip(targets, need) if nd)
        if not direct:
            targets = [torch.empty_like(g) if g is not None else None for g in gs]
        spectral_norm_bwd_raw(state, ctx.layout, gs, targets, direct)
        if not direct:
            return none + tuple(targets)
        for w, nd in zip(weights, need):
            if nd:
                C.grad_ready(w)
        return none + (None, ) * len(weights)


def spectral_norm_group(convs, training, eps=1e-12):
    """The spectral-normalised weights of ``convs`` (modules wrapped by ``torch.nn.utils.spectral_norm``: parameter
    ``weight_orig``, buffers ``weight_u`` / ``weight_v``), all from ONE grouped launch sequence whose length does not
    depend on ``len(convs)``.  ``training``: run the power iteration (one step, ``weight_u`` / ``weight_v`` updated in
    place, also under ``no_grad`` and with frozen parameters); else sigma comes from the stored vectors.  The modules
    themselves are never called.  Returns fresh fp32 tensors in the ``nn.Conv2d`` layout; the backward takes the
    convs' weight gradients G, launches nothing for a frozen ``weight_orig`` (nothing at all when every one is), and
    accumulates (G - <G, W> u v^T) / sigma with the u, v, sigma, W of ITS OWN forward straight into the FlatParams
    gradient views."""
    weights = [m.weight_orig for m in convs]
    bufs = [(m.weight_u, m.weight_v) for m in convs]
    for w, (u, v) in zip(weights, bufs):
        if not (w.is_cuda and u.is_cuda and v.is_cuda):
            raise NotImplementedError(_CPU_MESSAGE)
        if w.dtype != torch.float32 or not w.is_contiguous() or u.numel() != w.shape[0] or v.numel() != w[0].numel():
            raise ValueError('spectral_norm_group: weight_orig must be contiguous fp32 with weight_u [cout] and '
                             'weight_v [cin * kh * kw]')
    return _SpectralNormGroup.apply(bool(training), eps, bufs, *weights)


# --------------------------------------------------------------------------------------------- bilinear x2


def bilinear_up2_fwd_raw(x, scale=1.0):
    N, H, W, Cc = x.shape
    y = torch.empty(N, 2 * H, 2 * W, Cc, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    head = (_lib.dtype_code(x.dtype), _lib.ptr(x), N, H, W, Cc)
    if scale == 1.0:
        fn, args = lib.sr_bilinear_up2_fwd, head + (_lib.ptr(y), _lib.stream())
    else:
        fn, args = lib.sr_bilinear_up2_fwd_scaled, head + (float(scale), _lib.ptr(y), _lib.stream())
    # 4 taps per output element; x read once (each element 4 times, from cache), y written
    _launch('up2_fwd_kernel', 7.0 * y.numel(), x.element_size() * (x.numel() + y.numel()), fn, args, (x, y))
    return y


def bilinear_up2_bwd_raw(dy, scale=1.0):
    N, H2, W2, Cc = dy.shape
    dx = torch.empty(N, H2 // 2, W2 // 2, Cc, device=dy.device, dtype=dy.dtype)
    lib = _lib.load()
    head = (_lib.dtype_code(dy.dtype), _lib.ptr(dy), N, H2 // 2, W2 // 2, Cc)
    if scale == 1.0:
        fn, args = lib.sr_bilinear_up2_bwd, head + (_lib.ptr(dx), _lib.stream())
    else:
        fn, args = lib.sr_bilinear_up2_bwd_scaled, head + (float(scale), _lib.ptr(dx), _lib.stream())
    _launch('up2_bwd_kernel', 7.0 * dy.numel(), dy.element_size() * (dx.numel() + dy.numel()), fn, args, (dy, dx))
    return dx


class _BilinearUp2(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, scale=1.0):
        ctx.scale = scale
        return bilinear_up2_fwd_raw(x, scale)

    @staticmethod
    def backward(ctx, dy):
        return bilinear_up2_bwd_raw(dy.contiguous(), ctx.scale), None


def bilinear_up2(x, scale=1.0):
    """``F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)`` of an NHWC feature map
    [N, H, W, C] (C a multiple of 8, fp32 or bf16) -> [N, 2H, 2W, C], with its backward (a gather, no atomics).
    ``scale``: the result times it in the same pass (EDVR's ``upsample(offset) * 2``); 1 is the plain kernel."""
    _check_map(x, 'bilinear_up2')
    return _BilinearUp2.apply(x.contiguous(), float(scale))


# ---------------------------------------------------------------------------------------------- batch norm


def _bn_ws(lib, M, Cc, device):
    ws_bytes = lib.sr_bn_workspace(M, Cc)
    return torch.empty(ws_bytes // 4, device=device, dtype=torch.float32), ws_bytes


def bn_stats_raw(x, eps, momentum=0.1, nbt=None, running_mean=None, running_var=None):
    """(save_mean, save_rstd) of an NHWC map; updates the running statistics in place when given
    (``momentum=None``: the cumulative average over ``nbt``, already incremented)."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    lib = _lib.load()
    mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
    rstd = torch.empty(Cc, device=x.device, dtype=torch.float32)
    ws, ws_bytes = _bn_ws(lib, M, Cc, x.device)
    mom = -1.0 if momentum is None else float(momentum)

    def args(rm, rv):
        return (_lib.dtype_code(x.dtype), _lib.ptr(x), M, Cc, float(eps), mom, _lib.ptr(nbt), _lib.ptr(mean),
                _lib.ptr(rstd), _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(ws), ws_bytes)

    fn = lib.sr_bn_stats
    if C.ktrace.active():
        # the relaunch of a trace leaves the running statistics alone
        with C.ktrace.span('bn_stats_kernel+final', 6.0 * x.numel(), x.element_size() * x.numel() + 2 * ws_bytes,
                           relaunch=lambda a=args(None, None), k=(x, mean, rstd, ws): fn(*a, _lib.stream()), launches=2):
            _lib.check(fn(*args(running_mean, running_var), _lib.stream()))
    else:
        _lib.check(fn(*args(running_mean, running_var), _lib.stream()))
    return mean, rstd


def bn_apply_raw(x, mean, rv, use_var, eps, gamma, beta, act, slope):
    Cc = x.shape[-1]
    y = torch.empty_like(x)
    lib = _lib.load()
    args = (_lib.dtype_code(x.dtype), _lib.ptr(x), x.numel() // Cc, Cc, _lib.ptr(mean), _lib.ptr(rv), int(use_var),
            float(eps), _lib.ptr(gamma), _lib.ptr(beta), act, float(slope), _lib.ptr(y), _lib.stream())
    _launch('bn_apply_kernel', 5.0 * x.numel(), 2 * x.element_size() * x.numel(), lib.sr_bn_apply, args,
            (x, mean, rv, gamma, beta, y))
    return y


def bn_bwd_raw(x, dy, mean, rv, use_var, eps, gamma, beta, act, slope, training, need_dx=True):
    """(dx or None, dgamma, dbeta) of batch_norm_act."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    lib = _lib.load()
    dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = torch.empty(Cc, device=x.device, dtype=torch.float32)
    ws, ws_bytes = _bn_ws(lib, M, Cc, x.device)
    head = (_lib.dtype_code(x.dtype), _lib.ptr(x), _lib.ptr(dy), M, Cc, _lib.ptr(mean), _lib.ptr(rv), int(use_var),
            float(eps), _lib.ptr(gamma), _lib.ptr(beta), act, float(slope), _lib.ptr(dgamma), _lib.ptr(dbeta))
    keep = (x, dy, mean, rv, gamma, beta, dgamma, dbeta, ws)
    _launch('bn_bwd_reduce_kernel+final', 8.0 * x.numel(), 2 * x.element_size() * x.numel() + 2 * ws_bytes,
            lib.sr_bn_bwd_reduce, head + (_lib.ptr(ws), ws_bytes, _lib.stream()), keep, launches=2)
    dx = None
    if need_dx:
        dx = torch.empty_like(x)
        _launch('bn_bwd_dx_kernel', 10.0 * x.numel(), 3 * x.element_size() * x.numel(), lib.sr_bn_bwd_dx,
                head + (int(training), _lib.ptr(dx), _lib.stream()), keep + (dx, ))
    return dx, dgamma, dbeta


class _BatchNormAct(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, act, slope, training):
        if training:
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
            mean, rv = bn_stats_raw(x, bn.eps, bn.momentum, bn.num_batches_tracked, bn.running_mean, bn.running_var)
        else:
            mean, rv = bn.running_mean, bn.running_var
        g, b = gamma.detach(), beta.detach()
        y = bn_apply_raw(x, mean, rv, not training, bn.eps, g, b, act, slope)
        ctx.cfg = (bn.eps, act, slope, training)
        # eval: copies, so that a later update of the running statistics does not reach this backward
        ctx.save_for_backward(x, gamma, beta, mean if training else mean.clone(), rv if training else rv.clone())
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, rv = ctx.saved_tensors
        eps, act, slope, training = ctx.cfg
        dx, dgamma, dbeta = bn_bwd_raw(x, dy.to(x.dtype).contiguous(), mean, rv, not training, eps, gamma.detach(),
                                       beta.detach(), act, slope, training, need_dx=ctx.needs_input_grad[0])
        return (dx, dgamma if ctx.needs_input_grad[1] else None, dbeta if ctx.needs_input_grad[2] else None, None, None,
                None, None)


def batch_norm_act(x, bn, act=_lib.ACT_NONE, slope=0.2):
    """``act(bn(x))`` of an NHWC feature map for an ``nn.BatchNorm2d`` parameter module (affine, tracked running
    statistics), act ACT_NONE or ACT_LRELU.  ``bn.training`` chooses batch statistics (and the running-statistics
    update, as torch) or the running statistics."""
    if not isinstance(bn, torch.nn.BatchNorm2d) or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError('batch_norm_act: needs an nn.BatchNorm2d with affine=True and track_running_stats=True')
    if act not in (_lib.ACT_NONE, _lib.ACT_LRELU):
        raise ValueError('batch_norm_act: act must be ACT_NONE or ACT_LRELU')
    _check_map(x, 'batch_norm_act', C.pad8(bn.num_features))
    if bn.num_features % 8:
        raise ValueError(f'batch_norm_act: {bn.num_features} features (a multiple of 8 is supported)')
    if bn.training and x.numel() // x.shape[-1] == 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
    return _BatchNormAct.apply(x.contiguous(), bn.weight, bn.bias, bn, act, slope, bn.training)


# -------------------------------------------------------------------------------------------- head linears


def _fc_span(name, M, K, O, nbytes, fn, args, keep):
    _launch(name, 2.0 * M * K * O, nbytes, fn, args, keep)


class _Linear(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope, P):
        M, K = x.shape
        O = weight.shape[0]
        y = torch.empty(M, O, device=x.device, dtype=torch.float32)
        lib = _lib.load()
        w, b = weight.detach(), (bias.detach() if bias is not None else None)
        args = (_lib.dtype_code(x.dtype), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), M, K, O, P, act, float(slope), _lib.ptr(y),
                _lib.stream())
        _fc_span('fc_fwd_kernel', M, K, O, x.element_size() * x.numel() + 4 * (w.numel() + y.numel()), lib.sr_fc_fwd, args,
                 (x, w, b, y))
        ctx.cfg = (act, slope, P)
        ctx.save_for_backward(x, weight, bias, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, y = ctx.saved_tensors
        act, slope, P = ctx.cfg
        M, K = x.shape
        O = weight.shape[0]
        dy = dy.float().contiguous()
        lib = _lib.load()
        w = weight.detach()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            args = (_lib.dtype_code(x.dtype), _lib.ptr(dy), _lib.ptr(y), _lib.ptr(w), M, K, O, P, float(slope), _lib.ptr(dx),
                    _lib.stream())
            _fc_span('fc_dgrad_kernel', M, K, O, x.element_size() * x.numel() + 4 * (w.numel() + dy.numel()),
                     lib.sr_fc_dgrad, args, (dy, y, w, dx))
        need_b = bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or need_b:
            tw = C.grad_target(weight)
            tb = C.grad_target(bias) if bias is not None else None
            direct = tw is not None and (bias is None or tb is not None) and not C.ktrace.active()
            dw = tw if direct else torch.empty_like(w)
            db = (tb if direct else torch.empty(O, device=x.device, dtype=torch.float32)) if bias is not None else None
            args = (_lib.dtype_code(x.dtype), _lib.ptr(dy), _lib.ptr(y), _lib.ptr(x), M, K, O, P, float(slope), int(direct),
                    _lib.ptr(dw), _lib.ptr(db), _lib.stream())
            _fc_span('fc_wgrad_kernel', M, K, O, x.element_size() * x.numel() + 4 * (w.numel() + dy.numel()),
                     lib.sr_fc_wgrad, args, (dy, y, x, dw, db))
            if direct:
                C.grad_ready(weight)
                if bias is not None:
                    C.grad_ready(bias)
                dw = db = None
        return dx, dw, db, None, None, None


def linear(x, lin, act=_lib.ACT_NONE, slope=0.2, spatial=1):
    """``act(lin(x))`` for an ``nn.Linear`` parameter module: x [M, K] fp32 or bf16 on the device, the result
    fp32 [M, out_features].  ``spatial`` = H * W when x is a flattened NHWC map [M, H * W * C] and the weight
    expects the reference's NCHW flatten (index c * H * W + h * W + w)."""
    if not x.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if x.dim() != 2 or x.shape[1] != lin.in_features or lin.in_features % spatial:
        raise ValueError(f'linear: x must be [M, {lin.in_features}] (spatial {spatial}), got {tuple(x.shape)}')
    if act not in (_lib.ACT_NONE, _lib.ACT_LRELU):
        raise ValueError('linear: act must be ACT_NONE or ACT_LRELU')
    _lib.dtype_code(x.dtype)
    return _Linear.apply(x.contiguous(), lin.weight, lin.bias, act, slope, int(spatial))


# ------------------------------------------------------------------------------------------------ GAN loss


class _GanLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pred, kind, target_val, target_is_real, is_disc, loss_weight):
        if pred.dtype not in (torch.float32, torch.bfloat16):
            pred = pred.float()
        pred = pred.contiguous()
        lib = _lib.load()
        n = pred.numel()
        ws_bytes = lib.sr_gan_loss_workspace(n)
        ws = torch.empty(ws_bytes // 4, device=pred.device, dtype=torch.float32)
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        grad = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        args = (kind, _lib.dtype_code(pred.dtype), _lib.ptr(pred), n, float(target_val), int(bool(target_is_real)),
                int(bool(is_disc)), float(loss_weight), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), ws_bytes, _lib.stream())
        _launch('gan_loss_kernel+final', 8.0 * n, pred.element_size() * n * (1 + (grad is not None)), lib.sr_gan_loss, args,
                (pred, loss, grad, ws), launches=2)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad, ) = ctx.saved_tensors
        return (grad * g).to(grad.dtype), None, None, None, None, None


def gan_loss(pred, gan_type, target_is_real, is_disc=False, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
    """The GANLoss of the reference (gan_loss.py:89-112) for a prediction of any shape on the device: a 0-dim
    fp32 tensor with autograd (sr_gan_loss: the mean and its gradient from one pass)."""
    if gan_type not in GAN_KINDS:
        raise NotImplementedError(f'GAN type {gan_type} is not implemented.')
    if not pred.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if pred.numel() == 0:
        raise ValueError(f'gan_loss: the prediction is empty, shape {tuple(pred.shape)}')
    target_val = real_label_val if target_is_real else fake_label_val
    return _GanLoss.apply(pred, GAN_KINDS[gan_type], target_val, target_is_real, is_disc, loss_weight)
