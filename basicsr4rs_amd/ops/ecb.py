"""ECBSR (basicsr/archs/ecbsr_arch.py) on its collapsed form (csrc/ecb.hip).

The five branches of every ECB block sum to one 3x3 convolution, exactly, borders included.  The reference
uses that only in ``eval()``; here the train step does too.  Per forward pass one grouped kernel
(``sr_ecb_rep_fwd``) collapses all blocks' parameters into 3x3 weights and writes their GEMM images, then one
fused conv + PReLU kernel runs per layer (``sr_ecb_conv``); the last layer adds the shortcut and stores through
the PixelShuffle into the fp32 NCHW output.  Backward: per layer the gated input gradient (the same kernel on the
transposed image, times the producer's PReLU gate, with the slope-gradient partial sums) and the existing
``sr_convk_wgrad`` into one shared dRK / dRB buffer; then ``sr_ecb_da_reduce`` (all slope gradients) and
``sr_ecb_rep_bwd`` (dRK / dRB of all blocks -> the gradients of the reference's parameters), one launch each.

The parameters stay the reference's.  Their device pointers (and, with FlatParams, those of their gradient
views) live in a device table built once per (blocks, dtype, gradient mode) and rebuilt only when a pointer
moves, so the step can be captured.  With FlatParams the gradients accumulate in place and the gradient-ready
callbacks fire; without, plain tensors go back to autograd.  All weight gradients run on the current stream:
with ``async_wgrad`` of any mode the results are the synchronous ones.
"""
import weakref

import torch

from .. import _lib
from ..utils import ktrace
from . import conv as C
from . import convk as K

MAX_CH = 64
MAX_MID = 256
_EDGES = ('conv1x1_sbx', 'conv1x1_sby', 'conv1x1_lpl')


def image_taps(dtype):
    """Taps per GEMM image row: 9, or 18 for bf16 (the collapsed weight as hi + lo, see sr_ecb_rep_fwd)."""
    return 18 if dtype == torch.bfloat16 else 9


def block_params(blk):
    """The trainable tensors of an ECB block in table order (18, and the PReLU slopes when it has them)."""
    s = blk.conv1x1_3x3
    ps = [blk.conv3x3.weight, blk.conv3x3.bias, s.k0, s.b0, s.k1, s.b1]
    for name in _EDGES:
        e = getattr(blk, name)
        ps += [e.k0, e.b0, e.scale, e.bias]
    if blk.act_type == 'prelu':
        ps.append(blk.act.weight)
    return ps


class _State:
    """Device table, collapsed weights, images and gradient staging of a list of ECB blocks in one dtype."""

    def __init__(self, blocks, dtype, grads):
        # the blocks are held weakly: the state hangs off a module that owns them, and a strong reference back
        # would make every net a reference cycle (freed, with its GPU memory, only by the cycle collector)
        self._blocks = [weakref.ref(b) for b in blocks]
        self.dtype, self.grads = dtype, grads
        self.key = None
        self.version = None

    @property
    def blocks(self):
        return [r() for r in self._blocks]

    def _ptr_key(self, targets):
        ks = []
        for blk in self.blocks:
            ks += [p.data_ptr() for p in block_params(blk)]
            ks += [getattr(blk, n).mask.data_ptr() for n in _EDGES]
        if targets is not None:
            ks += [t.data_ptr() for t in targets]
        return tuple(ks)

    def _grad_targets(self):
        """The FlatParams gradient views of every trainable tensor, or None when any is missing."""
        out = []
        for blk in self.blocks:
            for p in block_params(blk):
                t = C.grad_target(p)
                if t is None:
                    return None
                out.append(t)
        return out

    def ensure(self):
        """Build (or rebuild, when a pointer moved) the device table; host work only when nothing moved."""
        targets = self._grad_targets() if self.grads else None
        key = self._ptr_key(targets)
        if key == self.key:
            return False
        dev = self.blocks[0].conv3x3.weight.device
        L = len(self.blocks)
        f32 = dict(device=dev, dtype=torch.float32)
        self.direct = targets is not None
        dims = []
        for blk in self.blocks:
            cout, cin = blk.conv3x3.weight.shape[:2]
            mid = blk.conv1x1_3x3.k0.shape[0]
            if cin > MAX_CH or cout > MAX_CH or mid > MAX_MID:
                raise ValueError(f'ECB: at most {MAX_CH} channels and mid_planes {MAX_MID}, got {cin} -> {mid} -> {cout}')
            dims.append((cin, cout, mid, C.pad8(cin), C.pad8(cout)))
        self.dims = dims
        self.rk = [torch.empty(co, ci, 3, 3, **f32) for ci, co, _, _, _ in dims]
        self.rb = [torch.empty(co, **f32) for _, co, _, _, _ in dims]
        kt = image_taps(self.dtype)
        self.wf = [torch.empty(cop, kt * cip, device=dev, dtype=self.dtype) for _, _, _, cip, cop in dims]
        self.wd = [torch.empty(cip, kt * cop, device=dev, dtype=self.dtype) for _, _, _, cip, cop in dims]
        self.bg = [torch.empty(cop, **f32) for _, _, _, _, cop in dims]
        self.zero_slope = torch.zeros(MAX_CH, **f32)
        items = (_lib.EcbBlock * L)()
        if self.grads:
            self.drk = [torch.zeros(co, ci, 3, 3, **f32) for ci, co, _, _, _ in dims]
            self.drb = [torch.zeros(co, **f32) for _, co, _, _, _ in dims]
            if not self.direct:  # staging for the gradients handed back to autograd
                self.stage = [[torch.zeros_like(p, dtype=torch.float32) for p in block_params(blk)]
                              for blk in self.blocks]
        ti = 0
        for l, (blk, it) in enumerate(zip(self.blocks, items)):
            ps = block_params(blk)
            it.w3, it.b3, it.k0, it.b0, it.k1, it.b1 = (p.data_ptr() for p in ps[:6])
            for e, name in enumerate(_EDGES):
                k0, b0, sc, bi = ps[6 + 4 * e:10 + 4 * e]
                it.ek0[e], it.eb0[e], it.escale[e], it.ebias[e] = k0.data_ptr(), b0.data_ptr(), sc.data_ptr(), bi.data_ptr()
                it.emask[e] = getattr(blk, name).mask.data_ptr()
            it.rk, it.rb = self.rk[l].data_ptr(), self.rb[l].data_ptr()
            it.wf, it.wd, it.bias_g = self.wf[l].data_ptr(), self.wd[l].data_ptr(), self.bg[l].data_ptr()
            it.Cin, it.Cout, it.mid, it.Cin_p, it.Cout_p = dims[l]
            it.with_idt = int(bool(blk.with_idt))
            if self.grads:
                it.drk, it.drb = self.drk[l].data_ptr(), self.drb[l].data_ptr()
                gs = targets[ti:ti + len(ps)] if self.direct else self.stage[l]
                ti += len(ps)
                it.g_w3, it.g_b3, it.g_k0, it.g_b0, it.g_k1, it.g_b1 = (g.data_ptr() for g in gs[:6])
                for e in range(3):
                    a, b, c, d = gs[6 + 4 * e:10 + 4 * e]
                    it.g_ek0[e], it.g_eb0[e], it.g_escale[e], it.g_ebias[e] = a.data_ptr(), b.data_ptr(), c.data_ptr(), \
                        d.data_ptr()
                it.g_act = gs[18].data_ptr() if len(ps) > 18 else None
        lib = _lib.load()
        _lib.check(lib.sr_ecb_table_check(items, L))
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
        self.max_cout_p = max(d[4] for d in dims)
        self.max_units = max(d[1] + d[2] for d in dims)
        self.key, self.version = key, None
        return True

    def _versions(self):
        vs = [C._PARAM_EPOCH[0]]
        for blk in self.blocks:
            vs += [p._version for p in block_params(blk)]
        return tuple(vs)

    def collapse(self, cached=False):
        """Run sr_ecb_rep_fwd; with ``cached`` (eval) only when a parameter changed since the last run."""
        self.ensure()
        if torch.cuda.is_current_stream_capturing():
            C._CAPTURED_TABLES.append(self)  # the graph launches on this table: its owner keeps it alive
        v = self._versions() if cached else None
        if cached and v == self.version:
            return
        lib = _lib.load()
        args = (_lib.dtype_code(self.dtype), _lib.ptr(self.table), len(self.blocks), self.max_cout_p)
        # the parameters read, and both images written
        img = 2 * self.wf[0].element_size() * image_taps(self.dtype)
        nb = sum(4 * (9 * ci * co + 9 * co * mid + mid * ci + 3 * co * ci) + img * cip * cop
                 for ci, co, mid, cip, cop in self.dims)
        with ktrace.span('ecb_rep_fwd_kernel', sum(2.0 * 9 * ci * co * mid for ci, co, mid, _, _ in self.dims), nb,
                         relaunch=lambda a=args, k=self: lib.sr_ecb_rep_fwd(*a, _lib.stream())):
            _lib.check(lib.sr_ecb_rep_fwd(*args, _lib.stream()))
        self.version = v


def state_of(owner, blocks, dtype, grads):
    """The cached _State of ``blocks`` on ``owner`` (a module) for a dtype and gradient mode."""
    cache = owner.__dict__.setdefault('_sr_ecb_state', {})
    st = cache.get((dtype, grads))
    # (a deep copy of the module carries the original's state, whose weak references still name the original blocks)
    if st is None or len(st._blocks) != len(blocks) or any(r() is not b for r, b in zip(st._blocks, blocks)):
        st = cache[(dtype, grads)] = _State(blocks, dtype, grads)
    return st


def _cdesc(dtype, mode, N, H, W, cin_p, cout_p, cout, ps=0, img_c=0):
    d = _lib.EcbConvDesc()
    d.dtype, d.mode, d.N, d.H, d.W = _lib.dtype_code(dtype), mode, N, H, W
    d.Cin, d.Cout, d.Cout_real, d.ps, d.img_c = cin_p, cout_p, cout, ps, img_c
    return d


def _launch_conv(name, d, x, w, bias, slope, y, z, parts, img, out, maps):
    """One sr_ecb_conv launch; ``maps``: how many NHWC maps of Cout channels the epilogue reads or writes."""
    lib = _lib.load()
    args = (d, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(slope), _lib.ptr(y), _lib.ptr(z), _lib.ptr(parts),
            _lib.ptr(img), _lib.ptr(out))
    if ktrace.active():
        M, esz = d.N * d.H * d.W, x.element_size()
        nbytes = esz * (M * d.Cin + image_taps(x.dtype) * d.Cin * d.Cout + maps * M * d.Cout)
        if out is not None:
            nbytes += 4 * (out.numel() + img.numel())
        if parts is not None:
            nbytes += 4 * lib.sr_ecb_conv_blocks(d) * MAX_CH
        keep = (x, w, bias, slope, y, z, parts, img, out)
        with ktrace.span(name, 2.0 * M * image_taps(x.dtype) * d.Cin * d.Cout, nbytes,
                         relaunch=lambda a=args, k=keep: lib.sr_ecb_conv(*a, _lib.stream())):
            _lib.check(lib.sr_ecb_conv(*args, _lib.stream()))
    else:
        _lib.check(lib.sr_ecb_conv(*args, _lib.stream()))


def conv_act(x, w_img, bias_g, slope, cout_p, cout, want_z=True):
    """y = prelu(conv3x3(x) + b, slope) on an NHWC map; returns (y, z) with z the stored pre-activation
    (None when ``want_z`` is false or the layer is linear)."""
    assert x.is_contiguous() and x.dim() == 4 and w_img.dtype == x.dtype
    N, H, W, cin_p = x.shape
    assert tuple(w_img.shape) == (cout_p, image_taps(x.dtype) * cin_p), (w_img.shape, cout_p, cin_p)
    y = torch.empty(N, H, W, cout_p, device=x.device, dtype=x.dtype)
    z = torch.empty_like(y) if want_z and slope is not None else None
    d = _cdesc(x.dtype, 0, N, H, W, cin_p, cout_p, cout)
    _launch_conv('ecb_conv_act_kernel', d, x, w_img, bias_g, slope, y, z, None, None, None, 1 + (z is not None))
    return y, z


def conv_tail(x, w_img, bias_g, img, cout_p, cout, scale):
    """The last block: conv + bias + shortcut stored through the PixelShuffle into fp32 NCHW."""
    assert x.is_contiguous() and img.is_contiguous() and img.dtype == torch.float32
    N, H, W, cin_p = x.shape
    assert tuple(w_img.shape) == (cout_p, image_taps(x.dtype) * cin_p) and img.shape[0] == N and tuple(img.shape[2:]) == (H, W)
    out = torch.empty(N, cout // (scale * scale), H * scale, W * scale, device=x.device, dtype=torch.float32)
    d = _cdesc(x.dtype, 1, N, H, W, cin_p, cout_p, cout, ps=scale, img_c=img.shape[1])
    _launch_conv('ecb_conv_tail_kernel', d, x, w_img, bias_g, None, None, None, None, img, out, 0)
    return out


def conv_dgrad(dz, wd_img, z, slope, cprod_p, cprod, want_parts=None):
    """Gradient with respect to the producer's pre-activation: conv of the consumer's ``dz`` with the transposed
    image, times the producer's gate from its stored ``z``; ``want_parts``: a [blocks, 64] fp32 buffer that receives
    the partial channel sums of g * min(z, 0)."""
    assert dz.is_contiguous() and (z is None or (z.is_contiguous() and z.dtype == dz.dtype))
    N, H, W, ccons_p = dz.shape
    assert tuple(wd_img.shape) == (cprod_p, image_taps(dz.dtype) * ccons_p) and (z is None or tuple(z.shape) == (N, H, W, cprod_p))
    out = torch.empty(N, H, W, cprod_p, device=dz.device, dtype=dz.dtype)
    d = _cdesc(dz.dtype, 2, N, H, W, ccons_p, cprod_p, cprod)
    parts = want_parts
    _launch_conv('ecb_conv_dgrad_kernel', d, dz, wd_img, None, slope, out, z, parts, None, None, 1 + (z is not None))
    return out


def conv_blocks(dtype, N, H, W, cin_p, cout_p, cout):
    return _lib.load().sr_ecb_conv_blocks(_cdesc(dtype, 2, N, H, W, cin_p, cout_p, cout))


def tail_bwd(dout, scale, cp, dtype):
    """fp32 NCHW dOut [N, C, H s, W s] -> NHWC dz [N, H, W, cp] of the last block (pixel-unshuffle)."""
    N, Cc, Hs, Ws = dout.shape
    H, W = Hs // scale, Ws // scale
    dz = torch.empty(N, H, W, cp, device=dout.device, dtype=dtype)
    lib = _lib.load()
    args = (_lib.dtype_code(dtype), _lib.ptr(dout), N, Cc, H, W, scale, cp, _lib.ptr(dz))
    with ktrace.span('ecb_tail_bwd_kernel', 0.0, 4 * dout.numel() + dz.element_size() * dz.numel(),
                     relaunch=lambda a=args, k=(dout, dz): lib.sr_ecb_tail_bwd(*a, _lib.stream())):
        _lib.check(lib.sr_ecb_tail_bwd(*args, _lib.stream()))
    return dz


def _wgrad_into(dz, x, cin, cout, drk, drb):
    """sr_convk_wgrad (k = 3) of one layer, written into its slice of the shared dRK / dRB buffer."""
    N, H, W, cin_p = x.shape
    d = K._kdesc(x.dtype, N, H, W, 3, cin_p, cin, dz.shape[-1], cout)
    lib = _lib.load()
    ws_bytes = lib.sr_convk_wgrad_workspace(d)
    if ws_bytes == 0:
        raise ValueError(f'ecb wgrad: unsupported shape cin={cin_p} cout={dz.shape[-1]} N={N} H={H} W={W}')
    ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
    args = (d, _lib.ptr(dz), _lib.ptr(x), _lib.ptr(ws), ws_bytes, _lib.ptr(drk), _lib.ptr(drb))
    M = N * H * W
    with ktrace.span('convk_wgrad_kernel+reduce', 2.0 * M * 9 * cin_p * dz.shape[-1],
                     x.element_size() * M * (cin_p + dz.shape[-1]) + 4 * (9 * cin * cout + cout),
                     relaunch=lambda a=args, k=(dz, x, ws, drk, drb): lib.sr_convk_wgrad(*a, _lib.stream()), launches=2):
        _lib.check(lib.sr_convk_wgrad(*args, _lib.stream()))


def rep_bwd(st):
    """sr_ecb_rep_bwd over the whole table (accumulating into the FlatParams views when bound)."""
    lib = _lib.load()
    args = (_lib.ptr(st.table), len(st.blocks), st.max_units, int(st.direct))
    nb = sum(4 * 2 * (9 * ci * co + 9 * co * mid + mid * ci + 3 * co * ci) for ci, co, mid, _, _ in st.dims)
    # (the relaunch would accumulate into the live gradients a second time: none)
    with ktrace.span('ecb_rep_bwd_kernel', sum(4.0 * 9 * ci * co * mid for ci, co, mid, _, _ in st.dims), nb):
        _lib.check(lib.sr_ecb_rep_bwd(*args, _lib.stream()))


def da_reduce(st, layers, parts, nblocks):
    lib = _lib.load()
    with ktrace.span('ecb_da_reduce_kernel', 0.0, 4 * parts.numel()):
        _lib.check(lib.sr_ecb_da_reduce(_lib.ptr(st.table), layers, _lib.ptr(parts), nblocks, int(st.direct),
                                        _lib.stream()))


def _slope(st, blk):
    if blk.act_type == 'prelu':
        return blk.act.weight.detach()
    if blk.act_type == 'relu':
        return st.zero_slope
    return None


class _Backbone(torch.autograd.Function):
    """The whole ECBSR forward (backbone + shortcut + PixelShuffle) as one autograd node."""

    @staticmethod
    def forward(ctx, x, st, scale, cached, *params):
        st.collapse(cached)
        dtype, L = st.dtype, len(st.blocks)
        img = x.detach().contiguous().float()
        N, Cimg, H, W = img.shape
        need = any(ctx.needs_input_grad[4:])
        h = C.nchw_to_nhwc(img, st.dims[0][3], dtype)
        ys, zs = [h], []
        for l in range(L - 1):
            blk = st.blocks[l]
            _, cout, _, _, cout_p = st.dims[l]
            # ReLU: the output's sign is the gate's, no z; PReLU keeps z for the gate and the slope gradient
            h, z = conv_act(h, st.wf[l], st.bg[l], _slope(st, blk), cout_p, cout, want_z=need and blk.act_type == 'prelu')
            ys.append(h)
            zs.append(z if blk.act_type == 'prelu' else (h if blk.act_type == 'relu' else None))
        _, cout, _, _, cout_p = st.dims[L - 1]
        out = conv_tail(h, st.wf[L - 1], st.bg[L - 1], img, cout_p, cout, scale)
        if need:
            ctx.st, ctx.scale = st, scale
            ctx.save_for_backward(*ys, *[z for z in zs if z is not None])
            ctx.has_z = [z is not None for z in zs]
        return out

    @staticmethod
    def backward(ctx, dout):
        st, scale = ctx.st, ctx.scale
        L, dtype = len(st.blocks), st.dtype
        saved = list(ctx.saved_tensors)
        ys, rest = saved[:L], saved[L:]
        zs = [rest.pop(0) if hz else None for hz in ctx.has_z]
        if st.ensure():  # a gradient view was replaced since the forward: the rebuilt table has new images
            st.collapse()
        dz = tail_bwd(dout.contiguous().float(), scale, st.dims[L - 1][4], dtype)
        N, H, W, _ = dz.shape
        nblocks = conv_blocks(dtype, N, H, W, 8, 8, 8)
        prelu = [st.blocks[l].act_type == 'prelu' for l in range(L - 1)]
        parts = torch.empty(L - 1, nblocks, MAX_CH, device=dz.device, dtype=torch.float32) if any(prelu) else None
        for l in reversed(range(L)):
            cin, cout, _, cin_p, _ = st.dims[l]
            _wgrad_into(dz, ys[l], cin, cout, st.drk[l], st.drb[l])
            if l > 0:
                pblk = st.blocks[l - 1]
                dz = conv_dgrad(dz, st.wd[l], zs[l - 1], _slope(st, pblk), cin_p, cin,
                                parts[l - 1] if prelu[l - 1] else None)
        if parts is not None:
            da_reduce(st, L - 1, parts, nblocks)
        rep_bwd(st)
        if st.direct:
            for blk in st.blocks:
                for p in block_params(blk):
                    C.grad_ready(p)
            return (None, None, None, None) + (None, ) * sum(len(block_params(b)) for b in st.blocks)
        grads = []
        for l, blk in enumerate(st.blocks):
            grads += [g.clone() for g in st.stage[l]]
        return (None, None, None, None, *grads)


def ecbsr_forward(owner, blocks, x, scale):
    """ECBSR's forward on an fp32 NCHW image: backbone, shortcut and PixelShuffle.  ``owner`` (the net module)
    keeps the cached tables; in ``eval()`` the collapsed images are reused until a parameter changes."""
    if x.requires_grad:
        raise NotImplementedError('ECBSR: the gradient with respect to the input image is not implemented '
                                  '(pass a tensor that does not require grad)')
    if x.dim() != 4:
        raise ValueError(f'ECBSR: x must be [N, C, H, W], got {tuple(x.shape)}')
    params = [p for b in blocks for p in block_params(b)]
    grads = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    if grads and not all(p.requires_grad for p in params):
        raise NotImplementedError('ECBSR: partially frozen parameters are not supported')
    st = state_of(owner, blocks, C.feature_dtype(), grads)
    return _Backbone.apply(x, st, int(scale), not owner.training and not grads, *params)


def rep_params(blk):
    """(rep_weight, rep_bias) of one ECB block in fp32, computed by the device collapse kernel."""
    st = state_of(blk, [blk], torch.float32, False)
    st.collapse()
    return st.rk[0].clone(), st.rb[0].clone()
