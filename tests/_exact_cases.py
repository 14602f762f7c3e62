"""Case tables of the exact-arithmetic conv tests and the builders that turn a case into stored operands, the
call's keyword arguments and the float64 result (tests/_exact.py has the arithmetic).  Host-only code: the
GPU test uploads what a builder returns.  A built case is cached and never modified."""
from types import SimpleNamespace

import torch

from . import _exact as E

BF, F32 = 'bf16', 'f32'
DT = {BF: torch.bfloat16, F32: torch.float32}
_BUILT = {}


def _ns(**kw):
    return SimpleNamespace(**kw)


def fw(family, shape, variant, kernel, epi='plain', dtype=BF, ksize=3, in_ps=0, out_ps=0, in_up=0, xpad=(0, 0),
       ypad=(0, 0), knobs=None, mode='dense', nchw=False, tag=''):
    """A forward case: shape (N, H, W, cin, cout) of the conv as computed (output pixels N H W)."""
    opts = ''.join(f'-{k}{v}' for k, v in (('k', ksize if ksize != 3 else 0), ('ips', in_ps), ('ops', out_ps),
                                            ('up', in_up)) if v)
    opts += ('-xs' if xpad != (0, 0) else '') + ('-ys' if ypad != (0, 0) else '') + ('-nchw' if nchw else '')
    opts += '-imp' + '.'.join(map(str, mode[1])) if mode != 'dense' else ''
    data = f'{family}-{"x".join(map(str, shape))}-{dtype}{opts}-{epi}'  # operands: shared by the variants / knobs
    return _ns(family=family, shape=shape, variant=variant, kernel=kernel, epi=epi, dtype=dtype, ksize=ksize,
               in_ps=in_ps, out_ps=out_ps, in_up=in_up, xpad=xpad, ypad=ypad, knobs=knobs or {}, mode=mode, nchw=nchw,
               data=data, id=f'{data}-v{variant}{tag}')


def wg(family, shape, variant, kernel, ps=0, in_up=0, ksize=3, xpad=(0, 0), ypad=(0, 0), knobs=None, cin_real=None,
       scale=1.0, dtype=BF, tag=''):
    """A weight-gradient case: shape (N, H, W, cin, cout) with cin the stored (padded) input channels."""
    opts = ''.join(f'-{k}{v}' for k, v in (('k', ksize if ksize != 3 else 0), ('ps', ps), ('up', in_up)) if v)
    opts += ('-xs' if xpad != (0, 0) else '') + ('-ys' if ypad != (0, 0) else '') + (f'-s{scale}' if scale != 1 else '')
    data = f'{family}-{"x".join(map(str, shape))}-{dtype}{opts}' + (f'-cr{cin_real}' if cin_real else '')
    return _ns(family=family, shape=shape, variant=variant, kernel=kernel, ps=ps, in_up=in_up, ksize=ksize, xpad=xpad,
               ypad=ypad, knobs=knobs or {}, cin_real=cin_real or shape[3], scale=scale, dtype=dtype, data=data,
               id=f'{data}-v{variant}{tag}')


# ------------------------------------------------------------------------------------------ forward tables

PP, PPH, BIG, HALO, BAND, TAIL = (f'conv3x3_fwd_{n}_kernel' for n in ('pp', 'pph', 'big', 'halo', 'band', 'tail'))
LIN, WK = 'conv3x3_lin_kernel', 'linear_wk_kernel'

FWD = []

# 256x256 phase-interleaved (24: never the halo form), two-barrier (2) and the 128x128 tile kernel (1)
for _shape, _o in [((1, 20, 36, 256, 512), {}), ((3, 17, 9, 256, 768), {}), ((1, 12, 20, 264, 256), {}),
                   ((1, 16, 16, 1024, 256), dict(in_ps=2)), ((1, 5, 13, 368, 544), dict(ksize=1))]:
    for _epi in ('plain', 'full'):
        FWD += [fw('pp', _shape, 24, PP, _epi, **_o), fw('big', _shape, 2, BIG, _epi, **_o),
                fw('tile', _shape, 1, 'conv3x3_fwd_kernel<bf16', _epi, **_o)]
# 1x1 with K 184 <= 192: the linear kernels whatever the variant (wide-K kernel with its compile-time epilogues,
# the lin kernel's run-time-flag form for LeakyReLU + residual), the tile kernel under variant 1
FWD += [fw('wk', (1, 9, 15, 184, 544), 24, WK, 'plain', ksize=1), fw('lin', (1, 9, 15, 184, 544), 24, LIN, 'full', ksize=1),
        fw('tile', (1, 9, 15, 184, 544), 1, 'conv3x3_fwd_kernel<bf16', 'plain', ksize=1),
        fw('tile', (1, 9, 15, 184, 544), 1, 'conv3x3_fwd_kernel<bf16', 'full', ksize=1)]

# fp32 on the generic path
for _shape in [(2, 8, 8, 24, 40), (1, 12, 20, 3, 64)]:
    for _epi in ('plain', 'full'):
        FWD.append(fw('f32', _shape, 0, 'conv3x3_fwd_kernel<f32', _epi, dtype=F32))

# halo-row 256x256 kernel: whole-row tiles, sliced input + channel sums, pixel-shuffled input, column strips,
# pixel-shuffled store, persistent (SR_PPH_GRID 1: both tiles in one block) against one tile per block (80)
for _epi in ('plain', 'full'):
    FWD += [fw('pph', (1, 4, 128, 64, 256), 0, PPH, _epi), fw('pph', (3, 4, 64, 128, 256), 0, PPH, _epi),
            fw('pph', (2, 4, 64, 1024, 256), 0, PPH, _epi, in_ps=2), fw('pph', (1, 4, 64, 2304, 256), 0, PPH, _epi, in_ps=3),
            fw('pph', (1, 8, 192, 128, 256), 0, PPH, _epi), fw('pph', (3, 12, 320, 64, 320), 0, PPH, _epi),
            fw('pph', (2, 4, 64, 256, 256), 0, PPH, _epi, knobs={'SR_PPH_GRID': 1}, tag='-persistent'),
            fw('pph', (2, 4, 64, 256, 256), 80, PPH, _epi, tag='-onetile')]
FWD += [fw('pph', (2, 4, 64, 512, 256), 0, PPH, 'colsum', xpad=(8, 8)),
        fw('pph', (2, 4, 64, 512, 256), 0, PPH, 'plain', xpad=(8, 8)),
        fw('pph', (2, 4, 64, 512, 256), 0, PPH, 'full', xpad=(8, 8)),
        fw('pph', (1, 4, 256, 256, 1024), 0, PPH, 'plain', out_ps=2),
        fw('pph', (1, 4, 256, 256, 1024), 0, PPH, 'lrelu', out_ps=2)]

# narrow halo kernel: ragged Cin chunks, slices on both sides, the Cout-32 form (34: band kernel off), in_ps
for _epi in ('plain', 'full'):
    FWD += [fw('halo', (1, 4, 128, 192, 32), 34, HALO, _epi), fw('halo', (2, 4, 64, 160, 8), 34, HALO, _epi),
            fw('halo', (1, 4, 64, 184, 184), 0, HALO, _epi, xpad=(8, 8), ypad=(16, 8)),
            fw('halo', (3, 20, 128, 96, 32), 34, HALO, _epi), fw('halo', (3, 20, 128, 160, 32), 34, HALO, _epi),
            fw('halo', (2, 4, 64, 576, 64), 0, HALO, _epi, in_ps=3)]

# row-streaming band kernel: one-row bands (36) and long bands crossing images (35).  Its epilogues are
# compile-time codes (band_epi of conv3x3.hip); LeakyReLU + residual is not one of them, so the full epilogues
# here are the instantiated ones: bias + residual, gate + alpha + residual, two residuals + row scale, the RRDB
# dgrad's column gate, and bias + LeakyReLU through channel slices
for _grid in (36, 35):
    for _shape in [(5, 13, 64, 64, 64), (1, 1, 64, 64, 64), (2, 9, 128, 32, 96), (3, 5, 128, 64, 192)]:
        for _epi in ('plain', 'res', 'relu', 'gate_alpha_res', 'res2_rowscale', 'rrdb_dgrad', 'colsum_plain', 'dot'):
            if _epi in ('colsum_plain', 'dot') and (_shape[4] > 64 or (_epi == 'dot' and _shape[3:] != (64, 64))):
                continue  # fused channel sums are not sliced (64-wide convs only)
            FWD.append(fw('band', _shape, _grid, BAND, _epi))
        FWD.append(fw('band', _shape, _grid, BAND, 'lrelu', xpad=(16, 16), ypad=(16, 8)))
# ... over 128-px column strips (wider images, the folded nearest x2 upsample, narrow inputs)
for _grid in (0, 35):
    for _shape, _o in [((3, 7, 384, 64, 64), {}), ((1, 6, 128, 64, 64), dict(in_up=2)), ((2, 5, 256, 8, 256), {}),
                       ((1, 3, 384, 16, 192), {})]:
        for _epi in ('plain', 'lrelu', 'gate'):
            if _shape[3] < 64 and _epi == 'lrelu':
                continue  # narrow-input strips: plain and gated (dgrad) epilogues only
            FWD.append(fw('band-strips', _shape, _grid, BAND, _epi, **_o))

# HR tail (fp32 NCHW store with the affine): row-streaming tail kernel (Cin 64 / 256), one-row halo tiles (Cin 96)
for _shape, _k in [((2, 3, 256, 256, 3), TAIL), ((1, 33, 256, 256, 16), TAIL), ((3, 35, 256, 64, 8), TAIL),
                   ((1, 2, 256, 96, 16), HALO)]:
    for _epi in ('plain', 'affine'):
        FWD.append(fw('tail', _shape, 0, _k, _epi, nchw=True))

# linear forward: 64-token lin kernel and the wide-K kernel (64: wide-K kernel off)
for _epi in ('plain', 'res'):
    FWD += [fw('lin', (3, 8, 40, 200, 96), 0, LIN, _epi, ksize=1), fw('lin', (3, 8, 40, 384, 40), 0, LIN, _epi, ksize=1),
            fw('lin', (3, 8, 40, 184, 184), 64, LIN, _epi, ksize=1), fw('wk', (3, 8, 40, 184, 184), 0, WK, _epi, ksize=1),
            fw('wk', (3, 8, 40, 360, 184), 0, WK, _epi, ksize=1)]


def _impulses(c):
    """Impulse positions of a case: the image corners, a strip seam (or the middle column of a narrow image),
    the last pixel of the last image, the first and last channel of the last (ragged) chunk."""
    N, H, W, cin, _ = c.shape
    seam = 64 if W > 64 else W // 2
    last8 = (cin - 1) // 8 * 8
    return [(0, 0, 0, 0), (0, 0, W - 1, cin - 1), (0, H - 1, 0, last8), (0, H - 1, W - 1, min(9, cin - 1)),
            (0, H // 2, seam, cin // 2), (0, H // 2, seam - 1, 1 % cin), (N - 1, H - 1, W - 1, cin - 1)]


# impulse mode: the first shape of each family
FWD_IMPULSE = []
for _c in [fw('pp', (1, 20, 36, 256, 512), 24, PP), fw('big', (1, 20, 36, 256, 512), 2, BIG),
           fw('tile', (1, 20, 36, 256, 512), 1, 'conv3x3_fwd_kernel<bf16'),
           fw('f32', (2, 8, 8, 24, 40), 0, 'conv3x3_fwd_kernel<f32', dtype=F32),
           fw('pph', (1, 4, 128, 64, 256), 0, PPH), fw('halo', (1, 4, 128, 192, 32), 34, HALO),
           fw('band', (5, 13, 64, 64, 64), 36, BAND), fw('band-strips', (3, 7, 384, 64, 64), 0, BAND),
           fw('tail', (2, 3, 256, 256, 3), 0, TAIL, nchw=True), fw('lin', (3, 8, 40, 200, 96), 0, LIN, ksize=1),
           fw('wk', (3, 8, 40, 184, 184), 0, WK, ksize=1)]:
    for _pos in _impulses(_c):
        FWD_IMPULSE.append(fw(_c.family, _c.shape, _c.variant, _c.kernel, dtype=_c.dtype, ksize=_c.ksize, nchw=_c.nchw,
                              mode=('impulse', _pos)))

# ------------------------------------------------------------------------------------------ wgrad tables

WPP, WBIG, ROW3, RING = (f'conv3x3_wgrad_{n}_kernel' for n in ('pp', 'big', 'row3', 'ring'))
WLIN, WSMALL = 'linear_wgrad_kernel', 'conv3x3_wgrad_kernel<bf16>'

WGRAD = [
    wg('pp', (2, 4, 64, 256, 256), 78, WPP), wg('pp', (1, 3, 128, 256, 1024), 78, WPP, ps=2, scale=0.5),
    wg('big', (2, 9, 14, 256, 768), 2, WBIG), wg('big', (1, 20, 12, 512, 256), 2, WBIG, scale=0.5),
    wg('small', (2, 9, 14, 256, 768), 1, WSMALL), wg('small', (1, 20, 12, 512, 256), 1, WSMALL),
    wg('small', (2, 8, 8, 24, 40), 0, 'conv3x3_wgrad_kernel<f32>', dtype=F32),
]
for _bg in (-1, 1, 5):
    WGRAD += [wg('row3', (1, 3, 64, 256, 256), 0, ROW3, knobs={'SR_WG_ROW3': _bg}, tag=f'-bg{_bg}'),
              wg('row3', (3, 1, 64, 256, 512), 0, ROW3, knobs={'SR_WG_ROW3': _bg}, tag=f'-bg{_bg}', scale=0.5),
              wg('row3', (1, 7, 192, 384, 256), 0, ROW3, knobs={'SR_WG_ROW3': _bg}, tag=f'-bg{_bg}'),
              wg('row3', (1, 2, 64, 128, 2304), 0, ROW3, ps=3, knobs={'SR_WG_ROW3': _bg}, tag=f'-bg{_bg}')]
WGRAD += [
    # all-taps halo form: channel slices of wider buffers on both operands, the folded nearest x2 gather
    wg('ring', (3, 1, 64, 96, 8), 0, RING, xpad=(8, 16), ypad=(16, 0)),
    wg('ring', (1, 2, 128, 64, 64), 0, RING, in_up=2, xpad=(8, 16), ypad=(16, 0), scale=0.5),
    wg('ring', (1, 5, 64, 160, 48), 0, RING, xpad=(8, 16), ypad=(16, 0)),
    # 64-channel output tiles (62)
    wg('ring-wide', (3, 3, 64, 8, 256), 62, RING), wg('ring-wide', (1, 3, 128, 184, 72), 62, RING, scale=0.5),
    wg('ring-wide', (1, 3, 64, 64, 576), 62, RING, ps=3),
    # 1x1: the token-range kernel, the 256x256 pp kernel (63) and the 128x128 kernel (1: variant 28 leaves 1x1
    # shapes on the token-range kernel)
    wg('lin', (1, 1, 1, 64, 64), 0, WLIN, ksize=1), wg('lin', (1, 3, 7, 200, 72), 0, WLIN, ksize=1, scale=0.5),
    wg('lin', (3, 8, 64, 184, 360), 0, WLIN, ksize=1),
    wg('lin-pp', (1, 3, 64, 128, 136), 63, WPP, ksize=1), wg('lin-small', (1, 3, 64, 128, 136), 1, WSMALL, ksize=1),
    # RGB head: block-per-channel slab reduce (0) and one thread per weight (33)
    wg('rgb', (1, 16, 16, 8, 64), 0, WSMALL, cin_real=1), wg('rgb', (1, 16, 16, 8, 64), 33, WSMALL, cin_real=1),
    wg('rgb', (2, 32, 48, 8, 256), 0, WSMALL, cin_real=3, scale=0.5), wg('rgb', (2, 32, 48, 8, 256), 33, WSMALL, cin_real=3),
]
PAIR_SHAPE = (1, 3, 64, 256, 256)  # the smallest case of test_wgrad_pair_gpu.py
PAIR_SCALES = (1.0, 0.5)

# k x k convs (ops/convk.py) and the discriminator's 4x4 stride-2 conv (ops/gan.py)
CONVK = [(k, ch, shp, dt) for k in (5, 9) for ch in ((4, 64), (32, 6)) for shp in ((1, 1, 1), (2, 3, 5), (2, 17, 33))
         for dt in (BF, F32)]
CONV4S2 = [((2, 8, 16, 2, 2), dt) for dt in (BF, F32)] + [((1, 16, 8, 6, 10), dt) for dt in (BF, F32)] + \
          [((3, 24, 40, 36, 20), dt) for dt in (BF, F32)]  # (N, Cin, Cout, H, W); the last one is split-K


# ------------------------------------------------------------------------------------------ builders


def _embed(t, pad, fill=E.SENTINEL):
    """[..., C] inside a wider buffer [..., lo + C + hi] whose other channels hold the sentinel."""
    lo, hi = pad
    if lo == hi == 0:
        return t
    out = torch.full(t.shape[:-1] + (lo + t.shape[-1] + hi,), fill, dtype=t.dtype)
    out[..., lo:lo + t.shape[-1]] = t
    return out


def _padc(t, cp):
    out = torch.zeros(t.shape[:-1] + (cp,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def build_fwd(c):
    """Stored operands, call arguments and the float64 result of a forward case.  Returns a namespace:
    x, w, bias, ops (epilogue tensors as stored, NHWC), kw (scalars of the call), ref (as stored: NHWC, or NCHW
    for the tail), stages, abs_sum, prep (the prepared_images shape tuple), ybuf (shape, coff, C), colsum_ref."""
    if c.data in _BUILT:
        return _BUILT[c.data]
    g = E.gen_for(c.data)
    N, H, W, cin, cout = c.shape
    dt = DT[c.dtype]
    cin_p, cout_p, k = E.pad8(cin), E.pad8(cout), c.ksize
    b = _ns(kw={}, ops={})
    # input as stored
    if c.mode != 'dense':
        assert not (c.in_ps or c.in_up)
        xs = E.impulse((N, H, W, cin), c.mode[1])
    elif c.in_ps:
        r = c.in_ps
        xs = E.grid((N, H * r, W * r, cin // (r * r)), gen=g)
    elif c.in_up:
        xs = E.grid((N, H // c.in_up, W // c.in_up, cin), gen=g)
    else:
        xs = E.grid((N, H, W, cin), gen=g)
    xl = E.gather_input(xs, c.in_up, c.in_ps)
    stored_c = xs.shape[-1] if c.in_ps else cin_p
    b.x = E.store(_embed(_padc(xs, stored_c), c.xpad), dt)
    b.kw.update(ldx=b.x.shape[-1], xcoff=c.xpad[0])
    for key in ('in_ps', 'in_up', 'out_ps'):
        if getattr(c, key):
            b.kw[key] = getattr(c, key)
    if k != 3:
        b.kw['ksize'] = k
    w = E.grid((cout, cin, k, k), scale=0.125, gen=g)
    b.w = w.float()
    b.prep = (cout, cin, cout_p, cin_p, c.out_ps, k)
    e = _ns(out_ps=c.out_ps)

    def operand(name):  # an epilogue map: float64 NCHW for the reference, stored NHWC (padded channels 0) for the call
        t = E.grid((N, H, W, cout), gen=g)
        b.ops[name] = E.store(_padc(t, cout_p), dt)
        setattr(e, name, E.nchw(t))

    epi = c.epi
    if epi in ('bias', 'full', 'relu', 'lrelu', 'colsum', 'colsum_plain', 'res', 'affine'):
        e.bias = E.grid((cout,), -8, 8, 0.125, gen=g)
    if epi in ('full', 'lrelu'):
        e.act, e.slope = E.ACT_LRELU, E.SLOPE
    if epi in ('relu', 'colsum'):
        e.act = E.ACT_RELU
    if epi in ('full', 'res', 'dot'):
        operand('res')
        e.beta = 1.0
    if epi == 'gate_alpha_res':
        operand('gate')
        operand('res')
        e.gate_slope, e.alpha, e.beta = E.SLOPE, E.ALPHA, 0.5
    if epi == 'gate':
        operand('gate')
        e.gate_slope, e.alpha = E.SLOPE, E.ALPHA
    if epi == 'res2_rowscale':
        operand('res')
        operand('res2')
        e.beta, e.beta2 = 1.0, E.BETA2
        e.row_scale = E.choice((N,), (0.5, 1.0, 2.0), gen=g)
    if epi == 'rrdb_dgrad':
        operand('res')
        operand('gate')
        e.alpha, e.beta, e.rcols = E.ALPHA, 1.0, min(64, cout)
        e.gate_slope, e.gate_mode, e.gcol0, e.gcol1 = E.SLOPE, 2, cout - 32, cout
    if epi == 'affine':
        e.aff_scale = E.choice((cout,), (0.5, 1.0, 2.0), gen=g)
        e.aff_shift = E.grid((cout,), -8, 8, 0.125, gen=g)
    if epi == 'dot':
        t = E.grid((N, H, W, cout), gen=g)
        b.ops['dot'], dot = E.store(t, dt), t
    b.colsum = epi in ('colsum', 'colsum_plain', 'dot')
    for key in ('act', 'slope', 'gate_slope', 'alpha', 'beta', 'beta2', 'rcols', 'gate_mode', 'gcol0', 'gcol1'):
        if hasattr(e, key):
            b.kw[key] = getattr(e, key)
    b.bias = e.bias.float() if hasattr(e, 'bias') else None
    for key in ('row_scale', 'aff_scale', 'aff_shift'):
        if hasattr(e, key):
            b.ops[key] = getattr(e, key).float()
    # the float64 result
    if c.mode != 'dense':
        acc = E.impulse_acc((N, H, W, cin), c.mode[1], w)
        mag = acc.abs()
    else:
        acc, mag = E.conv_acc(xl, w)
    y, b.stages = E.epilogue(acc, e)
    b.abs_sum = [('conv', mag, 0.125)]
    b.xl, b.w64, b.e, b.acc = xl, w, e, acc
    if c.nchw:
        b.ref = y.contiguous()
        b.ybuf = ((N, cout, H, W), 0, cout)
        b.kw['out_nchw'] = True
    else:
        b.ref = E.nhwc(y)
        cs = b.ref.shape[-1]  # cout, or cout / r^2 of a pixel-shuffled store
        b.ybuf = (b.ref.shape[:3] + (c.ypad[0] + cs + c.ypad[1],), c.ypad[0], cs)
        b.kw['ycoff'] = c.ypad[0]
    if b.colsum:
        ys = E.to_stored(b.ref, dt).double()
        terms = ys * dot if epi == 'dot' else ys
        b.colsum_ref = terms.sum((1, 2))
        b.stages.append(('channel sums', b.colsum_ref))
        b.abs_sum.append(('channel sums', terms.abs().sum((1, 2)), E.quantum(terms)))
    _BUILT[c.data] = b
    return b


def build_wgrad(c):
    """Stored operands and the float64 gradients of a weight-gradient case: x, dy, kw, ref (overwrite), acc
    (accumulate onto init = (dw0, db0)), stages, abs_sum."""
    if c.data in _BUILT:
        return _BUILT[c.data]
    g = E.gen_for(c.data)
    N, H, W, cin, cout = c.shape
    dt = DT[c.dtype]
    up, ps, k = max(c.in_up, 1), max(c.ps, 1), c.ksize
    b = _ns(kw={})
    xs = _padc(E.grid((N, H // up, W // up, c.cin_real), gen=g), cin)
    dys = E.grid((N, H * ps, W * ps, cout // (ps * ps)), gen=g)
    b.x, b.dy = E.store(_embed(xs, c.xpad), dt), E.store(_embed(dys, c.ypad), dt)
    b.kw.update(ldx=b.x.shape[-1], xcoff=c.xpad[0], ldy=b.dy.shape[-1], ycoff=c.ypad[0])
    if c.in_up:
        b.kw['in_up'] = c.in_up
    if k != 3:
        b.kw['ksize'] = k
    xl = E.gather_input(xs[..., :c.cin_real], c.in_up)
    dyl = E.pixel_unshuffle_nchw(dys, ps)
    b.init = (E.grid((cout, c.cin_real, k, k), gen=g), E.grid((cout,), gen=g))
    b.ref = E.wgrad_ref(xl, dyl, k, c.scale)
    b.acc = E.wgrad_ref(xl, dyl, k, c.scale, init=b.init)
    b.stages = b.ref.stages + b.acc.stages
    b.abs_sum = [('dw', b.ref.mag_w + b.init[0].abs(), 1.0), ('db', b.ref.mag_b + b.init[1].abs(), 1.0)]
    b.xl, b.dyl = xl, dyl
    _BUILT[c.data] = b
    return b


def build_convk(k, ch, shape):
    """Operands (float64, NHWC) and results of a k x k conv case: forward without and with ReLU, input gradient,
    weight / bias gradient at scale 0.5."""
    key = ('convk', k, ch, shape)
    if key not in _BUILT:
        (cin, cout), (N, H, W) = ch, shape
        g = E.gen_for(f'convk-{k}-{cin}-{cout}-{N}-{H}-{W}')
        b = _ns(xs=E.grid((N, H, W, cin), gen=g), dys=E.grid((N, H, W, cout), gen=g),
                w=E.grid((cout, cin, k, k), scale=0.125, gen=g), bias=E.grid((cout,), -8, 8, 0.125, gen=g))
        xl, dyl = E.nchw(b.xs), E.nchw(b.dys)
        acc, mag = E.conv_acc(xl, b.w)
        b.fwd = {act: E.epilogue(acc, _ns(bias=b.bias, act=act)) for act in (E.ACT_NONE, E.ACT_RELU)}
        b.dx, dmag = E.conv_acc(dyl, b.w, transpose=True)
        b.wr = E.wgrad_ref(xl, dyl, k, 0.5)
        b.stages = b.fwd[0][1] + b.fwd[1][1] + [('dx', b.dx)] + b.wr.stages
        b.abs_sum = [('conv', mag, 0.125), ('dgrad', dmag, 0.125), ('dw', b.wr.mag_w, 1.0), ('db', b.wr.mag_b, 1.0)]
        _BUILT[key] = b
    return _BUILT[key]


def build_conv4s2(case):
    """The same for the bias-free 4x4 stride-2 conv, case = (N, Cin, Cout, H, W)."""
    key = ('conv4s2', case)
    if key not in _BUILT:
        N, cin, cout, H, W = case
        g = E.gen_for('conv4s2-' + '-'.join(map(str, case)))
        b = _ns(xs=E.grid((N, H, W, cin), gen=g), dys=E.grid((N, H // 2, W // 2, cout), gen=g),
                w=E.grid((cout, cin, 4, 4), scale=0.125, gen=g))
        xl, dyl = E.nchw(b.xs), E.nchw(b.dys)
        b.y, mag = E.conv_acc(xl, b.w, stride=2)
        b.dx, dmag = E.conv_acc(dyl, b.w, transpose=True, stride=2)
        b.wr = E.wgrad_ref(xl, dyl, 4, 0.5, stride=2)
        b.stages = [('y', b.y), ('dx', b.dx)] + b.wr.stages
        b.abs_sum = [('conv', mag, 0.125), ('dgrad', dmag, 0.125), ('dw', b.wr.mag_w, 1.0)]
        _BUILT[key] = b
    return _BUILT[key]


def smallest(cases, gathers=True):
    """The smallest case (by multiply-adds) with more than one image row of every family in a table;
    ``gathers=False``: among the cases that read their input as stored (no in_ps / in_up)."""
    out = {}
    for c in cases:
        N, H, W, cin, cout = c.shape
        size = N * H * W * cin * cout
        if H == 1 or (not gathers and (c.in_ps or c.in_up)):
            continue
        if c.family not in out or size < out[c.family][0]:
            out[c.family] = (size, c)
    return [c for _, c in out.values()]
