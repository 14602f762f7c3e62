"""Exact-arithmetic tests of the conv GEMM kernels: integer-grid operands, bit for bit against float64.

Every operand is a small integer times a power of two (maps, dy, res, res2, gate, dot in {-3..3}; weights
{-3..3}/8; bias {-8..8}/8) and every slope / scale a power of two, so every product, partial sum, split-K slab,
atomic add and epilogue step is exact in fp32 (tests/_exact.py::assert_exactness checks that for each case before
the device is touched).  The kernel's result must then equal the float64 result exactly: fp32 outputs as they
are, bf16 outputs after one round-to-nearest-even.  A dropped, duplicated or misplaced term at one border pixel,
halo column, strip seam or ragged K chunk is a hard mismatch, and assert_bits reports its pattern.

Each case asserts the kernel the dispatch will launch under the variant that forces it, poisons the output with
NaN and the channels around an output slice with a sentinel that must stay bit-unchanged.  tests/_exact_cases.py
holds the case tables (tests/test_exact_grid_host.py proves on the CPU that single defects are rejected).

Not covered, because no operand grid makes them exact in fp32: the GELU ``aux`` store and ``gate_mode=1``,
LN-fused linears and sigmoid.  Their conv parts run the same kernels as the plain epilogue cases here.  DCN's
bilinear sampling is exact on a quarter-pixel offset lattice and is covered by tests/test_dcn_exact_gpu.py.

One assumption is not provable on the host: that the MFMA units keep multiples of the quantum exact while all
magnitudes stay below 2^20 quanta.  A mismatch confined to dense large-K cases would point there."""
import contextlib

import pytest
import torch

from basicsr4rs_amd import _lib
from basicsr4rs_amd.ops import conv as C

from . import _exact as E
from . import _exact_cases as X
from ._fp64 import _assert_outside_unchanged

pytestmark = pytest.mark.gpu
NAN = float('nan')


@contextlib.contextmanager
def forced(variant, knobs):
    """The kernel-selection variant and tuning knobs of a case; variant 0 and the knobs restored on exit."""
    lib = _lib.load()
    with contextlib.ExitStack() as st:
        for name, value in knobs.items():
            st.enter_context(_lib.knob(name, value))
        _lib.check(lib.sr_conv3x3_set_variant(variant))
        try:
            yield lib
        finally:
            _lib.check(lib.sr_conv3x3_set_variant(0))


def fwd_desc(c, b):
    N, H, W, cin, cout = c.shape
    kw = dict(b.kw)
    ldx = kw.pop('ldx')
    return C._desc(X.DT[c.dtype], N, H, W, E.pad8(cin), ldx, E.pad8(cout), cout, 0 if c.nchw else b.ybuf[0][-1], **kw)


def wgrad_desc(c, b):
    N, H, W, cin, cout = c.shape
    d = _lib.WgradDesc()
    d.dtype, d.N, d.H, d.W = _lib.dtype_code(X.DT[c.dtype]), N, H, W
    d.Cin, d.Cin_real, d.ldx, d.xcoff = cin, c.cin_real, b.kw['ldx'], b.kw['xcoff']
    d.Cout, d.Cout_real, d.ldy, d.ycoff, d.out_ps = cout, cout, b.kw['ldy'], b.kw['ycoff'], c.ps
    d.scale, d.in_up, d.ksize = c.scale, c.in_up, c.ksize
    return d


def _run_fwd(cuda, c):
    b = X.build_fwd(c)
    E.assert_exactness(b.stages, b.abs_sum)
    dt = X.DT[c.dtype]
    N, H, W, cin, cout = c.shape
    ops = {k: v.to(cuda) for k, v in b.ops.items()}
    x, w = b.x.to(cuda), b.w.to(cuda)
    bias = b.bias.to(cuda) if b.bias is not None else None
    shape, coff, cs = b.ybuf
    y = torch.full(shape, NAN, device=cuda, dtype=torch.float32 if c.nchw else dt)
    if not c.nchw:
        y[..., :coff] = E.SENTINEL
        y[..., coff + cs:] = E.SENTINEL
    before = y.clone()
    with forced(c.variant, c.knobs) as lib:
        name = lib.sr_conv3x3_fwd_kernel_name(fwd_desc(c, b)).decode()
        assert name.startswith(c.kernel), f'{c.id}: the dispatch chose {name}, the case is about {c.kernel}'
        wf, _, bg = C.prepared_images(w, bias, dt, b.prep)
        extra = {k: ops[k] for k in ('row_scale', 'dot') if k in ops}
        out = C.conv_fwd_raw(x, wf, bg if bias is not None else None, y, N, H, W, E.pad8(cin), E.pad8(cout), cout,
                             gate=ops.get('gate'), res=ops.get('res'), res2=ops.get('res2'),
                             aff_scale=ops.get('aff_scale'), aff_shift=ops.get('aff_shift'), colsum=b.colsum,
                             **b.kw, **extra)
        torch.cuda.synchronize()
    if c.nchw:
        E.assert_bits(y, b.ref, c.id, axes='ncyx')
        return
    _assert_outside_unchanged(y, before, coff, cs, c.id)
    got = y[..., coff:coff + cs]
    E.assert_bits(got, b.ref, c.id)
    if b.colsum:  # the partial rows, summed, are the sums of y as stored (of y * dot): fp32 sums of exact terms
        sums = out[1].double().sum(1).cpu()
        bad = int((sums != b.colsum_ref).sum())
        assert bad == 0, f'{c.id}: {bad} of {sums.numel()} fused channel sums differ from the sums of the stored y'


@pytest.mark.parametrize('case', X.FWD, ids=lambda c: c.id)
def test_conv_fwd_exact(cuda, case):
    """conv_fwd_raw, dense grid operands: every forward kernel family, plain and full epilogues."""
    _run_fwd(cuda, case)


@pytest.mark.parametrize('case', X.FWD_IMPULSE, ids=lambda c: c.id)
def test_conv_fwd_impulse(cuda, case):
    """conv_fwd_raw on a single 1 at an image corner, a strip seam, the last pixel, the ends of the last channel
    chunk: the output is the weight image, placed and clipped (bf16-exact: no rounding can mask anything)."""
    _run_fwd(cuda, case)


@pytest.mark.parametrize('shape,kernel', [((2, 4, 64, 256, 1024, 2), X.PPH), ((2, 4, 64, 64, 576, 3), X.HALO),
                                          ((1, 20, 36, 256, 512, 0), X.PP)], ids=lambda v: str(v).replace(' ', ''))
def test_conv_dgrad_exact(cuda, shape, kernel):
    """The input gradient as the nets compute it: conv_fwd_raw on the dgrad weight image of a (pixel-shuffling)
    conv, reading the HR output gradient through in_ps -- against conv_transpose2d of the unshuffled gradient, so
    the image's K order and the gather agree (the forward cases prepare an unshuffled weight over the LR map)."""
    N, H, W, cin, cout, r = shape
    g = E.gen_for('dgrad-' + '-'.join(map(str, shape)))
    rr = max(r, 1)
    dys = E.grid((N, H * rr, W * rr, cout // (rr * rr)), gen=g)
    w = E.grid((cout, cin, 3, 3), scale=0.125, gen=g)
    ref, mag = E.conv_acc(E.pixel_unshuffle_nchw(dys, rr), w, transpose=True)
    E.assert_exactness([('dx', ref)], [('dgrad', mag, 0.125)])
    dt = torch.bfloat16
    _, wd, _ = C.prepared_images(w.float().to(cuda), None, dt, (cout, cin, cout, cin, r, 3))
    dy = E.store(dys, dt).to(cuda)
    dx = torch.full((N, H, W, cin), NAN, device=cuda, dtype=dt)
    lib = _lib.load()
    name = lib.sr_conv3x3_fwd_kernel_name(C._desc(dt, N, H, W, cout, dy.shape[-1], cin, cin, cin, in_ps=r)).decode()
    assert name == kernel, name
    C.conv_fwd_raw(dy, wd, None, dx, N, H, W, cout, cin, cin, in_ps=r, ldx=dy.shape[-1])
    torch.cuda.synchronize()
    E.assert_bits(dx, E.nhwc(ref), f'dgrad {shape}')


def test_conv3x3_kpad_exact(cuda, monkeypatch):
    """SwinIR's 180 -> 180 conv (184-channel rows) with K-padded weight images through ops.conv.conv3x3: forward
    with bias and residual on the halo-row 256x256 kernel with a partial output tile, and its backward."""
    from basicsr4rs_amd.utils import ktrace
    N, H, W, cin, cout = 1, 8, 128, 180, 180
    g = E.gen_for('kpad-180')
    xs, res, gy = (E.grid((N, H, W, cin), gen=g) for _ in range(3))
    w, bias = E.grid((cout, cin, 3, 3), scale=0.125, gen=g), E.grid((cout,), -8, 8, 0.125, gen=g)
    xl, gyl = E.nchw(xs), E.nchw(gy)
    acc, mag = E.conv_acc(xl, w)
    e = X._ns(bias=bias, res=E.nchw(res), beta=1.0)
    yref, stages = E.epilogue(acc, e)
    dx, dmag = E.conv_acc(gyl, w, transpose=True)
    wr = E.wgrad_ref(xl, gyl, 3)
    E.assert_exactness(stages + [('dx', dx)] + wr.stages,
                       [('conv', mag, 0.125), ('dgrad', dmag, 0.125), ('dw', wr.mag_w, 1.0), ('db', wr.mag_b, 1.0)])
    monkeypatch.setenv('SR_CONV_KPAD', '1')
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).to(cuda)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(bias.float())
    dt = torch.bfloat16
    up = lambda t: E.store(X._padc(t, 184), dt).to(cuda)  # noqa: E731
    xx = up(xs).requires_grad_()
    ktrace.start()
    try:
        y = C.conv3x3(xx, conv, res=up(res))
        y.backward(up(gy))
        torch.cuda.synchronize()
    finally:
        ran = set(ktrace.stop())
    assert 'conv3x3_fwd_pph_kernel' in ran, ran
    E.assert_bits(y.detach()[..., :cout], E.nhwc(yref), 'kpad y')
    E.assert_bits(xx.grad[..., :cin], E.nhwc(dx), 'kpad dx')
    E.assert_bits(conv.weight.grad, wr.dw, 'kpad dW', axes=('co', 'ci', 'ky', 'kx'))
    E.assert_bits(conv.bias.grad, wr.db, 'kpad db', axes=('co',))


# ------------------------------------------------------------------------------------------ weight gradients

WAX = ('co', 'ci', 'ky', 'kx')


def _flat_param(init, cuda):
    """A parameter whose gradient lives in a flat-gradient view pre-filled with ``init`` (what
    utils.flat.FlatParams binds): the kernels accumulate into it."""
    p = torch.nn.Parameter(torch.zeros(init.shape, device=cuda))
    view = init.float().to(cuda)
    p._sr_grad_view, p._sr_flat = view, True
    p.grad = view
    return p


@pytest.mark.parametrize('case', X.WGRAD, ids=lambda c: c.id)
def test_conv_wgrad_exact(cuda, case):
    """conv_wgrad_raw: fp32 dW / db equal the float64 sums exactly, overwriting and accumulating onto grid
    values; a repeat call is bitwise equal."""
    c = case
    b = X.build_wgrad(c)
    E.assert_exactness(b.stages, b.abs_sum)
    N, H, W, cin, cout = c.shape
    x, dy = b.x.to(cuda), b.dy.to(cuda)
    pw, pb = _flat_param(b.init[0], cuda), _flat_param(b.init[1], cuda)

    def call(params=None):
        return C.conv_wgrad_raw(dy, x, N, H, W, cin, c.cin_real, cout, cout, scale=c.scale, out_ps=c.ps, params=params,
                                **b.kw)

    with forced(c.variant, c.knobs) as lib:
        name = lib.sr_conv3x3_wgrad_kernel_name(wgrad_desc(c, b)).decode()
        assert name == c.kernel, f'{c.id}: the dispatch chose {name}, the case is about {c.kernel}'
        dw, db = call()
        dw2, db2 = call()
        assert call((pw, pb)) == (None, None)
        torch.cuda.synchronize()
    E.assert_bits(dw, b.ref.dw, c.id + ' dW', axes=WAX)
    E.assert_bits(db, b.ref.db, c.id + ' db', axes=('co',))
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f'{c.id}: a repeat call differs'
    E.assert_bits(pw.grad, b.acc.dw, c.id + ' dW accumulated', axes=WAX)
    E.assert_bits(pb.grad, b.acc.db, c.id + ' db accumulated', axes=('co',))


def test_conv_wgrad_pair_exact(cuda):
    """conv_wgrad_pair_raw (both convs of a residual block in one launch): both blocks' dW / db, accumulated onto
    grid values with scales 1 and 0.5, equal float64 exactly; a repeat call from the same start is bitwise equal."""
    N, H, W, cin, cout = X.PAIR_SHAPE
    cases = [X.wg(f'pair{i}', X.PAIR_SHAPE, 0, X.ROW3, scale=s) for i, s in enumerate(X.PAIR_SCALES)]
    built = [X.build_wgrad(c) for c in cases]
    for b in built:
        E.assert_exactness(b.stages, b.abs_sum)
    lib = _lib.load()
    assert lib.sr_conv3x3_wgrad_kernel_name(wgrad_desc(cases[0], built[0])) == X.ROW3.encode()
    runs = []
    for _ in range(2):
        params = [(_flat_param(b.init[0], cuda), _flat_param(b.init[1], cuda)) for b in built]
        items = [(b.dy.to(cuda), b.x.to(cuda), c.scale, p) for b, c, p in zip(built, cases, params)]
        assert C.conv_wgrad_pair_raw(items, N, H, W, cin, cin, cout, cout), 'the paired launch did not run'
        torch.cuda.synchronize()
        runs.append(params)
    for i, (b, (pw, pb)) in enumerate(zip(built, runs[0])):
        E.assert_bits(pw.grad, b.acc.dw, f'pair item {i} dW', axes=WAX)
        E.assert_bits(pb.grad, b.acc.db, f'pair item {i} db', axes=('co',))
        assert torch.equal(pw.grad, runs[1][i][0].grad) and torch.equal(pb.grad, runs[1][i][1].grad)


# ------------------------------------------------------------------------------------------ k x k, 4x4 stride 2


@pytest.mark.parametrize('k,ch,shape,dtype', X.CONVK,
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_convk_exact(cuda, k, ch, shape, dtype):
    """convk_fwd_raw (with and without ReLU), the input gradient on the flipped image and convk_wgrad_raw."""
    from basicsr4rs_amd.ops import convk as K
    (cin, cout), (N, H, W), dt = ch, shape, X.DT[dtype]
    cin_p, cout_p = E.pad8(cin), E.pad8(cout)
    b = X.build_convk(k, ch, shape)
    E.assert_exactness(b.stages, b.abs_sum)
    xs, dys, w, bias, refs, dx, wr = b.xs, b.dys, b.w, b.bias, b.fwd, b.dx, b.wr
    wp, bp = w.float().to(cuda), bias.float().to(cuda)
    wf, wd, bg = C.prepared_images(wp, bp, dt, (cout, cin, cout_p, cin_p, 0, k))
    xg, dyg = E.store(X._padc(xs, cin_p), dt).to(cuda), E.store(X._padc(dys, cout_p), dt).to(cuda)
    tag = f'convk k{k} {cin}->{cout} {N}x{H}x{W} {dtype}'
    for act, (ref, _) in refs.items():
        y = K.convk_fwd_raw(xg, wf, bg, k, cout_p, cout, act=act)
        E.assert_bits(y[..., :cout], E.nhwc(ref), f'{tag} fwd act {act}')
        assert float(y[..., cout:].float().abs().sum()) == 0.0, tag
    gx = K.convk_fwd_raw(dyg, wd, None, k, cin_p, cin)
    E.assert_bits(gx[..., :cin], E.nhwc(dx), f'{tag} dgrad')
    assert float(gx[..., cin:].float().abs().sum()) == 0.0, tag
    dw, db = K.convk_wgrad_raw(dyg, xg, k, cin, cout, scale=0.5)
    dw2, db2 = K.convk_wgrad_raw(dyg, xg, k, cin, cout, scale=0.5)
    E.assert_bits(dw, wr.dw, f'{tag} dW', axes=WAX)
    E.assert_bits(db, wr.db, f'{tag} db', axes=('co',))
    assert torch.equal(dw, dw2) and torch.equal(db, db2), tag


@pytest.mark.parametrize('case,dtype', X.CONV4S2, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv4s2_exact(cuda, case, dtype):
    """The discriminator's 4x4 stride-2 conv: forward, input gradient and (split-K at the last case) weight
    gradient."""
    from basicsr4rs_amd.ops import gan as G
    (N, cin, cout, H, W), dt = case, X.DT[dtype]
    if case == X.CONV4S2[-1][0]:
        assert _lib.load().sr_conv4s2_wgrad_splits(N, H, W, cin, cout) > 1
    b = X.build_conv4s2(case)
    E.assert_exactness(b.stages, b.abs_sum)
    xs, dys, w, acc, dx, wr = b.xs, b.dys, b.w, b.y, b.dx, b.wr
    wp = torch.nn.Parameter(w.float().to(cuda))
    wf, wd = G.conv4s2_images(wp, dt)
    xg, dyg = E.store(xs, dt).to(cuda), E.store(dys, dt).to(cuda)
    tag = f'conv4s2 {case} {dtype}'
    E.assert_bits(G.conv4s2_fwd_raw(xg, wf, cout), E.nhwc(acc), tag + ' fwd')
    E.assert_bits(G.conv4s2_dgrad_raw(dyg, wd, H, W, cin), E.nhwc(dx), tag + ' dgrad')
    dw = G.conv4s2_wgrad_raw(dyg, xg, cin, cout, scale=0.5)
    dw2 = G.conv4s2_wgrad_raw(dyg, xg, cin, cout, scale=0.5)
    E.assert_bits(dw, wr.dw, tag + ' dW', axes=WAX)
    assert torch.equal(dw, dw2), tag
