"""The EDVR kernels (csrc/edvr.hip through ops/edvr.py) against float64 computed on the CPU from tests/_edvr_ref.py
(checked on the host by tests/test_edvr_ref_host.py), never against the code under test.

Bounds.  conv3s2 on integer grids: bit for bit (tests/_exact.py).  conv3s2 on random operands: the suite's conv bound
(K + 2) U sum|x w| per element, U = 2^-24, K the reduction length (9 Cin forward, at most 4 Cout dgrad, N Ho Wo wgrad),
plus one bf16 ulp for bf16 outputs (tests/_fp64.py:_check, the convention of tests/test_unet_disc_ops_gpu.py); the
LeakyReLU is 1-Lipschitz and leaves it unchanged; bf16 references from operands as the engine holds them (weights and
the activation backward's output rounded to bf16).  pool3s2: the max half is a selection, bit for bit; the average
half bit for bit where the window sums are multiples of 9, else (9 + 1) U sum|x| / 9 (nine adds and a division),
bf16 plus half a bf16 ulp of the result; the backward sums at most 4 + 4 gradients and divides once:
10 U (sum|dy_max chosen| + sum|dy_avg| / 9).  tsa_corr / tsa_modulate chain a dot product, a device exp and products:
the replay convention, per output tensor by relative L2: fp32 within 8 x the error of the same formulas in fp32 on
the CPU, bf16 within 2 x the error of a float64 run whose operands and stored outputs are rounded to bf16.  The op
takes ``emb_ref`` as a tensor of its own (the arch computes it with its own conv from the centre frame), so a centre
index away from the middle is exercised by the arch test (tests/test_edvr_arch_gpu.py, 5 frames with the centre at 1).
Every measured error is printed beside its bound."""
import functools

import pytest
import torch
from torch.nn import functional as F

from . import _edvr_ref as R
from ._exact import assert_bits, assert_exactness, conv_acc, gen_for, grid, nchw, nhwc, store, wgrad_ref
from ._fp64 import U, _bf16_ulp, _bits, _check, _ids, _rne_bf16

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
SLOPE = 0.25  # a power of two: exact on the grids


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _conv(cin, cout, w64, b64):
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w64.float())
        conv.bias.copy_(b64.float())
    return conv


# ----------------------------------------------------------------------------------------- conv3s2, exact

C3_SHAPES = [(1, 4, 4), (2, 6, 10), (1, 7, 9), (1, 16, 66), (1, 32, 33)]
C3_CHANNELS = [(64, 64), (128, 128), (16, 24)]


def test_conv3s2_split_plan():
    """(1, 32, 33) has 16 x 17 = 272 output pixels, the smallest count above one 256-pixel split-K block that a
    single image reaches with H, W >= 2; 16 x 16 = 256 still fits one."""
    from basicsr4rs_amd import _lib
    lib = _lib.load()
    for cin, cout in C3_CHANNELS:
        assert lib.sr_conv3s2_wgrad_splits(1, 32, 33, cin, cout) == 2
        assert lib.sr_conv3s2_wgrad_splits(1, 32, 31, cin, cout) == 1
        assert lib.sr_conv3s2_wgrad_workspace(1, 32, 33, cin, cout) == 2 * cout * 9 * cin * 4


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('ch', C3_CHANNELS, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('shape', C3_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv3s2_exact(shape, ch, dtype):
    """Integer-grid operands: forward (bias + LeakyReLU 1/4), dgrad and wgrad / bias gradient equal float64 bit for
    bit; the dgrad buffer is pre-filled with NaN and holds none afterwards."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import edvr as E
    (N, H, W), (cin, cout) = shape, ch
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = gen_for(f'c3 exact {shape} {ch}')
    x64 = grid((N, H, W, cin), -3, 3, gen=g)
    w64 = grid((cout, cin, 3, 3), -2, 2, 0.5, gen=g)
    b64 = grid((cout, ), -4, 4, 0.5, gen=g)
    dy64 = grid((N, Ho, Wo, cout), -2, 2, gen=g)
    acc, mag = conv_acc(nchw(x64), w64, stride=2)
    z = acc + b64.view(1, -1, 1, 1)
    y64 = torch.where(z > 0, z, z * SLOPE)
    dz = torch.where(z > 0, nchw(dy64), nchw(dy64) * SLOPE)
    dx64 = torch.nn.grad.conv2d_input((N, cin, H, W), w64, dz, stride=2, padding=1)
    mag_dx = torch.nn.grad.conv2d_input((N, cin, H, W), w64.abs(), dz.abs(), stride=2, padding=1)
    wg = wgrad_ref(nchw(x64), dz, 3, stride=2)
    assert_exactness([('acc', acc), ('y', y64), ('dz', dz), ('dx', dx64), ('dw', wg.dw), ('db', wg.db)],
                     [('fwd', mag, 0.5), ('dgrad', mag_dx, 0.125), ('wgrad', wg.mag_w, 0.25)])
    assert tuple(acc.shape) == (N, cout, Ho, Wo)

    conv = _conv(cin, cout, w64, b64)
    x = store(x64, dtype).cuda().requires_grad_(True)
    y = E.conv3s2(x, conv, act=_lib.ACT_LRELU, slope=SLOPE)
    assert y.shape == (N, Ho, Wo, cout) and y.dtype == dtype
    y.backward(store(dy64, dtype).cuda())
    assert_bits(y, nhwc(y64), f'conv3s2 fwd {shape} {ch}')
    assert_bits(x.grad, nhwc(dx64), f'conv3s2 dgrad {shape} {ch}')
    assert_bits(conv.weight.grad, wg.dw, f'conv3s2 wgrad {shape} {ch}', axes='oikl')
    assert_bits(conv.bias.grad, wg.db, f'conv3s2 bias grad {shape} {ch}', axes='o')
    # every dx element written: the raw call into a NaN-filled buffer
    lib = _lib.load()
    wd = E.conv3s2_images(conv.weight, dtype)[1]
    dzs = store(nhwc(dz), dtype).cuda()
    buf = torch.full((N, H, W, cin), float('nan'), dtype=dtype, device='cuda')
    _lib.check(lib.sr_conv3s2_dgrad(_lib.dtype_code(dtype), _lib.ptr(dzs), _lib.ptr(wd), N, H, W, cin, cout, _lib.ptr(buf),
                                    _lib.stream()))
    assert not torch.isnan(buf).any(), 'dgrad left elements unwritten'
    assert_bits(buf, nhwc(dx64), f'conv3s2 dgrad raw {shape} {ch}')


def test_conv3s2_padded_channels_and_no_bias():
    """3 -> 20 channels (both padded to 8 / 24) without a bias, no activation: padded output channels are zeros and
    the gradients come back in the parameter's own shape."""
    from basicsr4rs_amd.ops import edvr as E
    g = gen_for('c3 padded')
    conv = torch.nn.Conv2d(3, 20, 3, 2, 1, bias=False).cuda()
    w64 = grid((20, 3, 3, 3), -2, 2, 0.5, gen=g)
    with torch.no_grad():
        conv.weight.copy_(w64.float())
    x64 = torch.zeros(2, 5, 6, 8, dtype=torch.float64)
    x64[..., :3] = grid((2, 5, 6, 3), -3, 3, gen=g)
    dy64 = grid((2, 3, 3, 24), -2, 2, gen=g)
    x = x64.float().cuda().requires_grad_(True)
    y = E.conv3s2(x, conv)
    y.backward(dy64.float().cuda())
    z, _ = conv_acc(nchw(x64)[:, :3], w64, stride=2)
    assert_bits(y[..., :20], nhwc(z), 'conv3s2 padded fwd')
    assert not y[..., 20:].any()
    dzl = nchw(dy64)[:, :20]
    dx = torch.nn.grad.conv2d_input((2, 3, 5, 6), w64, dzl, stride=2, padding=1)
    assert_bits(x.grad[..., :3], nhwc(dx), 'conv3s2 padded dgrad')
    assert not x.grad[..., 3:].any()
    assert_bits(conv.weight.grad, wgrad_ref(nchw(x64)[:, :3], dzl, 3, stride=2).dw, 'conv3s2 padded wgrad', axes='oikl')


# ---------------------------------------------------------------------------------------- conv3s2, random

C3_RANDOM = [(16, 24, 7, 9, 2), (64, 64, 16, 18, 2), (128, 128, 12, 8, 1), (64, 64, 32, 33, 1)]


def _c3_random_run(case, dtype, act):
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import edvr as E
    cin, cout, H, W, N = case
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = gen_for(f'c3 random {case}')
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin))**0.5
    b = torch.randn(cout, generator=g) * 0.1
    conv = _conv(cin, cout, w.double(), b.double())
    x = torch.randn(N, H, W, cin, generator=g).to(dtype)
    w64, b64, x64 = w.double(), b.double(), nchw(x.double())
    if dtype == torch.bfloat16:
        w64 = _rne_bf16(w64)
    z = F.conv2d(x64, w64, b64, stride=2, padding=1)
    mag = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2, padding=1)
    fb = mag * (9 * cin + 2) * U
    dy = torch.randn(N, Ho, Wo, cout, generator=g)
    if act:  # within the forward bound of zero a gate may legitimately flip: no gradient there
        dy = dy * nhwc((z.abs() > fb).double()).float()
        assert (dy != 0).float().mean() > 0.9
    dy = dy.to(dtype)
    xg = x.cuda().requires_grad_(True)
    y = E.conv3s2(xg, conv, act=_lib.ACT_LRELU if act else _lib.ACT_NONE, slope=0.1)
    y.backward(dy.cuda())
    return dict(y=y.detach(), dx=xg.grad, dw=conv.weight.grad, db=conv.bias.grad), (x64, w64, z, fb, nchw(dy.double()))


@pytest.mark.parametrize('act', [False, True], ids=['none', 'lrelu'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('case', C3_RANDOM, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3s2_random(case, dtype, act):
    cin, cout, H, W, N = case
    got, (x64, w64, z, fb, dy64) = _c3_random_run(case, dtype, act)
    slope = float(torch.tensor(0.1, dtype=torch.float32))
    _check(got['y'], nhwc(torch.where(z > 0, z, z * slope) if act else z), nhwc(fb), f'conv3s2 fwd {case}')
    dz = dy64
    if act:  # the activation backward's output as the engine holds it: fp32 product, then the storage dtype
        dz = torch.where(z > 0, dy64, (dy64 * slope).float().double())
        if dtype == torch.bfloat16:
            dz = _rne_bf16(dz)
    shape = (N, cin, H, W)
    ref_dx = torch.nn.grad.conv2d_input(shape, w64, dz, stride=2, padding=1)
    mag_dx = torch.nn.grad.conv2d_input(shape, w64.abs(), dz.abs(), stride=2, padding=1)
    _check(got['dx'], nhwc(ref_dx), nhwc(mag_dx) * (4 * cout + 2) * U, f'conv3s2 dgrad {case}')
    M = dz.shape[0] * dz.shape[2] * dz.shape[3]
    wg = wgrad_ref(x64, dz, 3, stride=2)
    assert got['dw'].dtype == torch.float32 and got['db'].dtype == torch.float32
    _check(got['dw'], wg.dw, wg.mag_w * (M + 2) * U, f'conv3s2 wgrad {case}')
    _check(got['db'], wg.db, wg.mag_b * (M + 2) * U, f'conv3s2 bias grad {case}')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_conv3s2_two_runs_identical_bits(dtype):
    case = C3_RANDOM[3]  # two split-K blocks
    a, _ = _c3_random_run(case, dtype, True)
    b, _ = _c3_random_run(case, dtype, True)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_conv3s2_accumulates_into_flat_gradient_views():
    """With FlatParams the reduce adds onto the pre-filled gradient view: the same bits as write, then one fp32 add;
    a frozen weight gets nothing."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import edvr as E
    from basicsr4rs_amd.utils.flat import FlatParams
    g = gen_for('c3 flat')
    w, b = torch.randn(24, 16, 3, 3, generator=g) * 0.1, torch.randn(24, generator=g) * 0.1
    x = torch.randn(1, 32, 33, 16, generator=g)
    dy = torch.randn(1, 16, 17, 24, generator=g).cuda()
    plain = _conv(16, 24, w.double(), b.double())
    E.conv3s2(x.cuda(), plain, act=_lib.ACT_LRELU, slope=0.1).backward(dy)
    flat_conv = _conv(16, 24, w.double(), b.double())
    flat = FlatParams(flat_conv)
    pre = torch.randn(flat.grad.shape, generator=g).cuda()
    flat.grad.copy_(pre)
    E.conv3s2(x.cuda(), flat_conv, act=_lib.ACT_LRELU, slope=0.1).backward(dy)
    assert flat_conv.weight.grad.data_ptr() == flat_conv.weight._sr_grad_view.data_ptr()
    want = pre + torch.cat([plain.weight.grad.reshape(-1), plain.bias.grad.reshape(-1)])
    assert torch.equal(_bits(flat.grad), _bits(want))
    flat.grad.copy_(pre)
    flat_conv.weight.requires_grad = False
    E.conv3s2(x.cuda(), flat_conv, act=_lib.ACT_LRELU, slope=0.1).backward(dy)
    n = flat_conv.weight.numel()
    assert torch.equal(_bits(flat.grad[:n]), _bits(pre[:n])) and torch.equal(_bits(flat.grad[n:]), _bits(want[n:]))


def test_conv3s2_refusals():
    from basicsr4rs_amd.ops import edvr as E
    x = torch.zeros(1, 4, 4, 8, device='cuda')
    with pytest.raises(ValueError, match='3 x 3 conv with stride 2'):
        E.conv3s2(x, torch.nn.Conv2d(8, 8, 3, 1, 1).cuda())
    with pytest.raises(ValueError, match='at least 2'):
        E.conv3s2(torch.zeros(1, 1, 4, 8, device='cuda'), torch.nn.Conv2d(8, 8, 3, 2, 1).cuda())
    with pytest.raises(NotImplementedError):
        E.conv3s2(x.cpu(), torch.nn.Conv2d(8, 8, 3, 2, 1))


# ------------------------------------------------------------------------------------------------- pool3s2

P3_SHAPES = [(1, 4, 4), (1, 5, 7), (2, 8, 8)]
P3_CH = [8, 64]


def _pool_ref(x64, dy64=None):
    """float64 [max | avg] of an NHWC map through torch's CPU pools; with dy the gradient and the sum of the
    magnitudes of its terms (the same graph with |dy|: the gradient is linear in dy with non-negative weights)."""
    xl = nchw(x64).requires_grad_(dy64 is not None)
    y = R.pool3s2(xl)
    if dy64 is None:
        return nhwc(y.detach())
    dx, = torch.autograd.grad(y, xl, nchw(dy64), retain_graph=True)
    mag, = torch.autograd.grad(y, xl, nchw(dy64).abs())
    return nhwc(y.detach()), nhwc(dx), nhwc(mag)


def _same_or_both_nan(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _pool_bound(got, ref, mag, k):
    bound = k * U * mag
    if got.dtype == torch.bfloat16:
        bound = bound + 0.5 * _bf16_ulp(torch.maximum(ref.abs(), got.detach().double().cpu().abs()))
    return bound


def _pool_check(got, ref, mag, k, what):
    got64 = got.detach().double().cpu()
    bound = _pool_bound(got, ref, mag, k)
    err = (got64 - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f'{what} [{_ids(got.dtype)}]: max|err| {err.max().item():.3e}, max err/bound {ratio:.3f}')
    assert torch.isfinite(got64).all() and (err <= bound).all(), what


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('Cc', P3_CH)
@pytest.mark.parametrize('shape', P3_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool3s2_exact_grids(shape, Cc, dtype):
    """x = 9 * integers: every window sum is a multiple of 9, so both halves equal float64 bit for bit."""
    from basicsr4rs_amd.ops import edvr as E
    N, H, W = shape
    g = gen_for(f'pool grid {shape} {Cc}')
    x64 = grid((N, H, W, Cc), -3, 3, 9.0, gen=g)
    y = E.pool3s2(store(x64, dtype).cuda())
    assert y.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 2 * Cc) and y.dtype == dtype
    assert_bits(y, _pool_ref(x64), f'pool3s2 fwd {shape} {Cc}')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('Cc', P3_CH)
@pytest.mark.parametrize('shape', P3_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool3s2_random(shape, Cc, dtype):
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import edvr as E
    N, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = gen_for(f'pool random {shape} {Cc}')
    x = torch.randn(N, H, W, Cc, generator=g).to(dtype)
    dy = torch.randn(N, Ho, Wo, 2 * Cc, generator=g).to(dtype)
    ref, ref_dx, mag_dx = _pool_ref(x.double(), dy.double())
    mag = nhwc(F.avg_pool2d(nchw(x.double().abs()), 3, 2, 1))
    xg = x.cuda().requires_grad_(True)
    y = E.pool3s2(xg)
    y.backward(dy.cuda())
    assert torch.equal(y[..., :Cc].double().cpu(), ref[..., :Cc]), 'the max half is a selection: bit for bit'
    _pool_check(y[..., Cc:], ref[..., Cc:], mag, 10, f'pool3s2 avg {shape} {Cc}')
    _pool_check(xg.grad, ref_dx, mag_dx, 10, f'pool3s2 bwd {shape} {Cc}')
    # all of dx written: the raw call into a NaN-filled buffer
    buf = torch.full((N, H, W, Cc), float('nan'), dtype=dtype, device='cuda')
    lib = _lib.load()
    _lib.check(lib.sr_pool3s2_bwd(_lib.dtype_code(dtype), _lib.ptr(xg.detach()), _lib.ptr(dy.cuda()), N, H, W, Cc,
                                  _lib.ptr(buf), _lib.stream()))
    assert torch.equal(_bits(buf), _bits(xg.grad))


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_pool3s2_ties_and_nan(dtype):
    """Equal maxima inside one window (the first in row-major order takes the gradient, and a window that reads the
    same pair later makes its own choice) and one NaN (it wins its windows and takes their gradient): forward against
    torch's CPU max_pool2d, backward against torch's CPU autograd in float64."""
    from basicsr4rs_amd.ops import edvr as E
    g = gen_for('pool ties')
    x64 = grid((1, 6, 7, 8), -3, 3, gen=g)
    x64[0, 1, 1, :] = 5.0
    x64[0, 1, 2, :] = 5.0   # tie inside window (1, 1) -- and inside window (1, 0), (0, 0), (0, 1)
    x64[0, 2, 2, :4] = 5.0  # a later equal maximum one row down
    x64[0, 4, 5, ::2] = float('nan')
    dy64 = grid((1, 3, 4, 16), -2, 2, gen=g)
    ref, ref_dx, mag_dx = _pool_ref(x64, dy64)
    xg = x64.to(dtype).cuda().requires_grad_(True)
    y = E.pool3s2(xg)
    y.backward(dy64.to(dtype).cuda())
    got = y.double().cpu()
    cpu_max = nhwc(F.max_pool2d(nchw(x64.to(dtype).float()), 3, 2, 1)).double()
    assert _same_or_both_nan(got[..., :8], cpu_max), 'max half differs from torch max_pool2d'
    assert torch.isnan(got[0, 2, 2:4, 0]).all() and not torch.isnan(got[0, 2, 2:4, 1]).any()
    # the average of a window with a NaN is NaN, as torch's; elsewhere the bound
    nanavg = torch.isnan(ref[..., 8:])
    assert torch.equal(torch.isnan(got[..., 8:]), nanavg)
    dx = xg.grad.double().cpu()
    assert not torch.isnan(dx).any() and not torch.isnan(ref_dx).any()
    bound = _pool_bound(xg.grad, ref_dx, mag_dx, 10)
    err = (dx - ref_dx).abs()
    print(f'pool3s2 ties bwd [{_ids(dtype)}]: max|err| {err.max().item():.3e}, max err/bound '
          f'{(err / bound.clamp(min=1e-300)).max().item():.3f}')
    assert (err <= bound).all()
    # the tie: all of window (0, 0)'s max gradient on (1, 1), none on (1, 2) from it
    only_max = dy64.clone()
    only_max[..., 8:] = 0
    _, tie_dx, _ = _pool_ref(x64, only_max)
    xg2 = x64.to(dtype).cuda().requires_grad_(True)
    E.pool3s2(xg2).backward(only_max.to(dtype).cuda())
    assert_bits(xg2.grad, tie_dx, 'pool3s2 max-gradient routing')


# ------------------------------------------------------------------------------------ tsa_corr, tsa_modulate

TSA_CASES = [(2, 3, 16), (2, 5, 64), (2, 5, 16), (2, 3, 64)]
TSA_HW = (4, 6)


def _tsa_chain(emb, ref, ali, d_out, dtype, stored=lambda t: t):
    emb, ref, ali, d_out = (stored(t.to(dtype)) for t in (emb, ref, ali, d_out))
    out, prob = R.tsa_corr(emb, ref, ali)
    out = stored(out)
    d_ali, d_emb, d_ref = R.tsa_corr_bwd(d_out, emb, ref, ali, prob)
    return dict(out=out, prob=prob, d_aligned=stored(d_ali), d_emb=stored(d_emb), d_emb_ref=stored(d_ref))


@functools.lru_cache(None)
def _tsa_case(B, T, Cc):
    g = gen_for(f'tsa {B} {T} {Cc}')
    H, W = TSA_HW
    s = (4.0 / Cc**0.5)**0.5  # corr = sum of C products of N(0, s^2) pairs: std 4, reaching both sigmoid tails
    emb = torch.randn(B * T, H, W, Cc, generator=g) * s
    ref = torch.randn(B, H, W, Cc, generator=g) * s
    ali = torch.randn(B * T, H, W, Cc, generator=g)
    d_out = torch.randn(B, H, W, T * Cc, generator=g)
    runs = {'f64': _tsa_chain(emb, ref, ali, d_out, torch.float64), 'f32': _tsa_chain(emb, ref, ali, d_out, torch.float32),
            'emu': _tsa_chain(emb, ref, ali, d_out, torch.float64, _rne_bf16)}
    corr = (R._frames(emb.double(), B) * ref.double()[:, None]).sum(-1)
    assert corr.min() < -6 and corr.max() > 6
    f64 = runs['f64']
    bounds = {k: {torch.float32: 8 * _l2(runs['f32'][k], f64[k]), torch.bfloat16: 2 * _l2(runs['emu'][k], f64[k])}
              for k in f64}
    return (emb, ref, ali, d_out), f64, bounds


def _compare(got, ref, bounds, dtype, what):
    bad = []
    for k in ref:
        err, bound = _l2(got[k].cpu().reshape(ref[k].shape), ref[k]), bounds[k][dtype]
        print(f'{what} [{_ids(dtype)}] {k}: rel-L2 {err:.3e}, bound {bound:.3e}, ratio {err / max(bound, 1e-300):.3f}')
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


def _tsa_device(inputs, dtype):
    from basicsr4rs_amd.ops import edvr as E
    emb, ref, ali, d_out = (t.to(dtype).cuda() for t in inputs)
    emb.requires_grad_(True), ref.requires_grad_(True), ali.requires_grad_(True)
    out, prob = E.tsa_corr(emb, ref, ali)
    assert out.dtype == dtype and prob.dtype == torch.float32 and not prob.requires_grad
    out.backward(d_out)
    return dict(out=out.detach(), prob=prob, d_aligned=ali.grad, d_emb=emb.grad, d_emb_ref=ref.grad)


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('case', TSA_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_tsa_corr(case, dtype):
    inputs, ref, bounds = _tsa_case(*case)
    got = _tsa_device(inputs, dtype)
    B, T, Cc = case
    assert got['out'].shape == (B, *TSA_HW, T * Cc) and got['prob'].shape == (B, T, *TSA_HW)
    _compare(got, ref, bounds, dtype, f'tsa_corr {case}')
    again = _tsa_device(inputs, dtype)
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(again[k])), (k, 'two runs differ')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_tsa_corr_channel_order(dtype):
    """Frame t of ``aligned`` is the constant t + 1 and the embeddings are zero (prob 1 / 2): channel t * C + c of the
    output is (t + 1) / 2, exactly."""
    from basicsr4rs_amd.ops import edvr as E
    B, T, Cc, (H, W) = 2, 5, 16, TSA_HW
    ali = (torch.arange(T) + 1.0).repeat(B).view(B * T, 1, 1, 1).expand(B * T, H, W, Cc).contiguous()
    ali = ali + 8 * torch.arange(B).repeat_interleave(T).view(B * T, 1, 1, 1)
    zeros = torch.zeros(B * T, H, W, Cc)
    out, prob = E.tsa_corr(zeros.to(dtype).cuda(), zeros[:B].to(dtype).cuda(), ali.to(dtype).cuda())
    assert torch.equal(prob.cpu(), torch.full((B, T, H, W), 0.5))
    want = ((torch.arange(T) + 1.0).repeat_interleave(Cc).view(1, 1, 1, T * Cc) + 8 * torch.arange(B).view(B, 1, 1, 1)) / 2
    assert torch.equal(out.float().cpu(), want.expand(B, H, W, T * Cc))


def _mod_chain(feat, attn, add, dy, dtype, stored=lambda t: t):
    feat, attn, add, dy = (stored(t.to(dtype)) for t in (feat, attn, add, dy))
    y = stored(R.tsa_modulate(feat, attn, add))
    d_feat, d_attn, d_add = R.tsa_modulate_bwd(dy, feat, attn)
    return dict(y=y, d_feat=stored(d_feat), d_attn=stored(d_attn), d_attn_add=stored(d_add))


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', [(2, 4, 6, 16), (1, 5, 3, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_tsa_modulate(shape, dtype):
    from basicsr4rs_amd.ops import edvr as E
    g = gen_for(f'tsa mod {shape}')
    feat, add, dy = (torch.randn(shape, generator=g) for _ in range(3))
    attn = torch.randn(shape, generator=g) * 4  # both sigmoid tails
    f64 = _mod_chain(feat, attn, add, dy, torch.float64)
    f32 = _mod_chain(feat, attn, add, dy, torch.float32)
    emu = _mod_chain(feat, attn, add, dy, torch.float64, _rne_bf16)
    bounds = {k: {torch.float32: 8 * _l2(f32[k], f64[k]), torch.bfloat16: 2 * _l2(emu[k], f64[k])} for k in f64}
    # d_attn_add is dy itself: exact in fp32, one rounding of the operand in bf16
    bounds['d_attn_add'][torch.float32] = 0.0
    a, b, c = (t.to(dtype).cuda().requires_grad_(True) for t in (feat, attn, add))
    y = E.tsa_modulate(a, b, c)
    y.backward(dy.to(dtype).cuda())
    _compare(dict(y=y.detach(), d_feat=a.grad, d_attn=b.grad, d_attn_add=c.grad), f64, bounds, dtype, f'tsa_modulate {shape}')


# ------------------------------------------------------------------------------------------ scaled bilinear


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', [(1, 3, 5, 8), (2, 7, 6, 40)], ids=lambda s: 'x'.join(map(str, s)))
def test_bilinear_up2_scaled_is_twice_the_unscaled(shape, dtype):
    """A power-of-two scale commutes with every rounding: forward and backward equal the unscaled result times 2 bit
    for bit, and scale 1 is the unscaled call."""
    from basicsr4rs_amd.ops import gan as G_
    g = gen_for(f'up2 scaled {shape}')
    N, H, W, Cc = shape
    x = torch.randn(shape, generator=g).to(dtype).cuda()
    dy = torch.randn(N, 2 * H, 2 * W, Cc, generator=g).to(dtype).cuda()
    res = []
    for scale in (None, 1.0, 2.0):
        xx = x.clone().requires_grad_(True)
        y = G_.bilinear_up2(xx) if scale is None else G_.bilinear_up2(xx, scale)
        y.backward(dy)
        res.append((y.detach(), xx.grad))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(res[0], res[2]):
        assert torch.equal(_bits(a * 2), _bits(b))
