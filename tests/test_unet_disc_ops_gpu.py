"""The kernels behind UNetDiscriminatorSN (ops/gan.py: grouped spectral norm, bilinear x2, the 4x4 stride-2 conv with a
LeakyReLU) against float64 computed on the CPU by the formulas of tests/_unet_ref.py (checked against torch by
tests/test_unet_disc_host.py), never against the code under test.

Bounds.  Spectral norm: u, v, W and dweight_orig as vectors by relative L2, within 8 x the error of the same formulas
run in fp32 on the CPU (the suite's convention); the scalar sigma within 8 x max(that fp32 error, 2^-24 |sigma|): a
scalar's fp32 replay can land within a fraction of an ulp by luck, and a dropped row or column still moves sigma by
about 1 / K >= 2e-4.  Bilinear: bit for bit on integer grids; on random inputs (4 + 2) U sum|w x| per element (U =
2^-24), bf16 plus half a bf16 ulp of the result.  conv4s2: the existing (K + 2) U sum|x w| bound plus one bf16 ulp
(LeakyReLU is 1-Lipschitz); bf16 references from operands as the engine holds them (weights and the activation
backward's output rounded to bf16).  Every measured error is printed beside its bound."""
import functools

import pytest
import torch
from torch.nn import functional as F

from . import _unet_ref as R
from ._exact import assert_bits, gen_for, grid, store
from ._fp64 import U, _bf16_ulp, _bits, _check, _ids, _rne_bf16

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]

# ------------------------------------------------------------------------------------------- spectral norm

SN_PROBLEMS = [(8, 72), (16, 128), (24, 216), (64, 512), (256, 4608), (512, 4096)]


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _chain(M, u, v, G, dtype):
    """Training forward, backward with G, then an eval forward from the updated vectors, all in ``dtype``."""
    M, u, v, G = M.to(dtype), u.to(dtype), v.to(dtype), G.to(dtype)
    u1, v1, sigma, W = R.power_iteration(M, u, v)
    dw = R.sn_backward(G, W, u1, v1, sigma)
    _, _, sigma_e, W_e = R.power_iteration(M, u1, v1, iterate=False)
    return dict(u=u1, v=v1, sigma=sigma.reshape(1), W=W, dw=dw, sigma_e=sigma_e.reshape(1), W_e=W_e)


@functools.lru_cache(None)
def _sn_case(Rr, K):
    """fp32 inputs, the float64 results and the bounds from the fp32 CPU replay; computed once and shared."""
    g = gen_for(f'sn {Rr} {K}')
    M = torch.randn(Rr, K, generator=g) * (2.0 / (1.04 * K))**0.5
    u, v = F.normalize(torch.randn(Rr, generator=g), dim=0), F.normalize(torch.randn(K, generator=g), dim=0)
    G = torch.randn(Rr, K, generator=g)
    ref, f32 = _chain(M, u, v, G, torch.float64), _chain(M, u, v, G, torch.float32)
    bounds = {k: 8 * _l2(f32[k], ref[k]) for k in ref}
    for k in ('sigma', 'sigma_e'):  # a scalar: absolute, with the 2^-24 |sigma| floor
        bounds[k] = 8 * max((f32[k].double() - ref[k]).abs().item(), U * ref[k].abs().item())
    return M, u, v, G, ref, bounds


def _sn_device(cases, training=True, bufs=None, grads=True):
    """One grouped call over ``cases`` on the device (+ its backward): per problem a dict like _chain's."""
    from basicsr4rs_amd.ops import gan as G_
    ws = [c[0].cuda() for c in cases]
    bufs = bufs or [(c[1].cuda(), c[2].cuda()) for c in cases]
    outs, state, layout = G_.spectral_norm_fwd_raw(ws, bufs, training)
    res = []
    dws = [torch.full_like(w, float('nan')) for w in ws]
    if grads:
        G_.spectral_norm_bwd_raw(state, layout, [c[3].cuda() for c in cases], dws, False)
    for i, (w, (u, v)) in enumerate(zip(ws, bufs)):
        W, uf, vf, sig = G_.sn_state(state, layout, i)
        assert outs[i].data_ptr() == W.data_ptr() and outs[i].shape == w.shape
        res.append(dict(u=u, v=v, u_fwd=uf, v_fwd=vf, sigma=sig, W=W, dw=dws[i]))
    return res, state, layout, bufs


def _sn_compare(got, ref, bounds, keys, what):
    bad = []
    for k, rk in keys:
        if rk.startswith('sigma'):
            err = (got[k].double().cpu() - ref[rk]).abs().item()
        else:
            err = _l2(got[k].cpu().reshape(ref[rk].shape), ref[rk])
        print(f'{what} {k}: error {err:.3e}, bound {bounds[rk]:.3e}, ratio {err / max(bounds[rk], 1e-300):.3f}')
        if not err <= bounds[rk]:
            bad.append((k, err, bounds[rk]))
    assert not bad, bad


TRAIN_KEYS = [('u', 'u'), ('v', 'v'), ('u_fwd', 'u'), ('v_fwd', 'v'), ('sigma', 'sigma'), ('W', 'W'), ('dw', 'dw')]


@functools.lru_cache(None)
def _sn_singles():
    return [_sn_device([_sn_case(*p)])[0][0] for p in SN_PROBLEMS]


@pytest.mark.parametrize('prob', SN_PROBLEMS, ids=lambda p: 'x'.join(map(str, p)))
def test_spectral_norm_single_problem(prob):
    _, _, _, _, ref, bounds = _sn_case(*prob)
    _sn_compare(_sn_singles()[SN_PROBLEMS.index(prob)], ref, bounds, TRAIN_KEYS, f'sn {prob}')


def test_spectral_norm_grouped_equals_singles_and_repeats():
    cases = [_sn_case(*p) for p in SN_PROBLEMS]
    runs = [_sn_device(cases)[0] for _ in range(2)]
    for p, single, a, b in zip(SN_PROBLEMS, _sn_singles(), *runs):
        for k in single:
            assert torch.equal(_bits(a[k]), _bits(single[k])), (p, k, 'grouped differs from the single call')
            assert torch.equal(_bits(a[k]), _bits(b[k])), (p, k, 'two runs differ')


def test_spectral_norm_eval_leaves_buffers():
    """Eval: u, v bit-unchanged; sigma and W from the stored vectors (here the float64 result's first iterate)."""
    cases = [_sn_case(*p) for p in SN_PROBLEMS]
    bufs = [(c[4]['u'].float().cuda(), c[4]['v'].float().cuda()) for c in cases]
    before = [(u.clone(), v.clone()) for u, v in bufs]
    res, _, _, _ = _sn_device(cases, training=False, bufs=bufs, grads=False)
    for p, c, got, (u0, v0) in zip(SN_PROBLEMS, cases, res, before):
        assert torch.equal(_bits(got['u']), _bits(u0)) and torch.equal(_bits(got['v']), _bits(v0)), p
        assert torch.equal(_bits(got['u_fwd']), _bits(u0)) and torch.equal(_bits(got['v_fwd']), _bits(v0)), p
        _sn_compare(got, c[4], c[5], [('sigma', 'sigma_e'), ('W', 'W_e')], f'sn eval {p}')


def test_spectral_norm_backward_accumulates_and_skips():
    """acc = 1 adds onto a prefilled gradient (one more fp32 rounding: 2^-24 of the sum); a null G leaves its target
    untouched and a call without any G launches nothing."""
    from basicsr4rs_amd.ops import gan as G_
    cases = [_sn_case(*p) for p in SN_PROBLEMS[:4]]
    _, state, layout, _ = _sn_device(cases, grads=False)
    g = gen_for('sn prefill')
    pre = [torch.randn(c[0].shape, generator=g) for c in cases]
    targets = [p.cuda() for p in pre]
    gs = [c[3].cuda() if i != 1 else None for i, c in enumerate(cases)]
    G_.spectral_norm_bwd_raw(state, layout, gs, targets, True)
    for i, (c, p, t) in enumerate(zip(cases, pre, targets)):
        if i == 1:
            assert torch.equal(_bits(t.cpu()), _bits(p)), 'a problem without G was written'
            continue
        want = p.double() + c[4]['dw']
        err = (t.double().cpu() - want).norm().item()
        bound = c[5]['dw'] * c[4]['dw'].norm().item() + U * want.norm().item()
        print(f'sn acc {SN_PROBLEMS[i]}: |err| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}')
        assert err <= bound
    G_.spectral_norm_bwd_raw(state, layout, [None] * 4, targets, True)


def test_spectral_norm_group_autograd_into_flat_gradients():
    """spectral_norm_group on modules: the FlatParams gradient views receive the accumulated gradient, a frozen
    weight_orig gets nothing, and with everything frozen no backward kernel is launched."""
    from basicsr4rs_amd.ops import gan as G_
    from basicsr4rs_amd.utils import ktrace
    from basicsr4rs_amd.utils.flat import FlatParams
    net = R.he_init_sn(R.StockUNetSN(3, 8), seed=5).cuda()
    convs = [net.conv1, net.conv4]
    flat = FlatParams(net)
    net.conv4.weight_orig.requires_grad = False
    gw = [torch.randn_like(m.weight_orig) for m in convs]
    u0 = net.conv1.weight_u.clone()
    args = (net.conv1.weight_orig.detach().cpu().reshape(16, -1), u0.cpu(), net.conv1.weight_v.cpu(),
            gw[0].cpu().reshape(16, -1))
    ref, f32 = _chain(*args, torch.float64), _chain(*args, torch.float32)
    ws = G_.spectral_norm_group(convs, True)
    assert ws[0].requires_grad and not ws[1].requires_grad and not torch.equal(net.conv1.weight_u, u0)
    for _ in range(2):  # accumulated twice
        torch.autograd.backward([ws[0]], [gw[0]], retain_graph=True)
    view = net.conv1.weight_orig.grad
    assert view.data_ptr() == net.conv1.weight_orig._sr_grad_view.data_ptr()
    err, bound = _l2(view.cpu().reshape(16, -1), 2 * ref['dw']), 8 * _l2(f32['dw'], ref['dw']) + U
    print(f'sn group flat gradient: rel-L2 {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    idx = next(i for i, p in enumerate(flat.params) if p is net.conv1.weight_orig)
    assert not flat.grad[:flat.offsets[idx]].any() and not flat.grad[flat.offsets[idx + 1]:].any()
    for p in net.parameters():
        p.requires_grad = False
    ktrace.start()
    try:
        ws = G_.spectral_norm_group(convs, True)
    finally:
        rec = ktrace.stop()
    assert 'spectral_norm_fwd_kernels' in rec and not any(w.requires_grad for w in ws)


# ------------------------------------------------------------------------------------------------ bilinear

UP_SHAPES = [(1, 1, 1, 8), (1, 1, 5, 8), (2, 2, 1, 24), (1, 3, 5, 8), (2, 7, 6, 40), (2, 64, 64, 64)]


def _up_run(x):
    from basicsr4rs_amd.ops import gan as G_
    xx = x.cuda().requires_grad_(True)
    y = G_.bilinear_up2(xx)
    N, H, W, Cc = x.shape
    assert y.shape == (N, 2 * H, 2 * W, Cc) and y.dtype == x.dtype
    return xx, y


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', UP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bilinear_up2_exact_grids(shape, dtype):
    """Integer grids, |x| <= 8 and |dy| <= 2: forward and backward equal float64 bit for bit."""
    g = gen_for(f'up2 grid {shape}')
    N, H, W, Cc = shape
    x64, dy64 = grid(shape, -8, 8, gen=g), grid((N, 2 * H, 2 * W, Cc), -2, 2, gen=g)
    xx, y = _up_run(store(x64, dtype))
    y.backward(store(dy64, dtype).cuda())
    assert_bits(y, R.up2(x64, (1, 2)), f'bilinear_up2 fwd {shape}')
    assert_bits(xx.grad, R.up2_t(dy64, (1, 2)), f'bilinear_up2 bwd {shape}')


def _up_check(got, ref, mag, what):
    got64 = got.detach().double().cpu()
    bound = 6 * U * mag
    if got.dtype == torch.bfloat16:
        bound = bound + 0.5 * _bf16_ulp(torch.maximum(ref.abs(), got64.abs()))
    err = (got64 - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f'{what} [{_ids(got.dtype)}]: max|err| {err.max().item():.3e}, max err/bound {ratio:.3f}')
    assert torch.isfinite(got64).all() and (err <= bound).all(), what


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', UP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bilinear_up2_random(shape, dtype):
    g = gen_for(f'up2 random {shape}')
    N, H, W, Cc = shape
    x = torch.randn(shape, generator=g).to(dtype)
    dy = torch.randn(N, 2 * H, 2 * W, Cc, generator=g).to(dtype)
    xx, y = _up_run(x)
    y.backward(dy.cuda())
    _up_check(y, R.up2(x.double(), (1, 2)), R.up2(x.double().abs(), (1, 2)), f'bilinear_up2 fwd {shape}')
    _up_check(xx.grad, R.up2_t(dy.double(), (1, 2)), R.up2_t(dy.double().abs(), (1, 2)), f'bilinear_up2 bwd {shape}')


def test_bilinear_up2_refusals():
    from basicsr4rs_amd.ops import gan as G_
    with pytest.raises(ValueError, match='multiple of 8'):
        G_.bilinear_up2(torch.zeros(1, 2, 2, 12, device='cuda'))
    with pytest.raises(TypeError):
        G_.bilinear_up2(torch.zeros(1, 2, 2, 8, device='cuda', dtype=torch.float16))


# ---------------------------------------------------------------------------------- conv4s2 + LeakyReLU

C4_CASES = [(8, 16, 4, 4, 1), (16, 32, 8, 6, 2), (64, 128, 16, 16, 2)]
SLOPE = 0.2


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def _nhwc(t64):
    return t64.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('override', [False, True], ids=['cached', 'override'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('case', C4_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv4s2_lrelu(case, dtype, override):
    """y = leaky_relu(conv) and both gradients through the activation.  ``override``: the weight passed as a plain
    tensor (per-call images), its gradient returned through autograd.  The gate comes from the float64 conv; where
    an output lies within the forward bound of zero a gate may legitimately flip, so dy is zero there."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G_
    Cin, Cout, H, W, N = case
    g = gen_for(f'c4 act {case}')
    conv = torch.nn.Conv2d(Cin, Cout, 4, 2, 1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (16 * Cin))**0.5)
    x = torch.randn(N, H, W, Cin, generator=g).to(dtype).cuda().requires_grad_(True)
    w64 = conv.weight.detach().double().cpu()
    if dtype == torch.bfloat16:
        w64 = _rne_bf16(w64)
    x64 = _nchw64(x)
    z = F.conv2d(x64, w64, stride=2, padding=1)
    fb = F.conv2d(x64.abs(), w64.abs(), stride=2, padding=1) * (16 * Cin + 2) * U
    dy = torch.randn(N, H // 2, W // 2, Cout, generator=g) * _nhwc((z.abs() > fb).float())
    assert (dy != 0).float().mean() > 0.9
    dy = dy.to(dtype).cuda()
    wt = conv.weight.detach().clone().requires_grad_(True) if override else None
    y = G_.conv4s2(x, conv, act=_lib.ACT_LRELU, slope=SLOPE, weight=wt)
    y.backward(dy)
    dw = wt.grad if override else conv.weight.grad
    dy64 = _nchw64(dy)
    slope = float(torch.tensor(SLOPE, dtype=torch.float32))
    _check(y, _nhwc(torch.where(z > 0, z, z * slope)), _nhwc(fb), f'conv4s2+lrelu fwd {case}')
    # the activation backward's output as the engine holds it: fp32 product, then the storage dtype
    dz = torch.where(z > 0, dy64, (dy64 * slope).float().double())
    if dtype == torch.bfloat16:
        dz = _rne_bf16(dz)
    ref_dx = F.conv_transpose2d(dz, w64, stride=2, padding=1)
    mag_dx = F.conv_transpose2d(dz.abs(), w64.abs(), stride=2, padding=1)
    _check(x.grad, _nhwc(ref_dx), _nhwc(mag_dx) * (4 * Cout + 2) * U, f'conv4s2+lrelu dgrad {case}')
    ref_dw = torch.nn.grad.conv2d_weight(x64, w64.shape, dz, stride=2, padding=1)
    mag_dw = torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, dz.abs(), stride=2, padding=1)
    assert dw.dtype == torch.float32
    _check(dw, ref_dw, mag_dw * (N * (H // 2) * (W // 2) + 2) * U, f'conv4s2+lrelu wgrad {case}')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_conv4s2_act_none_keeps_the_bits(dtype):
    """ACT_NONE through the new entry point, the default call and the weight override give the same bits; with a
    LeakyReLU of slope 1 / 4 on an integer grid the result equals float64 bit for bit."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G_
    g = gen_for('c4 none')
    conv = torch.nn.Conv2d(16, 32, 4, 2, 1, bias=False).cuda()
    w64 = grid(conv.weight.shape, -3, 3, 0.25, gen=g)
    with torch.no_grad():
        conv.weight.copy_(w64.float())
    x64 = grid((2, 8, 6, 16), -3, 3, gen=g)
    x = store(x64, dtype).cuda()
    y0 = G_.conv4s2(x, conv)
    wf, _ = G_.conv4s2_images(conv.weight, dtype)
    y1 = G_.conv4s2_fwd_raw(x, wf, 32, _lib.ACT_NONE)
    y2 = torch.empty_like(y0)
    lib = _lib.load()
    _lib.check(lib.sr_conv4s2_fwd_act(_lib.dtype_code(dtype), _lib.ptr(x), _lib.ptr(wf), 2, 8, 6, 16, 32, 0, 0.0, _lib.ptr(y2),
                                      _lib.stream()))
    y3 = G_.conv4s2(x, conv, weight=conv.weight.detach().clone())
    for other in (y1, y2, y3):
        assert torch.equal(_bits(y0), _bits(other))
    z = F.conv2d(x64.permute(0, 3, 1, 2), w64, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
    assert_bits(y0, z, 'conv4s2 grid')
    ya = G_.conv4s2(x, conv, act=_lib.ACT_LRELU, slope=0.25)
    assert_bits(ya, torch.where(z > 0, z, z * 0.25), 'conv4s2+lrelu grid')
