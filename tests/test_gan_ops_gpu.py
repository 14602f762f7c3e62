"""The GAN ops of ops/gan.py against float64 computed on the CPU by plain torch (F.conv2d, F.batch_norm,
the formulas of basicsr/losses/gan_loss.py), never against the code under test.

Conventions (tests/_fp64.py, test_eltwise_gpu.py): U = 2^-24; a sum of K fp32 products in any order is within
(K + 2) U sum|terms| of the exact value; a bf16 result adds one bf16 ulp (``_check``); the bf16 references are
computed from operands already rounded to bf16 (feature maps are created in bf16, weights rounded with
``_rne_bf16``, as the prepared GEMM image rounds them)."""
import itertools

import pytest
import torch
from torch.nn import functional as F

from ._fp64 import U, _check, _ids, _rne_bf16

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def _nhwc(t64):
    return t64.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------- conv4s2

CONV_CASES = [(2, 8, 16, 2, 2), (2, 64, 64, 8, 8), (1, 16, 8, 6, 10), (3, 24, 40, 36, 20), (1, 512, 512, 8, 8)]


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv4s2_fwd_dgrad_wgrad(case, dtype):
    """Bounds: forward (K + 2) U sum|x w| with K = 16 Cin; dgrad the same over the 4 Cout products an input pixel
    receives (2 taps per axis for its parity class); wgrad with K = N Ho Wo.  The magnitude sums are the same
    convolutions of |x|, |w|, |dy|.  bf16: x and dy are bf16 tensors, w is rounded to bf16 in the reference; y and
    dx are bf16 (one ulp more), dw is fp32."""
    from basicsr4rs_amd.ops import gan as G
    N, Cin, Cout, H, W = case
    torch.manual_seed(sum(case))
    conv = torch.nn.Conv2d(Cin, Cout, 4, 2, 1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * (2.0 / (16 * Cin))**0.5)
    x = torch.randn(N, H, W, Cin, device='cuda').to(dtype).requires_grad_(True)
    dy = torch.randn(N, H // 2, W // 2, Cout, device='cuda').to(dtype)
    y = G.conv4s2(x, conv)
    assert y.shape == (N, H // 2, W // 2, Cout) and y.dtype == dtype
    y.backward(dy)
    w64 = conv.weight.detach().double().cpu()
    if dtype == torch.bfloat16:
        w64 = _rne_bf16(w64)
    x64, dy64 = _nchw64(x), _nchw64(dy)
    ref_y = F.conv2d(x64, w64, stride=2, padding=1)
    mag_y = F.conv2d(x64.abs(), w64.abs(), stride=2, padding=1)
    _check(y, _nhwc(ref_y), _nhwc(mag_y) * (16 * Cin + 2) * U, f'conv4s2 fwd {case}')
    ref_dx = F.conv_transpose2d(dy64, w64, stride=2, padding=1)
    mag_dx = F.conv_transpose2d(dy64.abs(), w64.abs(), stride=2, padding=1)
    assert ref_dx.shape == x64.shape
    _check(x.grad, _nhwc(ref_dx), _nhwc(mag_dx) * (4 * Cout + 2) * U, f'conv4s2 dgrad {case}')
    ref_dw = torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, stride=2, padding=1)
    mag_dw = torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, dy64.abs(), stride=2, padding=1)
    K = N * (H // 2) * (W // 2)
    assert conv.weight.grad.dtype == torch.float32
    _check(conv.weight.grad, ref_dw, mag_dw * (K + 2) * U, f'conv4s2 wgrad {case}')


def test_conv4s2_split_k_runs_and_repeats():
    """The ragged case spreads its N Ho Wo = 540 rows over more than one split-K block; two runs give the same bits."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G
    assert _lib.load().sr_conv4s2_wgrad_splits(3, 36, 20, 24, 40) > 1
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(24, 40, 4, 2, 1, bias=False).cuda()
    x0 = torch.randn(3, 36, 20, 24, device='cuda')
    outs = []
    for _ in range(2):
        conv.weight.grad = None
        x = x0.clone().requires_grad_(True)
        y = G.conv4s2(x, conv)
        y.backward(torch.ones_like(y) * 0.5)
        outs.append((y.detach().clone(), x.grad.clone(), conv.weight.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_conv4s2_refusals_and_frozen_weight():
    from basicsr4rs_amd.ops import gan as G
    from basicsr4rs_amd.utils import ktrace
    conv = torch.nn.Conv2d(8, 8, 4, 2, 1, bias=False).cuda()
    with pytest.raises(ValueError, match=r'\(1, 3, 4, 8\)'):
        G.conv4s2(torch.zeros(1, 3, 4, 8, device='cuda'), conv)
    with pytest.raises(ValueError, match=r'\(1, 4, 4, 16\)'):
        G.conv4s2(torch.zeros(1, 4, 4, 16, device='cuda'), conv)
    with pytest.raises(NotImplementedError):
        G.conv4s2(torch.zeros(1, 4, 4, 8), torch.nn.Conv2d(8, 8, 4, 2, 1, bias=False))
    with pytest.raises(ValueError, match='4 x 4 conv'):
        G.conv4s2(torch.zeros(1, 4, 4, 8, device='cuda'), torch.nn.Conv2d(8, 8, 3, 1, 1, bias=False).cuda())
    x = torch.randn(2, 8, 8, 8, device='cuda', requires_grad=True)
    for frozen in (False, True):
        conv.weight.requires_grad_(not frozen)
        conv.weight.grad = None
        x.grad = None
        ktrace.start()
        try:
            G.conv4s2(x, conv).sum().backward()
        finally:
            rec = ktrace.stop()
        assert 'conv4s2_fwd_kernel' in rec and 'conv4s2_dgrad_kernel' in rec, sorted(rec)
        assert any('wgrad' in k for k in rec) == (not frozen), sorted(rec)
        assert (conv.weight.grad is None) == frozen
        if frozen:
            dx_frozen = x.grad.clone()
        else:
            dx_live = x.grad.clone()
    assert torch.equal(dx_live, dx_frozen)


def test_conv4s2_images_follow_the_weight():
    """The cached GEMM images are rebuilt after an in-place weight update (``_version``) and after a parameter
    epoch bump (an optimizer that writes the flat buffer behind autograd's back)."""
    from basicsr4rs_amd.ops import conv as C
    from basicsr4rs_amd.ops import gan as G
    torch.manual_seed(1)
    conv = torch.nn.Conv2d(8, 8, 4, 2, 1, bias=False).cuda()
    x = torch.randn(1, 4, 4, 8, device='cuda')
    y0 = G.conv4s2(x, conv)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    y1 = G.conv4s2(x, conv)
    assert torch.equal(y1, y0 * 2)
    conv.weight.data.mul_(2.0)  # no version bump
    C.bump_param_epoch()
    assert torch.equal(G.conv4s2(x, conv), y0 * 4)


# ---------------------------------------------------------------------------------------------- batch norm


def _bn_ref(x64, dy64, gamma, beta, mean, var, eps, M_sum, training, slope):
    """float64 forward / backward of act(bn(x)) on [M, C] rows with the statistics (mean, var) given, and the
    rounding bounds of an fp32 evaluation (module docstring of the test below)."""
    M = x64.shape[0]
    d = x64 - mean
    rstd = (var + eps).rsqrt()
    xh = d * rstd
    z = gamma * xh + beta
    gate = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    y = z * gate
    e_mean = (M_sum + 2) * U * x64.abs().mean(0) if training else torch.zeros_like(mean)
    delta = 2 * U * (x64.abs().amax(0) + mean.abs()) + e_mean
    e_var = 2 * d.abs().mean(0) * delta + (M_sum + 2) * U * var if training else torch.zeros_like(var)
    e_rstd = rstd * (0.5 * e_var / (var + eps) + 3 * U)
    e_xh = d.abs() * e_rstd + rstd * delta + 2 * U * xh.abs()
    e_y = gamma.abs() * e_xh + 3 * U * ((gamma * xh).abs() + beta.abs())
    r = dict(y=y, e_y=e_y, mean=mean, e_mean=e_mean, rstd=rstd, e_rstd=e_rstd, var=var, e_var=e_var)
    if dy64 is None:
        return r
    g = dy64 * gate
    # an element whose pre-activation is within its own error of zero may take the other branch
    e_g = torch.where(z.abs() <= e_y, (1 - slope) * dy64.abs(), torch.zeros_like(g))
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    e_dbeta = (M + 2) * U * g.abs().sum(0) + e_g.sum(0)
    e_dgamma = (M + 2) * U * (g * xh).abs().sum(0) + (g.abs() * e_xh + e_g * xh.abs()).sum(0)
    if training:
        dx = rstd * gamma * (g - dbeta / M - xh * dgamma / M)
        T = g.abs() + g.abs().mean(0) + xh.abs() * (g * xh).abs().mean(0)
        inner = e_g + e_dbeta / M + e_xh * (dgamma / M).abs() + xh.abs() * e_dgamma / M
        e_dx = gamma.abs() * (e_rstd * T + rstd * inner) + 8 * U * rstd * gamma.abs() * T
    else:
        dx = g * gamma * rstd
        e_dx = gamma.abs() * (e_rstd * g.abs() + rstd * e_g) + 4 * U * dx.abs()
    r.update(dx=dx, e_dx=e_dx, dgamma=dgamma, e_dgamma=e_dgamma, dbeta=dbeta, e_dbeta=e_dbeta)
    return r


def _make_bn(C, momentum, seed):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C, momentum=momentum).cuda()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(C))
        bn.bias.copy_(0.2 * torch.randn(C))
        bn.running_mean.copy_(0.1 * torch.randn(C))
        bn.running_var.copy_(1 + 0.2 * torch.rand(C))
    return bn


BN_CASES = [(2, 1, 1, 8), (2, 4, 4, 512), (3, 10, 6, 24), (2, 64, 64, 64)]
BN_VARIANTS = [('lrelu', 0.1, 0.0), ('none', 0.1, 0.0), ('lrelu', None, 0.0), ('lrelu', 0.1, 100.0)]
# (activation, momentum, offset of the per-channel mean) x dtype; the offset variant is an fp32 case: a bf16
# input (8 significant bits) cannot hold mean 100 with standard deviation 1
BN_PARAMS = [(v, dt) for v in BN_VARIANTS for dt in DTYPES if not (v[2] and dt == torch.bfloat16)]


@pytest.mark.parametrize('variant,dtype', BN_PARAMS, ids=lambda p: _ids(p) if isinstance(p, torch.dtype) else
                         f'{p[0]}-m{p[1]}-off{p[2]:g}')
@pytest.mark.parametrize('case', BN_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_batch_norm_act_training(case, variant, dtype):
    """Two training calls; everything of the second, and the running statistics after both, against float64.

    Bounds, per channel over M = N H W rows, for any order of an fp32 mean / variance accumulation that works on
    deviations (Welford, Chan, two-pass): mean within e_mean = (M + 2) U mean|x|; a deviation d = x - mean within
    delta = 2 U (max|x| + |mean|) + e_mean; the variance within e_var = 2 mean|d| delta + (M + 2) U var; rstd
    within rstd (e_var / (2 (var + eps)) + 3 U); xhat within |d| e_rstd + rstd delta + 2 U |xhat|; y within
    |gamma| e_xhat + 3 U (|gamma xhat| + |beta|).  Backward: the gate may differ where |z| <= e_y (then g is off
    by (1 - slope) |dy|); dbeta, dgamma are M-term sums ((M + 2) U sum|terms|) plus the propagated e_xhat and
    gate terms; dx collects the errors of its factors.  Running statistics: the error of the batch value times
    the momentum, plus 4 U of the magnitudes.  A variance from E[x^2] - E[x]^2 has an error of about
    U M^(1/2) mean^2 (5e-3 at mean 100, std 1, M = 180, from sums near 1.8e6 whose ulp is 0.125), above the
    e_var = 1.8e-3 the offset fp32 case allows there."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G
    N, H, W, C = case
    act_name, momentum, offset = variant
    act = _lib.ACT_LRELU if act_name == 'lrelu' else _lib.ACT_NONE
    slope = 0.2 if act_name == 'lrelu' else 1.0
    M = N * H * W
    bn = _make_bn(C, momentum, seed=M + C)
    rm = [bn.running_mean.double().cpu()]
    rv = [bn.running_var.double().cpu()]
    gamma, beta = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    e_rm = torch.zeros(C, dtype=torch.float64)
    e_rv = torch.zeros(C, dtype=torch.float64)
    for call in (1, 2):
        x = (torch.randn(N, H, W, C, device='cuda') * (1 + 0.5 * torch.rand(C, device='cuda')) + offset
             + 0.3 * torch.randn(C, device='cuda')).to(dtype).requires_grad_(True)
        dy = torch.randn(N, H, W, C, device='cuda').to(dtype)
        bn.weight.grad = bn.bias.grad = None
        y = G.batch_norm_act(x, bn, act, 0.2)
        y.backward(dy)
        x64, dy64 = x.detach().double().cpu().reshape(M, C), dy.double().cpu().reshape(M, C)
        mean, var = x64.mean(0), x64.var(0, unbiased=False)
        r = _bn_ref(x64, dy64, gamma, beta, mean, var, bn.eps, M, True, slope)
        f = momentum if momentum is not None else 1.0 / call
        rm.append((1 - f) * rm[-1] + f * mean)
        rv.append((1 - f) * rv[-1] + f * var * M / (M - 1))
        e_rm = (1 - f) * e_rm + f * r['e_mean'] + 4 * U * (rm[-2].abs() + mean.abs())
        e_rv = (1 - f) * e_rv + f * r['e_var'] * M / (M - 1) + 4 * U * (rv[-2].abs() + var * M / (M - 1))
    what = f'bn {case} {variant}'
    _check(y, r['y'].reshape(N, H, W, C), r['e_y'].reshape(N, H, W, C), what + ' y')
    _check(x.grad, r['dx'].reshape(N, H, W, C), r['e_dx'].reshape(N, H, W, C), what + ' dx')
    assert bn.weight.grad.dtype == torch.float32 and bn.bias.grad.dtype == torch.float32
    _check(bn.weight.grad, r['dgamma'], r['e_dgamma'], what + ' dgamma')
    _check(bn.bias.grad, r['dbeta'], r['e_dbeta'], what + ' dbeta')
    save_mean, save_rstd = G.bn_stats_raw(x.detach(), bn.eps)
    _check(save_mean, r['mean'], r['e_mean'] + U * r['mean'].abs(), what + ' save_mean')
    _check(save_rstd, r['rstd'], r['e_rstd'], what + ' save_rstd')
    _check(bn.running_mean, rm[-1], e_rm, what + ' running_mean')
    _check(bn.running_var, rv[-1], e_rv, what + ' running_var')
    assert bn.num_batches_tracked.item() == 2


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_batch_norm_act_eval(dtype):
    """Eval mode: xhat from the running statistics (exact inputs, so e_mean = e_var = 0 in the bounds above),
    dx = g gamma rstd, and the running buffers bit-unchanged."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G
    N, H, W, C = 3, 10, 6, 24
    M = N * H * W
    bn = _make_bn(C, 0.1, seed=5).eval()
    before = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    x = torch.randn(N, H, W, C, device='cuda').to(dtype).requires_grad_(True)
    dy = torch.randn(N, H, W, C, device='cuda').to(dtype)
    y = G.batch_norm_act(x, bn, _lib.ACT_LRELU, 0.2)
    y.backward(dy)
    r = _bn_ref(x.detach().double().cpu().reshape(M, C), dy.double().cpu().reshape(M, C), bn.weight.detach().double().cpu(),
                bn.bias.detach().double().cpu(), before[0].double().cpu(), before[1].double().cpu(), bn.eps, M, False, 0.2)
    _check(y, r['y'].reshape(N, H, W, C), r['e_y'].reshape(N, H, W, C), 'bn eval y')
    _check(x.grad, r['dx'].reshape(N, H, W, C), r['e_dx'].reshape(N, H, W, C), 'bn eval dx')
    _check(bn.weight.grad, r['dgamma'], r['e_dgamma'], 'bn eval dgamma')
    _check(bn.bias.grad, r['dbeta'], r['e_dbeta'], 'bn eval dbeta')
    for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)


def test_batch_norm_act_refusals_and_repeatability():
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G
    bn = _make_bn(8, 0.1, seed=1)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        G.batch_norm_act(torch.zeros(1, 1, 1, 8, device='cuda'), bn)
    bn.eval()
    assert G.batch_norm_act(torch.zeros(1, 1, 1, 8, device='cuda'), bn).shape == (1, 1, 1, 8)
    with pytest.raises(NotImplementedError):
        G.batch_norm_act(torch.zeros(2, 1, 1, 8), torch.nn.BatchNorm2d(8))
    with pytest.raises(NotImplementedError):
        G.batch_norm_act(torch.zeros(2, 1, 1, 8, device='cuda'), torch.nn.BatchNorm2d(8, affine=False).cuda())
    with pytest.raises(NotImplementedError):
        G.batch_norm_act(torch.zeros(2, 1, 1, 8, device='cuda'), torch.nn.BatchNorm2d(8, track_running_stats=False).cuda())
    with pytest.raises(ValueError, match=r'\(2, 2, 2, 16\)'):
        G.batch_norm_act(torch.zeros(2, 2, 2, 16, device='cuda'), bn)
    torch.manual_seed(2)
    x0 = torch.randn(2, 64, 64, 64, device='cuda')
    dy = torch.randn_like(x0)
    outs = []
    for _ in range(2):
        b = _make_bn(64, 0.1, seed=9)
        x = x0.clone().requires_grad_(True)
        y = G.batch_norm_act(x, b, _lib.ACT_LRELU, 0.2)
        y.backward(dy)
        outs.append((y.detach(), x.grad, b.weight.grad, b.bias.grad, b.running_mean, b.running_var))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ GAN loss

KINDS = ['vanilla', 'lsgan', 'wgan', 'wgan_softplus', 'hinge']


def _gan_terms64(kind, x, real, disc, rl, fl):
    """Per-element loss terms of basicsr/losses/gan_loss.py:89-109 in float64 (their mean is the loss), from the
    functions the reference calls, so that autograd gives their gradients (sigmoid(x) - t at x = 0 as well, where a
    restated max(x, 0) + log1p(exp(-|x|)) would differentiate to a subgradient).  F.softplus returns z above its
    threshold 20, 2e-9 from the exact value: 1e-10 relative, far below U."""
    if kind == 'hinge':
        return F.relu(1 + (-x if real else x)) if disc else -x
    if kind == 'wgan':
        return -x if real else x
    if kind == 'wgan_softplus':
        return F.softplus(-x if real else x)
    t = rl if real else fl
    if kind == 'vanilla':
        return F.binary_cross_entropy_with_logits(x, torch.full_like(x, t), reduction='none')
    return (x - t)**2


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('kind', KINDS)
def test_gan_loss_against_float64(kind, dtype):
    """A term is a handful of fp32 operations (at most 16 roundings, the library exp / log1p at a few ulp) on
    magnitudes up to m = 1 + |x| (1 + |t|) + x^2 [lsgan]: each term within 16 U m.  The kernel sums the n terms in
    fp32 ((n + 2) U sum|l|) and folds the block partials in double; the mean and the weight multiply in double and
    round once (U |loss|).  The gradient l'(x) w / n: within 16 U (1 + |x| + |t|) w / n, one bf16 ulp more in bf16.
    The vanilla reference is nn.BCEWithLogitsLoss in double as well, to pin the restated formula."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.losses import build_loss
    blk = _lib.load().sr_gan_loss_block(_lib.dtype_code(dtype))
    shapes = [(1, ), (16, 1), (blk - 1, ), (blk, ), (blk + 1, ), (2, 1, 61, 67)]
    rl, fl, lw = 0.9, 0.1, 5e-3
    cri = build_loss(dict(type='GANLoss', gan_type=kind, real_label_val=rl, fake_label_val=fl, loss_weight=lw)).cuda()
    torch.manual_seed(11)
    for shape, real, disc in itertools.product(shapes, (True, False), (True, False)):
        x = (torch.randn(shape, device='cuda') * 3)
        flat = x.view(-1)
        if flat.numel() >= 16:
            flat[:3] = torch.tensor([80.0, -80.0, 0.0], device='cuda')
        x = x.to(dtype).requires_grad_(True)
        loss = cri(x, real, is_disc=disc)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward()
        x64 = x.detach().double().cpu().requires_grad_(True)
        w = 1.0 if disc else lw
        terms = _gan_terms64(kind, x64, real, disc, rl, fl)
        ref = terms.mean() * w
        ref.backward()
        n = x64.numel()
        t = abs(rl if real else fl)
        m = 1 + x64.detach().abs() * (1 + t) + (x64.detach()**2 if kind == 'lsgan' else 0)
        bound = ((n + 2) * U * terms.detach().abs().sum() + 16 * U * m.sum()) / n * w + U * ref.detach().abs()
        what = f'gan_loss {kind} {shape} real={real} disc={disc}'
        _check(loss, ref.detach(), bound, what)
        _check(x.grad, x64.grad, 16 * U * (1 + x64.detach().abs() + t) * w / n, what + ' grad')
        if kind == 'vanilla':
            bce = torch.nn.BCEWithLogitsLoss()(x64.detach(), torch.full_like(x64.detach(), rl if real else fl)) * w
            assert abs(bce.item() - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
        # the same bits from a second run
        x2 = x.detach().clone().requires_grad_(True)
        loss2 = cri(x2, real, is_disc=disc)
        loss2.backward()
        assert torch.equal(loss, loss2) and torch.equal(x.grad, x2.grad)


def test_gan_loss_refusals():
    from basicsr4rs_amd.ops import gan as G
    with pytest.raises(NotImplementedError, match='GAN type nope is not implemented.'):
        G.gan_loss(torch.zeros(4, device='cuda'), 'nope', True)
    with pytest.raises(NotImplementedError):
        G.gan_loss(torch.zeros(4), 'vanilla', True)
    with pytest.raises(ValueError, match=r'\(0, 1\)'):
        G.gan_loss(torch.zeros(0, 1, device='cuda'), 'vanilla', True)


# -------------------------------------------------------------------------------------------- head linears


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('M', [1, 3])
def test_head_linears(M, dtype):
    """linear1 on a flattened NHWC map [M, 16 C] with the reference's NCHW-flatten weight, LeakyReLU fused, then
    linear2 (100 -> 1), against float64 on the NCHW flatten.  Every output is a K-term fp32 sum: (K + 2) U
    sum|terms|; x is exact in both dtypes and the weights stay fp32; the gradients with respect to the weights
    come back in the parameter's own order."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import gan as G
    C, P = 24, 16
    K = C * P
    torch.manual_seed(M)
    l1, l2 = torch.nn.Linear(K, 100).cuda(), torch.nn.Linear(100, 1).cuda()
    feat = torch.randn(M, 4, 4, C, device='cuda').to(dtype).requires_grad_(True)
    h = G.linear(feat.reshape(M, K), l1, _lib.ACT_LRELU, 0.2, spatial=P)
    out = G.linear(h, l2)
    assert out.shape == (M, 1) and out.dtype == torch.float32 and h.dtype == torch.float32
    dout = torch.randn(M, 1, device='cuda')
    out.backward(dout)
    f64 = feat.detach().double().cpu().permute(0, 3, 1, 2).reshape(M, K).requires_grad_(True)
    w1, b1 = l1.weight.detach().double().cpu().requires_grad_(True), l1.bias.detach().double().cpu().requires_grad_(True)
    w2, b2 = l2.weight.detach().double().cpu().requires_grad_(True), l2.bias.detach().double().cpu().requires_grad_(True)
    z = f64 @ w1.t() + b1
    h64 = F.leaky_relu(z, 0.2)
    o64 = h64 @ w2.t() + b2
    o64.backward(dout.double().cpu())
    e_h = (K + 2) * U * (f64.detach().abs() @ w1.detach().abs().t() + b1.detach().abs())
    _check(h, h64.detach(), e_h, 'linear1')
    e_o = (102) * U * (h64.detach().abs() @ w2.detach().abs().t() + b2.detach().abs()) + e_h @ w2.detach().abs().t()
    _check(out, o64.detach(), e_o, 'linear2')
    d64 = dout.double().cpu()
    _check(l2.weight.grad, w2.grad, (M + 2) * U * (d64.abs().t() @ h64.detach().abs()) + d64.abs().t() @ e_h, 'dw2')
    _check(l2.bias.grad, b2.grad, (M + 2) * U * d64.abs().sum(0), 'db2')
    # dh = dout w2 (one product), gated; away from the kink (|z| > e_h) the gate is the reference's
    dh = (d64 @ w2.detach()) * torch.where(z.detach() > 0, torch.ones_like(z), torch.full_like(z, 0.2)).detach()
    e_dh = 4 * U * dh.abs() + torch.where(z.detach().abs() <= e_h, 0.8 * (d64 @ w2.detach()).abs(), torch.zeros_like(dh))
    _check(l1.weight.grad, w1.grad, (M + 2) * U * (dh.abs().t() @ f64.detach().abs()) + e_dh.t() @ f64.detach().abs(), 'dw1')
    _check(l1.bias.grad, b1.grad, (M + 2) * U * dh.abs().sum(0) + e_dh.sum(0), 'db1')
    ref_dx = f64.grad.reshape(M, C, 4, 4).permute(0, 2, 3, 1)
    e_dx = ((102) * U * (dh.abs() @ w1.detach().abs()) + e_dh @ w1.detach().abs()).reshape(M, C, 4, 4).permute(0, 2, 3, 1)
    _check(feat.grad, ref_dx.contiguous(), e_dx.contiguous(), 'dfeat')
