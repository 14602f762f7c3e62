"""Perceptual loss on the GPU against float64: the max-pool and Gram kernels (csrc/perceptual.hip), the VGG
feature extractor, PerceptualLoss and the train step with ``train.perceptual_opt``.

References are plain torch on the CPU in float64 (F.conv2d, F.max_pool2d, bmm) on the same input bits.
Kernel bounds are derived (U = 2^-24, an fp32 rounding; tests/_fp64._check adds one bf16 ulp for bf16
outputs).  Network-level bounds are MEASURED against the float64 restatement, never against the device:
fp32 -- 8x the relative L2 error of the same restatement run in fp32 by torch on the CPU; bf16 -- 2x that
of the restatement with bf16-rounded weights and every stored activation and gradient map rounded to bf16
(float64 arithmetic).  Relative L2, not max-abs: a near-tie in a pooling window can flip between
precisions and moves whole gradient entries."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from basicsr4rs_amd import _lib
from basicsr4rs_amd.archs.vgg_arch import NAMES, conv_channels
from tests._fp64 import U, _bits, _check, _ids, _rne_bf16

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------------------------------
# 1. max-pool
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape,stride,quant,nan', [
    ((2, 7, 9, 64), 2, False, False),   # the floor drops a row and a column: their dx is 0
    ((1, 6, 6, 8), 1, False, False),    # overlapping windows sum
    ((1, 8, 8, 72), 2, True, False),    # 4 distinct values: most windows tie, the first maximum wins
    ((1, 8, 8, 72), 1, True, False),
    ((1, 6, 7, 16), 2, False, True),    # one NaN propagates
    ((1, 6, 7, 16), 1, False, True),
], ids=['floor_s2', 'overlap_s1', 'ties_s2', 'ties_s1', 'nan_s2', 'nan_s1'])
def test_max_pool2_is_bit_exact(cuda, dtype, shape, stride, quant, nan):
    from basicsr4rs_amd.ops import perceptual as P
    g = torch.Generator().manual_seed(sum(shape) + stride)
    if quant:
        x = torch.randint(0, 4, shape, generator=g).float() / 2 - 0.5
    else:
        x = torch.randn(shape, generator=g)
    x = x.to(dtype)
    if nan:
        x[0, 2, 3, 1] = float('nan')
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y64 = F.max_pool2d(x64, 2, stride)
    # multiples of 1/4 up to 2: sums of up to four are exact in bf16, whatever the order
    dy = torch.randint(-8, 9, y64.shape, generator=g).double() / 4
    y64.backward(dy)
    xd = x.to(cuda).requires_grad_(True)
    yd = P.max_pool2(xd, stride)
    assert yd.dtype == dtype and tuple(yd.shape) == (shape[0], y64.shape[2], y64.shape[3], shape[3])
    yd.backward(dy.permute(0, 2, 3, 1).to(dtype).to(cuda))
    y_ref, dx_ref = y64.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1)
    got_y, got_dx = yd.detach().double().cpu(), xd.grad.double().cpu()
    assert torch.equal(torch.isnan(got_y), torch.isnan(y_ref)) and torch.isnan(y_ref).any() == nan
    assert torch.equal(torch.nan_to_num(got_y, nan=12345.0), torch.nan_to_num(y_ref, nan=12345.0))
    assert torch.equal(got_dx, dx_ref)
    if stride == 2 and shape[1] % 2:
        assert not got_dx[:, -1].any() and not got_dx[:, :, -1].any()
    if stride == 1 and not nan:
        assert (got_dx.abs() > 2).any()  # some element did collect more than one window


# ---------------------------------------------------------------------------------------------------------
# 2. / 3. Gram forward and backward
# ---------------------------------------------------------------------------------------------------------
def _gram_hw(case):
    """(C, HW) of a named case.  SPLIT_MIN_HW: the smallest HW at which the kernel's split rule (GRAM_KBLOCK
    rows per K block, sr_gram_kblock()) uses two K blocks; SPLIT_UNEVEN_HW: three blocks, the last with 300
    rows, which is also a K tail (300 % 32 != 0).  ROWS_PER_BLOCK_HW (backward only): 515 row tiles of 64 per
    image, the smallest odd count at which two images pass the 512 tiles (GB_MIN_BLOCKS of the kernel source)
    above which a block of the C <= 64 backward takes two row tiles; the last block of an image takes one."""
    kb = _lib.load().sr_gram_kblock()
    SPLIT_MIN_HW, SPLIT_UNEVEN_HW = kb + 1, 2 * kb + 300
    ROWS_PER_BLOCK_HW = 64 * 514 + 7
    return {'k_tail': (64, 5 * 7), 'partial_tile': (136, 64), 'c512': (512, 4), 'split_min': (64, SPLIT_MIN_HW),
            'split_uneven': (64, SPLIT_UNEVEN_HW), 'rows_per_block': (64, ROWS_PER_BLOCK_HW)}[case]


GRAM_CASES = ['k_tail', 'partial_tile', 'c512', 'split_min', 'split_uneven']
SENTINEL = -7.25


def _gram_raw(f, scale, tail=64):
    """sr_gram_fwd on buffers with a sentinel-filled tail after G and after the workspace."""
    lib = _lib.load()
    N, HW, C = f.shape
    ws_bytes = lib.sr_gram_workspace(N, HW, C)
    gbuf = torch.full((N * C * C + tail, ), SENTINEL, device=f.device)
    wbuf = torch.full((ws_bytes // 4 + tail, ), SENTINEL, device=f.device)
    _lib.check(lib.sr_gram_fwd(_lib.dtype_code(f.dtype), _lib.ptr(f), N, HW, C, ctypes.c_float(scale), _lib.ptr(gbuf),
                               _lib.ptr(wbuf) if ws_bytes else None, ws_bytes, _lib.stream()))
    torch.cuda.synchronize()
    assert (gbuf[N * C * C:] == SENTINEL).all(), 'gram_fwd wrote past G'
    assert (wbuf[ws_bytes // 4:] == SENTINEL).all(), 'gram_fwd wrote past its workspace'
    return gbuf[:N * C * C].view(N, C, C).clone(), ws_bytes


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('case', GRAM_CASES)
def test_gram_forward(cuda, dtype, case):
    from basicsr4rs_amd.ops import perceptual as P
    lib = _lib.load()
    C, HW = _gram_hw(case)
    N = 2
    assert lib.sr_gram_splits(HW) == {'split_min': 2, 'split_uneven': 3}.get(case, 1)
    g = torch.Generator().manual_seed(C + HW)
    f = torch.randn(N, HW, C, generator=g).to(dtype)
    scale = float(np.float32(1.0 / (C * HW)))
    f64 = f.double()
    ref = f64.transpose(1, 2).bmm(f64) * scale
    bound = (HW + 2) * U * scale * f64.abs().transpose(1, 2).bmm(f64.abs())
    fd = f.to(cuda)
    got, ws_bytes = _gram_raw(fd, scale)
    assert (ws_bytes > 0) == case.startswith('split')
    _check(got, ref, bound, f'gram_fwd {case} C={C} HW={HW}')
    again, _ = _gram_raw(fd, scale)
    assert torch.equal(_bits(got), _bits(again)), 'two runs differ'
    # the op (scale 1 / (C H W) computed by it) gives the same bits
    assert torch.equal(_bits(P.gram(fd)), _bits(got))


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('case', GRAM_CASES + ['rows_per_block'])
def test_gram_backward(cuda, dtype, case, with_res):
    from basicsr4rs_amd.ops import perceptual as P
    C, HW = _gram_hw(case)
    N = 2
    g = torch.Generator().manual_seed(C + HW + 1)
    f = torch.randn(N, HW, C, generator=g).to(dtype)
    dG = torch.randn(N, C, C, generator=g)  # not symmetric
    res = torch.randn(N, HW, C, generator=g).to(dtype) if with_res else None
    alpha, beta = float(np.float32(1.0 / (C * HW))), 0.75
    sym = dG.double() + dG.double().transpose(1, 2)
    ref = alpha * f.double().bmm(sym)
    bound = (C + 3) * U * f.double().abs().bmm(sym.abs()) * abs(alpha)
    if with_res:
        ref = ref + beta * res.double()
        bound = bound + (beta * res.double()).abs() * U
    fd, dGd = f.to(cuda), dG.to(cuda)
    resd = res.to(cuda) if with_res else None
    got = P.gram_bwd_raw(fd, dGd, alpha, res=resd, beta=beta)
    assert got.dtype == dtype
    _check(got, ref, bound, f'gram_bwd {case} C={C} HW={HW} res={with_res}')
    assert torch.equal(_bits(got), _bits(P.gram_bwd_raw(fd, dGd, alpha, res=resd, beta=beta))), 'two runs differ'
    if case == 'k_tail':
        # autograd: gram(feat, res_grad) hands res_grad to the same store with beta = 1
        fa = fd.clone().requires_grad_(True)
        P.gram(fa, res_grad=resd).backward(dGd)
        want = P.gram_bwd_raw(fd, dGd, P.gram_scale(fd), res=resd, beta=1.0)
        assert torch.equal(_bits(fa.grad), _bits(want))


# ---------------------------------------------------------------------------------------------------------
# float64 restatement of the extractor and of the loss
# ---------------------------------------------------------------------------------------------------------
class _Store(torch.autograd.Function):
    """A map as the bf16 engine keeps it: rounded to bf16 forward, its gradient map rounded to bf16 backward."""

    @staticmethod
    def forward(ctx, t):
        return _rne_bf16(t.detach())

    @staticmethod
    def backward(ctx, g):
        return _rne_bf16(g)


def _layers(upto, vgg_type='vgg19'):
    names = NAMES[vgg_type]
    return names[:names.index(upto) + 1]


def _vgg(x, W, layers, taps, range_norm, stored=lambda t: t):
    """vgg_arch.py:141-161 in x's dtype: {tap: NCHW map}; ``stored`` wraps every map the engine keeps."""
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    h = (x + 1) / 2 if range_norm else x
    h = stored((h - mean) / std)
    out = {}
    for name in layers:
        if name.startswith('conv'):
            w, b = W[name]
            h = stored(F.conv2d(h, w, b, padding=1))
        elif name.startswith('relu'):
            h = F.relu(h)
        else:
            h = F.max_pool2d(h, 2, 2)
        if name in taps:
            out[name] = h
    return out


def _gram_mat(f):
    n, c, h, w = f.shape
    m = f.reshape(n, c, h * w)
    return m.bmm(m.transpose(1, 2)) / (c * h * w)


def _ploss(xf, gf, layer_weights, pw, sw, crit):
    """basic_loss.py:198-238 on feature dicts."""

    def cr(a, b):
        if crit == 'l1':
            return (a - b).abs().mean()
        if crit == 'l2':
            return ((a - b)**2).mean()
        return torch.norm(a - b, p='fro')

    percep = style = None
    if pw > 0:
        percep = sum(cr(xf[k], gf[k]) * w for k, w in layer_weights.items()) * pw
    if sw > 0:
        style = sum(cr(_gram_mat(xf[k]), _gram_mat(gf[k])) * w for k, w in layer_weights.items()) * sw
    return percep, style


def _modes(W):
    """The three restatements: exact float64, fp32 on the CPU, bf16 storage emulated in float64."""
    return {
        'f64': (torch.float64, {k: (w.double(), b.double()) for k, (w, b) in W.items()}, lambda t: t),
        'f32': (torch.float32, {k: (w.float(), b.float()) for k, (w, b) in W.items()}, lambda t: t),
        'emu': (torch.float64, {k: (_rne_bf16(w.double()), b.double()) for k, (w, b) in W.items()}, _Store.apply),
    }


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _rel(a, b):
    return abs(float(a) - float(b)) / max(1e-300, abs(float(b)))


def _measure(fn, W):
    """fn(dtype, weights, stored) -> dict of tensors.  Returns the float64 results and, per key, the bounds
    {fp32: 8 x rel-L2 of the fp32 CPU run, bf16: 2 x rel-L2 of the bf16-storage emulation}."""
    runs = {m: fn(*a) for m, a in _modes(W).items()}
    ref = runs['f64']
    bounds = {k: {torch.float32: 8 * _l2(runs['f32'][k], ref[k]), torch.bfloat16: 2 * _l2(runs['emu'][k], ref[k])}
              for k in ref}
    return ref, bounds


@functools.lru_cache(None)
def _weights(upto='conv5_4', seed=0):
    """He-normal conv weights (std sqrt(2 / (9 cin))) and small biases: magnitudes hold through the depth."""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for name in _layers(upto):
        if name.startswith('conv'):
            cin, cout = conv_channels(name)
            W[name] = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin))**0.5,
                       torch.randn(cout, generator=g) * 0.01)
    return W


def _load(vgg, W):
    with torch.no_grad():
        for name, (w, b) in W.items():
            getattr(vgg.vgg_net, name).weight.copy_(w)
            getattr(vgg.vgg_net, name).bias.copy_(b)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------
# 4. extractor
# ---------------------------------------------------------------------------------------------------------
TAPS = ['conv1_2', 'relu2_1', 'conv3_4', 'pool4', 'conv5_4']


@functools.lru_cache(None)
def _extractor_case(range_norm):
    W = _weights()
    g = torch.Generator().manual_seed(1 + int(range_norm))  # another image, not the same one rescaled
    x = torch.rand(1, 3, 32, 32, generator=g)
    if range_norm:
        x = x * 2 - 1
    layers = _layers('conv5_4')
    with torch.no_grad():
        shapes = {t: v.shape for t, v in _vgg(x.double(), _modes(W)['f64'][1], layers, TAPS, range_norm).items()}
    cot = {t: torch.randn(s, generator=g, dtype=torch.float64) for t, s in shapes.items()}

    def run(dtype, Wm, stored):
        xr = x.detach().to(dtype).clone().requires_grad_(True)
        feats = _vgg(xr, Wm, layers, TAPS, range_norm, stored)
        sum((feats[t] * cot[t].to(dtype)).sum() for t in TAPS).backward()
        return dict({t: v.detach() for t, v in feats.items()}, dx=xr.grad)

    ref, bounds = _measure(run, W)
    return x, cot, ref, bounds


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('range_norm', [False, True], ids=['unit_range', 'range_norm'])
def test_extractor_matches_float64(cuda, dtype, range_norm):
    from basicsr4rs_amd.archs import build_network
    from basicsr4rs_amd.utils import ktrace
    x, cot, ref, bounds = _extractor_case(range_norm)
    net = build_network(dict(type='VGGFeatureExtractor', layer_name_list=TAPS, range_norm=range_norm, pretrained=False))
    assert list(net.vgg_net._modules)[-1] == 'conv5_4'
    _load(net, _weights())
    net = net.to(cuda)
    xd = x.to(cuda).requires_grad_(True)
    ktrace.start()
    try:
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            feats = net(xd)
            nchw = net(xd.detach(), to_nchw=True)
        assert list(feats) == TAPS
        sum((feats[t].float() * _nhwc(cot[t]).float().to(cuda)).sum() for t in TAPS).backward()
    finally:
        rec = ktrace.stop()
    bad = []
    for t in TAPS:
        assert feats[t].dtype == dtype and nchw[t].dtype == torch.float32
        got = feats[t].detach().float().permute(0, 3, 1, 2).cpu()
        assert torch.equal(nchw[t].cpu(), got), t
        err, b = _l2(got, ref[t]), bounds[t][dtype]
        print(f'extractor {_ids(dtype)} range_norm={range_norm} {t}: rel-L2 {err:.3e}, bound {b:.3e}')
        if not err <= b:
            bad.append((t, err, b))
    err, b = _l2(xd.grad.cpu(), ref['dx']), bounds['dx'][dtype]
    print(f'extractor {_ids(dtype)} range_norm={range_norm} dx: rel-L2 {err:.3e}, bound {b:.3e}')
    if not err <= b:
        bad.append(('dx', err, b))
    assert not bad, bad
    assert 'maxpool2_fwd_kernel' in rec and 'maxpool2_bwd_kernel' in rec, sorted(rec)
    assert any('conv3x3_fwd' in k for k in rec), sorted(rec)
    assert not any('wgrad' in k for k in rec), sorted(rec)  # frozen weights: no weight gradient is launched
    assert all(p.grad is None for p in net.parameters())


def test_extractor_trainable_weights_get_gradients(cuda):
    """requires_grad=True goes through the conv autograd (the wgrad kernels run)."""
    from basicsr4rs_amd.archs.vgg_arch import VGGFeatureExtractor
    from basicsr4rs_amd.utils import ktrace
    W = _weights('conv2_1')
    net = VGGFeatureExtractor(['conv2_1'], requires_grad=True, pretrained=False)
    _load(net, W)
    net = net.to(cuda)
    x = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    layers = _layers('conv2_1')
    W64 = {k: (w.double().requires_grad_(True), b.double().requires_grad_(True)) for k, (w, b) in W.items()}
    f64 = _vgg(x.double(), W64, layers, ['conv2_1'], False)['conv2_1']
    cot = torch.randn(f64.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (f64 * cot).sum().backward()
    ktrace.start()
    try:
        (net(x.to(cuda))['conv2_1'] * _nhwc(cot).float().to(cuda)).sum().backward()
    finally:
        rec = ktrace.stop()
    assert any('wgrad' in k for k in rec), sorted(rec)
    for name, (w, b) in W64.items():
        conv = getattr(net.vgg_net, name)
        assert _l2(conv.weight.grad.cpu(), w.grad) < 1e-5 and _l2(conv.bias.grad.cpu(), b.grad) < 1e-5, name


# ---------------------------------------------------------------------------------------------------------
# 5. PerceptualLoss
# ---------------------------------------------------------------------------------------------------------
ESRGAN_WEIGHTS = {'conv1_2': .1, 'conv2_2': .1, 'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1}


def _loss_inputs():
    g = torch.Generator().manual_seed(5)
    # x != gt (fro has no gradient at 0), and of another brightness, so that the Gram matrices differ too
    return torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g) * 0.5 + 0.1


def _loss_run(x, gt, layer_weights, layers, pw, sw, crit):

    def run(dtype, Wm, stored):
        xr = x.detach().to(dtype).clone().requires_grad_(True)
        taps = list(layer_weights)
        xf = _vgg(xr, Wm, layers, taps, False, stored)
        with torch.no_grad():
            gf = _vgg(gt.to(dtype), Wm, layers, taps, False, stored)
        p, s = _ploss(xf, gf, layer_weights, pw, sw, crit)
        sum(v for v in (p, s) if v is not None).backward()
        out = dict(dx=xr.grad)
        if p is not None:
            out['percep'] = p.detach()
        if s is not None:
            out['style'] = s.detach()
        return out

    return run


def _value_bound(dtype, *range_norms):
    """The widest per-tap bound of test 4 for this dtype: the bound of a scalar made of those features."""
    return max(b[dtype] for rn in range_norms for k, b in _extractor_case(rn)[3].items() if k != 'dx')


@pytest.mark.parametrize('pw,sw', [(1.0, 0.5), (1.0, 0.0), (0.0, 0.5)], ids=['both', 'percep_only', 'style_only'])
@pytest.mark.parametrize('crit', ['l1', 'l2', 'fro'])
def test_perceptual_loss_matches_float64(cuda, crit, pw, sw):
    from basicsr4rs_amd.losses import build_loss
    x, gt = _loss_inputs()
    W = _weights()
    ref, bounds = _measure(_loss_run(x, gt, ESRGAN_WEIGHTS, _layers('conv5_4'), pw, sw, crit), W)
    loss = build_loss(dict(type='PerceptualLoss', layer_weights=dict(ESRGAN_WEIGHTS), vgg_type='vgg19',
                           use_input_norm=True, range_norm=False, perceptual_weight=pw, style_weight=sw,
                           criterion=crit, pretrained=False))
    _load(loss.vgg, W)
    loss = loss.to(cuda)
    bad = []
    for dtype in DTYPES:
        xd = x.to(cuda).requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            p, s = loss(xd, gt.to(cuda))
        assert (p is None) == (pw == 0) and (s is None) == (sw == 0)
        sum(v for v in (p, s) if v is not None).backward()
        vb = _value_bound(dtype, False)
        for key, v in (('percep', p), ('style', s)):
            if v is not None:
                assert v.dtype == torch.float32 and v.dim() == 0
                err = _rel(v.item(), ref[key])
                print(f'PerceptualLoss {crit} pw={pw} sw={sw} {_ids(dtype)} {key}: {v.item():.6e} vs {float(ref[key]):.6e}, '
                      f'rel {err:.3e}, bound {vb:.3e} (its own restatements: {bounds[key][dtype]:.3e})')
                if not err <= vb:
                    bad.append((key, _ids(dtype), err, vb))
        err, b = _l2(xd.grad.cpu(), ref['dx']), bounds['dx'][dtype]
        print(f'PerceptualLoss {crit} pw={pw} sw={sw} {_ids(dtype)} dx: rel-L2 {err:.3e}, bound {b:.3e}')
        if not err <= b:
            bad.append(('dx', _ids(dtype), err, b))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# 6. train step
# ---------------------------------------------------------------------------------------------------------
STEP_WEIGHTS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0}


def _train_opt(model_type='SRModel', amp=False, graph=False):
    return dict(model_type=model_type, is_train=True, dist=False, num_gpu=1, path={}, scale=2,
                network_g=dict(type='MSRResNet', num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1, upscale=2),
                train=dict(ema_decay=0.999, use_amp=amp, cuda_graph=graph,
                           optim_g=dict(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99]),
                           scheduler=dict(type='MultiStepLR', milestones=[4], gamma=0.5),
                           pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean'),
                           perceptual_opt=dict(type='PerceptualLoss', layer_weights=dict(STEP_WEIGHTS), vgg_type='vgg19',
                                               use_input_norm=True, range_norm=False, perceptual_weight=1.0,
                                               style_weight=0.5, criterion='l1', pretrained=False)))


def _batch(it):
    g = torch.Generator().manual_seed(it)
    return {'lq': torch.rand(2, 3, 16, 16, generator=g), 'gt': torch.rand(2, 3, 32, 32, generator=g)}


@pytest.mark.parametrize('model_type,amp', [('SRModel', False), ('SRRSModel', True)], ids=['SRModel_fp32', 'SRRSModel_amp'])
def test_train_step_logs_the_float64_losses(cuda, model_type, amp):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_train_opt(model_type, amp))
    assert type(model).__name__ == model_type and model.cri_perceptual is not None
    vgg = model.cri_perceptual.vgg
    assert not any(p.requires_grad for p in vgg.parameters())
    net = model.get_bare_model(model.net_g)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    data = _batch(1)
    model.feed_data(data)
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) == {'l_pix', 'l_percep', 'l_style'} and all(np.isfinite(v) for v in log.values()), log
    # the float64 restatement of the three losses on the step's own network output
    out = model.output.detach().double().cpu()
    gt = data['gt']
    W = {n: (getattr(vgg.vgg_net, n).weight.detach().cpu(), getattr(vgg.vgg_net, n).bias.detach().cpu())
         for n in vgg.vgg_net._modules}
    dtype = torch.bfloat16 if amp else torch.float32
    layers = _layers('conv3_4')
    ref, bounds = _measure(_loss_run(out, gt, STEP_WEIGHTS, layers, 1.0, 0.5, 'l1'), W)

    def feats(dt, Wm, stored):
        with torch.no_grad():
            return _vgg(out.to(dt), Wm, layers, list(STEP_WEIGHTS), False, stored)

    vb = max(b[dtype] for b in _measure(feats, W)[1].values())
    l_pix = (out - gt.double()).abs().mean().item()
    print(f'{model_type} l_pix {log["l_pix"]:.6e} vs {l_pix:.6e}')
    assert _rel(log['l_pix'], l_pix) < 1e-5  # the bar of test_train_step_gpu.py for the fused L1
    for key, name in (('percep', 'l_percep'), ('style', 'l_style')):
        err = _rel(log[name], ref[key])
        print(f'{model_type} {name} {log[name]:.6e} vs {float(ref[key]):.6e}: rel {err:.3e}, bound {vb:.3e} '
              f'(its own restatements: {bounds[key][dtype]:.3e})')
        assert err <= vb, (name, err, vb)
    moved = [k for k, v in net.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))
    assert all(torch.isfinite(v).all() for v in net.parameters())


def test_train_step_hip_graph_matches_eager(cuda):
    """train.cuda_graph with the perceptual and style terms: steps 1-2 eager, step 3 captured and run, steps
    4-6 replays (an lr milestone in between) give bitwise the parameters, EMA and losses of six eager steps."""
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    runs = []
    for graph in (False, True):
        torch.manual_seed(0)
        model = build_model(_train_opt(graph=graph))
        losses = []
        for it in range(1, 7):
            model.feed_data(_batch(it))
            model.update_learning_rate(it)
            model.optimize_parameters(it)
            log = model.get_current_log()
            losses.append((log['l_pix'], log['l_percep'], log['l_style']))
        assert (model._graph is not None) == graph
        net = model.get_bare_model(model.net_g)
        runs.append((losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                     {k: v.detach().cpu().clone() for k, v in model.net_g_ema.state_dict().items()}))
    (l0, p0, e0), (l1, p1, e1) = runs
    assert l0 == l1
    assert all(np.isfinite(v) for row in l0 for v in row)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
        assert torch.equal(e0[k], e1[k]), k
