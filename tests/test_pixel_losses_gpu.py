"""Pixel-loss family on the GPU (csrc/loss.hip through losses/basic_loss.py) against a float64 CPU
restatement of the reference: the three phi of basicsr/losses/basic_loss.py:12-24 and weight_reduce_loss
(loss_util.py:26-55), in plain torch on the same fp32- (or bf16-) rounded inputs.

Shapes: (1,1,1,3) is less than one vector (tail only); (2,3,5,7) has n and H*W that are no multiples of 4,
so vector lanes straddle channel and image boundaries of the broadcast weight; _big_shape() is one notch
more than one full sweep of the kernel's grid -- min(8 * CUs, 4096) blocks x 256 threads x 4 fp32
elements, 2,097,152 elements on the 256 CUs of an MI355X, where it is (2,3,591,593) = 2,102,778 elements
(n % 4 = 2, H*W odd) -- so the last blocks take a second grid-stride trip.

Bounds (from the issue, not from the kernel's results): loss |got - ref| <= 1e-5 * max(1, |ref|); fp32
gradient |got - ref| <= 1e-5 * |ref| + 1e-6 * max|ref| elementwise; bf16 gradient one bf16 rounding,
2^-8 relative; exact zeros at d == 0 and under zero weight; the target gradient, an element-aligned
(storage-offset) prediction and a second call are bitwise equal to their counterparts.

The unweighted L1 mean / sum whose target needs no gradient -- the loss of every SR train YAML -- runs
another kernel, sr_l1_loss (csrc/eltwise.hip): the test_l1_fused_* tests put it under the same reference
and bounds, assert the autograd node so that they cannot run sr_pixel_loss instead, and cover a NaN
prediction and storage-offset views of both operands.
"""
import functools

import pytest
import torch

from oracle import nets as O

pytestmark = pytest.mark.gpu

KINDS = ['L1Loss', 'MSELoss', 'CharbonnierLoss']
WEIGHTS = ['none', 'n1hw', 'nchw']
REDUCTIONS = ['mean', 'sum', 'none']
LW = 0.7
EPS = 1e-12


def _big_shape():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweep = min(8 * cus, 4096) * 256 * 4
    h = 1
    while 6 * h * (h + 2) <= sweep or (6 * h * (h + 2)) % 4 == 0:
        h += 2
    assert sweep < 6 * h * (h + 2) < 2 * sweep
    return (2, 3, h, h + 2)


SHAPES = {'tail': lambda: (1, 1, 1, 3), 'odd': lambda: (2, 3, 5, 7), 'big': _big_shape}


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype=torch.float32, tdtype=torch.float32):
    """Seeded inputs of one shape, shared by every test (never modified): uniform in [-1, 1]; every
    97th prediction equals its target (sign(0), the Charbonnier eps), every 101st is target + 1e-7;
    the one-channel weight has about 30 % exact zeros, the full weight a few."""
    g = torch.Generator().manual_seed(1234 + len(shape) + sum(shape))
    n = 1
    for s in shape:
        n *= s
    target = (torch.rand(n, generator=g) * 2 - 1).to(tdtype).float()
    pred = torch.rand(n, generator=g) * 2 - 1
    pred[::101] = target[::101] + 1e-7
    pred[::97] = target[::97]
    pred = pred.to(dtype)
    N, C, H, W = shape
    w1 = torch.rand(N, 1, H, W, generator=g)
    w1[torch.rand(N, 1, H, W, generator=g) < 0.3] = 0.0
    wc = torch.rand(N, C, H, W, generator=g)
    wc.view(-1)[::13] = 0.0
    up = torch.rand(shape, generator=g) + 0.5  # upstream gradient map of reduction 'none'
    host = dict(pred=pred.view(shape), target=target.to(tdtype).view(shape), n1hw=w1, nchw=wc, up=up)
    dev = {k: v.cuda() for k, v in host.items()}
    return host, dev


def _phi(kind, d, eps):
    if kind == 'L1Loss':
        return d.abs()
    if kind == 'MSELoss':
        return d**2
    return torch.sqrt(d**2 + eps)


def _ref(kind, pred, target, weight, reduction, up=None, lw=LW, eps=EPS):
    """float64 restatement: (loss, d loss / d pred); for 'none' the gradient of sum(loss * up)."""
    p = pred.double().requires_grad_(True)
    loss = _phi(kind, p - target.double(), eps)
    if weight is not None:
        weight = weight.double()
        loss = loss * weight
    if reduction == 'sum':
        loss = loss.sum()
    elif reduction == 'mean':
        if weight is None:
            loss = loss.mean()
        else:
            loss = loss.sum() / (weight.sum() if weight.size(1) > 1 else weight.sum() * loss.size(1))
    loss = lw * loss
    (loss * up.double()).sum().backward() if reduction == 'none' else loss.backward()
    return loss.detach(), p.grad


def _build(kind, reduction, lw=LW):
    from basicsr4rs_amd.losses import build_loss
    opt = dict(type=kind, loss_weight=lw, reduction=reduction)
    if kind == 'CharbonnierLoss':
        opt['eps'] = EPS
    return build_loss(opt)


def _run(kind, reduction, pred, target, weight, up=None, target_grad=True, names=None):
    """(loss, pred gradient, target gradient) of the HIP path.  By default the target asks for its
    gradient, which also takes the unweighted L1 mean / sum onto sr_pixel_loss (sr_l1_loss has no target
    gradient); with target_grad=False that case runs sr_l1_loss.  ``names``: a list that receives the
    name of the loss's autograd node."""
    p = pred.detach().requires_grad_(True)
    t = target.detach().requires_grad_(target_grad)
    loss = _build(kind, reduction)(p, t, weight)
    if names is not None:
        names.append(type(loss.grad_fn).__name__)
    (loss * up).sum().backward() if reduction == 'none' else loss.backward()
    return loss.detach(), p.grad, t.grad


def _check_loss(got, ref, what):
    err = (got.double().cpu() - ref).abs()
    bound = 1e-5 * ref.abs().clamp(min=1.0)
    print(f'{what}: loss max|err| {err.max().item():.3e} (ref max {ref.abs().max().item():.6e})')
    assert (err <= bound).all(), (what, err.max().item())


def _check_grad(got, ref, what):
    err = (got.double().cpu() - ref).abs()
    bound = 1e-5 * ref.abs() + 1e-6 * ref.abs().max()
    rel = (err / ref.abs().clamp(min=1e-300))[ref != 0]
    print(f'{what}: grad max|err| {err.max().item():.3e}, max rel {rel.max().item() if rel.numel() else 0.0:.3e} '
          f'(ref max {ref.abs().max().item():.3e})')
    assert (err <= bound).all(), (what, err.max().item())


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('reduction', REDUCTIONS)
@pytest.mark.parametrize('wmode', WEIGHTS)
@pytest.mark.parametrize('kind', KINDS)
def test_loss_and_gradients_match_float64(cuda, kind, wmode, reduction, shape):
    shp = SHAPES[shape]()
    host, dev = _inputs(shp)
    w_h, w_d = (None, None) if wmode == 'none' else (host[wmode], dev[wmode])
    ref_loss, ref_grad = _ref(kind, host['pred'], host['target'], w_h, reduction, host['up'])
    loss, gp, gt = _run(kind, reduction, dev['pred'], dev['target'], w_d, dev['up'])
    what = f'{kind} {wmode} {reduction} {shp}'
    assert loss.dtype == torch.float32 and gp.dtype == torch.float32
    assert loss.shape == (shp if reduction == 'none' else ())
    _check_loss(loss, ref_loss, what)
    _check_grad(gp, ref_grad, what)
    # exact zeros where d == 0 and under zero weight; the target gradient is the negation, bitwise
    zero = host['pred'] == host['target']
    if w_h is not None:
        zero = zero | (w_h == 0).expand(shp)
    assert zero.any() or shape == 'tail'
    assert (gp.cpu()[zero] == 0).all()
    assert torch.equal(gt, -gp)


@pytest.mark.parametrize('tdtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('wmode', WEIGHTS)
@pytest.mark.parametrize('kind', KINDS)
def test_bf16_prediction(cuda, kind, wmode, tdtype):
    """bf16 pred read directly (fp32 or bf16 target) at the L2S band count: the inputs upcast exactly, so
    the loss bound is the fp32 one; the gradient is stored in bf16: one rounding, 2^-8 relative."""
    shp = (2, 6, 48, 48)
    host, dev = _inputs(shp, torch.bfloat16, tdtype)
    assert dev['pred'].dtype == torch.bfloat16 and dev['target'].dtype == tdtype
    w_h, w_d = (None, None) if wmode == 'none' else (host[wmode], dev[wmode])
    # the upstream map of 'none' reaches the backward in the map's dtype, bf16: use bf16 values, so that
    # the cast is exact and the reference sees the same map
    up_h, up_d = host['up'].bfloat16().float(), dev['up'].bfloat16().float()
    for reduction in ('mean', 'none'):
        ref_loss, ref_grad = _ref(kind, host['pred'], host['target'], w_h, reduction, up_h)
        loss, gp, gt = _run(kind, reduction, dev['pred'], dev['target'], w_d, up_d)
        what = f'{kind} {wmode} {reduction} bf16 pred, {tdtype} target'
        assert gp.dtype == torch.bfloat16 and gt.dtype == tdtype
        if reduction == 'none':
            # the map is stored in pred's dtype: one bf16 rounding of the float64 value
            assert loss.dtype == torch.bfloat16
            err = (loss.double().cpu() - ref_loss).abs()
            assert (err <= 2.0**-8 * ref_loss.abs()).all(), (what, err.max().item())
            # two bf16 roundings: the stored local derivative, and its product with the upstream map.
            # One rounding is at most u / (1 + u) relative, u = 2^-8, so two stay below 2u.
            gbound = 2 * 2.0**-8
        else:
            assert loss.dtype == torch.float32
            _check_loss(loss, ref_loss, what)
            gbound = 2.0**-8
        err = (gp.double().cpu() - ref_grad).abs()
        rel = (err / ref_grad.abs().clamp(min=1e-300))[ref_grad != 0].max().item()
        print(f'{what}: grad max rel {rel:.3e}')
        assert (err <= gbound * ref_grad.abs()).all(), (what, rel)
        assert torch.equal(gt.float(), -gp.float())


@pytest.mark.parametrize('shape', ['odd', 'big'])
@pytest.mark.parametrize('reduction', ['mean', 'none'])
@pytest.mark.parametrize('wmode', WEIGHTS)
@pytest.mark.parametrize('kind', KINDS)
def test_storage_offset_view_bitwise(cuda, kind, wmode, reduction, shape):
    """A prediction that is only element-aligned (a storage-offset view; the target stays aligned, and
    for the weighted cases the weight map is offset too) gives the bits of an aligned copy."""
    shp = SHAPES[shape]()
    _, dev = _inputs(shp)
    n = dev['pred'].numel()
    buf = torch.empty(n + 8, device=cuda)
    pv = buf.view(-1)[1:1 + n].view(shp)
    pv.copy_(dev['pred'])
    assert pv.data_ptr() % 16 == 4 and pv.is_contiguous() and dev['pred'].data_ptr() % 16 == 0
    w, wv = None, None
    if wmode != 'none':
        w = dev[wmode]
        wv = torch.empty(w.numel() + 8, device=cuda)[3:3 + w.numel()].view(w.shape)
        wv.copy_(w)
        assert wv.data_ptr() % 16 == 12
    a = _run(kind, reduction, dev['pred'], dev['target'], w, dev['up'])
    b = _run(kind, reduction, pv, dev['target'], wv, dev['up'])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_l1_fused_path_matches_float64(cuda, reduction, shape):
    """The hot path of every SR train YAML: unweighted L1 mean / sum with a target that needs no
    gradient runs sr_l1_loss (csrc/eltwise.hip), not sr_pixel_loss; same reference, same bounds."""
    shp = SHAPES[shape]()
    host, dev = _inputs(shp)
    ref_loss, ref_grad = _ref('L1Loss', host['pred'], host['target'], None, reduction)
    names = []
    loss, gp, gt = _run('L1Loss', reduction, dev['pred'], dev['target'], None, target_grad=False, names=names)
    assert '_L1Fused' in names[0], names
    what = f'L1Loss fused {reduction} {shp}'
    assert gt is None and loss.dtype == torch.float32 and gp.dtype == torch.float32 and loss.shape == ()
    _check_loss(loss, ref_loss, what)
    _check_grad(gp, ref_grad, what)
    zero = host['pred'] == host['target']
    assert zero.any() or shape == 'tail'
    assert (gp.cpu()[zero] == 0).all()


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_l1_fused_nan_prediction_gives_nan_loss(cuda, reduction):
    """SRRSModel skips the step on a non-finite loss: one NaN in the prediction must reach the loss."""
    shp = SHAPES['odd']()
    _, dev = _inputs(shp)
    pred = dev['pred'].clone()
    pred[1, 2, 3, 4] = float('nan')
    names = []
    loss, gp, _ = _run('L1Loss', reduction, pred, dev['target'], None, target_grad=False, names=names)
    assert '_L1Fused' in names[0], names
    assert torch.isnan(loss).item()
    ok = torch.ones(shp, dtype=torch.bool)
    ok[1, 2, 3, 4] = False
    assert torch.isfinite(gp.cpu()[ok]).all()


def _offset_view(x, off):
    buf = torch.empty(x.numel() + 8, device=x.device, dtype=x.dtype)
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16 and torch.equal(v, x)
    return v


@pytest.mark.parametrize('shape,which,off', [('odd', w, o) for w in ('pred', 'target', 'both') for o in (1, 2, 3)] +
                         [('tail', 'both', 1), ('big', 'both', 3)])
@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_l1_fused_storage_offset_view(cuda, reduction, shape, which, off):
    """Contiguous views at element offsets 1, 2, 3 of a larger buffer (4, 8, 12 bytes past a 16-byte
    boundary), e.g. buf[1:1 + n].view(shape), give the bits of aligned clones on the sr_l1_loss path."""
    shp = SHAPES[shape]()
    _, dev = _inputs(shp)
    assert dev['pred'].data_ptr() % 16 == 0 and dev['target'].data_ptr() % 16 == 0
    pv = _offset_view(dev['pred'], off) if which in ('pred', 'both') else dev['pred']
    tv = _offset_view(dev['target'], off) if which in ('target', 'both') else dev['target']
    names = []
    a = _run('L1Loss', reduction, dev['pred'], dev['target'], None, target_grad=False, names=names)
    b = _run('L1Loss', reduction, pv, tv, None, target_grad=False, names=names)
    assert all('_L1Fused' in n for n in names), names
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _tv_ref(pred, weight, reduction, lw=LW):
    p = pred.double().requires_grad_(True)
    yw = xw = None
    if weight is not None:
        yw, xw = weight[:, :, :-1, :], weight[:, :, :, :-1]

    def l1(a, b, w):
        loss = (a - b).abs()
        if w is not None:
            loss = loss * w.double()
        if reduction == 'sum':
            return lw * loss.sum()
        if w is None:
            return lw * loss.mean()
        return lw * loss.sum() / (w.double().sum() if w.size(1) > 1 else w.double().sum() * loss.size(1))

    loss = l1(p[:, :, :, :-1], p[:, :, :, 1:], xw) + l1(p[:, :, :-1, :], p[:, :, 1:, :], yw)
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('wmode', WEIGHTS)
def test_weighted_tv_loss(cuda, wmode, reduction):
    """WeightedTVLoss (basic_loss.py:117-143): both slices of each pair are views of the prediction, so
    its gradient arrives through pred and (negated) through target."""
    from basicsr4rs_amd.losses import build_loss
    shp = SHAPES['odd']()
    host, dev = _inputs(shp)
    w_h, w_d = (None, None) if wmode == 'none' else (host[wmode], dev[wmode])
    ref_loss, ref_grad = _tv_ref(host['pred'], w_h, reduction)
    p = dev['pred'].detach().requires_grad_(True)
    loss = build_loss(dict(type='WeightedTVLoss', loss_weight=LW, reduction=reduction))(p, weight=w_d)
    loss.backward()
    what = f'WeightedTVLoss {wmode} {reduction}'
    _check_loss(loss.detach(), ref_loss, what)
    _check_grad(p.grad, ref_grad, what)


@pytest.mark.parametrize('kind,wmode,reduction', [('CharbonnierLoss', 'n1hw', 'mean'), ('MSELoss', 'nchw', 'sum'),
                                                  ('L1Loss', 'n1hw', 'none')])
def test_two_calls_bitwise_equal(cuda, kind, wmode, reduction):
    _, dev = _inputs(SHAPES['big']())
    a = _run(kind, reduction, dev['pred'], dev['target'], dev[wmode], dev['up'])
    b = _run(kind, reduction, dev['pred'], dev['target'], dev[wmode], dev['up'])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_weight_requiring_grad_and_other_shapes_use_reference_formula(cuda):
    """A weight map that requires grad, or of a shape the kernel does not cover, goes through torch ops:
    same value, and the weight receives its gradient."""
    shp = SHAPES['odd']()
    host, dev = _inputs(shp)
    ref_loss, ref_grad = _ref('MSELoss', host['pred'], host['target'], host['nchw'], 'mean')
    w = dev['nchw'].clone().requires_grad_(True)
    p = dev['pred'].detach().requires_grad_(True)
    loss = _build('MSELoss', 'mean')(p, dev['target'], w)
    loss.backward()
    _check_loss(loss.detach(), ref_loss, 'MSE, weight requires grad')
    _check_grad(p.grad, ref_grad, 'MSE, weight requires grad')
    assert w.grad is not None and w.grad.shape == w.shape
    # a [1,C,1,1] weight broadcasts in torch; weight_reduce_loss divides by its own sum
    wb = torch.rand(1, shp[1], 1, 1, device=cuda)
    got = _build('L1Loss', 'sum')(dev['pred'], dev['target'], wb)
    ref = LW * ((host['pred'] - host['target']).abs().double() * wb.cpu().double()).sum()
    _check_loss(got, ref, 'L1 sum, per-channel weight')


def _opt(pixel_opt, ema=0.999):
    return dict(model_type='SRModel', is_train=True, dist=False, num_gpu=1, path={},
                network_g=dict(type='EDSR', num_in_ch=3, num_out_ch=3, num_feat=64, num_block=2, upscale=4,
                               res_scale=1),
                train=dict(ema_decay=ema, use_amp=False, optim_g=dict(type='Adam', lr=1e-3, weight_decay=0,
                                                                      betas=[0.9, 0.99]),
                           scheduler=dict(type='MultiStepLR', milestones=[100], gamma=0.5),
                           pixel_opt=pixel_opt))


@pytest.mark.parametrize('kind', ['MSELoss', 'CharbonnierLoss'])
def test_sr_model_train_step_matches_float64_replay(cuda, kind):
    """The set-up of test_train_step_gpu.test_sr_model_train_step_matches_oracle with another pixel_opt:
    2 fp32 steps of the 2-block EDSR against a float64 replay with torch.optim.Adam."""
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_opt(dict(type=kind, loss_weight=1.0, reduction='mean')))
    net = model.get_bare_model(model.net_g)
    sd0 = {k: v.detach().cpu().double().clone() for k, v in net.state_dict().items()}
    params = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    ema = {k: v.clone() for k, v in sd0.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-3, betas=(0.9, 0.99))
    lq = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(0))
    gt = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    model.feed_data({'lq': lq, 'gt': gt})
    for it in (1, 2):
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        opt.zero_grad()
        loss = _phi(kind, O.edsr(params, lq.double(), num_block=2, upscale=4) - gt.double(), 1e-12).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k in ema:
                ema[k].mul_(0.999).add_(params[k], alpha=0.001)
        got = model.get_current_log()['l_pix']
        print(f'{kind} step {it}: l_pix {got:.8f} replay {loss.item():.8f}')
        assert abs(got - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    worst = 0.0
    for k, v in net.state_dict().items():
        ref = params[k].detach()
        err = (v.cpu().double() - ref).abs().max().item() / max(1e-3, ref.abs().max().item())
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    for k, v in model.net_g_ema.state_dict().items():
        err = (v.cpu().double() - ema[k]).abs().max().item() / max(1e-3, ema[k].abs().max().item())
        assert err < 2e-4, (k, err)
    print(f'{kind}: worst relative parameter error after 2 steps {worst:.3e}')


def test_sr_model_hip_graph_matches_eager_charbonnier(cuda):
    """The pattern of test_sr_model_hip_graph_matches_eager with CharbonnierLoss: steps 1-2 eager, step 3
    captured, 4-6 replays; bitwise the eager losses, parameters and EMA."""
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    runs = []
    for graph in (False, True):
        torch.manual_seed(0)
        o = _opt(dict(type='CharbonnierLoss', loss_weight=1.0, reduction='mean'))
        o['train']['cuda_graph'] = graph
        o['train']['scheduler'] = dict(type='MultiStepLR', milestones=[4], gamma=0.5)
        model = build_model(o)
        losses = []
        for it in range(1, 7):
            g0 = torch.Generator().manual_seed(it)
            model.feed_data({'lq': torch.rand(2, 3, 16, 16, generator=g0), 'gt': torch.rand(2, 3, 64, 64, generator=g0)})
            model.update_learning_rate(it)
            model.optimize_parameters(it)
            losses.append(model.get_current_log()['l_pix'])
        assert (model._graph is not None) == graph
        net = model.get_bare_model(model.net_g)
        runs.append((losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                     {k: v.detach().cpu().clone() for k, v in model.net_g_ema.state_dict().items()}))
    (l0, p0, e0), (l1, p1, e1) = runs
    assert l0 == l1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
        assert torch.equal(e0[k], e1[k]), k
