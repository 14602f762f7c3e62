"""ECBSR on the HIP engine (collapsed train step) against the five-branch form of tests/_ecbsr_ref.py in float64
and against the recorded reference results: fp32 parity of the output and every parameter gradient, eval / train
equality, rep_params(), the slope gradients, the bf16 autocast gradients against a float64 emulation of the
engine's bf16 storage points, SRModel / SRRSModel train steps, the captured step and save -> load."""
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import _ecbsr_ref as R
from tests.golden.make_ecbsr_golden import CASES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'ecbsr.npz'))


def _state(gold, case):
    return {str(k): torch.from_numpy(gold[f'{case}.sd.{k}']) for k in gold[f'{case}.names']}


def _kw(case):
    cfg = CASES[case][0]
    return dict(scale=cfg['scale'], with_idt=cfg['with_idt'], act_type=cfg['act_type'])


def _grads(sd, x, g, kw, stored=lambda t: t):
    sdg = {k: (v.double().requires_grad_(True) if not k.endswith('.mask') else v.double()) for k, v in sd.items()}
    out = R.forward(sdg, x.double(), stored=stored, **kw)
    (out * g.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in sdg.items() if v.requires_grad}


def _net(case, sd, cuda):
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='ECBSR', **CASES[case][0]))
    net.load_state_dict(sd, strict=True)
    return net.to(cuda)


def _edge_b0(name):
    return name.endswith('.b0') and 'conv1x1_3x3' not in name


def _edge_b0_bound(sd, name, ref):
    """|g| <= 1e-5 |scale[o]| |dbias[o]| for an edge branch's b0 (exact value 0: the mask taps sum to 0)."""
    pre = name[:-2]
    return 1e-5 * sd[pre + 'scale'].reshape(-1).double().abs() * ref[pre + 'bias'].abs()


@pytest.mark.parametrize('case', list(CASES))
def test_ecbsr_parity_fp32(cuda, gold, case):
    sd = _state(gold, case)
    x, g = torch.from_numpy(gold[f'{case}.x']), torch.from_numpy(gold[f'{case}.g'])
    ref_out, ref = _grads(sd, x, g, _kw(case))
    net = _net(case, sd, cuda)
    net.train()
    out = net(x.to(cuda))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref_out.shape)
    (out * g.to(cuda)).sum().backward()
    err = (out.detach().cpu().double() - ref_out).abs().max().item()
    err_rec = (out.detach().cpu() - torch.from_numpy(gold[f'{case}.out_train'])).abs().max().item()
    print(f'ECBSR {case} fp32: output max-abs {err:.3e} vs fp64, {err_rec:.3e} vs the recording')
    assert err < 1e-3 and err_rec < 1e-3
    for n, p in net.named_parameters():
        if not p.requires_grad:
            assert p.grad is None
            continue
        got = p.grad.detach().cpu().double()
        e = (got - ref[n]).abs().max().item()
        print(f'  {n}: grad max-abs {e:.3e} (max |ref| {ref[n].abs().max().item():.3e})')
        assert e < 1e-3, (n, e)
        if _edge_b0(n):
            assert (got.abs() <= _edge_b0_bound(sd, n, ref)).all(), n
    # the slopes: zero and negative ones carry a gradient (not a vacuous check) and it is right, relatively too
    seen = {'zero': 0, 'negative': 0}
    for n, p in net.named_parameters():
        if n.endswith('act.weight'):
            a, r, got = sd[n], ref[n], p.grad.detach().cpu().double()
            for kind, sel in (('zero', a == 0), ('negative', a < 0)):
                live = sel & (r.abs() > 1e-2)
                seen[kind] += int(live.sum())
                assert ((got - r).abs()[live] <= 1e-4 * r.abs()[live]).all(), (n, kind)
    if CASES[case][0]['act_type'] == 'prelu':
        assert seen['zero'] > 0 and seen['negative'] > 0, seen
    # eval() output equals train() output bitwise
    net.eval()
    with torch.no_grad():
        ev = net(x.to(cuda))
        ev2 = net(x.to(cuda))  # cached images
    assert torch.equal(ev, out.detach()) and torch.equal(ev, ev2)
    err_ev = (ev.cpu() - torch.from_numpy(gold[f'{case}.out_eval'])).abs().max().item()
    assert err_ev < 1e-3
    # rep_params() against the fp64 collapse: (128 + 5) * 2^-24 * sum |products| (test_ecb_ops_gpu.py)
    sd64 = {k: v.double() for k, v in sd.items()}
    sda = {k: v.double().abs() for k, v in sd.items()}
    for l, blk in enumerate(net.backbone):
        w, b = blk.rep_params()
        rk, rb = R.collapse(sd64, f'backbone.{l}.', CASES[case][0]['with_idt'])
        ak, ab = R.collapse(sda, f'backbone.{l}.', CASES[case][0]['with_idt'])
        assert w.dtype == torch.float32
        assert ((w.cpu().double() - rk).abs() <= 133 * 2.0**-24 * ak).all()
        assert ((b.cpu().double() - rb).abs() <= 133 * 2.0**-24 * ab).all()


def test_ecbsr_eval_cache_follows_the_parameters(cuda, gold):
    sd = _state(gold, 'B')
    net = _net('B', sd, cuda).eval()
    x = torch.from_numpy(gold['B.x']).to(cuda)
    with torch.no_grad():
        a = net(x)
        net.backbone[0].conv3x3.bias.add_(0.125)
        b = net(x)
    assert not torch.equal(a, b)


class _Round(torch.autograd.Function):
    """A map stored in bf16: the value is rounded going forward, its gradient going backward."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


@pytest.mark.parametrize('case', ['A', 'B'])
def test_ecbsr_grad_error_is_bf16_storage_rounding(cuda, gold, case):
    """bf16 autocast: each gradient's error against the exact float64 replay is that of the same replay with the
    stored maps (input, per-layer y and z, and the dz maps) rounded to bf16: relative L2 <= 1.3 x the emulation's
    + 1e-2, max error <= 1.8 x + 2e-2 (test_srcnn_grad_error_is_bf16_storage_rounding).  Weights are pre-rounded.
    The edge branches' b0 (exact gradient 0) take their absolute bound instead.  (The collapsed weight is not a
    bf16 number even then: with a single bf16 weight image case A measured 6e-2 .. 1e-1 relative L2 against an
    emulated 3e-3, a PReLU gate flipped per layer; the engine's bf16 images carry hi + lo for that reason.)"""
    sd = {k: v.to(torch.bfloat16).float() for k, v in _state(gold, case).items()}
    x, g = torch.from_numpy(gold[f'{case}.x']), torch.from_numpy(gold[f'{case}.g'])
    _, ref = _grads(sd, x, g, _kw(case))
    _, emu = _grads(sd, x, g, _kw(case), stored=_Round.apply)
    net = _net(case, sd, cuda)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = net(x.to(cuda))
    assert out.dtype == torch.float32
    (out * g.to(cuda)).sum().backward()

    def l2(a, b):
        return (a - b).norm().item() / max(1e-12, b.norm().item())

    def mx(a, b):
        return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())

    bad = []
    for n, p in net.named_parameters():
        if not p.requires_grad:
            continue
        a, r, e = p.grad.detach().cpu().double(), ref[n], emu[n]
        if _edge_b0(n):
            assert (a.abs() <= _edge_b0_bound(sd, n, ref)).all(), n
            continue
        row = (n, l2(a, r), l2(e, r), mx(a, r), mx(e, r))
        print(f'{n}: gpu-vs-exact L2 {row[1]:.3e} (emulated {row[2]:.3e}), max {row[3]:.3e} (emulated {row[4]:.3e})')
        if row[1] > 1.3 * row[2] + 1e-2 or row[3] > 1.8 * row[4] + 2e-2:
            bad.append(row)
    assert not bad, bad


def _opt(amp, model_type='SRModel', **train):
    tr = dict(ema_decay=0.999, use_amp=amp, optim_g=dict(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99]),
              scheduler=dict(type='MultiStepLR', milestones=[100], gamma=0.5),
              pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean'))
    tr.update(train)
    return dict(model_type=model_type, is_train=True, dist=False, num_gpu=1, path={}, scale=4,
                network_g=dict(type='ECBSR', **CASES['A'][0]), train=tr)


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {'lq': torch.rand(2, 1, 7, 9, generator=g), 'gt': torch.rand(2, 1, 28, 36, generator=g)}


def _build(gold, amp, model_type='SRModel', **train):
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_opt(amp, model_type, **train))
    with torch.no_grad():  # the seeded state (visible edge branches, mixed-sign slopes), in place
        for k, v in model.get_bare_model(model.net_g).state_dict().items():
            v.copy_(torch.from_numpy(gold[f'A.sd.{k}']))
        if hasattr(model, 'net_g_ema'):
            model.model_ema(0)
    return model


def test_sr_model_ecbsr_fp32_steps_match_replay(cuda, gold):
    """SRModel + ECBSR (case A) with EMA, 3 fp32 steps against a float64 replay of the five-branch form with
    torch.optim.Adam and the EMA formula; tolerances of test_srrs_srcnn_fp32_steps_match_replay."""
    import basicsr4rs_amd.archs  # noqa: F401
    model = _build(gold, False)
    assert type(model).__name__ == 'SRModel'
    bare = model.get_bare_model(model.net_g)
    sd0 = {k: v.detach().cpu().clone() for k, v in bare.state_dict().items()}
    batch = _batch()
    got = []
    for it in (1, 2, 3):
        model.feed_data(batch)
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        got.append(float(model.get_current_log()['l_pix']))
    params = {k: (v.double().requires_grad_(True) if not k.endswith('.mask') else v.double()) for k, v in sd0.items()}
    ema = {k: v.double() for k, v in sd0.items()}
    train = [v for v in params.values() if v.requires_grad]
    opt = torch.optim.Adam(train, lr=1e-3, betas=(0.9, 0.99))
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = F.l1_loss(R.forward(params, batch['lq'].double(), **_kw('A')), batch['gt'].double())
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k in ema:
                if params[k].requires_grad:
                    ema[k].mul_(0.999).add_(params[k], alpha=0.001)
        losses.append(loss.item())
    print('SRModel + ECBSR fp32 losses', got, 'replay', losses)
    for a, b in zip(got, losses):
        assert abs(a - b) < 1e-5 * max(1.0, abs(b)), (got, losses)
    for k, v in bare.state_dict().items():
        err = (v.cpu().double() - params[k].detach()).abs().max().item() / max(1e-3, params[k].abs().max().item())
        assert err < 2e-4, (k, err)
    ema_sd = model.net_g_ema.state_dict()
    for k, v in ema_sd.items():
        err = (v.cpu().double() - ema[k]).abs().max().item() / max(1e-3, ema[k].abs().max().item())
        assert err < 2e-4, (k, err)
        if k.endswith('.mask'):
            assert torch.equal(v, bare.state_dict()[k]), k
    # validation runs through the EMA net's cached collapse
    model.feed_data(batch)
    model.test()
    assert tuple(model.output.shape) == (2, 1, 28, 36) and torch.isfinite(model.output).all()


def test_srrs_ecbsr_bf16_loss_decreases(cuda, gold):
    import basicsr4rs_amd.archs  # noqa: F401
    model = _build(gold, True, 'SRRSModel')
    assert type(model).__name__ == 'SRRSModel'
    batch = _batch()
    losses = []
    for it in range(1, 9):
        model.feed_data(batch)
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        losses.append(float(model.get_current_log()['l_pix']))
    print('SRRSModel + ECBSR bf16 losses', losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def _run_steps(gold, amp, steps=6, tmp=None, **train):
    model = _build(gold, amp, 'SRModel', scheduler=dict(type='MultiStepLR', milestones=[4], gamma=0.5), **train)
    losses = []
    for it in range(1, steps + 1):
        model.feed_data(_batch(it))
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        losses.append(float(model.get_current_log()['l_pix']))
    net = model.get_bare_model(model.net_g)
    return (model, losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in model.net_g_ema.state_dict().items()})


def _same(a, b):
    assert a[1] == b[1], (a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize('amp', [False, True])
def test_ecbsr_hip_graph_matches_eager(cuda, gold, amp):
    """Six steps with an lr milestone at 4: the captured step (collapse, convs, transpose and Adam inside the graph)
    gives bitwise the eager losses, parameters and EMA."""
    import basicsr4rs_amd.archs  # noqa: F401
    eager = _run_steps(gold, amp, cuda_graph=False)
    graph = _run_steps(gold, amp, cuda_graph=True)
    assert eager[0]._graph is None and graph[0]._graph is not None
    assert len(set(eager[1])) == 6
    _same(eager, graph)


def test_ecbsr_async_wgrad_modes_bitwise(cuda, gold):
    import basicsr4rs_amd.archs  # noqa: F401
    base = _run_steps(gold, False, steps=3, async_wgrad=False)
    for mode in (True, 'reduce'):
        _same(base, _run_steps(gold, False, steps=3, async_wgrad=mode))


def test_ecbsr_save_load_one_more_step_bitwise(cuda, gold, tmp_path):
    """Three steps, save the net, load it into a fresh model with the optimizer state, one more step: bitwise the
    fourth step of the uninterrupted run."""
    import basicsr4rs_amd.archs  # noqa: F401
    full = _run_steps(gold, False, steps=4)
    part = _run_steps(gold, False, steps=3)
    m = part[0]
    path = str(tmp_path / 'net_g.pth')
    torch.save({'params': m.get_bare_model(m.net_g).state_dict(), 'params_ema': m.net_g_ema.state_dict()}, path)
    state = m.get_training_state(0, 3)
    fresh = _build(gold, False, 'SRModel', scheduler=dict(type='MultiStepLR', milestones=[4], gamma=0.5))
    fresh.load_network(fresh.net_g, path, True, 'params')
    fresh.load_network(fresh.net_g_ema, path, True, 'params_ema')
    fresh.resume_training(state)
    fresh.feed_data(_batch(4))
    fresh.update_learning_rate(4)
    fresh.optimize_parameters(4)
    assert float(fresh.get_current_log()['l_pix']) == full[1][3]
    net = fresh.get_bare_model(fresh.net_g)
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), full[2][k]), k
    for k, v in fresh.net_g_ema.state_dict().items():
        assert torch.equal(v.cpu(), full[3][k]), k
