"""SRCNN on the HIP engine against torch on the CPU: fp32 parity of the output and all six gradients
(float64 replay), the bf16 autocast gradients against a float64 emulation of the engine's bf16
storage points, SRRSModel train steps (fp32 against torch.optim.Adam + the EMA formula, bf16 loss),
and the captured / side-stream step variants bitwise against the eager synchronous step."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

NET4 = dict(type='SRCNN', num_in_ch=4, num_out_ch=4, upscale=4)
NET6 = dict(type='SRCNN', num_in_ch=6, num_out_ch=6, upscale=3)


class _Round(torch.autograd.Function):
    """A map stored in bf16: the value is rounded going forward, its gradient going backward."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _srcnn(sd, x, scale, stored=lambda t: t):
    """The reference forward restated with torch functionals; ``stored`` wraps every map the engine
    keeps in the feature dtype (the upsampled input, both hidden activations, the output)."""
    h = stored(F.interpolate(x, scale_factor=scale, mode='bicubic', align_corners=True))
    h = stored(F.relu(F.conv2d(h, sd['conv1.weight'], sd['conv1.bias'], padding=4)))
    h = stored(F.relu(F.conv2d(h, sd['conv2.weight'], sd['conv2.bias'], padding=2)))
    return stored(F.conv2d(h, sd['conv3.weight'], sd['conv3.bias'], padding=2))


def _grads(sd, x, scale, g, stored=lambda t: t):
    sdg = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    out = _srcnn(sdg, x.double(), scale, stored)
    (out * g).sum().backward()
    return out.detach(), {k: v.grad for k, v in sdg.items()}


@pytest.mark.parametrize('cfg,shape', [(NET4, (2, 4, 12, 12)), (NET6, (2, 6, 7, 9))], ids=('4band_x4', '6band_x3'))
def test_srcnn_parity_fp32(cuda, cfg, shape):
    from basicsr4rs_amd.archs import build_network
    torch.manual_seed(0)
    net = build_network(dict(cfg))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(1)) * 2 - 1
    s = cfg['upscale']
    g = torch.randn(shape[0], cfg['num_out_ch'], shape[2] * s, shape[3] * s, generator=torch.Generator().manual_seed(2),
                    dtype=torch.float64)
    ref_out, ref = _grads(sd, x, s, g)
    gn = net.to(cuda)
    out = gn(x.to(cuda))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref_out.shape)
    (out * g.float().to(cuda)).sum().backward()
    err = (out.detach().cpu().double() - ref_out).abs().max().item()
    print(f'SRCNN fp32 {shape}: output max-abs {err:.3e}')
    assert err < 1e-3
    for n, p in gn.named_parameters():
        e = (p.grad.detach().cpu().double() - ref[n]).abs().max().item()
        print(f'  {n}: grad max-abs {e:.3e} (max |ref| {ref[n].abs().max().item():.3e})')
        assert e < 1e-3, (n, e)


@pytest.mark.parametrize('cfg,shape', [(NET4, (2, 4, 12, 12)), (NET6, (2, 6, 7, 9))], ids=('4band_x4', '6band_x3'))
def test_srcnn_grad_error_is_bf16_storage_rounding(cuda, cfg, shape):
    """bf16 autocast: each gradient's error against the exact float64 replay is that of the same
    replay with every stored map (upsampled input, hidden activations, output, and their gradients)
    rounded to bf16: relative L2 <= 1.3 x the emulation's + 1e-2, max error <= 1.8 x + 2e-2 (the
    ratios of test_swinir_grad_error_is_bf16_storage_rounding).  Weights are pre-rounded to bf16."""
    from basicsr4rs_amd.archs import build_network
    torch.manual_seed(0)
    net = build_network(dict(cfg))
    sd = {k: v.detach().to(torch.bfloat16).float() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(1)) * 2 - 1
    s = cfg['upscale']
    g = torch.randn(shape[0], cfg['num_out_ch'], shape[2] * s, shape[3] * s, generator=torch.Generator().manual_seed(2),
                    dtype=torch.float64)
    _, ref = _grads(sd, x, s, g)
    _, emu = _grads(sd, x, s, g, stored=_Round.apply)
    gn = net.to(cuda)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = gn(x.to(cuda))
    (out.float() * g.float().to(cuda)).sum().backward()

    def l2(a, b):
        return (a - b).norm().item() / max(1e-12, b.norm().item())

    def mx(a, b):
        return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())

    bad = []
    for n, p in gn.named_parameters():
        a, r, e = p.grad.detach().cpu().double(), ref[n], emu[n]
        row = (n, l2(a, r), l2(e, r), mx(a, r), mx(e, r))
        print(f'{n}: gpu-vs-exact L2 {row[1]:.3e} (emulated {row[2]:.3e}), max {row[3]:.3e} (emulated {row[4]:.3e})')
        if row[1] > 1.3 * row[2] + 1e-2 or row[3] > 1.8 * row[4] + 2e-2:
            bad.append(row)
    assert not bad, bad


def _opt(amp, model_type='SRRSModel', **train):
    tr = dict(ema_decay=0.999, use_amp=amp, optim_g=dict(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99]),
              scheduler=dict(type='MultiStepLR', milestones=[100], gamma=0.5),
              pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean'))
    tr.update(train)
    return dict(model_type=model_type, is_train=True, dist=False, num_gpu=1, path={}, network_g=dict(NET4), scale=4,
                train=tr)


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {'lq': torch.rand(2, 4, 12, 12, generator=g) * 2 - 1, 'gt': torch.rand(2, 4, 48, 48, generator=g) * 2 - 1}


def _replay(sd0, batch, steps):
    # float64 throughout: the replay's own rounding stays out of the comparison
    params = {k: v.double().requires_grad_(True) for k, v in sd0.items()}
    ema = {k: v.double() for k, v in sd0.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-3, betas=(0.9, 0.99))
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.l1_loss(_srcnn(params, batch['lq'].double(), 4), batch['gt'].double())
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k in ema:
                ema[k].mul_(0.999).add_(params[k], alpha=0.001)
        losses.append(loss.item())
    return params, ema, losses


def test_srrs_srcnn_fp32_steps_match_replay(cuda):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_opt(False))
    assert type(model).__name__ == 'SRRSModel'
    bare = model.get_bare_model(model.net_g)
    sd0 = {k: v.detach().cpu().clone() for k, v in bare.state_dict().items()}
    batch = _batch()
    got = []
    for it in (1, 2):
        model.feed_data(batch)
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        got.append(model.get_current_log()['l_pix'])
    params, ema, losses = _replay(sd0, batch, 2)
    print('SRRSModel + SRCNN fp32 losses', got, 'replay', losses)
    for a, b in zip(got, losses):
        assert abs(a - b) < 1e-5 * max(1.0, abs(b)), (got, losses)
    for k, v in bare.state_dict().items():
        err = (v.cpu().double() - params[k].detach()).abs().max().item() / max(1e-3, params[k].abs().max().item())
        print(f'  {k}: parameter error / max {err:.3e}')
        assert err < 2e-4, (k, err)
    for k, v in model.net_g_ema.state_dict().items():
        err = (v.cpu().double() - ema[k]).abs().max().item() / max(1e-3, ema[k].abs().max().item())
        assert err < 2e-4, (k, err)


def test_srrs_srcnn_bf16_step_loss(cuda):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_opt(True))
    bare = model.get_bare_model(model.net_g)
    sd0 = {k: v.detach().cpu().clone() for k, v in bare.state_dict().items()}
    batch = _batch()
    model.feed_data(batch)
    model.update_learning_rate(1)
    model.optimize_parameters(1)
    loss = model.get_current_log()['l_pix']
    _, _, losses = _replay(sd0, batch, 1)
    print(f'SRRSModel + SRCNN bf16 loss {loss:.6f} vs fp32 replay {losses[0]:.6f}')
    assert abs(loss - losses[0]) < 1e-2 * abs(losses[0])
    assert any(not torch.equal(v.cpu(), sd0[k]) for k, v in bare.state_dict().items())


def _run_steps(amp, model_type='SRRSModel', **train):
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_opt(amp, model_type, scheduler=dict(type='MultiStepLR', milestones=[4], gamma=0.5), **train))
    losses = []
    for it in range(1, 7):
        model.feed_data(_batch(it))
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        losses.append(model.get_current_log()['l_pix'])
    net = model.get_bare_model(model.net_g)
    return (model, losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in model.net_g_ema.state_dict().items()})


def _same(a, b):
    assert a[1] == b[1], (a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize('amp', [False, True])
def test_srcnn_hip_graph_matches_eager(cuda, amp):
    """Six steps with an lr milestone at 4: the captured step (weight images refreshed inside the graph)
    gives bitwise the eager losses, parameters and EMA.  On SRModel, as
    test_sr_model_hip_graph_matches_eager: SRRSModel reads its loss on the host every step (the
    reference's non-finite check) and therefore never captures."""
    import basicsr4rs_amd.archs  # noqa: F401
    eager = _run_steps(amp, 'SRModel', cuda_graph=False)
    graph = _run_steps(amp, 'SRModel', cuda_graph=True)
    assert eager[0]._graph is None and graph[0]._graph is not None
    assert len(set(eager[1])) == 6  # the steps do move the loss
    _same(eager, graph)


def test_srcnn_async_wgrad_modes_bitwise(cuda):
    import basicsr4rs_amd.archs  # noqa: F401
    base = _run_steps(True, async_wgrad=False)
    for mode in (True, 'reduce'):
        _same(base, _run_steps(True, async_wgrad=mode))
