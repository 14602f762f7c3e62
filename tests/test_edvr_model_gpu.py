"""EDVRModel on the GPU: eager train steps on a small 64-feature config with CharbonnierLoss, the ``tsa_iter``
freeze / release with the optimizer semantics of ``torch.optim.Adam``, the ``dcn_lr_mul`` grouping, and the refusals.

Optimizer semantics, separated from kernel error: the flat gradient of each of five steps (``tsa_iter = 3``) is
recorded and the steps are replayed on the CPU with ``torch.optim.Adam`` on those gradients, ``None`` for the frozen
parameters in steps 1 and 2 -- in float64, as the plumbing test of tests/test_fused_adam_gpu.py does, whose bound is
used unchanged: |p - p_ref| <= 1e-4 sum_k |D_ref,k| + t U max_k |p_ref,k| (the update good to 1e-4 of its size, the
stored parameter rounded once per step).  An optimizer with one global step counter applies step-3 bias corrections
to the released parameters' first update (a factor 0.1 / 0.271 on it) and reports step 5 for them: both checks fail.
The steps run with ``train.use_amp`` (bf16: the fused DCN kernels, whose fixed-point scatter is order-independent),
so two models from one seed end with identical bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0**-24
NET = dict(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=3, deformable_groups=8, num_extract_block=1,
           num_reconstruct_block=1, center_frame_idx=None, hr_in=False, with_predeblur=False, with_tsa=True)
LR, BETAS = 4e-4, (0.9, 0.99)


def _opt(tmp_path, **train):
    t = dict(ema_decay=0.999, use_amp=True, optim_g=dict(type='Adam', lr=LR, weight_decay=0, betas=list(BETAS)),
             scheduler=dict(type='CosineAnnealingRestartLR', periods=[100], restart_weights=[1], eta_min=1e-7),
             pixel_opt=dict(type='CharbonnierLoss', loss_weight=1.0, reduction='sum'), dcn_lr_mul=1)
    t.update(train)
    return dict(model_type='EDVRModel', name='edvr', is_train=True, dist=False, num_gpu=1, scale=4, network_g=dict(NET),
                path={'experiments_root': str(tmp_path / 'exp'), 'visualization': str(tmp_path / 'vis')}, train=t)


def _model(opt):
    """The model with small random ``conv_offset`` weights (std 0.01) in place of the zero init: behind a zero
    ``conv_offset`` the offset convs of PCD get an exactly zero gradient in their first trained step and would not
    move in it."""
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    from basicsr4rs_amd.ops.conv import bump_param_epoch
    torch.manual_seed(0)
    model = build_model(opt)
    assert type(model).__name__ == 'EDVRModel'
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, p in model.net_g.named_parameters():
            if 'conv_offset' in k:
                p.copy_((torch.randn(p.shape, generator=g) * 0.01).cuda())
        model.flat_ema.flat.copy_(model.flat_g.flat)
    bump_param_epoch()
    return model


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {'lq': torch.rand(2, 3, 3, 16, 16, generator=g), 'gt': torch.rand(2, 3, 64, 64, generator=g)}


def _params(model):
    return {k: v.detach().clone() for k, v in model.net_g.named_parameters()}


def _moved(before, after):
    return {k for k in before if not torch.equal(before[k], after[k])}


def test_two_eager_steps(tmp_path):
    from basicsr4rs_amd.utils.flat import FusedAdam, RangedFusedAdam
    models = [_model(_opt(tmp_path)) for _ in range(2)]
    m = models[0]
    assert isinstance(m.optimizer_g, FusedAdam) and not isinstance(m.optimizer_g, RangedFusedAdam)
    p0, ema0 = _params(m), m.flat_ema.flat.clone()
    assert torch.equal(ema0, m.flat_g.flat)
    losses = []
    for it in (1, 2):
        for mm in models:
            mm.feed_data(_batch(7))  # the same batch twice: the second loss is after one update on it
            assert mm.lq.dim() == 5
            mm.optimize_parameters(it)
        losses.append(m.get_current_log()['l_pix'])
        models[1].get_current_log()
    print(f'EDVRModel l_pix: {losses[0]:.4f} -> {losses[1]:.4f}')
    assert all(torch.isfinite(torch.tensor(v)) for v in losses) and losses[1] < losses[0]
    assert _moved(p0, _params(m)) == set(p0), 'every parameter moves'
    # the EMA follows: two steps of ema = 0.999 ema + 0.001 p from ema = p0 stay within 0.002 |p - p0| of p0
    d_ema, d_p = (m.flat_ema.flat - ema0).abs(), (m.flat_g.flat - ema0).abs().max()
    assert d_ema.max() > 0 and d_ema.max() <= 0.0021 * d_p
    assert torch.equal(m.flat_g.flat, models[1].flat_g.flat), 'two models from one seed differ after the same steps'
    assert torch.equal(m.flat_ema.flat, models[1].flat_ema.flat)
    assert m.output.shape == (2, 3, 64, 64)
    m.test()
    assert m.output.shape == (2, 3, 64, 64) and torch.isfinite(m.output).all()


def test_tsa_iter_matches_torch_adam(tmp_path):
    from basicsr4rs_amd.utils.flat import RangedFusedAdam
    m = _model(_opt(tmp_path, tsa_iter=3))
    assert isinstance(m.optimizer_g, RangedFusedAdam)
    names = [k for k, _ in m.net_g.named_parameters()]
    fusion = {k for k in names if 'fusion' in k}
    assert fusion and len(m.optimizer_g.ranges) == 3
    flat = m.flat_g
    p0 = flat.flat.detach().cpu().double()
    ref = [p0[flat.offsets[i]:flat.offsets[i + 1]].view_as(p).clone().requires_grad_(True)
           for i, p in enumerate(flat.params)]
    ropt = torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=1e-8)
    ema_ref = p0.clone()
    moved, pmax = torch.zeros_like(p0), torch.zeros_like(p0)
    for it in range(1, 6):
        before = _params(m)
        m.feed_data(_batch(it))
        m.optimize_parameters(it)
        assert torch.isfinite(torch.tensor(m.get_current_log()['l_pix']))
        changed = _moved(before, _params(m))
        if it < 3:
            assert changed == fusion, (it, 'frozen parameters must keep their bits while fusion.* moves',
                                       sorted(changed ^ fusion)[:4])
            assert not flat.grad[:flat.offsets[names.index(sorted(fusion, key=names.index)[0])]].any()
        else:
            assert changed == set(names), (it, sorted(set(names) - changed)[:4])
        # replay on the recorded gradients
        grad = flat.grad.detach().cpu().double()
        for i, (k, r) in enumerate(zip(names, ref)):
            frozen = it < 3 and k not in fusion
            r.grad = None if frozen else grad[flat.offsets[i]:flat.offsets[i + 1]].view_as(r).clone()
        prev = torch.cat([r.detach().reshape(-1) for r in ref]).clone()
        ropt.param_groups[0]['lr'] = m.optimizer_g.param_groups[0]['lr']
        ropt.step()
        p_ref = torch.cat([r.detach().reshape(-1) for r in ref])
        ema_ref = 0.999 * ema_ref + 0.001 * p_ref
        moved += (p_ref - prev).abs()
        pmax = torch.maximum(pmax, p_ref.abs())
        m.update_learning_rate(it + 1)
    bound = 1e-4 * moved + 5 * U * pmax
    err = (flat.flat.detach().cpu().double() - p_ref).abs()
    print(f'tsa_iter replay: p max|err| {err.max().item():.3e}, max err/bound '
          f'{(err / bound.clamp(min=1e-300)).max().item():.3f}')
    assert (err <= bound).all()
    emax = pmax + ema_ref.abs()
    e_err = (m.flat_ema.flat.detach().cpu().double() - ema_ref).abs()
    assert (e_err <= bound + 15 * U * emax).all(), 'the EMA follows all parameters, frozen ones included'
    state, rstate = m.optimizer_g.state_dict()['state'], ropt.state_dict()['state']
    for i, k in enumerate(names):
        want = 5 if k in fusion else 3
        assert float(rstate[i]['step']) == want
        assert float(state[i]['step']) == want, (k, float(state[i]['step']))
        assert tuple(state[i]['exp_avg'].shape) == tuple(flat.params[i].shape)
    # the state round-trips through torch.optim.Adam's layout
    sd = m.optimizer_g.state_dict()
    m.optimizer_g.load_state_dict(sd)
    assert m.optimizer_g.range_steps == [3, 5, 3]


def test_dcn_lr_mul_grouping(tmp_path):
    from basicsr4rs_amd.utils.flat import FusedAdam
    m = _model(_opt(tmp_path, dcn_lr_mul=2))
    opt = m.optimizer_g
    assert type(opt) is torch.optim.Adam and not isinstance(opt, FusedAdam)
    named = dict(m.net_g.named_parameters())
    dcn = [p for k, p in named.items() if 'dcn' in k]
    normal = [p for k, p in named.items() if 'dcn' not in k]
    assert len(opt.param_groups) == 2 and dcn and normal
    assert [id(p) for p in opt.param_groups[0]['params']] == [id(p) for p in normal]
    assert [id(p) for p in opt.param_groups[1]['params']] == [id(p) for p in dcn]
    assert opt.param_groups[0]['lr'] == LR and opt.param_groups[1]['lr'] == 2 * LR
    before = _params(m)
    m.feed_data(_batch(3))
    m.optimize_parameters(1)
    assert _moved(before, _params(m)) == set(before)
    assert not torch.equal(m.flat_ema.flat, m.flat_g.flat)


def test_refusals(tmp_path):
    with pytest.raises(NotImplementedError, match='cuda_graph'):
        _model(_opt(tmp_path, cuda_graph=True))
    m = _model(_opt(tmp_path))
    with pytest.raises(NotImplementedError, match='VideoTestDataset'):
        m.validation(None, 1, None)
