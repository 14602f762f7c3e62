"""SRGANModel / ESRGANModel with ``network_d.type: UNetDiscriminatorSN`` against a float64 replay in stock torch.

Generator MSRResNet (nf 8, 1 block, oracle/nets.py), discriminator (3, 8) (tests/_unet_ref.py: torch's
spectral_norm and F.interpolate), gt 32 x 32, batch 2, L1 + vanilla GAN, no perceptual loss.  The step order is the
reference's optimize_parameters (basicsr/models/srgan_model.py:85-141, esrgan_model.py:12-83), written out below.
Rules of tests/test_gan_models_gpu.py: a logged value within 1e-5 * max(1, |ref|); the gradients of both nets per
tensor within 8 x the rel-L2 error of the same replay run in fp32 on the CPU; weight_u / weight_v after the step
against the replay's (its 3rd iterate for SRGAN, 5th for ESRGAN: net_d runs that often per step, always in training
mode) under the same 8 x rule."""
import os
from collections import OrderedDict

import pytest
import torch

from oracle import nets as O

from . import _unet_ref as R

pytestmark = pytest.mark.gpu

NET_G = dict(type='MSRResNet', num_in_ch=3, num_out_ch=3, num_feat=8, num_block=1, upscale=4)
NET_D = dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=8, skip_connection=True)
LR, BETAS, EMA, EPS = 1e-4, (0.9, 0.99), 0.999, 1e-8
W_PIX, W_GAN = 1e-2, 5e-3
# The data seed of the gradient comparison: the first of 1, 2, ... for which the fp32 CPU replay itself stays at the
# 1e-5 level (no LeakyReLU gate within fp32 rounding of zero); chosen from the replay alone, before the engine runs
# (_pick_seed prints the levels; seed 1 serves both models).  One tensor is left out of that criterion, though not of
# the comparison: conv9.bias of net_d.  Its gradient is the plain sum of the gradients of all logits of both
# discriminator backwards, and in the relativistic (ESRGAN) step those cancel to 1e-3 of their size (norm 1.4e-5
# against 2e-2 for conv9.weight), so any fp32 evaluation is 2e-4 .. 2e-2 off relative to the remainder on every seed.
SEEDS = (1, 2, 3, 4, 5, 6)
CANCELLING = ('d.conv9.bias', )


def _opt(model_type):
    t = dict(ema_decay=EMA, optim_g=dict(type='Adam', lr=LR, weight_decay=0, betas=list(BETAS), eps=EPS),
             optim_d=dict(type='Adam', lr=LR, weight_decay=0, betas=list(BETAS), eps=EPS),
             scheduler=dict(type='MultiStepLR', milestones=[100], gamma=0.5),
             pixel_opt=dict(type='L1Loss', loss_weight=W_PIX, reduction='mean'),
             gan_opt=dict(type='GANLoss', gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0, loss_weight=W_GAN),
             net_d_iters=1, net_d_init_iters=0)
    return dict(model_type=model_type, is_train=True, dist=False, num_gpu=1, path={}, network_g=dict(NET_G),
                network_d=dict(NET_D), train=t)


def _build(model_type, seed=0):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(seed)
    return build_model(_opt(model_type))


def _data(it):
    g = torch.Generator().manual_seed(100 + it)
    return {'lq': torch.rand(2, 3, 8, 8, generator=g), 'gt': torch.rand(2, 3, 32, 32, generator=g)}


def _gan(x, real, disc):
    loss = torch.nn.BCEWithLogitsLoss()(x, torch.full_like(x, 1.0 if real else 0.0))
    return loss if disc else loss * W_GAN


class _Replay:
    """The stock-torch twin of a freshly built model in ``dtype``: same initial weights and buffers."""

    def __init__(self, g_sd, d_sd, model_type, dtype):
        self.kind, self.dtype = model_type, dtype
        self.pg = OrderedDict((k, v.detach().cpu().to(dtype).clone().requires_grad_(True)) for k, v in g_sd.items())
        self.d = R.stock_like(d_sd, 3, 8, dtype).train()

    def step(self, data):
        lq, gt = data['lq'].to(self.dtype), data['gt'].to(self.dtype)
        log = OrderedDict()
        for p in self.d.parameters():
            p.requires_grad = False
        out = O.msrresnet(self.pg, lq, num_block=1, upscale=4)
        l_pix = W_PIX * (out - gt).abs().mean()
        if self.kind == 'SRGANModel':
            l_gan = _gan(self.d(out), True, False)
        else:
            real_d_pred = self.d(gt).detach()
            fake_g_pred = self.d(out)
            l_gan = (_gan(real_d_pred - fake_g_pred.mean(), False, False) +
                     _gan(fake_g_pred - real_d_pred.mean(), True, False)) / 2
        log['l_g_pix'], log['l_g_gan'] = l_pix, l_gan
        (l_pix + l_gan).backward()
        for p in self.d.parameters():
            p.requires_grad = True
            p.grad = None
        if self.kind == 'SRGANModel':
            real = self.d(gt)
            l_real = _gan(real, True, True)
            l_real.backward()
            fake = self.d(out.detach())
            l_fake = _gan(fake, False, True)
            l_fake.backward()
        else:
            fake0 = self.d(out.detach()).detach()
            real = self.d(gt)
            l_real = _gan(real - fake0.mean(), True, True) * 0.5
            l_real.backward()
            fake = self.d(out.detach())
            l_fake = _gan(fake - real.detach().mean(), False, True) * 0.5
            l_fake.backward()
        log['l_d_real'], log['l_d_fake'] = l_real, l_fake
        log['out_d_real'], log['out_d_fake'] = real.detach().mean(), fake.detach().mean()
        self.grads = {'g.' + k: v.grad for k, v in self.pg.items()}
        self.grads.update({'d.' + k: p.grad for k, p in self.d.named_parameters()})
        self.bufs = {k: b.detach().clone() for k, b in self.d.named_buffers()}
        return OrderedDict((k, v.item()) for k, v in log.items())


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _pick_seed(g_sd, d_sd, model_type):
    """(seed, float64 replay, fp32 replay's per-tensor errors) of the first data seed whose fp32 replay stays at
    the 1e-5 level on every gradient tensor."""
    for seed in SEEDS:
        r64, r32 = _Replay(g_sd, d_sd, model_type, torch.float64), _Replay(g_sd, d_sd, model_type, torch.float32)
        log = r64.step(_data(seed))
        r32.step(_data(seed))
        errs = {k: _l2(r32.grads[k], v) for k, v in r64.grads.items()}
        berrs = {k: _l2(r32.bufs[k], v) for k, v in r64.bufs.items()}
        level = max(e for k, e in errs.items() if k not in CANCELLING)
        print(f'{model_type} data seed {seed}: fp32 replay gradient error max {level:.3e}; ' +
              ', '.join(f'{k} {errs[k]:.3e}' for k in CANCELLING))
        if level < 5e-5:
            return seed, r64, log, errs, berrs
    raise AssertionError('no data seed with an fp32 replay at the 1e-5 level')


@pytest.mark.parametrize('model_type', ['SRGANModel', 'ESRGANModel'])
def test_one_step_matches_float64_replay(cuda, model_type):
    model = _build(model_type)
    assert type(model.net_d).__name__ == 'UNetDiscriminatorSN'
    names = [k for k, _ in model.net_d.named_parameters()]
    assert len(model.flat_d.params) == 12 and sum(k.endswith('weight_orig') for k in names) == 8
    g_sd = {k: v.detach().cpu().clone() for k, v in model.get_bare_model(model.net_g).state_dict().items()}
    d_sd = {k: v.detach().cpu().clone() for k, v in model.net_d.state_dict().items()}
    seed, rep, ref_log, errs, berrs = _pick_seed(g_sd, d_sd, model_type)
    print(f'{model_type}: data seed {seed}')
    model.feed_data(_data(seed))
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) == set(ref_log), (list(log), list(ref_log))
    bad = []
    for k, r in ref_log.items():
        err, allowed = abs(log[k] - r), 1e-5 * max(1.0, abs(r))
        print(f'{model_type} {k}: got {log[k]:.8g} ref {r:.8g} err {err:.2e} (allowed {allowed:.2e})')
        if not err < allowed:
            bad.append(k)
    got = {'g.' + k: p.grad for k, p in model.get_bare_model(model.net_g).named_parameters()}
    got.update({'d.' + k: p.grad for k, p in model.net_d.named_parameters()})
    assert set(got) == set(rep.grads)
    for k, r in rep.grads.items():
        err, bound = _l2(got[k].cpu(), r), 8 * errs[k]
        print(f'{model_type} grad {k}: rel-L2 {err:.3e}, bound {bound:.3e}, ratio {err / max(bound, 1e-300):.3f}')
        if not err <= bound:
            bad.append((k, err, bound))
    calls = 3 if model_type == 'SRGANModel' else 5
    start = {k: v for k, v in d_sd.items() if k.endswith(('weight_u', 'weight_v'))}
    for k, b in model.net_d.named_buffers():
        err, bound = _l2(b.cpu(), rep.bufs[k]), 8 * berrs[k]
        print(f'{model_type} {k} after {calls} forwards: rel-L2 {err:.3e}, bound {bound:.3e}; the start is '
              f'{_l2(start[k], rep.bufs[k]):.3e} away')
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    assert all(p.requires_grad for p in model.net_d.parameters())


def _state(model):
    return ([model.flat_g.flat.clone(), model.flat_d.flat.clone(), model.flat_ema.flat.clone()] +
            [b.clone() for b in model.net_d.buffers()])


@pytest.mark.parametrize('model_type', ['SRGANModel', 'ESRGANModel'])
def test_save_rebuild_resume_is_bitwise(cuda, tmp_path, model_type):
    """Two steps, save, two more; a rebuilt model that loads the checkpoint (net_g with params_ema, net_d with its
    weight_u / weight_v, the training state with both optimizers) and runs the same two steps ends on the same bits."""
    from basicsr4rs_amd.models import build_model
    paths = dict(models=str(tmp_path / 'models'), training_states=str(tmp_path / 'states'))
    os.makedirs(paths['models'])
    os.makedirs(paths['training_states'])
    model = _build(model_type)
    model.opt['path'].update(paths)
    for it in (1, 2):
        model.feed_data(_data(it))
        model.optimize_parameters(it)
    model.save(0, 2)
    ck = torch.load(tmp_path / 'models/net_d_2.pth', weights_only=True)['params']
    assert 'conv1.weight_orig' in ck and 'conv8.weight_u' in ck and 'conv8.weight_v' in ck and 'conv1.weight' not in ck
    R.StockUNetSN(3, 8).load_state_dict(ck, strict=True)  # a checkpoint the reference's module loads strictly
    state = torch.load(tmp_path / 'states/2.state', weights_only=True)
    for it in (3, 4):
        model.feed_data(_data(it))
        model.optimize_parameters(it)
    want = _state(model)
    opt = _opt(model_type)
    opt['path'] = dict(paths, pretrain_network_g=str(tmp_path / 'models/net_g_2.pth'),
                       pretrain_network_d=str(tmp_path / 'models/net_d_2.pth'))
    torch.manual_seed(123)  # another init: everything must come from the checkpoint
    again = build_model(opt)
    again.resume_training(state)
    for it in (3, 4):
        again.feed_data(_data(it))
        again.optimize_parameters(it)
    for a, b in zip(want, _state(again)):
        assert torch.equal(a, b)
