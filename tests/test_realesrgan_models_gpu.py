"""RealESRNetModel / RealESRGANModel on the device: built from the committed reference option files (tiny networks, a
temporary ``meta_info`` over tests/golden/baboon.png), fed by RealESRGANDataset.

Geometry: MSRResNet nf 8 with 1 block, net_d UNetDiscriminatorSN (3, 8), gt 400 -> gt_size 64, batch 2,
queue_size 4, so lq is [2, 3, 16, 16].  Overrides beyond those: ``pretrain_network_g`` removed and
``perceptual_opt.pretrained: false`` (no weight files in a checkout).  The numerics of every degradation step are
carried by tests/test_degrade_ops_gpu.py; the rounding stages make a float64 comparison of the whole pipeline
meaningless, so here: the contract of ``feed_data`` (shapes, the 8-bit grid, the pool, determinism, every branch),
the switches, and one step of each model."""
import os
import random

import numpy as np
import pytest
import torch

from ._fp64 import _bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'golden', 'reference_options', 'train', 'RealESRGAN')
NET_G = dict(type='MSRResNet', num_in_ch=3, num_out_ch=3, num_feat=8, num_block=1, upscale=4)
NET_D = dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=8, skip_connection=True)
LOG_KEYS_GAN = ['l_g_pix', 'l_g_percep', 'l_g_gan', 'l_d_real', 'out_d_real', 'l_d_fake', 'out_d_fake']


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _opt(yaml, tmp_path, **over):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.utils.options import parse_options
    opt, _ = parse_options(str(tmp_path), is_train=True, argv=['-opt', os.path.join(REF, yaml)])
    meta = tmp_path / 'meta_info.txt'
    meta.write_text('baboon.png\nbaboon.png\n')
    opt['datasets']['train'].update(dataroot_gt=os.path.join(HERE, 'golden'), meta_info=str(meta))
    opt.update(num_gpu=1, dist=False, network_g=dict(NET_G), gt_size=64, queue_size=4)
    if 'network_d' in opt:
        opt['network_d'] = dict(NET_D)
    opt['path']['pretrain_network_g'] = None
    if opt['train'].get('perceptual_opt'):
        opt['train']['perceptual_opt']['pretrained'] = False
    opt.update(over)
    return opt


def _build(yaml, tmp_path, seed=0, **over):
    from basicsr4rs_amd.data import build_dataset
    from basicsr4rs_amd.models import build_model
    opt = _opt(yaml, tmp_path, **over)
    _seed(seed)
    return build_model(opt), build_dataset(opt['datasets']['train'])


def _batch(ds, seed):
    """Two items of the dataset, collated; the host generators seeded so that the batch is reproducible."""
    random.seed(seed)
    np.random.seed(seed)
    items = [ds[0], ds[1]]
    return {k: (torch.stack([it[k] for it in items]) if torch.is_tensor(items[0][k]) else [it[k] for it in items])
            for k in items[0]}


GAN_YAML, NET_YAML = 'train_realesrgan_x4plus.yml', 'train_realesrnet_x4plus.yml'


@pytest.mark.parametrize('yaml', [GAN_YAML, NET_YAML])
def test_feed_data_contract_and_pool(tmp_path, yaml):
    from basicsr4rs_amd.utils.img_process_util import USMSharp
    model, ds = _build(yaml, tmp_path)
    gan = yaml == GAN_YAML
    assert type(model).__name__ == ('RealESRGANModel' if gan else 'RealESRNetModel') and model.queue_size == 4
    sharpen = USMSharp().to(model.device)
    fed = []
    for step in range(3):
        _seed(10 + step)
        model.feed_data(_batch(ds, 20 + step))
        lq, gt = model.lq, model.gt
        assert tuple(lq.shape) == (2, 3, 16, 16) and tuple(gt.shape) == (2, 3, 64, 64)
        assert lq.is_contiguous() and lq.dtype == torch.float32 and lq.min() >= 0 and lq.max() <= 1
        q = lq.double() * 255
        assert torch.equal((lq * 255.0), (lq * 255.0).round()) and (q - q.round()).abs().max() < 1e-4
        # the correctly rounded k / 255, formed on the host (a device division by a scalar multiplies by 1 / 255)
        assert torch.equal(_bits(lq.cpu()), _bits((lq * 255.0).round().cpu() / 255.0)), 'lq: the true quotient k / 255'
        if gan:
            assert torch.equal(_bits(model.gt_usm), _bits(sharpen(model.gt))), 'gt_usm = USMSharp(post-pool gt)'
        fed.append((lq.clone(), gt.clone()))
    # steps 1 and 2 filled the pool and returned their own batches: the pool holds them in order
    pool_lq, pool_gt = torch.cat([fed[0][0], fed[1][0]]), torch.cat([fed[0][1], fed[1][1]])
    assert model.queue_ptr == 4
    # step 3: a permutation of the pooled pairs came back, each lq with the gt it was enqueued with
    used = set()
    for i in range(2):
        match = [j for j in range(4) if torch.equal(fed[2][0][i], pool_lq[j]) and torch.equal(fed[2][1][i], pool_gt[j])]
        assert len(match) == 1, f'returned pair {i} is not a pooled pair'
        used.add(match[0])
    assert len(used) == 2
    with pytest.raises(AssertionError, match='divisible'):
        m2, _ = _build(yaml, tmp_path, queue_size=3)
        m2.feed_data(_batch(ds, 1))


def test_same_seeds_same_lq(tmp_path):
    out = []
    for _ in range(2):
        model, ds = _build(GAN_YAML, tmp_path, seed=3)
        _seed(42)
        model.feed_data(_batch(ds, 43))
        out.append((model.lq.clone(), model.gt.clone()))
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(out[0][1], out[1][1])


def _trace_calls(monkeypatch):
    """Names of the degradation ops in call order (the module-level functions the pipeline goes through)."""
    from basicsr4rs_amd.ops import degrade as D
    calls = []
    for name in ('filter2d', 'resize', 'gaussian_noise', 'poisson_noise', 'jpeg'):
        fn = getattr(D, name)

        def spy(*a, _fn=fn, _name=name, **kw):
            calls.append((_name, kw.get('mode'), kw.get('scale_factor', kw.get('size'))))
            return _fn(*a, **kw)

        monkeypatch.setattr(D, name, spy)
    return calls


def test_every_branch_reached(tmp_path, monkeypatch):
    model, ds = _build(NET_YAML, tmp_path)
    calls = _trace_calls(monkeypatch)

    def run(seed, **over):
        model.opt.update(over)
        del calls[:]
        _seed(seed)
        model.feed_data(_batch(ds, seed))
        assert tuple(model.lq.shape) == (2, 3, 16, 16)
        return list(calls)

    names = lambda c: [n for n, _, _ in c]  # noqa: E731
    # noise kind and the second blur, by their probabilities
    c = run(1, gaussian_noise_prob=1, gaussian_noise_prob2=1, second_blur_prob=1)
    assert names(c).count('gaussian_noise') == 2 and 'poisson_noise' not in names(c) and names(c).count('filter2d') == 3
    c = run(2, gaussian_noise_prob=0, gaussian_noise_prob2=0, second_blur_prob=0)
    assert names(c).count('poisson_noise') == 2 and 'gaussian_noise' not in names(c) and names(c).count('filter2d') == 2
    # up / down / keep of both resizes: the first by its scale factor, the second by its size around 400 / 4
    for prob, s1, s2 in (([1, 0, 0], lambda f: 1 < f <= 1.5, lambda h: 100 <= h <= 120),
                         ([0, 1, 0], lambda f: 0.15 <= f < 1, lambda h: 30 <= h <= 100), ([0, 0, 1], lambda f: f == 1,
                                                                                         lambda h: h == 100)):
        c = run(3, resize_prob=prob, resize_prob2=prob)
        geo = [g for n, _, g in c if n == 'resize']
        assert s1(geo[0]) and s2(geo[1][0]) and geo[1][0] == geo[1][1] and geo[2] == (100, 100), (prob, geo)
    # the three resize modes and both orders of [resize back + sinc] and JPEG, by the host seeds
    model.opt.update(resize_prob=[0.2, 0.7, 0.1], resize_prob2=[0.3, 0.4, 0.3])
    modes, last = set(), set()
    for seed in range(4, 16):
        c = run(seed)
        modes.update(m for n, m, _ in c if n == 'resize')
        last.add(names(c)[-1])
        assert names(c).count('resize') == 3 and names(c).count('jpeg') == 2
    assert modes == {'area', 'bilinear', 'bicubic'} and last == {'jpeg', 'filter2d'}, (modes, last)


@pytest.mark.parametrize('yaml', [GAN_YAML, NET_YAML])
def test_paired_path_and_validation(tmp_path, yaml):
    model, ds = _build(yaml, tmp_path, high_order_degradation=False)
    data = {'lq': torch.rand(2, 3, 16, 16), 'gt': torch.rand(2, 3, 64, 64)}
    model.feed_data(data)
    assert torch.equal(model.lq.cpu(), data['lq']) and torch.equal(model.gt.cpu(), data['gt'])
    assert tuple(model.gt_usm.shape) == (2, 3, 64, 64)
    # validation: is_train is off while it runs and on afterwards; the batch passes through
    model, ds = _build(yaml, tmp_path)
    model.opt['val'] = {}
    seen = []
    feed = model.feed_data

    def spy(d):
        feed(d)
        seen.append((model.is_train, torch.equal(model.lq.cpu(), d['lq'])))

    model.feed_data = spy

    class Loader(list):
        dataset = type('D', (), {'opt': {'name': 'v'}})

    val = {'lq': torch.rand(1, 3, 16, 16), 'gt': torch.rand(1, 3, 64, 64), 'lq_path': ['a.png']}
    model.nondist_validation(Loader([val]), 0, None, False)
    assert seen == [(False, True)] and model.is_train is True


def test_gt_usm_switches(tmp_path, monkeypatch):
    from basicsr4rs_amd.models.srgan_model import SRGANModel
    model, ds = _build(GAN_YAML, tmp_path)
    _seed(5)
    model.feed_data(_batch(ds, 5))
    got = {}
    g_terms, d_terms = SRGANModel._g_content_terms, SRGANModel._d_terms

    def g_spy(self, loss_dict, pix_gt=None, percep_gt=None):
        got.update(pix=pix_gt, percep=percep_gt)
        return g_terms(self, loss_dict, pix_gt=pix_gt, percep_gt=percep_gt)

    def d_spy(self, loss_dict, real=None):
        got.update(real=real)
        return d_terms(self, loss_dict, real=real)

    monkeypatch.setattr(SRGANModel, '_g_content_terms', g_spy)
    monkeypatch.setattr(SRGANModel, '_d_terms', d_spy)
    assert model.gt_usm is not model.gt and not torch.equal(model.gt_usm, model.gt)
    # the option file: l1 and perceptual against the sharpened ground truth, the discriminator sees the plain one
    model.optimize_parameters(1)
    assert got['pix'] is model.gt_usm and got['percep'] is model.gt_usm and got['real'] is model.gt
    log = model.get_current_log()
    assert list(log) == LOG_KEYS_GAN, list(log)
    assert all(np.isfinite(v) for v in log.values()), log
    for flags in ((False, True, True), (True, False, False), (False, False, True)):
        model.opt.update(l1_gt_usm=flags[0], percep_gt_usm=flags[1], gan_gt_usm=flags[2])
        model.optimize_parameters(2)
        want = [model.gt_usm if f else model.gt for f in flags]
        assert got['pix'] is want[0] and got['percep'] is want[1] and got['real'] is want[2], flags


@pytest.mark.parametrize('gt_usm', [True, False])
def test_realesrnet_step(tmp_path, gt_usm):
    from basicsr4rs_amd.utils.img_process_util import USMSharp
    model, ds = _build(NET_YAML, tmp_path, gt_usm=gt_usm)
    batch = _batch(ds, 7)
    _seed(7)
    model.feed_data(batch)
    # gt[0] is a 64 x 64 window of the (sharpened) ground truth of sample 0: candidates from its first row
    full = batch['gt'].to(model.device)
    full = USMSharp().to(model.device)(full) if gt_usm else full
    rows = full[0, 0].unfold(1, 64, 1)  # [400, 337, 64]
    cand = (rows == model.gt[0, 0, 0]).all(-1).nonzero().tolist()
    assert any(y + 64 <= 400 and torch.equal(full[0, :, y:y + 64, x:x + 64], model.gt[0]) for y, x in cand), \
        'gt[0] is not a crop of the expected ground truth'
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert list(log) == ['l_pix'] and np.isfinite(log['l_pix']), log
