"""EDVR on the host: ``build_network`` for the ``network_g`` settings of the reference's four
options/train/EDVR/train_EDVR_{M,L}_x4_SR_REDS{,_woTSA}.yml files (written here as dicts; the two EDVR-L files also
carry a stray ``ema_decay`` key under ``network_g``, which the reference's constructor refuses as well and is left
out), state_dict names and shapes against tests/golden/edvr_state_keys.json, the parameter count against the stock
tree's, and a strict load of a reference-format checkpoint.  ``EDVRModel`` needs the device (flat parameters live
there): its optimizer grouping is checked in tests/test_edvr_model_gpu.py."""
import json
import os

import pytest
import torch

from . import _edvr_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edvr_state_keys.json')


def _net_opt(num_feat, blocks, with_tsa):
    return dict(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=num_feat, num_frame=5, deformable_groups=8,
                num_extract_block=5, num_reconstruct_block=blocks, center_frame_idx=None, hr_in=False,
                with_predeblur=False, with_tsa=with_tsa)


OPTION_FILES = {
    'train_EDVR_M_x4_SR_REDS': _net_opt(64, 10, True),
    'train_EDVR_M_x4_SR_REDS_woTSA': _net_opt(64, 10, False),
    'train_EDVR_L_x4_SR_REDS': _net_opt(128, 40, True),
    'train_EDVR_L_x4_SR_REDS_woTSA': _net_opt(128, 40, False),
}


def _scaled(golden, num_feat, blocks):
    """The golden EDVR-M table by the same rule at ``num_feat`` features and ``blocks`` reconstruction blocks: every
    64 that is a feature count becomes num_feat (the HR tail keeps its 64: upconv2's 256 outputs, conv_hr,
    conv_last), and reconstruction.{i} repeats."""
    out = {}

    def dims(key, shape):
        if key.startswith(('conv_hr', 'conv_last')):
            return shape
        if key.startswith('upconv2'):
            return [shape[0]] + [num_feat * (d // 64) if i == 1 else d for i, d in enumerate(shape)][1:]
        if 'conv_offset' in key:  # deformable_groups * 27 outputs
            return [shape[0]] + [num_feat * (d // 64) if i == 1 else d for i, d in enumerate(shape)][1:]
        return [num_feat * (d // 64) if i < 2 and d % 64 == 0 else d for i, d in enumerate(shape)]

    block0 = [(k.split('.', 2)[2], v) for k, v in golden.items() if k.startswith('reconstruction.0.')]
    done = False
    for key, shape in golden.items():
        if not key.startswith('reconstruction.'):
            out[key] = dims(key, shape)
        elif not done:
            done = True
            for b in range(blocks):
                for suffix, sh in block0:
                    out[f'reconstruction.{b}.{suffix}'] = dims('reconstruction', sh)
    return out


@pytest.mark.parametrize('name', sorted(OPTION_FILES))
def test_build_network_for_the_shipped_option_files(name):
    from basicsr4rs_amd.archs import build_network
    opt = OPTION_FILES[name]
    net = build_network(dict(opt))
    golden = json.load(open(GOLDEN))['edvr_m_tsa' if opt['with_tsa'] else 'edvr_m_wotsa']
    want = _scaled(golden, opt['num_feat'], opt['num_reconstruct_block'])
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    stock = R.StockEDVR(**{k: v for k, v in opt.items() if k != 'type'})
    n = sum(p.numel() for p in net.parameters())
    assert n == sum(p.numel() for p in stock.parameters())
    print(f'{name}: {n:,d} parameters')
    if opt['num_feat'] == 64 and opt['with_tsa']:
        assert n == 3300131  # EDVR-M
    # a reference-format checkpoint loads strictly
    sd = {'params': stock.state_dict()}
    net.load_state_dict(sd['params'], strict=True)
    k = 'pcd_align.dcn_pack.l2.conv_offset.weight'
    assert torch.equal(net.state_dict()[k], sd['params'][k])


def test_golden_predeblur_hr_config():
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='EDVR', **R.GOLDEN_CONFIGS['edvr_predeblur_hr']))
    golden = json.load(open(GOLDEN))['edvr_predeblur_hr']
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(golden) and got == golden


def test_initialisation_follows_the_reference():
    """conv_offset zeroed, the DCN bias zeroed and its weight uniform in +-1 / sqrt(fan), residual-block convs scaled
    by 0.1 with zero biases, plain convs with nn.Conv2d's default init."""
    from basicsr4rs_amd.archs import build_network
    torch.manual_seed(0)
    net = build_network(_net_opt(64, 1, True))
    pack = net.pcd_align.dcn_pack['l1']
    assert not pack.conv_offset.weight.any() and not pack.conv_offset.bias.any() and not pack.bias.any()
    bound = 1.0 / (64 * 9)**0.5
    assert pack.weight.abs().max() <= bound and pack.weight.abs().max() > 0.9 * bound
    rb = net.feature_extraction[0]
    assert not rb.conv1.bias.any() and 0.5 < rb.conv1.weight.std() / (0.1 * (2.0 / 576)**0.5) < 1.5
    assert net.conv_l2_1.bias.any() and net.conv_l2_1.weight.abs().max() <= bound + 1e-7


def test_refusals():
    from basicsr4rs_amd.archs import build_network
    with pytest.raises(ValueError, match='multiple of 8'):
        build_network(dict(type='EDVR', num_feat=60))
    with pytest.raises(ValueError, match='deformable_groups'):
        build_network(dict(type='EDVR', num_feat=64, deformable_groups=6))
    import basicsr4rs_amd.models  # noqa: F401
    from basicsr4rs_amd.utils.registry import ARCH_REGISTRY, MODEL_REGISTRY
    assert 'EDVR' in ARCH_REGISTRY and 'EDVRModel' in MODEL_REGISTRY
