"""ECBSR without a GPU: the arch is registered with the reference's module tree (state_dict names and shapes as
recorded from basicsr/archs/ecbsr_arch.py in tests/golden/ecbsr.npz), the recorded state loads strictly, the
reference's three ECBSR option files (stored unchanged under tests/golden/reference_options/) parse and build,
unsupported activations are refused, and the torch restatement tests/_ecbsr_ref.py -- which the GPU tests use in
float64 -- reproduces the recorded reference results."""
import os

import numpy as np
import pytest
import torch

from tests import _ecbsr_ref as R
from tests.golden.make_ecbsr_golden import CASES, M4C16

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'golden', 'reference_options')
YAMLS = ['train/ECBSR/train_ECBSR_x2_m4c16_prelu.yml', 'train/ECBSR/train_ECBSR_x4_m4c16_prelu.yml',
         'train/ECBSR/train_ECBSR_x4_m4c16_prelu_RGB.yml']


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'ecbsr.npz'))


def state(gold, case, dtype=torch.float32):
    return {k: torch.from_numpy(gold[f'{case}.sd.{k}']).to(dtype) for k in gold[f'{case}.names']}


@pytest.mark.parametrize('case', list(CASES))
def test_ecbsr_registered_with_reference_state_dict(gold, case):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.archs import build_network
    from basicsr4rs_amd.utils.registry import ARCH_REGISTRY
    assert 'ECBSR' in ARCH_REGISTRY
    cfg = CASES[case][0]
    net = build_network(dict(type='ECBSR', **cfg))
    sd = net.state_dict()
    names = [str(k) for k in gold[f'{case}.names']]
    assert list(sd.keys()) == names
    for k in names:
        assert tuple(sd[k].shape) == gold[f'{case}.sd.{k}'].shape, k
    net.load_state_dict(state(gold, case), strict=True)
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen == [k for k in names if k.endswith('.mask')] and len(frozen) == 3 * R.num_layers(sd)
    # the masks this arch builds are the reference's
    fresh = build_network(dict(type='ECBSR', **cfg)).state_dict()
    for k in frozen:
        assert np.array_equal(fresh[k].numpy(), gold[f'{case}.sd.{k}']), k


def test_ecbsr_default_init_is_the_references():
    """Same constructor arguments, same draws from the global generator in the same order."""
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.archs import build_network
    torch.manual_seed(3)
    net = build_network(dict(type='ECBSR', **M4C16))
    blk = net.backbone[1]
    assert blk.conv1x1_3x3.mid_planes == 32 and tuple(blk.conv1x1_3x3.k1.shape) == (16, 32, 3, 3)
    assert 0.0 < blk.conv1x1_sbx.scale.abs().max().item() < 1e-2 and tuple(blk.conv1x1_sbx.scale.shape) == (16, 1, 1, 1)
    assert torch.all(blk.act.weight == 0.25) and not hasattr(net.backbone[-1], 'act')


@pytest.mark.parametrize('rel', YAMLS)
def test_ecbsr_reference_yaml_parses_and_builds(gold, rel, tmp_path):
    import basicsr4rs_amd.archs  # noqa: F401
    import basicsr4rs_amd.losses  # noqa: F401
    import basicsr4rs_amd.models  # noqa: F401
    from basicsr4rs_amd.archs import build_network
    from basicsr4rs_amd.utils.options import parse_options
    from basicsr4rs_amd.utils.registry import LOSS_REGISTRY, MODEL_REGISTRY
    assert os.path.exists(os.path.join(REF, rel)), rel
    opt, _ = parse_options(str(tmp_path), is_train=True, argv=['-opt', os.path.join(REF, rel)])
    assert opt['network_g']['type'] == 'ECBSR' and opt['model_type'] == 'SRModel' and opt['model_type'] in MODEL_REGISTRY
    assert opt['train']['pixel_opt']['type'] == 'L1Loss' and 'L1Loss' in LOSS_REGISTRY
    assert opt['train']['scheduler']['type'] == 'MultiStepLR' and opt['train']['optim_g']['type'] == 'Adam'
    net = build_network(dict(opt['network_g']))
    assert type(net).__name__ == 'ECBSR'
    if rel.endswith('x4_m4c16_prelu.yml'):
        assert {k: v for k, v in opt['network_g'].items() if k != 'type'} == M4C16
        sd = net.state_dict()
        assert list(sd.keys()) == [str(k) for k in gold['m4c16.names']]
        assert [','.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold['m4c16.shapes']]
        assert sum(p.numel() for p in net.parameters()) == int(gold['m4c16.nparams'])


@pytest.mark.parametrize('act', ['rrelu', 'softplus'])
def test_ecbsr_unsupported_acts_raise(act):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.archs import build_network
    with pytest.raises(ValueError, match='prelu, relu, linear'):
        build_network(dict(type='ECBSR', **dict(M4C16, act_type=act)))


def test_ecbsr_input_gradient_is_refused():
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='ECBSR', **CASES['C'][0]))
    with pytest.raises(NotImplementedError, match='input image'):
        net(torch.zeros(1, 1, 2, 2, requires_grad=True))


def test_ecbsr_state_follows_a_deep_copy():
    """The cached collapse state names its blocks weakly; a deep copy of a net must not keep using the original's."""
    import copy

    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.archs import build_network
    from basicsr4rs_amd.ops import ecb as E
    net = build_network(dict(type='ECBSR', **CASES['C'][0]))
    st = E.state_of(net, list(net.backbone), torch.float32, False)
    assert E.state_of(net, list(net.backbone), torch.float32, False) is st
    twin = copy.deepcopy(net)
    st2 = E.state_of(twin, list(twin.backbone), torch.float32, False)
    assert st2 is not st and st2.blocks[0] is twin.backbone[0] and st.blocks[0] is net.backbone[0]
    assert len(E.block_params(net.backbone[0])) == 18 and len(E.block_params(build_network(
        dict(type='ECBSR', **CASES['A'][0])).backbone[0])) == 19


@pytest.mark.parametrize('case', list(CASES))
def test_ecbsr_ref_reproduces_the_recording(gold, case):
    """fp32 five-branch outputs and gradients, and the fp64 collapse against the recorded rep_params(): 1e-5
    absolute on values of order 1 (the reference's own two forms differ by 1.3e-6 here); the restatement's
    collapsed form equals its five-branch form in fp64 to 1e-12 relative."""
    cfg, _ = CASES[case]
    kw = dict(scale=cfg['scale'], with_idt=cfg['with_idt'], act_type=cfg['act_type'])
    sd = {k: (v.requires_grad_(True) if not k.endswith('.mask') else v) for k, v in state(gold, case).items()}
    x, g = torch.from_numpy(gold[f'{case}.x']), torch.from_numpy(gold[f'{case}.g'])
    torch.set_num_threads(1)
    out = R.forward(sd, x, **kw)
    (out * g).sum().backward()
    err = (out.detach() - torch.from_numpy(gold[f'{case}.out_train'])).abs().max().item()
    print(f'case {case}: train output max-abs {err:.3e} (max |ref| {np.abs(gold[f"{case}.out_train"]).max():.3e})')
    assert err <= 1e-5
    for k, v in sd.items():
        if k.endswith('.mask'):
            continue
        ref = torch.from_numpy(gold[f'{case}.grad.{k}'])
        e = (v.grad - ref).abs().max().item()
        assert e <= 1e-5, (k, e, ref.abs().max().item())
    sd64 = state(gold, case, torch.float64)
    for l in range(R.num_layers(sd64)):
        rk, rb = R.collapse(sd64, f'backbone.{l}.', cfg['with_idt'])
        assert (rk - torch.from_numpy(gold[f'{case}.rep.{l}.weight']).double()).abs().max().item() <= 1e-5
        assert (rb - torch.from_numpy(gold[f'{case}.rep.{l}.bias']).double()).abs().max().item() <= 1e-5
    a = R.forward(sd64, x.double(), **kw)
    b = R.forward(sd64, x.double(), collapsed=True, **kw)
    rel = (a - b).abs().max().item() / a.abs().max().item()
    print(f'case {case}: collapsed vs five-branch fp64 relative {rel:.3e}')
    assert rel <= 1e-12
    e2 = (b.float() - torch.from_numpy(gold[f'{case}.out_eval'])).abs().max().item()
    assert e2 <= 1e-5
