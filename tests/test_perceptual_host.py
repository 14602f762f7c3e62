"""Host side of the perceptual loss (no GPU): registries, the VGG layer tables and truncation, state-dict
keys, weight files in torchvision's and in the module's own keys, and the refusals.  The model build with
``train.perceptual_opt`` needs a device (SRModel moves its nets there), so it is covered in
test_perceptual_gpu.py."""
import ctypes

import pytest
import torch

from basicsr4rs_amd import _lib
from basicsr4rs_amd.archs import vgg_arch
from basicsr4rs_amd.archs.vgg_arch import NAMES, VGGFeatureExtractor, conv_channels
from basicsr4rs_amd.utils.registry import ARCH_REGISTRY, LOSS_REGISTRY


@pytest.fixture(autouse=True)
def _no_ambient_weights(monkeypatch, tmp_path):
    """No weight file from the environment or the working directory leaks into a test."""
    monkeypatch.delenv(vgg_arch.VGG_WEIGHTS_ENV, raising=False)
    monkeypatch.chdir(tmp_path)


def test_registries_resolve_the_new_names():
    from basicsr4rs_amd.losses import PerceptualLoss
    assert ARCH_REGISTRY.get('VGGFeatureExtractor') is VGGFeatureExtractor
    assert LOSS_REGISTRY.get('PerceptualLoss') is PerceptualLoss


def test_name_tables():
    # torchvision's ``features`` lengths and a few fixed positions (the index -> name map of a weight file)
    assert {k: len(v) for k, v in NAMES.items()} == {'vgg11': 21, 'vgg13': 25, 'vgg16': 31, 'vgg19': 37}
    assert NAMES['vgg19'][:5] == ['conv1_1', 'relu1_1', 'conv1_2', 'relu1_2', 'pool1']
    assert NAMES['vgg19'].index('conv5_4') == 34 and NAMES['vgg19'][-1] == 'pool5'
    assert NAMES['vgg16'].index('conv3_3') == 14 and 'conv3_4' not in NAMES['vgg16']
    assert NAMES['vgg11'][:4] == ['conv1_1', 'relu1_1', 'pool1', 'conv2_1']
    assert conv_channels('conv1_1') == (3, 64) and conv_channels('conv2_1') == (64, 128)
    assert conv_channels('conv3_4') == (256, 256) and conv_channels('conv5_1') == (512, 512)


def test_truncation_and_state_dict_keys():
    net = VGGFeatureExtractor(['conv3_4'], pretrained=False)
    convs = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv3_4']
    assert list(net.vgg_net._modules) == convs
    assert net.layers[-1] == 'conv3_4' and net.layers.count('pool2') == 1
    keys = [f'vgg_net.{c}.{p}' for c in convs for p in ('weight', 'bias')] + ['mean', 'std']
    assert sorted(net.state_dict()) == sorted(keys)
    assert net.vgg_net.conv2_1.weight.shape == (128, 64, 3, 3)
    assert tuple(net.mean.shape) == (1, 3, 1, 1)
    assert not any(p.requires_grad for p in net.parameters())
    assert all(p.requires_grad for p in VGGFeatureExtractor(['relu1_1'], pretrained=False, requires_grad=True).parameters())
    assert 'mean' not in VGGFeatureExtractor(['relu1_1'], pretrained=False, use_input_norm=False).state_dict()
    nopool = VGGFeatureExtractor(['conv2_1'], pretrained=False, remove_pooling=True)
    assert nopool.layers == ['conv1_1', 'relu1_1', 'conv1_2', 'relu1_2', 'conv2_1']
    with pytest.raises(ValueError, match='conv9_9'):
        VGGFeatureExtractor(['conv9_9'], pretrained=False)


def _torchvision_vgg11_state(seed=0):
    """State dict with torchvision's vgg11 keys: features.<i> of every conv plus the classifier."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, name in enumerate(NAMES['vgg11']):
        if name.startswith('conv'):
            cin, cout = conv_channels(name)
            sd[f'features.{i}.weight'] = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
            sd[f'features.{i}.bias'] = torch.randn(cout, generator=g) * 0.01
    sd['classifier.0.weight'] = torch.zeros(4, 4)
    sd['classifier.0.bias'] = torch.zeros(4)
    return sd


def test_weight_file_forms(tmp_path, monkeypatch):
    tv = _torchvision_vgg11_state()
    f_tv = tmp_path / 'vgg11_tv.pth'
    torch.save(tv, f_tv)
    a = VGGFeatureExtractor(['conv2_1'], vgg_type='vgg11', pretrain_path=str(f_tv))
    assert list(a.vgg_net._modules) == ['conv1_1', 'conv2_1']
    # vgg11: features.0 is conv1_1, features.3 is conv2_1
    assert torch.equal(a.vgg_net.conv1_1.weight, tv['features.0.weight'])
    assert torch.equal(a.vgg_net.conv2_1.weight, tv['features.3.weight'])
    assert torch.equal(a.vgg_net.conv2_1.bias, tv['features.3.bias'])
    assert not a.vgg_net.conv2_1.weight.requires_grad
    # the module's own keys give the same values
    f_own = tmp_path / 'vgg11_own.pth'
    torch.save(a.state_dict(), f_own)
    b = VGGFeatureExtractor(['conv2_1'], vgg_type='vgg11', pretrain_path=str(f_own))
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    # the environment variable, then the default place under the working directory
    monkeypatch.setenv(vgg_arch.VGG_WEIGHTS_ENV, str(f_tv))
    c = VGGFeatureExtractor(['conv2_1'], vgg_type='vgg11')
    assert torch.equal(c.vgg_net.conv2_1.weight, tv['features.3.weight'])
    monkeypatch.delenv(vgg_arch.VGG_WEIGHTS_ENV)
    default = tmp_path / vgg_arch.VGG_PRETRAIN_PATH
    default.parent.mkdir(parents=True)
    torch.save(tv, default)
    d = VGGFeatureExtractor(['conv1_1'], vgg_type='vgg11')
    assert torch.equal(d.vgg_net.conv1_1.weight, tv['features.0.weight'])
    # a file of another VGG: the shapes or the layers do not fit
    with pytest.raises((ValueError, KeyError)):
        VGGFeatureExtractor(['conv3_1'], vgg_type='vgg19', pretrain_path=str(f_tv))


def test_no_weight_file_raises_and_names_the_places(tmp_path):
    with pytest.raises(FileNotFoundError) as e:
        VGGFeatureExtractor(['conv1_1'])
    msg = str(e.value)
    assert 'pretrain_path' in msg and vgg_arch.VGG_WEIGHTS_ENV in msg and vgg_arch.VGG_PRETRAIN_PATH in msg
    with pytest.raises(FileNotFoundError):
        VGGFeatureExtractor(['conv1_1'], pretrain_path=str(tmp_path / 'missing.pth'))
    from basicsr4rs_amd.losses import build_loss
    with pytest.raises(FileNotFoundError):
        build_loss(dict(type='PerceptualLoss', layer_weights={'conv1_2': 1.0}))


def test_refusals():
    with pytest.raises(NotImplementedError):
        VGGFeatureExtractor(['conv1_1'], vgg_type='vgg19_bn', pretrained=False)
    net = VGGFeatureExtractor(['conv1_1'], pretrained=False)
    with pytest.raises(ValueError, match=r'\(1, 4, 8, 8\)'):
        net(torch.zeros(1, 4, 8, 8))
    from basicsr4rs_amd.losses import PerceptualLoss
    with pytest.raises(NotImplementedError, match='huber criterion has not been supported.'):
        PerceptualLoss({'conv1_1': 1.0}, criterion='huber', pretrained=False)
    loss = PerceptualLoss({'conv1_1': 1.0}, pretrained=False)
    with pytest.raises(NotImplementedError, match='MI355X'):
        loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_kernel_argument_checks():
    """The new ABI entries refuse bad arguments before any launch (no device needed)."""
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    odd = ctypes.c_void_p(68)
    err = lambda: lib.sr_last_error().decode()  # noqa: E731
    assert lib.sr_maxpool2_fwd(0, None, 1, 4, 4, 8, 2, p, None) == -1 and 'maxpool2_fwd' in err()
    assert lib.sr_maxpool2_fwd(0, p, 1, 4, 4, 8, 3, p, None) == -1 and 'stride' in err()
    assert lib.sr_maxpool2_fwd(0, p, 1, 4, 4, 12, 2, p, None) == -1 and 'multiple of 8' in err()
    assert lib.sr_maxpool2_fwd(0, p, 1, 1, 4, 8, 2, p, None) == -1 and 'window' in err()
    assert lib.sr_maxpool2_fwd(2, p, 1, 4, 4, 8, 2, p, None) == -1 and 'dtype' in err()
    assert lib.sr_maxpool2_fwd(0, odd, 1, 4, 4, 8, 2, p, None) == -1 and 'aligned' in err()
    assert lib.sr_maxpool2_fwd(0, p, 0, 4, 4, 8, 2, p, None) == -1
    assert lib.sr_maxpool2_fwd(0, p, 8, 4096, 4096, 8, 2, p, None) == -3  # 2^32 bytes
    assert lib.sr_maxpool2_bwd(1, p, None, 1, 4, 4, 8, 2, p, None) == -1 and 'maxpool2_bwd' in err()
    assert lib.sr_maxpool2_bwd(1, p, p, 4, 8192, 8192, 8, 1, p, None) == -3
    assert lib.sr_gram_fwd(0, None, 1, 4, 8, 1.0, p, None, 0, None) == -1
    assert lib.sr_gram_fwd(0, p, 1, 4, 520, 1.0, p, None, 0, None) == -1 and 'at most 512' in err()
    assert lib.sr_gram_fwd(0, p, 1, 4, 12, 1.0, p, None, 0, None) == -1
    assert lib.sr_gram_fwd(0, p, 1, 0, 8, 1.0, p, None, 0, None) == -1
    assert lib.sr_gram_fwd(1, p, 64, 1 << 16, 512, 1.0, p, p, 1 << 40, None) == -3
    kb = lib.sr_gram_kblock()
    assert lib.sr_gram_splits(kb) == 1 and lib.sr_gram_splits(kb + 1) == 2 and lib.sr_gram_splits(64 * kb) == 64
    assert lib.sr_gram_splits(64 * kb + 1) == 33  # blocks of 2 * kb rows
    assert lib.sr_gram_workspace(2, kb, 64) == 0 and lib.sr_gram_workspace(2, kb + 1, 64) == 2 * 2 * 64 * 64 * 4
    # more than one split needs the workspace
    assert lib.sr_gram_fwd(0, p, 1, kb + 1, 64, 1.0, p, None, 0, None) == -1 and 'workspace' in err()
    assert lib.sr_gram_fwd(0, p, 1, kb + 1, 64, 1.0, p, p, 16, None) == -1 and 'workspace' in err()
    assert lib.sr_gram_bwd(0, p, None, None, 1, 4, 8, 1.0, 0.0, p, None) == -1
    assert lib.sr_gram_bwd(0, p, p, odd, 1, 4, 8, 1.0, 1.0, p, None) == -1 and 'aligned' in err()
    assert lib.sr_gram_bwd(0, p, p, None, 1, 4, 1024, 1.0, 0.0, p, None) == -1
    assert lib.sr_gram_bwd(1, p, p, None, 64, 1 << 16, 512, 1.0, 0.0, p, None) == -3
