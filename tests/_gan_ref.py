"""Stock-torch restatements used by the GAN tests: the VGG-style discriminator as a plain ``nn.Module`` (the layer
list of basicsr/archs/discriminator_arch.py:19-87, NCHW, nn.Conv2d / nn.BatchNorm2d / nn.Linear forward), with an
optional ``store`` hook at every place the HIP engine keeps a feature map (for the bf16-storage emulation of
tests/test_perceptual_gpu.py), and a truncated VGG + perceptual loss in torch ops."""
import torch
from torch import nn as nn
from torch.nn import functional as F

from ._fp64 import _rne_bf16


class Store(torch.autograd.Function):
    """A map as the bf16 engine keeps it: rounded to bf16 forward, its gradient map rounded to bf16 backward."""

    @staticmethod
    def forward(ctx, t):
        return _rne_bf16(t.detach())

    @staticmethod
    def backward(ctx, g):
        return _rne_bf16(g)


class StockDiscriminator(nn.Module):

    def __init__(self, num_in_ch, num_feat, input_size=128):
        super().__init__()
        self.input_size = input_size
        self.stages = 5 if input_size == 128 else 6
        nf, mult = num_feat, (1, 2, 4, 8, 8, 8)
        self.conv0_0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1, bias=True)
        self.conv0_1 = nn.Conv2d(nf, nf, 4, 2, 1, bias=False)
        self.bn0_1 = nn.BatchNorm2d(nf, affine=True)
        for s in range(1, self.stages):
            cin, cout = nf * mult[s - 1], nf * mult[s]
            setattr(self, f'conv{s}_0', nn.Conv2d(cin, cout, 3, 1, 1, bias=False))
            setattr(self, f'bn{s}_0', nn.BatchNorm2d(cout, affine=True))
            setattr(self, f'conv{s}_1', nn.Conv2d(cout, cout, 4, 2, 1, bias=False))
            setattr(self, f'bn{s}_1', nn.BatchNorm2d(cout, affine=True))
        self.linear1 = nn.Linear(nf * 8 * 4 * 4, 100)
        self.linear2 = nn.Linear(100, 1)
        self.store = None

    def forward(self, x):
        st = self.store if self.store is not None else (lambda t: t)
        act = lambda t: F.leaky_relu(t, 0.2)  # noqa: E731
        h = st(act(self.conv0_0(st(x))))
        h = st(act(self.bn0_1(st(self.conv0_1(h)))))
        for s in range(1, self.stages):
            h = st(act(getattr(self, f'bn{s}_0')(st(getattr(self, f'conv{s}_0')(h)))))
            h = st(act(getattr(self, f'bn{s}_1')(st(getattr(self, f'conv{s}_1')(h)))))
        h = h.reshape(h.size(0), -1)
        return self.linear2(act(self.linear1(h)))


def he_init(net, seed):
    """He-scaled conv / linear weights (for LeakyReLU 0.2: std sqrt(2 / (1.04 fan_in))), gamma near 1, beta small,
    so that magnitudes hold through the depth."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (1.04 * fan_in))**0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.01)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=g))
    return net


def stock_like(sd, num_in_ch, num_feat, input_size, dtype, round_convs=False, store=None):
    """A StockDiscriminator of ``dtype`` loaded strictly from ``sd``; ``round_convs``: the conv weights rounded to
    bf16 (as the prepared GEMM images hold them; BatchNorm and linear parameters stay fp32 in the engine)."""
    net = StockDiscriminator(num_in_ch, num_feat, input_size).to(dtype)
    net.load_state_dict({k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu().clone()
                         for k, v in sd.items()}, strict=True)
    if round_convs:
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.copy_(_rne_bf16(m.weight.double()).to(dtype))
    net.store = store
    return net


# conv layers of vgg11 up to relu2_1: conv1_1 -> relu -> pool -> conv2_1 -> relu
VGG11_HEAD = (('conv1_1', 3, 64), ('conv2_1', 64, 128))


def vgg_head_features(sd, x, mean, std, store=None, round_convs=False):
    """{'relu2_1': feature} of a vgg11 truncated after relu2_1 with use_input_norm (vgg_arch.py semantics).
    ``store`` / ``round_convs``: the bf16-storage emulation (every kept map through ``store``, conv weights rounded)."""
    st = store if store is not None else (lambda t: t)
    w = (lambda k: _rne_bf16(sd[k].double()).to(sd[k].dtype)) if round_convs else (lambda k: sd[k])
    h = st((x - mean) / std)
    h = st(F.relu(F.conv2d(h, w('vgg_net.conv1_1.weight'), sd['vgg_net.conv1_1.bias'], padding=1)))
    h = st(F.max_pool2d(h, 2, 2))
    h = st(F.relu(F.conv2d(h, w('vgg_net.conv2_1.weight'), sd['vgg_net.conv2_1.bias'], padding=1)))
    return {'relu2_1': h}
