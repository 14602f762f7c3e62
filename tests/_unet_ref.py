"""Stock-torch restatements used by the UNetDiscriminatorSN tests.

``StockUNetSN``: the layer list of basicsr/archs/discriminator_arch.py:102-150 as a plain ``nn.Module`` (NCHW,
``nn.Conv2d`` wrapped by torch's ``spectral_norm``, ``F.interpolate``), with the optional bf16-storage emulation of
tests/_gan_ref.py: ``store`` at every place the HIP engine keeps a feature map, ``gstore`` where it keeps a gradient
map that has no forward counterpart (the activation backward's output, between the conv and its LeakyReLU), and
``round_w`` for the normalised conv weights as the GEMM images hold them.

The float64 helper formulas (any dtype in, computed in the dtype given): the power iteration of spectral norm, its
backward with u and v as constants, the separable bilinear x2 rule and its transpose."""
import torch
from torch import nn as nn
from torch.nn import functional as F
from torch.nn.utils import spectral_norm

from ._fp64 import _rne_bf16
from ._gan_ref import Store


class GradStore(torch.autograd.Function):
    """A gradient map as the bf16 engine keeps it, with nothing stored forward."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _rne_bf16(g)


class RoundWeight(torch.autograd.Function):
    """A conv weight as its bf16 GEMM image holds it; the gradient passes to the fp32 weight as it is."""

    @staticmethod
    def forward(ctx, w):
        return _rne_bf16(w.detach().double()).to(w.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class StockUNetSN(nn.Module):

    def __init__(self, num_in_ch, num_feat=64, skip_connection=True):
        super().__init__()
        self.skip_connection = skip_connection
        nf, norm = num_feat, spectral_norm
        self.conv0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        self.conv1 = norm(nn.Conv2d(nf, nf * 2, 4, 2, 1, bias=False))
        self.conv2 = norm(nn.Conv2d(nf * 2, nf * 4, 4, 2, 1, bias=False))
        self.conv3 = norm(nn.Conv2d(nf * 4, nf * 8, 4, 2, 1, bias=False))
        self.conv4 = norm(nn.Conv2d(nf * 8, nf * 4, 3, 1, 1, bias=False))
        self.conv5 = norm(nn.Conv2d(nf * 4, nf * 2, 3, 1, 1, bias=False))
        self.conv6 = norm(nn.Conv2d(nf * 2, nf, 3, 1, 1, bias=False))
        self.conv7 = norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv8 = norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(nf, 1, 3, 1, 1)
        self.store = self.gstore = self.round_w = None

    def _conv(self, m, x):
        if self.round_w is None:
            return m(x)
        for hook in m._forward_pre_hooks.values():  # torch's spectral norm: the power iteration, m.weight
            hook(m, (x, ))
        return F.conv2d(x, self.round_w(m.weight), m.bias, m.stride, m.padding)

    def forward(self, x):
        st = self.store if self.store is not None else (lambda t: t)
        gst = self.gstore if self.gstore is not None else (lambda t: t)
        act = lambda m, t: F.leaky_relu(gst(self._conv(m, t)), 0.2)  # noqa: E731
        up = lambda t: st(F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False))  # noqa: E731
        skip = self.skip_connection
        x0 = st(act(self.conv0, st(x)))
        x1 = st(act(self.conv1, x0))
        x2 = st(act(self.conv2, x1))
        x3 = st(act(self.conv3, x2))
        x4 = act(self.conv4, up(x3))
        x4 = st(x4 + x2 if skip else x4)
        x5 = act(self.conv5, up(x4))
        x5 = st(x5 + x1 if skip else x5)
        x6 = act(self.conv6, up(x5))
        x6 = st(x6 + x0 if skip else x6)
        out = st(act(self.conv7, x6))
        out = st(act(self.conv8, out))
        # the engine keeps the gradient of the fp32 output map in the feature dtype before conv9's backward
        return gst(self._conv(self.conv9, out))


def he_init_sn(net, seed):
    """He-scaled ``weight`` / ``weight_orig`` (LeakyReLU 0.2), small biases; u and v stay torch's unit vectors."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                w = m.weight_orig if hasattr(m, 'weight_orig') else m.weight
                w.copy_(torch.randn(w.shape, generator=g) * (2.0 / (1.04 * w[0].numel()))**0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.01)
    return net


def stock_like(sd, num_in_ch, num_feat, dtype, skip=True, emulate=False):
    """A StockUNetSN of ``dtype`` loaded strictly from ``sd``; ``emulate``: the bf16-storage emulation."""
    net = StockUNetSN(num_in_ch, num_feat, skip).to(dtype)
    net.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in sd.items()}, strict=True)
    if emulate:
        net.store, net.gstore, net.round_w = Store.apply, GradStore.apply, RoundWeight.apply
    return net


# ------------------------------------------------------------------------------------------------ formulas


def power_iteration(M, u, v, eps=1e-12, iterate=True):
    """One step of torch's spectral norm on M [R, K]: (u', v', sigma, W); ``iterate=False``: the stored vectors."""
    if iterate:
        t = M.t() @ u
        v = t / t.norm().clamp_min(eps)
        s = M @ v
        u = s / s.norm().clamp_min(eps)
    sigma = torch.dot(u, M @ v)
    return u, v, sigma, M / sigma


def sn_backward(G, W, u, v, sigma):
    """dL/dweight_orig from G = dL/dW with u, v constants: (G - <G, W> u v^T) / sigma."""
    return (G - (G * W).sum() * torch.outer(u, v)) / sigma


def up2_axis(x, dim):
    """out[2i] = .25 in[max(i-1,0)] + .75 in[i], out[2i+1] = .75 in[i] + .25 in[min(i+1,n-1)] along ``dim``."""
    n = x.shape[dim]
    i = torch.arange(n)
    lo, hi = x.index_select(dim, (i - 1).clamp(min=0)), x.index_select(dim, (i + 1).clamp(max=n - 1))
    even, odd = 0.25 * lo + 0.75 * x, 0.75 * x + 0.25 * hi
    return torch.stack([even, odd], dim + 1).flatten(dim, dim + 1)


def up2(x, dims=(-2, -1)):
    dims = [d % x.dim() for d in dims]
    return up2_axis(up2_axis(x, dims[0]), dims[1])


def up2_axis_t(dy, dim):
    """The transpose of up2_axis as a gather: dx[j] = .25 dy[2j-1] + .75 dy[2j] + .75 dy[2j+1] + .25 dy[2j+2] with
    the indices clamped to the map (the clamped edge taps fold onto the edge pixel)."""
    n2 = dy.shape[dim]
    j = torch.arange(n2 // 2)
    tap = lambda k: dy.index_select(dim, (2 * j + k).clamp(0, n2 - 1))  # noqa: E731
    return 0.25 * tap(-1) + 0.75 * tap(0) + 0.75 * tap(1) + 0.25 * tap(2)


def up2_t(dy, dims=(-2, -1)):
    dims = [d % dy.dim() for d in dims]
    return up2_axis_t(up2_axis_t(dy, dims[0]), dims[1])


def up2_absw(x, dims=(-2, -1)):
    """sum |w x| of the forward (the magnitude a rounding bound multiplies)."""
    return up2(x.abs(), dims)
