"""The float64 restatements of tests/_degrade_ref.py against torch on the CPU in float64 (no GPU): F.pad + F.conv2d
for the filter, F.interpolate in both coordinate conventions for the three modes, and plain torch compositions
(the dense 51 x 51 blur; the 64 x 64 DCT contraction) for USM and JPEG."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import _degrade_ref as R


def _conv_filter(x, kernel):
    k = kernel.shape[-1]
    B, C, H, W = x.shape
    xp = F.pad(x, (k // 2, ) * 4, mode='reflect')
    w = kernel.expand(B, k, k).reshape(B, 1, k, k).repeat_interleave(C, 0)
    return F.conv2d(xp.reshape(1, B * C, *xp.shape[-2:]), w, groups=B * C).view(B, C, H, W)


@pytest.mark.parametrize('k, shared', [(3, False), (7, True), (21, False)])
def test_filter2d_ref(k, shared):
    g = torch.Generator().manual_seed(k)
    x = torch.rand(2, 3, 24, 40, generator=g, dtype=torch.float64)
    kern = torch.randn(1 if shared else 2, k, k, generator=g, dtype=torch.float64)
    y, mag = R.filter2d(x, kern)
    want = _conv_filter(x, kern)
    assert (y - want).abs().max() <= 1e-12 * mag.max()
    assert (mag >= y.abs() - 1e-12).all()


def test_round255_ref():
    # 0.5, 1.5 and 2.5 are exact ties (half to even: 0, 2, 2); 79.05 is 0.45 from a tie; the ends clamp
    v = torch.tensor([0.0, 0.5, 1.5, 2.5, 79.05, 306.0, -25.5], dtype=torch.float64) / 255
    q, margin = R.round255(v)
    assert torch.allclose(q * 255, torch.tensor([0.0, 0, 2, 2, 79, 255, 0], dtype=torch.float64), atol=1e-12)
    assert margin[1] < 1e-9 and abs(margin[4].item() - 0.45) < 1e-9


def test_gaussian_taps_and_usm_ref():
    taps = R.gaussian_taps(51, 0)
    assert abs(taps.sum().item() - 1) < 1e-15 and taps.argmax() == 25
    assert abs(taps[24] / taps[25] - math.exp(-1 / 128.0)) < 1e-15  # sigma = 8
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, 30, 34, generator=g, dtype=torch.float64)
    dense = torch.outer(taps, taps)[None]
    r = R.usm(x, taps, 0.5, 10)
    blur = _conv_filter(x, dense)
    assert (r.blur - blur).abs().max() < 1e-13
    res = x - blur
    mask = (res.abs() * 255 > 10).double()
    soft = _conv_filter(mask, dense)
    out = soft * torch.clip(x + 0.5 * res, 0, 1) + (1 - soft) * x
    assert torch.equal(r.mask, mask) and (r.out - out).abs().max() < 1e-13
    assert 0 < r.mask.mean() < 1


@pytest.mark.parametrize('mode', ['area', 'bilinear', 'bicubic'])
@pytest.mark.parametrize('how', [('scale', 1.37), ('scale', 0.46), ('size', (13, 21)), ('size', (24, 40))])
def test_resize_ref(mode, how):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 24, 40, generator=g, dtype=torch.float64)
    if how[0] == 'scale':
        want = F.interpolate(x, scale_factor=how[1], mode=mode)
        (Ho, sh), (Wo, sw) = R.resize_geometry(24, scale_factor=how[1]), R.resize_geometry(40, scale_factor=how[1])
    else:
        want = F.interpolate(x, size=how[1], mode=mode)
        (Ho, sh), (Wo, sw) = R.resize_geometry(24, size=how[1][0]), R.resize_geometry(40, size=how[1][1])
    y, bound = R.resize(x, (Ho, Wo), (sh, sw), mode)
    assert y.shape == want.shape
    assert (y - want).abs().max() < 1e-12
    assert (bound > 0).all()


def test_noise_refs():
    g = torch.Generator().manual_seed(5)
    img = torch.rand(2, 3, 8, 10, generator=g, dtype=torch.float64)
    normal, ngray = torch.randn(2, 3, 8, 10, generator=g, dtype=torch.float64), torch.randn(8, 10, generator=g, dtype=torch.float64)
    sigma, gray = torch.tensor([3.0, 20.0], dtype=torch.float64), torch.tensor([0.0, 1.0], dtype=torch.float64)
    out, mag = R.gaussian_noise(img, normal, ngray, sigma, gray)
    assert torch.allclose(out[0], torch.clamp(img[0] + normal[0] * 3 / 255, 0, 1), atol=1e-15)
    assert torch.allclose(out[1], torch.clamp(img[1] + ngray[None] * 20 / 255, 0, 1), atol=1e-15)
    lv = R.poisson_levels(img)
    for i in range(2):
        n = torch.unique(torch.clamp((img[i] * 255).round(), 0, 255)).numel()
        assert lv.count_c[i] == n and lv.vals[i, 0] == 2**math.ceil(math.log2(n))
    draw_c, draw_g = torch.poisson(lv.rate_c, generator=g), torch.poisson(lv.rate_g, generator=g)
    out, _ = R.poisson_noise(img, lv, draw_c, draw_g, torch.tensor([1.0, 2.0]), gray)
    want0 = torch.clamp(img[0] + (draw_c[0] / lv.vals[0, 0] - lv.qc[0]), 0, 1)
    want1 = torch.clamp(img[1] + 2 * (draw_g[1] / lv.vals[1, 1] - lv.qg[1]).expand(3, 8, 10), 0, 1)
    assert torch.allclose(out[0], want0, atol=1e-15) and torch.allclose(out[1], want1, atol=1e-15)


def _jpeg_torch(x, factor):
    """DiffJPEG's forward written with the dense 8 x 8 x 8 x 8 contraction, float64, round half to even."""
    B, _, H, W = x.shape
    x = F.pad(x, (0, -W % 16, 0, -H % 16)) * 255
    Hp, Wp = x.shape[-2:]
    m = torch.tensor(R.RGB2YCC, dtype=torch.float64).t()
    img = torch.tensordot(x.permute(0, 2, 3, 1), m, dims=1) + torch.tensor([0.0, 128, 128], dtype=torch.float64)
    t = np.zeros((8, 8, 8, 8))
    for a, b, u, v in itertools.product(range(8), repeat=4):
        t[a, b, u, v] = np.cos((2 * a + 1) * u * np.pi / 16) * np.cos((2 * b + 1) * v * np.pi / 16)
    fwd = torch.from_numpy(t)
    inv = fwd.permute(2, 3, 0, 1).contiguous()
    alpha = torch.tensor([1 / np.sqrt(2)] + [1] * 7, dtype=torch.float64)
    al = torch.outer(alpha, alpha)
    yt = torch.tensor(R.Y_TABLE_ROWS, dtype=torch.float64).t()
    ct = torch.full((8, 8), 99.0, dtype=torch.float64)
    ct[:4, :4] = torch.tensor(R.C_CORNER, dtype=torch.float64).t()
    comps = []
    for c in range(3):
        p = img[..., c]
        h, w = Hp, Wp
        if c:
            p = F.avg_pool2d(p.unsqueeze(1), 2, 2).squeeze(1)
            h, w = Hp // 2, Wp // 2
        blk = p.view(B, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4).reshape(B, -1, 8, 8)
        d = al * 0.25 * torch.tensordot(blk - 128, fwd, dims=2)
        table = (yt if c == 0 else ct) * factor.view(B, 1, 1, 1)
        q = torch.round(d / table) * table
        rec = 0.25 * torch.tensordot(q * al, inv, dims=2) + 128
        rec = rec.view(B, h // 8, w // 8, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, h, w)
        if c:
            rec = rec.repeat_interleave(2, 1).repeat_interleave(2, 2)
        comps.append(rec)
    ycc = torch.stack(comps, 3) + torch.tensor([0.0, -128, -128], dtype=torch.float64)
    rgb = torch.tensordot(ycc, torch.tensor(R.YCC2RGB, dtype=torch.float64).t(), dims=1).permute(0, 3, 1, 2)
    return (torch.clamp(rgb, 0, 255) / 255)[:, :, :H, :W]


def test_jpeg_ref():
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, 3, 40, 56, generator=g, dtype=torch.float64)
    q = torch.tensor([30.0, 75.0], dtype=torch.float64)
    f = R.quality_factor(q)
    assert torch.allclose(f, torch.tensor([5000 / 30 / 100, 0.5], dtype=torch.float64), atol=1e-15)
    want = _jpeg_torch(x, f)
    got = R.jpeg(x, q)
    assert got.shape == (2, 3, 40, 56)
    # the two differ only in summation order: far below the distance to a rounding boundary on this input
    assert (got - want).abs().max() < 1e-10
    pre = R.jpeg_encode(x, q)
    assert pre[0].shape == (2, 6, 8, 8, 8) and pre[1].shape == (2, 3, 4, 8, 8)
    img, mag = R.jpeg_decode(tuple(torch.round(p) for p in pre), q, 40, 56)
    assert torch.equal(img, got) and (mag >= img - 1e-12).all()
    # the fp32 replay stays close to the float64 coefficients
    pre32 = R.jpeg_encode(x, q, torch.float32)
    assert max((a.double() - b).abs().max().item() for a, b in zip(pre32, pre)) < 1e-3
