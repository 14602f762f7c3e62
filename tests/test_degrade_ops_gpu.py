"""The degradation kernels (csrc/degrade.hip through ops/degrade.py) against the float64 restatements of
tests/_degrade_ref.py, never against the code under test.  Conventions of tests/_fp64.py: U = 2^-24, ``_check`` prints
each measured error beside its derived bound.  Bounds:

filter2D: (k^2 + 2) U sum |w x| per element; bit for bit on integer grids and for the pulse kernel.
round255: the inputs keep the float64 255 v at least 1e-3 from a half-integer (asserted on the reference), so the
result is exact.
resize: (taps + 2) U sum |w x|, plus for bilinear / bicubic the coordinate term sum |dw/dt| |x| 4 U max(1, |src|)
(the source coordinate is formed in fp32; both modes are continuous across integer coordinates).
USM: stage-wise.  blur: (2 * 51 + 2) U sum |w x|; the mask is exact when the float64 ||residual| 255 - threshold| >=
1e-3 everywhere (asserted); output: the sum of the bounds of its terms.
JPEG: stage-wise, because rounding is discontinuous.  (a) the device's quantised coefficients equal rint of the
float64 pre-round coefficients except where those lie within delta of a half-integer, delta = 8 x the largest
pre-round error of an fp32 CPU replay of the case; at most 0.5 % of the coefficients may be so.  (b) the image against
a float64 decode of the device's own coefficients, bound (64 + 8) U sum |terms| / 255.
noise: gaussian 6 U (|img| + |noise terms|); poisson: levels, counts and vals exact on images kept 1e-3 from a rounding
tie, rates within U |rate|, the output within 8 U of its term sum."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from . import _degrade_ref as R
from . import _exact as E
from ._fp64 import U, _bits, _check

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _D():
    from basicsr4rs_amd.ops import degrade
    return degrade


@functools.lru_cache(None)
def _baboon():
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(GOLDEN, 'baboon.png')).convert('RGB')).copy()
    return torch.from_numpy(im).permute(2, 0, 1).float() / 255


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ filter2D

FILTER_SHAPES = [(2, 3, 24, 40), (2, 3, 37, 53), (1, 3, 33, 65)]  # the last: the 32 x 64 tile plus one row and column


def _kernel(kind, B, g):
    if kind == 'pad7':  # a 7 x 7 zero-padded to 21 (the dataset's kernels)
        k = torch.zeros(B, 21, 21)
        k[:, 7:14, 7:14] = torch.rand(B, 7, 7, generator=g)
    elif kind == 'pulse':
        k = torch.zeros(B, 21, 21)
        k[:, 10, 10] = 1
    else:
        k = torch.rand(B, kind, kind, generator=g) - 0.25  # mixed signs, a positive sum
    return k / k.sum((1, 2), keepdim=True) if kind not in ('pulse', ) else k


@pytest.mark.parametrize('shape', FILTER_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', [3, 7, 21, 'pad7', 'pulse'])
@pytest.mark.parametrize('shared', [False, True], ids=['per_sample', 'shared'])
def test_filter2d(cuda, shape, kind, shared):
    g = _gen(1, shape[2], str(kind), shared)
    x = torch.rand(shape, generator=g)
    kern = _kernel(kind, 1 if shared else shape[0], g)
    got = _D().filter2d(x.to(cuda), kern.to(cuda))
    if kind == 'pulse':
        assert torch.equal(_bits(got.cpu()), _bits(x)), 'the pulse kernel must return the input bit for bit'
        return
    ref, mag = R.filter2d(x, kern)
    k = kern.shape[-1]
    _check(got, ref, (k * k + 2) * U * mag, f'filter2d {shape} k {kind} shared {shared}')


@pytest.mark.parametrize('k', [3, 7, 21])
def test_filter2d_integer_grid(cuda, k):
    g = E.gen_for(f'filter2d grid {k}')
    x = E.grid((2, 3, 37, 53), -3, 3, 1.0, g)
    kern = E.grid((2, k, k), -3, 3, 0.25, g)
    ref, mag = R.filter2d(x, kern)
    E.assert_exactness([('x', x), ('kernel', kern), ('y', ref)], [('y', mag, 0.25)])
    got = _D().filter2d(x.float().to(cuda), kern.float().to(cuda))
    E.assert_bits(got, ref, f'filter2d integer grid k {k}', axes='ncyx')


def test_filter2d_round255(cuda):
    """x = (m + 0.1) / 255 and weights c / 64 summing to 1: 255 v = (an integer multiple of 1 / 64) + 0.1 up to the
    fp32 storage of x, at least 0.6 / 64 from a half-integer."""
    g = _gen(2)
    x = ((torch.randint(0, 255, (2, 3, 37, 53), generator=g).double() + 0.1) / 255).float()
    counts = torch.stack([torch.bincount(torch.randint(0, 49, (64, ), generator=g), minlength=49) for _ in range(2)])
    kern = (counts.double() / 64).view(2, 7, 7).float()
    ref, _ = R.filter2d(x, kern)
    want, margin = R.round255(ref)
    assert margin.min() >= 1e-3, margin.min()
    got = _D().filter2d(x.to(cuda), kern.to(cuda), round255=True)
    _check(got, want, 0, 'filter2d round255')
    assert len(torch.unique(want)) > 100


def test_filter2d_refusals(cuda):
    D = _D()
    with pytest.raises(RuntimeError, match='reflect pad'):
        D.filter2d(torch.rand(1, 3, 10, 40, device=cuda), torch.rand(1, 21, 21, device=cuda))
    with pytest.raises(ValueError, match='Wrong kernel size'):
        D.filter2d(torch.rand(1, 3, 24, 40, device=cuda), torch.rand(1, 4, 4, device=cuda))
    with pytest.raises(NotImplementedError):
        D.filter2d(torch.rand(1, 3, 24, 40), torch.rand(1, 3, 3))
    with pytest.raises(NotImplementedError, match='forward only'):
        D.filter2d(torch.rand(1, 3, 24, 40, device=cuda, requires_grad=True), torch.rand(1, 3, 3, device=cuda))


# -------------------------------------------------------------------------------------------------- resize

RESIZE_HOW = [('scale', 1.37), ('scale', 0.46), ('size', (13, 21)), ('size', (24, 40))]


def _resize_args(how, H, W):
    if how[0] == 'scale':
        (Ho, sh), (Wo, sw) = R.resize_geometry(H, scale_factor=how[1]), R.resize_geometry(W, scale_factor=how[1])
        return dict(scale_factor=how[1]), (Ho, Wo), (sh, sw)
    (Ho, sh), (Wo, sw) = R.resize_geometry(H, size=how[1][0]), R.resize_geometry(W, size=how[1][1])
    return dict(size=how[1]), (Ho, Wo), (sh, sw)


@pytest.mark.parametrize('mode', ['area', 'bilinear', 'bicubic'])
@pytest.mark.parametrize('how', RESIZE_HOW, ids=lambda h: f'{h[0]}{h[1]}')
def test_resize(cuda, mode, how):
    x = torch.randn(2, 3, 24, 40, generator=_gen(3))
    kw, out_hw, scales = _resize_args(how, 24, 40)
    got = _D().resize(x.to(cuda), mode=mode, **kw)
    ref, bound = R.resize(x, out_hw, scales, mode)
    _check(got, ref, bound, f'resize {mode} {how}')
    if mode == 'area':  # a ramp: every window sum is an exact integer, so one correctly rounded division remains
        ramp = torch.arange(24 * 40, dtype=torch.float32).view(1, 1, 24, 40).expand(2, 3, 24, 40).contiguous()
        got = _D().resize(ramp.to(cuda), mode=mode, **kw)
        _check(got, R.resize(ramp, out_hw, scales, mode)[0], 0, f'resize area ramp {how}')


@pytest.mark.parametrize('mode', ['area', 'bilinear'])
@pytest.mark.parametrize('scale', [0.5, 2])
def test_resize_integer_grid(cuda, mode, scale):
    x = E.grid((2, 3, 24, 40), -3, 3, 1.0, E.gen_for(f'resize {mode} {scale}'))
    ref, _ = R.resize(x, (int(24 * scale), int(40 * scale)), (1 / scale, 1 / scale), mode)
    E.assert_exactness([('y', ref)], [])
    got = _D().resize(x.float().to(cuda), scale_factor=scale, mode=mode)
    E.assert_bits(got, ref, f'resize integer grid {mode} x{scale}', axes='ncyx')


# ----------------------------------------------------------------------------------------------------- USM


@functools.lru_cache(None)
def _usm_case(name):
    if name == 'baboon':
        im = _baboon()
        x = torch.stack([im[:, 100:140, 100:156], im[:, 160:200, 120:176]]).contiguous()
    else:  # the smallest image a reflect pad of 25 allows
        x = torch.rand(1, 3, 26, 26, generator=torch.Generator().manual_seed(0))
    taps = R.gaussian_taps(51, 0)
    return x, taps, R.usm(x, taps, 0.5, 10)


@pytest.mark.parametrize('name', ['baboon', 'min26'])
def test_usm_stages(cuda, name):
    D = _D()
    x, taps, r = _usm_case(name)
    assert r.margin >= 1e-3, f'the case puts |residual| 255 within {r.margin:.2e} of the threshold'
    assert 0.05 < r.mask.mean() < 0.95
    t = taps.float().to(cuda)
    bb = (2 * 51 + 2) * U * r.blur_mag  # the fp32 storage of the taps is inside the + 2
    _check(D.sep_blur(x.to(cuda), t), r.blur, bb, f'usm {name} blur')
    y, res, mask = D.usm_sharp_raw(x.to(cuda), t, 0.5, 10)
    x64 = x.double()
    bres = bb + U * r.res.abs()
    _check(res, r.res, bres, f'usm {name} residual')
    _check(mask, r.mask, 0, f'usm {name} mask')
    bsoft = (2 * 51 + 2) * U * r.soft_mag
    bsharp = 0.5 * bres + 2 * U * (x64.abs() + 0.5 * r.res.abs())
    bout = (bsoft * (r.sharp - x64).abs() + r.soft.abs() * bsharp + 4 * U * ((r.soft * r.sharp).abs() +
                                                                             ((1 - r.soft) * x64).abs() + x64.abs()))
    _check(y, r.out, bout, f'usm {name} output')


def test_usm_module_launches_and_buffer(cuda):
    from basicsr4rs_amd.utils import ktrace
    from basicsr4rs_amd.utils.img_process_util import USMSharp
    x, taps, r = _usm_case('baboon')
    m = USMSharp()
    assert m.radius == 51 and tuple(m.kernel.shape) == (1, 51, 51)
    assert torch.equal(m.kernel[0], torch.outer(taps, taps).float()), 'kernel buffer: the float64 outer product in fp32'
    assert list(m.state_dict()) == ['kernel']
    m = m.to(cuda)
    ktrace.start()
    try:
        y = m(x.to(cuda))
    finally:
        recs = ktrace.stop()
    assert set(recs) == {'usm_sharp_kernels'} and recs['usm_sharp_kernels']['launches'] == 4, recs
    assert torch.equal(y, _D().usm_sharp(x.to(cuda), taps.float().to(cuda)))
    m5 = USMSharp(radius=5, sigma=1.5)
    assert torch.equal(m5.kernel[0], torch.outer(R.gaussian_taps(5, 1.5), R.gaussian_taps(5, 1.5)).float())
    with pytest.raises(RuntimeError, match='reflect pad'):
        m(torch.rand(1, 3, 25, 40, device=cuda))


# ---------------------------------------------------------------------------------------------------- JPEG

JPEG_CASES = {
    'pad40x56_q30_75': ((2, 3, 40, 56), [30.0, 75.0]),  # pads to 48 x 64
    'one_mb_q50': ((1, 3, 16, 16), 50),
    '32x48_q90': ((2, 3, 32, 48), 90),
}


@functools.lru_cache(None)
def _jpeg_case(name):
    shape, q = JPEG_CASES[name]
    if shape[2] == 40:
        im = _baboon()
        x = torch.stack([im[:, 100:140, 100:156], im[:, 160:200, 120:176]]).contiguous()
    else:
        x = torch.rand(shape, generator=torch.Generator().manual_seed(shape[3]))
    qt = torch.tensor(q if isinstance(q, list) else [float(q)] * shape[0], dtype=torch.float64)
    pre = R.jpeg_encode(x, qt)
    pre32 = R.jpeg_encode(x, qt, torch.float32)
    delta = 8 * max((a.double() - b).abs().max().item() for a, b in zip(pre32, pre))
    return x, q, qt, pre, delta


def _ambiguous(pre, delta):
    return [((p - torch.floor(p)) - 0.5).abs() <= delta for p in pre]


@pytest.mark.parametrize('name', list(JPEG_CASES))
@pytest.mark.parametrize('differentiable', [False, True], ids=['round', 'diff_round'])
def test_jpeg_stages(cuda, name, differentiable):
    D = _D()
    x, q, qt, pre, delta = _jpeg_case(name)
    B, _, H, W = x.shape
    quality = torch.tensor(q, device=cuda) if isinstance(q, list) else q
    y, coef = D.jpeg_raw(x.to(cuda), quality, differentiable=differentiable, want_coef=True)
    got = [c.double().cpu() for c in D.jpeg_coef_views(coef, B, H, W)]
    amb = _ambiguous(pre, delta)
    n_amb, total = sum(int(a.sum()) for a in amb), sum(a.numel() for a in amb)
    print(f'jpeg {name}: delta {delta:.3e}, ambiguous coefficients {n_amb} of {total} ({n_amb / total:.3%}, cap 0.5 %)')
    assert n_amb <= 0.005 * total
    for nm, g_, p, a in zip(('Y', 'Cb', 'Cr'), got, pre, amb):
        assert g_.shape == p.shape, (nm, g_.shape, p.shape)
        if differentiable:  # |d/dv (r + (v - r)^3)| <= 3/4 and the device's pre-round error is below delta
            want = R.diff_round(p)
            err = (g_ - want).abs()
            bound = delta + 4 * U * want.abs()
            print(f'  {nm}: max|err| {err[~a].max().item():.3e} (bound {delta:.3e} + 4 U |coef|)')
            assert (err[~a] <= bound[~a]).all()
        else:
            flips = (g_ != torch.round(p)) & ~a
            assert not flips.any(), f'{nm}: {int(flips.sum())} rounding flips outside the ambiguous coefficients'
            assert ((g_ - p).abs()[a] <= 0.5 + delta).all()
    # (b) the image from the device's own coefficients
    ref, mag = R.jpeg_decode(tuple(got), qt, H, W)
    _check(y, ref, (64 + 8) * U * mag, f'jpeg {name} decode')
    assert y.min() >= 0 and y.max() <= 1


def test_jpeg_interface(cuda):
    from basicsr4rs_amd.utils.diffjpeg import DiffJPEG, quality_to_factor
    x = torch.rand(2, 3, 40, 56, generator=_gen(9)).to(cuda)
    j = DiffJPEG(differentiable=False)
    q = torch.tensor([50.0, 50.0], device=cuda)
    keep = q.clone()
    a, b = j(x, quality=50), j(x, quality=q)
    assert torch.equal(_bits(a), _bits(b)), 'scalar and tensor quality must agree bit for bit'
    assert torch.equal(q, keep), "the caller's quality tensor must stay unchanged"
    assert torch.equal(j(x, quality=q), b)
    assert quality_to_factor(30) == 5000. / 30 / 100 and quality_to_factor(90) == 0.2
    r8 = _D().jpeg(x, 50, round255=True)
    want, margin = R.round255(b.double().cpu())
    ok = margin >= 1e-3
    assert torch.equal(r8.double().cpu()[ok], want.float().double()[ok]) and ok.double().mean() > 0.99
    with pytest.raises(NotImplementedError, match='forward only'):
        j(x.clone().requires_grad_(True), quality=50)
    with torch.no_grad():
        j(x.clone().requires_grad_(True), quality=50)
    with pytest.raises(NotImplementedError):
        j(x.cpu(), quality=50)


# --------------------------------------------------------------------------------------------------- noise

NOISE_SHAPE = (2, 3, 40, 56)


def test_gaussian_noise(cuda):
    g = _gen(11)
    img = torch.rand(NOISE_SHAPE, generator=g)
    normal, ngray = torch.randn(NOISE_SHAPE, generator=g), torch.randn(40, 56, generator=g)
    sigma, gray = torch.tensor([3.0, 25.0]), torch.tensor([0.0, 1.0])
    ref, mag = R.gaussian_noise(img, normal, ngray, sigma, gray)
    got = _D().gaussian_noise(img.to(cuda), sigma.to(cuda), gray.to(cuda), normal.to(cuda), ngray.to(cuda))
    _check(got, ref, 6 * U * mag, 'gaussian noise')
    assert (ref == 0).any() and (ref == 1).any(), 'the case must reach both clamps'
    # rounds=True: exact where the reference is not at a rounding tie
    want, margin = R.round255(torch.clamp(ref, 0, 1))
    got8 = _D().gaussian_noise(img.to(cuda), sigma.to(cuda), gray.to(cuda), normal.to(cuda), ngray.to(cuda), rounds=True)
    ok = margin >= 1e-3
    assert torch.equal(got8.double().cpu()[ok], want.float().double()[ok]) and ok.double().mean() > 0.99


def _levels_image(kind, g):
    """[2, 3, 40, 56] with 64 distinct 8-bit levels in sample 0 and 65 in sample 1 (vals 64 and 128), every
    255 v (channels and gray) at least 1e-3 from a half-integer."""
    B, _, H, W = NOISE_SHAPE
    out = []
    for n, nlev in enumerate((64, 65)):
        if kind == 'gray':  # r = g = b on the 1 / 255 grid with jitter <= 0.2 / 255
            m = torch.randint(0, nlev, (1, H, W), generator=g).expand(3, H, W) * 3
            jit = (torch.rand(1, H, W, generator=g) * 0.4 - 0.2).expand(3, H, W)
        else:
            m = torch.randint(0, nlev, (3, H, W), generator=g) * 3
            jit = torch.rand(3, H, W, generator=g) * 0.8 - 0.4
        v = ((m.double() + jit.double()) / 255).float()
        for _ in range(50):  # redraw the jitter of any pixel too close to a rounding tie
            _, mc = R.round255(v.double())
            _, mg = R.round255(R.gray_of(v.double()[None])[0])
            bad = (mc < 1e-3) | (mg < 1e-3).expand(3, H, W)
            if not bad.any():
                break
            bad = bad.any(0, keepdim=True).expand(3, H, W)
            nj = (torch.rand(1 if kind == 'gray' else 3, H, W, generator=g) * 0.4 - 0.2).expand(3, H, W)
            v = torch.where(bad, ((m.double() + nj.double()) / 255).float(), v)
        out.append(v)
    return torch.stack(out)


@pytest.mark.parametrize('kind', ['gray', 'colour'])
def test_poisson_noise(cuda, kind):
    D = _D()
    g = _gen(13, kind)
    img = _levels_image(kind, g)
    lv = R.poisson_levels(img)
    assert lv.margin >= 1e-3, lv.margin
    assert lv.count_c.tolist() == [64, 65] and lv.vals[:, 0].tolist() == [64.0, 128.0], (lv.count_c, lv.vals)
    rate_c, rate_g, vals, bitmap = D.poisson_levels(img.to(cuda))
    bits = bitmap.cpu().numpy().view(np.uint32)
    counts = np.array([[sum(bin(int(w)).count('1') for w in bits[n, c]) for c in range(2)] for n in range(2)])
    assert counts[:, 0].tolist() == lv.count_c.tolist() and counts[:, 1].tolist() == lv.count_g.tolist(), counts
    assert torch.equal(vals.double().cpu(), lv.vals)
    _check(rate_c, lv.rate_c, U * lv.rate_c.abs() + 1e-300, f'poisson {kind} colour rates')
    _check(rate_g, lv.rate_g, U * lv.rate_g.abs() + 1e-300, f'poisson {kind} gray rates')
    draw_c = torch.poisson(lv.rate_c.float(), generator=g)
    draw_g = torch.poisson(lv.rate_g.float(), generator=g)
    scale, gray = torch.tensor([0.7, 2.5]), torch.tensor([0.0, 1.0])
    ref, mag = R.poisson_noise(img, lv, draw_c, draw_g, scale, gray)
    got = D.poisson_noise(img.to(cuda), scale.to(cuda), gray.to(cuda), draw_c.to(cuda), draw_g.to(cuda),
                          levels=(rate_c, rate_g, vals, bitmap))
    _check(got, ref, 8 * U * mag, f'poisson {kind} output')
    # the gray sample carries one noise field on its three channels
    n1 = got[1].double().cpu() - img[1].double()
    inner = (ref[1] > 0).all(0) & (ref[1] < 1).all(0)
    assert inner.any() and (n1[0] - n1[1]).abs()[inner].max() < 1e-6


def test_random_noise_statistics(cuda):
    """Mean and variance of the noise the public random_add_*_pt functions add, over 2 * 3 * 40 * 56 samples, within
    5 standard errors of 0 and of sigma^2 / 255^2 (Gaussian) or scale^2 level / (255 vals) (Poisson, standardised per
    pixel; its squared noise has variance 2 + 1 / lambda)."""
    from basicsr4rs_amd.data import degradations as G
    torch.manual_seed(1234)
    n = 2 * 3 * 40 * 56
    img = torch.full(NOISE_SHAPE, 0.5, device=cuda)
    noise = (G.random_add_gaussian_noise_pt(img, sigma_range=(10, 10), gray_prob=0, clip=False) - img).double().cpu()
    s = 10 / 255
    print(f'gaussian: mean {noise.mean().item():.3e} (5 se {5 * s / n**0.5:.3e}), var {noise.var().item():.4e} vs {s * s:.4e}')
    assert abs(noise.mean().item()) <= 5 * s / n**0.5
    assert abs(noise.var().item() - s * s) <= 5 * s * s * (2 / (n - 1))**0.5
    g = torch.Generator().manual_seed(5)
    lev = torch.randint(50, 250, NOISE_SHAPE, generator=g)
    img = ((lev.double() + 0.2) / 255).float()
    lv = R.poisson_levels(img)
    assert lv.vals[:, 0].tolist() == [256.0, 256.0]
    out = G.random_add_poisson_noise_pt(img.to(cuda), scale_range=(1.5, 1.5), gray_prob=0, clip=False)
    z = (out.double().cpu() - img.double()) / (1.5 * torch.sqrt(lv.qc / 256))
    lam_min = 50 / 255 * 256
    print(f'poisson: mean z {z.mean().item():.3e}, mean z^2 {(z * z).mean().item():.4f}')
    assert abs(z.mean().item()) <= 5 / n**0.5
    assert abs((z * z).mean().item() - 1) <= 5 * ((2 + 1 / lam_min) / n)**0.5
    with pytest.raises(NotImplementedError):
        G.random_add_gaussian_noise_pt(img, sigma_range=(1, 2))
