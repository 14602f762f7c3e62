"""Host NIQE (metrics/niqe.py) pinned to the reference (basicsr/metrics/niqe.py) without executing it:

* known answer: the reference's docstring gives 5.7295763 for ``calculate_niqe(img, crop_border=0)`` on its
  baboon picture (MATLAB R2021a: 5.72957338); the fixture is the fork's test_scripts/data/baboon.png
  (480 x 492).  Bound 1e-4: about 30 times the gap between those two values and well below one unit of the
  third decimal.  This implementation gives 5.7295608 (2e-5 off): the picture is the right one;
* the 7 x 7 filter equals scipy.ndimage.convolve(mode='nearest') on float32 input exactly;
* the half-size step: the eight exact taps, constants preserved, interior pixels equal torch's antialiased
  bicubic to float32 rounding, borders equal a direct loop over the reflected taps;
* the AGGD fit recovers the shape of generalised-Gaussian samples; an empty side gives NaN features and the
  row is dropped;
* registry, parameter-file lookup order and the error paths.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from basicsr4rs_amd.metrics import calculate_metric
from basicsr4rs_amd.metrics import niqe as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PARAMS = os.path.join(GOLDEN, 'niqe_pris_params.npz')


def baboon_bgr():
    from PIL import Image
    rgb = np.array(Image.open(os.path.join(GOLDEN, 'baboon.png')).convert('RGB'))
    assert rgb.shape == (480, 492, 3)
    return np.ascontiguousarray(rgb[..., ::-1])


def test_known_answer_baboon():
    v = calculate_metric(dict(img=baboon_bgr(), img2=None), dict(type='calculate_niqe', crop_border=0, params_path=PARAMS))
    print(f'NIQE baboon {v!r}, reference docstring 5.7295763, MATLAB 5.72957338')
    assert abs(v - 5.7295763) <= 1e-4


def test_filter7_equals_scipy_convolve():
    ndimage = pytest.importorskip('scipy.ndimage')
    window = Q.load_niqe_params(PARAMS)[2]
    rng = np.random.default_rng(0)
    for shape, scale in (((96, 192), 255.0), ((101, 57), 255.0), ((48, 96), 1.0)):
        img = (rng.random(shape) * scale).astype(np.float32)
        if scale == 255.0:
            img = img.round()
        for x in (img, np.square(img)):
            want = ndimage.convolve(x, window, mode='nearest')
            got = Q.filter7(x, window)
            assert got.dtype == want.dtype == np.float32
            assert np.array_equal(got, want), np.abs(got - want).max()


def test_half_size_taps_and_constant():
    assert Q.HALF_TAPS == (-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625,
                           -0.01171875)
    assert sum(Q.HALF_TAPS) == 1.0
    # 0.5 * cubic(a = -0.5) at |x| = 1.75, 1.25, 0.75, 0.25
    cubic = lambda x: 1.5 * x**3 - 2.5 * x**2 + 1 if x <= 1 else -0.5 * x**3 + 2.5 * x**2 - 4 * x + 2  # noqa: E731
    assert [0.5 * cubic(x) for x in (1.75, 1.25, 0.75, 0.25)] == list(Q.HALF_TAPS[:4])
    for level in (0.0, 255.0, 51.0):  # level / 255 * 255 is exact for these
        out = Q.half_size(np.full((96, 192), level, np.float32))
        assert out.shape == (48, 96) and out.dtype == np.float32
        assert np.array_equal(out, np.full((48, 96), level, np.float32)), level


def _torch_half(img):
    return torch.nn.functional.interpolate(torch.from_numpy(img)[None, None].double(), scale_factor=0.5, mode='bicubic',
                                           antialias=True, align_corners=False)[0, 0].numpy()


def test_half_size_interior_matches_torch_antialias():
    """Interior pixels (at least 4 from every edge, where no border rule is involved) against torch's
    antialiased bicubic evaluated in float64, on a [0, 255] scale.

    1e-5 is below the float32 spacing of values above 128 (2^-16 = 1.5e-5), and half_size stores float32
    four times (/ 255, between the passes, the result, * 255), as the reference does.  So the taps and
    offsets are held to 1e-5 with the stores in float64 (measured 1e-13), and the float32 path to what its
    four roundings of values up to 255 * sum|taps| = 303 allow, 4 * 2^-24 * 303 = 7.2e-5 (measured 2.1e-5)."""
    rng = np.random.default_rng(1)
    img = (rng.random((96, 192)) * 255).astype(np.float32)
    ref = _torch_half(img)
    d = np.abs(Q.half_size(img, store=np.float64) - ref)[4:-4, 4:-4]
    print(f'half-size interior max |diff| vs torch antialiased bicubic, float64 stores: {d.max():.3e}')
    assert d.max() <= 1e-5
    got = Q.half_size(img)
    assert got.dtype == np.float32
    d = np.abs(got.astype(np.float64) - ref)[4:-4, 4:-4]
    print(f'half-size interior max |diff| vs torch antialiased bicubic, float32 stores: {d.max():.3e}')
    assert d.max() <= 4 * 2.0**-24 * 255 * sum(abs(t) for t in Q.HALF_TAPS)


def test_half_size_borders_direct_loop():
    rng = np.random.default_rng(2)
    img = (rng.random((96, 192)) * 255).round().astype(np.float32)
    got = Q.half_size(img)

    def refl(i, n):
        return -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)

    x = img / np.float32(255)
    h, w = x.shape
    tmp = np.zeros((h // 2, w), np.float32)
    for o in range(h // 2):
        acc = np.zeros(w, np.float64)
        for k, t in enumerate(Q.HALF_TAPS):
            acc += t * x[refl(2 * o - 3 + k, h)].astype(np.float64)
        tmp[o] = acc.astype(np.float32)
    want = np.zeros((h // 2, w // 2), np.float32)
    for o in range(w // 2):
        acc = np.zeros(h // 2, np.float64)
        for k, t in enumerate(Q.HALF_TAPS):
            acc += t * tmp[:, refl(2 * o - 3 + k, w)].astype(np.float64)
        want[:, o] = acc.astype(np.float32)
    want = want * np.float32(255)
    assert refl(-1, 96) == 0 and refl(-3, 96) == 2 and refl(96, 96) == 95 and refl(99, 96) == 92
    assert np.array_equal(got, want)


def _gg_samples(shape, n, rng):
    """Symmetric generalised Gaussian, density ~ exp(-|x|^shape): |x| = G^(1/shape), G ~ Gamma(1/shape)."""
    g = rng.gamma(1.0 / shape, 1.0, n)
    return (g**(1.0 / shape) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


@pytest.mark.parametrize('shape', [1.0, 2.0])
def test_aggd_fit_recovers_shape(shape):
    x = _gg_samples(shape, 200000, np.random.default_rng(int(shape * 10)))
    mom = np.array(Q.map_moments(x), dtype=np.float64)
    pos, beta_l, beta_r = Q.aggd_fit(mom, float(x.size))
    alpha = Q.gamma_table()[0][pos]
    print(f'shape {shape}: alpha {alpha:.3f}, beta_l {beta_l:.4f}, beta_r {beta_r:.4f}')
    assert abs(alpha - shape) <= 0.05
    assert abs(beta_l / beta_r - 1) <= 0.02  # symmetric


def test_empty_side_gives_nan_and_row_is_dropped():
    mu, cov, window = Q.load_niqe_params(PARAMS)
    rng = np.random.default_rng(3)
    plane = (rng.random((96, 288)) * 255).round().astype(np.float32)
    mom = Q.niqe_moments(plane, window)
    assert mom.shape == (2, 1, 3, 5, 6) and mom.dtype == np.float64
    full = Q.niqe_from_moments(mom, mu, cov)
    assert np.isfinite(full)
    broken = mom.copy()
    broken[0, 0, 1, 0, Q.N_NEG] = 0  # no negative element in the first map of the middle block
    broken[0, 0, 1, 0, Q.SS_NEG] = 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')  # no warning spam
        feat = Q.features_from_moments(broken[0], 96.0 * 96.0)
        assert np.isnan(feat[0, 1]).any() and not np.isnan(feat[0, 0]).any() and not np.isnan(feat[0, 2]).any()
        dropped = Q.niqe_from_moments(broken, mu, cov)
        two = Q.niqe_from_moments(mom[:, :, [0, 2]], mu, cov)
    assert np.isfinite(dropped)
    # the covariance is of the two clean rows; the mean still sees the broken row's finite features
    assert dropped != full and abs(dropped - two) / two < 0.5
    # a constant block (with a margin wider than the reach of the window and of the resample): every count
    # is zero at both scales
    plane[:, 96 - 12:192 + 12] = 77
    mom_c = Q.niqe_moments(plane, window)
    assert (mom_c[:, 0, 1, :, Q.N_NEG] == 0).all() and (mom_c[:, 0, 1, :, Q.N_POS] == 0).all()
    assert (mom_c[:, 0, 1, :, Q.SUM_SQ] == 0).all()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.isfinite(Q.niqe_from_moments(mom_c, mu, cov))


def test_registry_and_parameters(tmp_path, monkeypatch):
    rng = np.random.default_rng(4)
    img = (rng.random((100, 200, 4)) * 255).astype(np.uint8)
    data = dict(img=img, img2=None)
    monkeypatch.delenv(Q.PARAMS_ENV, raising=False)
    base = dict(crop_border=2, params_path=PARAMS)
    a = calculate_metric(data, dict(type='calculate_rs_niqe', **base))
    assert np.isfinite(a)
    # img2 is ignored
    assert calculate_metric(dict(img=img, img2=img[::-1]), dict(type='calculate_rs_niqe', **base)) == a
    assert calculate_metric(data, dict(type='calculate_rs_niqe', input_bands=[2, 1, 0], **base)) == a
    assert calculate_metric(data, dict(type='calculate_rs_niqe', input_bands=[0, 1, 2], **base)) != a
    b = calculate_metric(data, dict(type='calculate_niqe_band', band=3, **base))
    assert np.isfinite(b) and b != a
    assert calculate_metric(data, dict(type='calculate_rs_niqe', input_bands=[3], **base)) == b  # one band: / 255 * 255
    assert calculate_metric(dict(img=img[..., :3], img2=None), dict(type='calculate_niqe', **base)) == \
        calculate_metric(data, dict(type='calculate_rs_niqe', input_bands=[0, 1, 2], **base))
    assert calculate_metric(dict(img=img.transpose(2, 0, 1), img2=None),
                            dict(type='calculate_niqe_band', band=3, input_order='CHW', **base)) == b
    assert calculate_metric(data, dict(type='calculate_niqe_none')) == -1

    # lookup order: params_path, then the environment variable, then an installed basicsr; none: an error
    # that names all three
    monkeypatch.setattr(Q.importlib.util, 'find_spec', lambda name: None)
    with pytest.raises(FileNotFoundError, match='params_path.*BASICSR4RS_NIQE_PARAMS.*basicsr'):
        calculate_metric(data, dict(type='calculate_niqe_band', band=0, crop_border=0))
    monkeypatch.setenv(Q.PARAMS_ENV, PARAMS)
    assert calculate_metric(data, dict(type='calculate_niqe_band', band=3, crop_border=2)) == b
    # a params_path wins over the variable: other pristine parameters, another score
    with np.load(PARAMS) as p:
        other = {k: p[k] for k in p.files}
    other['mu_pris_param'] = other['mu_pris_param'] * 1.5
    np.savez(tmp_path / 'other.npz', **other)
    c = calculate_metric(data, dict(type='calculate_niqe_band', band=3, crop_border=2,
                                    params_path=str(tmp_path / 'other.npz')))
    assert np.isfinite(c) and c != b
    monkeypatch.setenv(Q.PARAMS_ENV, str(tmp_path / 'missing.npz'))
    with pytest.raises(FileNotFoundError, match='missing.npz'):
        calculate_metric(data, dict(type='calculate_niqe_band', band=3, crop_border=2))
    assert calculate_metric(data, dict(type='calculate_niqe_band', band=3, **base)) == b
    monkeypatch.undo()
    monkeypatch.delenv(Q.PARAMS_ENV, raising=False)
    # a basicsr package on the path is located, not imported (its __init__ would raise)
    pkg = tmp_path / 'site' / 'basicsr'
    (pkg / 'metrics').mkdir(parents=True)
    (pkg / '__init__.py').write_text('raise RuntimeError("imported")\n')
    with np.load(PARAMS) as p:
        np.savez(pkg / 'metrics' / 'niqe_pris_params.npz', **{k: p[k] for k in p.files})
    monkeypatch.syspath_prepend(str(tmp_path / 'site'))
    assert calculate_metric(data, dict(type='calculate_niqe_band', band=3, crop_border=2)) == b
    assert 'basicsr' not in sys.modules

    with pytest.raises(NotImplementedError, match='OpenCV'):
        calculate_metric(dict(img=img[..., :3], img2=None), dict(type='calculate_niqe', convert_to='gray', **base))
    # a single 96 x 96 block: one feature row, no covariance
    one = calculate_metric(dict(img=img[:100, :100], img2=None), dict(type='calculate_niqe_band', band=0, **base))
    assert np.isnan(one)


def test_gamma_table_built_once():
    assert Q.gamma_table() is Q.gamma_table()
    gam, r_gam = Q.gamma_table()[:2]
    assert gam.shape == r_gam.shape == (9801,) and gam[0] == 0.2 and abs(gam[-1] - 10.0) < 1e-9
    assert (np.diff(r_gam) > 0).all()
