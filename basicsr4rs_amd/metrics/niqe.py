"""NIQE, the no-reference quality score of the fork's remote-sensing configs (mirror of
basicsr/metrics/niqe.py:13-231; "Making a 'Completely Blind' Image Quality Analyzer", Mittal et al.).

numpy only.  The module is cut where the device path (csrc/niqe.hip, ops/metrics.py) joins it:

  niqe_plane         the image plane the score is taken from: float32 [H, W] of integer values in
                     [0, 255], cropped and truncated to whole 96 x 96 blocks
  niqe_moments       per scale, block and map the six sums the AGGD fits need (float64)
  niqe_from_moments  the fits, the 36 features per block, the Gaussian model and the score

Host and device share ``niqe_from_moments``, and with it every discontinuous step: the argmin over the
gamma table and the NaN handling.  The reference refits the 9801-entry gamma table in every fit
(niqe.py:24-26); here it is built once per process.

Where this differs from the reference in arithmetic (not in meaning): the block sums are taken in float64
(the reference's ``np.mean`` of float32 arrays sums pairwise in float32), and both passes of the half-size
resample accumulate their eight exact taps in float64 before the float32 store (the reference's torch ``mv``
leaves the order open).  Both are closer to the exact value than the reference is.

The score needs the fork's ``niqe_pris_params.npz`` (``mu_pris_param`` [1, 36], ``cov_pris_param`` [36, 36],
``gaussian_window`` [7, 7]), which this package does not ship.  It is looked for in this order:
  1. the ``params_path`` key of the metric entry;
  2. the environment variable ``BASICSR4RS_NIQE_PARAMS``;
  3. ``metrics/niqe_pris_params.npz`` inside an installed ``basicsr`` package (found, not imported).
"""
import importlib.util
import math
import os

import numpy as np

from ..utils.registry import METRIC_REGISTRY
from .psnr_ssim import _to_y

BLOCK = 96
PARAMS_ENV = 'BASICSR4RS_NIQE_PARAMS'
# half-size antialiased bicubic (basicsr/utils/matlab_functions.py:16-82 at scale 0.5, even length): output o
# reads inputs 2o-3 .. 2o+4 with 0.5 * cubic(a = -0.5) at |x| = 1.75, 1.25, 0.75, 0.25; exact in binary
HALF_TAPS = (-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875)
# the five maps of a block: itself and its products with the block rolled by these (rows, columns)
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
# the six moments of a map, in the order of niqe_moments' last axis
N_NEG, SS_NEG, N_POS, SS_POS, SUM_ABS, SUM_SQ = range(6)

_PARAMS = {}
_TABLE = None


def load_niqe_params(params_path=None):
    """``(mu_pris_param, cov_pris_param, gaussian_window)`` from the first of the three places in the module
    docstring that names a file; cached per path."""
    tried = []
    path = None
    for source, cand in (('params_path', params_path), (f'${PARAMS_ENV}', os.environ.get(PARAMS_ENV))):
        if cand:
            if os.path.isfile(cand):
                path = cand
                break
            tried.append(f'{source}={cand!r} (no such file)')
        else:
            tried.append(f'{source} (not set)')
    if path is None:
        try:
            spec = importlib.util.find_spec('basicsr')
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.submodule_search_locations:
            cand = os.path.join(list(spec.submodule_search_locations)[0], 'metrics', 'niqe_pris_params.npz')
            if os.path.isfile(cand):
                path = cand
            else:
                tried.append(f'{cand!r} (no such file)')
        else:
            tried.append('metrics/niqe_pris_params.npz of an installed basicsr package (basicsr is not installed)')
    if path is None:
        raise FileNotFoundError('NIQE needs niqe_pris_params.npz; looked for it in: ' + '; '.join(tried))
    path = os.path.abspath(path)
    if path not in _PARAMS:
        with np.load(path) as p:
            _PARAMS[path] = (np.array(p['mu_pris_param'], dtype=np.float64),
                             np.array(p['cov_pris_param'], dtype=np.float64),
                             np.array(p['gaussian_window'], dtype=np.float64))
    return _PARAMS[path]


def gamma_table():
    """The AGGD shape grid and what the fits read from it (niqe.py:24-26, 36-37, 63), once per process:
    ``gam``, ``r_gam = G(2/g)^2 / (G(1/g) G(3/g))``, ``sqrt(G(1/g) / G(3/g))`` and ``G(2/g) / G(1/g)``."""
    global _TABLE
    if _TABLE is None:
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        g = np.vectorize(math.gamma, otypes=[np.float64])
        r_gam = np.square(g(rec * 2)) / (g(rec) * g(rec * 3))
        g1, g2, g3 = g(1 / gam), g(2 / gam), g(3 / gam)
        _TABLE = (gam, r_gam, np.sqrt(g1 / g3), g2 / g1)
    return _TABLE


def niqe_plane(img, crop_border=0, input_order='HWC', convert_to='y', input_bands=None, band=None):
    """preprocess_for_niqe (niqe.py:150-175) and niqe's block crop (niqe.py:100-103): float32, HWC, the
    ``input_bands`` then the ``band`` selection, Y of a 3-channel (BGR) selection, border crop, round,
    top-left truncation to multiples of 96."""
    img = np.asarray(img).astype(np.float32)
    if input_order != 'HW':
        if input_order not in ('HWC', 'CHW'):
            raise ValueError(f"Wrong input_order {input_order}. Supported input_orders are 'HWC' and 'CHW'")
        if img.ndim == 2:
            img = img[..., None]
        elif input_order == 'CHW':
            img = img.transpose(1, 2, 0)
        if input_bands is not None:
            img = img[..., list(input_bands)]
        if band is not None:
            img = img[..., band]
        if convert_to == 'y':
            img = _to_y(img)
        elif convert_to == 'gray':
            raise NotImplementedError("NIQE convert_to='gray' is OpenCV's BGR2GRAY, and OpenCV is not a "
                                      "dependency of this package; use convert_to='y' or a band")
        img = np.squeeze(img)
    if crop_border > 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border]
    img = img.round()
    assert img.ndim == 2, 'Input image must be a gray or Y (of YCbCr) image with shape (h, w).'
    h, w = img.shape
    return np.ascontiguousarray(img[:h // BLOCK * BLOCK, :w // BLOCK * BLOCK])


def filter7(img, window):
    """scipy.ndimage.convolve(img, window, mode='nearest') for a float32 image and a 7 x 7 window: replicate
    borders, the 49 products summed in float64 in the window's raster order, stored as float32."""
    h, w = img.shape
    k = np.asarray(window, dtype=np.float64)[::-1, ::-1]  # convolve = correlate with the flipped window
    pad = np.pad(img.astype(np.float64), 3, mode='edge')
    acc = np.zeros((h, w), dtype=np.float64)
    for a in range(7):
        for b in range(7):
            acc += pad[a:a + h, b:b + w] * k[a, b]
    return acc.astype(np.float32)


def mscn(img, window):
    """The normalised map of niqe.py:107-110 in the reference's float32 steps."""
    mu = filter7(img, window)
    sigma = np.sqrt(np.abs(filter7(np.square(img), window) - np.square(mu)))
    return (img - mu) / (sigma + np.float32(1))


def _half_axis0(x, store=np.float32):
    """One pass of the half-size resample along axis 0 (even length): reflected borders with the edge
    repeated, float64 accumulation over the eight taps, float32 store."""
    n = x.shape[0]
    o = np.arange(n // 2)
    acc = np.zeros((n // 2,) + x.shape[1:], dtype=np.float64)
    for k, wk in enumerate(HALF_TAPS):
        idx = 2 * o - 3 + k
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
        acc += x[idx].astype(np.float64) * wk
    return acc.astype(store)


def half_size(img, store=np.float32):
    """``imresize(img / 255, 0.5, antialiasing=True) * 255`` of niqe.py:122-124 for an even-sized float32
    plane: the pass along the height first, float32 between the passes, no rounding of the result.
    ``store=np.float64`` keeps every intermediate in float64 (for checks of the taps and offsets alone)."""
    x = img.astype(store) / store(255)
    x = _half_axis0(x, store)
    x = np.ascontiguousarray(_half_axis0(np.ascontiguousarray(x.T), store).T)
    return x * store(255)


def block_maps(block):
    """The five float32 maps of a block (niqe.py:58-61): itself and its products with the circular rolls."""
    return [block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]


def map_moments(x):
    """The six sums an AGGD fit (niqe.py:28-32) needs of a float32 map, in float64."""
    x = x.reshape(-1).astype(np.float64)
    neg, pos = x[x < 0], x[x > 0]
    return (neg.size, np.sum(neg * neg), pos.size, np.sum(pos * pos), np.sum(np.abs(x)), np.sum(x * x))


def niqe_moments(plane, window, return_mscn=False):
    """Moments ``[2 scales][block rows][block columns][5 maps][6]`` (float64) of a plane from niqe_plane:
    blocks of 96 x 96 at scale 1 and 48 x 48 of the half-size plane at scale 2."""
    h, w = plane.shape
    bh, bw = h // BLOCK, w // BLOCK
    out = np.zeros((2, bh, bw, 5, 6), dtype=np.float64)
    img = plane.astype(np.float32)
    maps = []
    for s in range(2):
        n = mscn(img, window)
        maps.append(n)
        bs = BLOCK >> s
        for i in range(bh):
            for j in range(bw):
                for m, x in enumerate(block_maps(n[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs])):
                    out[s, i, j, m] = map_moments(x)
        if s == 0:
            img = half_size(img)
    return (out, maps) if return_mscn else out


def aggd_fit(mom, count):
    """estimate_aggd_param (niqe.py:13-38) from moments [..., 6] of ``count`` elements each: the index into
    the gamma table and the two scale parameters.  An empty side gives NaN scale parameters (numpy's empty
    mean) and a NaN matching value, whose argmin is index 0, as in the reference."""
    gam, r_gam, beta_scale, _ = gamma_table()
    mom = np.asarray(mom, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        left_std = np.sqrt(mom[..., SS_NEG] / mom[..., N_NEG])
        right_std = np.sqrt(mom[..., SS_POS] / mom[..., N_POS])
        gammahat = left_std / right_std
        rhat = (mom[..., SUM_ABS] / count)**2 / (mom[..., SUM_SQ] / count)
        rhatnorm = (rhat * (gammahat**3 + 1) * (gammahat + 1)) / ((gammahat**2 + 1)**2)
        flat = rhatnorm.reshape(-1)
        pos = np.array([np.argmin((r_gam - v)**2) for v in flat], dtype=np.int64).reshape(rhatnorm.shape)
        beta_l = left_std * beta_scale[pos]
        beta_r = right_std * beta_scale[pos]
    return pos, beta_l, beta_r


def features_from_moments(mom, count):
    """compute_feature (niqe.py:41-65): 18 features per block from its moments [..., 5, 6]."""
    gam, _, _, mean_scale = gamma_table()
    pos, beta_l, beta_r = aggd_fit(mom, count)
    alpha = gam[pos]
    feat = [alpha[..., 0], (beta_l[..., 0] + beta_r[..., 0]) / 2]
    for m in range(1, 5):
        feat += [alpha[..., m], (beta_r[..., m] - beta_l[..., m]) * mean_scale[pos[..., m]], beta_l[..., m],
                 beta_r[..., m]]
    return np.stack(feat, axis=-1)


def niqe_from_moments(moments, mu_pris, cov_pris):
    """The score (niqe.py:126-141) from niqe_moments' array: features per block in the reference's block
    order (column index outer, row index inner), nanmean, covariance of the rows without NaN, pseudo-inverse
    of the pooled covariance, quadratic form, sqrt.  Fewer than two clean rows give NaN."""
    moments = np.asarray(moments, dtype=np.float64)
    feats = []
    for s in range(2):
        f = features_from_moments(moments[s], float((BLOCK >> s)**2))  # [bh, bw, 18]
        feats.append(f.transpose(1, 0, 2).reshape(-1, 18))
    distparam = np.concatenate(feats, axis=1)
    clean = distparam[~np.isnan(distparam).any(axis=1)]
    if clean.shape[0] < 2:
        return float('nan')
    mu_distparam = np.nanmean(distparam, axis=0)  # no column is all NaN: there are clean rows
    cov_distparam = np.cov(clean, rowvar=False)
    invcov = np.linalg.pinv((cov_pris + cov_distparam) / 2)
    d = mu_pris - mu_distparam
    with np.errstate(invalid='ignore'):
        quality = np.sqrt(np.matmul(np.matmul(d, invcov), np.transpose(d)))
    return float(np.squeeze(quality))


def niqe(plane, mu_pris, cov_pris, window):
    """NIQE of a plane from niqe_plane."""
    if plane.shape[0] < BLOCK or plane.shape[1] < BLOCK:
        return float('nan')  # no block: the reference's covariance of an empty feature table
    return niqe_from_moments(niqe_moments(plane, window), mu_pris, cov_pris)


@METRIC_REGISTRY.register()
def calculate_niqe(img, crop_border, input_order='HWC', convert_to='y', params_path=None, **kwargs):
    """NIQE of a [0, 255] image (BGR when it has three channels), niqe.py:178-211.  ``img2`` and any other
    key of the metric entry are ignored."""
    mu, cov, window = load_niqe_params(params_path)
    return niqe(niqe_plane(img, crop_border, input_order, convert_to), mu, cov, window)


@METRIC_REGISTRY.register()
def calculate_rs_niqe(img, crop_border, input_order='HWC', convert_to='y', input_bands=(2, 1, 0), params_path=None,
                      **kwargs):
    """NIQE of the ``input_bands`` of a multi-band image, read as BGR (niqe.py:214-219)."""
    mu, cov, window = load_niqe_params(params_path)
    return niqe(niqe_plane(img, crop_border, input_order, convert_to, input_bands=input_bands), mu, cov, window)


@METRIC_REGISTRY.register()
def calculate_niqe_band(img, crop_border, band, input_order='HWC', params_path=None, **kwargs):
    """NIQE of one band as it is (niqe.py:222-226)."""
    mu, cov, window = load_niqe_params(params_path)
    return niqe(niqe_plane(img, crop_border, input_order, convert_to=None, band=band), mu, cov, window)


@METRIC_REGISTRY.register()
def calculate_niqe_none(**kwargs):
    """The fork's placeholder entry (niqe.py:229-231)."""
    return -1
