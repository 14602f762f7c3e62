"""Degradation building blocks of Real-ESRGAN (basicsr/data/degradations.py).

Host side (numpy, run in the dataset workers): the blur-kernel generators of degradations.py:16-416, with the
reference's order of ``np.random`` / ``random`` draws, so a seeded worker produces the reference's kernels.
Device side (csrc/degrade.hip): the four ``*_noise_pt`` families of degradations.py:460-553, 609-723.  The normal and
Poisson draws stay with torch's device generator; the per-sample count of distinct 8-bit levels that the Poisson
branch needs is formed on the device, so nothing comes back to the host.  The gray noise is therefore always drawn
and mixed by the per-sample flags (the reference first sums the flags on the host to decide whether to draw it);
with all flags 0 the result is the same, only the generator advances further.

Not provided: the numpy noise functions and ``add_jpg_compression`` (cv2), and the skewed Gaussian (``cdf2``), which no
kernel list of the reference's option files names.
"""
import math
import random

import numpy as np
import torch
from scipy import special

from ..ops import degrade as D

# ------------------------------------------------------------------------------------------- blur kernels


def sigma_matrix2(sig_x, sig_y, theta):
    """The covariance U diag(sig_x^2, sig_y^2) U^T of a Gaussian rotated by ``theta`` (radians)."""
    d = np.array([[sig_x**2, 0], [0, sig_y**2]])
    u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    return np.dot(u, np.dot(d, u.T))


def mesh_grid(kernel_size):
    """(xy [K, K, 2], xx, yy [K, K]): integer coordinates centred at zero."""
    ax = np.arange(-kernel_size // 2 + 1., kernel_size // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    xy = np.stack((xx, yy), axis=-1)
    return xy, xx, yy


def _quadratic_form(kernel_size, sig_x, sig_y, theta, grid, isotropic):
    """g^T Sigma^-1 g at every grid point."""
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    if isotropic:
        sigma = np.array([[sig_x**2, 0], [0, sig_x**2]])
    else:
        sigma = sigma_matrix2(sig_x, sig_y, theta)
    return np.sum(np.dot(grid, np.linalg.inv(sigma)) * grid, 2)


def pdf2(sigma_matrix, grid):
    """The un-normalised bivariate Gaussian density on ``grid``."""
    return np.exp(-0.5 * np.sum(np.dot(grid, np.linalg.inv(sigma_matrix)) * grid, 2))


def bivariate_Gaussian(kernel_size, sig_x, sig_y, theta, grid=None, isotropic=True):
    """exp(-q / 2), normalised; isotropic: only ``sig_x`` is used."""
    kernel = np.exp(-0.5 * _quadratic_form(kernel_size, sig_x, sig_y, theta, grid, isotropic))
    return kernel / np.sum(kernel)


def bivariate_generalized_Gaussian(kernel_size, sig_x, sig_y, theta, beta, grid=None, isotropic=True):
    """exp(-q^beta / 2), normalised (beta = 1: the Gaussian)."""
    kernel = np.exp(-0.5 * np.power(_quadratic_form(kernel_size, sig_x, sig_y, theta, grid, isotropic), beta))
    return kernel / np.sum(kernel)


def bivariate_plateau(kernel_size, sig_x, sig_y, theta, beta, grid=None, isotropic=True):
    """1 / (1 + q^beta), normalised."""
    kernel = np.reciprocal(np.power(_quadratic_form(kernel_size, sig_x, sig_y, theta, grid, isotropic), beta) + 1)
    return kernel / np.sum(kernel)


def _draw_shape(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic):
    assert kernel_size % 2 == 1, 'Kernel size must be an odd number.'
    assert sigma_x_range[0] < sigma_x_range[1], 'Wrong sigma_x_range.'
    sigma_x = np.random.uniform(sigma_x_range[0], sigma_x_range[1])
    if isotropic is False:
        assert sigma_y_range[0] < sigma_y_range[1], 'Wrong sigma_y_range.'
        assert rotation_range[0] < rotation_range[1], 'Wrong rotation_range.'
        sigma_y = np.random.uniform(sigma_y_range[0], sigma_y_range[1])
        rotation = np.random.uniform(rotation_range[0], rotation_range[1])
    else:
        sigma_y, rotation = sigma_x, 0
    return sigma_x, sigma_y, rotation


def _draw_beta(beta_range):
    # the reference assumes beta_range[0] < 1 < beta_range[1]
    if np.random.uniform() < 0.5:
        return np.random.uniform(beta_range[0], 1)
    return np.random.uniform(1, beta_range[1])


def _kernel_noise(kernel, noise_range):
    if noise_range is not None:
        assert noise_range[0] < noise_range[1], 'Wrong noise range.'
        kernel = kernel * np.random.uniform(noise_range[0], noise_range[1], size=kernel.shape)
    return kernel / np.sum(kernel)


def random_bivariate_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, noise_range=None, isotropic=True):
    sx, sy, rot = _draw_shape(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    return _kernel_noise(bivariate_Gaussian(kernel_size, sx, sy, rot, isotropic=isotropic), noise_range)


def random_bivariate_generalized_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, beta_range,
                                          noise_range=None, isotropic=True):
    sx, sy, rot = _draw_shape(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    beta = _draw_beta(beta_range)
    return _kernel_noise(bivariate_generalized_Gaussian(kernel_size, sx, sy, rot, beta, isotropic=isotropic), noise_range)


def random_bivariate_plateau(kernel_size, sigma_x_range, sigma_y_range, rotation_range, beta_range, noise_range=None,
                             isotropic=True):
    sx, sy, rot = _draw_shape(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    beta = _draw_beta(beta_range)
    return _kernel_noise(bivariate_plateau(kernel_size, sx, sy, rot, beta, isotropic=isotropic), noise_range)


def random_mixed_kernels(kernel_list, kernel_prob, kernel_size=21, sigma_x_range=(0.6, 5), sigma_y_range=(0.6, 5),
                         rotation_range=(-math.pi, math.pi), betag_range=(0.5, 8), betap_range=(0.5, 8),
                         noise_range=None):
    """One kernel of a type drawn from ``kernel_list`` with ``kernel_prob``: 'iso', 'aniso', 'generalized_iso',
    'generalized_aniso', 'plateau_iso', 'plateau_aniso' (the plateau kernels never get the multiplicative noise)."""
    kernel_type = random.choices(kernel_list, kernel_prob)[0]
    shape = (kernel_size, sigma_x_range, sigma_y_range, rotation_range)
    if kernel_type in ('iso', 'aniso'):
        return random_bivariate_Gaussian(*shape, noise_range=noise_range, isotropic=kernel_type == 'iso')
    if kernel_type in ('generalized_iso', 'generalized_aniso'):
        return random_bivariate_generalized_Gaussian(*shape, betag_range, noise_range=noise_range,
                                                     isotropic=kernel_type == 'generalized_iso')
    if kernel_type in ('plateau_iso', 'plateau_aniso'):
        return random_bivariate_plateau(*shape, betap_range, noise_range=None, isotropic=kernel_type == 'plateau_iso')
    raise NotImplementedError(f'kernel type {kernel_type!r}')


def circular_lowpass_kernel(cutoff, kernel_size, pad_to=0):
    """The 2-D circularly symmetric sinc filter w J1(w r) / (2 pi r) (w^2 / (4 pi) at r = 0), normalised to sum 1
    and zero-padded to ``pad_to``; ``cutoff`` w in radians (pi is the maximum)."""
    assert kernel_size % 2 == 1, 'Kernel size must be an odd number.'
    c = (kernel_size - 1) / 2
    yy, xx = np.mgrid[0:kernel_size, 0:kernel_size].astype(np.float64)
    r = np.sqrt((yy - c)**2 + (xx - c)**2)
    with np.errstate(divide='ignore', invalid='ignore'):
        kernel = cutoff * special.j1(cutoff * r) / (2 * np.pi * r)
    kernel[(kernel_size - 1) // 2, (kernel_size - 1) // 2] = cutoff**2 / (4 * np.pi)
    kernel = kernel / np.sum(kernel)
    if pad_to > kernel_size:
        pad = (pad_to - kernel_size) // 2
        kernel = np.pad(kernel, ((pad, pad), (pad, pad)))
    return kernel


# -------------------------------------------------------------------------------------------------- noise


def generate_gaussian_noise_pt(img, sigma=10, gray_noise=0):
    """Gaussian noise of standard deviation ``sigma`` / 255 (a number or [b]) for ``img`` (b, 3, h, w);
    ``gray_noise`` (a number or [b] of 0 / 1): the samples that get one gray field, shared by the batch up to sigma."""
    return D.gaussian_noise(img, sigma, gray_noise, clip=False, noise_only=True)


def add_gaussian_noise_pt(img, sigma=10, gray_noise=0, clip=True, rounds=False):
    return D.gaussian_noise(img, sigma, gray_noise, clip=clip, rounds=rounds)


def _random_amp_gray(img, amp_range, gray_prob):
    b = img.size(0)
    amp = torch.rand(b, dtype=img.dtype, device=img.device) * (amp_range[1] - amp_range[0]) + amp_range[0]
    gray = (torch.rand(b, dtype=img.dtype, device=img.device) < gray_prob).float()
    return amp, gray


def random_generate_gaussian_noise_pt(img, sigma_range=(0, 10), gray_prob=0):
    sigma, gray = _random_amp_gray(img, sigma_range, gray_prob)
    return generate_gaussian_noise_pt(img, sigma, gray)


def random_add_gaussian_noise_pt(img, sigma_range=(0, 1.0), gray_prob=0, clip=True, rounds=False):
    sigma, gray = _random_amp_gray(img, sigma_range, gray_prob)
    return add_gaussian_noise_pt(img, sigma, gray, clip=clip, rounds=rounds)


def generate_poisson_noise_pt(img, scale=1.0, gray_noise=0):
    """Poisson (shot) noise for ``img`` (b, 3, h, w) times ``scale`` (a number or [b]): per sample the image is
    rounded to its 8-bit levels, vals = 2^ceil(log2(number of distinct levels)), noise = poisson(level vals) / vals -
    level; ``gray_noise`` samples take it from the gray image for all three channels."""
    return D.poisson_noise(img, scale, gray_noise, clip=False, noise_only=True)


def add_poisson_noise_pt(img, scale=1.0, clip=True, rounds=False, gray_noise=0):
    return D.poisson_noise(img, scale, gray_noise, clip=clip, rounds=rounds)


def random_generate_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0):
    scale, gray = _random_amp_gray(img, scale_range, gray_prob)
    return generate_poisson_noise_pt(img, scale, gray)


def random_add_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0, clip=True, rounds=False):
    scale, gray = _random_amp_gray(img, scale_range, gray_prob)
    return add_poisson_noise_pt(img, scale, clip=clip, rounds=rounds, gray_noise=gray)
