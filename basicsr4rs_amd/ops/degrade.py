"""Ops of the Real-ESRGAN degradation pipeline on the HIP kernels of csrc/degrade.hip (the reference runs the same
sequence with stock torch ops inside ``feed_data``, basicsr/models/realesrgan_model.py:68-185).

Images are NCHW fp32 on the device; every op is forward only (the pipeline runs under ``no_grad``): an input that
requires grad while grad is enabled raises ``NotImplementedError``, and so does a CPU tensor.

``filter2d(img, kernel, round255)``: ``filter2D`` of img_process_util.py:7-31.
``sep_blur(img, taps)``: a separable reflect-padded blur; ``usm_sharp(img, taps, weight, threshold)``: USMSharp in
four launches.
``resize(img, scale_factor= | size=, mode)``: ``F.interpolate`` for 'area', 'bilinear', 'bicubic'.
``gaussian_noise(img, sigma, gray, normal, normal_gray)`` / ``poisson_levels`` / ``poisson_noise``: the noise of
data/degradations.py with the draws made by torch's device generator and no value returned to the host.
``jpeg(img, quality, differentiable)``: ``DiffJPEG.forward`` as one kernel.

Every launch runs under a ``ktrace.span`` with the kernel name and its algorithmic FLOPs / bytes.
"""
import math

import torch

from .. import _lib
from .perceptual import _launch

RESIZE_MODES = {'area': 0, 'bilinear': 1, 'bicubic': 2}
_CPU_MESSAGE = 'basicsr4rs_amd HIP ops need tensors on the MI355X (cuda) device'


def _image(img, what, channels=None):
    if not img.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if img.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f'{what}: forward only; the input requires grad')
    if img.dim() != 4 or img.dtype != torch.float32 or (channels is not None and img.shape[1] != channels):
        want = f'[B, {channels}, H, W]' if channels is not None else '[B, C, H, W]'
        raise ValueError(f'{what}: an fp32 {want} image is expected, got {img.dtype} {tuple(img.shape)}')
    return img.detach().contiguous()


def _per_sample(v, B, device, what):
    """A Python number or a [B] tensor as an fp32 [B] device tensor (no host sync for a device tensor)."""
    if isinstance(v, (int, float)):
        return torch.full((B, ), float(v), device=device, dtype=torch.float32)
    if not v.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if v.numel() != B:
        raise ValueError(f'{what}: one value per sample is expected, got {tuple(v.shape)} for a batch of {B}')
    return v.detach().reshape(B).float().contiguous()


# ------------------------------------------------------------------------------------------------ filter2d


def filter2d(img, kernel, round255=False):
    """Reflect-padded correlation of every channel of sample n with ``kernel[n]`` ([B, k, k]) or the shared
    ``kernel[0]`` ([1, k, k]); k odd, 3 to 21.  ``round255``: store clamp(rint(255 v), 0, 255) / 255."""
    x = _image(img, 'filter2d')
    B, Cc, H, W = x.shape
    if not kernel.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    k = kernel.shape[-1]
    if kernel.dim() != 3 or kernel.shape[-2] != k or kernel.shape[0] not in (1, B):
        raise ValueError(f'filter2d: the kernel must be [B, k, k] or [1, k, k], got {tuple(kernel.shape)}')
    if k % 2 == 0:
        raise ValueError('Wrong kernel size')
    kern = kernel.detach().float().contiguous()
    y = torch.empty_like(x)
    lib = _lib.load()
    batched = int(kernel.shape[0] != 1)
    args = (_lib.ptr(x), B, Cc, H, W, _lib.ptr(kern), batched, k, int(bool(round255)), _lib.ptr(y), _lib.stream())
    _launch('filter2d_kernel', 2.0 * x.numel() * k * k, 4.0 * (2 * x.numel() + kern.numel()), lib.sr_filter2d, args,
            (x, kern, y))
    return y


# ------------------------------------------------------------------------------------------ separable blur


def gaussian_taps(radius, sigma=0):
    """The 1-D Gaussian of ``cv2.getGaussianKernel(radius, sigma)`` from its definition, float64: sigma <= 0 means
    0.3 ((radius - 1) 0.5 - 1) + 0.8; weights exp(-(i - (radius - 1) / 2)^2 / (2 sigma^2)) normalised to sum 1."""
    if sigma <= 0:
        sigma = 0.3 * ((radius - 1) * 0.5 - 1) + 0.8
    i = torch.arange(radius, dtype=torch.float64) - (radius - 1) * 0.5
    w = torch.exp(-(i * i) / (2.0 * sigma * sigma))
    return w / w.sum()


def _taps(taps, what):
    if not taps.is_cuda:
        raise NotImplementedError(_CPU_MESSAGE)
    if taps.dim() != 1:
        raise ValueError(f'{what}: a 1-D filter is expected, got {tuple(taps.shape)}')
    return taps.detach().float().contiguous()


def sep_blur(img, taps):
    """Rows then columns of the 1-D filter ``taps`` (odd length <= 51), each reflect-padded: two launches."""
    x = _image(img, 'sep_blur')
    t = _taps(taps, 'sep_blur')
    B, Cc, H, W = x.shape
    tmp, y = torch.empty_like(x), torch.empty_like(x)
    lib = _lib.load()
    args = (_lib.ptr(x), B * Cc, H, W, _lib.ptr(t), t.numel(), _lib.ptr(tmp), _lib.ptr(y), _lib.stream())
    _launch('blur_row_kernel+col', 4.0 * x.numel() * t.numel(), 16.0 * x.numel(), lib.sr_sep_blur, args, (x, t, tmp, y),
            launches=2)
    return y


def usm_sharp_raw(img, taps, weight=0.5, threshold=10):
    """(sharpened image, residual, mask) of USMSharp from ``sr_usm_sharp_launches()`` launches."""
    x = _image(img, 'usm_sharp')
    t = _taps(taps, 'usm_sharp')
    B, Cc, H, W = x.shape
    tmp, res, mask, y = (torch.empty_like(x) for _ in range(4))
    lib = _lib.load()
    args = (_lib.ptr(x), B * Cc, H, W, _lib.ptr(t), t.numel(), float(weight), float(threshold), _lib.ptr(tmp),
            _lib.ptr(res), _lib.ptr(mask), _lib.ptr(y), _lib.stream())
    # two separable blurs; x read by three passes, tmp written and read twice, residual and mask written and read
    _launch('usm_sharp_kernels', 8.0 * x.numel() * t.numel(), 4.0 * x.numel() * 12, lib.sr_usm_sharp, args,
            (x, t, tmp, res, mask, y), launches=lib.sr_usm_sharp_launches())
    return y, res, mask


def usm_sharp(img, taps, weight=0.5, threshold=10):
    return usm_sharp_raw(img, taps, weight, threshold)[0]


# -------------------------------------------------------------------------------------------------- resize


def resize_geometry(in_size, scale_factor=None, size=None):
    """torch's two conventions: (output size, coordinate scale) of one axis.  ``scale_factor=s``: floor(in s) and
    1 / s; ``size=``: that size and in / out.  The scale is rounded to fp32 by the kernel entry, as torch does."""
    if (scale_factor is None) == (size is None):
        raise ValueError('resize: exactly one of scale_factor and size is expected')
    if scale_factor is not None:
        return int(math.floor(float(in_size) * float(scale_factor))), 1.0 / float(scale_factor)
    return int(size), float(in_size) / float(size)


def resize(img, scale_factor=None, size=None, mode='bilinear'):
    """``F.interpolate(img, scale_factor= | size=, mode=)`` with align_corners=False and no antialiasing."""
    if mode not in RESIZE_MODES:
        raise NotImplementedError(f"resize: mode {mode!r} (supported: 'area', 'bilinear', 'bicubic')")
    x = _image(img, 'resize')
    B, Cc, H, W = x.shape
    if scale_factor is not None and not isinstance(scale_factor, (tuple, list)):
        scale_factor = (scale_factor, scale_factor)
    if size is not None and not isinstance(size, (tuple, list)):
        size = (size, size)
    Ho, sh = resize_geometry(H, scale_factor[0] if scale_factor is not None else None, size[0] if size is not None else None)
    Wo, sw = resize_geometry(W, scale_factor[1] if scale_factor is not None else None, size[1] if size is not None else None)
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f'resize: the output size {(Ho, Wo)} must be positive')
    y = torch.empty(B, Cc, Ho, Wo, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    args = (_lib.ptr(x), B * Cc, H, W, Ho, Wo, RESIZE_MODES[mode], sh, sw, _lib.ptr(y), _lib.stream())
    taps = {'area': max(1.0, (H / Ho) * (W / Wo)), 'bilinear': 4.0, 'bicubic': 16.0}[mode]
    _launch(f'resize_kernel<{mode}>', 2.0 * y.numel() * taps, 4.0 * (x.numel() + y.numel()), lib.sr_resize, args, (x, y))
    return y


# --------------------------------------------------------------------------------------------------- noise


def _finish(clip, rounds, noise_only):
    """The finish flags of the noise entries: 1 = round to 8 bits, 2 = no clip, 4 = the noise alone."""
    return int(bool(rounds)) | (0 if clip else 2) | (4 if noise_only else 0)


def gaussian_noise(img, sigma, gray=None, normal=None, normal_gray=None, clip=True, rounds=False, noise_only=False):
    """``add_gaussian_noise_pt`` (``clip`` / ``rounds`` as there; ``noise_only``: the noise alone):
    ``normal`` [B, 3, H, W] and (with ``gray``, the [B] 0 / 1
    flags) ``normal_gray`` [H, W], drawn here by ``torch.randn`` when not given."""
    x = _image(img, 'gaussian_noise', 3)
    B, _, H, W = x.shape
    sig = _per_sample(sigma, B, x.device, 'gaussian_noise')
    g = _per_sample(gray, B, x.device, 'gaussian_noise') if gray is not None else None
    if g is not None and normal_gray is None:
        normal_gray = torch.randn(H, W, device=x.device, dtype=torch.float32)
    if normal is None:
        normal = torch.randn(B, 3, H, W, device=x.device, dtype=torch.float32)
    if tuple(normal.shape) != tuple(x.shape) or (g is not None and tuple(normal_gray.shape) != (H, W)):
        raise ValueError('gaussian_noise: normal must match the image and normal_gray must be [H, W]')
    nc = normal.float().contiguous()
    ng = normal_gray.float().contiguous() if g is not None else None
    out = torch.empty_like(x)
    lib = _lib.load()
    args = (_lib.ptr(x), _lib.ptr(nc), _lib.ptr(ng), _lib.ptr(sig), _lib.ptr(g), B, H, W, _finish(clip, rounds, noise_only),
            _lib.ptr(out), _lib.stream())
    _launch('gaussian_apply_kernel', 8.0 * x.numel(), 12.0 * x.numel(), lib.sr_gaussian_apply, args, (x, nc, ng, sig, g, out))
    return out


def poisson_levels(img):
    """(rate_c [B, 3, H, W], rate_g [B, 1, H, W], vals [B, 2], bitmap [B, 2, 8] int32): the Poisson rates
    level / 255 * vals of the colour and gray images with vals = 2^ceil(log2(distinct 8-bit levels of the sample)),
    all formed on the device from a 256-bit presence map per sample."""
    x = _image(img, 'poisson_levels', 3)
    B, _, H, W = x.shape
    bitmap = torch.zeros(B, 2, 8, device=x.device, dtype=torch.int32)
    rate_c = torch.empty_like(x)
    rate_g = torch.empty(B, 1, H, W, device=x.device, dtype=torch.float32)
    vals = torch.empty(B, 2, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    _launch('level_presence_kernel', 12.0 * x.numel(), 4.0 * x.numel(), lib.sr_level_presence,
            (_lib.ptr(x), B, H, W, _lib.ptr(bitmap), _lib.stream()), (x, bitmap))
    _launch('poisson_rate_kernel', 12.0 * x.numel(), 4.0 * (2 * x.numel() + rate_g.numel()), lib.sr_poisson_rate,
            (_lib.ptr(x), _lib.ptr(bitmap), B, H, W, _lib.ptr(rate_c), _lib.ptr(rate_g), _lib.ptr(vals), _lib.stream()),
            (x, bitmap, rate_c, rate_g, vals))
    return rate_c, rate_g, vals, bitmap


def poisson_noise(img, scale, gray=None, draw_c=None, draw_g=None, levels=None, clip=True, rounds=False,
                  noise_only=False):
    """``add_poisson_noise_pt`` (``clip`` / ``rounds`` as there; ``noise_only``: the noise alone).
    ``levels``: the result of ``poisson_levels(img)``;
    ``draw_c`` / ``draw_g``: Poisson draws from its rates, made here by ``torch.poisson`` when not given."""
    x = _image(img, 'poisson_noise', 3)
    B, _, H, W = x.shape
    sc = _per_sample(scale, B, x.device, 'poisson_noise')
    g = _per_sample(gray, B, x.device, 'poisson_noise') if gray is not None else None
    rate_c, rate_g, vals, _ = levels if levels is not None else poisson_levels(x)
    if g is not None and draw_g is None:
        draw_g = torch.poisson(rate_g)
    if draw_c is None:
        draw_c = torch.poisson(rate_c)
    dc = draw_c.float().contiguous()
    dg = draw_g.float().contiguous() if g is not None else None
    if tuple(dc.shape) != tuple(x.shape) or (dg is not None and dg.numel() != B * H * W):
        raise ValueError('poisson_noise: draw_c must match the image and draw_g must be [B, 1, H, W]')
    out = torch.empty_like(x)
    lib = _lib.load()
    args = (_lib.ptr(x), _lib.ptr(dc), _lib.ptr(dg), _lib.ptr(vals), _lib.ptr(sc), _lib.ptr(g), B, H, W,
            _finish(clip, rounds, noise_only), _lib.ptr(out), _lib.stream())
    _launch('poisson_apply_kernel', 16.0 * x.numel(), 12.0 * x.numel(), lib.sr_poisson_apply, args,
            (x, dc, dg, vals, sc, g, out))
    return out


# ---------------------------------------------------------------------------------------------------- JPEG


def jpeg_raw(img, quality, differentiable=False, round255=False, want_coef=False):
    """(image, coef or None) of DiffJPEG.forward.  ``quality``: a Python number or a [B] device tensor (left
    unchanged); the quality-to-factor map runs in the kernel either way."""
    x = _image(img, 'jpeg', 3)
    B, _, H, W = x.shape
    q = _per_sample(quality, B, x.device, 'jpeg')
    y = torch.empty_like(x)
    coef = None
    if want_coef:
        H16, W16 = (H + 15) // 16 * 16, (W + 15) // 16 * 16
        coef = torch.empty(B * H16 * W16 * 3 // 2, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    args = (_lib.ptr(x), B, H, W, _lib.ptr(q), int(bool(differentiable)), int(bool(round255)), _lib.ptr(y), _lib.ptr(coef),
            _lib.stream())
    # four 8-point transforms per coefficient (1.5 coefficients per pixel) plus the colour conversions
    _launch('jpeg_kernel', 2.0 * 1.5 * 32 * B * H * W + 30.0 * B * H * W, 8.0 * x.numel(), lib.sr_jpeg, args,
            (x, q, y, coef))
    return y, coef


def jpeg_coef_views(coef, B, H, W):
    """(Y [B, H16/8, W16/8, 8, 8], Cb, Cr [B, H16/16, W16/16, 8, 8]) views of ``jpeg_raw``'s coefficient buffer."""
    H16, W16 = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    ny, nc = B * H16 * W16, B * H16 * W16 // 4
    return (coef[:ny].view(B, H16 // 8, W16 // 8, 8, 8), coef[ny:ny + nc].view(B, H16 // 16, W16 // 16, 8, 8),
            coef[ny + nc:].view(B, H16 // 16, W16 // 16, 8, 8))


def jpeg(img, quality, differentiable=False, round255=False):
    return jpeg_raw(img, quality, differentiable, round255)[0]
