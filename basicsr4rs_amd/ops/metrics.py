"""Validation metrics on the HIP engine (csrc/metrics.hip): per (image, channel) the integer sum of
squared ubyte differences and the float64 SSIM of a [-1, 1] NCHW pair, and the PSNR / SSIM scores of
metrics/psnr_ssim.py derived from them on the host with that module's numpy expressions."""
import numpy as np
import torch

from .. import _lib

# the metric functions the device path can stand in for (all with test_y_channel false)
DEVICE_METRICS = ('calculate_psnr', 'calculate_ssim', 'calculate_psnr_band', 'calculate_ssim_band')


def val_metrics_launch(sr, gt, crop):
    """Launch sr_val_metrics on fp32 NCHW tensors in nominal [-1, 1]; returns the device tensors
    ``(sse int64 [N, C], ssim float64 [N, C])`` without synchronising."""
    if sr.shape != gt.shape or sr.dim() != 4:
        raise ValueError(f'val_metrics: two NCHW tensors of one shape, got {tuple(sr.shape)} and {tuple(gt.shape)}')
    sr = sr.detach().float().contiguous()
    gt = gt.detach().float().contiguous()
    N, C, H, W = sr.shape
    lib = _lib.load()
    ws_bytes = lib.sr_val_metrics_workspace(N, C, H, W, int(crop))
    if ws_bytes == 0:
        raise ValueError(f'val_metrics: unsupported shape {tuple(sr.shape)} with crop_border {crop}')
    ws = torch.empty(ws_bytes // 8, device=sr.device, dtype=torch.float64)
    sse = torch.empty(N, C, device=sr.device, dtype=torch.int64)
    ssim = torch.empty(N, C, device=sr.device, dtype=torch.float64)
    _lib.check(lib.sr_val_metrics(_lib.ptr(sr), _lib.ptr(gt), N, C, H, W, int(crop), _lib.ptr(sse), _lib.ptr(ssim),
                                  _lib.ptr(ws), ws_bytes, _lib.stream()))
    return sse, ssim


def val_metrics(sr, gt, crop):
    """``(sse, ssim)`` of :func:`val_metrics_launch` as numpy arrays [N, C] (int64, float64)."""
    sse, ssim = val_metrics_launch(sr, gt, crop)
    return sse.cpu().numpy(), ssim.cpu().numpy()


def psnr_from_sse(sse, count):
    """calculate_psnr's value from the integer squared-difference sum over ``count`` pixels: the mean of
    integers below 2^53 is the same float64 whether numpy sums squares or this divides their exact
    sum, as long as numpy's own sum is exact -- which it is, every partial sum being an integer
    below 2^53."""
    mse = np.float64(int(sse)) / np.float64(count)
    if mse == 0:
        return float('inf')
    return 10. * np.log10(255. * 255. / mse)


def scores_from_device(metrics_opt, sr, gt):
    """Every configured score of one image pair (batch 1) from the device kernel: one launch per
    distinct ``crop_border``, one device-to-host copy of all results, then the host expressions of
    calculate_psnr / calculate_ssim and their ``_band`` forms.  ``metrics_opt`` is ``val.metrics``;
    the caller has checked that every entry is in DEVICE_METRICS with test_y_channel false."""
    _, C, H, W = sr.shape
    crops = sorted({int(o['crop_border']) for o in metrics_opt.values()})
    sr = sr.detach().float().contiguous()
    gt = gt.detach().float().contiguous()
    parts = [val_metrics_launch(sr, gt, c) for c in crops]
    # one copy: the int64 sums travel as float64 bit patterns next to the SSIM values
    packed = torch.cat([torch.cat([sse.view(torch.float64).reshape(-1), ssim.reshape(-1)]) for sse, ssim in parts])
    host = packed.cpu().numpy()
    res = {}
    for i, c in enumerate(crops):
        blk = host[i * 2 * C:(i + 1) * 2 * C]
        res[c] = (blk[:C].view(np.int64), blk[C:])
    scores = {}
    for name, o in metrics_opt.items():
        crop = int(o['crop_border'])
        sse, ssim = res[crop]
        npix = (H - 2 * crop) * (W - 2 * crop)
        kind = o['type']
        if kind.endswith('_band'):
            band = o['band']
            assert band < C, f'Band index {band} out of range for shape {(H, W, C)}.'
        if kind == 'calculate_psnr':
            scores[name] = psnr_from_sse(int(sse.sum()), npix * C)
        elif kind == 'calculate_psnr_band':
            scores[name] = psnr_from_sse(sse[band], npix)
        elif kind == 'calculate_ssim':
            scores[name] = np.array(ssim).mean()
        else:
            scores[name] = ssim[band]
    return scores
