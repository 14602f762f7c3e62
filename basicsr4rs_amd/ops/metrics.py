"""Validation metrics on the HIP engine (csrc/metrics.hip): per (image, channel) the integer sum of
squared ubyte differences and the float64 SSIM of a [-1, 1] NCHW pair, and the PSNR / SSIM scores of
metrics/psnr_ssim.py derived from them on the host with that module's numpy expressions.  NIQE
(csrc/niqe.hip): the block moments of the configured planes, and the scores metrics/niqe.py derives from
them on the host."""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..metrics import niqe as _niqe

# the metric functions the device path can stand in for (all with test_y_channel false)
DEVICE_METRICS = ('calculate_psnr', 'calculate_ssim', 'calculate_psnr_band', 'calculate_ssim_band')
# the NIQE entries it can stand in for, under the conditions of niqe_device_reason
NIQE_DEVICE_METRICS = ('calculate_niqe', 'calculate_rs_niqe', 'calculate_niqe_band')
# bgr2ycbcr(y_only=True) on a [0, 1] BGR pixel (metrics/psnr_ssim.py:_to_y): the three weights, the offset
Y_COEF = (24.966, 128.553, 65.481, 16.0)


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


def niqe_moments_device(sr, planes, crop, window, return_maps=False):
    """Launch sr_niqe_moments on an fp32 NCHW tensor in nominal [-1, 1].  ``planes`` is a list of
    ``(n, channels)`` with one channel (the band as it is) or three (read as BGR, their Y); ``window`` the
    7 x 7 window of the parameter file.  Returns the device tensor of moments
    ``[P, 2, block rows, block columns, 5, 6]`` (float64) without synchronising; with ``return_maps`` also
    the planes and the scale-1 MSCN maps, fp32 ``[P, Hb, Wb]``."""
    if sr.dim() != 4:
        raise ValueError(f'niqe_moments: an NCHW tensor, got {tuple(sr.shape)}')
    sr = sr.detach().float().contiguous()
    N, C, H, W = sr.shape
    P = len(planes)
    desc = []
    for n, ch in planes:
        ch = [int(c) for c in ch]
        if len(ch) not in (1, 3):
            raise ValueError(f'niqe_moments: a plane has 1 or 3 channels, got {ch}')
        desc += [int(n)] + ch + [-1] * (3 - len(ch))
    lib = _lib.load()
    ws_bytes = lib.sr_niqe_moments_workspace(N, C, H, W, int(crop), P)
    if ws_bytes == 0:
        raise ValueError(f'niqe_moments: unsupported shape {tuple(sr.shape)} with crop_border {crop} and {P} planes')
    bh, bw = (H - 2 * int(crop)) // _niqe.BLOCK, (W - 2 * int(crop)) // _niqe.BLOCK
    ws = torch.empty(ws_bytes // 4, device=sr.device, dtype=torch.float32)
    mom = torch.empty(P, 2, bh, bw, 5, 6, device=sr.device, dtype=torch.float64)
    maps = [torch.empty(P, bh * _niqe.BLOCK, bw * _niqe.BLOCK, device=sr.device, dtype=torch.float32)
            for _ in range(2)] if return_maps else [None, None]
    desc_c = (ctypes.c_int * len(desc))(*desc)
    coef_c = (ctypes.c_double * 4)(*Y_COEF)
    win = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    if win.size != 49:
        raise ValueError(f'niqe_moments: a 7 x 7 window, got {np.shape(window)}')
    win_c = (ctypes.c_double * 49)(*win)
    _lib.check(lib.sr_niqe_moments(_lib.ptr(sr), N, C, H, W, int(crop), P, ctypes.cast(desc_c, ctypes.c_void_p),
                                   ctypes.cast(coef_c, ctypes.c_void_p), ctypes.cast(win_c, ctypes.c_void_p),
                                   _lib.ptr(mom), _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.ptr(ws), ws_bytes,
                                   _lib.stream()))
    return (mom, maps[0], maps[1]) if return_maps else mom


def niqe_plane_channels(o, C):
    """The channels of the [H, W, C] image that the NIQE entry ``o`` takes its plane from, or a string
    saying why the device kernel cannot stand in for it (metrics/niqe.py:niqe_plane decides on the host)."""
    kind = o['type']
    if o.get('input_order', 'HWC') != 'HWC':
        return f'input_order {o["input_order"]!r}'
    if kind == 'calculate_niqe_band':
        ch = [o['band']]
    else:
        if o.get('convert_to', 'y') != 'y':
            return f'convert_to {o.get("convert_to")!r}'
        ch = list(o.get('input_bands', (2, 1, 0))) if kind == 'calculate_rs_niqe' else list(range(C))
        if len(ch) not in (1, 3):
            return f'a selection of {len(ch)} bands'
    if not all(isinstance(c, int) and 0 <= c < C for c in ch):
        return f'band selection {ch} outside the {C} channels'
    return ch


def niqe_device_reason(o, C, H, W):
    """None when sr_niqe_moments can stand in for the NIQE entry ``o`` on a [C, H, W] image, else why not."""
    ch = niqe_plane_channels(o, C)
    if isinstance(ch, str):
        return ch
    crop = int(o['crop_border'])
    if H - 2 * crop < _niqe.BLOCK or W - 2 * crop < _niqe.BLOCK:
        return f'{H} x {W} with crop_border {crop} is smaller than one {_niqe.BLOCK} x {_niqe.BLOCK} block'
    return None


def niqe_launch(metrics_opt, sr):
    """Launch sr_niqe_moments for the NIQE entries of ``metrics_opt`` on one image (batch 1): one call per
    distinct ``crop_border`` with every distinct plane once.  Returns the flat device tensors of moments
    (float64, not synchronised) and ``finish(host)``, which turns their concatenation, copied to the host,
    into ``{name: score}`` with metrics/niqe.py:niqe_from_moments.  The caller has checked
    niqe_device_reason."""
    _, C, H, W = sr.shape
    sr = sr.detach().float().contiguous()
    params = {name: _niqe.load_niqe_params(o.get('params_path')) for name, o in metrics_opt.items()}
    window = next(iter(params.values()))[2]
    launches = {}  # crop -> list of distinct channel tuples
    where = {}
    for name, o in metrics_opt.items():
        if not np.array_equal(params[name][2], window):
            raise ValueError('niqe: the entries of one validation name parameter files with different windows')
        ch = tuple(niqe_plane_channels(o, C))
        planes = launches.setdefault(int(o['crop_border']), [])
        if ch not in planes:
            planes.append(ch)
        where[name] = (int(o['crop_border']), planes.index(ch))
    crops = sorted(launches)
    parts = [niqe_moments_device(sr, [(0, ch) for ch in launches[c]], c, window) for c in crops]

    def finish(host):
        moments, at = {}, 0
        for c, m in zip(crops, parts):
            moments[c] = host[at:at + m.numel()].reshape(m.shape)
            at += m.numel()
        return {name: _niqe.niqe_from_moments(moments[c][i], params[name][0], params[name][1])
                for name, (c, i) in where.items()}

    return [m.reshape(-1) for m in parts], finish


def niqe_scores_from_device(metrics_opt, sr):
    """The score of every NIQE entry of ``metrics_opt`` for one image: niqe_launch, one device-to-host copy of
    all moments, the host fits."""
    tensors, finish = niqe_launch(metrics_opt, sr)
    return finish(torch.cat(tensors).cpu().numpy())


def scores_from_device(metrics_opt, sr, gt):
    """Every configured score of one image pair (batch 1) from the device kernels: one launch per
    distinct ``crop_border``, one device-to-host copy of all results, then the host expressions of
    calculate_psnr / calculate_ssim and their ``_band`` forms.  ``metrics_opt`` is ``val.metrics``;
    the caller has checked that every entry is in DEVICE_METRICS with test_y_channel false, or a NIQE
    entry that niqe_device_reason accepts.  The NIQE entries are launched through niqe_launch and their
    moments ride in the same copy; a configuration without them runs what it always ran."""
    names = list(metrics_opt)
    niqe_opt = {name: o for name, o in metrics_opt.items() if o['type'] in NIQE_DEVICE_METRICS}
    niqe_tensors, niqe_finish = niqe_launch(niqe_opt, sr) if niqe_opt else ([], None)
    if niqe_opt:
        metrics_opt = {name: o for name, o in metrics_opt.items() if name not in niqe_opt}
    _, C, H, W = sr.shape
    crops = sorted({int(o['crop_border']) for o in metrics_opt.values()})
    sr = sr.detach().float().contiguous()
    gt = gt.detach().float().contiguous()
    parts = [val_metrics_launch(sr, gt, c) for c in crops]
    # one copy: the int64 sums travel as float64 bit patterns next to the SSIM values
    packed = torch.cat([torch.cat([sse.view(torch.float64).reshape(-1), ssim.reshape(-1)]) for sse, ssim in parts]
                       + niqe_tensors)
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
    if niqe_opt:
        scores.update(niqe_finish(host[len(crops) * 2 * C:]))
        scores = {name: scores[name] for name in names}
    return scores
