"""sr_val_metrics against the host validation path: minusone_one_tensor_to_ubyte_numpy, the crop, then the
integer squared-difference sum and metrics/psnr_ssim.py:_ssim per channel.

* ``sse`` is the host's integer exactly, so every PSNR derived from it is ``==`` the host's float
  (``inf`` for an identical pair included);
* ``ssim`` is NaN where the host's is (a crop smaller than the 11 x 11 window) and otherwise within 1e-10:
  two float64 evaluations of the map in different summation orders differ by a few 1e-13 on inputs of
  this kind and the worst-case cancellation bound is about 1e-11, so 1e-10 admits any float64 ordering
  and no float32 arithmetic;
* two calls on the same input are bitwise equal (no floating-point atomics).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, C, H, W, crop)
CASES = [
    (1, 6, 37, 53, 4),    # odd sizes, partial tiles
    (1, 2, 11, 11, 0),    # 1 x 1 SSIM map
    (1, 3, 19, 12, 4),    # Wc = 4: SSIM NaN, SSE still right
    (2, 6, 48, 80, 4),    # N > 1 through the ABI
    (1, 3, 75, 141, 3),   # several tiles in both directions
    (1, 6, 96, 96, 0),    # no crop
]
KINDS = ['uniform', 'noise', 'identical', 'rounding_edge', 'bright_flat']


def _inputs(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    if kind == 'uniform':  # beyond [-1, 1]: the clamp
        return (torch.rand(shape, generator=g) * 2.4 - 1.2, torch.rand(shape, generator=g) * 2.4 - 1.2)
    if kind == 'noise':
        gt = torch.rand(shape, generator=g) * 2 - 1
        return gt + 0.03 * torch.randn(shape, generator=g), gt
    if kind == 'identical':
        gt = torch.rand(shape, generator=g) * 2.2 - 1.1
        return gt.clone(), gt
    if kind == 'rounding_edge':  # t * 255 lands on k + 0.5 (or next to it): half-to-even and fp32 rounding decide
        k = np.arange(255, dtype=np.float32)
        edge = ((k + np.float32(0.5)) / np.float32(255)).astype(np.float32) * np.float32(2) - np.float32(1)
        idx = np.arange(n)
        gt = torch.from_numpy(edge[idx % 255].reshape(shape))
        sr = torch.from_numpy(edge[(idx * 7 + 3) % 255].reshape(shape))
        return sr, gt
    # bright, flat: gt on levels 250..255, sr within one level of it (sigma^2 = E[x^2] - mu^2 cancels hardest)
    lv = torch.randint(250, 256, shape, generator=g)
    sv = (lv + torch.randint(-1, 2, shape, generator=g)).clamp(0, 255)
    return sv.float() / 255 * 2 - 1, lv.float() / 255 * 2 - 1


def _host(sr, gt, crop):
    """(sse int64 [N, C], ssim float64 [N, C], the cropped ubyte HWC pairs) by the host path."""
    from basicsr4rs_amd.metrics.psnr_ssim import _ssim
    from basicsr4rs_amd.utils.img_util import minusone_one_tensor_to_ubyte_numpy
    N, C, H, W = sr.shape
    sse = np.zeros((N, C), np.int64)
    ssim = np.zeros((N, C), np.float64)
    imgs = []
    for n in range(N):
        a = minusone_one_tensor_to_ubyte_numpy(sr[n:n + 1])
        b = minusone_one_tensor_to_ubyte_numpy(gt[n:n + 1])
        assert a.shape == (H, W, C) and a.dtype == np.uint8
        imgs.append((a, b))
        a, b = a[crop:H - crop, crop:W - crop], b[crop:H - crop, crop:W - crop]
        for c in range(C):
            d = a[..., c].astype(np.int64) - b[..., c].astype(np.int64)
            sse[n, c] = int((d * d).sum())
            ssim[n, c] = _ssim(a[..., c].astype(np.float64), b[..., c].astype(np.float64))
    return sse, ssim, imgs


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,C,H,W,crop', CASES)
def test_val_metrics_match_host(cuda, N, C, H, W, crop, kind):
    from basicsr4rs_amd.metrics import calculate_psnr, calculate_psnr_band, calculate_ssim
    from basicsr4rs_amd.ops import metrics as M
    sr, gt = _inputs(kind, (N, C, H, W), seed=H * 1000 + W * 10 + crop)
    ref_sse, ref_ssim, imgs = _host(sr, gt, crop)
    srd, gtd = sr.to(cuda), gt.to(cuda)
    sse, ssim = M.val_metrics(srd, gtd, crop)
    assert sse.shape == (N, C) and sse.dtype == np.int64 and ssim.dtype == np.float64
    nan = np.isnan(ref_ssim)
    diff = np.abs(np.where(nan, 0.0, ssim - ref_ssim)).max()
    print(f'{kind} {N}x{C}x{H}x{W} crop {crop}: sse {sse.sum()} (host {ref_sse.sum()}), ssim max |diff| {diff:.3e}, '
          f'ssim range [{np.nanmin(ssim) if not nan.all() else np.nan:.6f}, {np.nanmax(ssim) if not nan.all() else np.nan:.6f}]')
    assert np.array_equal(sse, ref_sse), (sse, ref_sse)
    npix = (H - 2 * crop) * (W - 2 * crop)
    for n in range(N):
        a, b = imgs[n]
        assert M.psnr_from_sse(int(sse[n].sum()), npix * C) == calculate_psnr(a, b, crop)
        for c in range(C):
            assert M.psnr_from_sse(sse[n, c], npix) == calculate_psnr_band(a, b, crop, c), (n, c)
        if kind == 'identical':
            assert M.psnr_from_sse(sse[n, 0], npix) == float('inf')
        if not nan[n].any():
            assert abs(ssim[n].mean() - calculate_ssim(a, b, crop)) <= 1e-10
    assert np.array_equal(np.isnan(ssim), nan), (ssim, ref_ssim)
    assert nan.all() == (min(H, W) - 2 * crop < 11)
    assert diff <= 1e-10, diff
    # deterministic: a second call is bitwise the first
    sse2, ssim2 = M.val_metrics(srd, gtd, crop)
    assert sse2.tobytes() == sse.tobytes() and ssim2.tobytes() == ssim.tobytes()


def test_scores_from_device_match_calculate_metric(cuda):
    """The L2S metric list (overall + six bands, PSNR and SSIM) and a second crop_border from one
    call: the scores of calculate_metric on the host images, PSNR exactly."""
    from basicsr4rs_amd.metrics import calculate_metric
    from basicsr4rs_amd.ops import metrics as M
    from basicsr4rs_amd.utils.img_util import minusone_one_tensor_to_ubyte_numpy
    sr, gt = _inputs('noise', (1, 6, 40, 44), seed=5)
    opt = {'psnr': dict(type='calculate_psnr', crop_border=4, test_y_channel=False, better='higher'),
           'ssim': dict(type='calculate_ssim', crop_border=4, test_y_channel=False, better='higher'),
           'psnr_c0': dict(type='calculate_psnr', crop_border=0)}
    for b in range(6):
        opt[f'psnr_b{b}'] = dict(type='calculate_psnr_band', crop_border=4, test_y_channel=False, band=b)
        opt[f'ssim_b{b}'] = dict(type='calculate_ssim_band', crop_border=4, test_y_channel=False, band=b)
    got = M.scores_from_device(opt, sr.to(cuda), gt.to(cuda))
    assert list(got) == list(opt)
    data = {'img': minusone_one_tensor_to_ubyte_numpy(sr), 'img2': minusone_one_tensor_to_ubyte_numpy(gt)}
    for name, o in opt.items():
        o = {k: v for k, v in o.items() if k != 'better'}
        ref = calculate_metric(data, o)
        if 'psnr' in name:
            assert got[name] == ref, (name, got[name], ref)
        else:
            assert abs(got[name] - ref) <= 1e-10, (name, got[name], ref)
    with pytest.raises(AssertionError, match='out of range'):
        M.scores_from_device({'x': dict(type='calculate_psnr_band', crop_border=4, band=6)}, sr.to(cuda), gt.to(cuda))
