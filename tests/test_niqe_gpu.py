"""sr_niqe_moments (csrc/niqe.hip) against the host NIQE (metrics/niqe.py), which tests/test_niqe_host.py pins
to the reference.  The device replaces niqe_plane and niqe_moments; both sides share niqe_from_moments.

* plane: exactly the host's;
* scale-1 counts: |difference| at most the number of host MSCN elements of that block with |n| <= 1e-6 (the
  sign of such an element is below float32 resolution); the inputs leave that set empty in at least 9 of 10
  blocks (checked on the CPU);
* scale-1 sums: relative 1e-6 (float32 storage rounding is 6e-8 per element: a 10 x margin);
* scale-2 sums pass through the float32 resample: 10 x the largest relative difference measured on an
  MI355X (S2_MEASURED), never looser than 1e-4;
* scores: niqe_from_moments on the device moments against the host score, 10 x the largest relative
  difference measured (SCORE_MEASURED) with 1e-3 as a hard cap (logs print four decimals); NaN matches NaN;
* two launches give bitwise-equal moments;
* the model path: SRRSModel.nondist_validation with val.device_metrics writes the host run's table.

Measured on an MI355X over all cases and inputs below: scale-1 MSCN maps equal to the host's bit for bit,
counts equal, scale-1 sums 4.3e-16, scale-2 sums 4.3e-16, scores 3.2e-14 (relative); also in DESIGN.md.
"""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from basicsr4rs_amd.metrics import niqe as Q

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PARAMS = os.path.join(GOLDEN, 'niqe_pris_params.npz')

# largest relative differences seen on an MI355X over every case below (printed by the tests): the planes and
# the MSCN maps come out bit for bit, so what is left is the order of the float64 block sums (scale-1 sums
# 4.3e-16 as well) and what the pseudo-inverse makes of it in the score
S2_MEASURED = 4.3e-16
SCORE_MEASURED = 3.2e-14
S1_BOUND = 1e-6
S2_BOUND = min(1e-4, 10 * S2_MEASURED)
SCORE_BOUND = min(1e-3, 10 * SCORE_MEASURED)

N, C = 2, 4
# (H, W, crop): the smallest shapes that exercise each index path
SHAPES = [
    (192, 192, 0),  # 2 x 2 blocks, no crop, exact multiples of 96
    (200, 296, 4),  # 2 x 3, non-square, border crop
    (205, 301, 4),  # 197 x 293 truncated to 2 x 3: top-left truncation
    (96, 192, 0),   # 1 x 2: two rows in the covariance
    (100, 100, 0),  # one block: host and device both return NaN
]
# every input kind on the 2 x 3 shape, the smooth one on every shape
CASES = [(s, 'smooth') for s in SHAPES] + [(SHAPES[1], k) for k in ('uniform', 'clamp', 'const_block')]
IDS = [f'{h}x{w}c{c}-{k}' for (h, w, c), k in CASES]
# the planes: every single band of both images, and the BGR -> Y selection [2, 1, 0]
PLANES = [(n, (c,)) for n in range(N) for c in range(C)] + [(n, (2, 1, 0)) for n in range(N)]


def _input(kind, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + len(kind))
    if kind == 'uniform':
        return torch.rand(N, C, H, W, generator=g) * 2 - 1
    if kind == 'clamp':  # values outside [-1, 1]
        return torch.rand(N, C, H, W, generator=g) * 2.6 - 1.3
    # low-pass-filtered noise scaled into [-1, 1]
    x = torch.randn(N * C, 1, H + 8, W + 8, generator=g)
    k = torch.tensor([1., 4., 6., 4., 1.])
    k = (k[:, None] * k[None, :] / 256).view(1, 1, 5, 5)
    x = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, k), k).view(N, C, H, W)
    x = x / x.abs().amax(dim=(2, 3), keepdim=True)
    if kind == 'const_block':
        # one constant 96 x 96 block of the cropped plane (block row 1, column 1 with crop 4) with the 3-pixel
        # reach of the window around it: its scale-1 MSCN is zero, its features NaN, the row is dropped
        x[:, :, 100 - 3:, 100 - 3:196 + 3] = 0.25
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _host(shape, kind):
    """The input and, per plane, the host's (plane, scale-1 MSCN, moments, score): computed once, shared."""
    from basicsr4rs_amd.utils.img_util import minusone_one_tensor_to_ubyte_numpy
    H, W, crop = shape
    mu, cov, window = Q.load_niqe_params(PARAMS)
    x = _input(kind, H, W)
    out = []
    for n, ch in PLANES:
        img = minusone_one_tensor_to_ubyte_numpy(x[n:n + 1])  # HWC ubyte
        if len(ch) == 1:
            plane = Q.niqe_plane(img, crop, convert_to=None, band=ch[0])
        else:
            plane = Q.niqe_plane(img, crop, convert_to='y', input_bands=list(ch))
        mom, maps = Q.niqe_moments(plane, window, return_mscn=True)
        score = Q.niqe_from_moments(mom, mu, cov) if mom.shape[1] * mom.shape[2] else float('nan')
        out.append((plane, maps[0], mom, score))
    return x, out


def _near_zero(n1, i, j):
    return int((np.abs(n1[i * 96:(i + 1) * 96, j * 96:(j + 1) * 96]) <= 1e-6).sum())


def test_inputs_leave_sign_unambiguous_in_nine_of_ten_blocks():
    """CPU: over the inputs of this file, at most one block in ten holds an MSCN element with |n| <= 1e-6."""
    blocks = ambiguous = 0
    for shape, kind in CASES[1:2] + CASES[5:]:  # the 2 x 3 shape with every input kind
        for plane, n1, mom, _ in _host(shape, kind)[1]:
            for i in range(mom.shape[1]):
                for j in range(mom.shape[2]):
                    blocks += 1
                    ambiguous += _near_zero(n1, i, j) > 0
    print(f'{ambiguous} of {blocks} blocks hold an element with |n| <= 1e-6')
    assert blocks >= 200 and ambiguous * 10 <= blocks


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


@gpu
@pytest.mark.parametrize('shape,kind', CASES, ids=IDS)
def test_device_moments_match_host(cuda, shape, kind):
    from basicsr4rs_amd.ops import metrics as M
    H, W, crop = shape
    mu, cov, window = Q.load_niqe_params(PARAMS)
    x, host = _host(shape, kind)
    xd = x.to(cuda)
    mom_d, planes_d, mscn_d = M.niqe_moments_device(xd, PLANES, crop, window, return_maps=True)
    again = M.niqe_moments_device(xd, PLANES, crop, window)
    assert torch.equal(mom_d.view(torch.int64), again.view(torch.int64)), 'two launches differ'
    mom_d, planes_d, mscn_d = mom_d.cpu().numpy(), planes_d.cpu().numpy(), mscn_d.cpu().numpy()
    worst = dict(s1=0.0, s2=0.0, score=0.0, count=0, mscn=0.0)
    sums = [Q.SS_NEG, Q.SS_POS, Q.SUM_ABS, Q.SUM_SQ]
    for p, (plane, n1, mom, score) in enumerate(host):
        assert np.array_equal(planes_d[p], plane), f'plane {PLANES[p]}'
        worst['mscn'] = max(worst['mscn'], float(np.abs(mscn_d[p] - n1).max()))
        assert mom_d[p].shape == mom.shape
        for i in range(mom.shape[1]):
            for j in range(mom.shape[2]):
                slack = _near_zero(n1, i, j)
                for k in (Q.N_NEG, Q.N_POS):
                    dc = np.abs(mom_d[p][0, i, j, :, k] - mom[0, i, j, :, k]).max()
                    worst['count'] = max(worst['count'], int(dc))
                    assert dc <= slack, (PLANES[p], i, j, dc, slack)
        # sums: where the host's is zero (a constant block) the device's is zero too
        for s, key in ((0, 's1'), (1, 's2')):
            h, d = mom[s][..., sums], mom_d[p][s][..., sums]
            assert np.array_equal(d[h == 0], h[h == 0])
            if (h != 0).any():
                worst[key] = max(worst[key], float(_rel(d[h != 0], h[h != 0]).max()))
        got = Q.niqe_from_moments(mom_d[p], mu, cov) if mom.shape[1] * mom.shape[2] else float('nan')
        if np.isnan(score):
            assert np.isnan(got), (PLANES[p], got)
        else:
            worst['score'] = max(worst['score'], abs(got - score) / abs(score))
    print(f'niqe {shape} {kind}: scale-1 sums rel {worst["s1"]:.3e}, scale-2 sums rel {worst["s2"]:.3e}, '
          f'score rel {worst["score"]:.3e}, count diff {worst["count"]}, mscn max abs diff {worst["mscn"]:.3e}')
    assert worst['s1'] <= S1_BOUND
    assert worst['s2'] <= S2_BOUND
    assert worst['score'] <= SCORE_BOUND
    if shape == (100, 100, 0):
        assert all(np.isnan(h[3]) for h in host)
    if kind == 'const_block':  # the constant block's features are NaN on both sides, the row is dropped
        for p, (plane, n1, mom, score) in enumerate(host):
            assert (mom[0, 1, 1, :, Q.N_NEG] == 0).all() and (mom_d[p][0, 1, 1, :, Q.N_NEG] == 0).all()
            assert np.isnan(Q.features_from_moments(mom_d[p][0], 96.0 * 96.0)[1, 1]).any()
            assert np.isfinite(score)


@gpu
def test_baboon_rs_niqe_device_matches_host(cuda):
    from PIL import Image

    from basicsr4rs_amd.metrics import calculate_metric
    from basicsr4rs_amd.ops import metrics as M
    from basicsr4rs_amd.utils.img_util import minusone_one_tensor_to_ubyte_numpy
    rgb = np.array(Image.open(os.path.join(GOLDEN, 'baboon.png')).convert('RGB'))
    x = torch.from_numpy(rgb.transpose(2, 0, 1).copy()).float()[None] / 255 * 2 - 1
    img = minusone_one_tensor_to_ubyte_numpy(x)
    assert np.array_equal(img, rgb)
    opt = dict(type='calculate_rs_niqe', crop_border=0, input_bands=[2, 1, 0], params_path=PARAMS)
    host = calculate_metric(dict(img=img, img2=None), opt)
    dev = M.niqe_scores_from_device({'niqe': opt}, x.to(cuda))['niqe']
    print(f'baboon calculate_rs_niqe [2, 1, 0]: host {host!r} device {dev!r}')
    assert abs(dev - host) <= SCORE_BOUND * abs(host)


class _ValSet(torch.utils.data.Dataset):
    """Two synthetic 4-band [-1, 1] pairs, 50 x 50 LR and 200 x 200 GT."""

    def __init__(self):
        self.opt = {'name': 'RS_val'}
        g = torch.Generator().manual_seed(5)
        self.items = []
        for i in range(2):
            gt = _input('smooth', 200, 200)[i]
            lq = torch.nn.functional.avg_pool2d(gt[None], 4)[0] + 0.02 * torch.randn(4, 50, 50, generator=g)
            self.items.append({'lq': lq, 'gt': gt, 'lq_path': f'val/lq/tile_{i}.png'})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


SWINIR = dict(type='SwinIR', upscale=4, in_chans=4, img_size=16, window_size=8, img_range=1., depths=[2], embed_dim=60,
              num_heads=[6], mlp_ratio=2, upsampler='pixelshuffle', resi_connection='1conv', drop_path_rate=0.)


def _model(tmp_path, metrics):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    opt = dict(model_type='SwinIRRSModel', name='niqe_val', is_train=False, dist=False, num_gpu=1, scale=4,
               network_g=dict(SWINIR), path={'visualization': str(tmp_path / 'vis')}, val=dict(metrics=metrics))
    torch.manual_seed(0)
    return build_model(opt)


def _validate(model, loader, it, tmp_path):
    model.nondist_validation(loader, it, None, save_img=False)
    rows = list(csv.reader(open(tmp_path / 'vis' / f'RS_val_{it}.csv')))
    return dict(model.metric_results), rows


@gpu
def test_model_validation_device_niqe_matches_host(cuda, tmp_path):
    metrics = {
        'psnr': dict(type='calculate_psnr', crop_border=4, test_y_channel=False),
        'ssim': dict(type='calculate_ssim', crop_border=4, test_y_channel=False),
        'niqe_rgb': dict(type='calculate_rs_niqe', crop_border=4, input_bands=[2, 1, 0], params_path=PARAMS),
        'niqe_nir': dict(type='calculate_rs_niqe', crop_border=4, input_bands=[3], params_path=PARAMS),
        'niqe_b0': dict(type='calculate_niqe_band', crop_border=0, band=0, params_path=PARAMS),
    }
    model = _model(tmp_path, metrics)
    loader = torch.utils.data.DataLoader(_ValSet(), batch_size=1)
    host, host_rows = _validate(model, loader, 1, tmp_path)
    model.opt['val']['device_metrics'] = True
    dev, dev_rows = _validate(model, loader, 2, tmp_path)
    assert not getattr(model, '_device_metrics_warned', None), 'the device path fell back to the host'
    assert host_rows[0] == dev_rows[0] == [''] + list(metrics)
    assert [r[0] for r in host_rows[1:]] == [r[0] for r in dev_rows[1:]] == ['val/lq/tile_0', 'val/lq/tile_1']
    for hr, dr in zip(host_rows[1:], dev_rows[1:]):
        for name, h, d in zip(host_rows[0][1:], hr[1:], dr[1:]):
            print(f'{hr[0]} {name}: host {h} device {d}')
            if name == 'psnr':
                assert h == d
            elif name == 'ssim':
                assert abs(float(h) - float(d)) <= 1e-10
            else:
                assert np.isfinite(float(h)) and abs(float(h) - float(d)) <= SCORE_BOUND * abs(float(h)), name
    for name in metrics:
        assert abs(dev[name] - host[name]) <= SCORE_BOUND * abs(host[name]), name


@gpu
def test_model_validation_lpips_entry_still_falls_back(cuda, tmp_path):
    """An entry the kernels do not stand in for: one warning, the whole image on the host (where the
    registry then has no LPIPS, as before this metric family)."""
    metrics = {'niqe_b0': dict(type='calculate_niqe_band', crop_border=0, band=0, params_path=PARAMS),
               'lpips_b0': dict(type='calculate_lpips_band', crop_border=0, band=0)}
    model = _model(tmp_path, metrics)
    model.opt['val']['device_metrics'] = True
    item = _ValSet().items[0]
    model.feed_data({'lq': item['lq'][None], 'gt': item['gt'][None]})
    model.test()
    assert not model._device_metrics_ok()
    assert len(model._device_metrics_warned) == 1 and 'calculate_lpips_band' in next(iter(model._device_metrics_warned))
    loader = torch.utils.data.DataLoader(_ValSet(), batch_size=1)
    with pytest.raises(KeyError):
        model.nondist_validation(loader, 1, None, save_img=False)
    # a NIQE entry outside the kernel's envelope falls back too, with its own reason
    model.opt['val']['metrics'] = {'niqe': dict(type='calculate_rs_niqe', crop_border=60, input_bands=[2, 1, 0],
                                                params_path=PARAMS)}
    model.feed_data({'lq': item['lq'][None], 'gt': item['gt'][None]})
    model.test()
    assert not model._device_metrics_ok()
    assert any('smaller than one 96 x 96 block' in w for w in model._device_metrics_warned)


@gpu
def test_argument_validation_returns_errors(cuda):
    from basicsr4rs_amd import _lib
    lib = _lib.load()
    window = Q.load_niqe_params(PARAMS)[2]
    win = (ctypes.c_double * 49)(*window.reshape(-1))
    coef = (ctypes.c_double * 4)(24.966, 128.553, 65.481, 16.0)
    x = torch.zeros(1, 4, 200, 200, device=cuda)
    need = lib.sr_niqe_moments_workspace(1, 4, 200, 200, 4, 2)
    assert need == 2 * 192 * 192 * 3 * 4
    ws = torch.empty(need // 4, device=cuda)
    mom = torch.full((2, 2, 2, 2, 5, 6), -7.0, device=cuda, dtype=torch.float64)

    def call(H, W, crop, desc, ws_bytes):
        d = (ctypes.c_int * len(desc))(*desc)
        return lib.sr_niqe_moments(_lib.ptr(x), 1, 4, H, W, crop, len(desc) // 4, ctypes.cast(d, ctypes.c_void_p),
                                   ctypes.cast(coef, ctypes.c_void_p), ctypes.cast(win, ctypes.c_void_p),
                                   _lib.ptr(mom), None, None, _lib.ptr(ws), ws_bytes, _lib.stream())

    good = [0, 0, -1, -1, 0, 2, 1, 0]
    assert call(200, 200, 4, good, need - 4) == -1 and b'workspace too small' in lib.sr_last_error()
    assert lib.sr_niqe_moments_workspace(1, 4, 200, 103, 4, 2) == 0
    assert call(200, 103, 4, good, need) == -1 and b'at least 96' in lib.sr_last_error()
    assert call(95, 200, 0, good, need) == -1 and b'at least 96' in lib.sr_last_error()
    assert call(200, 200, 4, [0, 4, -1, -1, 0, 2, 1, 0], need) == -1 and b'channel index' in lib.sr_last_error()
    assert call(200, 200, 4, [0, 0, -1, -1, 0, 2, 1, 4], need) == -1 and b'channel index' in lib.sr_last_error()
    assert call(200, 200, 4, [1, 0, -1, -1, 0, 2, 1, 0], need) == -1 and b'image index' in lib.sr_last_error()
    assert lib.sr_niqe_moments_workspace(1, 4, 200, 200, 4, 65) == 0
    torch.cuda.synchronize()
    assert (mom == -7.0).all(), 'a refused call launched something'
    assert call(200, 200, 4, good, need) == 0
    torch.cuda.synchronize()
    assert (mom != -7.0).all()
