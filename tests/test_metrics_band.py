"""The Landsat-to-Sentinel surface without a GPU: the per-band PSNR / SSIM metrics
(basicsr/metrics/psnr_ssim.py:51-88, 171-206), the host-side refusals of sr_val_metrics and
sr_bicubic_up_hp, and the two L2S option files (stored unchanged under tests/golden/reference_options/)
resolving their model and metric types."""
import ctypes
import os

import numpy as np
import pytest

from basicsr4rs_amd import _lib

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_options')
SWINIR_L2S = 'train/SwinIR/train_SwinIR_L2S288_scratch.yml'
SRCNN_L2S = 'train/SRCNN/train_SRCNN_L2S288.yml'


@pytest.fixture(scope='module')
def pair():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (23, 31, 6), dtype=np.uint8)
    noise = rng.integers(-9, 10, a.shape)
    b = np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return a, b


def test_band_metrics_registered():
    import basicsr4rs_amd.metrics as M
    from basicsr4rs_amd.utils.registry import METRIC_REGISTRY
    for name in ('calculate_psnr_band', 'calculate_ssim_band'):
        assert name in METRIC_REGISTRY and name in M.__all__ and callable(getattr(M, name))


@pytest.mark.parametrize('crop', [0, 3])
def test_band_metrics_match_single_channel(pair, crop):
    from basicsr4rs_amd.metrics import calculate_psnr, calculate_psnr_band, calculate_ssim, calculate_ssim_band
    from basicsr4rs_amd.metrics.psnr_ssim import _ssim
    a, b = pair
    ac, bc = a.transpose(2, 0, 1), b.transpose(2, 0, 1)
    ssims = []
    for band in range(6):
        p_hwc = calculate_psnr_band(a, b, crop, band)
        p_chw = calculate_psnr_band(ac, bc, crop, band, input_order='CHW')
        assert p_hwc == p_chw == calculate_psnr(a[..., band:band + 1], b[..., band:band + 1], crop)
        assert np.isfinite(p_hwc)
        s_hwc = calculate_ssim_band(a, b, crop, band)
        s_chw = calculate_ssim_band(ac, bc, crop, band, input_order='CHW')
        sl = (slice(crop, a.shape[0] - crop), slice(crop, a.shape[1] - crop), band)
        assert s_hwc == s_chw == _ssim(a[sl].astype(np.float64), b[sl].astype(np.float64))
        assert 0.0 < s_hwc < 1.0
        ssims.append(s_hwc)
    assert abs(np.mean(ssims) - calculate_ssim(a, b, crop)) <= 1e-15
    # calculate_psnr_band forwards test_y_channel (a one-channel image stays as it is, rescaled through
    # float32); calculate_ssim_band has no such parameter and does not apply the key
    assert calculate_psnr_band(a, b, crop, 2, test_y_channel=True) == calculate_psnr(a[..., 2:3], b[..., 2:3], crop,
                                                                                   test_y_channel=True)
    assert calculate_ssim_band(a, b, crop, 2, test_y_channel=True) == ssims[2]


def test_band_index_out_of_range(pair):
    from basicsr4rs_amd.metrics import calculate_psnr_band, calculate_ssim_band
    a, b = pair
    for fn in (calculate_psnr_band, calculate_ssim_band):
        with pytest.raises(AssertionError, match='out of range'):
            fn(a, b, 0, 6)
        with pytest.raises(AssertionError, match='out of range'):
            fn(a.transpose(2, 0, 1), b.transpose(2, 0, 1), 0, 6, input_order='CHW')
        with pytest.raises(AssertionError, match='shapes are different'):
            fn(a, b[:-1], 0, 0)
        with pytest.raises(ValueError, match='input_order'):
            fn(a, b, 0, 0, input_order='WHC')


def test_val_metrics_refusals_are_host_side():
    """Every invalid argument returns SR_EINVAL before any HIP call (the pointers are not device memory)."""
    lib = _lib.load()
    d = ctypes.c_void_p(4096)
    ws = lib.sr_val_metrics_workspace(1, 6, 37, 53, 4)
    assert ws > 0 and ws % 8 == 0
    assert lib.sr_val_metrics_workspace(2, 6, 48, 80, 4) == 2 * lib.sr_val_metrics_workspace(1, 6, 48, 80, 4)
    good = dict(sr=d, gt=d, N=1, C=6, H=37, W=53, crop=4, sse=d, ssim=d, ws=d, ws_bytes=ws)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sr_val_metrics(a['sr'], a['gt'], a['N'], a['C'], a['H'], a['W'], a['crop'], a['sse'], a['ssim'],
                                  a['ws'], a['ws_bytes'], None)

    for key in ('sr', 'gt', 'sse', 'ssim', 'ws'):
        assert call(**{key: None}) == -1 and b'null pointer' in lib.sr_last_error(), key
    for key in ('N', 'C', 'H', 'W'):
        for bad in (0, -1):
            assert call(**{key: bad}) == -1 and b'>= 1' in lib.sr_last_error(), (key, bad)
            assert lib.sr_val_metrics_workspace(*[dict(good, **{key: bad})[k] for k in ('N', 'C', 'H', 'W', 'crop')]) == 0
    assert call(crop=-1) == -1 and b'crop' in lib.sr_last_error()
    assert call(crop=19) == -1 and b'crop' in lib.sr_last_error()      # 2 * 19 >= 37
    assert call(H=8, crop=4) == -1 and b'crop' in lib.sr_last_error()  # 2 * 4 >= 8
    assert lib.sr_val_metrics_workspace(1, 6, 37, 53, 19) == 0
    assert lib.sr_val_metrics_workspace(1, 6, 37, 53, 18) > 0
    assert call(ws_bytes=ws - 1) == -1 and b'workspace too small' in lib.sr_last_error()
    assert call(ws_bytes=0) == -1
    with pytest.raises(RuntimeError, match='workspace too small'):
        _lib.check(-1)


def test_bicubic_up_hp_refusals_are_host_side():
    lib = _lib.load()
    d = ctypes.c_void_p(4096)

    def call(x=d, N=1, C=3, H=4, W=4, s=2, y=d, Cy=6, c0=3):
        return lib.sr_bicubic_up_hp(x, N, C, H, W, s, y, Cy, c0, None)

    assert call(x=None) == -1 and b'null pointer' in lib.sr_last_error()
    assert call(y=None) == -1 and b'null pointer' in lib.sr_last_error()
    for key in ('N', 'C', 'H', 'W', 's'):
        for bad in (0, -2):
            assert call(**{key: bad}) == -1 and b'bad shape' in lib.sr_last_error(), (key, bad)
    assert call(c0=-1) == -1 and b'c0' in lib.sr_last_error()
    assert call(c0=4) == -1 and b'c0' in lib.sr_last_error()   # 4 + 3 > 6
    assert call(Cy=2, c0=0) == -1 and b'c0' in lib.sr_last_error()
    assert call(H=1 << 30, s=4) == -3 and b'too large' in lib.sr_last_error()  # SR_ETOOBIG


def test_bicubic_up_hp_op_argument_checks():
    import torch

    from basicsr4rs_amd.ops import convk as K
    with pytest.raises(NotImplementedError, match='gradient'):
        K.bicubic_up_hp(torch.zeros(1, 3, 4, 4, requires_grad=True), 2)
    with pytest.raises(ValueError, match='scale'):
        K.bicubic_up_hp(torch.zeros(1, 3, 4, 4), 1.5)
    with pytest.raises(ValueError, match='out must be'):
        K.bicubic_up_hp(torch.zeros(1, 3, 4, 4), 2, out=torch.zeros(1, 6, 8, 9), c0=3)
    with pytest.raises(NotImplementedError):
        K.bicubic_up_hp(torch.zeros(1, 3, 4, 4), 2)  # CPU tensors: no CPU path


def _parse(rel, tmp_path):
    import basicsr4rs_amd.archs  # noqa: F401
    import basicsr4rs_amd.metrics  # noqa: F401
    import basicsr4rs_amd.models  # noqa: F401
    from basicsr4rs_amd.utils.options import parse_options
    assert os.path.exists(os.path.join(REF, rel)), rel
    opt, _ = parse_options(str(tmp_path), is_train=True, argv=['-opt', os.path.join(REF, rel)])
    return opt


def test_swinir_l2s_yaml_resolves(tmp_path):
    from basicsr4rs_amd.models.srrs_l2s_model import L2SSingleModel
    from basicsr4rs_amd.models.swinir_model import SwinIRL2sModel, SwinIRModel
    from basicsr4rs_amd.utils.registry import METRIC_REGISTRY, MODEL_REGISTRY
    opt = _parse(SWINIR_L2S, tmp_path)
    assert opt['model_type'] == 'SwinIRL2sModel' and opt['model_type'] in MODEL_REGISTRY
    assert MODEL_REGISTRY.get('SwinIRL2sModel') is SwinIRL2sModel
    kinds = [m['type'] for m in opt['val']['metrics'].values()]
    assert len(kinds) == 20 and kinds.count('calculate_lpips_band') == 6
    assert kinds.count('calculate_psnr_band') == kinds.count('calculate_ssim_band') == 6
    for kind in kinds:
        if kind != 'calculate_lpips_band':  # needs pretrained weights: out of scope
            assert kind in METRIC_REGISTRY, kind
    bands = [m['band'] for m in opt['val']['metrics'].values() if m['type'] == 'calculate_ssim_band']
    assert bands == list(range(6))
    mro = SwinIRL2sModel.__mro__
    assert mro.index(SwinIRModel) < mro.index(L2SSingleModel)  # SwinIRModel.test pads to the window
    assert SwinIRL2sModel.feed_data is L2SSingleModel.feed_data and SwinIRL2sModel.test is SwinIRModel.test


def test_srcnn_l2s_yaml_resolves(tmp_path):
    from basicsr4rs_amd.utils.registry import METRIC_REGISTRY, MODEL_REGISTRY
    opt = _parse(SRCNN_L2S, tmp_path)
    assert opt['model_type'] == 'L2SSingleModel' and opt['model_type'] in MODEL_REGISTRY
    metrics = opt['val']['metrics']
    assert len(metrics) >= 2
    for name, m in metrics.items():
        assert m['type'] in METRIC_REGISTRY, (name, m['type'])
