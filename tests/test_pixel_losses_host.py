"""Pixel-loss family, host side (no GPU): the registry resolves MSELoss / CharbonnierLoss / WeightedTVLoss
with the reference's defaults (basicsr/losses/basic_loss.py:55-143), the constructors refuse what the
reference refuses, CPU tensors are refused, and the ctypes layer declares the two new entry points."""
import ctypes
import inspect

import pytest
import torch

from basicsr4rs_amd import _lib
from basicsr4rs_amd.losses import CharbonnierLoss, L1Loss, MSELoss, WeightedTVLoss, build_loss


def test_build_loss_resolves_family_with_reference_defaults():
    mse = build_loss(dict(type='MSELoss'))
    assert type(mse) is MSELoss and (mse.loss_weight, mse.reduction) == (1.0, 'mean')
    ch = build_loss(dict(type='CharbonnierLoss'))
    assert type(ch) is CharbonnierLoss and (ch.loss_weight, ch.reduction, ch.eps) == (1.0, 'mean', 1e-12)
    tv = build_loss(dict(type='WeightedTVLoss'))
    assert type(tv) is WeightedTVLoss and isinstance(tv, L1Loss) and (tv.loss_weight, tv.reduction) == (1.0, 'mean')
    ch = build_loss(dict(type='CharbonnierLoss', loss_weight=0.5, reduction='sum', eps=1e-6))
    assert (ch.loss_weight, ch.reduction, ch.eps) == (0.5, 'sum', 1e-6)
    # constructor and forward signatures of the reference
    assert list(inspect.signature(MSELoss.__init__).parameters) == ['self', 'loss_weight', 'reduction']
    assert list(inspect.signature(CharbonnierLoss.__init__).parameters) == ['self', 'loss_weight', 'reduction', 'eps']
    assert list(inspect.signature(WeightedTVLoss.__init__).parameters) == ['self', 'loss_weight', 'reduction']
    for cls in (L1Loss, MSELoss, CharbonnierLoss):
        assert list(inspect.signature(cls.forward).parameters) == ['self', 'pred', 'target', 'weight', 'kwargs']
    assert list(inspect.signature(WeightedTVLoss.forward).parameters) == ['self', 'pred', 'weight']


@pytest.mark.parametrize('name', ['L1Loss', 'MSELoss', 'CharbonnierLoss', 'WeightedTVLoss'])
def test_bad_reduction_raises(name):
    with pytest.raises(ValueError, match='Unsupported reduction mode: average'):
        build_loss(dict(type=name, reduction='average'))


def test_tv_refuses_reduction_none():
    with pytest.raises(ValueError, match='Supported ones are: mean | sum'):
        WeightedTVLoss(reduction='none')
    for cls in (L1Loss, MSELoss, CharbonnierLoss):
        assert cls(reduction='none').reduction == 'none'


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
def test_cpu_tensors_raise(reduction):
    a, b, w = torch.rand(1, 3, 4, 4), torch.rand(1, 3, 4, 4), torch.rand(1, 1, 4, 4)
    for cls in (L1Loss, MSELoss, CharbonnierLoss):
        for weight in (None, w):
            with pytest.raises(NotImplementedError, match='run on the MI355X device'):
                cls(reduction=reduction)(a, b, weight)
    if reduction != 'none':
        for weight in (None, w):
            with pytest.raises(NotImplementedError, match='run on the MI355X device'):
                WeightedTVLoss(reduction=reduction)(a, weight)


def test_lib_declares_pixel_loss_symbols():
    assert 'sr_pixel_loss' in _lib.SIGNATURES and 'sr_pixel_loss_workspace' in _lib.SIGNATURES
    res, args = _lib.SIGNATURES['sr_pixel_loss']
    assert res is ctypes.c_int and len(args) == 20
    assert _lib.SIGNATURES['sr_pixel_loss_workspace'] == (ctypes.c_size_t, [ctypes.c_int64])
    lib = _lib.load()
    assert lib.sr_pixel_loss_workspace(1) >= 8
    # argument validation happens before any launch: SR_EINVAL and a message
    dummy = ctypes.c_void_p(16)
    ws = lib.sr_pixel_loss_workspace(48)
    rc = lib.sr_pixel_loss(7, _lib.REDUCE_MEAN, 0, 0, dummy, dummy, None, 0, 1, 3, 4, 4, 1.0, 0.0, dummy, None, None,
                           dummy, ws, None)
    assert rc == -1 and b'unknown loss kind' in lib.sr_last_error()
    rc = lib.sr_pixel_loss(_lib.LOSS_MSE, _lib.REDUCE_MEAN, 0, 0, dummy, dummy, dummy, 2, 1, 3, 4, 4, 1.0, 0.0, dummy,
                           None, None, dummy, ws, None)
    assert rc == -1 and b'1 or C channels' in lib.sr_last_error()
    rc = lib.sr_pixel_loss(_lib.LOSS_MSE, _lib.REDUCE_NONE, 0, 0, dummy, dummy, None, 0, 1, 3, 4, 4, 1.0, 0.0, dummy,
                           None, None, dummy, ws, None)
    assert rc == -1 and b"'none' needs out" in lib.sr_last_error()
    rc = lib.sr_pixel_loss(_lib.LOSS_L1, _lib.REDUCE_SUM, 0, 1, dummy, dummy, None, 0, 1, 3, 4, 4, 1.0, 0.0, dummy,
                           None, None, dummy, ws, None)
    assert rc == -1 and b"pred's dtype" in lib.sr_last_error()
    rc = lib.sr_pixel_loss(_lib.LOSS_L1, _lib.REDUCE_SUM, 0, 0, dummy, dummy, None, 0, 1, 3, 4, 4, 1.0, 0.0, dummy,
                           None, None, dummy, ws - 1, None)
    assert rc == -1 and b'workspace too small' in lib.sr_last_error()
