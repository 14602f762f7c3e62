"""RegisteredLoss / EncoderLoss without a GPU: the host-built taps against the reference's (bit for bit), the float64
restatement of tests/_registered_ref.py against the values recorded from the reference (tests/golden/
registered_loss.npz, written by tests/golden/make_registered_golden.py) and against autograd, the input builder of the
GPU tests, the workspace size, the registry and the refusals of the entry point and the modules."""
import ctypes
import os

import numpy as np
import pytest
import torch

from basicsr4rs_amd import _lib
from basicsr4rs_amd.losses import EncoderLoss, RegisteredLoss, ShiftConv2d, build_loss, lanczos_kernel
from basicsr4rs_amd.losses.align_loss import shift_taps

from . import _registered_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'registered_loss.npz')
GRIDS = {'unit': (-1.0, 1.0, 1.0), 'half': (-1.0, 1.0, 0.5), 'asym': (0.0, 1.5, 0.5)}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('name', list(GRIDS))
def test_taps_equal_the_reference_bit_for_bit(golden, name):
    want = golden[f'{name}.taps']
    taps = shift_taps(*GRIDS[name])
    assert taps.dtype == torch.float32 and tuple(taps.shape) == want.shape
    assert np.array_equal(taps.numpy().view(np.int32), want.view(np.int32))
    conv = ShiftConv2d(*GRIDS[name])
    S, K = want.shape
    assert tuple(conv.K_y.shape) == (S, 1, 1, K, 1) and tuple(conv.K_x.shape) == (S, 1, 1, 1, K)
    assert np.array_equal(conv.taps.numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(conv.K_y.reshape(S, K).numpy().view(np.int32), want.view(np.int32))
    # an integer shift is a near-delta, not a delta; the taps are not normalised
    row = lanczos_kernel(torch.tensor([[1.0]]), a=3)
    assert tuple(row.shape) == (1, 9) and 0.99 < row.max().item() < 1.0 and (row != 0).all()


def _ratio(got, ref, bound, what, worst):
    err = (torch.as_tensor(got).double() - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f'{what}: max|err| {err.max().item():.3e}, max err/bound {ratio:.3f}')
    worst[what.split()[-1]] = max(worst.get(what.split()[-1], 0.0), ratio)
    assert (err <= bound).all(), what


@pytest.mark.parametrize('kind', ['l1', 'mse'])
@pytest.mark.parametrize('name', list(GRIDS))
def test_restatement_agrees_with_the_reference(golden, name, kind):
    """Table, argmin, the three losses and pred.grad of the reference's fp32 CPU run within the restatement's bounds
    with the operation counts of a naive fp32 evaluation: the sum over the crop one element after another (depth n)."""
    pred, target = torch.from_numpy(golden[f'{name}.pred']), torch.from_numpy(golden[f'{name}.target'])
    T = torch.from_numpy(golden[f'{name}.taps'])
    n = pred.shape[1] * (pred.shape[2] - T.shape[1] + 1) * (pred.shape[3] - T.shape[1] + 1)
    f = R.forward_ref(pred, target, T, kind, depth=n)
    worst = {}
    _ratio(golden[f'{name}.{kind}.table'], f.table, f.b_table, f'{name} {kind} table', worst)
    assert f.idx.tolist() == golden[f'{name}.{kind}.argmin'].tolist() == golden[f'{name}.picks'].tolist()
    for red in ('mean', 'sum', 'none'):
        res = R.backward_ref(f, red)
        _ratio(golden[f'{name}.{kind}.loss_{red}'], res.loss, res.b_loss + 2 * R.U * res.loss.abs(), f'{name} {kind} {red} loss',
               worst)
        if red != 'sum':
            _ratio(golden[f'{name}.{kind}.grad_{red}'], res.grad, res.b_grad, f'{name} {kind} {red} grad', worst)
    print('worst error / bound:', {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_closed_form_gradient_matches_autograd(kind):
    f = R.build_case((0.0, 1.5, 0.5), (2, 2, 13, 16), kind)
    up = torch.tensor([0.75, -1.5], dtype=torch.float64)
    for red in ('mean', 'sum', 'none'):
        p = f.pred.clone().requires_grad_(True)
        loss = R.torch_ref(p, f.target, f.taps, kind, red, loss_weight=0.7)
        (loss * up).sum().backward() if red == 'none' else loss.backward()
        res = R.backward_ref(f, red, loss_weight=0.7, upstream=up if red == 'none' else None)
        assert torch.allclose(loss.detach(), res.loss, rtol=1e-13, atol=0)
        err = (p.grad - res.grad).abs().max().item()
        print(f'{kind} {red}: closed form against autograd {err:.3e}')
        assert err <= 1e-13 * res.grad.abs().max().item()
        # the border strips do receive gradient
        assert res.grad[:, :, 0].abs().max() > 0 and res.grad[..., -1].abs().max() > 0


@pytest.mark.parametrize('grid', [(-1.0, 1.0, 0.5), (-2.0, 2.0, 1.0), (-1.0, 1.0, 1.0), (-0.5, 0.5, 0.25), (0.0, 1.5, 0.5)])
def test_builder_separates_the_minimum(grid):
    for kind in ('l1', 'mse'):
        f = R.build_case(grid, (2, 2, 16, 19), kind)
        print(grid, kind, 'runner-up / minimum:', [round(v, 1) for v in f.runner_up])
        assert f.idx.tolist() == f.picks.tolist() and f.picks[0] != f.picks[1]


def test_workspace_holds_partials_only():
    lib = _lib.load()
    B, C, H, W, S = 12, 6, 192, 192, 9
    ws = lib.sr_registered_loss_workspace(B, C, H, W, S)
    stack = B * S * S * C * H * W * 4
    print(f'workspace {ws} B, one shift stack {stack} B, ratio {ws / stack:.5f}')
    assert 0 < ws < stack / 100
    assert lib.sr_registered_loss_workspace(B, C, H, W, 10) == 0


def test_entry_point_refusals():
    lib = _lib.load()
    p = ctypes.c_void_p(64)

    def call(kind=0, S=5, K=9, B=1, C=1, H=16, W=16, pdt=0, tdt=0, taps=p, ws=1 << 24):
        return lib.sr_registered_loss(kind, _lib.REDUCE_MEAN, pdt, tdt, p, p, taps, S, K, B, C, H, W, 1.0, p, p, None, None, p,
                                      ws, None)

    for kw, why in ((dict(kind=_lib.LOSS_CHARBONNIER), b'kind'), (dict(S=10), b'S must be'), (dict(K=15), b'K must be'),
                    (dict(K=8), b'K must be'), (dict(H=8), b'at least K'), (dict(W=8), b'at least K'),
                    (dict(B=8, C=4, H=8192, W=8192), b'below 2^31'), (dict(pdt=0, tdt=1), b'dtype'), (dict(taps=None), b'null'),
                    (dict(ws=16), b'workspace too small')):
        assert call(**kw) == -1, kw
        assert b'registered_loss' in lib.sr_last_error() and why in lib.sr_last_error(), (kw, lib.sr_last_error())


def test_registry_and_module_refusals():
    loss = build_loss({'type': 'RegisteredLoss', 'start': -2, 'end': 2, 'step': 0.5, 'loss_func': 'L1'})
    assert isinstance(loss, RegisteredLoss) and tuple(loss._shiftconv2d.taps.shape) == (9, 11) and loss.last_shift is None
    assert isinstance(build_loss({'type': 'RegisteredLoss', 'start': -1, 'end': 1, 'step': 0.5, 'loss_func': 'l2'}),
                      RegisteredLoss)
    assert isinstance(build_loss({'type': 'EncoderLoss'}), EncoderLoss)
    with pytest.raises(ValueError, match='loss_func'):
        RegisteredLoss(-1, 1, 0.5, 'huber')
    with pytest.raises(ValueError, match='strategy'):
        EncoderLoss(strategy='both')
    x = torch.zeros(1, 1, 12, 12)
    with pytest.raises(NotImplementedError):
        RegisteredLoss(-1, 1, 0.5, 'l1')(x, x)
    with pytest.raises(NotImplementedError):
        RegisteredLoss(-1, 1, 0.5, 'l1')._shifted_loss(x, x)
    with pytest.raises(NotImplementedError):
        EncoderLoss()(x, x, x)
    with pytest.raises(TypeError):
        EncoderLoss()(x, x)  # lq is required


def test_shiftconv_stack_matches_the_restatement():
    """ShiftConv2d.forward (torch ops, here on the CPU) against the direct sums: the order sy * S + sx and the
    direction of the correlation."""
    conv = ShiftConv2d(0.0, 1.5, 0.5)
    x = torch.rand(2, 2, 12, 15, generator=torch.Generator().manual_seed(3))
    got = conv(x)
    ref = R.shift_all(x.double(), conv.taps.double())
    assert tuple(got.shape) == (2, 16, 2, 12, 15)
    assert (got.double() - ref).abs().max().item() < 1e-5
