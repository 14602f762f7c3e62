"""RegisteredLoss on the kernels of csrc/regloss.hip against the float64 restatement of tests/_registered_ref.py under
its derived bounds (u = 2^-24; a bf16 gradient within one bf16 ulp of the rounded reference plus the fp32 bound),
each measured error printed beside its bound; the tie and NaN rules of the selection; the refusals and the torch
fallback; EncoderLoss against the values recorded from the reference (tests/golden/registered_loss.npz).

Shapes: the smallest places the kernels can go wrong -- a crop of one pixel; the reference test's configuration;
K = 11 with a crop one row high and 6 bands; an asymmetric grid with S = 4 and an odd width (catches a transposed
sy / sx or a flipped correlation); S = 9 (81 accumulators); several tiles with remainders in both directions and
halos crossing tile edges; and the two tap counts the other cases leave out, K = 13 and K = 7 (a single shift)."""
import os

import numpy as np
import pytest
import torch

from . import _degrade_ref as DR
from . import _registered_ref as R
from ._fp64 import U, _bits, _check, _ids

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'registered_loss.npz')

CASES = [
    ((-1.0, 1.0, 1.0), (1, 1, 9, 9)),
    ((-1.0, 1.0, 0.5), (2, 3, 15, 18)),
    ((-2.0, 2.0, 1.0), (2, 6, 11, 70)),
    ((0.0, 1.5, 0.5), (1, 2, 40, 37)),
    ((-2.0, 2.0, 0.5), (1, 1, 13, 14)),
    ((-1.0, 1.0, 0.5), (2, 3, 70, 135)),
    ((-3.0, 3.0, 1.5), (2, 2, 14, 29)),
    ((0.0, 0.0, 1.0), (2, 1, 8, 9)),
]
LW = 0.7


def _case_id(c):
    return f'{c[0][0]:g}:{c[0][1]:g}:{c[0][2]:g}-' + 'x'.join(map(str, c[1]))


def _module(grid, kind, reduction, device, loss_weight=LW):
    from basicsr4rs_amd.losses import RegisteredLoss
    return RegisteredLoss(*grid, kind, loss_weight=loss_weight, reduction=reduction).to(device)


def _upstream(B):
    return torch.tensor([0.75, -1.5, 2.0, 0.5][:B], dtype=torch.float32)


def _run(mod, pred, target, up):
    p = pred.detach().clone().requires_grad_(True)
    loss = mod(p, target)
    (loss * up.to(loss.device)).sum().backward() if mod.reduction == 'none' else loss.backward()
    return loss.detach(), p.grad, mod.last_shift.clone()


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
@pytest.mark.parametrize('kind', ['l1', 'mse'])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_registered_loss_vs_fp64(cuda, case, dt, kind, reduction):
    grid, shape = case
    f = R.build_case(grid, shape, kind)
    up = _upstream(shape[0])
    res = R.backward_ref(f, reduction, LW, upstream=up if reduction == 'none' else None)
    mod = _module(grid, kind, reduction, cuda)
    assert tuple(mod._shiftconv2d.taps.shape) == (f.S, f.K)
    pred, target = f.pred.to(cuda, dt), f.target.float().to(cuda)
    assert torch.equal(pred.double().cpu(), f.pred) and torch.equal(target.double().cpu(), f.target)
    what = f'{_case_id(case)} {kind} {reduction}'
    loss, grad, shift = _run(mod, pred, target, up)
    assert loss.dtype == torch.float32 and grad.dtype == dt and shift.dtype == torch.int32
    assert shift.tolist() == f.picks.tolist(), what
    _check(loss, res.loss, res.b_loss, f'{what} loss')
    _check(grad, res.grad, res.b_grad, f'{what} grad')
    table = mod._shifted_loss(pred, target)
    assert not table.requires_grad
    _check(table, f.table, f.b_table, f'{what} table')
    # a second call gives the same bits
    loss2, grad2, shift2 = _run(mod, pred, target, up)
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(grad), _bits(grad2)) and torch.equal(shift, shift2)
    assert torch.equal(_bits(table), _bits(mod._shifted_loss(pred, target)))


def test_bf16_target(cuda):
    """pred and target both bf16 (the third instantiation of the kernels)."""
    grid, shape = (-1.0, 1.0, 0.5), (2, 3, 15, 18)
    f = R.build_case(grid, shape, 'mse', torch.bfloat16)
    res = R.backward_ref(f, 'mean', LW)
    mod = _module(grid, 'mse', 'mean', cuda)
    loss, grad, shift = _run(mod, f.pred.to(cuda, torch.bfloat16), f.target.to(cuda, torch.bfloat16), None)
    assert shift.tolist() == f.picks.tolist()
    _check(loss, res.loss, res.b_loss, 'bf16 target loss')
    _check(grad, res.grad, res.b_grad, 'bf16 target grad')


@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_tie_selects_the_first_shift(cuda, kind):
    """pred = 0, target = 1/4: every shifted image is 0, all S^2 losses are bitwise equal and index 0 is chosen; its
    gradient, the transposed filter of rows T[0], T[0], differs from every other shift's by more than the bounds."""
    grid, shape = (-1.0, 1.0, 0.5), (1, 2, 12, 13)
    pred, target = torch.zeros(shape, dtype=torch.float64), torch.full(shape, 0.25, dtype=torch.float64)
    mod = _module(grid, kind, 'mean', cuda)
    f = R.forward_ref(pred, target, mod._shiftconv2d.taps.cpu(), kind)
    assert f.idx.tolist() == [0]
    res = R.backward_ref(f, 'mean', LW)
    loss, grad, shift = _run(mod, pred.float().to(cuda), target.float().to(cuda), None)
    table = mod._shifted_loss(pred.float().to(cuda), target.float().to(cuda))
    assert (_bits(table) == _bits(table)[0, 0]).all()
    assert shift.tolist() == [0]
    _check(loss, res.loss, res.b_loss, f'tie {kind} loss')
    _check(grad, res.grad, res.b_grad, f'tie {kind} grad')
    for s in range(1, f.S * f.S):
        f.idx = torch.tensor([s])
        other = R.backward_ref(f, 'mean', LW)
        assert ((other.grad - res.grad).abs() > other.b_grad + res.b_grad).any(), s


def test_nan_entry_is_selected(cuda):
    grid, shape = (-1.0, 1.0, 0.5), (2, 3, 15, 18)
    f = R.build_case(grid, shape, 'l1')
    res = R.backward_ref(f, 'none', LW, upstream=torch.ones(2))
    mod = _module(grid, 'l1', 'none', cuda)
    pred = f.pred.float().to(cuda)
    pred[0, 1, 7, 9] = float('nan')
    loss, grad, shift = _run(mod, pred, f.target.float().to(cuda), torch.ones(2))
    assert tuple(loss.shape) == (2, ) and bool(torch.isnan(loss[0])) and bool(torch.isfinite(loss[1]))
    assert shift[1].item() == f.picks[1].item()
    assert 0 <= shift[0].item() < f.S * f.S and bool(torch.isnan(mod._shifted_loss(pred, f.target.float().to(cuda))[0, shift[0]]))
    _check(loss[1], res.loss[1], res.b_loss[1], 'NaN batch, image 1 loss')
    _check(grad[1], res.grad[1], res.b_grad[1], 'NaN batch, image 1 grad')


def test_refusals(cuda):
    mod = _module((-1.0, 1.0, 0.5), 'l1', 'mean', cuda)  # K = 9, r = 4
    ok = torch.zeros(1, 1, 9, 9, device=cuda)
    assert torch.isfinite(mod(ok, ok))
    for shape in ((1, 1, 8, 12), (1, 1, 12, 8)):
        x = torch.zeros(shape, device=cuda)
        with pytest.raises(ValueError, match='2r \\+ 1'):
            mod(x, x)
    with pytest.raises(ValueError):
        mod(ok, torch.zeros(1, 1, 9, 10, device=cuda))
    mod.reduction = 'median'
    with pytest.raises(NotImplementedError):
        mod(ok, ok)


@pytest.mark.parametrize('kind', ['l1', 'mse'])
@pytest.mark.parametrize('why', ['target_grad', 'S10'])
def test_fallback_matches_the_restatement(cuda, monkeypatch, kind, why):
    """A target that requires grad, and a grid of 10 shift values, take the torch composition: both gradients against
    the restatement, under its bounds with the summation depth of a naive fp32 evaluation (n).  d pred comes out of
    the library's convolution backward, whose algorithm is not ours to know: a transformed-domain or blocked
    algorithm commits errors relative to the largest magnitude it handles, not to each element's own, so its bound
    is norm-wise -- the element's bound plus 2 K u max over the image of sum |T||T||g|.  (First run on the device, with
    the element-wise bound alone: max|err| 6.5e-10 against 3.4e-9 at that element, but 1.7e4 times the bound at
    elements whose own magnitude sum is ~1e-14.)"""
    from basicsr4rs_amd.losses import align_loss
    grid = (-1.0, 1.0, 0.5) if why == 'target_grad' else (-2.25, 2.25, 0.5)
    shape = (2, 3, 15, 18)
    f = R.build_case(grid, shape, kind)
    assert f.S == (5 if why == 'target_grad' else 10)
    fn = R.forward_ref(f.pred, f.target, f.taps, kind, depth=f.n)
    res = R.backward_ref(fn, 'mean', LW)

    def no_kernel(*a, **k):
        raise AssertionError('the fused path was taken')

    monkeypatch.setattr(align_loss._RegisteredFused, 'apply', no_kernel)
    mod = _module(grid, kind, 'mean', cuda)
    p = f.pred.float().to(cuda).requires_grad_(True)
    t = f.target.float().to(cuda).requires_grad_(why == 'target_grad')
    loss = mod(p, t)
    loss.backward()
    assert mod.last_shift.tolist() == f.picks.tolist()
    _check(loss.detach(), res.loss, res.b_loss, f'fallback {why} {kind} loss')
    normwise = 2 * f.K * U * res.gmag.amax((1, 2, 3), keepdim=True)
    _check(p.grad, res.grad, res.b_grad + normwise, f'fallback {why} {kind} d pred')
    if why == 'target_grad':
        _check(t.grad, -res.g, res.b_g + 2 * U * res.g.abs(), f'fallback {why} {kind} d target')
    else:
        _check(mod._shifted_loss(p.detach(), t), fn.table, fn.b_table, f'fallback {why} {kind} table')


def test_double_backward_goes_through_torch_ops(cuda):
    grid, shape = (0.0, 1.5, 0.5), (1, 2, 13, 16)
    f = R.build_case(grid, shape, 'mse')
    mod = _module(grid, 'mse', 'mean', cuda, loss_weight=1.0)
    p = f.pred.float().to(cuda).requires_grad_(True)
    (g1, ) = torch.autograd.grad(mod(p, f.target.float().to(cuda)), p, create_graph=True)
    (g1 * g1).sum().backward()
    p64 = f.pred.clone().requires_grad_(True)
    (r1, ) = torch.autograd.grad(R.torch_ref(p64, f.target, f.taps, 'mse', 'mean'), p64, create_graph=True)
    (r1 * r1).sum().backward()
    err = (p.grad.double().cpu() - p64.grad).abs().max().item()
    print(f'double backward: max|err| {err:.3e} (ref max {p64.grad.abs().max().item():.3e})')
    assert err <= 1e-4 * p64.grad.abs().max().item()


def test_shiftconv_stack_on_the_device(cuda):
    from basicsr4rs_amd.losses import ShiftConv2d
    conv = ShiftConv2d(0.0, 1.5, 0.5).to(cuda)
    x = torch.rand(2, 2, 12, 15, generator=torch.Generator().manual_seed(3))
    ref = R.shift_all(x.double(), conv.taps.double().cpu())
    mag = R.shift_all(x.double().abs(), conv.taps.double().abs().cpu())
    got = conv(x.to(cuda))
    assert tuple(got.shape) == (2, 16, 2, 12, 15)
    # the library's convolution: a norm-wise bound, as in test_fallback_matches_the_restatement
    _check(got.contiguous(), ref, 2 * 11 * U * (mag + mag.amax((3, 4), keepdim=True)) + U * ref.abs(), 'ShiftConv2d stack')


@pytest.mark.parametrize('strategy', ['gt', 'lq'])
def test_encoder_loss_against_the_reference(cuda, strategy):
    """Against the reference's recorded loss and z.grad, under the bounds of tests/test_pixel_losses_gpu.py for the
    fused MSE (1e-5 relative) and, for 'lq', the resize bound of tests/_degrade_ref.py carried through the square."""
    from basicsr4rs_amd.losses import EncoderLoss
    z = np.load(GOLDEN)
    zs, gt, lq = (torch.from_numpy(z[k]) for k in ('enc.z', 'enc.gt', 'enc.lq'))
    p = zs.to(cuda).requires_grad_(True)
    loss = EncoderLoss(strategy=strategy)(p, gt.to(cuda), lq.to(cuda))
    loss.backward()
    want = torch.tensor(float(z[f'enc.{strategy}.loss']), dtype=torch.float64)
    extra_loss, extra_grad = 0.0, 0.0
    if strategy == 'lq':
        up, b_up = DR.resize(lq, (15, 21), (5 / 15, 7 / 21), 'bilinear')
        extra_loss = (2 * (zs.double() - up).abs() * b_up).mean().item()
        extra_grad = 2 * b_up / zs.numel()
        ref64 = ((zs.double() - up)**2).mean()
        assert abs(ref64.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item())) + extra_loss
    err = abs(loss.item() - want.item())
    print(f'EncoderLoss {strategy}: loss {loss.item():.8f} reference {want.item():.8f} err {err:.3e}')
    assert err <= 1e-5 * max(1.0, abs(want.item())) + extra_loss
    if strategy == 'lq':
        gref = torch.from_numpy(z['enc.lq.grad']).double()
        gerr = (p.grad.double().cpu() - gref).abs()
        bound = 1e-5 * gref.abs() + 1e-6 * gref.abs().max() + extra_grad
        print(f'EncoderLoss lq: grad max|err| {gerr.max().item():.3e}')
        assert (gerr <= bound).all()
