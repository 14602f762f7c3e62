"""The LDL kernels of csrc/ldl.hip through losses/loss_util.py against the float64 restatement of tests/_ldl_ref.py:
the artifact map w, the fused L1 term and d out, under the bounds derived there (conventions: the top of
tests/test_eltwise_gpu.py; u = 2^-24, a bf16 result within one bf16 ulp + the fp32 bound of the rounded reference).

Inputs are on a lattice (multiples of 1/64, or 1/128 for the second image of a batch) that is exact in fp32 and
bf16, so r, e and the mask decision r >= e -- ties included -- are exact in every type; the two images of a batch
are scaled differently so that P_0 != P_1.

Worst error / bound ratios observed on an MI355X: DESIGN.md §6j."""
import functools

import numpy as np
import pytest
import torch

from tests._fp64 import _check, _ids
from tests._ldl_ref import artifact_map64, lattice, ldl_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
# every window mostly reflection; 6 bands, odd W; odd W, rows not 16-byte aligned; wide and low; several 64 x 16
# tiles with remainders in both directions
SHAPES = [(2, 3, 4, 4), (1, 6, 8, 5), (2, 3, 19, 37), (2, 3, 7, 64), (2, 3, 70, 135)]
LARGE = {(2, 3, 19, 37), (2, 3, 70, 135)}
LOSS_WEIGHT = 0.7


def _f32(x):
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    out, gt, ema = lattice(shape, sum(shape), scale=[1.0, 0.5][:shape[0]])
    r, e = (gt - out).abs().sum(1), (gt - ema).abs().sum(1)
    masked = (r < e).double().mean().item()
    assert 0.25 <= masked <= 0.75, f'degenerate draw: masked share {masked}'
    if shape in LARGE:
        assert (r == e).any(), 'no tie r == e in the draw'
        assert (out == gt).any(), 'no zero of out - gt in the draw'
    return out, gt, ema


@functools.lru_cache(maxsize=None)
def _upstream(shape):
    N, _, H, W = shape
    return torch.randn(N, 1, H, W, generator=torch.Generator().manual_seed(11), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _ref(shape, reduction=None):
    out, gt, ema = _inputs(shape)
    if reduction is None:
        return ldl_ref(out, gt, ema, dW=_upstream(shape))
    k = _f32(LOSS_WEIGHT) / (out.numel() if reduction == 'mean' else 1)
    return ldl_ref(out, gt, ema, k=k)


def _device(shape, dtype, cuda):
    """out in ``dtype``, gt fp32, ema in ``dtype``: the lattice values are exact in both."""
    out, gt, ema = _inputs(shape)
    return out.to(dtype).to(cuda).requires_grad_(True), gt.float().to(cuda), ema.to(dtype).to(cuda)


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_artifact_map_and_general_backward(cuda, shape, dtype):
    """get_refined_artifact_map on the kernels: w, and d out under a random upstream map dW (the T_n reduce runs)."""
    from basicsr4rs_amd.losses.loss_util import get_refined_artifact_map
    out, gt, ema = _device(shape, dtype, cuda)
    ref = _ref(shape)
    if shape[0] > 1:
        assert ref.P[0] != ref.P[1]
    w = get_refined_artifact_map(gt, out, ema, 7)
    assert type(w.grad_fn).__name__ == '_ArtifactMapBackward' and w.dtype == torch.float32
    assert tuple(w.shape) == (shape[0], 1, shape[2], shape[3])
    _check(w.detach(), ref.w.unsqueeze(1), ref.b_w.unsqueeze(1), f'ldl w {shape}')
    assert (w.detach().cpu()[:, 0][ref.m == 0] == 0).all(), 'a masked pixel has a weight'
    w.backward(_upstream(shape).to(cuda))
    assert out.grad.dtype == dtype
    _check(out.grad, ref.dout, ref.b_dout, f'ldl general d out {shape}')


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_fused_l1_term(cuda, shape, dtype, reduction):
    from basicsr4rs_amd.losses.loss_util import ldl_l1_term
    out, gt, ema = _device(shape, dtype, cuda)
    ref = _ref(shape, reduction)
    loss = ldl_l1_term(out, gt, ema, LOSS_WEIGHT, reduction)
    # the fused node, not the map followed by a pixel loss, and not the torch composition
    assert type(loss.grad_fn).__name__ == '_LdlL1FusedBackward' and loss.dtype == torch.float32 and loss.dim() == 0
    _check(loss.detach().reshape(1), ref.loss.reshape(1), ref.b_loss.reshape(1), f'ldl l1 loss {shape} {reduction}')
    loss.backward()
    assert out.grad.dtype == dtype
    _check(out.grad, ref.dout, ref.b_dout, f'ldl l1 d out {shape} {reduction}')
    assert (out.grad.cpu()[_inputs(shape)[0] == _inputs(shape)[1]] == 0).all(), 'sign(0) = 0'


def test_operand_dtypes_give_the_same_bits(cuda):
    """gt and ema in fp32 or in out's dtype: the lattice is exact in both, so nothing may change."""
    from basicsr4rs_amd.losses.loss_util import get_refined_artifact_map, ldl_l1_term
    shape = (2, 3, 19, 37)
    o64, g64, e64 = _inputs(shape)
    got = []
    for od, gd, ed in ((torch.float32, ) * 3, (torch.bfloat16, torch.float32, torch.float32),
                       (torch.bfloat16, torch.bfloat16, torch.float32), (torch.bfloat16, ) * 3):
        out, gt, ema = o64.to(od).to(cuda).requires_grad_(True), g64.to(gd).to(cuda), e64.to(ed).to(cuda)
        loss = ldl_l1_term(out, gt, ema, LOSS_WEIGHT, 'mean')
        loss.backward()
        got.append((get_refined_artifact_map(gt, out, ema, 7).detach(), loss.detach(), out.grad))
    for w, loss, grad in got[1:]:
        assert torch.equal(w, got[0][0]) and torch.equal(loss, got[0][1])
        assert torch.equal(grad, got[1][2])  # the three bf16 outputs
    assert torch.equal(got[1][2], got[0][2].bfloat16()), 'the bf16 gradient is the fp32 one rounded once'


def test_two_runs_same_bits(cuda):
    from basicsr4rs_amd.losses.loss_util import get_refined_artifact_map, ldl_l1_term
    shape = (2, 3, 70, 135)
    runs = []
    for _ in range(2):
        out, gt, ema = _device(shape, torch.float32, cuda)
        loss = ldl_l1_term(out, gt, ema, LOSS_WEIGHT, 'mean')
        loss.backward()
        g1, out.grad = out.grad, None
        w = get_refined_artifact_map(gt, out, ema, 7)
        w.backward(_upstream(shape).to(cuda))
        runs.append((loss.detach(), g1, w.detach(), out.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_upstream_scalar_on_the_device(cuda):
    """The backward launch multiplies by the upstream scalar before its one rounding: a factor 2 is exact."""
    from basicsr4rs_amd.losses.loss_util import ldl_l1_term
    shape = (2, 3, 19, 37)
    grads = []
    for f in (1.0, 2.0):
        out, gt, ema = _device(shape, torch.bfloat16, cuda)
        (ldl_l1_term(out, gt, ema, LOSS_WEIGHT, 'sum') * f).backward()
        grads.append(out.grad.float())
    assert torch.equal(grads[1], grads[0] * 2.0) and grads[0].abs().max() > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_constant_residual(cuda, dtype):
    """out = gt + 1/8 everywhere: V_n == 0, so P_n = 0 with a zero derivative -- loss 0 and a finite, all-zero
    gradient, where the reference formula gives NaN."""
    from basicsr4rs_amd.losses.loss_util import get_refined_artifact_map, ldl_l1_term
    gt64 = _inputs((2, 3, 19, 37))[1]
    gt = gt64.float().to(cuda)
    out = (gt64 + 0.125).to(dtype).to(cuda).requires_grad_(True)
    ema = out.detach().clone()  # r == e: nothing is masked
    loss = ldl_l1_term(out, gt, ema, 1.0, 'mean')
    loss.backward()
    assert loss.item() == 0 and torch.isfinite(out.grad).all() and (out.grad == 0).all()
    out.grad = None
    w = get_refined_artifact_map(gt, out, ema, 7)
    w.sum().backward()
    assert (w == 0).all() and torch.isfinite(out.grad).all() and (out.grad == 0).all()


def test_other_window_takes_the_torch_composition(cuda):
    """ksize 5 is outside the kernels: the torch composition of the same formula, here in float64 on the device
    against the restatement, forward and backward; the bound is _ldl_ref's operation-count bound with the float64
    unit in place of u."""
    from basicsr4rs_amd.losses.loss_util import get_refined_artifact_map
    shape = (2, 3, 19, 37)
    o64, g64, e64 = _inputs(shape)
    dW = _upstream(shape).double()
    ref = ldl_ref(o64, g64, e64, ksize=5, dW=dW)
    assert torch.equal(ref.w.unsqueeze(1), artifact_map64(o64, g64, e64, ksize=5))
    out = o64.to(cuda).requires_grad_(True)
    w = get_refined_artifact_map(g64.to(cuda), out, e64.to(cuda), 5)
    assert 'ArtifactMap' not in type(w.grad_fn).__name__ and w.dtype == torch.float64
    w.backward(dW.to(cuda))
    unit = 2.0**-53 / 2.0**-24
    err_w = (w.detach().cpu()[:, 0] - ref.w).abs()
    err_g = (out.grad.cpu() - ref.dout).abs()
    print(f'ksize 5: w err/bound {(err_w / (unit * ref.b_w).clamp(min=1e-300)).max().item():.3f}, '
          f'd out err/bound {(err_g / (unit * ref.b_dout).clamp(min=1e-300)).max().item():.3f}')
    assert (err_w <= unit * ref.b_w).all() and (err_g <= unit * ref.b_dout).all()
