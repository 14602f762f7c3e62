"""tests/_ldl_ref.py checked on the host: its closed-form backward against torch autograd of the forward
restatement in float64, the fold multiplicities of the reflect pad, the V == 0 rule and the lattice inputs."""
import pytest
import torch

from tests._ldl_ref import _reflect_index, artifact_map64, fold_multiplicity, lattice, ldl_ref

SHAPES = [(2, 3, 4, 4), (1, 6, 8, 5), (2, 3, 19, 37)]


def _random(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g, dtype=torch.float64)
    return gt + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64), gt, \
        gt + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('kind', ['random', 'lattice'])
def test_closed_form_backward_is_autograd(shape, kind):
    out, gt, ema = _random(shape, 1) if kind == 'random' else lattice(shape, 1, scale=[1.0, 0.5][:shape[0]])
    N, C, H, W = shape
    # the bare map under a random upstream dW
    dW = torch.randn(N, 1, H, W, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    x = out.clone().requires_grad_(True)
    w = artifact_map64(x, gt, ema)
    w.backward(dW)
    ref = ldl_ref(out, gt, ema, dW=dW, residual='fp64')
    assert torch.equal(ref.w.unsqueeze(1), w.detach())
    scale = x.grad.abs().max().item()
    assert (ref.dout - x.grad).abs().max().item() <= 1e-13 * max(scale, 1.0), 'general backward'
    # the L1 term, mean and sum
    for k in (0.7 / out.numel(), 1.3):
        x = out.clone().requires_grad_(True)
        w = artifact_map64(x, gt, ema)
        loss = k * (w * x - w * gt).abs().sum()
        loss.backward()
        ref = ldl_ref(out, gt, ema, k=k, residual='fp64')
        assert abs(ref.loss.item() - loss.item()) <= 1e-13 * abs(loss.item())
        assert (ref.dout - x.grad).abs().max().item() <= 1e-13 * max(x.grad.abs().max().item(), 1e-30), 'L1 backward'


def test_fp32_residual_is_exact_on_the_lattice():
    out, gt, ema = lattice((2, 6, 9, 11), 3, scale=[1.0, 0.25])
    a, b = ldl_ref(out, gt, ema, residual='fp32'), ldl_ref(out, gt, ema, residual='fp64')
    assert torch.equal(a.r, b.r) and torch.equal(a.e, b.e) and torch.equal(a.w, b.w)
    assert out.float().double().equal(out) and out.bfloat16().double().equal(out)


def test_fold_multiplicities():
    """Interior pixels are hit once; pixels 1..3 from an edge twice (the edge pixel itself once); a corner region
    pixel 2 x 2 = 4 times; on a 4-pixel axis the middle pixels are reached from both sides."""
    assert fold_multiplicity(12).tolist() == [1, 2, 2, 2, 1, 1, 1, 1, 2, 2, 2, 1]
    assert fold_multiplicity(4).tolist() == [2, 3, 3, 2]  # pads -3..-1 -> 3, 2, 1; pads 4..6 -> 2, 1, 0
    assert _reflect_index(5, 3).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    my, mx = fold_multiplicity(9), fold_multiplicity(10)
    m2 = my[:, None] * mx[None, :]
    assert m2[0, 0] == 1 and m2[1, 1] == 4 and m2[4, 1] == 2 and m2[4, 5] == 1 and m2.sum() == 15 * 16
    # an upstream map that is 1 at one window centre: the gradient of L there w.r.t. r sums to 0 over the fold
    out, gt, ema = lattice((1, 3, 9, 10), 5)
    dW = torch.zeros(1, 1, 9, 10, dtype=torch.float64)
    dW[0, 0, 0, 0] = 1.0
    ref = ldl_ref(out, gt, out, dW=dW)  # ema = out: r == e everywhere, ties are kept, nothing is masked
    assert ref.m.all()
    assert abs(ref.G.sum().item()) <= 1e-15 and ref.G[0, 4:, :].abs().max() == 0 and ref.G[0, :, 4:].abs().max() == 0


def test_constant_residual_rule():
    """V == 0: the reference formula's backward is NaN; the rule makes P = 0 with a zero derivative."""
    gt = lattice((1, 3, 6, 7), 4)[1]
    out = gt + 0.125
    ema = out.clone()  # r == e: nothing is masked
    x = out.clone().requires_grad_(True)
    artifact_map64(x, gt, ema, v0_rule=False).sum().backward()
    assert not torch.isfinite(x.grad).all()
    x = out.clone().requires_grad_(True)
    w = artifact_map64(x, gt, ema)
    w.sum().backward()
    assert (w == 0).all() and (x.grad == 0).all()
    ref = ldl_ref(out, gt, ema, k=1.0)
    assert ref.loss == 0 and (ref.dout == 0).all() and (ref.b_dout == 0).all()
