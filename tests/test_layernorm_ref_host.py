"""tests/_fp64.layernorm_ref (the float64 reference of test_layernorm_gpu.py: closed-form backward) against
torch.autograd of F.layer_norm in float64, to 1e-12 of each tensor's largest magnitude."""
import pytest
import torch
import torch.nn.functional as F

from tests._fp64 import layernorm_ref

REL = 1e-12


def _close(a, b, what):
    err, mag = (a - b).abs().max().item(), b.abs().max().item()
    print(f'{what}: max|err| {err:.3e} of max|ref| {mag:.3e}')
    assert a.shape == b.shape and err <= REL * mag, (what, err, mag)


@pytest.mark.parametrize('n,hw,c', [(1, 1, 5), (3, 7, 60), (2, 13, 180), (4, 3, 512)])
def test_layernorm_ref_matches_autograd(n, hw, c):
    g = torch.Generator().manual_seed(11 + c)
    m = n * hw
    x = torch.randn(m, c, generator=g, dtype=torch.float64) * 2 + 0.5
    if m > 4:  # the rows test_layernorm_gpu.py stresses: constant, all zero, mean 100 with deviation 1
        x[1], x[2] = 3.25, 0.0
        x[3] = 100.0 + torch.randn(c, generator=g, dtype=torch.float64)
    gamma = torch.randn(c, generator=g, dtype=torch.float64) * 0.5 + 1
    beta = torch.randn(c, generator=g, dtype=torch.float64) * 0.1
    dy = torch.randn(m, c, generator=g, dtype=torch.float64)
    res = torch.randn(m, c, generator=g, dtype=torch.float64)
    scale = torch.tensor([0.0, 1 / 0.9, 0.37, 1.0][:n], dtype=torch.float64)
    r = layernorm_ref(x, gamma, beta, dy, res, scale, hw)
    xa, ga, ba = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = F.layer_norm(xa, (c, ), ga, ba, 1e-5)
    y.backward(dy)
    _close(r.y, y.detach(), 'y')
    _close(r.mean, x.mean(-1), 'mean')
    _close(r.rstd, (x.var(-1, unbiased=False) + 1e-5).rsqrt(), 'rstd')
    _close(r.dx0, xa.grad, 'dx')
    _close(r.dx, xa.grad + res, 'dx + res')
    _close(r.dxs, (xa.grad + res) * scale.repeat_interleave(hw)[:, None], 'dx row_scale')
    _close(r.dgamma, ga.grad, 'dgamma')
    _close(r.dbeta, ba.grad, 'dbeta')
    assert (r.dxs[:hw] == 0).all()
    # handed the statistics it computed itself, the backward is the same
    r2 = layernorm_ref(x, gamma, beta, dy, None, None, hw, stats=(r.mean, r.rstd))
    assert torch.equal(r2.dx0, r.dx0) and torch.equal(r2.dx, r.dx0) and torch.equal(r2.dgamma, r.dgamma)


def test_layernorm_ref_magnitudes_dominate():
    """The magnitude sums bound the values they belong to (triangle inequality), so a bound k u mag is a
    bound relative to at least the result."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(21, 60, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma, beta = torch.randn(60, generator=g, dtype=torch.float64), torch.randn(60, generator=g, dtype=torch.float64)
    dy = torch.randn(21, 60, generator=g, dtype=torch.float64)
    r = layernorm_ref(x, gamma, beta, dy)
    tiny = 1e-12
    assert (r.y.abs() <= r.ymag * (1 + tiny)).all() and (r.mean.abs() <= r.xmax).all()
    assert (r.dx0.abs() <= r.dxmag * (1 + tiny)).all()
    assert (r.dgamma.abs() <= r.dgmag * (1 + tiny)).all() and (r.dbeta.abs() <= r.dbmag * (1 + tiny)).all()
