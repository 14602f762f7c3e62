"""The float64 restatements of tests/_edvr_ref.py, checked on the host: the hand-written backward formulas of the
temporal attention and the sigmoid modulation against autograd, the pure-torch modulated deformable conv against
the float64 oracle (oracle/ops.py: forward and every gradient it provides), and the stock EDVR tree's state_dict
names and shapes against tests/golden/edvr_state_keys.json (written down from basicsr/archs/edvr_arch.py and
arch_util.py:237-263 by reading them: the reference's package does not import here)."""
import json
import os

import numpy as np
import pytest
import torch

from . import _edvr_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edvr_state_keys.json')


def _rel(a, b):
    return (a - b).abs().max().item() / max(1e-300, b.abs().max().item())


@pytest.mark.parametrize('B,T,C', [(2, 3, 16), (1, 5, 8)])
def test_tsa_corr_backward_formulas_match_autograd(B, T, C):
    g = torch.Generator().manual_seed(B * 100 + T)
    H, W = 3, 4
    emb = torch.randn(B * T, H, W, C, generator=g, dtype=torch.float64, requires_grad=True)
    ref = torch.randn(B, H, W, C, generator=g, dtype=torch.float64, requires_grad=True)
    ali = torch.randn(B * T, H, W, C, generator=g, dtype=torch.float64, requires_grad=True)
    d_out = torch.randn(B, H, W, T * C, generator=g, dtype=torch.float64)
    out, prob = R.tsa_corr(emb, ref, ali)
    assert out.shape == (B, H, W, T * C) and prob.shape == (B, T, H, W)
    # the (t, c) channel order of the reference's (b, t * c, h, w) view
    want = (ali.reshape(B, T, H, W, C) * prob[..., None]).permute(0, 1, 4, 2, 3).reshape(B, T * C, H, W)
    assert torch.equal(out.permute(0, 3, 1, 2), want)
    out.backward(d_out)
    d_ali, d_emb, d_ref = R.tsa_corr_bwd(d_out, emb.detach(), ref.detach(), ali.detach(), prob.detach())
    for name, got, auto in (('d_aligned', d_ali, ali.grad), ('d_emb', d_emb, emb.grad), ('d_emb_ref', d_ref, ref.grad)):
        err = _rel(got, auto)
        print(f'tsa_corr {name}: rel err {err:.3e}')
        assert err < 1e-13, name


def test_tsa_modulate_backward_formulas_match_autograd():
    g = torch.Generator().manual_seed(3)
    feat, attn, add = (torch.randn(2, 3, 4, 8, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3))
    dy = torch.randn(2, 3, 4, 8, generator=g, dtype=torch.float64)
    y = R.tsa_modulate(feat, attn * 4, add)
    assert torch.allclose(y, feat * torch.sigmoid(attn * 4) * 2 + add, rtol=1e-14, atol=1e-14)
    R.tsa_modulate(feat, attn, add).backward(dy)
    d_feat, d_attn, d_add = R.tsa_modulate_bwd(dy, feat.detach(), attn.detach())
    for name, got, auto in (('d_feat', d_feat, feat.grad), ('d_attn', d_attn, attn.grad), ('d_attn_add', d_add, add.grad)):
        assert _rel(got, auto) < 1e-13, name


def test_torch_dcn_matches_the_oracle():
    """One small case with samples inside, across the border and outside: forward and all five gradients."""
    from oracle import ops as O
    g = torch.Generator().manual_seed(11)
    N, C, H, W, Co, dg = 2, 8, 5, 6, 6, 2
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    offset = (torch.randn(N, dg * 18, H, W, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    mask = torch.rand(N, dg * 9, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    weight = torch.randn(Co, C, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(N, Co, H, W, generator=g, dtype=torch.float64)
    y = R.dcn(x, offset, mask, weight, bias, dg)
    y.backward(dy)
    args = [t.detach().numpy() for t in (x, offset, mask, weight, bias)]
    ref = O.dcn_forward(*args, 1, 1, 1, 1, dg, coords='f64')
    assert np.abs(y.detach().numpy() - ref).max() < 1e-12 * np.abs(ref).max()
    grads = O.dcn_backward(*args, 1, 1, 1, 1, dg, dy.numpy(), coords='f64')
    for name, t, r in zip(('x', 'offset', 'mask', 'weight', 'bias'), (x, offset, mask, weight, bias), grads):
        err = np.abs(t.grad.numpy() - r).max() / np.abs(r).max()
        print(f'dcn grad {name}: rel err {err:.3e}')
        assert err < 1e-12, name


def test_conv3s2_and_pool_restatements():
    """Shapes for odd sizes, the window rule of the stride-2 conv written out for one output, and the pool pair."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, 7, 9, generator=g, dtype=torch.float64)
    w = torch.randn(6, 4, 3, 3, generator=g, dtype=torch.float64)
    y = R.conv3s2(x, w)
    assert y.shape == (1, 6, 4, 5)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    oh, ow = 3, 4  # the last window: half outside
    assert torch.allclose(y[0, :, oh, ow], (xp[0, :, 2 * oh:2 * oh + 3, 2 * ow:2 * ow + 3] * w).sum((1, 2, 3)), atol=1e-13)
    p = R.pool3s2(x)
    assert p.shape == (1, 8, 4, 5)
    assert torch.allclose(p[0, 4:, 0, 0], x[0, :, :2, :2].sum((1, 2)) / 9, atol=1e-14)  # count_include_pad
    assert torch.equal(p[0, :4, 0, 0], x[0, :, :2, :2].amax((1, 2)))


@pytest.mark.parametrize('name', sorted(R.GOLDEN_CONFIGS))
def test_stock_tree_state_dict_matches_golden(name):
    golden = json.load(open(GOLDEN))[name]
    shapes = R.state_shapes(R.StockEDVR(**R.GOLDEN_CONFIGS[name]))
    assert list(shapes) == list(golden), 'state_dict names or their order differ'
    assert shapes == golden


def test_stock_tree_runs_and_emulation_differs():
    cfg = dict(num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1, num_reconstruct_block=1)
    net = R.init_edvr(R.StockEDVR(**cfg).double(), seed=1)
    x = torch.rand(1, 3, 3, 8, 8, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    y = net(x)
    assert y.shape == (1, 3, 32, 32)
    emu = R.stock_like(net.state_dict(), cfg, torch.float64, emulate=True)(x)
    rel = (emu - y).norm() / y.norm()
    assert 0 < rel < 0.05
    with pytest.raises(AssertionError):
        net(torch.rand(1, 3, 3, 10, 8, dtype=torch.float64))
