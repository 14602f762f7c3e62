"""The float64 stage references of test_swin_fused_fp64_gpu.py (tests/_fp64.py) checked on the host:
window_attention_ref on padded heads against oracle.nets.window_attention_core on the unpadded map, gelu_ref
against torch.autograd of the erf-form GELU in float64, linear_ref against F.linear; to 1e-12 of each
tensor's largest magnitude.  The magnitude sums dominate the values they belong to."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nets as O
from tests._fp64 import gelu_ref, linear_ref, window_attention_ref

REL = 1e-12
HDP = 32


def _close(a, b, what):
    err, mag = (a - b).abs().max().item(), b.abs().max().item()
    print(f'{what}: max|err| {err:.3e} of max|ref| {mag:.3e}')
    assert a.shape == b.shape and err <= REL * mag, (what, err, mag)


def _pad_heads(t, lead, nH, hd):
    """[..., lead nH hd] -> [..., lead nH HDP], zeros in the pad dims."""
    t = t.reshape(*t.shape[:-1], lead, nH, hd)
    return F.pad(t, (0, HDP - hd)).reshape(*t.shape[:-3], lead * nH * HDP)


@pytest.mark.parametrize('shift', [0, 3, 4, 7])
@pytest.mark.parametrize('hd', [10, 25, 32])
def test_window_attention_ref_matches_oracle(shift, hd):
    """ws 8, two images of 2 x 3 windows (H = 16 != W = 24), 3 heads padded from hd to 32."""
    N, H, W, nH = 2, 16, 24, 3
    g = torch.Generator().manual_seed(100 * shift + hd)
    qkv = torch.randn(N, H, W, 3 * nH * hd, generator=g, dtype=torch.float64)
    table = torch.randn(225, nH, generator=g, dtype=torch.float64)
    scale = hd**-0.5
    want = O.window_attention_core(qkv, nH, 8, shift, scale, table)
    r = window_attention_ref(_pad_heads(qkv, 3, nH, hd), nH, shift, scale, table)
    out = r.out.reshape(N, H, W, nH, HDP)
    _close(out[..., :hd].reshape(N, H, W, nH * hd), want, 'out')
    assert (out[..., hd:] == 0).all() and (r.pabsv.reshape(N, H, W, nH, HDP)[..., hd:] == 0).all()
    nwin = N * (H // 8) * (W // 8)
    assert r.P.shape == r.s.shape == r.absqk.shape == (nwin, nH, 64, 64) and r.lse.shape == (nwin, nH, 64)
    _close(r.P.sum(-1), torch.ones(nwin, nH, 64, dtype=torch.float64), 'sum_k P')
    _close(r.lse, torch.log(torch.exp(r.s - r.s.amax(-1, keepdim=True)).sum(-1)) + r.s.amax(-1), 'lse')
    # the mask is the oracle's (swinir_arch.py calculate_mask), the same for every image
    if shift:
        m = O.swin_mask(H, W, 8, shift) != 0
        assert torch.equal(r.masked, m.repeat(N, 1, 1)) and r.masked.any() and not r.masked.all()
        assert r.P[r.masked[:, None].expand_as(r.P)].max().item() < 1e-30
    else:
        assert not r.masked.any()
    tiny = 1 + 1e-12
    assert (r.out.abs() <= r.pabsv * tiny).all()
    assert ((r.s - r.bias[None] - torch.where(r.masked, -100.0, 0.0)[:, None]).abs() <= scale * r.absqk * tiny + 1e-12).all()
    # to_map is the inverse of the roll + partition: the queries' own v rows come back as the v map
    vmap = _pad_heads(qkv, 3, nH, hd).reshape(N, H, W, 3, nH * HDP)[..., 2, :]
    assert torch.equal(r.to_map(r.v), vmap)


def test_gelu_ref_matches_autograd():
    v = torch.linspace(-9, 9, 3601, dtype=torch.float64).requires_grad_()
    y = F.gelu(v)  # approximate='none': the erf form
    y.sum().backward()
    h, dh, phi = gelu_ref(v.detach())
    _close(h, y.detach(), 'gelu')
    _close(dh, v.grad, "gelu'")
    _close(phi, torch.distributions.Normal(0.0, 1.0).log_prob(v.detach()).exp(), 'phi')
    assert dh.abs().max().item() <= 1.13 and dh.min().item() >= -0.13  # the Lipschitz constant the bounds use


def test_linear_ref_matches_f_linear():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 5, 24, generator=g, dtype=torch.float64)
    w, b = torch.randn(40, 24, generator=g, dtype=torch.float64), torch.randn(40, generator=g, dtype=torch.float64)
    y, mag = linear_ref(x.to(torch.bfloat16), w.float(), b.float())
    _close(y, F.linear(x.to(torch.bfloat16).double(), w.float().double(), b.float().double()), 'linear')
    assert (y.abs() <= mag * (1 + 1e-12)).all()
    y0, mag0 = linear_ref(x, w)
    _close(y0, F.linear(x, w), 'linear, no bias')
    _close(mag0, F.linear(x.abs(), w.abs()), 'linear magnitude')
