"""Helpers of the float64-reference kernel tests (test_eltwise_gpu.py, test_layernorm_gpu.py): the
comparison of a device result with a float64 value under a derived fp32 bound (conventions at the top of
test_eltwise_gpu.py), and the float64 restatement of LayerNorm forward and backward."""
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0**-24


def _ids(dt):
    return 'f32' if dt == torch.float32 else 'bf16'


def _rne_bf16(x64):
    """One round-to-nearest-even of float64 values to 8 significant bits (bf16; values in normal range)."""
    m, e = np.frexp(x64.numpy())
    return torch.from_numpy(np.ldexp(np.rint(m * 256.0) / 256.0, e))


def _bf16_ulp(x64):
    _, e = np.frexp(x64.abs().clamp(min=2.0**-120).numpy())
    return torch.from_numpy(np.ldexp(np.ones_like(e, dtype=np.float64), e - 8))


def _check(got, ref, fbound, what):
    """got (device, fp32 or bf16) against the float64 ref; fbound: the derived fp32 bound (tensor or 0)."""
    got64 = got.detach().double().cpu()
    assert got64.shape == ref.shape, (what, got64.shape, ref.shape)
    fb = fbound if torch.is_tensor(fbound) else torch.full_like(ref, float(fbound))
    if got.dtype == torch.float32:
        target, bound = (ref.float().double(), fb) if not fb.any() else (ref, fb)
    else:
        target = _rne_bf16(ref)
        bound = torch.where(fb > 0, _bf16_ulp(torch.maximum(target.abs(), got64.abs())) + fb, fb)
    err = (got64 - target).abs()
    assert torch.isfinite(got64).all(), what
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    rounded = got.dtype != torch.float32 or not fb.any()
    print(f'{what} [{_ids(got.dtype)}]: max|err| {err.max().item():.3e}, bound there '
          f'{bound.reshape(-1)[err.argmax()].item():.3e}, max err/bound {ratio.max().item():.3f}' +
          (f', {(err > 0).double().mean().item():.2%} of elements differ from the rounded reference' if rounded else ''))
    assert (err <= bound).all(), (what, err.max().item())


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _assert_outside_unchanged(buf, before, coff, C, what):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[coff:coff + C] = False
    assert torch.equal(_bits(buf)[..., keep], _bits(before)[..., keep]), f'{what}: wrote outside the channel slice'


def layernorm_ref(x, gamma, beta, dy=None, res=None, row_scale=None, hw=1, eps=1e-5, stats=None):
    """LayerNorm over the last axis of x [M, C] and its backward, in float64 (every argument is upcast).

    Forward: mean, rstd = (var + eps)^-1/2 (biased variance), xhat = (x - mean) rstd, y = xhat gamma + beta.
    Backward (with dy): g = dy gamma, dx0 = rstd (g - mean_c(g) - xhat mean_c(g xhat)), dx = dx0 + res,
    dxs = dx row_scale[row // hw], dgamma = sum_rows dy xhat, dbeta = sum_rows dy.  ``stats`` = (mean, rstd)
    replaces the statistics the backward uses (what a backward kernel is handed).

    Magnitude sums for rounding bounds: xmax = max_c |x| per row; ymag = |gamma| rstd (|x| + |mean|) + |beta|;
    dxmag = rstd (|g| + mean_c|g| + |xhat| mean_c|g xhat|); dgmag = sum_rows |dy xhat|; dbmag = sum_rows |dy|."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    r = SimpleNamespace()
    r.mean = x.mean(-1)
    r.rstd = ((x - r.mean[:, None]).pow(2).mean(-1) + eps).rsqrt()
    r.y = (x - r.mean[:, None]) * r.rstd[:, None] * gamma + beta
    r.xmax = x.abs().amax(-1)
    r.ymag = gamma.abs() * r.rstd[:, None] * (x.abs() + r.mean.abs()[:, None]) + beta.abs()
    if dy is None:
        return r
    mean, rstd = (r.mean, r.rstd) if stats is None else (stats[0].double(), stats[1].double())
    dy = dy.double()
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    gx = g * xhat
    r.dx0 = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * gx.mean(-1, keepdim=True))
    r.dxmag = rstd[:, None] * (g.abs() + g.abs().mean(-1, keepdim=True) + xhat.abs() * gx.abs().mean(-1, keepdim=True))
    r.dx = r.dx0 + res.double() if res is not None else r.dx0
    if row_scale is not None:
        r.scale = row_scale.double().repeat_interleave(hw)[:, None]
        r.dxs = r.dx * r.scale
    dyx = dy * xhat
    r.dgamma, r.dbeta = dyx.sum(0), dy.sum(0)
    r.dgmag, r.dbmag = dyx.abs().sum(0), dy.abs().sum(0)
    return r
