"""Helpers of the float64-reference kernel tests (test_eltwise_gpu.py, test_layernorm_gpu.py,
test_swin_fused_fp64_gpu.py): the comparison of a device result with a float64 value under a derived fp32
bound (conventions at the top of test_eltwise_gpu.py), and the float64 restatements of LayerNorm forward and
backward, the erf-form GELU pair, a linear and shifted-window attention, each with the magnitude sums a
rounding bound multiplies (checked on the host by test_layernorm_ref_host.py and test_swin_ref_host.py)."""
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
    r.xabsmean = x.abs().mean(-1)
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


SQRT1_2, INV_SQRT_2PI = 0.5**0.5, (2.0 * np.pi)**-0.5


def gelu_ref(v):
    """Exact (erf-form) GELU and its derivative in float64: Phi(v) = (1 + erf(v / sqrt 2)) / 2, phi(v) the
    normal density; returns (v Phi(v), Phi(v) + v phi(v), phi(v))."""
    v = v.double()
    Phi = 0.5 * (1.0 + torch.erf(v * SQRT1_2))
    phi = INV_SQRT_2PI * torch.exp(-0.5 * v * v)
    return v * Phi, Phi + v * phi, phi


def linear_ref(x, w, b=None):
    """y = x w^T + b over the last axis of x in float64 (w [out, in]), with mag = sum_k |w x| + |b| per
    output element (the magnitude a k-term fp32 accumulation bound multiplies)."""
    x, w = x.double(), w.double()
    y, mag = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        y, mag = y + b.double(), mag + b.double().abs()
    return y, mag


def _to_windows(t, ws):
    """[N, H, W, ...] -> [N * nWy * nWx, ws * ws, ...]: windows in (image, window row, window column) order,
    tokens row-major inside a window."""
    N, H, W = t.shape[:3]
    rest = t.shape[3:]
    t = t.reshape(N, H // ws, ws, W // ws, ws, *rest)
    perm = (0, 1, 3, 2, 4) + tuple(range(5, 5 + len(rest)))
    return t.permute(*perm).reshape(N * (H // ws) * (W // ws), ws * ws, *rest)


def _from_windows(t, ws, N, H, W):
    rest = t.shape[2:]
    t = t.reshape(N, H // ws, W // ws, ws, ws, *rest)
    perm = (0, 1, 3, 2, 4) + tuple(range(5, 5 + len(rest)))
    return t.permute(*perm).reshape(N, H, W, *rest)


def window_attention_ref(qkv, nH, shift, scale, table, ws=8, hdp=32):
    """Shifted-window attention of a padded-head qkv map [N, H, W, 3 nH hdp] (channel = (which, head, dim);
    dims past the real head dim are whatever the map holds, zeros for a padded head) in float64:
    roll by -shift, partition into ws x ws windows, s = scale q.k + table[relative position] - 100 between
    tokens of different shift regions (rows / columns [0, L-ws), [L-ws, L-shift), [L-shift, L) of the rolled
    map; no mask at shift 0), P = softmax_k s, out = P v, rolled back.

    Returns: s, P [windows, nH, q, k]; lse [windows, nH, q] (natural log); masked [windows, q, k] (bool);
    absqk = sum_d |q_d k_d| per score; bias [nH, q, k]; v, absv [windows, nH, k, hdp]; out, pabsv
    (= sum_k P_k |v_k|) as maps [N, H, W, nH hdp] at the un-shifted pixels; and to_map(t [windows, nH, q,
    hdp]) which puts any per-(query, dim) tensor on that map."""
    qkv, table = qkv.double(), table.double()
    N, H, W, ld = qkv.shape
    assert ld == 3 * nH * hdp and H % ws == 0 and W % ws == 0 and 0 <= shift < ws
    n = ws * ws
    t = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift else qkv
    tw = _to_windows(t.reshape(N, H, W, 3, nH, hdp), ws).permute(2, 0, 3, 1, 4)  # [3, windows, nH, n, hdp]
    q, k, v = tw[0], tw[1], tw[2]
    r = SimpleNamespace()
    qk = q @ k.transpose(-1, -2)
    r.absqk = q.abs() @ k.abs().transpose(-1, -2)
    iy, ix = torch.arange(n) // ws, torch.arange(n) % ws
    idx = (iy[:, None] - iy[None, :] + ws - 1) * (2 * ws - 1) + (ix[:, None] - ix[None, :] + ws - 1)
    r.bias = table[idx.reshape(-1)].reshape(n, n, nH).permute(2, 0, 1)
    nwin = (H // ws) * (W // ws)
    if shift:
        reg = lambda L: (torch.arange(L) >= L - ws).long() + (torch.arange(L) >= L - shift).long()  # noqa: E731
        label = _to_windows((reg(H)[:, None] * 3 + reg(W)[None, :]).reshape(1, H, W), ws)  # [nwin, n]
        r.masked = (label[:, :, None] != label[:, None, :]).repeat(N, 1, 1)
    else:
        r.masked = torch.zeros(N * nwin, n, n, dtype=torch.bool)
    r.s = qk * scale + r.bias[None] + torch.where(r.masked, -100.0, 0.0)[:, None]
    r.lse = torch.logsumexp(r.s, -1)
    r.P = torch.exp(r.s - r.lse[..., None])
    r.v, r.absv = v, v.abs()

    def to_map(o):  # [windows, nH, n, hdp] -> [N, H, W, nH hdp], rolled back
        m = _from_windows(o.permute(0, 2, 1, 3).reshape(-1, n, nH * hdp), ws, N, H, W)
        return torch.roll(m, shifts=(shift, shift), dims=(1, 2)) if shift else m

    r.to_map = to_map
    r.out, r.pabsv = to_map(r.P @ v), to_map(r.P @ r.absv)
    return r
