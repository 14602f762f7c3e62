"""Float64 restatement of the LDL artifact map and of the ldl_opt L1 term (csrc/ldl.hip, losses/loss_util.py;
DESIGN.md §6j), written for this repository from the formulas, with the magnitude sums the rounding bounds of
tests/test_ldl_ops_gpu.py multiply (checked on the host by tests/test_ldl_ref_host.py).

``artifact_map64`` is the forward in differentiable float64 torch ops, by explicit k x k windows over the
reflect-padded residual.  ``ldl_ref`` is the forward again plus the closed-form backward:

  a = m dW (zero outside the image), A = box(a), B = box(a mu) at the padded coordinates [-p, H+p) x [-p, W+p),
  G~ = 2/(k^2-1) (r~ A - B), G = G~ folded onto the pixel each padded position reflects,
  T_n = sum a L, g_r = P_n G + T_n (1/5) V_n^(-4/5) 2 (r - mean_n) / (M - 1)   (the last term 0 when V_n == 0),
  d out[c] = sign(out - gt) (g_r + direct), direct = k w for the L1 term (dW = k r) and 0 for the bare map.

Bounds (u = 2^-24, first order; the kernel's operation counts are stated where they enter):
  L   two separable 7-tap passes: an element of sum x meets <= 12 additions, one of sum x^2 <= 13 roundings (7
      fused multiply-adds, 6 additions), mu = S1 / 49 two more, S2 - S1 mu one, / 48 two:
      |dL| <= 16u (S2 + 98 mu^2) / 48.
  V   per block the mean (<= 4 values per thread, a 6-level shuffle tree per wave, 4 waves, the division: 12
      roundings), then sum (x - mean)^2 likewise (14 with the subtraction), merged in double:
      |dV| <= u (27 V + 12 sum x^2 / (M - 1)), for any tiling.
  P   V^(1/5) in double, rounded once: |dP| <= P (0.2 dV / V + 2u).
  S   sum m L r per block (4 fused multiply-adds, 6 + 3 additions: 13 roundings), double afterwards:
      |dS| <= 13u S + sum m r dL.
  G   a and a mu (17u relative), two 7-tap passes of multiplicity-weighted fused multiply-adds (14), r A - B
      fused, 2/48: |dG| <= 34u Gmag, Gmag = fold(2/48 (r~ box|a| + box|a mu|)).
The residuals r and e are the kernel's own fp32 sums over the channels in channel order (``residual='fp32'``:
IEEE subtraction, absolute value and addition, the same bits on the host; exact on the lattice inputs of the
tests), so the mask, a discontinuous decision, is the kernel's."""
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0**-24


def lattice(shape, seed, scale=None):
    """gt = randint(-32, 33) / 64, out = gt + randint(-16, 17) / 64, ema likewise: exact in bf16, r and e exact
    sums, ties r == e and zeros of out - gt present.  ``scale``: per-image factors (powers of two) of both
    differences, so that P differs between the images of a batch."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(-32, 33, shape, generator=g).double() / 64
    do = torch.randint(-16, 17, shape, generator=g).double() / 64
    de = torch.randint(-16, 17, shape, generator=g).double() / 64
    if scale is not None:
        s = torch.tensor(scale, dtype=torch.float64).view(-1, 1, 1, 1)
        do, de = do * s, de * s
    return gt + do, gt, gt + de


def _reflect_index(n, pad):
    i = np.abs(np.arange(-pad, n + pad))
    return torch.from_numpy(np.where(i >= n, 2 * n - 2 - i, i))


def _windows(x, k):
    """x [N, H, W] -> [N, k*k, H, W]: the k x k window of the reflect-padded x around every pixel."""
    _, H, W = x.shape
    pad = (k - 1) // 2
    xp = x[:, _reflect_index(H, pad)][:, :, _reflect_index(W, pad)]
    return torch.stack([xp[:, i:i + H, j:j + W] for i in range(k) for j in range(k)], 1)


def _box(a, k):
    """a [N, H, W], zero outside -> its k x k box sum at the padded coordinates, [N, H + 2p, W + 2p]."""
    _, H, W = a.shape
    p = (k - 1) // 2
    z = torch.zeros(a.shape[0], H + 4 * p, W + 4 * p, dtype=a.dtype)
    z[:, 2 * p:2 * p + H, 2 * p:2 * p + W] = a
    return sum(z[:, i:i + H + 2 * p, j:j + W + 2 * p] for i in range(k) for j in range(k))


def _fold(gp, H, W, k):
    """A map at the padded coordinates folded onto the image: every padded position adds to the pixel it reflects."""
    pad = (k - 1) // 2
    rows = torch.zeros(gp.shape[0], H, gp.shape[2], dtype=gp.dtype).index_add_(1, _reflect_index(H, pad), gp)
    return torch.zeros(gp.shape[0], H, W, dtype=gp.dtype).index_add_(2, _reflect_index(W, pad), rows)


def fold_multiplicity(n, pad=3):
    """How many padded positions of an axis of length n reflect to each pixel."""
    return torch.bincount(_reflect_index(n, pad), minlength=n)


def artifact_map64(out, gt, ema, ksize=7, v0_rule=True):
    """w [N, 1, H, W] in differentiable float64 torch ops.  ``v0_rule``: P = 0 with a zero derivative where V == 0."""
    out, gt, ema = out.double(), gt.double(), ema.double()
    r, e = (gt - out).abs().sum(1), (gt - ema).abs().sum(1)
    win = _windows(r, ksize)
    L = (win - win.mean(1, keepdim=True)).pow(2).sum(1) / (ksize * ksize - 1)
    M = r.shape[1] * r.shape[2]
    V = (r - r.mean((1, 2), keepdim=True)).pow(2).sum((1, 2)) / (M - 1)
    if v0_rule:
        P = torch.where(V > 0, V, torch.ones_like(V)).pow(0.2) * (V > 0)
    else:
        P = V.pow(0.2)
    return (P.view(-1, 1, 1) * L * (r >= e)).unsqueeze(1)


def _residual(a, b, mode):
    if mode == 'fp64':
        return (a.double() - b.double()).abs().sum(1)
    a, b = a.float(), b.float()  # the inputs are fp32 or bf16 values: exact
    s = torch.zeros(a.shape[0], *a.shape[2:], dtype=torch.float32)
    for c in range(a.shape[1]):
        s = s + (a[:, c] - b[:, c]).abs()
    return s.double()


def ldl_ref(out, gt, ema, ksize=7, dW=None, k=None, residual='fp32'):
    """Forward and closed-form backward in float64 with the bounds of the module docstring.

    ``k`` (a float, the L1 term's loss_weight / (N C H W) or loss_weight): the fused term, dW = k r, direct = k w,
    ``loss`` = k sum_n P_n S_n.  ``dW`` [N, 1, H, W]: the bare map's backward for that upstream map.  Neither: the
    forward only.  Returns a namespace of [N, H, W] maps (r, e, m, mu, L, w, G, g), per-image vectors (mean, V, P, S,
    T), ``dout`` [N, C, H, W] and the bounds b_L, b_V, b_P, b_w, b_S, b_loss, b_g, b_dout."""
    res = SimpleNamespace()
    N, C, H, W = out.shape
    M, kk = H * W, ksize * ksize
    r, e = _residual(gt, out, residual), _residual(gt, ema, residual)
    res.r, res.e, res.m = r, e, (r >= e).double()
    win = _windows(r, ksize)
    res.mu = win.mean(1)
    res.L = (win - res.mu[:, None]).pow(2).sum(1) / (kk - 1)
    res.mean = r.mean((1, 2))
    res.V = (r - res.mean.view(-1, 1, 1)).pow(2).sum((1, 2)) / (M - 1)
    res.P = torch.where(res.V > 0, res.V, torch.ones_like(res.V)).pow(0.2) * (res.V > 0)
    lm = res.L * res.m
    Pv = res.P.view(-1, 1, 1)
    res.w = Pv * lm
    res.S = (lm * r).sum((1, 2))
    # forward bounds
    res.b_L = 16 * U * (win.pow(2).sum(1) + 2 * kk * res.mu.pow(2)) / (kk - 1)
    res.b_V = U * (27 * res.V + 12 * r.pow(2).sum((1, 2)) / (M - 1))
    relV = torch.where(res.V > 0, res.b_V / res.V.clamp(min=1e-300), torch.zeros_like(res.V))
    res.b_P = res.P * (0.2 * relV + 2 * U)
    res.b_w = res.m * (Pv * res.b_L + res.L * res.b_P.view(-1, 1, 1)) + U * res.w
    res.b_S = 13 * U * res.S + (res.m * r * res.b_L).sum((1, 2))
    if k is not None:
        res.loss = k * (res.P * res.S).sum()
        res.b_loss = abs(k) * (res.P * res.b_S + res.S * res.b_P).sum() + 2 * U * res.loss.abs()
        dWm, direct = k * r, k * res.w
    elif dW is not None:
        dWm, direct = dW.double().reshape(N, H, W), torch.zeros_like(r)
    else:
        return res
    # closed-form backward
    a = res.m * dWm
    pad = (ksize - 1) // 2
    rp = r[:, _reflect_index(H, pad)][:, :, _reflect_index(W, pad)]
    c2 = 2.0 / (kk - 1)
    res.G = _fold(c2 * (rp * _box(a, ksize) - _box(a * res.mu, ksize)), H, W, ksize)
    Gmag = _fold(c2 * (rp * _box(a.abs(), ksize) + _box((a * res.mu).abs(), ksize)), H, W, ksize)
    res.T = (a * res.L).sum((1, 2))
    live = res.V > 0
    Q = torch.where(live, 0.2 * torch.where(live, res.V, torch.ones_like(res.V)).pow(-0.8) * 2.0 / (M - 1),
                    torch.zeros_like(res.V))
    dev = r - res.mean.view(-1, 1, 1)
    term1, term2 = Pv * res.G, (res.T * Q).view(-1, 1, 1) * dev
    res.g = term1 + term2 + direct
    res.dout = torch.sign(out.double() - gt.double()) * res.g[:, None]
    # backward bounds.  T: the fused term has it from S (k S, two roundings); the general one sums dW m L per block
    # (a thread's strided fused multiply-adds, <= max(4, M / 16384), and the 6 + 3 additions of the block sum), in double
    # afterwards
    if k is not None:
        b_T = abs(k) * res.b_S + 2 * U * res.T.abs()
    else:
        nloc = max(4, -(-M // 16384))
        b_T = (nloc + 9) * U * (a * res.L).abs().sum((1, 2)) + (a.abs() * res.b_L).sum((1, 2))
    b_G = 34 * U * Gmag
    # T Q (r - mean): Q = (1/5) V^(-4/5) 2 / (M - 1) in double, rounded once; the mean as the block means (13u); two
    # products
    b_Q = Q * (0.8 * relV + 2 * U)
    b_dev = 13 * U * res.mean.view(-1, 1, 1) + U * dev.abs()
    b_term2 = ((Q * b_T + res.T.abs() * b_Q).view(-1, 1, 1) * dev.abs() + (res.T * Q).abs().view(-1, 1, 1) * b_dev
               + 3 * U * term2.abs())
    b_direct = abs(k) * (Pv * res.m * res.b_L + lm * res.b_P.view(-1, 1, 1)) + 3 * U * direct.abs() if k is not None else 0
    res.b_g = (Pv * b_G + res.G.abs() * res.b_P.view(-1, 1, 1) + b_term2 + b_direct
               + 3 * U * (term1.abs() + term2.abs() + direct.abs()))
    res.b_dout = (out.double() != gt.double()) * res.b_g[:, None]
    return res
