"""Float64 restatement of RegisteredLoss (csrc/regloss.hip, losses/align_loss.py), written for this
repository from the formulas as direct padded sums, with the closed-form gradient and the magnitude sums the rounding
bounds of tests/test_registered_loss_gpu.py multiply (checked on the host by tests/test_registered_ref_host.py).

With the tap table T [S, K], r = K // 2, shift s = sy * S + sx, n = C (H - 2r)(W - 2r):
  shifted[b, s, c, h, w] = sum_j sum_i T[sy, j] T[sx, i] pred[b, c, h + j - r, w + i - r]     (zero outside the image)
  table[b, s] = mean over c and the crop [r, H - r) x [r, W - r) of phi(d),  d = shifted - target,  phi = |d| or d^2
  idx[b] = the first minimum of table[b] (a NaN entry before any number),  loss = loss_weight * reduce_b table[b, idx[b]]
  g = k_b phi'(d) / n on the crop of shift idx[b], 0 on the border strips;  phi' = sign(d) (sign(0) = 0) or 2 d;
  k_b = loss_weight / B (mean), loss_weight (sum), loss_weight * upstream[b] (none)
  d pred[b, c, p, q] = sum_j sum_i T[sy*, j] T[sx*, i] g[b, c, p - j + r, q - i + r].

Bounds (u = 2^-24, first order; the kernel's operation counts are stated where they enter):
  v   a shifted value is two passes of K fused multiply-adds: |dv| <= 2 K u M, M = sum_j sum_i |T||T||pred|.
  d   one subtraction: |dd| <= |dv| + u |d|.
  phi |d|: |dd|;  d^2: 2 |d| |dd| + u d^2.
  table  a thread adds 4 values, a 6-level shuffle tree per wave, the 4 waves (``depth`` = 13 roundings), double
      afterwards, the mean rounded to fp32:  (sum dphi + depth u sum phi) / n + 2 u table.
  loss   the selected means summed in double, rounded once: |loss_weight| reduce_b(b_table[b, idx[b]]) + 2 u |loss|.
  g   k_b / n rounded once, for d^2 times the rounded d:  |d|: 2 u |g| (the sign is the kernel's where |d| exceeds its
      bound, which ``build_case`` asserts);  d^2: 2 |k_b / n| |dd| + 3 u |g|.
  d pred  two passes of K fused multiply-adds over g:  sum |T||T| b_g + 2 K u sum |T||T||g|, plus 2 u |d pred| for the
      upstream product.
A naive fp32 evaluation that sums the crop one element after another has depth n instead of 13: ``depth=`` says so.
"""
import functools
from types import SimpleNamespace

import torch

from basicsr4rs_amd.losses.align_loss import shift_taps

U = 2.0**-24
KERNEL_DEPTH = 13


def shift_all(x, T):
    """x [B, C, H, W], T [S, K] (float64) -> [B, S^2, C, H, W]: every shift as a direct zero-padded sum."""
    B, C, H, W = x.shape
    S, K = T.shape
    r = K // 2
    xp = torch.zeros(B, C, H + 2 * r, W + 2 * r, dtype=torch.float64)
    xp[:, :, r:r + H, r:r + W] = x
    ys = torch.zeros(B, S, C, H, W + 2 * r, dtype=torch.float64)
    for j in range(K):
        ys += T[:, j].view(1, S, 1, 1, 1) * xp[:, None, :, j:j + H, :]
    out = torch.zeros(B, S, S, C, H, W, dtype=torch.float64)
    for i in range(K):
        out += T[:, i].view(1, 1, S, 1, 1, 1) * ys[:, :, None, :, :, i:i + W]
    return out.view(B, S * S, C, H, W)


def shift_transposed(g, Ty, Tx):
    """g [C, H, W], Ty / Tx [K] -> sum_j sum_i Ty[j] Tx[i] g[p - j + r, q - i + r], g zero outside."""
    C, H, W = g.shape
    K = Ty.numel()
    r = K // 2
    gp = torch.zeros(C, H + 4 * r, W + 4 * r, dtype=torch.float64)
    gp[:, 2 * r:2 * r + H, 2 * r:2 * r + W] = g
    rows = torch.zeros(C, H, W + 4 * r, dtype=torch.float64)
    for j in range(K):
        rows += Ty[j] * gp[:, 3 * r - j:3 * r - j + H, :]
    out = torch.zeros(C, H, W, dtype=torch.float64)
    for i in range(K):
        out += Tx[i] * rows[:, :, 3 * r - i:3 * r - i + W]
    return out


def first_argmin(table):
    """torch.argmin's rule stated directly: the first NaN if there is one, else the first minimum."""
    idx = []
    for row in table:
        nan = torch.isnan(row).nonzero()
        idx.append(int(nan[0]) if nan.numel() else int((row == row.min()).nonzero()[0]))
    return torch.tensor(idx, dtype=torch.int64)


def forward_ref(pred, target, T, kind, depth=KERNEL_DEPTH):
    """d of every shift on the crop, the table, its bound and the selected indices."""
    pred, target, T = pred.double(), target.double(), T.double()
    B, C, H, W = pred.shape
    S, K = T.shape
    r = K // 2
    f = SimpleNamespace(B=B, C=C, H=H, W=W, S=S, K=K, r=r, kind=kind, T=T, n=C * (H - 2 * r) * (W - 2 * r))
    crop = (Ellipsis, slice(r, H - r), slice(r, W - r))
    f.d = shift_all(pred, T)[crop] - target[:, None][crop]
    f.b_d = 2 * K * U * shift_all(pred.abs(), T.abs())[crop] + U * f.d.abs()
    if kind == 'l1':
        phi, b_phi = f.d.abs(), f.b_d
    else:
        phi, b_phi = f.d * f.d, 2 * f.d.abs() * f.b_d + U * f.d * f.d
    f.table = phi.sum((-3, -2, -1)) / f.n
    f.b_table = (b_phi.sum((-3, -2, -1)) + depth * U * phi.sum((-3, -2, -1))) / f.n + 2 * U * f.table
    f.idx = first_argmin(f.table)
    return f


def backward_ref(f, reduction, loss_weight=1.0, upstream=None):
    """The loss of a reduction and d loss / d pred in closed form, with their bounds.  upstream: [B] for 'none'.
    ``g`` (zero on the border strips) is also -d loss / d target; ``gmag`` = sum |T||T||g|, the magnitude the
    gradient's accumulation bound multiplies."""
    B, r, K, S = f.B, f.r, f.K, f.S
    rows = torch.arange(B)
    picked, b_picked = f.table[rows, f.idx], f.b_table[rows, f.idx]
    res = SimpleNamespace()
    if reduction == 'mean':
        res.loss, res.b_loss = loss_weight * picked.mean(), abs(loss_weight) * b_picked.mean()
    elif reduction == 'sum':
        res.loss, res.b_loss = loss_weight * picked.sum(), abs(loss_weight) * b_picked.sum()
    else:
        res.loss, res.b_loss = loss_weight * picked, abs(loss_weight) * b_picked
    res.b_loss = res.b_loss + 2 * U * res.loss.abs()
    kb = torch.full((B, ), loss_weight / B if reduction == 'mean' else float(loss_weight), dtype=torch.float64)
    if upstream is not None:
        kb = kb * upstream.double()
    res.grad = torch.zeros(B, f.C, f.H, f.W, dtype=torch.float64)
    res.b_grad, res.g, res.b_g, res.gmag = (torch.zeros_like(res.grad) for _ in range(4))
    for b in range(B):
        s = int(f.idx[b])
        sy, sx = divmod(s, S)
        d, b_d, kf = f.d[b, s], f.b_d[b, s], kb[b] / f.n
        if f.kind == 'l1':
            g = kf * torch.sign(d)
            b_g = 2 * U * g.abs()
        else:
            g = 2 * kf * d
            b_g = 2 * kf.abs() * b_d + 3 * U * g.abs()
        full, b_full = torch.zeros(f.C, f.H, f.W, dtype=torch.float64), torch.zeros(f.C, f.H, f.W, dtype=torch.float64)
        full[:, r:f.H - r, r:f.W - r], b_full[:, r:f.H - r, r:f.W - r] = g, b_g
        res.g[b], res.b_g[b] = full, b_full
        Ty, Tx = f.T[sy], f.T[sx]
        res.grad[b] = shift_transposed(full, Ty, Tx)
        res.gmag[b] = shift_transposed(full.abs(), Ty.abs(), Tx.abs())
        res.b_grad[b] = shift_transposed(b_full, Ty.abs(), Tx.abs()) + 2 * K * U * res.gmag[b] + 2 * U * res.grad[b].abs()
    return res


def torch_ref(pred, target, T, kind, reduction, loss_weight=1.0):
    """The same loss by differentiable float64 torch ops (autograd checks the closed form against it)."""
    T = T.double()
    r = T.shape[1] // 2
    d = shift_all_autograd(pred, T)[..., r:-r, r:-r] - target.double()[:, None, :, r:-r, r:-r]
    table = (d.abs() if kind == 'l1' else d * d).mean((-3, -2, -1))
    picked = table[torch.arange(table.shape[0]), first_argmin(table.detach())]
    return loss_weight * (picked.mean() if reduction == 'mean' else picked.sum() if reduction == 'sum' else picked)


def shift_all_autograd(x, T):
    B, C, H, W = x.shape
    S, K = T.shape
    r = K // 2
    xp = torch.nn.functional.pad(x, (r, r, r, r))
    ys = sum(T[:, j].view(1, S, 1, 1, 1) * xp[:, None, :, j:j + H, :] for j in range(K))
    out = sum(T[:, i].view(1, 1, S, 1, 1, 1) * ys[:, :, None, :, :, i:i + W] for i in range(K))
    return out.view(B, S * S, C, H, W)


def _round_to(x64, dtype):
    return x64.to(dtype).double()


@functools.lru_cache(maxsize=None)
def build_case(grid, shape, kind, target_dtype=torch.float32, seed=0):
    """Inputs whose discontinuous choices are safe, and their forward reference (computed once, shared, not to be
    modified).  pred is on the lattice k / 64, |k| <= 64 (exact in bf16); the target of image b is the float64 shift
    ``picks[b]`` (1 and S^2 - 2 alternating: non-symmetric, different per image) of pred plus a noise of +-(1..8) / 256,
    never 0, rounded once to ``target_dtype``; the reference is computed from the rounded values, so fp32 and bf16
    runs see exact inputs.  Asserted: per image, second smallest - smallest >= 16 x the sum of the two entries'
    bounds, and the selected index is the chosen one; for l1, |d| of the selected shift >= 16 x its bound everywhere
    (the sign is safe)."""
    T = shift_taps(*grid)
    S = T.shape[0]
    g = torch.Generator().manual_seed(1000 + seed)
    pred = torch.randint(-64, 65, shape, generator=g).double() / 64
    noise = torch.randint(1, 9, shape, generator=g).double() / 256 * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    picks = torch.tensor([min(1, S * S - 1) if b % 2 == 0 else max(S * S - 2, 0) for b in range(shape[0])])
    stack = shift_all(pred, T.double())
    target = _round_to(stack[torch.arange(shape[0]), picks] + noise, target_dtype)
    f = forward_ref(pred, target, T, kind)
    f.pred, f.target, f.picks, f.taps = pred, target, picks, T
    assert torch.equal(f.idx, picks), (f.idx, picks)
    rows = torch.arange(shape[0])
    if S > 1:  # a single shift has no runner-up
        order = f.table.argsort(1)
        first, second = order[:, 0], order[:, 1]
        gap = f.table[rows, second] - f.table[rows, first]
        f.runner_up = (f.table[rows, second] / f.table[rows, first]).tolist()
        assert (gap >= 16 * (f.b_table[rows, first] + f.b_table[rows, second])).all(), (gap, f.b_table[rows, first])
    if kind == 'l1':
        sel_d, sel_b = f.d[rows, picks], f.b_d[rows, picks]
        assert (sel_d.abs() >= 16 * sel_b).all()
    return f
