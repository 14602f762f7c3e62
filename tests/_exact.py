"""Helpers of the exact-arithmetic conv tests (test_exact_grid_host.py, test_conv_exact_gpu.py).

Every operand is a small integer times a power of two and every slope / scale is a power of two, so each product,
each partial sum in any order, each split-K slab, each atomic add and each epilogue step of a conv kernel is
exactly representable in fp32: the device result must equal the float64 result bit for bit (fp32 outputs
directly, bf16 outputs after one round-to-nearest-even).  Here: the operand grids, the float64 restatement of
sr_conv3x3_fwd / sr_conv3x3_wgrad calls (gathers, channel slices, the epilogue in epilogue_tile's order), the
check that a case really is exact (assert_exactness), the bitwise comparison with a mismatch-pattern report
(assert_bits), and the single defects the host test applies to the reference (drop_term, ...)."""
import zlib
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from ._fp64 import _rne_bf16

QUANTA_LIMIT = 2.0**20
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
SLOPE, ALPHA, BETA2 = 0.25, 0.5, -0.5
SENTINEL = 7.0  # channels around a slice (input: a misread term is large; output: must stay bit-unchanged)


def pad8(c):
    return (c + 7) // 8 * 8


def gen_for(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def grid(shape, lo=-3, hi=3, scale=1.0, gen=None):
    """Float64 tensor of integers in [lo, hi] times ``scale`` (a power of two)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).double() * scale


def choice(shape, values, gen=None):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=gen)]


def impulse(shape, pos):
    """Zeros [N, H, W, C] with a single 1 at pos = (n, y, x, c)."""
    t = torch.zeros(tuple(shape), dtype=torch.float64)
    t[tuple(pos)] = 1.0
    return t


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def store(t64, dtype):
    """A float64 grid tensor in the storage dtype (exact: the grids are bf16-exact)."""
    out = t64.to(dtype)
    assert torch.equal(out.double(), t64), 'operand not exact in its storage dtype'
    return out


def to_stored(ref64, dtype):
    """What a correct kernel stores for the float64 result: fp32 as is, bf16 after one RNE rounding."""
    if dtype == torch.float32:
        return ref64.float()
    return _rne_bf16(ref64).to(torch.bfloat16)


def rhu_bf16(x64):
    """Round-half-up (away from zero on ties) to 8 significant bits: the wrong bf16 rounding."""
    m, e = np.frexp(x64.numpy())
    r = np.sign(m) * np.floor(np.abs(m) * 256.0 + 0.5) / 256.0
    return torch.from_numpy(np.ldexp(r, e))


# ------------------------------------------------------------------------------------------ gathers


def gather_input(x, in_up=0, in_ps=0):
    """Logical NCHW conv input of a stored NHWC map: nearest-up by in_up, or (in_ps = r) the HR map
    [N, H r, W r, C'] read as the LR map of r r C' channels, LR channel (si r + sj) C' + c = HR pixel
    (y r + si, x r + sj) channel c."""
    if in_ps > 1:
        r = in_ps
        N, Hr, Wr, cp = x.shape
        H, W = Hr // r, Wr // r
        return x.reshape(N, H, r, W, r, cp).permute(0, 2, 4, 5, 1, 3).reshape(N, r * r * cp, H, W).contiguous()
    xl = nchw(x)
    if in_up > 1:
        xl = F.interpolate(xl, scale_factor=in_up, mode='nearest')
    return xl


def conv_acc(xl, w, transpose=False, stride=1):
    """The accumulation alone: (sum of terms, sum of |terms|), NCHW float64; pad k // 2 (k 4, stride 2: 1)."""
    pad = 1 if w.shape[-1] == 4 else w.shape[-1] // 2
    f = F.conv_transpose2d if transpose else F.conv2d
    return f(xl, w, stride=stride, padding=pad), f(xl.abs(), w.abs(), stride=stride, padding=pad)


def impulse_acc(shape, pos, w):
    """The accumulation of an impulse input, written down directly: the weight image, placed and clipped."""
    N, H, W, _ = shape
    n, y0, x0, c = pos
    k = w.shape[-1]
    acc = torch.zeros(N, w.shape[0], H, W, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            y, x = y0 - ky + k // 2, x0 - kx + k // 2
            if 0 <= y < H and 0 <= x < W:
                acc[n, :, y, x] = w[:, c, ky, kx]
    return acc


def epilogue(acc, e):
    """The fp32 epilogue on the accumulation [N, Cout, H, W], in epilogue_tile's order: bias, act, gate mode 0,
    alpha * row_scale, res, res2 (both on columns < rcols), gate mode 2 on [gcol0, gcol1), affine; then the
    pixel shuffle of the store.  ``e``: a namespace of float64 NCHW operands / scalars (absent = off).
    Returns (y NCHW, [(stage name, tensor)])."""
    g = lambda k, d=None: getattr(e, k, d)  # noqa: E731
    v, stages = acc, [('acc', acc)]

    def step(name, t):
        stages.append((name, t))
        return t

    if g('bias') is not None:
        v = step('bias', v + e.bias.view(1, -1, 1, 1))
    if g('act', 0) == ACT_RELU:
        v = step('relu', v.clamp(min=0))
    elif g('act', 0) == ACT_LRELU:
        v = step('lrelu', torch.where(v > 0, v, v * e.slope))
    gate, mode = g('gate'), g('gate_mode', 0)
    assert mode in (0, 2), 'gate_mode 1 (stored GELU derivative) is not exact on any grid'
    if gate is not None and mode == 0:
        v = step('gate', v * torch.where(gate > 0, 1.0, e.gate_slope))
    al = torch.full((acc.shape[0],), float(g('alpha', 1.0)), dtype=torch.float64)
    if g('row_scale') is not None:
        al = step('alpha*row_scale', al * e.row_scale)
    v = step('alpha', v * al.view(-1, 1, 1, 1))
    rc = g('rcols') or acc.shape[1]
    if g('res') is not None:
        v = step('res', torch.cat([v[:, :rc] + g('beta', 1.0) * e.res[:, :rc], v[:, rc:]], 1))
    if g('res2') is not None:
        v = step('res2', torch.cat([v[:, :rc] + g('beta2', 1.0) * e.res2[:, :rc], v[:, rc:]], 1))
    if gate is not None and mode == 2:
        m = torch.ones_like(v)
        m[:, e.gcol0:e.gcol1] = torch.where(gate[:, e.gcol0:e.gcol1] > 0, 1.0, e.gate_slope)
        v = step('gate2', v * m)
    if g('aff_scale') is not None:
        v = step('aff_scale', v * e.aff_scale.view(1, -1, 1, 1))
    if g('aff_shift') is not None:
        v = step('aff_shift', v + e.aff_shift.view(1, -1, 1, 1))
    if g('out_ps', 0) > 1:
        v = F.pixel_shuffle(v, e.out_ps)
    return v, stages


def wgrad_ref(xl, dyl, k, scale=1.0, init=None, stride=1):
    """dW [Cout, Cin, k, k], db [Cout] of logical NCHW x and dy in float64, times ``scale``, plus ``init``
    (the accumulate path); and the sums of |terms|.  Returns a namespace dw, db, mag_w, mag_b, stages."""
    pad = 1 if k == 4 else k // 2
    shape = (dyl.shape[1], xl.shape[1], k, k)
    r = SimpleNamespace()
    raw_w = torch.nn.grad.conv2d_weight(xl, shape, dyl, stride=stride, padding=pad)
    raw_b = dyl.sum((0, 2, 3))
    r.mag_w = torch.nn.grad.conv2d_weight(xl.abs(), shape, dyl.abs(), stride=stride, padding=pad)
    r.mag_b = dyl.abs().sum((0, 2, 3))
    r.dw, r.db = raw_w * scale, raw_b * scale
    r.stages = [('dw sum', raw_w), ('db sum', raw_b), ('dw scaled', r.dw), ('db scaled', r.db)]
    if init is not None:
        r.dw, r.db = r.dw + init[0], r.db + init[1]
        r.stages += [('dw accumulated', r.dw), ('db accumulated', r.db)]
    return r


def pixel_unshuffle_nchw(dy, r):
    """HR NHWC dy [N, H r, W r, C'] -> the conv's NCHW output gradient [N, C' r r, H, W] (channel c r r + s)."""
    return F.pixel_unshuffle(nchw(dy), r) if r > 1 else nchw(dy)


# ------------------------------------------------------------------------------------------ checks


def quantum(t):
    """Largest power of two q with t / q all integers (t exact multiples of some 2^-j, j <= 40)."""
    q = 1.0
    for _ in range(41):
        if bool((t / q == torch.round(t / q)).all()):
            return q
        q *= 0.5
    raise AssertionError('values are not multiples of a power of two >= 2^-40')


def assert_exactness(stages, abs_sum):
    """A test-construction check, run before the device is touched: every stage [(name, float64 tensor)] is
    exactly an fp32 value, and every accumulation's sum of |terms| [(name, tensor, quantum of one term)] stays
    below 2^20 quanta, so no partial sum in any order can round."""
    for name, t in stages:
        assert torch.equal(t.float().double(), t), f'case is not fp32-exact at stage {name!r}'
    for name, mag, q in abs_sum:
        top = float(mag.max()) / q if mag.numel() else 0.0
        assert top < QUANTA_LIMIT, f'case is not exact: sum |terms| of {name!r} reaches {top:.0f} quanta (>= 2^20)'


def _shared(idx, size=None):
    v = idx if size is None else idx // size
    return bool((v == v[0]).all())


def assert_bits(got, ref64, what, axes='nyxc'):
    """got (fp32 or bf16, any device) must equal the float64 reference bit for bit: fp32 directly, bf16 after
    one RNE rounding of the reference.  A mismatch reports how many elements differ, the first index, what the
    differing elements share (a row, a column, a 64-pixel strip seam, an 8 / 32 / 64-channel chunk, an image)
    and got - ref in quanta of the reference."""
    got64 = got.detach().double().cpu()
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    target = ref64 if got.dtype == torch.float32 else _rne_bf16(ref64)
    bad = ~(got64 == target)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    idx = bad.nonzero()
    names = list(axes) if len(axes) == ref64.dim() else [f'd{i}' for i in range(ref64.dim())]
    first = ', '.join(f'{a}={int(i)}' for a, i in zip(names, idx[0]))
    share = []
    for d, a in enumerate(names):
        col = idx[:, d]
        if ref64.shape[d] > 1 and _shared(col):
            share.append({'n': 'one image', 'y': 'one row', 'x': 'one column', 'c': 'one channel'}.get(a, f'one {a}') +
                         f' ({a}={int(col[0])})')
        elif a == 'x' and ref64.shape[d] > 64 and bool(((col % 64 == 0) | (col % 64 == 63)).all()):
            share.append('64-pixel strip seam columns')
        elif a.startswith('c'):
            for size in (8, 32, 64):
                if ref64.shape[d] > size and _shared(col, size):
                    share.append(f'one {size}-channel chunk (chunk {int(col[0]) // size})')
                    break
    q = quantum(ref64)
    diff = (got64 - target)[bad]
    nan = int(torch.isnan(diff).sum())
    dq = diff[~torch.isnan(diff)] / q
    rng = f'{float(dq.min()):g} .. {float(dq.max()):g}' if dq.numel() else 'n/a'
    raise AssertionError(
        f'{what} [{"f32" if got.dtype == torch.float32 else "bf16"}]: {nbad} of {bad.numel()} elements differ from the '
        f'float64 result; first at ({first}); shared: {"; ".join(share) or "nothing"}; got - ref in quanta of '
        f'{q:g}: {rng}' + (f'; {nan} NaN (never written)' if nan else ''))


# ------------------------------------------------------------------------------------------ defects
# Single defects of a conv kernel, applied to the float64 accumulation (NCHW) of logical input xl and weight w.


def _term(xl, w, tap, c, n=None, y=None, x=None):
    """Contribution of (tap, channel c) to the outputs, zero outside the selected image / row / column."""
    ky, kx = tap
    k = w.shape[-1]
    xp = F.pad(xl[:, c], (k // 2,) * 4)
    N, _, H, W = xl.shape
    t = w[:, c, ky, kx].view(1, -1, 1, 1) * xp[:, ky:ky + H, kx:kx + W].unsqueeze(1)
    m = torch.zeros(N, 1, H, W, dtype=torch.float64)
    m[slice(None) if n is None else n, :, slice(None) if y is None else y, slice(None) if x is None else x] = 1.0
    return t * m


def drop_term(acc, xl, w, tap, c, **where):
    """One (tap, channel) product missing at the selected pixels (one column: x=col)."""
    return acc - _term(xl, w, tap, c, **where)


def double_term(acc, xl, w, tap, c, **where):
    """One K element counted twice."""
    return acc + _term(xl, w, tap, c, **where)


def swap_channels(xl, w, c, n, y, x):
    """Channels c and c + 1 (one 8-channel group) swapped when pixel (n, y, x) is read: the accumulation."""
    x2 = xl.clone()
    x2[n, c, y, x], x2[n, c + 1, y, x] = xl[n, c + 1, y, x], xl[n, c, y, x]
    return conv_acc(x2, w)[0]


def shift_halo_row(acc, xl, w, n, y):
    """Output row y of image n reads its upper halo row (input row y - 1) one pixel to the right."""
    x2 = xl.clone()
    x2[n, :, y - 1, 1:] = xl[n, :, y - 1, :-1]
    x2[n, :, y - 1, 0] = 0
    out = acc.clone()
    out[n, :, y] = conv_acc(x2[n:n + 1], w)[0][0, :, y]
    return out


def omit_pixels(dyl, n, y=None, m0=None, m1=None):
    """dy with one pixel row of image n zeroed (that row's products and bias terms omitted), or with the
    flattened pixel range [m0, m1) zeroed (one split's slab omitted)."""
    out = dyl.clone()
    if y is not None:
        out[n, :, y] = 0
    else:
        N, C, H, W = out.shape
        flat = out.permute(1, 0, 2, 3).reshape(C, -1)
        flat[:, m0:m1] = 0
        out = flat.reshape(C, N, H, W).permute(1, 0, 2, 3).contiguous()
    return out
