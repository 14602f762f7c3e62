"""The HBM-bound helper kernels of csrc/eltwise.hip, csrc/blocks.hip and the tail of csrc/swin.hip, each
against a float64 CPU restatement on the same fp32 / bf16 input bits (bf16 upcasts exactly).

Conventions.  u = 2^-24.  A fp32 result is checked against a bound derived from the kernel's roundings
(stated at each test); a bound of 0 means bitwise.  A bf16 result is compared with one round-to-nearest-
even of the float64 value: the kernel rounds an fp32 intermediate that is within the fp32 bound of the
float64 value, so it may land on the neighbouring bf16 value: |got - rne(ref)| <= 1 bf16 ulp + the fp32
bound (bitwise where the fp32 intermediate is exact).  Where the kernel's fp32 arithmetic is a fixed
sequence of products (act_backward, row_scale) the reference applies the same roundings to the float64
value and the comparison is bitwise in both types.  Every strided write goes into a buffer pre-filled
with a sentinel and every byte outside the addressed slice is asserted unchanged.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests._fp64 import U, _assert_outside_unchanged, _bf16_ulp, _bits, _check, _ids, _rne_bf16  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SWEEP = 8192 * 256  # vectors one sweep of the element-wise kernels' grid covers


def _lib():
    from basicsr4rs_amd import _lib
    return _lib


def _randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _f32(x):
    """A Python float rounded to fp32, as a float64 value (what a kernel receives as a float argument)."""
    return float(np.float32(x))


SENTINEL = -12345.0


# ---------------------------------------------------------------------------------------- nhwc_to_nchw

NHWC_CASES = [(2, 5, 7, 8, 0, 3), (1, 9, 13, 24, 8, 16), (2, 7, 9, 104, 8, 40), (1, 16, 16, 64, 0, 64)]


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('case', NHWC_CASES, ids=str)
def test_nhwc_to_nchw(cuda, case, dtype):
    """Per-pixel kernel (C < 16) and LDS-tiled kernel (C >= 16), a channel slice of a wider map.  Without
    scale / shift the result is the upcast, bitwise; with them y = x scale + shift: two roundings, or one
    when the compiler fuses the multiply-add: |err| <= 2u (|x scale| + |shift|)."""
    from basicsr4rs_amd.ops import conv as C
    N, H, W, ld, coff, c = case
    x = _randn((N, H, W, ld), dtype, 1)
    xs = x.double()[..., coff:coff + c].permute(0, 3, 1, 2).contiguous()
    scale, shift = _randn((c, ), torch.float32, 2) + 2.0, _randn((c, ), torch.float32, 3)
    xd, sc, sh = x.to(cuda), scale.to(cuda), shift.to(cuda)
    got = C.nhwc_to_nchw(xd, c, coff=coff)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), xs.float())
    s64, h64 = scale.double().view(1, c, 1, 1), shift.double().view(1, c, 1, 1)
    _check(C.nhwc_to_nchw(xd, c, scale=sc, shift=sh, coff=coff), xs * s64 + h64,
           2 * U * ((xs * s64).abs() + h64.abs()), f'nhwc_to_nchw {case} scale+shift')
    _check(C.nhwc_to_nchw(xd, c, scale=sc, coff=coff), xs * s64, 2 * U * (xs * s64).abs(), f'nhwc_to_nchw {case} scale')
    _check(C.nhwc_to_nchw(xd, c, shift=sh, coff=coff), xs + h64, 2 * U * (xs.abs() + h64.abs()),
           f'nhwc_to_nchw {case} shift')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('c,cp', [(3, 8), (20, 24)])
def test_layout_autograd_round_trip(cuda, c, cp, dtype):
    """_ToNHWC then _ToNCHW: out = ((x - s0) a0) a1 + s1 with the middle map stored in ``dtype``; the
    gradient is dy a1 a0 through the two transposed kernels.  ub = 2^-8 for the bf16 store, else 0:
    |out - ref| <= (ub + 4u) |y a1| + 2u (|y a1| + |s1|);  |dx - ref| <= (ub + 4u) |dx_ref|."""
    from basicsr4rs_amd.ops import conv as C
    N, H, W = 2, 5, 9
    x = _randn((N, c, H, W), torch.float32, 4)
    a0, s0 = _randn((c, ), torch.float32, 5) + 2.0, _randn((c, ), torch.float32, 6)
    a1, s1 = _randn((c, ), torch.float32, 7) + 2.0, _randn((c, ), torch.float32, 8)
    dy = _randn((N, c, H, W), torch.float32, 9)
    xd = x.to(cuda).requires_grad_(True)
    y = C.to_nhwc(xd, cp, dtype, shift=s0.to(cuda), scale=a0.to(cuda))
    assert y.shape == (N, H, W, cp) and y.dtype == dtype and (y[..., c:] == 0).all()
    out = C.to_nchw(y, c, scale=a1.to(cuda), shift=s1.to(cuda))
    out.backward(dy.to(cuda))
    v = lambda t: t.double().view(1, c, 1, 1)
    ub = 2.0**-8 if dtype == torch.bfloat16 else 0.0
    ya = (x.double() - v(s0)) * v(a0) * v(a1)
    err = (out.detach().double().cpu() - (ya + v(s1))).abs()
    bound = (ub + 4 * U) * ya.abs() + 2 * U * (ya.abs() + v(s1).abs())
    dref = dy.double() * v(a1) * v(a0)
    derr = (xd.grad.double().cpu() - dref).abs()
    print(f'layout round trip c={c} [{_ids(dtype)}]: out err/bound {(err / bound).max().item():.3f}, '
          f'dx err/bound {(derr / ((ub + 4 * U) * dref.abs())).max().item():.3f}')
    assert (err <= bound).all() and (derr <= (ub + 4 * U) * dref.abs()).all()


# ---------------------------------------------------------------------------------------- act_backward

ACT_BIG = SWEEP * 8 + 8 * 256 + 5


def _act_inputs(n, dtype, seed):
    dy, y = _randn((n, ), dtype, seed), _randn((n, ), dtype, seed + 1)
    y[::5] = 0.0
    y[1::5] = -0.0
    return dy, y


def _act_ref(dy, y, neg, alpha, dtype):
    """(alpha dy) rounded to fp32, times (y > 0 ? 1 : neg) rounded to fp32: the products of two fp32
    values are exact in float64, so .float() applies exactly the kernel's two roundings."""
    r = (dy.double() * _f32(alpha)).float().double()
    sel = torch.ones_like(r)
    sel[~(y.double() > 0)] = _f32(neg)
    return (r * sel).float().to(dtype).double()


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('n', [5, 8 * 256 + 3, ACT_BIG])
def test_act_backward(cuda, n, dtype):
    """dz = alpha dy (y > 0 ? 1 : neg) over a flat map: scalar tail only, one block plus tail, and one
    vector past two sweeps of the 8192 x 256 grid.  y holds exact 0 and -0.0: both take the negative
    branch.  Bitwise: one rounding per product (and the bf16 store)."""
    from basicsr4rs_amd.ops import conv as C
    L = _lib()
    dy, y = _act_inputs(n, dtype, 20)
    dyd, yd = dy.to(cuda), y.to(cuda)
    combos = [(L.ACT_LRELU, 0.2, 0.2)] if n == ACT_BIG else [(L.ACT_RELU, 0.0, 1.0), (L.ACT_RELU, 0.0, 0.2),
                                                             (L.ACT_LRELU, 0.2, 1.0), (L.ACT_LRELU, 0.2, 0.2)]
    for act, slope, alpha in combos:
        got = C.act_backward(dyd, yd, act, slope, alpha)
        _check(got, _act_ref(dy, y, slope, alpha, dtype), 0, f'act_backward n={n} act={act} alpha={alpha}')
        zero = (y == 0)
        assert zero.sum() >= 2 * (n // 5)
        if act == L.ACT_RELU:
            assert (got.cpu()[zero] == 0).all()


RRDB_LD, RRDB_P = 64 + 4 * 32, 35
RRDB_SLICES = [(0, 64), (64, 32), (160, 32)]


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_act_backward_nhwc_and_copy_channels(cuda, dtype):
    """Channel slices of an RRDB dense buffer (P pixels x ld channels): LeakyReLU backward in place (as
    _act_bwd_inplace runs it) and out of place into a narrower sentinel-filled buffer, and the slice copy."""
    from basicsr4rs_amd.ops import blocks as B
    L = _lib()
    slices = RRDB_SLICES + ([(4, 4)] if dtype == torch.float32 else [])  # fp32 vectors hold 4 channels
    dy, y = _act_inputs(RRDB_P * RRDB_LD, dtype, 30)
    dy, y = dy.view(RRDB_P, RRDB_LD), y.view(RRDB_P, RRDB_LD)
    yd = y.to(cuda)
    for coff, c in slices:
        ref = _act_ref(dy[:, coff:coff + c], y[:, coff:coff + c], 0.2, 1.0, dtype)
        buf = dy.to(cuda)
        before = buf.clone()
        B._act_bwd_inplace(buf, yd, RRDB_LD, coff, c, RRDB_P, 0.2)
        _check(buf[:, coff:coff + c], ref, 0, f'act_backward_nhwc in place ({coff},{c})')
        _assert_outside_unchanged(buf, before, coff, c, f'act_backward_nhwc in place ({coff},{c})')
        # out of place: ReLU, alpha 0.5, into columns 8 .. 8 + c of a [P, c + 24] buffer
        ldo, ocoff = c + 24, 8
        out = torch.full((RRDB_P, ldo), SENTINEL, dtype=dtype, device=cuda)
        before = out.clone()
        dyd = dy.to(cuda)
        L.check(L.load().sr_act_backward_nhwc(L.dtype_code(dtype), RRDB_P, c, L.ptr(dyd), RRDB_LD, coff, L.ptr(yd),
                                              RRDB_LD, coff, L.ptr(out), ldo, ocoff, L.ACT_RELU, 0.0, 0.5, L.stream()))
        ref = _act_ref(dy[:, coff:coff + c], y[:, coff:coff + c], 0.0, 0.5, dtype)
        _check(out[:, ocoff:ocoff + c], ref, 0, f'act_backward_nhwc out of place ({coff},{c})')
        _assert_outside_unchanged(out, before, ocoff, c, f'act_backward_nhwc out of place ({coff},{c})')
        assert torch.equal(_bits(dyd), _bits(dy.to(cuda)))
        # copy_channels: slice (coff, c) of the source into columns 8 .. 8 + c
        dst = torch.full((RRDB_P, ldo), SENTINEL, dtype=dtype, device=cuda)
        before = dst.clone()
        B._copy_channels(dyd, RRDB_LD, coff, dst, ldo, ocoff, RRDB_P, c)
        assert torch.equal(_bits(dst[:, ocoff:ocoff + c]), _bits(dyd[:, coff:coff + c]))
        _assert_outside_unchanged(dst, before, ocoff, c, f'copy_channels ({coff},{c})')


# --------------------------------------------------------------------------------- nearest_up_backward

@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('s', [2, 3])
@pytest.mark.parametrize('shape', [(2, 3, 5, 8), (1, 4, 4, 24)], ids=str)
def test_nearest_up_backward_plain(cuda, shape, s, accumulate, dtype):
    """Ungated s x s block sum into the first C channels of a wider, prefilled ``out`` (ldo = C + 8).
    fp32: s^2 (+ 1 when accumulating) terms summed in sequence, at most that many roundings of partial
    sums bounded by the sum of magnitudes: |err| <= (s^2 + acc) u (sum |d| + |prev|)."""
    from basicsr4rs_amd.ops import conv as C
    N, H, W, c = shape
    d = _randn((N, H * s, W * s, c), dtype, 40 + s)
    prev = _randn((N, H, W, c + 8), dtype, 50)
    out = prev.to(cuda)
    before = out.clone()
    res = C.nearest_up_backward(d.to(cuda), s, out=out, accumulate=accumulate)
    assert res.data_ptr() == out.data_ptr()
    pool = lambda t: (F.avg_pool2d(t.permute(0, 3, 1, 2), s) * (s * s)).permute(0, 2, 3, 1)
    ref, mag = pool(d.double()), pool(d.double().abs())
    if accumulate:
        ref, mag = ref + prev.double()[..., :c], mag + prev.double()[..., :c].abs()
    _check(out[..., :c], ref, (s * s + int(accumulate)) * U * mag, f'nearest_up_backward {shape} s={s} acc={accumulate}')
    _assert_outside_unchanged(out, before, 0, c, 'nearest_up_backward')


# ------------------------------------------------------------------------------------------- nc_affine

NC_BIG = (1, 513, 515, 32)  # 2,113,560 fp32 vectors: past one sweep of 8192 x 256


@pytest.mark.parametrize('shape,dtype', [(s, d) for s in [(3, 5, 7, 24), (2, 6, 6, 40), (1, 1, 1, 8)] for d in DTYPES] +
                         [(NC_BIG, torch.float32)], ids=lambda v: _ids(v) if isinstance(v, torch.dtype) else str(v))
def test_nc_affine(cuda, shape, dtype):
    """out = beta x + alpha u s[n,c] + gamma t[n,c], the two call forms of RCAB: forward (x, no t) and du
    (no x, t, gamma = 1/HW).  C / PER and HW C / PER are no powers of two (FastDiv).  Roundings: alpha u,
    (.) s, gamma t, beta x (exact for beta = 1) and two sums of partial results bounded by the sum of
    magnitudes: |err| <= 4u (|beta x| + |alpha u s| + |gamma t|)."""
    from basicsr4rs_amd.ops import blocks as B
    N, H, W, c = shape
    if shape == NC_BIG:
        assert N * H * W * c // 4 > SWEEP
    x, u = _randn(shape, dtype, 60), _randn(shape, dtype, 61)
    s, t = torch.rand(N, c, generator=torch.Generator().manual_seed(62)), _randn((N, c), torch.float32, 63)
    xd, ud, sd, td = x.to(cuda), u.to(cuda), s.to(cuda), t.to(cuda)
    s64, t64 = s.double().view(N, 1, 1, c), t.double().view(N, 1, 1, c)
    rs, gamma = _f32(0.1), _f32(1.0 / (H * W))
    fwd = x.double() + rs * u.double() * s64
    _check(B.nc_affine(xd, ud, sd, None, 1.0, 0.1, 0.0), fwd, 4 * U * (x.double().abs() + (rs * u.double() * s64).abs()),
           f'nc_affine forward {shape}')
    du = rs * u.double() * s64 + gamma * t64
    _check(B.nc_affine(None, ud, sd, td, 0.0, 0.1, 1.0 / (H * W)), du,
           4 * U * ((rs * u.double() * s64).abs() + (gamma * t64).abs()).expand(shape), f'nc_affine du {shape}')


# ------------------------------------------------------------------------------------------- row_scale

@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', [(3, 35, 184), (2, 64, 24), (5, 1, 8)], ids=str)
def test_row_scale(cuda, shape, dtype):
    """out[n, p, :] = x[n, p, :] scale[n]: one product, one rounding: bitwise.  Scales of exactly 0 (a
    dropped stochastic-depth path) and 1 / 0.9 (a kept one)."""
    from basicsr4rs_amd.ops import swin as S
    N, HW, c = shape
    x = _randn(shape, dtype, 70)
    scale = torch.tensor(([0.0, 1.0 / 0.9, 1.0, 1.0 / 0.9, 0.37])[:N], dtype=torch.float32)
    got = S.row_scale(x.to(cuda), scale.to(cuda), HW)
    ref = (x.double() * scale.double().view(N, 1, 1)).float().to(dtype).double()
    _check(got, ref, 0, f'row_scale {shape}')
    assert (got[0] == 0).all()


# -------------------------------------------------------------------- channel_reduce, channel_partials

CR_C = [8, 24, 64, 184, 256, 264, 512]
CR_HW = {1: (1, 1), 100: (10, 10), 256: (16, 16), 257: (1, 257), 700: (28, 25)}
CR_N = 3


def _cr_inputs(c, hw, dtype, sliced):
    H, W = CR_HW[hw]
    ld, coff = (c + 16, 8) if sliced else (c, 0)
    a, b = _randn((CR_N, H, W, ld), dtype, 80 + c), _randn((CR_N, H, W, ld), dtype, 81 + hw)
    return a, b, ld, coff


def _cr_ref(a, b, coff, c, scale):
    """(float64 scale * sum_p a (b), the issue's bound HW u sum |a b| |scale|) per (n, channel)."""
    N = a.shape[0]
    t = a.double()[..., coff:coff + c].reshape(N, -1, c)
    if b is not None:
        t = t * b.double()[..., coff:coff + c].reshape(N, -1, c)
    hw = t.shape[1]
    return scale * t.sum(1), hw * U * abs(scale) * t.abs().sum(1)


def _check_f32(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    ok = torch.isfinite(got).all().item()
    print(f'{what}: max|err| {err.max().item():.3e}, max err/bound '
          f'{(err / bound.clamp(min=1e-300)).max().item():.3f}, finite {ok}')
    assert ok, f'{what}: non-finite result (channels that were never written)'
    assert (err <= bound).all(), (what, err.max().item())


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('hw', list(CR_HW))
@pytest.mark.parametrize('c', CR_C)
def test_channel_reduce(cuda, c, hw, dtype):
    """ops.blocks.channel_reduce: per-(n, c) sum over pixels, with and without the second operand, on
    whole maps and on channel slices (coff 8 of ld C + 16), scale 1 and 1 / HW.  The bound HW u sum|a b|
    covers the HW - 1 roundings of the partial sums (whatever their order) plus one for the product or
    the scaling (bf16 products are exact; only fp32 with both has HW + 1 roundings in the worst case, which
    needs every one of them at its maximum and in the same direction); it is a condition: a dropped pixel
    or channel misses it by orders of magnitude."""
    from basicsr4rs_amd.ops import blocks as B
    for sliced in (False, True):
        a, b, ld, coff = _cr_inputs(c, hw, dtype, sliced)
        ad, bd = a.to(cuda), b.to(cuda)
        for with_b in (False, True):
            for scale in (1.0, 1.0 / hw):
                got = B.channel_reduce(ad, bd if with_b else None, scale=scale, C_=c, coff=coff)
                ref, bound = _cr_ref(a, b if with_b else None, coff, c, _f32(scale))
                _check_f32(got, ref, bound,
                           f'channel_reduce C={c} HW={hw} {_ids(dtype)} b={with_b} slice={sliced} scale={scale:.4f}')


def _raw_reduce(cuda, ad, bd, ld, coff, c, hw, scale, fill):
    """sr_channel_reduce on a workspace pre-filled with ``fill``."""
    L = _lib()
    lib = L.load()
    wsb = lib.sr_channel_reduce_workspace(CR_N, hw, c)
    assert wsb == CR_N * ((hw + 255) // 256) * c * 4
    ws = torch.full((wsb // 4, ), fill, dtype=torch.float32, device=cuda)
    out = torch.full((CR_N, c), fill, dtype=torch.float32, device=cuda)
    L.check(lib.sr_channel_reduce(L.dtype_code(ad.dtype), L.ptr(ad), ld, coff, L.ptr(bd), ld if bd is not None else 0, coff,
                                  CR_N, hw, c, scale, L.ptr(out), L.ptr(ws), wsb, L.stream()))
    return out


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('hw', [100, 700])
@pytest.mark.parametrize('c', [264, 512])
def test_channel_reduce_wide_on_nan_workspace(cuda, c, hw, dtype):
    """C above the 256 threads of the first pass: every channel's partial must be written -- on a
    workspace pre-filled with NaN an unwritten one reaches the result."""
    a, b, ld, coff = _cr_inputs(c, hw, dtype, True)
    ad, bd = a.to(cuda), b.to(cuda)
    for with_b in (False, True):
        got = _raw_reduce(cuda, ad, bd if with_b else None, ld, coff, c, hw, 1.0 / hw, float('nan'))
        ref, bound = _cr_ref(a, b if with_b else None, coff, c, _f32(1.0 / hw))
        _check_f32(got, ref, bound, f'channel_reduce on NaN workspace C={c} HW={hw} {_ids(dtype)} b={with_b}')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('hw', list(CR_HW))
@pytest.mark.parametrize('c', CR_C)
def test_channel_partials(cuda, c, hw, dtype):
    """sr_channel_partials: the first pass alone; row k of sample n holds the sums over pixels
    256 k .. 256 k + 255.  The rows are pre-filled with NaN.  Bound per row as above with its pixel count."""
    L = _lib()
    lib = L.load()
    a, b, ld, coff = _cr_inputs(c, hw, dtype, True)
    ad, bd = a.to(cuda), b.to(cuda)
    nchunk = lib.sr_channel_partials_count(hw)
    assert nchunk == (hw + 255) // 256
    for with_b in (False, True):
        parts = torch.full((CR_N, nchunk, c), float('nan'), dtype=torch.float32, device=cuda)
        L.check(lib.sr_channel_partials(L.dtype_code(dtype), L.ptr(ad), ld, coff, L.ptr(bd) if with_b else None,
                                        ld if with_b else 0, coff, CR_N, hw, c, L.ptr(parts), L.stream()))
        t = a.double()[..., coff:coff + c].reshape(CR_N, hw, c)
        if with_b:
            t = t * b.double()[..., coff:coff + c].reshape(CR_N, hw, c)
        ref = torch.stack([t[:, k * 256:(k + 1) * 256].sum(1) for k in range(nchunk)], 1)
        bound = torch.stack([t[:, k * 256:(k + 1) * 256].abs().sum(1) * min(256, hw - k * 256) * U
                             for k in range(nchunk)], 1)
        _check_f32(parts, ref, bound, f'channel_partials C={c} HW={hw} {_ids(dtype)} b={with_b}')


def _emulate_channel_reduce(t, scale):
    """The kernels' summation order in numpy fp32 on the per-pixel terms t [N, HW, C]: per 256-pixel
    chunk, lane l of 256 // (C / 8) sums pixels l, l + lanes, ...; the lanes are summed in order, then
    the chunks, then the scale is applied."""
    N, hw, c = t.shape
    lanes = 256 // (c // 8)
    out = np.zeros((N, c), dtype=np.float32)
    for k in range((hw + 255) // 256):
        chunk = t[:, k * 256:(k + 1) * 256]
        acc = np.zeros((N, lanes, c), dtype=np.float32)
        for j in range(0, chunk.shape[1], lanes):
            blk = chunk[:, j:j + lanes]
            acc[:, :blk.shape[1]] += blk
        s = np.zeros((N, c), dtype=np.float32)
        for l in range(lanes):
            s += acc[:, l]
        out += s
    return out * np.float32(scale)


@pytest.mark.parametrize('c,hw', [(64, 700), (64, 256), (184, 257), (264, 700)])
def test_channel_reduce_summation_order_bitwise(cuda, c, hw):
    """The deterministic summation order, bit for bit (fixed seed): pins the C = 64 arithmetic of the
    RCAN path (and two other widths) against any change of the reduction.  fp32 sums and bf16 dot
    products only: a product of two bf16 values is exact in fp32, so these have no fused multiply-add
    whose contraction the compiler could choose."""
    a, b, ld, coff = _cr_inputs(c, hw, torch.float32, True)
    got = _raw_reduce(cuda, a.to(cuda), None, ld, coff, c, hw, 1.0 / hw, 0.0)
    t = a[..., coff:coff + c].reshape(CR_N, hw, c).numpy()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _emulate_channel_reduce(t, 1.0 / hw).view(np.uint32))
    a, b, ld, coff = _cr_inputs(c, hw, torch.bfloat16, True)
    got = _raw_reduce(cuda, a.to(cuda), b.to(cuda), ld, coff, c, hw, 1.0, 0.0)
    t = (a.float() * b.float())[..., coff:coff + c].reshape(CR_N, hw, c).numpy()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _emulate_channel_reduce(t, 1.0).view(np.uint32))


# ------------------------------------------------------------------------------------- bilinear_up_add

def _taps(n_in, s):
    """Source taps of output index o for align_corners=False, scale 1/s, in exact arithmetic."""
    o = torch.arange(n_in * s, dtype=torch.float64)
    src = ((o + 0.5) / s - 0.5).clamp(min=0.0)
    i0 = src.floor().long()
    return i0, (i0 + 1).clamp(max=n_in - 1)


@pytest.mark.parametrize('s', [1, 2, 3, 4])
@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (2, 3, 5, 7), (1, 2, 1, 9), (1, 2, 6, 1)], ids=str)
def test_bilinear_up_add(cuda, shape, s):
    """MSRResNet skip: base + bilinear upsample (fp32 only).  Bound 8u (max |x| over the four taps +
    |base|): four weights of one or two roundings each (the source index is split into tap and weight in
    integers, so the taps are those of exact arithmetic), six products and four sums.  With the index
    evaluated in fp32 from a rounded 1/3 the kernel missed this bound at (2, 3, 5, 7), s = 3: 1.135 of it."""
    from basicsr4rs_amd.ops import blocks as B
    N, c, H, W = shape
    x = _randn(shape, torch.float32, 90)
    base = _randn((N, c, H * s, W * s), torch.float32, 91)
    got = B.bilinear_up_add(base.to(cuda), x.to(cuda), s)
    if s == 1:
        up = x.double()
    else:
        up = F.interpolate(x.double(), scale_factor=s, mode='bilinear', align_corners=False)
    ref = up + base.double()
    y0, y1 = _taps(H, s)
    x0, x1 = _taps(W, s)
    ax = x.double().abs()
    tapmax = torch.stack([ax[:, :, ya][:, :, :, xa] for ya in (y0, y1) for xa in (x0, x1)]).amax(0)
    _check(got, ref, 8 * U * (tapmax + base.double().abs()), f'bilinear_up_add {shape} s={s}')


def test_bilinear_up_add_gradients(cuda):
    from basicsr4rs_amd.ops import blocks as B
    x = _randn((1, 2, 3, 4), torch.float32, 92).to(cuda)
    base = _randn((1, 2, 6, 8), torch.float32, 93).to(cuda).requires_grad_(True)
    dy = _randn((1, 2, 6, 8), torch.float32, 94).to(cuda)
    B.bilinear_up_add(base, x, 2).backward(dy)
    assert torch.equal(base.grad, dy)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match='LR input'):
        B.bilinear_up_add(base, xg, 2).backward(dy)


# ---------------------------------------------------------------------- add_pos_embed, pos_embed_grad

APE_BIG = (2, 96, 96, 240, 240)  # N P Cp and P C both past one sweep of 8192 blocks x 256 threads


class _Ape(nn.Module):

    def __init__(self, P, c):
        super().__init__()
        g = torch.Generator().manual_seed(95)
        self.w = nn.Parameter(torch.randn(5, generator=g))  # puts the embedding at an odd flat offset
        self.absolute_pos_embed = nn.Parameter(torch.randn(1, P, c, generator=g))


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('shape', [(3, 4, 6, 60, 64), (2, 8, 8, 184, 184), APE_BIG], ids=str)
def test_add_pos_embed_and_grad(cuda, shape, dtype):
    """y = x + pos on the first C of Cp channels (one fp32 sum: u |ref|), padded channels copied through
    bitwise; dx = dy bitwise; dpos = sum over the batch of dy (N terms from 0: (N - 1) u sum|dy|), either
    freshly written, or accumulated into a FlatParams .grad view that already holds values (one more
    term: N u (sum|dy| + |prev|))."""
    from basicsr4rs_amd.ops import swin as S
    from basicsr4rs_amd.utils.flat import FlatParams
    N, H, W, c, cp = shape
    P = H * W
    if shape == APE_BIG:
        assert SWEEP < P * c < N * P * cp < 3 * SWEEP  # both kernels' grid-stride loops run again
    x, dy = _randn((N, H, W, cp), dtype, 96), _randn((N, H, W, cp), dtype, 97)
    dsum = dy.double()[..., :c].reshape(N, P, c).sum(0, keepdim=True)
    dmag = dy.double()[..., :c].reshape(N, P, c).abs().sum(0, keepdim=True)
    # fresh: a plain parameter, the gradient goes through autograd
    mod = _Ape(P, c).to(cuda)
    pos = mod.absolute_pos_embed
    pos64 = pos.detach().double().cpu()
    xd = x.to(cuda).requires_grad_(True)
    y = S.add_pos_embed(xd, pos, c)
    ref = x.double().clone()
    ref[..., :c] += pos64.view(1, H, W, c)
    fb = torch.zeros_like(ref)
    fb[..., :c] = U * ref[..., :c].abs()
    _check(y, ref, fb, f'add_pos_embed {shape}')
    assert torch.equal(_bits(y.detach()[..., c:]), _bits(xd.detach()[..., c:]))
    y.backward(dy.to(cuda))
    assert torch.equal(_bits(xd.grad), _bits(dy.to(cuda)))
    _check(pos.grad, dsum, (N - 1) * U * dmag, f'pos_embed_grad fresh {shape}')
    # accumulated: the parameter lives in a FlatParams whose gradient buffer already holds values
    mod = _Ape(P, c).to(cuda)
    flat = FlatParams(mod)
    prev = _randn((5 + P * c, ), torch.float32, 98)
    flat.grad.copy_(prev)
    pos = mod.absolute_pos_embed
    view = pos.grad
    assert view.data_ptr() == flat.grad.data_ptr() + 4 * 5
    S.add_pos_embed(x.to(cuda).requires_grad_(True), pos, c).backward(dy.to(cuda))
    assert pos.grad.data_ptr() == view.data_ptr()
    p64 = prev.double()[5:].view(1, P, c)
    _check(flat.grad[5:].view(1, P, c), dsum + p64, N * U * (dmag + p64.abs()), f'pos_embed_grad accumulated {shape}')
    assert torch.equal(flat.grad[:5].cpu(), prev[:5])
