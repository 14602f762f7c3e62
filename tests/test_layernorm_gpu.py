"""The LayerNorm kernels of csrc/swin.hip through the C ABI, against the float64 restatement
tests/_fp64.layernorm_ref on the same fp32 / bf16 input bits (conventions: top of test_eltwise_gpu.py).

Every kernel has a capped grid and a grid-stride loop; the shapes below are the smallest that enter each
loop again (and, for the unrolled vector forward, that have whole, ragged and absent rows among the RU
rows in flight).  The caps are mirrored here as named constants.

Bounds (u = 2^-24; a bf16 result: one RNE of the float64 value + 1 bf16 ulp + the fp32 bound).  Roundings
counted from the kernels, C <= 512 channels per row:
  mean   8 adds per lane + 6 butterfly adds (5 on the vector path) + the division: <= 15 roundings, each of a
         partial sum of magnitude <= C max|x|, divided by C:                          16 u max_row|x|
  rstd   d = x - mean (1), d d summed as for the mean (15), / C (1), + eps (1), rsqrtf (1 ulp = 2u), and the
         error of the fp32 mean enters squared; the power -1/2 halves the relative error of the sum:
                                                                                      32 u rstd
  y      (x - mean) (1, plus the 16 u |mean| of the mean), rstd (32 u relative + 1), gamma (1), + beta (1):
                                                             64 u (|gamma| rstd (|x| + |mean|) + |beta|)
  dx     the backward gets mean / rstd as fp32 values and the reference uses the same values, so xhat has 2
         roundings, g = dy gamma 1, the two row means 15 each relative to mean|g| and mean|g xhat|, then two
         subtractions, two products and the residual sum:
                             64 u rstd (|g| + mean_c|g| + |xhat| mean_c|g xhat|) + 2 u |res|
  dxs    dx scale: the same times |scale| + one rounding of the product.
  dgamma / dbeta, per column   D 2u sum_rows|term|, D the longest chain of sequential fp32 additions (the
         factor 2 covers the <= 3 roundings of each term for every D >= 3):
         vector path  rows per slot (ceil(M / (blocks 16))) + 16 slots summed in order + ln_bwd_reduce8:
                      1 add per accumulator (<= 512 partial rows over 64 x 8 accumulators), 3 to fold the 8, 6
                      levels of the LDS tree, 1 onto the output: rows + 27 (<= 31 here)
         scalar path  rows per wave (ceil(M / (grid 4))) + the ln_bwd_reduce loop over grid 4 partials in
                      sequence + 1: about 8200 at M > 8192.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests._fp64 import U, _assert_outside_unchanged, _bits, _check, _ids, layernorm_ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
NAN = float('nan')
JUNK = 3.0  # in the pad and gap columns of every input: the kernels must not read them into a result
SENTINEL = -12345.0
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the float argument the kernels receive
SR_EINVAL = -1

# mirrors of csrc/swin.hip
MAXC = 512  # MAXE 8 x 64 lanes of the scalar kernels
VEC_MAX_CP = 256  # ln_vec8: 32 lanes x 8 channels
FWD8_SWEEP = 4096 * 8  # ln_fwd8_kernel: blocks x half-waves; rows one k of the unrolled loop covers
FWD8_RU = 4  # rows in flight per half-wave: the outer loop steps FWD8_RU * FWD8_SWEEP
FWD_SWEEP = 16384 * 4  # ln_fwd_kernel: blocks x waves
BWD8_SLOTS, LN_BWD_BLOCKS = 16, 512  # ln_bwd8_kernel<16>
BWD8_SWEEP = LN_BWD_BLOCKS * BWD8_SLOTS
BWD_GRID, BWD_WAVES = 2048, 4  # ln_bwd_kernel
BWD_SWEEP = BWD_GRID * BWD_WAVES


def _lib():
    from basicsr4rs_amd import _lib
    return _lib


def _cp(c):
    return (c + 7) // 8 * 8


def _is_vec(dtype, cp, *lds):
    return dtype == BF16 and cp <= VEC_MAX_CP and all(ld % 8 == 0 for ld in lds)


def _depth(M, vec):
    """D of the module docstring: the longest chain of sequential fp32 additions into dgamma / dbeta."""
    if vec:
        blocks = min(-(-M // BWD8_SLOTS), LN_BWD_BLOCKS)
        return -(-M // (blocks * BWD8_SLOTS)) + BWD8_SLOTS + 1 + 3 + 6 + 1
    waves = min(-(-M // BWD_WAVES), BWD_GRID) * BWD_WAVES
    return -(-M // waves) + waves + 1


def _inputs(M, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return SimpleNamespace(x=(r(M, C) * 2 + 0.5).to(dtype), dy=r(M, C).to(dtype), res=r(M, C).to(dtype),
                           gamma=r(C) * 0.5 + 1, beta=r(C) * 0.1)


def _buf(t, ld, device):
    """[M, C] -> [M, ld] rows with JUNK in the pad and gap columns."""
    b = torch.full((t.shape[0], ld), JUNK, dtype=t.dtype)
    b[:, :t.shape[1]] = t
    return b.to(device)


# ---------------------------------------------------------------------------------------------- forward

def _fwd(cuda, x, gamma, beta, Cp, ldx=None, ldy=None, C=None):
    L = _lib()
    M, C = x.shape[0], C or x.shape[1]
    ldx, ldy = ldx or Cp, ldy or Cp
    xb = _buf(x, ldx, cuda)
    o = SimpleNamespace(y=torch.full((M, ldy), NAN, dtype=x.dtype, device=cuda),
                        mean=torch.full((M, ), NAN, device=cuda), rstd=torch.full((M, ), NAN, device=cuda))
    o.before = o.y.clone()
    gd, bd = gamma.to(cuda), beta.to(cuda)
    o.rc = L.load().sr_layernorm_fwd(L.dtype_code(x.dtype), L.ptr(xb), ldx, L.ptr(gd), L.ptr(bd), M, C, Cp, EPS, L.ptr(o.y),
                                     ldy, L.ptr(o.mean), L.ptr(o.rstd), L.stream())
    torch.cuda.synchronize()
    return o


def _check_fwd(o, R, C, Cp, what):
    assert o.rc == 0, what
    _check(o.mean, R.mean, 16 * U * R.xmax, f'{what} mean')
    _check(o.rstd, R.rstd, 32 * U * R.rstd, f'{what} rstd')
    _check(o.y[:, :C], R.y, 64 * U * R.ymag, f'{what} y')
    assert (o.y[:, C:Cp] == 0).all(), f'{what}: pad columns of y'
    _assert_outside_unchanged(o.y, o.before, 0, Cp, f'{what} y')


FWD_CASES = [
    # vector path (bf16, 16-B aligned rows, Cp <= 256)
    ((1, 1, 1), 180, BF16),  # one row: 7 idle half-waves, k = 1..3 out of range
    ((1, 1, 5), 180, BF16),  # fewer rows than the half-waves of one block
    ((5, 113, 117), 180, BF16),  # 66 105 rows: k = 0, 1 whole, k = 2 ragged, k = 3 out of range
    ((3, 211, 209), 60, BF16),  # 132 297 rows: a second outer iteration whose k = 0 is ragged
    # scalar path: more than one sweep of 16 384 blocks x 4 waves, ragged last block
    ((1, 255, 258), 60, F32),
    ((1, 255, 258), 300, BF16),
]


@pytest.mark.parametrize('shape,C,dtype', FWD_CASES, ids=lambda v: _ids(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_fwd_regimes(cuda, shape, C, dtype):
    """mean: 15 roundings -> 16u max|x|; rstd: 32u relative; y: 64u (|gamma| rstd (|x| + |mean|) + |beta|)
    (module docstring).  Rows past one sweep of each capped grid."""
    M, Cp = shape[0] * shape[1] * shape[2], _cp(C)
    vec = _is_vec(dtype, Cp, Cp)
    if M > 5:
        if vec:
            assert FWD8_SWEEP < M and (M <= FWD8_RU * FWD8_SWEEP or M < FWD8_RU * FWD8_SWEEP + FWD8_SWEEP)
            assert M % FWD8_SWEEP % 8  # the ragged k ends inside a block
        else:
            assert FWD_SWEEP < M < 2 * FWD_SWEEP and M % 4
    d = _inputs(M, C, dtype, 100 + C)
    R = layernorm_ref(d.x, d.gamma, d.beta, eps=EPS)
    _check_fwd(_fwd(cuda, d.x, d.gamma, d.beta, Cp), R, C, Cp, f'ln fwd {shape} C={C}')


# --------------------------------------------------------------------------------------------- backward

def _bwd(cuda, d, mean, rstd, Cp, res=False, scale=None, hw=1, acc=0, ld=None, fill=NAN, C=None):
    """sr_layernorm_bwd (or _scaled when ``scale`` is given) on NaN-filled dx / dxs / workspace and
    ``fill``-ed dgamma / dbeta.  ld: row strides {'dy','x','r','dx'}, default Cp."""
    L = _lib()
    lib = L.load()
    M, C = d.x.shape[0], C or d.x.shape[1]
    dtype = d.x.dtype
    ld = {**dict(dy=Cp, x=Cp, r=Cp, dx=Cp), **(ld or {})}
    ldr = ld['r'] if res else 0
    dyb, xb = _buf(d.dy, ld['dy'], cuda), _buf(d.x, ld['x'], cuda)
    rb = _buf(d.res, ld['r'], cuda) if res else None
    md, rd, gd = mean.float().to(cuda), rstd.float().to(cuda), d.gamma.to(cuda)
    o = SimpleNamespace(dx=torch.full((M, ld['dx']), NAN, dtype=dtype, device=cuda), dxs=None,
                        dg=torch.full((C, ), fill, device=cuda), db=torch.full((C, ), fill, device=cuda))
    wsb = lib.sr_layernorm_bwd_workspace(M, C)
    o.ws = torch.full((wsb // 4, ), NAN, device=cuda)
    o.before = o.dx.clone()
    o.parts = lib.sr_layernorm_bwd_parts(L.dtype_code(dtype), M, Cp, ld['x'], ld['dx'], ld['dy'], ldr)
    args = (L.dtype_code(dtype), L.ptr(dyb), ld['dy'], L.ptr(xb), ld['x'], L.ptr(md), L.ptr(rd), L.ptr(gd), M, C, Cp,
            L.ptr(rb), ldr, L.ptr(o.dx), ld['dx'], L.ptr(o.dg), L.ptr(o.db), L.ptr(o.ws), wsb, acc)
    if scale is None:
        o.rc = lib.sr_layernorm_bwd(*args, L.stream())
    else:
        o.dxs = torch.full_like(o.dx, NAN)
        sd = scale.to(cuda)
        o.rc = lib.sr_layernorm_bwd_scaled(*args, L.ptr(sd), hw, L.ptr(o.dxs), L.stream())
    torch.cuda.synchronize()
    return o


def _check_dx(o, R, d, C, Cp, res, what):
    assert o.rc == 0, what
    ref = R.dx0 + d.res.double() if res else R.dx0
    fb = 64 * U * R.dxmag + (2 * U * d.res.double().abs() if res else 0)
    _check(o.dx[:, :C], ref, fb, f'{what} dx')
    assert (o.dx[:, C:Cp] == 0).all(), f'{what}: pad columns of dx'
    _assert_outside_unchanged(o.dx, o.before, 0, Cp, f'{what} dx')
    if o.dxs is not None:
        refs = ref * R.scale
        _check(o.dxs[:, :C], refs, fb * R.scale.abs() + U * refs.abs(), f'{what} dx row_scale')
        assert (o.dxs[:, C:Cp] == 0).all(), f'{what}: pad columns of dx_scaled'
        _assert_outside_unchanged(o.dxs, o.before, 0, Cp, f'{what} dx row_scale')


def _check_params(o, R, M, vec, what):
    D = _depth(M, vec)
    _check(o.dg, R.dgamma, D * 2 * U * R.dgmag, f'{what} dgamma (D = {D})')
    _check(o.db, R.dbeta, D * 2 * U * R.dbmag, f'{what} dbeta (D = {D})')


def _scale(n):
    """A distinct stochastic-depth scale per image, one of them 0 (a dropped path)."""
    return torch.tensor([1.0 / 0.9, 0.0, 0.37, 1.0, 2.5][:n], dtype=torch.float32)


@functools.lru_cache(maxsize=3)
def _bwd_case(shape, C, dtype):
    """Inputs and the float64 reference of one backward shape, shared (read-only) by the tests below.  The
    backward is handed the fp32 rounding of the float64 statistics and the reference uses those values."""
    N, H, W = shape
    d = _inputs(N * H * W, C, dtype, 200 + C)
    d.scale = _scale(N)
    F = layernorm_ref(d.x, d.gamma, d.beta, eps=EPS)
    d.mean, d.rstd = F.mean.float(), F.rstd.float()
    return d, layernorm_ref(d.x, d.gamma, d.beta, d.dy, None, d.scale, H * W, EPS, stats=(d.mean, d.rstd))


BWD_VEC = [((1, 1, 1), 180), ((3, 47, 59), 180), ((3, 91, 91), 60)]


@pytest.mark.parametrize('shape,C', BWD_VEC, ids=str)
def test_layernorm_bwd_vector_regimes(cuda, shape, C):
    """ln_bwd8_kernel<16> + ln_bwd_reduce8: one row, just past one sweep of 512 blocks x 16 slots (8319 rows,
    three images), and three sweeps deep (24 843 rows); each with / without the residual and with / without
    the row-scaled second output.  dx: 64u rstd (...) + 2u |res|; dgamma / dbeta: D 2u sum|term|, D = rows per
    slot + 27 (module docstring)."""
    N, H, W = shape
    M, Cp = N * H * W, _cp(C)
    if M > 1:
        assert M % (H * W) == 0 and M > BWD8_SWEEP and M % BWD8_SLOTS
    d, R = _bwd_case(shape, C, BF16)
    for res in (False, True):
        for scaled in (False, True):
            what = f'ln bwd8 {shape} C={C} res={res} scaled={scaled}'
            o = _bwd(cuda, d, d.mean, d.rstd, Cp, res=res, scale=d.scale if scaled else None, hw=H * W)
            assert o.parts == min(-(-M // BWD8_SLOTS), LN_BWD_BLOCKS)
            _check_dx(o, R, d, C, Cp, res, what)
            _check_params(o, R, M, True, what)
            if scaled:
                assert (o.dxs[H * W:2 * H * W] == 0).all() if N > 1 else True
                # the partial rows are all the kernel leaves in the workspace
                used = o.parts * 2 * C
                assert torch.isfinite(o.ws[:used]).all() and torch.isnan(o.ws[used:]).all()
    if N == 1:  # a single image cannot hold both: the dropped path on its own
        o = _bwd(cuda, d, d.mean, d.rstd, Cp, res=True, scale=torch.zeros(1), hw=1)
        assert o.rc == 0 and (o.dxs[:, :Cp] == 0).all()


@pytest.mark.parametrize('C,dtype', [(180, F32), (300, BF16)],
                         ids=lambda v: _ids(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_bwd_scalar_regime(cuda, C, dtype):
    """ln_bwd_kernel<T> + ln_bwd_reduce just past one sweep of 2048 blocks x 4 waves (8319 rows): two rows
    for the first waves, one for the rest.  D = 2 + 8192 + 1.  The row-scaled form is refused on this path
    and launches nothing."""
    shape = (3, 47, 59)
    M, Cp = 3 * 47 * 59, _cp(C)
    assert BWD_SWEEP < M < 2 * BWD_SWEEP and M % 4
    d, R = _bwd_case(shape, C, dtype)
    for res in (False, True):
        what = f'ln bwd scalar {shape} C={C} res={res}'
        o = _bwd(cuda, d, d.mean, d.rstd, Cp, res=res)
        assert o.parts == 0
        _check_dx(o, R, d, C, Cp, res, what)
        _check_params(o, R, M, False, what)
    o = _bwd(cuda, d, d.mean, d.rstd, Cp, res=True, scale=d.scale, hw=47 * 59, fill=SENTINEL)
    assert o.rc == SR_EINVAL
    assert torch.equal(_bits(o.dx), _bits(o.before)) and torch.equal(_bits(o.dxs), _bits(o.before))
    assert (o.dg == SENTINEL).all() and (o.db == SENTINEL).all() and torch.isnan(o.ws).all()


# ----------------------------------------------------------------------------------------------- widths

WIDTH_M = 37  # ragged against the 8 half-waves, 16 slots and 4 waves of a block; one image per row


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('C,Cp', [(256, 256), (250, 256), (5, 8), (512, 512)])
def test_layernorm_widths(cuda, C, Cp, dtype):
    """The last lane group of the vector kernels (Cp 256, full and with 6 pad columns), one lane group
    (Cp 8), and MAXE full in the scalar kernels (C 512); bounds as in the regime tests."""
    M = WIDTH_M
    vec = _is_vec(dtype, Cp, Cp)
    d = _inputs(M, C, dtype, 300 + C)
    Rf = layernorm_ref(d.x, d.gamma, d.beta, eps=EPS)
    _check_fwd(_fwd(cuda, d.x, d.gamma, d.beta, Cp), Rf, C, Cp, f'ln fwd width C={C}/{Cp}')
    mean, rstd = Rf.mean.float(), Rf.rstd.float()
    scale = torch.arange(M, dtype=torch.float32) * 0.05  # image 0 dropped
    R = layernorm_ref(d.x, d.gamma, d.beta, d.dy, None, scale, 1, EPS, stats=(mean, rstd))
    o = _bwd(cuda, d, mean, rstd, Cp, res=True, scale=scale if vec else None, hw=1)
    assert (o.parts > 0) == vec
    _check_dx(o, R, d, C, Cp, True, f'ln bwd width C={C}/{Cp}')
    _check_params(o, R, M, vec, f'ln bwd width C={C}/{Cp}')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_layernorm_c513_refused(cuda, dtype):
    """C above the 512 channels the scalar kernels hold in registers: SR_EINVAL, nothing launched."""
    C, Cp, M = MAXC + 1, _cp(MAXC + 1), 5
    d = _inputs(M, C, dtype, 313)
    o = _fwd(cuda, d.x, d.gamma, d.beta, Cp)
    assert o.rc == SR_EINVAL and torch.equal(_bits(o.y), _bits(o.before))
    assert torch.isnan(o.mean).all() and torch.isnan(o.rstd).all()
    o = _bwd(cuda, d, torch.zeros(M), torch.ones(M), Cp, res=True, fill=SENTINEL)
    assert o.rc == SR_EINVAL and torch.equal(_bits(o.dx), _bits(o.before))
    assert (o.dg == SENTINEL).all() and (o.db == SENTINEL).all() and torch.isnan(o.ws).all()


# ---------------------------------------------------------------------------------------------- strides

STRIDE_SHAPE = (3, 1, 59)  # 177 rows: several blocks of every kernel, the last one ragged


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
@pytest.mark.parametrize('odd', [False, True], ids=['ld%8==0', 'ld%8!=0'])
def test_layernorm_row_strides(cuda, odd, dtype):
    """Five different row strides.  All multiples of 8: bf16 stays on the vector kernels
    (sr_layernorm_bwd_parts > 0); with ldx = Cp + 4 it takes the scalar kernels (parts == 0) and still
    matches.  The gap columns between Cp and each stride keep their sentinel bits."""
    N, H, W = STRIDE_SHAPE
    M, C = N * H * W, 180
    Cp = _cp(C)
    ld = dict(x=Cp + (4 if odd else 8), dy=Cp + 32, r=Cp + 40, dx=Cp + 24)
    ldy = Cp + 16
    d = _inputs(M, C, dtype, 400)
    Rf = layernorm_ref(d.x, d.gamma, d.beta, eps=EPS)
    _check_fwd(_fwd(cuda, d.x, d.gamma, d.beta, Cp, ldx=ld['x'], ldy=ldy), Rf, C, Cp, f'ln fwd strides odd={odd}')
    mean, rstd = Rf.mean.float(), Rf.rstd.float()
    scale = _scale(N)
    R = layernorm_ref(d.x, d.gamma, d.beta, d.dy, None, scale, H * W, EPS, stats=(mean, rstd))
    vec = _is_vec(dtype, Cp, *ld.values())
    assert vec == (dtype == BF16 and not odd)
    o = _bwd(cuda, d, mean, rstd, Cp, res=True, scale=scale if vec else None, hw=H * W, ld=ld)
    assert (o.parts > 0) == vec and (vec or o.parts == 0)
    _check_dx(o, R, d, C, Cp, True, f'ln bwd strides odd={odd}')
    _check_params(o, R, M, vec, f'ln bwd strides odd={odd}')


# ------------------------------------------------------------------------ rows that stress the statistics

CONST = 3.25  # bf16-representable: the 180 partial sums of the row are exact in fp32, so is sum / C


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_layernorm_degenerate_rows(cuda, dtype):
    """A constant row (every partial sum and the mean exact in fp32, so x - mean = 0 and y == beta exactly),
    an all-zero row, and a row with mean 100 and deviation 1 (the variance is a difference of values 100
    times its size); rstd of the first two against eps^-1/2 to 32u; dx finite and within the bound."""
    M, C = WIDTH_M, 180
    Cp = _cp(C)
    d = _inputs(M, C, dtype, 500)
    d.x[3], d.x[7] = CONST, 0.0
    d.x[11] = (100.0 + torch.randn(C, generator=torch.Generator().manual_seed(501))).to(dtype)
    Rf = layernorm_ref(d.x, d.gamma, d.beta, eps=EPS)
    assert abs(Rf.mean[11].item() - 100) < 1 and abs(Rf.rstd[11].item() - 1) < 0.2
    o = _fwd(cuda, d.x, d.gamma, d.beta, Cp)
    _check_fwd(o, Rf, C, Cp, 'ln fwd degenerate rows')
    for r in (3, 7):
        assert torch.equal(o.y[r, :C].cpu(), d.beta.to(dtype)), f'row {r}: y != beta'
        assert abs(o.rstd[r].item() - EPS**-0.5) <= 32 * U * EPS**-0.5
    assert o.mean[3].item() == CONST and o.mean[7].item() == 0
    mean, rstd = Rf.mean.float(), Rf.rstd.float()
    R = layernorm_ref(d.x, d.gamma, d.beta, d.dy, stats=(mean, rstd), eps=EPS)
    vec = _is_vec(dtype, Cp, Cp)
    for res in (False, True):
        ob = _bwd(cuda, d, mean, rstd, Cp, res=res)
        _check_dx(ob, R, d, C, Cp, res, f'ln bwd degenerate rows res={res}')
        _check_params(ob, R, M, vec, f'ln bwd degenerate rows res={res}')


# ------------------------------------------------------------------------------------------- accumulate

ACC_SHAPE, ACC_C = (3, 47, 59), 180


def test_layernorm_bwd_accumulate_vector_bitwise(cuda):
    """accumulate on the vector path.  Bit 0: dgamma / dbeta pre-filled with 0.5 end as fl(0.5 + inline
    result), bitwise.  Bit 1: they keep their sentinel bits and sr_layernorm_bwd_reduce on the workspace
    gives the inline result (with its own accumulate bit: 0.5 + it), bitwise.  A repeat is bitwise equal.
    dx / dx_scaled do not depend on the bits.  The workspace is NaN before every call."""
    L = _lib()
    lib = L.load()
    N, H, W = ACC_SHAPE
    M, C, Cp = N * H * W, ACC_C, _cp(ACC_C)
    d, R = _bwd_case(ACC_SHAPE, C, BF16)
    run = lambda acc, fill: _bwd(cuda, d, d.mean, d.rstd, Cp, res=True, scale=d.scale, hw=H * W, acc=acc, fill=fill)
    base, again = run(0, NAN), run(0, NAN)
    assert base.rc == 0 and base.parts == LN_BWD_BLOCKS
    _check_params(base, R, M, True, 'ln bwd8 accumulate base')
    same = lambda a, b: all(torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))) for k in ('dx', 'dxs'))
    assert same(base, again)
    assert torch.equal(_bits(base.dg), _bits(again.dg)) and torch.equal(_bits(base.db), _bits(again.db))
    used = base.parts * 2 * C
    assert torch.equal(_bits(base.ws[:used]), _bits(again.ws[:used]))
    half = lambda t: _bits(t.cpu() + 0.5)
    o = run(1, 0.5)
    assert o.rc == 0 and same(o, base)
    assert torch.equal(_bits(o.dg.cpu()), half(base.dg)) and torch.equal(_bits(o.db.cpu()), half(base.db))
    for acc in (2, 3):
        o = run(acc, SENTINEL)
        assert o.rc == 0 and same(o, base)
        assert (o.dg == SENTINEL).all() and (o.db == SENTINEL).all(), f'accumulate {acc} wrote dgamma / dbeta'
        assert torch.equal(_bits(o.ws[:used]), _bits(base.ws[:used])) and torch.isnan(o.ws[used:]).all()
        for racc, fill, want in ((0, NAN, lambda t: _bits(t.cpu())), (1, 0.5, half)):
            dg, db = torch.full((C, ), fill, device=cuda), torch.full((C, ), fill, device=cuda)
            L.check(lib.sr_layernorm_bwd_reduce(L.ptr(o.ws), o.parts, C, L.ptr(dg), L.ptr(db), racc, L.stream()))
            torch.cuda.synchronize()
            assert torch.equal(_bits(dg.cpu()), want(base.dg)) and torch.equal(_bits(db.cpu()), want(base.db))


def test_layernorm_bwd_accumulate_scalar(cuda):
    """On the scalar path (here fp32) sr_layernorm_bwd_parts is 0 and bit 1 is ignored: the inline result
    appears (bitwise the accumulate-0 one, which is checked against the bound), bit 0 adds onto 0.5."""
    N, H, W = ACC_SHAPE
    M, C, Cp = N * H * W, ACC_C, _cp(ACC_C)
    d, R = _bwd_case(ACC_SHAPE, C, F32)
    run = lambda acc, fill: _bwd(cuda, d, d.mean, d.rstd, Cp, res=True, acc=acc, fill=fill)
    base = run(0, NAN)
    assert base.rc == 0 and base.parts == 0
    _check_params(base, R, M, False, 'ln bwd scalar accumulate base')
    for acc, fill in ((2, NAN), (0, NAN), (1, 0.5), (3, 0.5)):
        o = run(acc, fill)
        want = (lambda t: _bits(t.cpu() + 0.5)) if acc & 1 else (lambda t: _bits(t.cpu()))
        assert o.rc == 0 and torch.equal(_bits(o.dx), _bits(base.dx))
        assert torch.equal(_bits(o.dg.cpu()), want(base.dg)) and torch.equal(_bits(o.db.cpu()), want(base.db)), acc


# --------------------------------------------------------------------------------------------- wrappers

@pytest.mark.parametrize('C,dtype', [(180, BF16), (180, F32), (300, BF16)],
                         ids=lambda v: _ids(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_wrappers_chained(cuda, C, dtype):
    """ops.swin.layernorm -> ops.swin.layernorm_bwd on an [N, H, W, Cp] map, one case per kernel pair; the
    backward is handed the forward kernel's own mean / rstd (the reference uses those values too).  Where the
    wrapper cannot use the fused row-scaled output it scales the stored dx with row_scale: one product of
    the rounded dx, bitwise."""
    from basicsr4rs_amd.ops import swin as S
    N, H, W = ACC_SHAPE
    M, Cp = N * H * W, _cp(C)
    d, _ = _bwd_case(ACC_SHAPE, C, dtype)
    pad = lambda t: torch.nn.functional.pad(t, (0, Cp - C)).view(N, H, W, Cp).to(cuda)
    gamma, beta = d.gamma.to(cuda), d.beta.to(cuda)
    y, mean, rstd = S.layernorm(pad(d.x), gamma, beta, C, eps=1e-5)
    Rf = layernorm_ref(d.x, d.gamma, d.beta, eps=EPS)
    o = SimpleNamespace(rc=0, y=y.view(M, Cp), mean=mean, rstd=rstd, before=y.view(M, Cp))
    _check_fwd(o, Rf, C, Cp, f'S.layernorm C={C}')
    R = layernorm_ref(d.x, d.gamma, d.beta, d.dy, None, d.scale, H * W, EPS, stats=(mean.cpu(), rstd.cpu()))
    (dx, dxs), dg, db = S.layernorm_bwd(pad(d.dy), pad(d.x), mean, rstd, gamma, C, res=pad(d.res),
                                        row_scale=d.scale.to(cuda))
    vec = _is_vec(dtype, Cp, Cp)
    o = SimpleNamespace(rc=0, dx=dx.view(M, Cp), dxs=dxs.view(M, Cp) if vec else None, dg=dg, db=db, before=dx.view(M, Cp))
    _check_dx(o, R, d, C, Cp, True, f'S.layernorm_bwd C={C}')
    _check_params(o, R, M, vec, f'S.layernorm_bwd C={C}')
    if not vec:
        want = (dx.view(M, Cp).double().cpu() * R.scale).float().to(dtype)
        assert torch.equal(_bits(dxs.view(M, Cp).cpu()), _bits(want))
