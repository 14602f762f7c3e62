"""The two fused Swin block kernels of csrc/swin_fused.hip through the C ABI, stage by stage against the
float64 restatements of tests/_fp64.py (conventions: top of test_eltwise_gpu.py).

    sr_swin_attn_fused_fwd   x -> ln_out, mean, rstd -> qkv -> lse, attention out -> x2
    sr_swin_mlp_fused_fwd    x -> ln_out, mean, rstd -> z (= GELU'), h (= GELU) -> out

Every stage is compared with float64 computed from the kernel's OWN stored input to that stage (the kernel
writes the same bf16 bits to HBM and to the LDS tile the next stage reads), so a comparison crosses one bf16
rounding: `_check` allows one RNE of the float64 value + 1 bf16 ulp + the fp32 bound derived below.  Every
output is pre-filled with NaN and sits inside a larger allocation whose sentinel rows before and after must
keep their bits.  One end-to-end float64 assertion per case remains (x2, out), normalised per element.

Bounds (u = 2^-24), roundings counted from the kernels:
  mean     ln_row4_stats: 24 sequential packed adds per half, the fold of the two halves, two shuffle adds,
           the division: <= 28 roundings of partial sums of magnitude <= sum_c|x|, over C:  28 u mean_c|x|
  rstd     32 u rstd, the bound of the standalone LayerNorm kernel these kernels replace
           (test_layernorm_gpu.py).  With the pad lanes out of the squared-deviation sum: d = x - mu (1), d d
           (1), 24 + 1 + 2 adds, / C, + eps: <= 31 roundings relative to the sum, halved by the power -1/2,
           + 2 u |mu error|-terms (the error of mu enters squared) + rsqrtf (2 u): < 32 u.
  ln_out   x A + B with A = rs gamma, B = beta - mu A: 64 u (|gamma| rstd (|x| + |mean|) + |beta|) as for the
           standalone kernel; pad channels C..Cp exactly 0.
  qkv      from the stored ln_out and the bf16 weight image: Cp products summed in fp32 by the MFMAs + the
           bias add: (Cp + 2) u (sum|w x| + |b|); pad head dims exactly 0.
  scores   (natural-log units; the kernel works in base 2) v = fma(q.k, scale log2e, table log2e + mask):
           32-term fp32 dot (32), fl(scale log2e) (1.5), the fma (1): 36 u scale sum|q k|; the table entry
           times log2e (1.5), + mask (1), the fma (1): 4 u |bias|, 4 u 100 on masked pairs; v - max: u |s - max s|;
           v_exp_f32: 1 ulp = 2 u.  rho_k = the sum of these is the relative error of the unnormalised P_k.
  lse      d lse = sum_k P_k rho_k; the sum of 64 terms: 15 sequential adds + 2 cross-lane: 18 u; v_log_f32
           1 ulp: 2 u (ln sum + 1); max + log2, times ln 2 (constant rounded): 3 u |lse|
  attn out numerator sum_k bf16(e_k) v_k / denominator sum_k e_k, e_k = exp(s_k - max s) the unnormalised P:
           sum_k halfulp_bf16(e_k) |v_k| / sum_k e_k  [the RNE of each e_k to bf16: half an ulp of e_k, between
           2^-9 e_k and 2^-8 e_k, so between 2^-9 and 2^-8 sum_k P_k|v_k|; with the flat 2^-9 the kernel measured
           1.04 of the bound]  +  sum_k P_k |v_k| rho_k  +  sum_k P_k|v_k| (64 u [MFMA accumulation over 64 keys]
           + 18 u + rho_bar [the denominator, rho_bar = sum_k P_k rho_k] + 2 u [v_rcp_f32] + u [the product]:
           90 u + rho_bar) + 64 2^-126 max|v| (e_k below the smallest normal may flush to 0); pad head dims exactly 0.
  x2       from the stored attention out: x + s1[n] (proj + bias): nH 32 products, the bias add, the scale
           and the residual add: (nH 32 + 3) u |s1| (sum|w a| + |b|) + u |x|; pad channels exactly 0.
  z, h     from the stored ln_out: v = fc1 with e_v = (Cp + 2) u (sum|w x| + |b|), through the GELU pair of
           csrc/sr_common.h whose erf approximation documents |erf error| <= 4.7e-7 (ERF_ERR, taken from that
           comment): h = v Phi(v): |GELU'| <= 1.13 -> 1.13 e_v + 0.5 |v| ERF_ERR + 2 u |h|;
           z = Phi(v) + v phi(v): |GELU''| <= 0.8 -> 0.8 e_v + 0.5 ERF_ERR + |v| phi(v) u (2 v^2 + 6) [the
           exponent -v^2 log2e / 2 carries 4 relative roundings, v_exp_f32 2 u, the product and fma] + u |z|.
           Pad hidden columns: bitwise what the unfused lin kernel writes there.
  out      from the stored h: (Hp + 3) u |s2| (sum|w h| + |b|) + u |x|.

Measured on an MI355X, worst max err / bound over the cases (attention kernel; MLP kernel): mean 0.039; 0.033,
rstd 0.075; 0.065 (before the pads left the squared-deviation sum of ln_row4_stats: 199.6 at C 60 and 2.9 at
C 180 on the offset rows, 5.6 at C 8 on randn rows), lse 0.129, attention out 0.736, and 0.99 for every other
bf16 stage (one bf16 ulp of the two the comparison allows, as in every bf16 `_check` of the suite).

End to end (x2, out against float64 through all stages, four bf16 roundings on the way): the error per
element over |x| + |s| (sum|w a| + |b|) of the float64 chain, worst element per case, must stay within twice
what the unfused HIP path (LN + lin kernel, sr_window_attn_fwd, linears), which rounds at the same four
points and differs by summation order only, measured on the same case (E2E_UNFUSED_ATTN / _MLP below,
recorded on an MI355X with the fused kernels' ratios of the same run next to them: fused / unfused is 0.85 ..
1.08 for the attention half; the MLP half reaches the same worst element to every printed digit).  Each
test prints both ratios again.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests._fp64 import U, _bf16_ulp, _bits, _check, gelu_ref, layernorm_ref, linear_ref, window_attention_ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float('nan')
SENTINEL = -12345.0
GUARD = 16  # sentinel rows (of a map) or 16-element groups (of a vector) before and after every output
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the float argument the kernels receive
SR_EINVAL = -1
ERF_ERR = 4.7e-7  # csrc/sr_common.h, erf_fast: |error| <= 4.7e-7 over all x
SCALES = [1.0 / 0.9, 0.37, 2.5]  # stochastic-depth factors: distinct per image, none of them 1
SIGMAS, OFFSETS = [2.0, 1.0, 0.25], [0.0, 2.0, -2.0, 4.0, -4.0, 8.0]


def _lib():
    from basicsr4rs_amd import _lib
    return _lib


def _cp(c):
    return (c + 7) // 8 * 8


class _Out:
    """An output of ``rows`` rows, NaN-filled, inside an allocation with GUARD sentinel rows on either side."""

    def __init__(self, device, dtype, rows, width=None):
        g = GUARD if width is not None else GUARD * 16
        shape = (rows + 2 * g, ) + ((width, ) if width is not None else ())
        self.buf = torch.full(shape, SENTINEL, dtype=dtype, device=device)
        self.t = self.buf[g:g + rows]
        self.t.fill_(NAN)
        self.before = self.buf.clone()
        self.g = g

    def guards_intact(self):
        b, a = _bits(self.buf), _bits(self.before)
        return torch.equal(b[:self.g], a[:self.g]) and torch.equal(b[-self.g:], a[-self.g:])

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def _x_rows(g, M, C, offset_rows):
    """[M, C] bf16 rows: randn, or randn sigma + offset with sigma cycling over SIGMAS and the offset over
    OFFSETS by row (every pair occurs), rows whose mean is large against their spread."""
    x = torch.randn(M, C, generator=g)
    if offset_rows:
        r = torch.arange(M)
        x = x * torch.tensor(SIGMAS)[r % 3][:, None] + torch.tensor(OFFSETS)[(r // 3) % 6][:, None]
    return x.to(BF16)


def _padded(t, width):
    out = torch.zeros(*t.shape[:-1], width, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def _dev(d, device):
    """The tensors of a data namespace on the device (None stays None)."""
    return SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(d).items()})


def _check_ln(o, x, gamma, beta, C, Cp, what):
    """mean / rstd / ln_out of either kernel against layernorm_ref of the bf16 input rows."""
    R = layernorm_ref(x[:, :C], gamma, beta, eps=EPS)
    _check(o.mean.t, R.mean, 28 * U * R.xabsmean, f'{what} mean')
    _check(o.rstd.t, R.rstd, 32 * U * R.rstd, f'{what} rstd')
    _check(o.ln.t[:, :C], R.y, 64 * U * R.ymag, f'{what} ln_out')
    assert (o.ln.t[:, C:] == 0).all(), f'{what}: pad channels of ln_out'
    return R


# ------------------------------------------------------------------------------------------- attention kernel

ATTN_CASES = [  # N, H, W, C, nH, shift, row_scale, data
    (3, 8, 24, 60, 6, 4, True, 'randn'),  # 9 windows: pair (2, 3) straddles images 0 / 1, odd tail block, H == window
    (1, 24, 24, 180, 6, 4, False, 'randn'),  # 3 x 3 windows: interior, edge and corner masks; odd count
    (1, 16, 16, 96, 3, 3, False, 'randn'),  # shift 3
    (1, 16, 16, 96, 3, 7, False, 'randn'),  # shift 7
    (1, 8, 16, 192, 6, 0, True, 'randn'),  # C = Cp = 192, hd 32: no pad anywhere, the _ok limit
    (2, 8, 8, 24, 1, 4, True, 'randn'),  # one head: no next-head prefetch; C = 24
    (1, 8, 16, 160, 5, 0, False, 'randn'),  # five heads: odd slot parity at the last head
    (1, 8, 16, 100, 4, 4, False, 'randn'),  # hd 25, Cp 104
    (2, 16, 16, 60, 6, 4, True, 'offset'),  # rows with a mean offset
    (2, 16, 16, 180, 6, 4, True, 'offset'),
    (1, 8, 16, 96, 3, 4, False, 'wide'),  # scores of a query spread over >= 40 nats
]

# worst |x2 - float64| / (|x| + |s1| (sum|w a| + |b|)) per case: (unfused path, fused kernel), MI355X
E2E_UNFUSED_ATTN = {
    (3, 8, 24, 60, 6, 4, True, 'randn'): (4.127e-03, 3.867e-03),
    (1, 24, 24, 180, 6, 4, False, 'randn'): (3.022e-03, 2.667e-03),
    (1, 16, 16, 96, 3, 3, False, 'randn'): (3.200e-03, 3.463e-03),
    (1, 16, 16, 96, 3, 7, False, 'randn'): (3.088e-03, 3.253e-03),
    (1, 8, 16, 192, 6, 0, True, 'randn'): (2.490e-03, 2.436e-03),
    (2, 8, 8, 24, 1, 4, True, 'randn'): (5.837e-03, 5.417e-03),
    (1, 8, 16, 160, 5, 0, False, 'randn'): (2.545e-03, 2.545e-03),
    (1, 8, 16, 100, 4, 4, False, 'randn'): (3.374e-03, 2.853e-03),
    (2, 16, 16, 60, 6, 4, True, 'offset'): (3.755e-03, 4.019e-03),
    (2, 16, 16, 180, 6, 4, True, 'offset'): (3.644e-03, 3.609e-03),
    (1, 8, 16, 96, 3, 4, False, 'wide'): (1.492e-02, 1.492e-02),
}


@functools.lru_cache(maxsize=None)
def _attn_data(case):
    N, H, W, C, nH, shift, rsc, kind = case
    g = torch.Generator().manual_seed(1000 * N + 10 * H + C + shift)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    Cp, hd, M = _cp(C), C // nH, N * H * W
    assert hd * nH == C and hd <= 32
    d = SimpleNamespace(N=N, H=H, W=W, C=C, Cp=Cp, nH=nH, hd=hd, shift=shift, M=M)
    d.x = _padded(_x_rows(g, M, C, kind == 'offset'), Cp)
    d.gamma, d.beta = 1 + 0.1 * r(C), 0.1 * r(C)
    wq = torch.zeros(3, nH, 32, Cp)
    wq[:, :, :hd, :C] = r(3, nH, hd, C) * C**-0.5
    if kind == 'wide':
        wq[:2] *= 3.5  # q and k rows: scores 12 times as wide
    d.wq = wq.reshape(3 * nH * 32, Cp).to(BF16)
    bq = torch.zeros(3, nH, 32)
    bq[:, :, :hd] = r(3, nH, hd) * 0.05
    d.bq = bq.reshape(-1)
    d.table = r(225, nH) * 0.5
    wp = torch.zeros(Cp, nH, 32)
    wp[:C, :, :hd] = r(C, nH, hd) * C**-0.5
    d.wp = wp.reshape(Cp, nH * 32).to(BF16)
    d.bp = _padded(r(C) * 0.05, Cp)
    d.s1 = torch.tensor(SCALES[:N]) if rsc else None
    d.scale = float(torch.tensor(hd**-0.5, dtype=torch.float32))
    d.srow = (d.s1.double().repeat_interleave(H * W) if rsc else torch.ones(M, dtype=torch.float64))[:, None]
    return d


def _attn_outputs(device, d, geom=None):
    N, H, W, nH, Cp = geom or (d.N, d.H, d.W, d.nH, d.Cp)
    M = N * H * W
    return SimpleNamespace(x2=_Out(device, BF16, M, Cp), ln=_Out(device, BF16, M, Cp), mean=_Out(device, torch.float32, M),
                           rstd=_Out(device, torch.float32, M), qkv=_Out(device, BF16, M, 3 * nH * 32),
                           ao=_Out(device, BF16, M, nH * 32),
                           lse=_Out(device, torch.float32, N * (H // 8) * (W // 8) * nH * 64))


ATTN_SAVED = ('ln', 'mean', 'rstd', 'qkv', 'ao', 'lse')


def _call_attn(dd, o, train=True, null=(), **geom):
    """sr_swin_attn_fused_fwd on the device data ``dd`` into the outputs ``o``; ``geom`` overrides the
    geometry arguments, ``null`` names saved-tensor pointers passed as NULL."""
    L = _lib()
    a = dict(N=dd.N, H=dd.H, W=dd.W, shift=dd.shift, nH=dd.nH, C=dd.C, Cp=dd.Cp)
    a.update(geom)
    p = {k: (L.ptr(getattr(o, k).t) if train and k not in null else None) for k in ATTN_SAVED}
    rc = L.load().sr_swin_attn_fused_fwd(L.ptr(dd.x), L.ptr(dd.gamma), L.ptr(dd.beta), a['C'], EPS, L.ptr(dd.wq), L.ptr(dd.bq),
                                         L.ptr(dd.table), L.ptr(dd.wp), L.ptr(dd.bp), L.ptr(dd.s1), a['N'], a['H'], a['W'],
                                         a['shift'], a['nH'], a['Cp'], dd.scale, L.ptr(o.x2.t), p['ln'], p['mean'],
                                         p['rstd'], p['qkv'], p['ao'], p['lse'], L.stream())
    torch.cuda.synchronize()
    return rc


def _unfused_attn(dd):
    """x2 of the three-launch path on the same operands (LN + qkv lin kernel, attention kernel, proj)."""
    from basicsr4rs_amd.ops import swin as S
    g = S.AttnGeom(dd.C, dd.nH, 8, dd.shift)
    N, H, W = dd.N, dd.H, dd.W
    x = dd.x.view(N, H, W, dd.Cp)
    fz = S.linear_ln_fwd(x, dd.gamma, dd.beta, dd.C, dd.wq, dd.bq, g.qkv, N, H, W)
    if fz is not None:
        qkv = fz[0]
    else:
        qkv = S.linear_fwd(S.layernorm(x, dd.gamma, dd.beta, dd.C)[0], dd.wq, dd.bq, g.qkv, N, H, W)
    a, _ = S.window_attn(qkv, g, N, H, W, dd.scale, dd.table)
    x2 = S.linear_fwd(a, dd.wp, dd.bp, g.proj, N, H, W, res=x, beta=1.0, row_scale=dd.s1)
    torch.cuda.synchronize()
    return x2.view(dd.M, dd.Cp)


def _e2e_ratio(got, ref, mag, C):
    return ((got[:, :C].double().cpu() - ref[:, :C]).abs() / mag[:, :C]).max().item()


@pytest.mark.parametrize('case', ATTN_CASES, ids=str)
def test_swin_attn_fused_stages(cuda, case):
    """Each stage of swin_attn_block_fwd_kernel from its own stored input under the bounds of the module
    docstring; pads exactly 0; sentinels intact; the inference call bitwise the same x2; x2 end to end against
    float64 within twice the unfused path's ratio (E2E_UNFUSED_ATTN)."""
    N, H, W, C, nH, shift, rsc, kind = case
    d = _attn_data(case)
    dd = _dev(d, cuda)
    Cp, hd, M = d.Cp, d.hd, d.M
    what = f'attn {case}'
    o = _attn_outputs(cuda, d)
    assert _call_attn(dd, o) == 0, what
    for k, v in vars(o).items():
        assert v.guards_intact(), f'{what}: wrote outside {k}'
    x = d.x.double()

    # ---- LayerNorm
    R = _check_ln(o, x, d.gamma, d.beta, C, Cp, what)

    # ---- qkv from the stored ln_out
    ln = o.ln.t.double().cpu()
    y, mag = linear_ref(ln, d.wq, d.bq)
    _check(o.qkv.t, y, (Cp + 2) * U * mag, f'{what} qkv')
    assert (o.qkv.t.view(M, 3 * nH, 32)[..., hd:] == 0).all(), f'{what}: pad head dims of qkv'

    # ---- lse and the attention output from the stored qkv
    A = window_attention_ref(o.qkv.t.double().cpu().view(N, H, W, -1), nH, shift, d.scale, d.table)
    live = ~A.masked[:, None].expand_as(A.P)
    if shift:  # the windows of a shifted case hold masked and unmasked (query, key) pairs
        per_win = A.masked.flatten(1)
        assert (per_win.any(1) & ~per_win.all(1)).any(), what
    if kind == 'wide':
        s_live = torch.where(live, A.s, A.s.amax(-1, keepdim=True))
        spread = (A.s.amax(-1) - s_live.amin(-1)).max().item()
        small = ((A.P < 2.0**-24 * A.P.amax(-1, keepdim=True)) & live).sum().item()
        print(f'{what}: widest unmasked score spread {spread:.1f} nats, {small} unmasked P below 2^-24 of their row maximum')
        assert spread >= 40 and small > 0
    smax = A.s.amax(-1, keepdim=True)
    rho = U * (36 * d.scale * A.absqk + 4 * A.bias.abs()[None] + 400.0 * A.masked[:, None] + (A.s - smax).abs() + 2)
    Prho = A.P * rho
    rho_bar = Prho.sum(-1)
    lnsum = A.lse - smax[..., 0]
    _check(o.lse.t, A.lse.reshape(-1), (rho_bar + U * (18 + 2 * (lnsum + 1) + 3 * A.lse.abs())).reshape(-1), f'{what} lse')
    e = torch.exp(A.s - smax)  # the unnormalised P the kernel rounds to bf16 (its row maximum is exactly 1)
    half_ulp = 0.5 * _bf16_ulp(e * (1 + 2.0**-12))  # (the kernel's e_k may sit across a binade edge from ours)
    fb = A.to_map((half_ulp @ A.absv) / e.sum(-1, keepdim=True) + Prho @ A.absv) \
        + A.pabsv * (90 * U + A.to_map(rho_bar[..., None].expand(-1, -1, -1, 32))) + 64 * 2.0**-126 * A.absv.max()
    pad_dim = (torch.arange(nH * 32) % 32 >= hd)
    fb[..., pad_dim] = 0
    _check(o.ao.t, A.out.reshape(M, -1), fb.reshape(M, -1), f'{what} attention out')
    assert (o.ao.t[:, pad_dim.to(cuda)] == 0).all(), f'{what}: pad head dims of the attention output'

    # ---- x2 from the stored attention output
    ao = o.ao.t.double().cpu()
    y, mag = linear_ref(ao, d.wp, d.bp)
    _check(o.x2.t, x + d.srow * y, (nH * 32 + 3) * U * d.srow.abs() * mag + U * x.abs(), f'{what} x2')
    assert (o.x2.t[:, C:] == 0).all(), f'{what}: pad channels of x2'

    # ---- the inference call: the same x2, nothing else written
    oi = _attn_outputs(cuda, d)
    assert _call_attn(dd, oi, train=False) == 0
    assert torch.equal(_bits(oi.x2.t), _bits(o.x2.t)) and oi.x2.guards_intact(), f'{what}: inference x2'
    assert all(getattr(oi, k).untouched() for k in ATTN_SAVED)

    # ---- end to end against float64
    q64, _ = linear_ref(_padded(R.y, Cp), d.wq, d.bq)
    A64 = window_attention_ref(q64.view(N, H, W, -1), nH, shift, d.scale, d.table)
    y64, mag64 = linear_ref(A64.out.reshape(M, -1), d.wp, d.bp)
    ref, emag = x + d.srow * y64, x.abs() + d.srow.abs() * mag64
    fused, unfused = _e2e_ratio(o.x2.t, ref, emag, C), _e2e_ratio(_unfused_attn(dd), ref, emag, C)
    print(f'{what} x2 end to end: fused {fused:.3e}, unfused {unfused:.3e} of |x| + |s1| (sum|w a| + |b|)')
    assert fused <= 2 * E2E_UNFUSED_ATTN[case][0], (what, fused)


# ------------------------------------------------------------------------------------------------- MLP kernel

MLP_CASES = [  # N, HW, C, hidden, row_scale, data
    (3, 192, 60, 120, True, 'randn'),  # 4.5 tiles of 128 rows; tile 1 straddles images 0 / 1; three scales
    (1, 64, 180, 360, False, 'randn'),  # M below 128
    (1, 200, 96, 192, True, 'randn'),  # ragged M
    (2, 64, 192, 368, True, 'randn'),  # Cp and Hp limits; 23 hidden tiles
    (1, 128, 8, 8, False, 'randn'),  # one hidden tile, one K chunk
    (1, 128, 96, 128, False, 'randn'),  # exactly one hidden tile per wave
    (1, 128, 96, 136, False, 'randn'),  # 8.5 hidden tiles
    (2, 64, 100, 100, True, 'randn'),  # Hp 104: pad hidden columns
    (2, 128, 60, 120, True, 'offset'),  # rows with a mean offset
    (1, 128, 96, 192, False, 'tails'),  # pre-activations in the GELU tails, <= -5 and >= 5
]

# worst |out - float64| / (|x| + |s2| (sum|w h| + |b|)) per case: (unfused path, fused kernel), MI355X
E2E_UNFUSED_MLP = {
    (3, 192, 60, 120, True, 'randn'): (2.944e-03, 2.944e-03),
    (1, 64, 180, 360, False, 'randn'): (1.768e-03, 1.768e-03),
    (1, 200, 96, 192, True, 'randn'): (2.150e-03, 2.150e-03),
    (2, 64, 192, 368, True, 'randn'): (2.601e-03, 2.601e-03),
    (1, 128, 8, 8, False, 'randn'): (4.932e-03, 4.932e-03),
    (1, 128, 96, 128, False, 'randn'): (2.515e-03, 2.515e-03),
    (1, 128, 96, 136, False, 'randn'): (2.281e-03, 2.281e-03),
    (2, 64, 100, 100, True, 'randn'): (2.768e-03, 2.768e-03),
    (2, 128, 60, 120, True, 'offset'): (3.541e-03, 3.541e-03),
    (1, 128, 96, 192, False, 'tails'): (2.000e-03, 2.000e-03),
}


@functools.lru_cache(maxsize=None)
def _mlp_data(case):
    N, HW, C, hid, rsc, kind = case
    g = torch.Generator().manual_seed(100 * N + HW + C + hid)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    Cp, Hp, M = _cp(C), _cp(hid), N * HW
    d = SimpleNamespace(N=N, HW=HW, C=C, Cp=Cp, hid=hid, Hp=Hp, M=M)
    d.x = _padded(_x_rows(g, M, C, kind == 'offset'), Cp)
    d.gamma, d.beta = 1 + 0.1 * r(C), 0.1 * r(C)
    w1 = torch.zeros(Hp, Cp)
    w1[:hid, :C] = r(hid, C) * C**-0.5 * (2.0 if kind == 'tails' else 1.0)
    d.w1, d.b1 = w1.to(BF16), _padded(r(hid) * 0.05, Hp)
    w2 = torch.zeros(Cp, Hp)
    w2[:C, :hid] = r(C, hid) * hid**-0.5
    d.w2, d.b2 = w2.to(BF16), _padded(r(C) * 0.05, Cp)
    d.s2 = torch.tensor(SCALES[:N]) if rsc else None
    d.srow = (d.s2.double().repeat_interleave(HW) if rsc else torch.ones(M, dtype=torch.float64))[:, None]
    return d


def _mlp_outputs(device, M, Cp, Hp):
    return SimpleNamespace(out=_Out(device, BF16, M, Cp), ln=_Out(device, BF16, M, Cp), mean=_Out(device, torch.float32, M),
                           rstd=_Out(device, torch.float32, M), z=_Out(device, BF16, M, Hp), h=_Out(device, BF16, M, Hp))


MLP_SAVED = ('ln', 'mean', 'rstd', 'z', 'h')


def _call_mlp(dd, o, train=True, null=(), **geom):
    L = _lib()
    a = dict(N=dd.N, HW=dd.HW, C=dd.C, Cp=dd.Cp, Hp=dd.Hp)
    a.update(geom)
    p = {k: (L.ptr(getattr(o, k).t) if train and k not in null else None) for k in MLP_SAVED}
    rc = L.load().sr_swin_mlp_fused_fwd(L.ptr(dd.x), L.ptr(dd.gamma), L.ptr(dd.beta), a['C'], EPS, L.ptr(dd.w1), L.ptr(dd.b1),
                                        L.ptr(dd.w2), L.ptr(dd.b2), L.ptr(dd.s2), a['N'], a['HW'], a['Cp'], a['Hp'],
                                        L.ptr(o.out.t), p['ln'], p['mean'], p['rstd'], p['z'], p['h'], L.stream())
    torch.cuda.synchronize()
    return rc


def _unfused_mlp(dd):
    """(out, z, h) of the two-launch path on the same operands: LN-prologue lin kernel with GELU and the
    GELU' side output, then the fc2 linear with the scaled residual."""
    from basicsr4rs_amd.ops import swin as S
    N, H, W = dd.N, dd.HW // 8, 8
    fc1s, fc2s = S.plain_spec(dd.C, dd.hid), S.plain_spec(dd.hid, dd.C)
    x = dd.x.view(N, H, W, dd.Cp)
    z = torch.full((N, H, W, dd.Hp), NAN, device=x.device, dtype=BF16)
    uf = S.linear_ln_fwd(x, dd.gamma, dd.beta, dd.C, dd.w1, dd.b1, fc1s, N, H, W, act=S.GELU, aux=z)
    if uf is not None:
        h = uf[0]
    else:
        h = S.linear_fwd(S.layernorm(x, dd.gamma, dd.beta, dd.C)[0], dd.w1, dd.b1, fc1s, N, H, W, act=S.GELU, aux=z)
    out = S.linear_fwd(h, dd.w2, dd.b2, fc2s, N, H, W, res=x, beta=1.0, row_scale=dd.s2)
    torch.cuda.synchronize()
    return out.view(dd.M, dd.Cp), z.view(dd.M, dd.Hp), h.view(dd.M, dd.Hp)


@pytest.mark.parametrize('case', MLP_CASES, ids=str)
def test_swin_mlp_fused_stages(cuda, case):
    """Each stage of swin_mlp_block_fwd_kernel from its own stored input under the bounds of the module
    docstring; pad hidden columns bitwise the unfused lin kernel's; sentinels intact; the inference call
    bitwise the same out; out end to end against float64 within twice the unfused path's ratio."""
    N, HW, C, hid, rsc, kind = case
    d = _mlp_data(case)
    dd = _dev(d, cuda)
    Cp, Hp, M = d.Cp, d.Hp, d.M
    assert HW % 8 == 0
    what = f'mlp {case}'
    o = _mlp_outputs(cuda, M, Cp, Hp)
    assert _call_mlp(dd, o) == 0, what
    for k, v in vars(o).items():
        assert v.guards_intact(), f'{what}: wrote outside {k}'
    x = d.x.double()

    # ---- LayerNorm
    R = _check_ln(o, x, d.gamma, d.beta, C, Cp, what)

    # ---- z = GELU'(v), h = GELU(v), v = fc1 of the stored ln_out
    v, mag = linear_ref(o.ln.t.double().cpu(), d.w1, d.b1)
    if kind == 'tails':
        print(f'{what}: pre-activations in [{v.min().item():.2f}, {v.max().item():.2f}]')
        assert v.min().item() <= -5 and v.max().item() >= 5
    ev = (Cp + 2) * U * mag
    h64, z64, phi = gelu_ref(v)
    _check(o.h.t, h64, 1.13 * ev + 0.5 * v.abs() * ERF_ERR + 2 * U * h64.abs(), f'{what} h')
    _check(o.z.t, z64, 0.8 * ev + 0.5 * ERF_ERR + v.abs() * phi * U * (2 * v * v + 6) + U * z64.abs(), f'{what} z')
    uout, uz, uh = _unfused_mlp(dd)
    assert torch.equal(_bits(o.z.t[:, hid:]), _bits(uz[:, hid:])), f'{what}: pad hidden columns of z'
    assert torch.equal(_bits(o.h.t[:, hid:]), _bits(uh[:, hid:])), f'{what}: pad hidden columns of h'

    # ---- out from the stored h
    y, mag = linear_ref(o.h.t.double().cpu(), d.w2, d.b2)
    _check(o.out.t, x + d.srow * y, (Hp + 3) * U * d.srow.abs() * mag + U * x.abs(), f'{what} out')
    assert (o.out.t[:, C:] == 0).all(), f'{what}: pad channels of out'

    # ---- the inference call
    oi = _mlp_outputs(cuda, M, Cp, Hp)
    assert _call_mlp(dd, oi, train=False) == 0
    assert torch.equal(_bits(oi.out.t), _bits(o.out.t)) and oi.out.guards_intact(), f'{what}: inference out'
    assert all(getattr(oi, k).untouched() for k in MLP_SAVED)

    # ---- end to end against float64
    v64, _ = linear_ref(_padded(R.y, Cp), d.w1, d.b1)
    y64, mag64 = linear_ref(gelu_ref(v64)[0], d.w2, d.b2)
    ref, emag = x + d.srow * y64, x.abs() + d.srow.abs() * mag64
    fused, unfused = _e2e_ratio(o.out.t, ref, emag, C), _e2e_ratio(uout, ref, emag, C)
    print(f'{what} out end to end: fused {fused:.3e}, unfused {unfused:.3e} of |x| + |s2| (sum|w h| + |b|)')
    assert fused <= 2 * E2E_UNFUSED_MLP[case][0], (what, fused)


# -------------------------------------------------------------------------------------------------- refusals

ATTN_BASE = (1, 16, 16, 96, 3, 4, True, 'randn')
ATTN_REFUSED = {
    'Cp 200': dict(C=200, Cp=200),
    'nH 7': dict(nH=7),
    'H 12': dict(H=12),
    'shift 8': dict(shift=8),
    'shift -1': dict(shift=-1),
    **{f'{k} null': dict(null=(k, )) for k in ATTN_SAVED if k != 'qkv'},
}


@pytest.mark.parametrize('bad', ATTN_REFUSED, ids=str)
def test_swin_attn_fused_refusals(cuda, bad):
    """Geometry outside the kernel's envelope, or a training call (qkv given) with one saved-tensor pointer
    null: sr_swin_attn_fused_ok is 0 for the geometry, the forward returns SR_EINVAL and launches nothing --
    every NaN-filled output keeps its bits.  Operands are allocated for the geometry the call claims."""
    L = _lib()
    lib = L.load()
    kw = dict(ATTN_REFUSED[bad])
    null = kw.pop('null', ())
    d = _attn_data(ATTN_BASE)
    a = dict(N=d.N, H=d.H, W=d.W, shift=d.shift, nH=d.nH, C=d.C, Cp=d.Cp)
    a.update(kw)
    M = a['N'] * a['H'] * a['W']
    big = SimpleNamespace(**vars(d))
    big.x = torch.zeros(M, a['Cp']).to(BF16)
    big.gamma, big.beta = torch.ones(a['C']), torch.zeros(a['C'])
    big.wq, big.bq = torch.zeros(3 * a['nH'] * 32, a['Cp']).to(BF16), torch.zeros(3 * a['nH'] * 32)
    big.table = torch.zeros(225, a['nH'])
    big.wp, big.bp = torch.zeros(a['Cp'], a['nH'] * 32).to(BF16), torch.zeros(a['Cp'])
    dd = _dev(big, cuda)
    if kw and 'shift' not in kw:
        assert lib.sr_swin_attn_fused_ok(L.dtype_code(BF16), a['N'], a['H'], a['W'], 8, a['nH'], 32, 32, a['C'], a['Cp']) == 0
    else:
        assert lib.sr_swin_attn_fused_ok(L.dtype_code(BF16), a['N'], a['H'], a['W'], 8, a['nH'], 32, 32, a['C'], a['Cp']) == 1
    o = _attn_outputs(cuda, d, (a['N'], a['H'], a['W'], a['nH'], a['Cp']))
    assert _call_attn(dd, o, null=null, **kw) == SR_EINVAL
    assert all(v.untouched() for v in vars(o).values()), bad


MLP_BASE = (1, 128, 96, 192, True, 'randn')
MLP_REFUSED = {
    'Hp 376': dict(Hp=376),
    'Cp 200': dict(C=200, Cp=200),
    **{f'{k} null': dict(null=(k, )) for k in MLP_SAVED if k != 'z'},
}


@pytest.mark.parametrize('bad', MLP_REFUSED, ids=str)
def test_swin_mlp_fused_refusals(cuda, bad):
    """Hidden width or channels past the kernel's LDS tile, or a training call (z given) with one saved-tensor
    pointer null: sr_swin_mlp_fused_ok is 0 for the geometry, SR_EINVAL, nothing launched."""
    L = _lib()
    lib = L.load()
    kw = dict(MLP_REFUSED[bad])
    null = kw.pop('null', ())
    d = _mlp_data(MLP_BASE)
    a = dict(C=d.C, Cp=d.Cp, Hp=d.Hp)
    a.update(kw)
    big = SimpleNamespace(**vars(d))
    big.x = torch.zeros(d.M, a['Cp']).to(BF16)
    big.gamma, big.beta = torch.ones(a['C']), torch.zeros(a['C'])
    big.w1, big.b1 = torch.zeros(a['Hp'], a['Cp']).to(BF16), torch.zeros(a['Hp'])
    big.w2, big.b2 = torch.zeros(a['Cp'], a['Hp']).to(BF16), torch.zeros(a['Cp'])
    dd = _dev(big, cuda)
    assert lib.sr_swin_mlp_fused_ok(L.dtype_code(BF16), a['C'], a['Cp'], a['Hp']) == (0 if kw else 1)
    o = _mlp_outputs(cuda, d.M, a['Cp'], a['Hp'])
    assert _call_mlp(dd, o, null=null, **kw) == SR_EINVAL
    assert all(v.untouched() for v in vars(o).values()), bad
