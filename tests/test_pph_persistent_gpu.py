"""Persistent multi-tile form of conv3x3_fwd_pph_kernel (W 64, Cout 256, bf16): one K loop across a
block's run of tiles, the accumulators staged through the free ring slots.  Bitwise against the
one-tile form (variant 80), against fp64, and the fallbacks of the dispatch."""
import pytest
import torch
import torch.nn.functional as F

from basicsr4rs_amd import _lib
from basicsr4rs_amd.ops import conv as C

pytestmark = pytest.mark.gpu

W = 64
ONE_TILE = 80  # sr_conv3x3_set_variant: the one-tile form for the persistent form's arguments

# (N, H, Cin, Cout, G).  Ring: 11 slots, 6 rows per chunk; after a tile the staging slots are
# (6 * chunks_done + 6 + k) mod 11, k = 0..3, so they wrap past slot 10 when 6 * chunks_done mod 11 is in
# 2..4.  Per block the chunks done after its tiles 1, 2, ... are nchunk, 2 nchunk, ...:
#   nchunk 4 (Cin 256): 24 mod 11 = 2 (wraps), 48 mod 11 = 4 (wraps)
#   nchunk 1 (Cin 64):  6, 1, 7 (runs of three: no wrap, the slots past 10 shift as a whole)
#   nchunk 2 (Cin 128): 1, 2 (wraps), 3 (wraps)
#   nchunk 8 (Cin 512): 48 mod 11 = 4 (wraps), 96 mod 11 = 8
# and the last case is the slot formula's wrap at EVERY boundary of a run of three: nchunk 6 (Cin 384):
# 36 mod 11 = 3, 72 mod 11 = 6 -> the first boundary wraps with the run starting in the middle (slots 9, 10, 0, 1)
CASES = [
    (1, 12, 256, 256, 2),   # 3 tiles, runs of 2 and 1
    (2, 4, 256, 256, 1),    # the tile boundary is an image boundary: the top halo row is padding
    (3, 8, 64, 256, 2),     # nchunk 1: rows and B tiles roll over in the only chunk; 6 tiles
    (1, 20, 128, 256, 2),   # 5 tiles as 3 + 2, nchunk 2
    (1, 8, 512, 256, 1),    # nchunk 8: the ring counter wraps several times before the boundary
    (1, 12, 384, 256, 1),   # staging slots 9, 10, 0, 1 at the first boundary (see above)
]
EPIS = ['bias', 'relu', 'res_beta', 'gate']


def _bf(t):
    return t.to(torch.bfloat16).float()


class _Operands:
    """Operands of one case (made once per case, left unchanged)."""

    def __init__(self, cuda, case, sliced):
        N, H, cin, cout, _ = case
        torch.manual_seed(11)
        dt = torch.bfloat16
        self.case, self.sliced = case, sliced
        self.ldx = cin + 16 if sliced else cin
        self.xcoff = 8 if sliced else 0
        self.xw = torch.randn(N, H, W, self.ldx, device=cuda).to(dt)
        self.wt = torch.randn(cout, cin, 3, 3, device=cuda) * 0.05
        self.bias = torch.randn(cout, device=cuda)
        self.wf, _, self.bg = C.prepared(torch.nn.Parameter(self.wt), torch.nn.Parameter(self.bias),
                                         C.ConvSpec(cin, cout), dt)
        self.res = torch.randn(N, H, W, cout, device=cuda).to(dt)
        self.gate = torch.randn(N, H, W, cout, device=cuda).to(dt)

    def kwargs(self, epi):
        kw = dict(ldx=self.ldx, xcoff=self.xcoff)
        if epi == 'relu':
            kw.update(act=_lib.ACT_RELU)
        elif epi == 'res_beta':
            kw.update(res=self.res, beta=0.5, alpha=0.25)
        elif epi == 'gate':
            kw.update(gate=self.gate, gate_mode=0, gate_slope=0.0)
        return kw

    def run(self, epi, **extra):
        N, H, cin, cout, _ = self.case
        y = torch.full((N, H, W, cout), float('nan'), device=self.xw.device, dtype=torch.bfloat16)
        bg = None if epi == 'gate' else self.bg  # the dgrad has no bias
        kw = self.kwargs(epi)
        kw.update(extra)
        out = C.conv_fwd_raw(self.xw, self.wf, bg, y, N, H, W, cin, cout, cout, **kw)
        return y, out

    def ref64(self, epi):
        N, H, cin, cout, _ = self.case
        x = self.xw[..., self.xcoff:self.xcoff + cin].permute(0, 3, 1, 2).double().cpu()
        b = None if epi == 'gate' else self.bias.double().cpu()
        ref = F.conv2d(x, _bf(self.wt.cpu()).double(), b, padding=1)
        if epi == 'relu':
            ref = F.relu(ref)
        elif epi == 'res_beta':
            ref = 0.25 * ref + 0.5 * self.res.permute(0, 3, 1, 2).double().cpu()
        elif epi == 'gate':
            ref = ref * (self.gate.permute(0, 3, 1, 2).double().cpu() > 0)
        return ref


_OPS = {}


def _operands(cuda, case):
    if case not in _OPS:
        _OPS[case] = _Operands(cuda, case, sliced=case == CASES[3])  # one case reads a channel slice
    return _OPS[case]


def _assert_pph(ops):
    N, H, cin, cout, _ = ops.case
    d = C._desc(torch.bfloat16, N, H, W, cin, ops.ldx, cout, cout, cout)
    assert _lib.load().sr_conv3x3_fwd_kernel_name(d) == b'conv3x3_fwd_pph_kernel'


def _old_form(ops, epi, **extra):
    lib = _lib.load()
    _lib.check(lib.sr_conv3x3_set_variant(ONE_TILE))
    try:
        return ops.run(epi, **extra)
    finally:
        _lib.check(lib.sr_conv3x3_set_variant(0))


@pytest.mark.parametrize('epi', EPIS)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_persistent_bitwise_vs_one_tile(cuda, case, epi):
    """Default (persistent) form with the grid knob forcing several tiles per block == the one-tile
    form, bitwise, for each body epilogue; two calls of each configuration agree too."""
    ops = _operands(cuda, case)
    _assert_pph(ops)
    with _lib.knob('SR_PPH_GRID', case[4]):
        y1, _ = ops.run(epi)
        y2, _ = ops.run(epi)
    o1, _ = _old_form(ops, epi)
    o2, _ = _old_form(ops, epi)
    torch.cuda.synchronize()
    assert not torch.isnan(y1.float()).any() and not torch.isnan(o1.float()).any()
    assert torch.equal(o1, o2)
    assert torch.equal(y1, y2)
    assert torch.equal(y1, o1), (y1.float() - o1.float()).abs().max().item()


@pytest.mark.parametrize('epi', ['res_beta', 'gate'])
@pytest.mark.parametrize('case', [CASES[0], CASES[3]], ids=lambda c: 'x'.join(str(v) for v in c))
def test_persistent_vs_fp64(cuda, case, epi):
    """Against F.conv2d in float64 on the same bf16 operands (the bound of test_fwd_pph_vs_fp64)."""
    ops = _operands(cuda, case)
    _assert_pph(ops)
    with _lib.knob('SR_PPH_GRID', case[4]):
        y, _ = ops.run(epi)
    torch.cuda.synchronize()
    ref = ops.ref64(epi)
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert (got - ref).abs().max().item() <= 2e-2 * max(1.0, ref.abs().max().item())


def test_fallback_tiles_le_grid(cuda):
    """Knob unset and fewer tiles than CUs: the one-tile form runs; equal to variant 80 bitwise."""
    ops = _operands(cuda, CASES[0])
    _assert_pph(ops)
    for epi in ('res_beta', 'gate'):
        y, _ = ops.run(epi)
        o, _ = _old_form(ops, epi)
        assert not torch.isnan(y.float()).any()
        assert torch.equal(y, o)


def test_fallback_colsum(cuda):
    """Fused channel sums keep the one-tile kernel also when the knob asks for several tiles per block."""
    ops = _operands(cuda, CASES[0])
    with _lib.knob('SR_PPH_GRID', 2):
        y, (_, parts) = ops.run('res_beta', colsum=True)
    o, (_, oparts) = _old_form(ops, 'res_beta', colsum=True)
    assert not torch.isnan(y.float()).any()
    assert torch.equal(y, o) and torch.equal(parts, oparts)


@pytest.mark.parametrize('kind', ['out_ps', 'w128'])
def test_fallback_other_callers(cuda, kind):
    """The upsample conv (pixel-shuffled output) and W 128 keep their kernels under the grid knob."""
    torch.manual_seed(3)
    dt = torch.bfloat16
    lib = _lib.load()
    if kind == 'out_ps':
        N, H, Wd, cin, cout, ps = 1, 12, 64, 64, 256, 2
    else:
        N, H, Wd, cin, cout, ps = 1, 6, 128, 64, 256, 0
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).to(cuda)
    spec = C.ConvSpec(cin, cout, out_ps=ps)
    wf, _, bg = C.prepared(conv.weight, conv.bias, spec, dt)
    x = torch.randn(N, H, Wd, cin, device=cuda).to(dt)
    yshape = C._out_shape(spec, N, H, Wd)
    assert lib.sr_conv3x3_fwd_kernel_name(C._desc(dt, N, H, Wd, cin, cin, cout, cout, cout, out_ps=ps)) == \
        b'conv3x3_fwd_pph_kernel'

    def run():
        y = torch.full(yshape, float('nan'), device=cuda, dtype=dt)
        C.conv_fwd_raw(x, wf, bg, y, N, H, Wd, cin, cout, cout, out_ps=ps)
        return y

    with _lib.knob('SR_PPH_GRID', 2):
        y = run()
    _lib.check(lib.sr_conv3x3_set_variant(ONE_TILE))
    try:
        o = run()
    finally:
        _lib.check(lib.sr_conv3x3_set_variant(0))
    assert not torch.isnan(y.float()).any()
    assert torch.equal(y, o)
