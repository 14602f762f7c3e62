"""The ECB kernels (csrc/ecb.hip) against float64: the grouped collapse and its transpose against the formulas
of tests/_ecbsr_ref.py and their autograd, the conv epilogues (PReLU forward, tail store, gated input gradient,
slope gradient) against float64 conv + PReLU.

Collapse bounds: a sum of n fp32 products accumulated in any order is within n * 2^-24 * sum|products| of the
exact sum (plus the roundings of the few terms added around it: + 5), so every element is checked against
K * 2^-24 * sum|products| with the sum of absolute products computed here in float64 (the same formulas on the
absolute values of the operands).  Forward: K = 128 + 5 (mid_planes <= 128).  Transpose: K = 9 * 64 + 5, its
longest sum (dk0 over Cout x 9 taps)."""
import pytest
import torch
from torch.nn import functional as F

from tests import _ecbsr_ref as R

pytestmark = pytest.mark.gpu

BLOCKS = [(1, 16, False), (16, 16, True), (3, 8, False), (16, 48, False), (64, 64, True)]
U = 2.0**-24


def _blocks(cuda, act='prelu'):
    from basicsr4rs_amd.archs.ecbsr_arch import ECB
    torch.manual_seed(5)
    blks = [ECB(ci, co, 2.0, act_type=act, with_idt=idt) for ci, co, idt in BLOCKS]
    with torch.no_grad():
        for b in blks:
            for e in (b.conv1x1_sbx, b.conv1x1_sby, b.conv1x1_lpl):
                e.scale.mul_(300.0)
                e.bias.mul_(300.0)
    return [b.to(cuda) for b in blks]


def _parts(img, dtype):
    """An fp32 GEMM image in the layout the conv reads: itself, or for bf16 its [hi | lo] halves."""
    if dtype != torch.bfloat16:
        return img
    hi = img.to(dtype)
    return torch.cat([hi, (img - hi.float()).to(dtype)], dim=1)


def _sd(blk, fn=lambda t: t.double()):
    return {'b.' + k: fn(v.detach().cpu()) for k, v in blk.state_dict().items()}


def test_collapse_grouped_against_fp64(cuda):
    from basicsr4rs_amd.ops import ecb as E
    for dtype in (torch.float32, torch.bfloat16):
        blks = _blocks(cuda)
        st = E._State(blks, dtype, False)
        st.collapse()
        st.collapse()
        again = [t.clone() for t in st.rk + st.rb + st.wf + st.wd]
        st.collapse()
        assert all(torch.equal(a, b) for a, b in zip(again, st.rk + st.rb + st.wf + st.wd))  # bit-identical runs
        for l, (blk, (ci, co, idt)) in enumerate(zip(blks, BLOCKS)):
            rk, rb = R.collapse(_sd(blk), 'b.', idt)
            ak, ab = R.collapse(_sd(blk, lambda t: t.double().abs()), 'b.', idt)  # sum |products|
            ek = (st.rk[l].cpu().double() - rk).abs()
            eb = (st.rb[l].cpu().double() - rb).abs()
            print(f'{dtype} block {BLOCKS[l]}: RK err/bound {(ek / (133 * U * ak)).max():.3f} RB {(eb / (133 * U * ab)).max():.3f}')
            assert (ek <= 133 * U * ak).all() and (eb <= 133 * U * ab).all()
            cip, cop = (ci + 7) // 8 * 8, (co + 7) // 8 * 8
            # layout: wf[o][tap * Cin_p + ci], wd[ci][(8 - tap) * Cout_p + o] of RK in the image dtype; bf16 rows
            # carry a second half, the bf16 remainder RK - hi in the same order; padding exactly 0
            want = torch.zeros(cop, 9, cip, device=cuda)
            want[:co, :, :ci] = st.rk[l].reshape(co, ci, 9).permute(0, 2, 1)
            assert torch.equal(st.wf[l], _parts(want.reshape(cop, 9 * cip), dtype))
            wantd = torch.zeros(cip, 9, cop, device=cuda)
            wantd[:ci, :, :co] = st.rk[l].reshape(co, ci, 9).flip(2).permute(1, 2, 0)
            assert torch.equal(st.wd[l], _parts(wantd.reshape(cip, 9 * cop), dtype))
            if dtype == torch.bfloat16:  # hi + lo is RK to 2^-16 of each element (two bf16 roundings)
                both = st.wf[l].float().reshape(cop, 2, 9 * cip).sum(1)
                assert ((both - want.reshape(cop, 9 * cip)).abs() <= 2.0**-16 * want.reshape(cop, 9 * cip).abs()).all()
            wantb = torch.zeros(cop, device=cuda)
            wantb[:co] = st.rb[l]
            assert torch.equal(st.bg[l], wantb)
    # ECB.rep_params(): the same kernel through the module
    w, b = blks[1].rep_params()
    assert torch.equal(w, st.rk[1]) and torch.equal(b, st.rb[1]) and w.dtype == torch.float32


def test_collapse_transpose_against_fp64_autograd(cuda):
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import ecb as E
    blks = _blocks(cuda)
    st = E._State(blks, torch.float32, True)
    st.ensure()
    assert not st.direct
    g = torch.Generator().manual_seed(9)
    K = 9 * 64 + 5
    refs = []
    for l, (blk, (ci, co, idt)) in enumerate(zip(blks, BLOCKS)):
        drk, drb = torch.randn(co, ci, 3, 3, generator=g), torch.randn(co, generator=g)
        st.drk[l].copy_(drk)
        st.drb[l].copy_(drb)
        got = []
        for absolute in (False, True):
            fn = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
            sd = {k: (v.requires_grad_(True) if not k.endswith('mask') else v) for k, v in _sd(blk, fn).items()}
            rk, rb = R.collapse(sd, 'b.', idt)
            ((rk * fn(drk)).sum() + (rb * fn(drb)).sum()).backward()
            got.append(sd)
        refs.append(got)
    lib = _lib.load()
    for accumulate in (0, 1):
        if accumulate:  # accumulate mode adds to a non-zero buffer
            for stage in st.stage:
                for t in stage:
                    t.fill_(0.5)
        _lib.check(lib.sr_ecb_rep_bwd(_lib.ptr(st.table), len(blks), st.max_units, accumulate, _lib.stream()))
        first = [[t.clone() for t in stage] for stage in st.stage]
        if not accumulate:
            _lib.check(lib.sr_ecb_rep_bwd(_lib.ptr(st.table), len(blks), st.max_units, 0, _lib.stream()))
            assert all(torch.equal(a, b) for s0, s1 in zip(first, st.stage) for a, b in zip(s0, s1))
        for l, blk in enumerate(blks):
            names = [n for n, p in blk.named_parameters() if p.requires_grad]
            by_id = {id(p): n for n, p in blk.named_parameters()}
            for p, got in zip(E.block_params(blk), first[l]):
                n = 'b.' + by_id[id(p)]
                if n.endswith('act.weight'):
                    continue  # the slope gradient comes from the conv kernels
                ref, bound = refs[l][0][n].grad, K * U * refs[l][1][n].grad
                err = (got.cpu().double() - 0.5 * accumulate - ref).abs()
                if accumulate:
                    bound = bound + 2 * U * (0.5 + ref.abs())
                edge_b0 = n.endswith('.b0') and 'conv1x1_3x3' not in n
                if edge_b0:  # exact value 0 (the mask taps sum to 0)
                    pre = n[:-2]
                    sc = blk.state_dict()[pre[2:] + 'scale'].reshape(-1).cpu().double().abs()
                    dbias = st.drb[l].cpu().double().abs()
                    assert ref.abs().max() == 0 and (err <= 1e-5 * sc * dbias + (2 * U * 0.5 if accumulate else 0)).all(), n
                else:
                    assert (err <= bound).all(), (BLOCKS[l], n, (err / bound).max().item())
            assert len(names) == len(E.block_params(blk))


MAPS = [(2, 2, 3, 8, 16), (1, 1, 1, 8, 8), (2, 37, 70, 16, 16)]


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _case(shape, seed):
    N, H, W, ci, co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci**0.5)
    b = torch.randn(co, generator=g) * 0.1
    a = torch.linspace(-0.3, 0.4, co)
    a[1] = 0.0
    return x, w, b, a


def _images(w, b, dtype, cuda):
    co, ci = w.shape[:2]
    cip, cop = (ci + 7) // 8 * 8, (co + 7) // 8 * 8
    wf = torch.zeros(cop, 9, cip)
    wf[:co, :, :ci] = w.reshape(co, ci, 9).permute(0, 2, 1)
    wd = torch.zeros(cip, 9, cop)
    wd[:ci, :, :co] = w.reshape(co, ci, 9).flip(2).permute(1, 2, 0)
    bg = torch.zeros(cop)
    bg[:co] = b
    return _parts(wf.reshape(cop, -1).to(cuda), dtype), _parts(wd.reshape(cip, -1).to(cuda), dtype), bg.to(cuda)


def _nhwc(t, dtype, cuda, cp=None):
    N, Cc, H, W = t.shape
    out = torch.zeros(N, H, W, cp or (Cc + 7) // 8 * 8)
    out[..., :Cc] = t.permute(0, 2, 3, 1)
    return out.to(cuda, dtype).contiguous()


@pytest.mark.parametrize('shape', MAPS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=('fp32', 'bf16'))
def test_conv_act_forward_and_gated_backward(cuda, shape, dtype):
    """z, y of the activated forward; dz and da of the gated input gradient, with negative, zero and positive
    slopes and some z exactly 0 (a bias-free layer on an input with zero pixels).  fp32: relative L2 <= 1e-4
    against float64 (test_hr_tail_chain_fp32_vs_fp64's figure).  bf16 (operands pre-rounded, so only the stored
    maps round): relative L2 <= 2^-8, one bf16 rounding of each stored value, + 1e-4."""
    from basicsr4rs_amd.ops import ecb as E
    N, H, W, ci, co = shape
    x, w, b, a = _case(shape, 11)
    bf = dtype == torch.bfloat16
    tol = 2.0**-8 + 1e-4 if bf else 1e-4
    if bf:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    x[:, :, 0, 0] = 0.0
    b[0] = 0.0
    if H * W == 1:
        b[2] = 0.0  # with the pixel zeroed, channels 0 and 2 have z == 0 exactly
    wf, wd, bg = _images(w, b, dtype, cuda)
    xs = _nhwc(x, dtype, cuda)
    slope = a.to(cuda)
    y, z = E.conv_act(xs, wf, bg, slope, wf.shape[0], co)
    y2, z2 = E.conv_act(xs, wf, bg, slope, wf.shape[0], co)
    assert torch.equal(y, y2) and torch.equal(z, z2)
    zr = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    yr = F.prelu(zr, a.double())
    zg, yg = z.float().cpu().double(), y.float().cpu().double()
    assert (zg[..., co:] == 0).all() and (yg[..., co:] == 0).all()
    ez, ey = _rel(zg[..., :co].permute(0, 3, 1, 2), zr), _rel(yg[..., :co].permute(0, 3, 1, 2), yr)
    print(f'{shape} {dtype}: z rel L2 {ez:.3e}, y rel L2 {ey:.3e}')
    assert ez <= tol and ey <= tol
    if H * W == 1:
        assert zg[0, 0, 0, 0] == 0 and zg[0, 0, 0, 2] == 0
    # linear / ReLU epilogues: same kernel, slope none / 0, no z
    yl, zl = E.conv_act(xs, wf, bg, None, wf.shape[0], co)
    assert zl is None and torch.equal(yl, z)
    yre, _ = E.conv_act(xs, wf, bg, torch.zeros(co, device=cuda), wf.shape[0], co, want_z=False)
    assert torch.equal(yre, torch.relu(z))

    # gated input gradient of a consumer conv (co -> ci channels reversed: this layer as the consumer, a producer
    # with `ci` channels whose stored z is zp)
    g = torch.Generator().manual_seed(12)
    dzc = torch.randn(N, co, H, W, generator=g)
    zp = torch.randn(N, ci, H, W, generator=g)
    zp[:, :, 0, 0] = 0.0
    ap = torch.linspace(-0.3, 0.4, ci)
    ap[1] = 0.0
    if bf:
        dzc, zp = dzc.bfloat16().float(), zp.bfloat16().float()
    nb = E.conv_blocks(dtype, N, H, W, 8, 8, 8)
    parts = torch.full((nb, 64), float('nan'), device=cuda)
    dzs, zps = _nhwc(dzc, dtype, cuda), _nhwc(zp, dtype, cuda)
    dz = E.conv_dgrad(dzs, wd, zps, ap.to(cuda), wd.shape[0], ci, parts)
    parts2 = torch.empty_like(parts)
    dzb = E.conv_dgrad(dzs, wd, zps, ap.to(cuda), wd.shape[0], ci, parts2)
    assert torch.equal(dz, dzb) and torch.equal(parts[:, :ci], parts2[:, :ci])
    zp64 = zp.double().requires_grad_(True)
    ap64 = ap.double().requires_grad_(True)
    out = F.conv2d(F.prelu(zp64, ap64), w.double(), None, padding=1)
    (out * dzc.double()).sum().backward()
    dg = dz.float().cpu().double()
    assert (dg[..., ci:] == 0).all()
    ed = _rel(dg[..., :ci].permute(0, 3, 1, 2), zp64.grad)
    da = parts[:, :ci].cpu().double().sum(0)
    eda = _rel(da, ap64.grad)
    print(f'{shape} {dtype}: dz rel L2 {ed:.3e}, da rel L2 {eda:.3e} over {nb} blocks')
    assert ed <= tol and eda <= (1e-4 if not bf else tol)
    # at z == 0 the gate is the slope (torch's), zero slope included
    gfull = F.conv_transpose2d(dzc.double(), w.double(), padding=1)
    assert torch.allclose(dg[:, 0, 0, :ci], gfull[:, :, 0, 0] * ap.double(), rtol=4 * tol, atol=4 * tol * gfull.abs().max().item())


@pytest.mark.parametrize('s,cimg', [(2, 3), (3, 1), (4, 1), (2, 1)])
def test_conv_tail_store(cuda, s, cimg):
    """The tail: conv + bias + shortcut through the PixelShuffle, element for element against pixel_shuffle of the
    engine's own linear conv output (exact: the same accumulators), and against float64 at relative L2 1e-4.
    cimg 1 with several output channels is the reference's broadcast of a one-channel input."""
    from basicsr4rs_amd.ops import ecb as E
    cout_img = 3 if (s, cimg) == (2, 1) else cimg
    N, H, W, ci = 2, 5, 19, 16
    co = cout_img * s * s
    x, w, b, _ = _case((N, H, W, ci, co), 21)
    img = torch.rand(N, cimg, H, W, generator=torch.Generator().manual_seed(22))
    wf, _, bg = _images(w, b, torch.float32, cuda)
    xs = _nhwc(x, torch.float32, cuda)
    out = E.conv_tail(xs, wf, bg, img.to(cuda), wf.shape[0], co, s)
    out2 = E.conv_tail(xs, wf, bg, img.to(cuda), wf.shape[0], co, s)
    assert torch.equal(out, out2) and tuple(out.shape) == (N, cout_img, H * s, W * s) and out.dtype == torch.float32
    lin, _ = E.conv_act(xs, wf, bg, None, wf.shape[0], co)
    short = torch.repeat_interleave(img, s * s, dim=1) if cimg > 1 else img
    want = F.pixel_shuffle(lin[..., :co].permute(0, 3, 1, 2) + short.to(cuda), s)
    assert torch.equal(out, want)
    ref = F.pixel_shuffle(F.conv2d(x.double(), w.double(), b.double(), padding=1) + short.double(), s)
    assert _rel(out.cpu().double(), ref) <= 1e-4


def test_tail_bwd_is_pixel_unshuffle(cuda):
    from basicsr4rs_amd.ops import ecb as E
    for s, c in ((2, 3), (3, 1), (4, 1)):
        d = torch.randn(2, c, 5 * s, 7 * s, device=cuda)
        for dtype in (torch.float32, torch.bfloat16):
            cp = (c * s * s + 7) // 8 * 8
            dz = E.tail_bwd(d, s, cp, dtype)
            want = F.pixel_unshuffle(d, s).permute(0, 2, 3, 1).to(dtype)
            assert torch.equal(dz[..., :c * s * s], want) and (dz[..., c * s * s:] == 0).all()


def test_da_reduce_grouped(cuda):
    """The slope gradients of all layers in one launch, from [layers][blocks][64] partials; two runs are identical."""
    from basicsr4rs_amd.ops import ecb as E
    blks = _blocks(cuda)[:2]
    st = E._State(blks, torch.float32, True)
    st.ensure()
    nb = 37
    parts = torch.randn(2, nb, 64, device=cuda)
    E.da_reduce(st, 2, parts, nb)
    for l in range(2):
        got = st.stage[l][18].cpu().double()
        ref = parts[l, :, :16].cpu().double().sum(0)
        assert (got - ref).abs().max().item() <= nb * U * parts[l].abs().sum(0).max().item()
    a = [st.stage[l][18].clone() for l in range(2)]
    E.da_reduce(st, 2, parts, nb)
    assert all(torch.equal(a[l], st.stage[l][18]) for l in range(2))
