"""Exact-lattice tests of the deformable conv kernels (csrc/dcn_cols.hip, dcn_fwd_fused.hip, dcn_bwd_win.hip; entry
points and geometry in csrc/dcn.hip): bit for bit against the float64 oracle.

Offsets on a quarter-pixel lattice, masks in {0, 1/2, 1} and small-integer maps make every coordinate, bilinear
weight, column value, gradient term and fixed-point scatter contribution exactly representable (tests/_dcn_exact.py
states why, stage by stage; tests/test_dcn_exact_host.py checks it for every case on the host and shows that single
defects are rejected).  So the kernels must reproduce oracle/ops.py exactly: fp32 outputs as they are, y of the
bf16 paths after one round-to-nearest-even.  One dropped corner at a tile seam, one sample on the wrong side of
h > -1, one lost scatter contribution is a hard mismatch, and assert_bits reports its pattern.

The offset families put samples exactly on -1, on H, on the integers, into (-1, 0) and [H - 1, H), inside,
across and beyond the LDS windows of every tile, all on one cell (the fixed-point image's worst case) and far
outside the image (an image that scatters nothing beside one that does).

Kernels and the cases that reach them (bf16 autocast unless noted): dcn_fwd_win F1-F5, F7 (op); dcn_fwd_mfma F1-F5,
F7 (sr_dcn_fwd_fused, x_blocked 1); dcn_im2col<bf16, 8> F6 (op) and F1-F7 (entry point), <float, 4> / <float, 1> G*
(fp32 op); dcn_coord_dy8 and dcn_gradx_dy8<32 | 64, NCHW> F1, F2, F3, F5, F5k5, F7 (op), <32 | 64, NHWC> the same
(sr_dcn_bwd_fused); dcn_coord_win and dcn_grad_x<bf16, 8> F4, F6 (op) and F1-F7 (sr_dcn_col2im); dcn_coord_grad and
dcn_grad_x<float> G* and F1 converge (fp32 op).  F7 is the case whose scatter-tile LDS images end inside the map on
all four sides (28 x 36: the seams of a large map)."""
import contextlib

import pytest
import torch

from basicsr4rs_amd import _lib
from basicsr4rs_amd.ops import dcn as D

from . import _dcn_exact as X
from . import _exact as E
from ._fp64 import _rne_bf16

pytestmark = pytest.mark.gpu
NAN = float('nan')
BF = torch.bfloat16


def _run_op(b, dev, bf16, dy=None):
    """The public op on the case's operands, forward and backward: (out, {name: grad})."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = b.case
    t = {n: (None if v is None else v.to(dev, torch.float32).requires_grad_())
         for n, v in (('x', b.x), ('offset', b.offset), ('mask', b.mask), ('weight', b.weight), ('bias', b.bias))}
    with torch.autocast('cuda', dtype=BF) if bf16 else contextlib.nullcontext():
        if mod:
            out = D.modulated_deform_conv(t['x'], t['offset'], t['mask'], t['weight'], t['bias'], s, p, d, groups, dg)
        else:
            out = D.deform_conv(t['x'], t['offset'], t['weight'], s, p, d, groups, dg)
    out.backward((b.dy if dy is None else dy).to(dev, torch.float32))
    return out.detach(), {n: v.grad for n, v in t.items() if v is not None}


def _assert_op(b, out, grads, bf16, images=None):
    """out and the five gradients against the oracle, bit for bit (``images``: only these images of the per-image
    outputs)."""
    sel = (lambda t: t) if images is None else (lambda t: t[images])
    assert out.dtype == torch.float32
    E.assert_bits(sel(out), sel(_rne_bf16(b.y) if bf16 else b.y), f'{b.cid}/{b.family} y', axes='nchw')
    E.assert_bits(sel(grads['x']), sel(b.gx), f'{b.cid}/{b.family} grad x', axes='nchw')
    E.assert_bits(sel(grads['offset']), sel(b.goff), f'{b.cid}/{b.family} grad offset', axes='nchw')
    if b.gmask is not None:
        E.assert_bits(sel(grads['mask']), sel(b.gmask), f'{b.cid}/{b.family} grad mask', axes='nchw')
    if images is None:
        E.assert_bits(grads['weight'], b.gw, f'{b.cid}/{b.family} grad weight', axes='oikl')
        if b.gb is not None:
            E.assert_bits(grads['bias'], b.gb, f'{b.cid}/{b.family} grad bias', axes='c')


def _geom(b, dev):
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = b.case
    return D._Geom(torch.empty(N, C, H, W, device=dev), torch.empty(Cout, C // groups, k, k, device=dev), s, p, d,
                   groups, dg)


def _assert_paths(b, dev):
    g = _geom(b, dev)
    assert (D.fused_ok(g, BF), D.bwd_fused_ok(g, BF)) == X.FUSED[b.cid], b.cid


def test_case_tables_agree():
    from .test_ops_gpu import DCN_CASES
    assert [X.CASES[c] for c in X.G_IDS] == DCN_CASES


F_PLAN = [(c, f) for c, f in X.PLAN if c in X.F_IDS and f in ('lattice', 'integer', 'zero', 'edges', 'converge')]


@pytest.mark.parametrize('r', [0, 2], ids=['R0', 'R2'])
@pytest.mark.parametrize('fx', [32, 64], ids=['i32', 'i64'])
@pytest.mark.parametrize('cid,family', F_PLAN, ids=[f'{c}-{f}' for c, f in F_PLAN])
def test_op_bf16_exact(cuda, knob, cid, family, fx, r):
    """The public op under bf16 autocast: out and all five gradients equal the oracle.  SR_DCN_GX_FX selects the
    int32 / int64 scatter image (both exact now, not within 7e-5 of each other); SR_DCN_R moves the forward window's
    edges.  The zero family is the route ops/dcn.py::_offset_conv takes for a non-standard geometry."""
    b = X.build(cid, family)
    b.check()
    knob('SR_DCN_GX_FX', fx)
    knob('SR_DCN_R', r)
    _assert_paths(b, cuda)
    out, grads = _run_op(b, cuda, True)
    _assert_op(b, out, grads, True)


G_PLAN = [(c, f) for c in X.G_IDS for f in ('lattice', 'edges', 'integer')] + [('F1', 'converge')]


@pytest.mark.parametrize('cid,family', G_PLAN, ids=[f'{c}-{f}' for c, f in G_PLAN])
def test_op_fp32_exact(cuda, cid, family):
    """The public op in fp32: the generic kernels (dcn_im2col, dcn_coord_grad, dcn_grad_x with the int64 image) at
    vector and scalar widths, groups 2, 1 x 1, odd channels; F1 converge puts 6480 samples on one cell."""
    b = X.build(cid, family)
    b.check()
    out, grads = _run_op(b, cuda, False)
    _assert_op(b, out, grads, False)


def _rows(b, t5, g):
    """[N, C, K, Ho, Wo] float64 -> the column rows [N, Ho, Wo, L] (column (group K + tap) cgp + ci, padding 0)."""
    N = b.case[0]
    r = t5.reshape(N, g.G, g.cg, g.K, g.Ho, g.Wo).permute(0, 4, 5, 1, 3, 2)  # [N, Ho, Wo, G, K, cg]
    out = torch.zeros(N, g.Ho, g.Wo, g.G, g.K, g.cgp, dtype=torch.float64)
    out[..., :g.cg] = r
    return out.reshape(N, g.Ho, g.Wo, g.L)


E_PLAN = [(c, f) for c in X.F_IDS for f in ('lattice', 'edges')]


@pytest.mark.parametrize('cid,family', E_PLAN, ids=[f'{c}-{f}' for c, f in E_PLAN])
def test_entry_points_exact(cuda, cid, family):
    """The C entry points on NaN-filled outputs: sr_dcn_im2col (bf16 and fp32) and the cols of sr_dcn_fwd_fused for
    x_blocked 0 (dcn_fwd_win) and 1 (dcn_fwd_mfma, which the op never reaches) equal the oracle's columns; y of both;
    sr_dcn_col2im on the float64 dcols stored as bf16; sr_dcn_bwd_fused in its NHWC form into a zeroed map."""
    b = X.build(cid, family)
    b.check()
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = b.case
    lib = _lib.load()
    g = _geom(b, cuda)
    what = f'{cid}/{family}'
    x = b.x.to(cuda, torch.float32)
    off = b.offset.to(cuda).contiguous()
    msk = b.mask.to(cuda).contiguous() if mod else None
    wt = b.weight.to(cuda, torch.float32)
    bias = b.bias.to(cuda, torch.float32) if mod else None
    cols_ref = _rows(b, b.cols, g)
    for dt in (BF, torch.float32):
        xh = D.C.nchw_to_nhwc(x, g.Cp, dt)
        cols = torch.full((N, g.Ho, g.Wo, g.L), NAN, device=cuda, dtype=dt)
        _lib.check(lib.sr_dcn_im2col(g.desc(dt), _lib.ptr(xh), _lib.ptr(off), _lib.ptr(msk), _lib.ptr(cols),
                                     _lib.stream()))
        E.assert_bits(cols, cols_ref, f'{what} sr_dcn_im2col', axes='nyxc')
    xh = D.C.nchw_to_nhwc(x, g.Cp, BF)
    wf, wd, bg = D._prepared(wt, bias, g, D._spec(g), BF)[0]
    desc = g.desc(BF)
    if X.FUSED[cid][0]:
        xb = D.C.nchw_to_nhwc(x.reshape(N * 8, 8, H, W), 8, BF)
        for blocked, xin in ((0, xh), (1, xb)):
            y = torch.full((N, Cout, g.Ho, g.Wo), NAN, device=cuda)
            cols = torch.full((N, g.Ho, g.Wo, g.L), NAN, device=cuda, dtype=BF)
            _lib.check(lib.sr_dcn_fwd_fused(desc, _lib.ptr(xin), blocked, _lib.ptr(off), _lib.ptr(msk), _lib.ptr(wf),
                                            wf.shape[1], wf.shape[0], Cout, _lib.ptr(bg if mod else None), _lib.ptr(y),
                                            _lib.ptr(cols), _lib.stream()))
            E.assert_bits(cols, cols_ref, f'{what} sr_dcn_fwd_fused cols, x_blocked {blocked}', axes='nyxc')
            E.assert_bits(y, _rne_bf16(b.y), f'{what} sr_dcn_fwd_fused y, x_blocked {blocked}', axes='nchw')
    wsb = lib.sr_dcn_col2im_workspace(desc)
    dcols = E.store(_rows(b, b.dcols, g), BF).to(cuda)
    dyh = D.C.nchw_to_nhwc(b.dy.to(cuda, torch.float32), g.ldy, BF)
    gx_ref = E.nhwc(b.gx)
    for fused, fx in ((False, 32), (True, 32), (True, 64)):  # fx: the int32 (R 4) / int64 (R 2) scatter image
        if fused and not X.FUSED[cid][1]:
            continue
        gx = torch.zeros(N, H, W, g.Cp, device=cuda)
        goff = torch.full_like(off, NAN)
        gm = torch.full_like(msk, NAN) if mod else None
        ws = torch.empty(wsb // 4 + 1, device=cuda, dtype=torch.int32)
        if fused:
            with _lib.knob('SR_DCN_GX_FX', fx):
                _lib.check(lib.sr_dcn_bwd_fused(desc, _lib.ptr(dyh), g.ldy, _lib.ptr(wd), wd.shape[1], g.cout_gp,
                                                _lib.ptr(xh), _lib.ptr(off), _lib.ptr(msk), _lib.ptr(gx), 0,
                                                _lib.ptr(goff), _lib.ptr(gm), _lib.ptr(ws), wsb, _lib.stream()))
        else:
            _lib.check(lib.sr_dcn_col2im(desc, _lib.ptr(dcols), _lib.ptr(xh), _lib.ptr(off), _lib.ptr(msk),
                                         _lib.ptr(gx), _lib.ptr(goff), _lib.ptr(gm), _lib.ptr(ws), wsb, _lib.stream()))
        name = f'sr_dcn_bwd_fused (NHWC, i{fx})' if fused else 'sr_dcn_col2im'
        E.assert_bits(gx[..., :C], gx_ref, f'{what} {name} grad x', axes='nyxc')
        E.assert_bits(goff, b.goff, f'{what} {name} grad offset', axes='nchw')
        if mod:
            E.assert_bits(gm, b.gmask, f'{what} {name} grad mask', axes='nchw')


@pytest.mark.parametrize('fx', [32, 64], ids=['i32', 'i64'])
@pytest.mark.parametrize('cid', ['F1', 'F5k5', 'F5'], ids=['9taps', '25taps', '49taps'])
def test_same_sign_convergence(cuda, knob, cid, fx):
    """Every sample of image 0 on one cell, all contributions of one sign, max |mask * dcols| = Cout - 1 just below a
    power of two: the least headroom the fixed-point scatter image can have.  The cell must hold dcols Ho Wo K (the
    closed form) and everything must equal the oracle.

    With the scale fixed at 2^(18 - ex) the int32 image of a 16 x 16 tile sums 256 pixels x 49 taps x 15 x 2^14 =
    3.08e9 > 2^31 at 49 taps and wrapped: the cell held 2456 instead of 264600 (one 2^32 / 2^14 = 262144 short) on
    the MI355X, while 9 and 25 taps (1.57e9) and the int64 image were exact.  dcn_gradx_dy8_kernel now takes
    30 - ceil(log2(256 K)) bits per contribution (18 up to 16 taps), see gx_fx_bits in csrc/dcn.hip."""
    b = X.build(cid, 'same_sign')
    b.check()
    knob('SR_DCN_GX_FX', fx)
    _assert_paths(b, cuda)
    out, grads = _run_op(b, cuda, True)
    cell = grads['x'][0].double().cpu()
    H, W = b.case[2:4]
    print(f'{cid} i{fx}: cell holds {cell[:, H // 2, W // 2 + 1].unique().tolist()}, closed form '
          f'{float(X.same_sign_cell(b).max())}')
    E.assert_bits(grads['x'][0], X.same_sign_cell(b), f'{cid} same_sign cell, closed form', axes='cyx')
    _assert_op(b, out, grads, True)


@pytest.mark.parametrize('fx', [32, 64], ids=['i32', 'i64'])
@pytest.mark.parametrize('cid,family', [('F1', 'far'), ('F1', 'far_m0'), ('F4', 'far')])
def test_far_image_beside_a_real_one(cuda, knob, cid, family, fx):
    """Image 1's samples all lie far outside (finite offsets up to 3e9): y == bias exactly, grad offset, grad mask and
    grad x exactly zero with no NaN (the scatter kernel returns early for it; the coordinate kernel zeroes grad x),
    while image 0 beside it stays bit-exact."""
    b = X.build(cid, family)
    b.check()
    knob('SR_DCN_GX_FX', fx)
    out, grads = _run_op(b, cuda, True)
    want = torch.zeros_like(out[1]) if b.bias is None else b.bias.to(cuda, torch.float32).view(-1, 1, 1).expand_as(out[1])
    assert torch.equal(out[1], want)
    for n in ('x', 'offset') + (('mask',) if b.mask is not None else ()):
        assert torch.equal(grads[n][1], torch.zeros_like(grads[n][1])), n
    _assert_op(b, out, grads, True)


def test_non_finite_gradient(cuda):
    """One +inf in image 0's dy: its grad x goes through the direct fp32 atomics and keeps a non-finite element (a
    float -> int conversion would have made it finite); image 1 keeps its bits."""
    b = X.build('F1', 'lattice')
    dy = b.dy.clone()
    dy[0, 5, 7, 11] = float('inf')
    out, grads = _run_op(b, cuda, True, dy=dy)
    assert not torch.isfinite(grads['x'][0]).all()
    _assert_op(b, out, grads, True, images=slice(1, 2))
