"""Host-side proof of the exact-lattice deformable conv tests (tests/_dcn_exact.py, test_dcn_exact_gpu.py).

No device is involved.  Checked here:
  * every case x family is exact (assert_exactness, columns and dcols exact in bf16, the fixed-point exponent): an
    inexact case is a broken test, not a tolerance;
  * every family reaches the sample classes it claims with at least 32 samples (the validity edges, the integers, the
    bands next to the image border, and every position relative to an LDS window);
  * the float64 oracle's conventions at the discontinuities against numbers worked by hand;
  * zero offsets with unit masks are a plain convolution;
  * a single defect applied to the oracle is rejected by assert_bits on the family named for it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O

from . import _dcn_exact as X
from . import _exact as E

PLAN = X.PLAN


@pytest.mark.parametrize('cid,family', PLAN, ids=[f'{c}-{f}' for c, f in PLAN])
def test_case_is_exact(cid, family):
    b = X.build(cid, family)
    b.check()
    # a real bf16 rounding of y must occur somewhere, or the RNE step of the stores would go unexercised
    if cid in X.F_IDS and family in ('lattice', 'edges'):
        assert float((E.to_stored(b.y, torch.bfloat16).double() != b.y).double().mean()) > 0.05


POINT_CLAIMS = {
    'lattice': ['inv_h_low', 'inv_h_high', 'inv_w_low', 'inv_w_high', 'integer', 'in_m1_0', 'in_last'],
    'integer': ['inv_h_low', 'inv_h_high', 'inv_w_low', 'inv_w_high', 'on_minus1', 'on_size', 'integer'],
    'edges': ['inv_h_low', 'inv_h_high', 'inv_w_low', 'inv_w_high', 'on_minus1', 'on_size', 'integer', 'in_m1_0',
              'in_last'],
}
FLOOR = 32


@pytest.mark.parametrize('cid', X.F_IDS)
@pytest.mark.parametrize('family', list(POINT_CLAIMS))
def test_coverage_of_point_classes(cid, family):
    n = X.sample_classes(X.CASES[cid], X.build(cid, family).offset, 2)
    for cls in POINT_CLAIMS[family]:
        assert n[cls] >= FLOOR, (cid, family, cls, n[cls])


# A sample straddles a window side only where the pixels past that side belong to the image, so the claims follow
# the maps.  F7 (28 x 36: 4 x 3 forward tiles, 2 x 3 scatter tiles whose first row of LDS images ends at row 17 + R
# of 28) has every side of both windows inside the image, at every R asked for: all six classes, which is what
# holds the ``ly < RH`` / ``lx < RW`` guards, the direct-atomic fallback behind them and the RH / RW sizing of
# dcn_gradx_dy8_kernel (R 4 with the int32 image, R 2 with the int64 one).  F1 (20 x 36) lacks only the bottom side
# of the scatter image (row 20 or 22 of 20).  The one-tile maps claim what their geometry allows: their windows
# reach past the map on the sides left out, so no image pixel lies beyond those sides (F2 12 x 10, F3 11 x 11 and
# F4 9 x 13 are covered by a single window at R >= 2 but for a few samples, fewer than the floor: they hold the
# image-border logic, not the window seams).  dcn_grad_x (the scatter of F4 and F6, and of sr_dcn_col2im) takes
# grad_x_geom's {16, 4} tile and halo at stride 1, 3 x 3 -- the 'win16x16' geometry at R 4, claimed below for F7
# (test_entry_points_exact runs it there) -- and {8, 4} at F4's stride 2 ('win8x8'), where one window holds the map.
WIN_ALL = X.CLASSES_WIN
NO_BOTTOM = ['inside', 'top', 'left', 'right', 'outside']
ITLO = ['inside', 'top', 'left', 'outside']
WINDOW_CLAIMS = {
    'F7': {('win8x16', 0): WIN_ALL, ('win8x16', 2): WIN_ALL, ('win16x16', 2): WIN_ALL, ('win16x16', 4): WIN_ALL},
    'F1': {('win8x16', 0): WIN_ALL, ('win8x16', 2): WIN_ALL, ('win16x16', 2): NO_BOTTOM, ('win16x16', 4): NO_BOTTOM},
    'F2': {('win8x16', 0): ['inside', 'outside'], ('win8x16', 2): ['inside'], ('win16x16', 2): ['inside'],
           ('win16x16', 4): ['inside']},
    'F3': {('win8x16', 0): ['inside', 'top', 'outside'], ('win8x16', 2): ['inside'], ('win16x16', 2): ['inside'],
           ('win16x16', 4): ['inside']},
    'F4': {('win8x16', 0): ['inside'], ('win8x16', 2): ['inside'], ('win8x8', 4): ['inside']},
    'F5': {('win8x16', 0): ITLO + ['bottom'], ('win8x16', 2): ITLO + ['bottom'], ('win16x16', 2): ITLO,
           ('win16x16', 4): ['inside', 'left', 'outside']},
    'F5k5': {('win8x16', 0): ITLO + ['bottom'], ('win8x16', 2): ITLO + ['bottom'], ('win16x16', 2): ['inside', 'left', 'outside'],
             ('win16x16', 4): ['inside', 'outside']},
    'F6': {('win8x16', 0): ITLO, ('win8x16', 2): ITLO, ('win16x16', 2): ['inside', 'left', 'outside'],
           ('win16x16', 4): ['inside', 'outside']},
}


@pytest.mark.parametrize('cid', list(WINDOW_CLAIMS))
def test_coverage_of_window_classes(cid):
    """lattice reaches the positions relative to the 8 x 16 tile's window (R 0 and 2) and the 16 x 16 scatter
    tile's image (R 2 and 4) that WINDOW_CLAIMS lists."""
    off = X.build(cid, 'lattice').offset
    for (tile, R), classes in WINDOW_CLAIMS[cid].items():
        n = X.sample_classes(X.CASES[cid], off, R)
        for cls in classes:
            assert n[f'{tile}/{cls}'] >= FLOOR, (cid, tile, R, cls, n[f'{tile}/{cls}'])


def test_coverage_converge_and_far():
    for cid in ('F1', 'F5', 'F5k5'):
        b = X.build(cid, 'same_sign')
        h, w = X.coords(b.case, b.offset)
        H, W = b.case[2:4]
        assert (h[0] == H // 2).all() and (w[0] == W // 2 + 1).all()
        assert b.max_mdc == b.case[4] - 1  # just below a power of two
    b = X.build('F1', 'converge')
    h, w = X.coords(b.case, b.offset)
    assert (np.floor(h[0]) == 10).all() and (np.floor(w[0]) == 19).all() and (h[0] != 10).sum() >= FLOOR
    for fam in ('far', 'far_m0'):
        b = X.build('F1', fam)
        h, w = X.coords(b.case, b.offset)
        H, W = b.case[2:4]
        assert not ((h[1] > -1) & (w[1] > -1) & (h[1] < H) & (w[1] < W)).any() and np.isfinite(b.offset.numpy()).all()
        # image 1: y == bias, nothing scattered, no offset / mask gradient
        assert torch.equal(b.y[1], b.bias.view(-1, 1, 1).expand_as(b.y[1]))
        assert not b.gx[1].any() and not b.goff[1].any() and not b.gmask[1].any() and b.gx[0].any()


# ------------------------------------------------------------------------------------------ convention pins
# One 3 x 3 map, 1 x 1 kernel, weight 1, dy 1, mask 1: the sample of output pixel q sits at (PIN_T[q], 1) -- or at
# (1, PIN_T[q]) on the transposed map -- so the column value, d / d(moving coordinate), d / d(fixed coordinate) and
# the scattered weights can be worked by hand.  The literals restate the reference's rules: valid iff
# -1 < h < H (deform_conv_cuda_kernel.cu:229, 618); corners outside the image read 0 and the upper corner is
# h_low + 1 <= H - 1 (:122, 151 region, 503-569); at an integer coordinate lh = 0, so the derivative is the forward
# difference x[h + 1] - x[h] (:527-569, :747).
PIN_X = [[1.0, 2.0, 4.0], [6.0, 7.0, 5.0], [8.0, 3.0, 9.0]]  # column 1 = (2, 7, 3), column 2 = (4, 5, 9)
PIN_T = [-1.0, -0.5, 0.0, 1.0, 2.0, 2.75, 3.0, -1.0, 3.0]
#           h:   -1   -0.5   0    1     2    2.75   3   -1    3
PIN_VAL = [0.0, 1.0, 2.0, 7.0, 3.0, 0.75, 0.0, 0.0, 0.0]    # h = 2 = H - 1: x[H - 1]; 2.75: 0.25 x[2]
PIN_DMOVE = [0.0, 2.0, 5.0, -4.0, -3.0, -3.0, 0.0, 0.0, 0.0]  # -0.5: +x[0]; 0: x[1] - x[0]; 1: x[2] - x[1]; 2: -x[2]
PIN_DFIX = [0.0, 1.0, 2.0, -2.0, 6.0, 1.5, 0.0, 0.0, 0.0]   # (column 2 - column 1) times the row weights
PIN_GX_COL1 = [1.5, 1.0, 1.25]                               # 0.5 + 1 | 1 | 1 + 0.25


@pytest.mark.parametrize('transposed', [False, True])
def test_convention_pins(transposed):
    x = np.array(PIN_X)
    t = np.array(PIN_T).reshape(3, 3)
    base_r, base_c = np.meshgrid(np.arange(3.0), np.arange(3.0), indexing='ij')
    moving, fixed = t - (base_c if transposed else base_r), 1.0 - (base_r if transposed else base_c)
    if transposed:
        x = x.T.copy()
    off = np.stack([fixed, moving] if transposed else [moving, fixed])[None]
    xx, msk = x[None, None], np.ones((1, 1, 3, 3))
    w, dy = np.ones((1, 1, 1, 1)), np.ones((1, 1, 3, 3))
    cols = O.dcn_columns(xx, off, msk, 1, 1, 1, 0, 1, 1)
    gx, goff, gm, gw, gb = O.dcn_backward(xx, off, msk, w, np.zeros(1), 1, 0, 1, 1, 1, dy)
    assert cols.reshape(-1).tolist() == PIN_VAL
    assert gm.reshape(-1).tolist() == PIN_VAL
    assert goff[0, 1 if transposed else 0].reshape(-1).tolist() == PIN_DMOVE
    assert goff[0, 0 if transposed else 1].reshape(-1).tolist() == PIN_DFIX
    want = np.zeros((3, 3))
    want[:, 1] = PIN_GX_COL1
    assert np.array_equal(gx[0, 0], want.T if transposed else want)
    assert float(gw.reshape(-1)[0]) == sum(PIN_VAL) and float(gb[0]) == 9.0


@pytest.mark.parametrize('geo', [(3, 2, 1, 1), (3, 1, 2, 2), (7, 1, 3, 1)], ids=['stride2', 'dil2', '7x7'])
def test_zero_offsets_are_a_convolution(geo):
    """Zero offsets and unit masks: the deformable conv is F.conv2d in float64 (what ops/dcn.py::_offset_conv
    relies on for its non-standard geometries)."""
    k, s, p, d = geo
    gen = E.gen_for(f'dcn/zero/{geo}')
    x, w, b = E.grid((2, 6, 11, 13), gen=gen), E.grid((8, 6, k, k), -2, 2, gen=gen), E.grid((8,), -4, 4, 0.5, gen=gen)
    ref = F.conv2d(x, w, b, stride=s, padding=p, dilation=d)
    Ho, Wo = ref.shape[2:]
    off, msk = np.zeros((2, 2 * k * k, Ho, Wo)), np.ones((2, k * k, Ho, Wo))
    y = O.dcn_forward(x.numpy(), off, msk, w.numpy(), b.numpy(), s, p, d, 1, 1)
    assert torch.equal(torch.from_numpy(y), ref)


# ------------------------------------------------------------------------------------------ single defects


def _corners_defect(kind):
    """oracle.ops._corners with one rule changed."""

    def corners(h, w, H, W):
        if kind == 'closed_validity':  # h >= -1 for h > -1 and h <= H for h < H
            valid = (h >= -1) & (w >= -1) & (h <= H) & (w <= W)
        elif kind == 'closed_high_only':
            valid = (h > -1) & (w > -1) & (h <= H) & (w <= W)
        else:
            valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        if kind == 'ceil':  # the cell below / left of an integer coordinate: lh = 1 there, not 0
            hl, wl = np.ceil(h).astype(np.int64) - 1, np.ceil(w).astype(np.int64) - 1
        else:
            hl, wl = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
        lh, lw = h - hl, w - wl
        hh, hw = 1 - lh, 1 - lw
        top = 2 if kind == 'strict_corner' else 1  # bottom / right corner guarded by < H - 1
        out = []
        for dy, dx, wt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
            y, xx = hl + dy, wl + dx
            ok = valid & (y >= 0) & (y <= H - (top if dy else 1)) & (xx >= 0) & (xx <= W - (top if dx else 1))
            out.append((np.where(ok, y, 0), np.where(ok, xx, 0), ok, wt))
        return valid, (lh, lw, hh, hw), out

    return corners


def _oracle(b, mask='same'):
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = b.case
    npy = lambda t: None if t is None else t.numpy().astype(np.float64)  # noqa: E731
    x, off, w, bias, dy = (npy(t) for t in (b.x, b.offset, b.weight, b.bias, b.dy))
    msk = npy(b.mask) if isinstance(mask, str) else mask
    y = O.dcn_forward(x, off, msk, w, bias, s, p, d, groups, dg)
    return (torch.from_numpy(y),) + tuple(None if g is None else torch.from_numpy(g)
                                          for g in O.dcn_backward(x, off, msk, w, bias, s, p, d, groups, dg, dy))


def _rejected(got64, ref64, what):
    with pytest.raises(AssertionError, match='differ from the float64 result'):
        E.assert_bits(got64.float(), ref64, what, axes='nchw')


@pytest.mark.parametrize('kind,family,outputs', [
    ('closed_validity', 'edges', ('goff',)),  # h == -1: lh = 0, no value, but a derivative from row 0
    ('strict_corner', 'edges', ('y', 'gx', 'goff', 'gmask', 'gw')),
    ('ceil', 'integer', ('goff',)),  # same value, the one-sided derivative from the other side
])
def test_corner_rule_defects_are_rejected(monkeypatch, kind, family, outputs):
    b = X.build('F2', family)
    ref = dict(zip(('y', 'gx', 'goff', 'gmask', 'gw', 'gb'), _oracle(b)))
    assert torch.equal(ref['y'], b.y) and torch.equal(ref['goff'], b.goff)
    monkeypatch.setattr(O, '_corners', _corners_defect(kind))
    bad = dict(zip(('y', 'gx', 'goff', 'gmask', 'gw', 'gb'), _oracle(b)))
    for name in outputs:
        _rejected(bad[name], ref[name], f'{kind}: {name}')


def test_closed_upper_validity_changes_nothing(monkeypatch):
    """h <= H for h < H alone cannot be seen in any output: at h == H both corner rows lie outside the image, so the
    sample reads 0 with derivative 0 either way.  (``round`` for ``floor`` likewise equals floor on the integer
    family.)  Stated here so that the defect list is honest about what a test can reject."""
    b = X.build('F2', 'edges')
    ref = _oracle(b)
    monkeypatch.setattr(O, '_corners', _corners_defect('closed_high_only'))
    for a_, r_ in zip(_oracle(b), ref):
        assert torch.equal(a_, r_)


def test_window_and_mask_defects_are_rejected():
    b = X.build('F1', 'lattice')
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = b.case
    # samples whose corners leave the 8 x 16 tile's R = 2 window read as zero
    inside = X.class_masks(b.case, b.offset, 2)['win8x16/inside'].reshape(b.mask.shape)
    lost = b.mask.numpy().astype(np.float64) * inside
    cols = O.dcn_columns(b.x.numpy(), b.offset.numpy().astype(np.float64), lost, k, k, s, p, d, dg)
    _rejected(torch.from_numpy(cols), b.cols, 'window fallback dropped: cols')
    # grad_offset without the mask factor; grad_mask with the mask applied
    ones = np.ones(b.mask.shape)
    _rejected(_oracle(b, ones)[2], b.goff, 'grad offset without mask')
    _rejected(b.gmask * b.mask.double(), b.gmask, 'grad mask with mask')
    # y rounded half-up instead of to nearest even
    with pytest.raises(AssertionError, match='differ from the float64 result'):
        E.assert_bits(E.rhu_bf16(b.y).to(torch.bfloat16), b.y, 'y half-up', axes='nchw')


def test_fixed_point_wrap_is_rejected():
    """One 16 x 16 tile's cell sum taken modulo 2^32 in units of 2^-(18 - ex): at 49 taps 256 pixels x 49 taps x 15
    x 2^14 = 3.08e9 leaves int32, at 9 and 25 taps it does not (which is why the scale must follow the tap count)."""
    for cid, wraps in (('F1', False), ('F5k5', False), ('F5', True)):
        b = X.build(cid, 'same_sign')
        assert torch.equal(b.gx[0], X.same_sign_cell(b))
        ex = int(np.frexp(b.max_mdc)[1])
        units = 256 * b.K * b.max_mdc * 2.0**(18 - ex)  # the full tile's sum on the cell, in fixed-point units
        wrapped = (units + 2.0**31) % 2.0**32 - 2.0**31
        assert (wrapped != units) == wraps, (cid, units)
        # with the tap-dependent headroom nothing wraps
        assert 256 * b.K * b.max_mdc * 2.0**(X.gx_headroom_bits(b.K) - ex) < 2.0**31
        if wraps:
            bad = b.gx.clone()
            bad[0, :, b.case[2] // 2, b.case[3] // 2 + 1] += (wrapped - units) * 2.0**(ex - 18)
            _rejected(bad, b.gx, 'wrapped cell')


def test_unwritten_grad_x_is_rejected():
    b = X.build('F1', 'far')
    bad = b.gx.clone()
    bad[1] = float('nan')  # the early return of an image that scatters nothing, without the zeroing
    _rejected(bad, b.gx, 'grad x left unwritten')
