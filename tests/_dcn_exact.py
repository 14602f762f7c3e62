"""Helpers of the exact-lattice deformable conv tests (test_dcn_exact_host.py, test_dcn_exact_gpu.py and the exact
variants of test_dcn_ext_gpu.py), on top of tests/_exact.py.

Operand lattice: x integers in [-3, 3], weight integers in [-2, 2], bias integers in [-4, 4] / 2, dy integers in
[-2, 2], mask in {0, 1/2, 1}, offset a multiple of 1/4.  Then
  * the coordinate h = int + offset is exact in fp32, so the kernels and the float64 oracle (oracle/ops.py with
    coords='f32') take the same branch everywhere, exactly on -1, on H and on the integers too;
  * lh, lw are in {0, 1/4, 1/2, 3/4}, the corner weights multiples of 1/16, a column value a multiple of 1/32 with
    |value| <= 3 (<= 96 levels: exact in bf16);
  * dcols = W^T dy is an integer (build() checks that it is exact in bf16: what own8 and the dcols GEMM store);
  * every gradient term is a multiple of 1/32 and all partial sums stay below 2^20 quanta;
  * the scatter's fixed-point conversion wt * (mask * dcols) * 2^(hb - ex) is an integer while ex <= hb - 5
    (hb = gx_headroom_bits(K): 18 up to 16 taps) and the flush (float)(int) * 2^-e is exact;
  * y is fp32-exact before its single bf16 rounding.
So the whole op, forward and all five gradients, equals the float64 oracle bit for bit.  build() checks all of this
for a case on the host (assert_exactness and the two extra conditions) before a device is touched."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ops as O

from . import _exact as E
from ._fp64 import _rne_bf16

CASES = {
    # id: N, C, H, W, Cout, k, stride, pad, dil, groups, DG, modulated
    'F1': (2, 64, 20, 36, 64, 3, 1, 1, 1, 1, 8, True),  # 3 x 3 partial 8 x 16 tiles, 2 x 3 scatter tiles (C5 geometry)
    'F2': (1, 64, 12, 10, 48, 3, 1, 1, 1, 1, 1, True),  # Cout < 64, ragged tile, Wo % 4 != 0 store path
    'F3': (1, 64, 11, 11, 16, 3, 1, 2, 2, 1, 2, True),  # dilation 2
    'F4': (2, 64, 9, 13, 64, 3, 2, 1, 1, 1, 4, False),  # DCNv1, stride 2: dcn_coord_win + dcn_grad_x {8, 4}
    'F5': (1, 64, 18, 20, 16, 7, 1, 3, 1, 1, 1, True),  # 49 taps
    'F5k5': (1, 64, 18, 20, 16, 5, 1, 2, 1, 1, 1, True),  # 25 taps
    'F6': (1, 64, 10, 18, 72, 3, 1, 1, 1, 1, 8, True),  # Cout > 64: dcn_im2col<bf16, 8> + GEMM, dcols path
    # two scatter-tile rows, the first one's LDS image ending inside the map (its last row 17 + R of 28): bottom side
    'F7': (1, 64, 28, 36, 16, 3, 1, 1, 1, 1, 4, True),
    # the five DCN_CASES of tests/test_ops_gpu.py (test_dcn_exact_gpu.py asserts they are the same tuples)
    'G0': (2, 16, 9, 9, 24, 3, 1, 1, 1, 1, 2, True),
    'G1': (2, 64, 12, 10, 64, 3, 1, 1, 1, 1, 8, True),
    'G2': (1, 6, 7, 8, 16, 3, 2, 1, 1, 2, 1, False),
    'G3': (1, 8, 6, 6, 8, 3, 1, 2, 2, 1, 1, True),
    'G4': (2, 5, 5, 5, 7, 1, 1, 0, 1, 1, 1, True),
    # v1 over four images (im2col_step 2 in test_dcn_ext_gpu.py)
    'E4': (4, 16, 9, 9, 24, 3, 1, 1, 1, 1, 2, False),
}
F_IDS = ['F1', 'F2', 'F3', 'F4', 'F5', 'F5k5', 'F6', 'F7']
G_IDS = ['G0', 'G1', 'G2', 'G3', 'G4']
# (forward fused, backward fused) under bf16 autocast, as the issue's table states
FUSED = {'F1': (True, True), 'F2': (True, True), 'F3': (True, True), 'F4': (True, False), 'F5': (True, True),
         'F5k5': (True, True), 'F6': (False, False), 'F7': (True, True)}

# which families run on which case (the host test proves each pair exact, the GPU tests run them)
PLAN = [(c, f) for c in F_IDS for f in ('lattice', 'integer', 'zero', 'edges', 'converge')]
PLAN += [(c, 'same_sign') for c in ('F1', 'F5k5', 'F5')]
PLAN += [('F1', 'far'), ('F1', 'far_m0'), ('F4', 'far')]
PLAN += [(c, f) for c in G_IDS for f in ('lattice', 'edges', 'integer')]
PLAN += [('E4', 'lattice'), ('E4', 'edges')]

FAMILIES = ['lattice', 'integer', 'zero', 'edges', 'converge', 'same_sign', 'far', 'far_m0']
EDGE_TARGETS = lambda L: [-1.25, -1.0, -0.75, -0.5, 0.0, 0.25, L - 1.5, L - 1.0, L - 0.75, L - 0.25, L, L + 0.5]  # noqa
FAR_VALUES = [1e4, -1e4, 3e9, -3e9, 65536.0, -40.0]


def out_size(case):
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    span = d * (k - 1) + 1
    return (H + 2 * p - span) // s + 1, (W + 2 * p - span) // s + 1


def gx_headroom_bits(K):
    """Bits of one contribution in the int32 scatter image of dcn_gradx_dy8_kernel: a cell of a 16 x 16 tile sums
    at most 256 K contributions, so min(18, 30 - ceil(log2(256 K))) bits each keep the sum below 2^30 (18 up to 16
    taps; gx_fx_bits in csrc/dcn.hip)."""
    return min(18, 30 - int(np.ceil(np.log2(256 * K))))


def base_grid(case):
    """Undeformed sampling rows [K, Ho, 1] and columns [K, 1, Wo] (integers, as float64)."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    ii, jj = np.divmod(np.arange(k * k), k)
    hb = (np.arange(Ho) * s - p)[None, :, None] + (ii * d)[:, None, None]
    wb = (np.arange(Wo) * s - p)[None, None, :] + (jj * d)[:, None, None]
    return hb.astype(np.float64), wb.astype(np.float64)


def coords(case, offset):
    """Sampling coordinates (h, w) [N, DG, K, Ho, Wo]: one fp32 addition of the integer base and the offset, the
    kernels' expression."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    off = offset.numpy().reshape(N, dg, k * k, 2, Ho, Wo).astype(np.float32)
    hb, wb = base_grid(case)
    h = hb.astype(np.float32)[None, None] + off[:, :, :, 0]
    w = wb.astype(np.float32)[None, None] + off[:, :, :, 1]
    return h.astype(np.float64), w.astype(np.float64)


# ------------------------------------------------------------------------------------------ offset families


def _from_targets(case, th, tw):
    """offset [N, DG 2K, Ho, Wo] (float32) that sends sample (n, g, k, ho, wo) to (th, tw) [N, DG, K, Ho, Wo]."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    hb, wb = base_grid(case)
    off = torch.stack([th - torch.from_numpy(hb)[None, None], tw - torch.from_numpy(wb)[None, None]], 3)
    return off.reshape(N, dg * 2 * k * k, Ho, Wo).float()


def offsets(case, family, gen):
    """Offsets of one family for every image.  lattice: multiples of 1/4, about 70 % in [-3.5, 3.5] and the rest in
    [-12, 12] (inside an LDS window, across its edge and beyond it, for every tile position); integer: the same
    with integers; zero: zeros; edges: row and column targets drawn independently from EDGE_TARGETS; converge /
    same_sign: every sample on one interior point (+ a per-tap fraction in {0, 1/2}; same_sign: none); far: values
    of FAR_VALUES (finite, every sample invalid)."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    shape = (N, dg * 2 * k * k, Ho, Wo)
    if family in ('lattice', 'integer'):
        q = 4 if family == 'lattice' else 1
        near = torch.randint(-7 * q // 2, 7 * q // 2 + 1, shape, generator=gen)
        wide = torch.randint(-12 * q, 12 * q + 1, shape, generator=gen)
        pick = torch.rand(shape, generator=gen) < 0.7
        return (torch.where(pick, near, wide).double() / q).float()
    if family == 'zero':
        return torch.zeros(shape)
    s5 = (N, dg, k * k, Ho, Wo)
    if family == 'edges':
        return _from_targets(case, E.choice(s5, EDGE_TARGETS(H), gen), E.choice(s5, EDGE_TARGETS(W), gen))
    if family in ('converge', 'same_sign'):
        fr = E.choice((2, 1, 1, k * k, 1, 1), [0.0, 0.5], gen) * (0.0 if family == 'same_sign' else 1.0)
        th = torch.full(s5, float(H // 2), dtype=torch.float64) + fr[0]
        tw = torch.full(s5, float(W // 2 + 1), dtype=torch.float64) + fr[1]
        return _from_targets(case, th, tw)
    if family == 'far':
        return E.choice(shape, FAR_VALUES, gen).float()
    raise KeyError(family)


# ------------------------------------------------------------------------------------------ sample classes

CLASSES_POINT = ['inv_h_low', 'inv_h_high', 'inv_w_low', 'inv_w_high', 'on_minus1', 'on_size', 'integer', 'in_m1_0',
                 'in_last']
CLASSES_WIN = ['inside', 'top', 'bottom', 'left', 'right', 'outside']


def _window_class(case, h, w, valid, th, tw, R):
    """Per valid sample: where its 2 x 2 corners lie relative to the LDS window / image of the th x tw output tile
    that owns the sample's pixel, halo R (origin tile0 * stride - pad - R, extent (t - 1) stride + (k - 1) dil +
    2 + 2 R as win_geom / bwd_fused_geom / grad_x_geom)."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    y0 = ((np.arange(Ho) // th) * th * s - p - R)[None, None, None, :, None]
    x0 = ((np.arange(Wo) // tw) * tw * s - p - R)[None, None, None, None, :]
    WH = (th - 1) * s + (k - 1) * d + 2 + 2 * R
    WW = (tw - 1) * s + (k - 1) * d + 2 + 2 * R
    ly = np.floor(h) - y0
    lx = np.floor(w) - x0
    in_y, in_x = (ly >= 0) & (ly + 1 < WH), (lx >= 0) & (lx + 1 < WW)
    out_y, out_x = (ly + 1 < 0) | (ly >= WH), (lx + 1 < 0) | (lx >= WW)
    hl, wl = np.floor(h), np.floor(w)  # a straddle counts when the corners past the window side are image pixels
    c = {'inside': in_y & in_x, 'top': (ly == -1) & ~out_x & (hl >= 0), 'bottom': (ly + 1 == WH) & ~out_x & (hl + 1 < H),
         'left': (lx == -1) & ~out_y & (wl >= 0), 'right': (lx + 1 == WW) & ~out_y & (wl + 1 < W),
         'outside': out_y | out_x}
    return {n: m & valid for n, m in c.items()}


def class_masks(case, offset, R):
    """Boolean masks [N, DG, K, Ho, Wo] of every sample class: the point classes (invalid by each of the four
    inequalities, exactly on -1, exactly on H or W, an integer coordinate, in (-1, 0), in [size - 1, size)) and,
    for valid samples, the window classes of the 8 x 16 forward / coordinate tile ('win8x16/...') and of the
    16 x 16 scatter tile ('win16x16/...': dcn_gradx_dy8, and dcn_grad_x where its {16, R} image fits) and of
    dcn_grad_x's 8 x 8 tile ('win8x8/...', the stride-2 case) at halo R."""
    N, C, H, W = case[:4]
    h, w = coords(case, offset)
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    m = {'inv_h_low': ~(h > -1), 'inv_h_high': ~(h < H), 'inv_w_low': ~(w > -1), 'inv_w_high': ~(w < W),
         'on_minus1': (h == -1) | (w == -1), 'on_size': (h == H) | (w == W),
         'integer': valid & ((h == np.floor(h)) | (w == np.floor(w))),
         'in_m1_0': valid & (((h > -1) & (h < 0)) | ((w > -1) & (w < 0))),
         'in_last': valid & (((h >= H - 1) & (h < H)) | ((w >= W - 1) & (w < W)))}
    for name, (th, tw) in (('win8x16', (8, 16)), ('win16x16', (16, 16)), ('win8x8', (8, 8))):
        for cn, cm in _window_class(case, h, w, valid, th, tw, R).items():
            m[f'{name}/{cn}'] = cm
    return m


def sample_classes(case, offset, R):
    """Samples per class (class_masks): {class name: count}."""
    return {n: int(m.sum()) for n, m in class_masks(case, offset, R).items()}


# ------------------------------------------------------------------------------------------ cases


def _scatter_weight(case, offset, mask, amp):
    """Upper bound of the sum of |terms| of every grad_x cell: the bilinear scatter of mask * amp, amp [N, DG, K, Ho,
    Wo] = max over the deformable group's channels of |dcols|; [N, DG, H, W]."""
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    hs, ws = O._sample_points(offset.numpy(), k, k, s, s, p, p, d, d, Ho, Wo, dg)
    out = np.zeros((N, dg, H, W))
    nidx = np.broadcast_to(np.arange(N)[:, None, None, None], (N, k * k, Ho, Wo))
    qmin = [1.0] * N  # per image: the quantum of wt * mask
    for g in range(dg):
        _, _, corners = O._corners(hs[:, g], ws[:, g], H, W)
        for y, xx, ok, wt in corners:
            t = np.where(ok, wt * mask[:, g] * amp[:, g], 0.0)
            np.add.at(out[:, g], (nidx, y, xx), t)
            for n in range(N):
                qmin[n] = min(qmin[n], E.quantum(torch.from_numpy(np.where(ok[n], wt[n] * mask[n, g], 0.0))))
    return torch.from_numpy(out), qmin


@functools.lru_cache(maxsize=None)
def build(cid, family):
    """Operands (torch: x, offset, mask, weight, bias, dy; float32 offset / mask, the rest float64), the float64
    results of oracle/ops.py (cols [N, C, K, Ho, Wo], dcols, y, gx, goff, gmask, gw, gb), the ``stages`` / ``abs_sum``
    lists of assert_exactness, and check() which asserts that the case is exact (assert_exactness, columns and
    dcols equal to their bf16 rounding, frexp exponent of max |mask * dcols| <= headroom - 5).  Cached: callers
    must not modify what they get."""
    case = CASES[cid]
    N, C, H, W, Cout, k, s, p, d, groups, dg, mod = case
    Ho, Wo = out_size(case)
    K = k * k
    gen = E.gen_for(f'dcn/{cid}/{family}')
    b = SimpleNamespace(cid=cid, family=family, case=case, K=K, Ho=Ho, Wo=Wo)
    b.x = E.grid((N, C, H, W), -3, 3, gen=gen)
    b.weight = E.grid((Cout, C // groups, k, k), -2, 2, gen=gen)
    b.bias = E.grid((Cout,), -4, 4, 0.5, gen=gen) if mod else None
    b.dy = E.grid((N, Cout, Ho, Wo), -2, 2, gen=gen)
    b.mask = E.choice((N, dg * K, Ho, Wo), [0.0, 0.5, 1.0], gen).float() if mod else None
    if family in ('far', 'far_m0'):  # image 0 on the lattice, image 1 far away (far_m0: and its mask all zero)
        b.offset = offsets(case, 'lattice', gen)
        b.offset[1] = offsets(case, 'far', gen)[1]
        if family == 'far_m0':
            b.mask[1] = 0.0
    else:
        b.offset = offsets(case, family, gen)
    if family == 'zero' and mod:
        b.mask = torch.ones_like(b.mask)
    if family == 'same_sign':
        # all ones but one output channel's weights: max |mask * dcols| = Cout - 1, just below a power of two
        b.weight = torch.ones_like(b.weight)
        b.weight[Cout - 1] = 0.0
        b.dy = torch.ones_like(b.dy)
        b.mask = torch.ones_like(b.mask)
    if family == 'converge':
        # thousands of samples on one cell: weight and dy from [-1, 1] keep the cell's sum of |terms| below 2^20 quanta
        b.weight = E.grid(b.weight.shape, -1, 1, gen=gen)
        b.dy = E.grid(b.dy.shape, -1, 1, gen=gen)
    if family in ('converge', 'same_sign') and N > 1:  # image 1 stays an ordinary image
        b.offset[1:] = offsets(case, 'lattice', gen)[1:]
    npy = lambda t: None if t is None else t.numpy().astype(np.float64)  # noqa: E731
    x, off, msk, w, bias, dy = (npy(t) for t in (b.x, b.offset, b.mask, b.weight, b.bias, b.dy))
    geo = (s, p, d)
    tt = torch.from_numpy
    cols = O.dcn_columns(x, off, msk, k, k, *geo, dg)
    b.cols = tt(cols)
    b.y = tt(O.dcn_forward(x, off, msk, w, bias, *geo, groups, dg))
    gx, goff, gm, gw, gb = O.dcn_backward(x, off, msk, w, bias, *geo, groups, dg, dy)
    b.gx, b.goff, b.gw = tt(gx), tt(goff), tt(gw)
    b.gmask = None if gm is None else tt(gm)
    b.gb = None if gb is None else tt(gb)
    cg, og = C // groups, Cout // groups
    dcols = np.zeros((N, C, K, Ho, Wo))
    wr = w.reshape(Cout, cg, K)
    for g in range(groups):
        dcols[:, g * cg:(g + 1) * cg] = np.einsum('ock,nohw->nckhw', wr[g * og:(g + 1) * og],
                                                  dy[:, g * og:(g + 1) * og])
    b.dcols = tt(dcols)
    m5 = np.ones((N, dg, K, Ho, Wo)) if msk is None else msk.reshape(N, dg, K, Ho, Wo)
    amp = np.abs(dcols).reshape(N, dg, C // dg, K, Ho, Wo).max(2)
    b.max_mdc = float((m5 * amp).max())
    # sums of |terms|
    mag_y = np.zeros_like(b.y.numpy())
    mag_gw = np.zeros((Cout, cg, K))
    for g in range(groups):
        mag_y[:, g * og:(g + 1) * og] = np.einsum('ock,nckhw->nohw', np.abs(wr[g * og:(g + 1) * og]),
                                                  np.abs(cols[:, g * cg:(g + 1) * cg]))
        mag_gw[g * og:(g + 1) * og] = np.einsum('nohw,nckhw->ock', np.abs(dy[:, g * og:(g + 1) * og]),
                                                np.abs(cols[:, g * cg:(g + 1) * cg]))
    if bias is not None:
        mag_y += np.abs(bias)[None, :, None, None]
    mag_gx, q_wm = _scatter_weight(case, b.offset, m5, amp)
    cpg = C // dg
    b.stages = [('x', b.x), ('weight', b.weight), ('dy', b.dy), ('offset', b.offset.double()), ('cols', b.cols),
                ('dcols', b.dcols), ('y', b.y), ('grad x', b.gx), ('grad offset', b.goff), ('grad weight', b.gw)]
    b.stages += [(n, t) for n, t in (('bias', b.bias), ('grad mask', b.gmask), ('grad bias', b.gb)) if t is not None]
    q_cols = E.quantum(b.cols)
    b.abs_sum = [('y', tt(mag_y), q_cols), ('grad weight', tt(mag_gw), q_cols)]
    b.abs_sum += [(f'grad x, image {n}', mag_gx[n], q_wm[n]) for n in range(N)]
    b.abs_sum += [
        ('grad bias', b.dy.abs().sum((0, 2, 3)), 1.0),
        # a group's channel sum: |d bilinear| <= 2 max|x| = 6 (multiples of 1/4, mask 1/2), |sample| <= 3
        ('grad offset', torch.tensor(cpg * 6.0 * b.max_mdc), 1.0 / 8),
        ('grad mask', torch.tensor(cpg * 3.0 * float(amp.max())), 1.0 / 16)]

    def check():
        E.assert_exactness(b.stages, b.abs_sum)
        for name, t in (('cols', b.cols), ('dcols', b.dcols)):
            assert torch.equal(_rne_bf16(t), t), f'{cid}/{family}: {name} is not exact in bf16'
        ex = int(np.frexp(b.max_mdc)[1])
        assert ex <= gx_headroom_bits(K) - 5, f'{cid}/{family}: max |mask dcols| {b.max_mdc} leaves the fixed point'

    b.check = check
    return b


def same_sign_cell(b):
    """Closed form of the same_sign case: image 0's grad x is dcols Ho Wo K on the one cell every sample hits (for
    every input channel: dcols = Cout - 1 from the all-ones weights with one output channel zeroed), else zero."""
    N, C, H, W, Cout = b.case[:5]
    ref = torch.zeros(C, H, W, dtype=torch.float64)
    ref[:, H // 2, W // 2 + 1] = float((Cout - 1) * b.Ho * b.Wo * b.K)
    return ref
