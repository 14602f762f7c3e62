"""Host checks of the exact-arithmetic conv tests (no GPU): the operand grids are bf16-exact, every case of
every table of tests/_exact_cases.py passes assert_exactness, and -- a test that cannot fail proves nothing --
assert_bits rejects each single defect applied to the float64 reference at the smallest case of every kernel
family, in dense and (where the defect touches the impulse) impulse mode, while the unmutated reference passes."""
import pytest
import torch

from . import _exact as E
from . import _exact_cases as X
from ._fp64 import _rne_bf16

FWD_SMALL = X.smallest(X.FWD)
FWD_SMALL_PLAIN_INPUT = X.smallest(X.FWD, gathers=False)  # impulse mode: no input gather
WGRAD_SMALL = X.smallest(X.WGRAD)


# ------------------------------------------------------------------------------------------ grids and helpers


def test_grids_are_bf16_exact():
    g = E.gen_for('grids')
    for t in (E.grid((4096,), gen=g), E.grid((4096,), scale=0.125, gen=g), E.grid((4096,), -8, 8, 0.125, gen=g),
              E.choice((64,), (0.5, 1.0, 2.0), gen=g), torch.tensor([E.SLOPE, E.ALPHA, E.BETA2, E.SENTINEL]).double()):
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    gate = E.grid((4096,), gen=g)
    assert (gate == 0).any() and (gate > 0).any() and (gate < 0).any()  # g > 0 is the branch: zeros on both sides
    with pytest.raises(AssertionError):
        E.store(torch.tensor([0.2], dtype=torch.float64), torch.bfloat16)


def test_rne_bf16_is_torch_rounding_and_differs_from_half_up_on_ties():
    g = E.gen_for('rne')
    v = torch.cat([E.grid((20000,), -4000, 4000, 0.125, gen=g), torch.tensor([257.0, 259.0, -257.0, 1028.0, 0.0]).double()])
    assert torch.equal(_rne_bf16(v), v.float().to(torch.bfloat16).double())
    assert torch.equal(E.to_stored(v, torch.bfloat16).double(), _rne_bf16(v))
    ties = torch.tensor([257.0, 259.0, -257.0]).double()  # halfway between two bf16 values
    assert _rne_bf16(ties).tolist() == [256.0, 260.0, -256.0] and E.rhu_bf16(ties).tolist() == [258.0, 260.0, -258.0]


def test_assert_exactness_rejects_inexact_cases():
    ok = torch.tensor([1.5, -0.125]).double()
    E.assert_exactness([('a', ok)], [('s', torch.tensor([2.0**17 - 1]).double(), 0.125)])
    with pytest.raises(AssertionError, match='not fp32-exact'):
        E.assert_exactness([('lrelu 0.2', ok * 0.2)], [])
    with pytest.raises(AssertionError, match='quanta'):
        E.assert_exactness([], [('s', torch.tensor([2.0**17]).double(), 0.125)])


def test_assert_bits_reports_the_pattern():
    ref = E.grid((2, 4, 128, 16), scale=0.125, gen=E.gen_for('pattern'))
    good = E.to_stored(ref, torch.bfloat16)
    E.assert_bits(good, ref, 'unchanged')
    E.assert_bits(ref.float(), ref, 'unchanged f32')
    bad = good.clone()
    bad[1, :, 64, 8:16] += 1
    with pytest.raises(AssertionError) as ei:
        E.assert_bits(bad, ref, 'column')
    msg = str(ei.value)
    assert '32 of' in msg and 'first at (n=1, y=0, x=64, c=8)' in msg and 'one image (n=1)' in msg
    assert 'one column (x=64)' in msg and 'one 8-channel chunk (chunk 1)' in msg and '8 .. 8' in msg
    bad = good.clone()
    bad[:, :, 63:65, :] -= 0.25
    with pytest.raises(AssertionError, match='64-pixel strip seam columns'):
        E.assert_bits(bad, ref, 'seam')
    bad = good.clone()
    bad[0, 1, 5, 3] = float('nan')
    with pytest.raises(AssertionError, match=r'1 NaN \(never written\)'):
        E.assert_bits(bad, ref, 'poison')


def test_impulse_result_is_the_placed_weight_image():
    shape, w = (2, 5, 7, 16), E.grid((24, 16, 3, 3), scale=0.125, gen=E.gen_for('imp'))
    for pos in [(0, 0, 0, 0), (0, 0, 6, 15), (1, 4, 0, 8), (1, 4, 6, 15), (0, 2, 3, 5)]:
        acc, _ = E.conv_acc(E.gather_input(E.impulse(shape, pos)), w)
        assert torch.equal(acc, E.impulse_acc(shape, pos, w))
        assert torch.equal(acc.to(torch.bfloat16).double(), acc)
    w1 = E.grid((24, 16, 1, 1), scale=0.125, gen=E.gen_for('imp1'))
    assert torch.equal(E.conv_acc(E.gather_input(E.impulse(shape, (1, 2, 3, 4))), w1)[0],
                       E.impulse_acc(shape, (1, 2, 3, 4), w1))


# ------------------------------------------------------------------------------------------ every table is exact


def test_forward_tables_are_exact():
    ids = set()
    for c in X.FWD + X.FWD_IMPULSE:
        assert c.id not in ids, c.id
        ids.add(c.id)
        b = X.build_fwd(c)
        E.assert_exactness(b.stages, b.abs_sum)
        assert tuple(b.ref.shape) == ((b.ybuf[0]) if c.nchw else b.ybuf[0][:3] + (b.ybuf[2],))
        assert b.ref.abs().max() > 0
    fam = {c.family for c in X.FWD}
    assert fam == {'pp', 'big', 'tile', 'wk', 'lin', 'f32', 'pph', 'halo', 'band', 'band-strips', 'tail'}
    assert {c.family for c in X.FWD_IMPULSE} == fam


def test_wgrad_tables_are_exact():
    ids = set()
    for c in X.WGRAD + [X.wg(f'pair{i}', X.PAIR_SHAPE, 0, X.ROW3, scale=s) for i, s in enumerate(X.PAIR_SCALES)]:
        assert c.id not in ids, c.id
        ids.add(c.id)
        b = X.build_wgrad(c)
        E.assert_exactness(b.stages, b.abs_sum)
        assert b.ref.dw.abs().max() > 0 and b.ref.db.abs().max() > 0


def test_convk_and_conv4s2_tables_are_exact():
    for k, ch, shape, _ in X.CONVK:
        b = X.build_convk(k, ch, shape)
        E.assert_exactness(b.stages, b.abs_sum)
    for case, _ in X.CONV4S2:
        b = X.build_conv4s2(case)
        E.assert_exactness(b.stages, b.abs_sum)


# ------------------------------------------------------------------------------------------ mutation checks


def _flagged(acc, b, c, what):
    """A kernel that computed ``acc`` and ran the case's epilogue correctly must be rejected."""
    y, _ = E.epilogue(acc, b.e)
    y = y.contiguous() if c.nchw else E.nhwc(y)
    got = E.to_stored(y, torch.float32 if c.nchw else X.DT[c.dtype])
    with pytest.raises(AssertionError, match='elements differ'):
        E.assert_bits(got, b.ref, f'{c.id}: {what}', axes='ncyx' if c.nchw else 'nyxc')


def _fwd_defects(c, b, pos=None):
    """(name, mutated accumulation) of every forward defect for a case; with an impulse at ``pos`` = (n, y, x, ch)
    the defects sit on it."""
    N, H, W, cin, cout = c.shape
    k = c.ksize
    xl, w, acc = b.xl, b.w64, b.acc
    mid = (k // 2, k // 2)
    if pos is not None:
        n, y, x, ch = pos
    else:  # a pixel and a channel pair where the defect is one: a non-zero product, two different neighbours
        n, y, x = N - 1, H // 2, 0
        px = xl[n, :, y, x]
        ok = [i for i in range(0, cin - 1, 2)
              if px[i] != 0 and px[i] != px[i + 1] and w[:, i, mid[0], mid[1]].abs().max() > 0]
        ch = ok[-1]
    right = (0, k - 1) if k == 3 else (0, 0)  # at column 0 the tap reading column 1 (row above)
    seam = 64 if W > 64 else W // 2  # an interior strip seam (x = 64), else the middle column of a narrow image
    out = []
    if pos is None:
        out += [('tap dropped at the left border column', E.drop_term(acc, xl, w, right, ch, x=0)),
                ('tap dropped at the right border column', E.drop_term(acc, xl, w, mid, ch, x=W - 1)),
                ('tap dropped at a strip seam column', E.drop_term(acc, xl, w, mid, ch, x=seam)),
                ('tap dropped left of the seam', E.drop_term(acc, xl, w, right, ch, x=seam - 1))]
    else:
        out.append(('tap dropped at the impulse column', E.drop_term(acc, xl, w, mid, ch, x=x)))
    out.append(('one K element counted twice', E.double_term(acc, xl, w, mid, ch, n=n, y=y, x=x)))
    c0 = ch // 8 * 8 + (ch % 8) // 2 * 2  # the even channel of ch's pair inside its 8-channel group
    if c0 + 1 < cin:
        out.append(('adjacent channels swapped at one pixel', E.swap_channels(xl, w, c0, n, y, x)))
    if k == 3 and y + 1 < H:
        out.append(('halo row shifted by one pixel', E.shift_halo_row(acc, xl, w, n, y + 1)))
    return out


@pytest.mark.parametrize('case', FWD_SMALL, ids=lambda c: c.id)
def test_forward_defects_are_rejected_dense(case):
    c = case
    b = X.build_fwd(c)
    dt = torch.float32 if c.nchw else X.DT[c.dtype]
    E.assert_bits(E.to_stored(b.ref, dt), b.ref, c.id, axes='ncyx' if c.nchw else 'nyxc')
    for what, acc in _fwd_defects(c, b):
        _flagged(acc, b, c, what)


BF16_FAMILIES = sorted({c.family for c in X.FWD if not c.nchw and c.dtype == X.BF})


@pytest.mark.parametrize('family', BF16_FAMILIES)
def test_round_half_up_is_rejected(family):
    """Round-half-up in place of RNE on the bf16 store, at the family's smallest case whose result holds a tie
    that the two roundings resolve differently (a K = 184 linear stays below 32, where the 1/8 grid has no ties:
    there the next larger case of the family takes its place)."""
    cases = sorted((c for c in X.FWD if c.family == family), key=lambda c: torch.tensor(c.shape).prod().item())
    for c in cases:
        b = X.build_fwd(c)
        if not torch.equal(E.rhu_bf16(b.ref), _rne_bf16(b.ref)):
            break
    else:
        raise AssertionError(f'no case of family {family} has a rounding tie')
    with pytest.raises(AssertionError, match='elements differ'):
        E.assert_bits(E.rhu_bf16(b.ref).to(torch.bfloat16), b.ref, f'{c.id}: round half up')


@pytest.mark.parametrize('case', FWD_SMALL_PLAIN_INPUT, ids=lambda c: c.id)
def test_forward_defects_are_rejected_impulse(case):
    c0 = case
    N, H, W, cin, cout = c0.shape
    for pos in [(0, 0, 0, 1), (N - 1, H - 2 if H > 1 else 0, (64 if W > 64 else W // 2), cin - 2)]:
        c = X.fw(c0.family, c0.shape, c0.variant, c0.kernel, dtype=c0.dtype, ksize=c0.ksize, nchw=c0.nchw,
                 mode=('impulse', pos))
        b = X.build_fwd(c)
        dt = torch.float32 if c.nchw else X.DT[c.dtype]
        assert torch.equal(E.to_stored(b.ref, dt).double(), b.ref)  # bf16-exact: no rounding can mask anything
        E.assert_bits(E.to_stored(b.ref, dt), b.ref, c.id, axes='ncyx' if c.nchw else 'nyxc')
        for what, acc in _fwd_defects(c, b, pos):
            _flagged(acc, b, c, what)


@pytest.mark.parametrize('case', WGRAD_SMALL, ids=lambda c: c.id)
def test_wgrad_defects_are_rejected(case):
    c = case
    b = X.build_wgrad(c)
    N, H, W, cin, cout = c.shape
    M = N * H * W
    for ref, init in ((b.ref, None), (b.acc, b.init)):
        E.assert_bits(ref.dw.float(), ref.dw, c.id, axes=('co', 'ci', 'ky', 'kx'))
        E.assert_bits(ref.db.float(), ref.db, c.id, axes=('co',))
        m0 = (M // 64 // 2) * 64
        for what, dyl in (('one pixel row of one image omitted', E.omit_pixels(b.dyl, N - 1, y=H - 1)),
                          ('one split slab omitted', E.omit_pixels(b.dyl, 0, m0=m0, m1=min(M, m0 + 64)))):
            bad = E.wgrad_ref(b.xl, dyl, c.ksize, c.scale, init=init)
            with pytest.raises(AssertionError, match='elements differ'):
                E.assert_bits(bad.dw.float(), ref.dw, f'{c.id}: {what} (dW)', axes=('co', 'ci', 'ky', 'kx'))
            with pytest.raises(AssertionError, match='elements differ'):
                E.assert_bits(bad.db.float(), ref.db, f'{c.id}: {what} (db)', axes=('co',))
