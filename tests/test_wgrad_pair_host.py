"""Host side of the paired kernel-row weight gradient (sr_conv3x3_wgrad_pair: both convs of a residual
block in one split-K launch and one reduce launch): where the paired form runs, its split plan and the
argument refusals.  No GPU: every check here returns before a launch."""
import ctypes

import pytest
import torch

from basicsr4rs_amd import _lib

BF = _lib.dtype_code(torch.bfloat16)


def desc(N, H, W, cin, cout, dtype=BF, out_ps=0, ldy=None):
    d = _lib.WgradDesc()
    d.dtype, d.N, d.H, d.W = dtype, N, H, W
    d.Cin, d.Cin_real, d.ldx, d.Cout, d.Cout_real, d.ksize = cin, cin, cin, cout, cout, 3
    d.ldy, d.out_ps, d.scale, d.accumulate = cout if ldy is None else ldy, out_ps, 1.0, 0
    return d


def plan(d):
    s, k, b = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().sr_conv3x3_wgrad_pair_plan(d, ctypes.byref(s), ctypes.byref(k), ctypes.byref(b)))
    return s.value, k.value, b.value


BODY_LIKE = [(32, 64, 64, 256, 256), (16, 64, 64, 256, 256), (2, 64, 64, 256, 256), (1, 3, 64, 256, 256),
             (4, 8, 64, 256, 256), (1, 6, 64, 128, 256), (2, 5, 128, 128, 512), (3, 1, 64, 256, 512),
             (8, 48, 192, 384, 256), (32, 64, 64, 512, 512), (5, 7, 64, 256, 256)]


@pytest.mark.parametrize('bg', [-1, 1, 2, 3, 5])
@pytest.mark.parametrize('shape', BODY_LIKE)
def test_pair_plan_covers_one_wave_and_every_pixel_once(shape, bg):
    N, H, W, cin, cout = shape
    lib = _lib.load()
    d = desc(*shape)
    with _lib.knob('SR_WG_PAIR', bg):
        assert lib.sr_conv3x3_wgrad_pair_ok(d) == 1
        S, kper, blocks = plan(d)
        ws = lib.sr_conv3x3_wgrad_pair_workspace(d)
    g = 3 if bg <= 0 else bg
    M = N * H * W
    tco, ntile = cout // 256, 3 * (cout // 256) * (cin // 128)
    assert blocks == 2 * S * ntile + 2 * -(-S // g) * tco and blocks <= 256
    assert kper % 64 == 0 and kper > 0 and 1 <= S <= M // 64
    assert (S - 1) * kper < M <= S * kper  # the S ranges [s kper, min(M, (s + 1) kper)) tile M, none empty
    assert ws == 2 * (S * 9 * cout * cin + S * cout) * 4 + 256
    # the largest S of one 256-block wave, capped at one 64-pixel step per split
    S0 = min(max(s for s in range(1, 129) if 2 * s * ntile + 2 * -(-s // g) * tco <= 256), M // 64)
    kp0 = -(-(-(-M // S0)) // 64) * 64
    assert (S, kper) == (-(-M // kp0), kp0)


def test_pair_plan_of_the_edsr_body():
    d = desc(32, 64, 64, 256, 256)
    assert plan(d) == (20, 6592, 254)
    with _lib.knob('SR_WG_PAIR', 2):
        assert plan(d) == (19, 6912, 248)


def test_pair_ok_only_where_the_paired_form_runs():
    lib = _lib.load()
    ok = lib.sr_conv3x3_wgrad_pair_ok
    assert ok(desc(32, 64, 64, 256, 256)) == 1
    assert ok(desc(32, 64, 64, 256, 264)) == 0                   # Cout 264
    assert ok(desc(32, 64, 64, 64, 256)) == 0                    # Cin 64
    assert ok(desc(32, 64, 96, 256, 256)) == 0                   # W 96
    assert ok(desc(32, 64, 64, 256, 1024, out_ps=2, ldy=256)) == 0  # pixel-shuffled dy
    assert ok(desc(32, 64, 64, 256, 256, dtype=_lib.dtype_code(torch.float32))) == 0
    assert ok(None) == 0
    with _lib.knob('SR_WG_PAIR', 0):
        assert ok(desc(32, 64, 64, 256, 256)) == 0
        assert lib.sr_conv3x3_wgrad_pair_workspace(desc(32, 64, 64, 256, 256)) == 0
    with _lib.knob('SR_WG_ROW3', 0):                             # the kernel-row wgrad itself off
        assert ok(desc(32, 64, 64, 256, 256)) == 0
    try:
        _lib.check(lib.sr_conv3x3_set_variant(78))
        assert ok(desc(32, 64, 64, 256, 256)) == 0
    finally:
        _lib.check(lib.sr_conv3x3_set_variant(0))
    assert ok(desc(32, 64, 64, 256, 256)) == 1


def test_pair_plan_ignores_the_single_call_knob_and_is_stable():
    d = desc(32, 64, 64, 256, 256)
    base = plan(d)
    with _lib.knob('SR_WG_ROW3', 5):  # the single call's bias group: another plan's knob
        assert plan(d) == base
    assert plan(d) == base


def test_pair_argument_refusals():
    lib = _lib.load()
    d = desc(1, 3, 64, 256, 256)
    p = 4096  # never dereferenced: every refusal is decided on the host

    def items(db0=p, db1=p, dy0=p):
        arr = (_lib.WgradItem * 2)()
        arr[0].dy, arr[0].x, arr[0].dw, arr[0].db, arr[0].scale = dy0, p, p, db0, 1.0
        arr[1].dy, arr[1].x, arr[1].dw, arr[1].db, arr[1].scale = p, p, p, db1, 0.1
        return arr

    ws_bytes = lib.sr_conv3x3_wgrad_pair_workspace(d)
    ws = ctypes.c_void_p(p)

    def refused(rc, word):
        assert rc == -1 and word in lib.sr_last_error().decode(), (rc, lib.sr_last_error())

    refused(lib.sr_conv3x3_wgrad_pair(None, items(), ws, ws_bytes, None), 'null')
    refused(lib.sr_conv3x3_wgrad_pair(d, None, ws, ws_bytes, None), 'null')
    refused(lib.sr_conv3x3_wgrad_pair(d, items(), None, ws_bytes, None), 'null')
    refused(lib.sr_conv3x3_wgrad_pair(d, items(dy0=None), ws, ws_bytes, None), 'null item')
    refused(lib.sr_conv3x3_wgrad_pair(d, items(), ws, ws_bytes - 1, None), 'workspace too small')
    refused(lib.sr_conv3x3_wgrad_pair(d, items(db0=None), ws, ws_bytes, None), 'both db or neither')
    refused(lib.sr_conv3x3_wgrad_pair(d, items(db1=None), ws, ws_bytes, None), 'both db or neither')
    refused(lib.sr_conv3x3_wgrad_pair(desc(1, 3, 64, 256, 264), items(), ws, 1 << 40, None), 'not on the paired')
    with _lib.knob('SR_WG_PAIR', 0):
        refused(lib.sr_conv3x3_wgrad_pair(d, items(), ws, 1 << 40, None), 'not on the paired')
    d2 = desc(1, 3, 64, 256, 256)
    d2.accumulate = 2
    refused(lib.sr_conv3x3_wgrad_pair(d2, items(), ws, ws_bytes, None), 'slab-only')
    s = ctypes.c_int(0)
    refused(lib.sr_conv3x3_wgrad_pair_plan(desc(1, 3, 64, 64, 256), ctypes.byref(s), ctypes.byref(s), ctypes.byref(s)),
            'not on the paired')
    refused(lib.sr_conv3x3_wgrad_pair_plan(d, None, ctypes.byref(s), ctypes.byref(s)), 'null')
