"""The paired kernel-row weight gradient (sr_conv3x3_wgrad_pair: both convs of a residual block in one
split-K launch of conv3x3_wgrad_row3_kernel and one slab-reduce launch) on the GPU.

Kernel level, five shapes (one-step splits; splits crossing images with a short last split; one ci tile;
W 128 with two co tiles; H 1), the two items with independent bf16 operands and scales 1.0 / 0.1:
  * dW / db of both items against an fp64 conv2d of the same bf16 operands under the bound of
    test_conv_gpu.py::test_wgrad_row3_vs_fp64 (2e-5 max|ref| + 1e-4), overwriting and accumulating;
  * bitwise equal to two sr_conv3x3_wgrad calls where the two plans are the same splits;
  * an item's result does not depend on the other item, swapping items swaps results, runs repeat bitwise;
  * the workspace of exactly sr_conv3x3_wgrad_pair_workspace bytes between NaN guards.
Net level (EDSR, 256 features, 2 blocks, x4, res_scale 0.1, B 2, LR 64 x 64: the existing train-step tests
run 64 features, which never reach the kernel-row wgrad): gradients against the float64 oracle under the
bounds of test_workload_tiles_gpu.py::test_edsr_l_workload_tile_bf16_fwd_bwd, the traced launch counts, and
the train step bitwise across eager / graph replay and the side-stream modes.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from basicsr4rs_amd import _lib
from basicsr4rs_amd.ops import conv as C
from oracle import nets as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 64, 256, 256), (4, 8, 64, 256, 256), (1, 6, 64, 128, 256), (2, 5, 128, 128, 512),
          (3, 1, 64, 256, 512)]
SCALES = (1.0, 0.1)
_CASES = {}


def _desc(shape, accumulate=0):
    N, H, W, cin, cout = shape
    d = _lib.WgradDesc()
    d.dtype, d.N, d.H, d.W = _lib.dtype_code(torch.bfloat16), N, H, W
    d.Cin, d.Cin_real, d.ldx, d.Cout, d.Cout_real, d.ldy, d.ksize = cin, cin, cin, cout, cout, cout, 3
    d.scale, d.accumulate = 1.0, accumulate
    return d


def _plan(d):
    s, k, b = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().sr_conv3x3_wgrad_pair_plan(d, ctypes.byref(s), ctypes.byref(k), ctypes.byref(b)))
    return s.value, k.value, b.value


def _case(shape, cuda):
    """Operands of both items and their fp64 gradients (scaled), computed once per shape and left unchanged."""
    if shape not in _CASES:
        N, H, W, cin, cout = shape
        g = torch.Generator().manual_seed(31 + sum(shape))
        ops, refs = [], []
        for scale in SCALES:
            x = torch.randn(N, H, W, cin, generator=g).to(torch.bfloat16)
            dy = torch.randn(N, H, W, cout, generator=g).to(torch.bfloat16)
            w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
            b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
            F.conv2d(x.permute(0, 3, 1, 2).double(), w, b, padding=1).mul(dy.permute(0, 3, 1, 2).double()).sum().backward()
            ops.append((dy.to(cuda), x.to(cuda)))
            refs.append((w.grad * scale, b.grad * scale))
        _CASES[shape] = (ops, refs)
    return _CASES[shape]


def _pair(shape, ops, scales=SCALES, init=None, bias=True, ws=None):
    """One sr_conv3x3_wgrad_pair call: [(dw, db)] * 2.  ``init``: accumulate into clones of these buffers."""
    N, H, W, cin, cout = shape
    lib = _lib.load()
    d = _desc(shape, 0 if init is None else 1)
    assert lib.sr_conv3x3_wgrad_pair_ok(d) == 1
    ws_bytes = lib.sr_conv3x3_wgrad_pair_workspace(d)
    dev = ops[0][0].device
    if ws is None:
        ws = torch.empty(ws_bytes // 4 + 1, device=dev, dtype=torch.float32)
    outs = []
    arr = (_lib.WgradItem * 2)()
    for i in range(2):
        if init is None:
            dw = torch.empty(cout, cin, 3, 3, device=dev)
            db = torch.empty(cout, device=dev) if bias else None
        else:
            dw, db = init[i][0].clone(), init[i][1].clone()
        outs.append((dw, db))
        arr[i].dy, arr[i].x, arr[i].dw = ops[i][0].data_ptr(), ops[i][1].data_ptr(), dw.data_ptr()
        arr[i].db, arr[i].scale = (db.data_ptr() if db is not None else None), scales[i]
    _lib.check(lib.sr_conv3x3_wgrad_pair(d, arr, _lib.ptr(ws), ws_bytes, _lib.stream()))
    torch.cuda.synchronize()
    return outs


def _within(got, ref):
    err = (got.double().cpu() - ref).abs().max().item()
    bound = 2e-5 * ref.abs().max().item() + 1e-4
    print(f'max err {err:.3e} bound {bound:.3e}')
    return err <= bound


@pytest.mark.parametrize('shape', SHAPES)
def test_pair_vs_fp64_and_single_calls(cuda, shape):
    N, H, W, cin, cout = shape
    lib = _lib.load()
    ops, refs = _case(shape, cuda)
    outs = _pair(shape, ops)
    for (dw, db), (rw, rb) in zip(outs, refs):
        assert _within(dw, rw) and _within(db, rb)
    # accumulating into non-zero buffers: the sum is the fp64 gradient on top of what was there
    g = torch.Generator().manual_seed(5)
    init = [(torch.randn(cout, cin, 3, 3, generator=g).to(cuda), torch.randn(cout, generator=g).to(cuda)) for _ in range(2)]
    acc = _pair(shape, ops, init=init)
    for (dw, db), (iw, ib), (rw, rb) in zip(acc, init, refs):
        assert _within(dw.double() - iw.double(), rw) and _within(db.double() - ib.double(), rb)
    # two single calls: bitwise where both plans are one 64-pixel step per split, else the same bound
    single = [C.conv_wgrad_raw(dy, x, N, H, W, cin, cin, cout, cout, scale=s) for (dy, x), s in zip(ops, SCALES)]
    torch.cuda.synchronize()
    d = _desc(shape)
    S, kper, _ = _plan(d)
    S1 = (lib.sr_conv3x3_wgrad_workspace(d) - 256) // 4 // (9 * cout * cin + cout)
    M = N * H * W
    same_plan = S == S1 == M // 64  # then kper is 64 for both: the same splits
    if shape == SHAPES[0]:
        assert same_plan and kper == 64
    for (dw, db), (sw, sb), (rw, rb) in zip(outs, single, refs):
        if same_plan:
            assert torch.equal(dw, sw) and torch.equal(db, sb)
        else:
            assert S < S1
            assert _within(sw, rw) and _within(sb, rb)


@pytest.mark.parametrize('shape', SHAPES)
def test_pair_items_are_isolated_and_deterministic(cuda, shape):
    ops, _ = _case(shape, cuda)
    base = _pair(shape, ops)
    again = _pair(shape, ops)
    for (dw, db), (aw, ab) in zip(base, again):
        assert torch.equal(dw, aw) and torch.equal(db, ab)
    other = (torch.randn_like(ops[1][0].float()).to(torch.bfloat16), torch.randn_like(ops[1][1].float()).to(torch.bfloat16))
    repl = _pair(shape, [ops[0], other])
    assert torch.equal(base[0][0], repl[0][0]) and torch.equal(base[0][1], repl[0][1])
    assert not torch.equal(base[1][0], repl[1][0])
    swapped = _pair(shape, [ops[1], ops[0]], scales=SCALES[::-1])
    for i in range(2):
        assert torch.equal(base[i][0], swapped[1 - i][0]) and torch.equal(base[i][1], swapped[1 - i][1])
    nobias = _pair(shape, ops, bias=False)  # no bias-role blocks: the same weight gradients
    for (dw, _), (nw, _) in zip(base, nobias):
        assert torch.equal(dw, nw)


@pytest.mark.parametrize('shape', SHAPES)
def test_pair_workspace_bounds(cuda, shape):
    lib = _lib.load()
    ops, refs = _case(shape, cuda)
    ws_bytes = lib.sr_conv3x3_wgrad_pair_workspace(_desc(shape))
    assert ws_bytes % 4 == 0
    guard, n = 1 << 16, ws_bytes // 4
    buf = torch.full((guard + n + guard, ), float('nan'), device=cuda, dtype=torch.float32)
    outs = _pair(shape, ops, ws=buf[guard:guard + n])
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    for (dw, db), (rw, rb) in zip(outs, refs):  # every slab row that the reduce reads was written
        assert torch.isfinite(dw).all() and torch.isfinite(db).all()
        assert _within(dw, rw) and _within(db, rb)


# ---- the whole net ----

EDSR_P = dict(type='EDSR', num_in_ch=3, num_out_ch=3, num_feat=256, num_block=2, upscale=4, res_scale=0.1,
              img_range=255., rgb_mean=[0.4488, 0.4371, 0.4040])
SPAN = 'conv3x3_wgrad_row3_kernel+reduce'


def _bf16_round(t):
    return t.to(torch.bfloat16).float() if t.is_floating_point() else t


@pytest.fixture(scope='module')
def edsr_oracle():
    """bf16-rounded weights and input of the net, the float64 oracle's parameter gradients (computed once)."""
    from basicsr4rs_amd.archs import build_network
    torch.manual_seed(0)
    net = build_network(dict(EDSR_P))
    sd = {k: _bf16_round(v.detach()) for k, v in net.state_dict().items()}
    x = _bf16_round(torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)))
    sdg = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    ref = O.edsr(sdg, x.double(), num_block=2, upscale=4, res_scale=0.1)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (ref * g).sum().backward()
    return sd, x, ref.detach(), g, {k: v.grad for k, v in sdg.items() if torch.is_tensor(v) and v.grad is not None}


def _net_backward(cuda, edsr_oracle):
    """The HIP net's bf16 forward / backward with flat gradient buffers (as in training): output, gradients,
    traced spans."""
    from basicsr4rs_amd.archs import build_network
    from basicsr4rs_amd.utils import ktrace
    from basicsr4rs_amd.utils.flat import FlatParams
    sd, x, _, g, _ = edsr_oracle
    net = build_network(dict(EDSR_P))
    net.load_state_dict(sd)
    gn = net.to(cuda)
    flat = FlatParams(gn)
    ktrace.start()
    try:
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = gn(x.to(cuda))
        (out.float() * g.float().to(cuda)).sum().backward()
    finally:
        stats = ktrace.stop()
    grads = {n: p.grad.detach().cpu().double() for n, p in gn.named_parameters()}
    # the spans' relaunch closures (the roofline's re-timing) write into scratch, never into the live gradients
    assert ktrace.relaunch_count(SPAN) == stats[SPAN]['count'] and ktrace.time_relaunch(SPAN, reps=1) > 0
    ktrace.clear_relaunch()
    for n, p in gn.named_parameters():
        assert torch.equal(p.grad.detach().cpu().double(), grads[n]), n
    del flat
    return out.float().detach().cpu().double(), grads, stats


def test_edsr_net_paired_grads_vs_oracle_and_launch_counts(cuda, edsr_oracle):
    _, _, ref, _, rgrads = edsr_oracle
    out, grads, stats = _net_backward(cuda, edsr_oracle)
    with _lib.knob('SR_WG_PAIR', 0):
        out0, grads0, stats0 = _net_backward(cuda, edsr_oracle)
    # the parent's spans: 4 body convs + conv_after_body + 2 upsample convs; paired: one span per block
    assert stats0[SPAN]['count'] == 7, stats0[SPAN]
    assert stats[SPAN]['count'] == 2 + (stats0[SPAN]['count'] - 4), stats[SPAN]
    assert stats[SPAN]['flops'] == stats0[SPAN]['flops'] and stats[SPAN]['bytes'] == stats0[SPAN]['bytes']
    assert torch.equal(out, out0)
    for o, gr in ((out, grads), (out0, grads0)):
        rng = max(1.0, ref.abs().max().item())
        assert (o - ref).abs().max().item() / rng <= 5e-3
        worst = worst_l2 = 0.0
        cos_min = 1.0
        for n, a in gr.items():
            r = rgrads[n]
            worst = max(worst, (a - r).abs().max().item() / max(1e-12, r.abs().max().item()))
            worst_l2 = max(worst_l2, (a - r).norm().item() / max(1e-12, r.norm().item()))
            cos_min = min(cos_min, F.cosine_similarity(a.flatten(), r.flatten(), dim=0).item())
        print(f'worst param-grad err {worst:.3e}, relative L2 {worst_l2:.3e}, lowest cosine {cos_min:.5f}')
        assert cos_min >= 0.995 and worst <= 0.13 and worst_l2 <= 0.085
    # only the paired body convs may differ from the single calls (fp32 summation order over fewer splits)
    for n in grads:
        if not n.startswith('body.'):
            assert torch.equal(grads[n], grads0[n]), n


# ---- the train step ----

def _opt(graph, mode):
    return dict(model_type='SRModel', is_train=True, dist=False, num_gpu=1, path={}, network_g=dict(EDSR_P),
                train=dict(ema_decay=0.999, use_amp=True, cuda_graph=graph, async_wgrad=mode,
                           optim_g=dict(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99]),
                           scheduler=dict(type='MultiStepLR', milestones=[100], gamma=0.5),
                           pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean')))


def _steps(cuda, monkeypatch, graph=False, mode=False, delay=False, steps=5):
    """5 train steps; losses, parameters, EMA, and how many residual-block backwards took the paired call."""
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    took = []
    real = C.conv_wgrad_pair_raw
    monkeypatch.setattr(C, 'conv_wgrad_pair_raw', lambda *a, **k: took.append(real(*a, **k)) or took[-1])
    torch.manual_seed(0)
    model = build_model(_opt(graph, mode))
    assert model.async_wgrad == mode
    lq = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(cuda)
    gt = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(cuda)
    model.feed_data({'lq': lq, 'gt': gt})
    losses = []
    for it in range(1, steps + 1):
        model.update_learning_rate(it)
        if delay:  # hold the side stream back: the main stream runs the whole dgrad chain first
            with torch.cuda.stream(C._side_stream(torch.device(cuda))):
                torch.cuda._sleep(20_000_000)
        model.optimize_parameters(it)
        losses.append(model.get_current_log()['l_pix'])
    torch.cuda.synchronize()
    assert (model._graph is not None) == graph
    net = model.get_bare_model(model.net_g)
    return (losses, {k: v.detach().clone() for k, v in net.state_dict().items()},
            {k: v.detach().clone() for k, v in model.net_g_ema.state_dict().items()}, took)


def _same(a, b):
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.fixture(scope='module')
def eager_run(cuda):
    mp = pytest.MonkeyPatch()
    try:
        run = _steps(cuda, mp)
    finally:
        mp.undo()
    assert run[3] == [True] * 10  # 2 blocks x 5 steps, every one paired
    assert all(torch.isfinite(torch.tensor(run[0])))
    return run


def test_paired_train_step_graph_replay_bitwise(cuda, monkeypatch, eager_run):
    run = _steps(cuda, monkeypatch, graph=True)
    assert run[3] and all(run[3])
    _same(eager_run, run)


@pytest.mark.parametrize('mode', [True, 'reduce'])
def test_paired_train_step_side_stream_modes_bitwise(cuda, monkeypatch, eager_run, mode):
    run = _steps(cuda, monkeypatch, mode=mode)
    assert run[3] == [True] * 10
    _same(eager_run, run)


def test_paired_train_step_delayed_side_stream_bitwise(cuda, monkeypatch, eager_run):
    run = _steps(cuda, monkeypatch, mode=True, delay=True)
    assert run[3] == [True] * 10
    _same(eager_run, run)


def test_pair_off_train_step_differs_only_by_summation_order(cuda, monkeypatch, eager_run, knob):
    """SR_WG_PAIR=0 takes the two single calls (no paired call is made) and lands within fp32 summation-order
    noise of the paired run after 5 steps."""
    knob('SR_WG_PAIR', 0)
    run = _steps(cuda, monkeypatch)
    assert run[3] == [False] * 10
    for a, b in zip(eager_run[0], run[0]):
        assert abs(a - b) <= 1e-3 * abs(a)
