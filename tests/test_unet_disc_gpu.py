"""UNetDiscriminatorSN on the HIP engine against the same network in stock nn modules (torch's spectral_norm,
F.interpolate) in float64 on the CPU, loaded strictly from the same state dict (tests/_unet_ref.py).

Bounds, by the convention of tests/test_discriminator_gpu.py: fp32 within 8 x the rel-L2 error of the stock network run
in fp32 on the CPU; bf16 within 2 x the rel-L2 error of a float64 run whose normalised conv weights, stored maps and
gradient maps are rounded to bf16; both measured here against the float64 run, never against the HIP result.  The
spectral-norm buffers are fp32 in both compute dtypes, so they keep the fp32 bound under bf16.  Each measured error is
printed beside its bound."""
import copy
import functools

import pytest
import torch

from . import _unet_ref as R
from ._fp64 import _bits, _ids

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _run_stock(net, x, dout, train=True, grads=True):
    net.train(train)
    dt = next(net.parameters()).dtype
    xx = x.to(dt).clone().requires_grad_(grads)
    out = net(xx)
    res = {'out': out.detach()}
    if grads:
        out.backward(dout.to(dt))
        res['dx'] = xx.grad
        for k, p in net.named_parameters():
            res['grad.' + k] = p.grad
    for k, b in net.named_buffers():
        res['buf.' + k] = b.detach().clone()
    return res


@functools.lru_cache(None)
def _case(nf, shape, train=True, grads=True, skip=True):
    """The state dict, inputs, the float64 results and the two bounds per quantity; computed once and shared."""
    sd = R.he_init_sn(R.StockUNetSN(3, nf, skip), seed=nf + shape[-1]).state_dict()
    g = torch.Generator().manual_seed(shape[0] + shape[-1])
    x = torch.rand(shape, generator=g)
    dout = torch.randn(shape[0], 1, shape[2], shape[3], generator=g)
    runs = {
        'f64': _run_stock(R.stock_like(sd, 3, nf, torch.float64, skip), x, dout, train, grads),
        'f32': _run_stock(R.stock_like(sd, 3, nf, torch.float32, skip), x, dout, train, grads),
        'emu': _run_stock(R.stock_like(sd, 3, nf, torch.float64, skip, emulate=True), x, dout, train, grads),
    }
    ref = runs['f64']
    bounds = {}
    for k in ref:
        f32 = 8 * _l2(runs['f32'][k], ref[k])
        bounds[k] = {torch.float32: f32, torch.bfloat16: f32 if k.startswith('buf.') else 2 * _l2(runs['emu'][k], ref[k])}
    return sd, x, dout, ref, bounds


def _build(sd, nf, skip=True):
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=nf, skip_connection=skip)).cuda()
    net.load_state_dict(sd, strict=True)
    return net


def _run_hip(net, x, dout, dtype, train=True, grads=True):
    net.train(train)
    xx = x.cuda().requires_grad_(grads)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        out = net(xx)
    assert out.shape == (x.shape[0], 1, x.shape[2], x.shape[3]) and out.dtype == torch.float32
    res = {'out': out.detach()}
    if grads:
        out.backward(dout.cuda())
        res['dx'] = xx.grad
        for k, p in net.named_parameters():
            assert p.grad is not None and p.grad.dtype == torch.float32, k
            res['grad.' + k] = p.grad
    for k, b in net.named_buffers():
        res['buf.' + k] = b.detach().clone()
    return res


def _compare(got, ref, bounds, dtype, what, keys=None):
    bad = []
    for k in keys or ref:
        err, bound = _l2(got[k].cpu(), ref[k]), bounds[k][dtype]
        print(f'{what} [{_ids(dtype)}] {k}: rel-L2 {err:.3e}, bound {bound:.3e}, ratio {err / max(bound, 1e-300):.3f}')
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


SHAPE = (2, 3, 32, 48)


@pytest.mark.parametrize('skip', [True, False], ids=['skip', 'noskip'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_unet_matches_float64(dtype, skip):
    """(3, 8), input [2, 3, 32, 48] (non-square), training mode: the output map, the input gradient, every parameter
    gradient, and weight_u / weight_v after the call."""
    sd, x, dout, ref, bounds = _case(8, SHAPE, skip=skip)
    assert any(k.endswith('weight_u') for k in sd) and 'grad.conv4.weight_orig' in ref and 'buf.conv8.weight_v' in ref
    got = _run_hip(_build(sd, 8, skip), x, dout, dtype)
    _compare(got, ref, bounds, dtype, f'unet 8 {"skip" if skip else "noskip"}')


def test_unet_real_channel_counts_forward():
    """num_feat 64, input [1, 3, 32, 32], forward only, fp32: the 64 .. 512 channel convs of the train YAMLs."""
    shape = (1, 3, 32, 32)
    sd, x, dout, ref, bounds = _case(64, shape, True, False)
    got = _run_hip(_build(sd, 64), x, dout, torch.float32, grads=False)
    _compare(got, ref, bounds, torch.float32, 'unet 64')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_unet_eval_forward(dtype):
    sd, x, dout, ref, bounds = _case(8, SHAPE, False, False)
    net = _build(sd, 8)
    got = _run_hip(net, x, dout, dtype, train=False, grads=False)
    _compare(got, ref, bounds, dtype, 'unet eval', keys=['out'])
    for k, b in net.named_buffers():
        assert torch.equal(_bits(b.cpu()), _bits(sd[k])), k  # eval leaves u and v alone


def test_unet_frozen_parameters():
    """With the parameters frozen (the generator half of a GAN step) the input gradient has the same bits, neither a
    weight-gradient nor a spectral-norm backward kernel is launched, and u / v still move."""
    from basicsr4rs_amd.utils import ktrace
    sd, x, dout, _, _ = _case(8, SHAPE)
    dxs, recs, bufs = [], [], []
    for frozen in (False, True):
        net = _build(sd, 8)
        for p in net.parameters():
            p.requires_grad = not frozen
        xx = x.cuda().requires_grad_(True)
        ktrace.start()
        try:
            net(xx).backward(dout.cuda())
        finally:
            recs.append(ktrace.stop())
        dxs.append(xx.grad.clone())
        bufs.append({k: b.clone() for k, b in net.named_buffers()})
        assert all((p.grad is None) == frozen for p in net.parameters())
    assert torch.equal(_bits(dxs[0]), _bits(dxs[1]))
    assert any('wgrad' in k for k in recs[0]) and 'spectral_norm_bwd_kernels' in recs[0], sorted(recs[0])
    assert not any('wgrad' in k or 'spectral_norm_bwd' in k for k in recs[1]), sorted(recs[1])
    for k in ('spectral_norm_fwd_kernels', 'up2_fwd_kernel', 'up2_bwd_kernel', 'conv4s2_dgrad_kernel'):
        assert k in recs[1], sorted(recs[1])
    # the launch count of the normalisation does not grow with the eight layers: one grouped sequence
    assert recs[1]['spectral_norm_fwd_kernels']['count'] == 1 and recs[1]['spectral_norm_fwd_kernels']['launches'] == 5
    for k, b in bufs[1].items():
        assert torch.equal(_bits(b), _bits(bufs[0][k])) and not torch.equal(b.cpu(), sd[k]), k


def test_unet_three_training_forwards_move_the_buffers_three_times():
    sd, x, _, _, _ = _case(8, SHAPE)
    nets = {dt: R.stock_like(sd, 3, 8, dt).train() for dt in (torch.float64, torch.float32)}
    hip = _build(sd, 8).train()
    for i in range(3):
        with torch.no_grad():
            for dt, n in nets.items():
                n(x.to(dt))
            hip(x.cuda())
    ref, f32 = dict(nets[torch.float64].named_buffers()), dict(nets[torch.float32].named_buffers())
    first = _case(8, SHAPE)[3]
    bad = []
    for k, b in hip.named_buffers():
        err, bound = _l2(b.cpu(), ref[k]), 8 * _l2(f32[k], ref[k])
        moved = _l2(first['buf.' + k], ref[k])
        print(f'unet 3 forwards {k}: rel-L2 {err:.3e}, bound {bound:.3e}; first iterate is {moved:.3e} away')
        if not err <= bound:
            bad.append((k, err, bound))
        assert moved > 100 * bound, (k, 'the third iterate cannot be told from the first')
    assert not bad, bad


def test_unet_two_forwards_then_both_backwards():
    """Forward A, forward B, backward of A, backward of B: each backward uses the W, u, v, sigma of its own forward
    (the ESRGAN generator half runs net_d(gt).detach() and net_d(output) before its backward)."""
    sd, xa, da, _, _ = _case(8, SHAPE)
    g = torch.Generator().manual_seed(77)
    xb, db = torch.rand(SHAPE, generator=g), torch.randn(da.shape, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        net = R.stock_like(sd, 3, 8, dt).train()
        params = dict(net.named_parameters())
        oa, ob = net(xa.to(dt)), net(xb.to(dt))
        refs[dt] = [dict(zip(params, torch.autograd.grad(o, list(params.values()), d.to(dt))))
                    for o, d in ((oa, da), (ob, db))]
    hip = _build(sd, 8).train()
    oa, ob = hip(xa.cuda()), hip(xb.cuda())
    bad = []
    for i, (o, d) in enumerate(((oa, da), (ob, db))):
        hip.zero_grad(set_to_none=True)
        o.backward(d.cuda())
        for k, p in hip.named_parameters():
            ref = refs[torch.float64][i][k]
            err, bound = _l2(p.grad.cpu(), ref), 8 * _l2(refs[torch.float32][i][k], ref)
            other = _l2(refs[torch.float64][1 - i][k], ref)
            print(f'unet backward of forward {"AB"[i]} {k}: rel-L2 {err:.3e}, bound {bound:.3e}; the other forward\'s '
                  f'gradient is {other:.3e} away')
            if not err <= bound:
                bad.append((i, k, err, bound))
    assert not bad, bad


def test_unet_refuses_sizes_and_channels():
    sd, _, _, _, _ = _case(8, SHAPE)
    net = _build(sd, 8)
    for hw in ((36, 32), (32, 20)):
        with pytest.raises(ValueError, match='multiples of 8'):
            net(torch.zeros(1, 3, *hw, device='cuda'))
    with pytest.raises(ValueError, match=r'\(1, 1, 32, 32\)'):
        net(torch.zeros(1, 1, 32, 32, device='cuda'))


def test_unet_deepcopy_after_forward_and_checkpoint_round_trip(tmp_path):
    sd, x, dout, _, _ = _case(8, SHAPE)
    net = _build(sd, 8)
    net(x.cuda()).backward(dout.cuda())
    cp = copy.deepcopy(net)
    for (k, a), (k2, b) in zip(net.state_dict().items(), cp.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(_bits(net.eval()(x.cuda())), _bits(cp.eval()(x.cuda())))
    # a checkpoint in the reference's format, written from the stock module, loads strictly, and back
    path = tmp_path / 'net_d_5000.pth'
    torch.save({'params': R.he_init_sn(R.StockUNetSN(3, 8), seed=3).state_dict()}, path)
    net2 = _build(torch.load(path, weights_only=True)['params'], 8)
    R.StockUNetSN(3, 8).load_state_dict({k: v.cpu() for k, v in net2.state_dict().items()}, strict=True)


def test_unet_memory_does_not_grow():
    """torch.cuda.memory_allocated() is the same after step 3 and step 10 of forward + backward."""
    sd, x, dout, _, _ = _case(8, SHAPE)
    net = _build(sd, 8)
    xc, dc = x.cuda(), dout.cuda()
    seen = {}
    for step in range(1, 11):
        net.zero_grad(set_to_none=True)
        net(xc).backward(dc)
        torch.cuda.synchronize()
        seen[step] = torch.cuda.memory_allocated()
    print(f'memory after step 3: {seen[3]}, after step 10: {seen[10]}')
    assert seen[3] == seen[10]
