"""VGGStyleDiscriminator on the HIP engine against the same network in stock nn modules in float64 on the CPU,
loaded strictly from the same state dict.

Bounds, by the convention of tests/test_perceptual_gpu.py::_measure: fp32 within 8 x the rel-L2 error of the
stock network run in fp32 on the CPU, bf16 within 2 x the rel-L2 error of a float64 run whose conv weights and
stored activations (and gradient maps) are rounded to bf16; both measured here against the float64 run, never
against the HIP result.  Each measured error is printed beside its bound."""
import functools

import pytest
import torch

from ._fp64 import _ids
from ._gan_ref import Store, StockDiscriminator, he_init, stock_like

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _run_stock(net, x, dout, train=True, grads=True):
    """logits, input gradient, parameter gradients and running statistics of one forward (+ backward)."""
    net.train(train)
    xx = x.to(next(net.parameters()).dtype).clone().requires_grad_(grads)
    out = net(xx)
    res = {'logits': out.detach()}
    if grads:
        out.backward(dout.to(out.dtype))
        res['dx'] = xx.grad
        for k, p in net.named_parameters():
            res['grad.' + k] = p.grad
    for k, b in net.named_buffers():
        if b.is_floating_point():
            res['buf.' + k] = b.detach().clone()
    return res


@functools.lru_cache(None)
def _case(nf, size, batch, train=True, grads=True):
    """The state dict, inputs, the float64 results and the two bounds per quantity; computed once and shared."""
    sd = he_init(StockDiscriminator(3, nf, size), seed=nf + size).state_dict()
    g = torch.Generator().manual_seed(batch)
    x = torch.rand(batch, 3, size, size, generator=g)
    dout = torch.randn(batch, 1, generator=g)
    runs = {
        'f64': _run_stock(stock_like(sd, 3, nf, size, torch.float64), x, dout, train, grads),
        'f32': _run_stock(stock_like(sd, 3, nf, size, torch.float32), x, dout, train, grads),
        'emu': _run_stock(stock_like(sd, 3, nf, size, torch.float64, round_convs=True, store=Store.apply), x, dout, train,
                          grads),
    }
    ref = runs['f64']
    bounds = {k: {torch.float32: 8 * _l2(runs['f32'][k], ref[k]), torch.bfloat16: 2 * _l2(runs['emu'][k], ref[k])}
              for k in ref}
    return sd, x, dout, ref, bounds


def _build(sd, nf, size):
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=nf, input_size=size)).cuda()
    net.load_state_dict(sd, strict=True)
    return net


def _run_hip(net, x, dout, dtype, train=True, grads=True):
    net.train(train)
    xx = x.cuda().requires_grad_(grads)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        out = net(xx)
    assert out.shape == (x.shape[0], 1) and out.dtype == torch.float32
    res = {'logits': out.detach()}
    if grads:
        out.backward(dout.cuda())
        res['dx'] = xx.grad
        for k, p in net.named_parameters():
            assert p.grad is not None and p.grad.dtype == torch.float32, k
            res['grad.' + k] = p.grad
    for k, b in net.named_buffers():
        if b.is_floating_point():
            res['buf.' + k] = b.detach().clone()
    return res


def _compare(got, ref, bounds, dtype, what):
    bad = []
    for k in ref:
        err, bound = _l2(got[k].cpu(), ref[k]), bounds[k][dtype]
        print(f'{what} [{_ids(dtype)}] {k}: rel-L2 {err:.3e}, bound {bound:.3e}, ratio {err / max(bound, 1e-300):.3f}')
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_discriminator_matches_float64(dtype):
    """(3, 8, 128), batch 2, training mode: logits, the gradient with respect to the input, every parameter
    gradient, and the running statistics after the call."""
    sd, x, dout, ref, bounds = _case(8, 128, 2)
    net = _build(sd, 8, 128)
    got = _run_hip(net, x, dout, dtype)
    _compare(got, ref, bounds, dtype, 'disc 8/128')
    assert all(m.num_batches_tracked.item() == 1 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_discriminator_input_256():
    sd, x, dout, ref, bounds = _case(8, 256, 1)
    got = _run_hip(_build(sd, 8, 256), x, dout, torch.float32)
    _compare(got, ref, bounds, torch.float32, 'disc 8/256')


def test_discriminator_real_channel_counts_forward():
    """num_feat 64 at 128^2, batch 1, forward only: the 64 .. 512 channel convs of the train YAMLs."""
    sd, x, dout, ref, bounds = _case(64, 128, 1, True, False)
    got = _run_hip(_build(sd, 64, 128), x, dout, torch.float32, grads=False)
    _compare(got, ref, bounds, torch.float32, 'disc 64/128')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ids)
def test_discriminator_eval_forward(dtype):
    sd, x, dout, ref, bounds = _case(8, 128, 2, False, False)
    net = _build(sd, 8, 128)
    got = _run_hip(net, x, dout, dtype, train=False, grads=False)
    _compare(got, ref, bounds, dtype, 'disc eval')
    for k, b in net.named_buffers():
        assert torch.equal(b.cpu(), sd[k]), k  # eval leaves the running statistics alone


def test_discriminator_frozen_parameters():
    """With the parameters frozen (the generator half of a GAN step) the input gradient is the same bits and no
    weight-gradient kernel is launched."""
    from basicsr4rs_amd.utils import ktrace
    sd, x, dout, _, _ = _case(8, 128, 2)
    dxs, recs = [], []
    for frozen in (False, True):
        net = _build(sd, 8, 128)
        for p in net.parameters():
            p.requires_grad = not frozen
        xx = x.cuda().requires_grad_(True)
        ktrace.start()
        try:
            net(xx).backward(dout.cuda())
        finally:
            recs.append(ktrace.stop())
        dxs.append(xx.grad.clone())
        assert all((p.grad is None) == frozen for p in net.parameters())
    assert torch.equal(dxs[0], dxs[1])
    assert any('wgrad' in k for k in recs[0]), sorted(recs[0])
    assert not any('wgrad' in k for k in recs[1]), sorted(recs[1])
    assert 'conv4s2_dgrad_kernel' in recs[1] and 'bn_bwd_dx_kernel' in recs[1] and 'fc_dgrad_kernel' in recs[1]


def test_discriminator_refuses_other_sizes():
    sd, _, _, _, _ = _case(8, 128, 2)
    net = _build(sd, 8, 128)
    with pytest.raises(AssertionError, match='Input size must be identical to input_size'):
        net(torch.zeros(1, 3, 64, 64, device='cuda'))
    with pytest.raises(ValueError, match=r'\(1, 1, 128, 128\)'):
        net(torch.zeros(1, 1, 128, 128, device='cuda'))


def test_reference_format_checkpoint_round_trip(tmp_path):
    """A checkpoint in the reference's format ({'params': state_dict}, written from the stock module) loads
    strictly; what this net saves loads strictly into the stock module, tensor for tensor."""
    stock = he_init(StockDiscriminator(3, 8, 128), seed=3)
    path = tmp_path / 'net_d_5000.pth'
    torch.save({'params': stock.state_dict()}, path)
    net = _build(torch.load(path, weights_only=True)['params'], 8, 128)
    back = tmp_path / 'net_d_back.pth'
    torch.save({'params': {k: v.cpu() for k, v in net.state_dict().items()}}, back)
    stock2 = StockDiscriminator(3, 8, 128)
    stock2.load_state_dict(torch.load(back, weights_only=True)['params'], strict=True)
    for (k, a), (k2, b) in zip(stock.state_dict().items(), stock2.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
