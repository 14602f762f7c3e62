"""EDVR on the HIP engine against the same network in stock torch ops in float64 on the CPU (tests/_edvr_ref.py),
loaded strictly from the same state dict: the output and every parameter gradient.  The gradient of the input frames
is not compared: the x4 bilinear skip (``bilinear_up_add``) refuses it.

Bounds, by the network convention of tests/test_discriminator_gpu.py: fp32 within 8 x the rel-L2 error of the stock
tree run in fp32 on the CPU, bf16 within 2 x the rel-L2 error of a float64 run whose conv / DCN weights, stored
activations, DCN columns and gradient maps are rounded to bf16; both measured against the float64 run, never against
the HIP result.  The ``conv_offset`` weights are small random values (std 0.01) instead of the zero init, so the
deformable convs sample off the grid.  Each measured error is printed beside its bound."""
import functools

import pytest
import torch

from . import _edvr_ref as R
from ._fp64 import _ids

pytestmark = pytest.mark.gpu

CASES = {
    'fused64': (dict(num_feat=64, deformable_groups=8, num_frame=3, num_extract_block=1, num_reconstruct_block=1), 16),
    'general16': (dict(num_feat=16, deformable_groups=2, num_frame=5, center_frame_idx=1, num_extract_block=1,
                       num_reconstruct_block=1), 16),
    'wotsa': (dict(num_feat=16, deformable_groups=2, num_frame=3, num_extract_block=1, num_reconstruct_block=1,
                   with_tsa=False), 16),
    'predeblur_hr': (dict(num_feat=16, deformable_groups=2, num_frame=3, num_extract_block=1, num_reconstruct_block=1,
                          with_predeblur=True, hr_in=True), 32),
}


def _l2(a, b):
    return (a.double() - b.double()).norm().item() / max(1e-300, b.double().norm().item())


def _run_stock(net, x, dout, grads):
    out = net(x.to(next(net.parameters()).dtype))
    res = {'out': out.detach()}
    if grads:
        out.backward(dout.to(out.dtype))
        for k, p in net.named_parameters():
            res['grad.' + k] = p.grad
    return res


@functools.lru_cache(None)
def _case(name, grads=True):
    """The state dict, inputs, the float64 results and the two bounds per quantity; computed once and shared."""
    cfg, size = CASES[name]
    sd = R.init_edvr(R.StockEDVR(**cfg), seed=len(name)).state_dict()
    g = torch.Generator().manual_seed(size + len(name))
    x = torch.rand(1, cfg['num_frame'], 3, size, size, generator=g)
    hr = size if cfg.get('hr_in') else 4 * size
    dout = torch.randn(1, 3, hr, hr, generator=g)
    runs = {'f64': _run_stock(R.stock_like(sd, cfg, torch.float64), x, dout, grads),
            'f32': _run_stock(R.stock_like(sd, cfg, torch.float32), x, dout, grads),
            'emu': _run_stock(R.stock_like(sd, cfg, torch.float64, emulate=True), x, dout, grads)}
    ref = runs['f64']
    bounds = {k: {torch.float32: 8 * _l2(runs['f32'][k], ref[k]), torch.bfloat16: 2 * _l2(runs['emu'][k], ref[k])}
              for k in ref}
    return sd, x, dout, ref, bounds


def _run_hip(name, sd, x, dout, dtype, grads=True):
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='EDVR', **CASES[name][0])).cuda()
    net.load_state_dict(sd, strict=True)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        out = net(x.cuda())
    assert out.shape == dout.shape and out.dtype == torch.float32
    res = {'out': out.detach()}
    if grads:
        out.backward(dout.cuda())
        for k, p in net.named_parameters():
            assert p.grad is not None and p.grad.dtype == torch.float32, k
            res['grad.' + k] = p.grad
    return res


def _compare(got, ref, bounds, dtype, what):
    bad = []
    for k in ref:
        err, bound = _l2(got[k].cpu(), ref[k]), bounds[k][dtype]
        print(f'{what} [{_ids(dtype)}] {k}: rel-L2 {err:.3e}, bound {bound:.3e}, ratio {err / max(bound, 1e-300):.3f}')
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=_ids)
def test_edvr_fused_dcn_path(dtype):
    """num_feat 64, 8 deformable groups, 3 frames, TSA: the shapes of the fused DCN kernels (bf16) and of the
    im2col + GEMM path (fp32)."""
    sd, x, dout, ref, bounds = _case('fused64')
    _compare(_run_hip('fused64', sd, x, dout, dtype), ref, bounds, dtype, 'edvr fused64')


@pytest.mark.parametrize('name', ['general16', 'wotsa'])
def test_edvr_general_path(name):
    """16 features / 2 deformable groups: 5 frames with the centre frame at index 1, and the plain 1 x 1 fusion."""
    sd, x, dout, ref, bounds = _case(name)
    _compare(_run_hip(name, sd, x, dout, torch.float32), ref, bounds, torch.float32, f'edvr {name}')


def test_edvr_predeblur_hr_in_forward():
    sd, x, dout, ref, bounds = _case('predeblur_hr', False)
    got = _run_hip('predeblur_hr', sd, x, dout, torch.float32, grads=False)
    _compare(got, ref, bounds, torch.float32, 'edvr predeblur_hr')


def test_edvr_size_assert():
    from basicsr4rs_amd.archs import build_network
    net = build_network(dict(type='EDVR', **CASES['wotsa'][0])).cuda()
    with pytest.raises(AssertionError, match='multiple of 4'):
        net(torch.zeros(1, 3, 3, 18, 16, device='cuda'))
