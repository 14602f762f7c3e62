"""Host-side checks of the UNetDiscriminatorSN work (no GPU): the parameter modules against a stock module built
from the reference's layer list with torch's ``spectral_norm``, the reference's Real-ESRGAN option file (stored
unchanged under tests/golden/reference_options/, read as data), the float64 helper formulas of tests/_unet_ref.py
against torch autograd, and that the exact-grid inputs of the GPU tests really are exact."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F
import yaml

from . import _unet_ref as R
from ._exact import gen_for, grid
from ._fp64 import _rne_bf16

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_options')


def _build(nf, **kw):
    from basicsr4rs_amd.archs import build_network
    return build_network(dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=nf, **kw))


@pytest.mark.parametrize('nf', [8, 64])
def test_state_dict_matches_stock_and_deepcopies(nf):
    net, stock = _build(nf), R.he_init_sn(R.StockUNetSN(3, nf), seed=nf)
    a, b = net.state_dict(), stock.state_dict()
    assert list(a) == list(b)
    assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
    assert any(k.endswith('weight_orig') for k in a) and any(k.endswith('weight_u') for k in a)
    net.load_state_dict(b, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, b[k]), k
    R.StockUNetSN(3, nf).load_state_dict(net.state_dict(), strict=True)
    if nf == 64:
        assert sum(p.numel() for p in net.parameters()) == 4376897
    cp = copy.deepcopy(net)
    for (k, v), (k2, v2) in zip(net.state_dict().items(), cp.state_dict().items()):
        assert k == k2 and torch.equal(v, v2) and v.data_ptr() != v2.data_ptr()


def test_num_feat_refused():
    for nf in (12, 72):
        with pytest.raises(ValueError, match='multiple of 8 up to 64'):
            _build(nf)


def test_reference_yaml_network_d_builds():
    from basicsr4rs_amd.archs import build_network
    with open(os.path.join(REF, 'train', 'RealESRGAN', 'train_realesrgan_x4plus.yml')) as f:
        opt = yaml.safe_load(f)
    assert opt['network_d']['type'] == 'UNetDiscriminatorSN'
    net = build_network(dict(opt['network_d']))
    assert type(net).__name__ == 'UNetDiscriminatorSN' and net.skip_connection is True
    assert sum(p.numel() for p in net.parameters()) == 4376897


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-300)


@pytest.mark.parametrize('R_,K', [(16, 128), (24, 216)])
def test_spectral_norm_formulas_match_torch(R_, K):
    """The power iteration, sigma, W, the updated buffers and the backward formula against torch's spectral_norm and
    autograd in float64."""
    g = gen_for(f'sn{R_}x{K}')
    cin = K // 9 if K % 9 == 0 else K // 16
    k = 3 if K % 9 == 0 else 4
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, R_, k, bias=False)).double()
    with torch.no_grad():
        conv.weight_orig.copy_(torch.randn(conv.weight_orig.shape, generator=g, dtype=torch.float64))
    M, u0, v0 = conv.weight_orig.detach().reshape(R_, K).clone(), conv.weight_u.clone(), conv.weight_v.clone()
    u, v, sigma, W = R.power_iteration(M, u0, v0)
    conv.train()
    x = torch.randn(2, cin, 6, 6, generator=g, dtype=torch.float64)
    y = conv(x)
    errs = {'u': _rel(u, conv.weight_u), 'v': _rel(v, conv.weight_v), 'W': _rel(W, conv.weight.detach().reshape(R_, K))}
    dout = torch.randn(y.shape, generator=g, dtype=torch.float64)
    Wl = conv.weight.detach().clone().requires_grad_(True)
    F.conv2d(x, Wl).backward(dout)
    y.backward(dout)
    errs['dweight_orig'] = _rel(R.sn_backward(Wl.grad.reshape(R_, K), W, u, v, sigma),
                                conv.weight_orig.grad.reshape(R_, K))
    conv.eval()
    ue, ve, se, We = R.power_iteration(M, u, v, iterate=False)
    conv(x)
    errs['W eval'] = _rel(We, conv.weight.detach().reshape(R_, K))
    assert torch.equal(ue, u) and torch.equal(ve, v)
    for k_, e in errs.items():
        print(f'sn formulas ({R_}, {K}) {k_}: rel {e:.3e}, bound 1e-12')
        assert e <= 1e-12, (k_, e)


def test_bilinear_formulas_match_torch():
    g = gen_for('up2')
    for shape in ((2, 3, 5, 3), (1, 2, 1, 1), (1, 1, 1, 4), (1, 1, 6, 1)):
        x = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        e1, e2 = _rel(R.up2(x.detach()), y.detach()), _rel(R.up2_t(dy), x.grad)
        print(f'bilinear formulas {shape}: forward rel {e1:.3e}, transpose rel {e2:.3e}, bound 1e-12')
        assert e1 <= 1e-12 and e2 <= 1e-12


def test_bilinear_exact_grids_are_exact():
    """Integer grids, |x| <= 8 forward and |dy| <= 2 backward: F.interpolate and its gradient in float32 equal float64
    bit for bit, and the float64 results are bf16 values; the tap weights are k / 16 and sum to 4 per input pixel."""
    g = gen_for('up2 grids')
    for shape in ((1, 8, 1, 1), (1, 8, 1, 5), (2, 24, 2, 1), (1, 8, 3, 5), (2, 40, 7, 6)):
        x = grid(shape, -8, 8, gen=g)
        dy = grid(shape[:2] + (2 * shape[2], 2 * shape[3]), -2, 2, gen=g)
        res = {}
        for dt in (torch.float64, torch.float32):
            xx = x.to(dt).clone().requires_grad_(True)
            y = F.interpolate(xx, scale_factor=2, mode='bilinear', align_corners=False)
            y.backward(dy.to(dt))
            res[dt] = (y.detach().double(), xx.grad.double())
        for a, b, ours, what in zip(res[torch.float64], res[torch.float32], (R.up2(x), R.up2_t(dy)), ('y', 'dx')):
            assert torch.equal(a, b), (shape, what)
            assert torch.equal(a, ours), (shape, what)
            assert torch.equal(_rne_bf16(a), a), (shape, what, 'not a bf16 value')
            assert torch.equal(a * 16, torch.round(a * 16)), (shape, what)
        ones = torch.ones(shape[:2] + (2 * shape[2], 2 * shape[3]), dtype=torch.float64)
        assert torch.equal(R.up2_t(ones), torch.full(shape, 4.0, dtype=torch.float64))


def test_cpu_tensors_refused():
    from basicsr4rs_amd.ops import gan as G
    net = _build(8)
    with pytest.raises(NotImplementedError, match='need tensors on the MI355X'):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match='need tensors on the MI355X'):
        G.bilinear_up2(torch.zeros(1, 2, 2, 8))
    with pytest.raises(NotImplementedError, match='need tensors on the MI355X'):
        G.spectral_norm_group([net.conv1], True)
    with pytest.raises(NotImplementedError, match='need tensors on the MI355X'):
        G.conv4s2(torch.zeros(1, 4, 4, 8), net.conv1, act=2, weight=net.conv1.weight_orig)


def test_sn_problem_layout_matches_header():
    """Field order, kind and size of the ctypes mirror of sr_sn_problem (8-byte pointers, 4-byte ints)."""
    import ctypes
    import re

    from basicsr4rs_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'sr_hip.h')).read(), flags=re.S)
    body = re.search(r'typedef struct sr_sn_problem \{(.*?)\}', src, re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ptr = '*' in decl
        names = decl.replace('*', ' ').split()[-1] if ptr else decl.split(None, 1)[1]
        fields += [(n.strip(), ptr) for n in names.split(',')]
    assert [f[0] for f in _lib.SnProblem._fields_] == [n for n, _ in fields]
    assert [f[1] is ctypes.c_void_p for f in _lib.SnProblem._fields_] == [p for _, p in fields]
    assert ctypes.sizeof(_lib.SnProblem) == 8 * sum(p for _, p in fields) + 4 * sum(not p for _, p in fields)
    assert int(re.search(r'#define SR_SN_MAX_PROBLEMS (\d+)', src).group(1)) == _lib.SN_MAX_PROBLEMS


def test_library_refuses_bad_spectral_norm_and_bilinear_arguments():
    import ctypes

    from basicsr4rs_amd import _lib
    lib = _lib.load()
    ok, odd = ctypes.c_void_p(64), ctypes.c_void_p(72)
    assert lib.sr_bilinear_up2_fwd(0, odd, 1, 2, 2, 8, ok, None) == -1
    assert b'bilinear_up2_fwd: tensors must be 16-byte aligned' in lib.sr_last_error()
    assert lib.sr_bilinear_up2_bwd(1, ok, 1, 2, 2, 12, ok, None) == -1
    assert b'C a multiple of 8' in lib.sr_last_error()
    p = (_lib.SnProblem * 1)()
    p[0].w = p[0].u = p[0].v = p[0].u_fwd = p[0].v_fwd = p[0].sigma = p[0].out = 64
    p[0].R, p[0].K = 8, 72
    need = lib.sr_spectral_norm_workspace(p, 1)
    assert need >= 4 * (72 + 8)
    assert lib.sr_spectral_norm_fwd(p, 1, 1, 1e-12, ok, need - 4, None) == -1
    assert b'workspace smaller' in lib.sr_last_error()
    assert lib.sr_spectral_norm_fwd(p, 0, 1, 1e-12, ok, need, None) == -1
    assert lib.sr_conv4s2_fwd_act(0, ok, ok, 1, 4, 4, 8, 8, 1, 0.2, ok, None) == -1
    assert b'act must be none (0) or LeakyReLU (2)' in lib.sr_last_error()
