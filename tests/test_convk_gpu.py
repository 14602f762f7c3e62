"""k x k convolution kernels (csrc/convk.hip) against torch on the CPU in float64, on operands already
rounded to the dtype under test: forward, input gradient (the same kernel on the flipped weight
image), weight / bias gradient, the accumulate bit, run-to-run determinism, NaN containment and the
k = 3 cross-check against conv3x3.  Bounds: tests/test_conv_gpu.py's (forward / dgrad bf16 2e-2, f32
1e-5 of max(1, max|ref|); wgrad bf16 1e-3 * max|ref| + 1e-3, f32 2e-5 * max|ref| + 1e-4)."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

KS = (3, 5, 7, 9)
CH = ((4, 64), (64, 32), (32, 6), (64, 64))
SHAPES = ((1, 1, 1), (2, 3, 5), (2, 17, 33), (1, 40, 70))
DTYPES = (torch.bfloat16, torch.float32)


def _pad8(c):
    return (c + 7) // 8 * 8


def _nhwc(t, cp, dtype, dev):
    """NCHW float64 CPU -> NHWC [N, H, W, cp] of dtype on the device (padded channels zero)."""
    N, C, H, W = t.shape
    out = torch.zeros(N, H, W, cp, dtype=dtype)
    out[..., :C] = t.permute(0, 2, 3, 1).to(dtype)
    return out.to(dev)


def _case(k, cin, cout, N, H, W, dtype, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + k * 131 + cin * 17 + cout + N * 3 + H * 5 + W)
    x = torch.randn(N, cin, H, W, generator=g).to(dtype).double()
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k)**0.5).to(dtype).double()
    b = torch.randn(cout, generator=g).float().double()
    dy = torch.randn(N, cout, H, W, generator=g).to(dtype).double()
    return x, w, b, dy


def _images(w, b, dtype, dev):
    from basicsr4rs_amd.ops import conv as C
    cout, cin, k, _ = w.shape
    wp = w.float().to(dev).contiguous()
    bp = b.float().to(dev).contiguous()
    wf, wd, bg = C.prepared_images(wp, bp, dtype, (cout, cin, _pad8(cout), _pad8(cin), 0, k))
    return wf, wd, bg, (wp, bp)


@pytest.mark.parametrize('dtype', DTYPES, ids=('bf16', 'f32'))
@pytest.mark.parametrize('cin,cout', CH)
@pytest.mark.parametrize('k', KS)
def test_convk_fwd_dgrad_wgrad(cuda, k, cin, cout, dtype):
    """All four shapes of one (k, channels, dtype) combination: forward with ReLU and without, input
    gradient, weight / bias gradient, accumulate and determinism."""
    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import convk as K
    ftol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    wrel, wabs = (1e-3, 1e-3) if dtype == torch.bfloat16 else (2e-5, 1e-4)
    cin_p, cout_p = _pad8(cin), _pad8(cout)
    for (N, H, W) in SHAPES:
        x, w, b, dy = _case(k, cin, cout, N, H, W, dtype)
        wf, wd, bg, keep = _images(w, b, dtype, cuda)
        xg, dyg = _nhwc(x, cin_p, dtype, cuda), _nhwc(dy, cout_p, dtype, cuda)
        tag = f'k{k} {cin}->{cout} {N}x{H}x{W} {dtype}'
        # forward
        for act in (_lib.ACT_NONE, _lib.ACT_RELU):
            ref = F.conv2d(x, w, b, padding=k // 2)
            if act:
                ref = ref.relu()
            y = K.convk_fwd_raw(xg, wf, bg, k, cout_p, cout, act=act)
            y2 = K.convk_fwd_raw(xg, wf, bg, k, cout_p, cout, act=act)
            assert torch.equal(y, y2), tag
            yc = y.cpu().double()
            assert float(yc[..., cout:].abs().max()) == 0.0 if cout_p > cout else True, tag
            err = (yc[..., :cout].permute(0, 3, 1, 2) - ref).abs().max().item()
            bound = ftol * max(1.0, ref.abs().max().item())
            print(f'{tag} fwd act{act}: err {err:.3e} bound {bound:.3e}')
            assert err <= bound, tag
        # input gradient: conv of dy with the flipped, transposed weight
        ref_dx = F.conv_transpose2d(dy, w, padding=k // 2)
        dx = K.convk_fwd_raw(dyg, wd, None, k, cin_p, cin).cpu().double()
        if cin_p > cin:
            assert float(dx[..., cin:].abs().max()) == 0.0, tag
        err = (dx[..., :cin].permute(0, 3, 1, 2) - ref_dx).abs().max().item()
        bound = ftol * max(1.0, ref_dx.abs().max().item())
        print(f'{tag} dgrad: err {err:.3e} bound {bound:.3e}')
        assert err <= bound, tag
        # weight / bias gradient
        ref_dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=k // 2)
        ref_db = dy.sum(dim=(0, 2, 3))
        dw, db = K.convk_wgrad_raw(dyg, xg, k, cin, cout)
        dw2, db2 = K.convk_wgrad_raw(dyg, xg, k, cin, cout)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), tag
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (cout, cin, k, k)
        ew = (dw.cpu().double() - ref_dw).abs().max().item()
        eb = (db.cpu().double() - ref_db).abs().max().item()
        bw = wrel * ref_dw.abs().max().item() + wabs
        bb = wrel * ref_db.abs().max().item() + wabs
        print(f'{tag} wgrad: dw err {ew:.3e} bound {bw:.3e}; db err {eb:.3e} bound {bb:.3e}')
        assert ew <= bw and eb <= bb, tag


@pytest.mark.parametrize('dtype', DTYPES, ids=('bf16', 'f32'))
def test_convk_wgrad_accumulate_doubles(cuda, dtype):
    """accumulate bit 0: a second call adds into dw / db in place (scale applies to the new term)."""
    import ctypes

    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import convk as K
    k, cin, cout, (N, H, W) = 5, 64, 32, (2, 17, 33)
    x, w, b, dy = _case(k, cin, cout, N, H, W, dtype, seed=1)
    xg, dyg = _nhwc(x, cin, dtype, cuda), _nhwc(dy, cout, dtype, cuda)
    dw, db = K.convk_wgrad_raw(dyg, xg, k, cin, cout)
    lib = _lib.load()
    d = K._kdesc(dtype, N, H, W, k, cin, cin, cout, cout, scale=1.0, accumulate=1)
    nbytes = lib.sr_convk_wgrad_workspace(d)
    ws = torch.empty(nbytes // 4, device=cuda)
    acc_w, acc_b = dw.clone(), db.clone()
    _lib.check(lib.sr_convk_wgrad(ctypes.byref(d), _lib.ptr(dyg), _lib.ptr(xg), _lib.ptr(ws), nbytes, _lib.ptr(acc_w),
                                  _lib.ptr(acc_b), _lib.stream()))
    assert torch.equal(acc_w, dw * 2) and torch.equal(acc_b, db * 2)
    d.scale = 0.5
    d.accumulate = 0
    _lib.check(lib.sr_convk_wgrad(ctypes.byref(d), _lib.ptr(dyg), _lib.ptr(xg), _lib.ptr(ws), nbytes, _lib.ptr(acc_w),
                                  _lib.ptr(acc_b), _lib.stream()))
    assert torch.equal(acc_w, dw * 0.5) and torch.equal(acc_b, db * 0.5)


@pytest.mark.parametrize('dtype', DTYPES, ids=('bf16', 'f32'))
def test_convk_nan_containment(cuda, dtype):
    """One NaN input pixel of image 0 makes exactly the 9 x 9 window of outputs around it (clipped to
    the image) non-finite; nothing in image 1."""
    from basicsr4rs_amd.ops import convk as K
    k, cin, cout, (N, H, W) = 9, 4, 64, (2, 17, 33)
    x, w, b, _ = _case(k, cin, cout, N, H, W, dtype, seed=2)
    wf, _, bg, keep = _images(w, b, dtype, cuda)
    for (py, px) in ((2, 30), (16, 0), (8, 16)):
        xb = x.clone()
        xb[0, 1, py, px] = float('nan')
        y = K.convk_fwd_raw(_nhwc(xb, 8, dtype, cuda), wf, bg, k, cout, cout).cpu().float()
        bad = ~torch.isfinite(y)  # [N, H, W, C]
        want = torch.zeros(N, H, W, dtype=torch.bool)
        want[0, max(0, py - 4):py + 5, max(0, px - 4):px + 5] = True
        assert not bad[1].any()
        assert torch.equal(bad.all(dim=-1), want), (py, px)
        assert torch.equal(bad.any(dim=-1), want), (py, px)


@pytest.mark.parametrize('dtype', DTYPES, ids=('bf16', 'f32'))
def test_convk_k3_matches_conv3x3(cuda, dtype):
    from torch import nn

    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import conv as C
    from basicsr4rs_amd.ops import convk as K
    torch.manual_seed(3)
    conv = nn.Conv2d(64, 32, 3, 1, 1).to(cuda)
    x = torch.randn(2, 17, 33, 64, device=cuda).to(dtype)
    with torch.no_grad():
        a = K.convk(x, conv, act=_lib.ACT_RELU).float()
        r = C.conv3x3(x, conv, act=_lib.ACT_RELU).float()
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    assert (a - r).abs().max().item() <= tol * max(1.0, r.abs().max().item())


def test_convk_autograd_matches_torch(cuda):
    """The autograd op end to end in f32: gradients of x, weight and bias against torch autograd in float64."""
    from torch import nn

    from basicsr4rs_amd import _lib
    from basicsr4rs_amd.ops import convk as K
    torch.manual_seed(4)
    conv = nn.Conv2d(12, 20, 7, 1, 3)
    x = torch.randn(2, 12, 9, 11)
    ref_c = nn.Conv2d(12, 20, 7, 1, 3).double()
    ref_c.load_state_dict(conv.state_dict())
    xr = x.double().requires_grad_(True)
    yr = ref_c(xr).relu()
    gy = torch.randn(yr.shape, dtype=torch.float64)
    yr.backward(gy)
    conv = conv.to(cuda)
    xg = _nhwc(x.double(), 16, torch.float32, cuda).requires_grad_(True)
    y = K.convk(xg, conv, act=_lib.ACT_RELU)
    y.backward(_nhwc(gy, 24, torch.float32, cuda))
    for got, ref in ((y[..., :20].permute(0, 3, 1, 2), yr), (xg.grad[..., :12].permute(0, 3, 1, 2), xr.grad),
                     (conv.weight.grad, ref_c.weight.grad), (conv.bias.grad, ref_c.bias.grad)):
        err = (got.detach().cpu().double() - ref.detach()).abs().max().item()
        assert err <= 2e-5 * ref.abs().max().item() + 1e-4, err
