"""sr_bicubic_up_hp against F.interpolate(mode='bicubic') (align_corners=False) on the CPU in float64,
with the bound of tests/test_bicubic_gpu.py, and its write into a channel range of a wider tensor."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

CASES = ((1, 3, 1, 1, 2), (2, 3, 2, 3, 2), (1, 3, 7, 9, 2), (1, 1, 5, 4, 3), (1, 3, 16, 16, 1))


def _x(N, C, H, W, s):
    g = torch.Generator().manual_seed(N * 1000 + C * 100 + H * 10 + W + s)
    return torch.rand(N, C, H, W, generator=g) * 2.2 - 1.1


@pytest.mark.parametrize('N,C,H,W,s', CASES)
def test_bicubic_up_hp_matches_interpolate(cuda, N, C, H, W, s):
    from basicsr4rs_amd.ops import convk as K
    x = _x(N, C, H, W, s)
    ref = F.interpolate(x.double(), scale_factor=s, mode='bicubic')
    y = K.bicubic_up_hp(x.to(cuda), s)
    assert tuple(y.shape) == (N, C, H * s, W * s) and y.dtype == torch.float32 and y.is_contiguous()
    err = (y.cpu().double() - ref).abs().max().item()
    print(f'bicubic hp {N}x{C}x{H}x{W} x{s}: fp32 err {err:.3e}, max |ref| {ref.abs().max().item():.3f}')
    assert err <= 1e-5 * max(1.0, ref.abs().max().item())
    if s == 1:
        assert torch.equal(y.cpu(), x)  # phase 0 of scale 1: the weights are (0, 1, 0, 0)


def test_bicubic_up_hp_writes_channel_range_only(cuda):
    from basicsr4rs_amd.ops import convk as K
    N, C, H, W, s = 2, 3, 7, 9, 2
    x = _x(N, C, H, W, s)
    ref = F.interpolate(x.double(), scale_factor=s, mode='bicubic')
    sentinel = torch.full((N, 6, H * s, W * s), -123.456, device=cuda)
    before = sentinel.cpu().clone()
    out = K.bicubic_up_hp(x.to(cuda), s, out=sentinel, c0=3)
    assert out is sentinel
    got = sentinel.cpu()
    assert torch.equal(got[:, :3], before[:, :3])  # bitwise untouched
    err = (got[:, 3:].double() - ref).abs().max().item()
    assert err <= 1e-5 * max(1.0, ref.abs().max().item())
    # the lower range of the same tensor, leaving the upper one as it now is
    K.bicubic_up_hp(x.to(cuda), s, out=sentinel, c0=0)
    again = sentinel.cpu()
    assert torch.equal(again[:, 3:], got[:, 3:]) and torch.equal(again[:, :3], got[:, 3:])
    with pytest.raises(RuntimeError, match='c0'):
        K.bicubic_up_hp(x.to(cuda), s, out=sentinel, c0=4)


def test_bicubic_up_hp_refuses_requires_grad(cuda):
    from basicsr4rs_amd.ops import convk as K
    x = torch.rand(1, 3, 4, 4, device=cuda, requires_grad=True)
    with pytest.raises(NotImplementedError, match='gradient'):
        K.bicubic_up_hp(x, 2)
