"""sr_bicubic_up against F.interpolate(mode='bicubic', align_corners=True) on the CPU in float64."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

CASES = ((2, 4, 1, 1, 4), (2, 6, 2, 3, 3), (1, 4, 7, 9, 4), (2, 3, 5, 4, 2), (1, 4, 16, 16, 1))


@pytest.mark.parametrize('N,C,H,W,s', CASES)
def test_bicubic_up_matches_interpolate(cuda, N, C, H, W, s):
    from basicsr4rs_amd.ops import convk as K
    g = torch.Generator().manual_seed(N * 1000 + C * 100 + H * 10 + W + s)
    x = torch.rand(N, C, H, W, generator=g) * 2.2 - 1.1
    ref = F.interpolate(x.double(), scale_factor=s, mode='bicubic', align_corners=True)
    cp = (C + 7) // 8 * 8
    y32 = K.bicubic_up(x.to(cuda), s, torch.float32)
    assert tuple(y32.shape) == (N, H * s, W * s, cp) and y32.dtype == torch.float32
    got = y32.cpu()
    assert float(got[..., C:].abs().max()) == 0.0
    err = (got[..., :C].permute(0, 3, 1, 2).double() - ref).abs().max().item()
    print(f'bicubic {N}x{C}x{H}x{W} x{s}: fp32 err {err:.3e}')
    assert err <= 1e-5 * max(1.0, ref.abs().max().item())
    # bf16 output: the fp32 result rounded to bf16, within one bf16 ulp
    y16 = K.bicubic_up(x.to(cuda), s, torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and tuple(y16.shape) == tuple(y32.shape)
    b = y16.cpu()
    assert float(b[..., C:].float().abs().max()) == 0.0
    want = got.to(torch.bfloat16)
    _, e = torch.frexp(want.float())  # |want| in [2^(e-1), 2^e): one bf16 ulp (8 significand bits) = 2^(e-8)
    ulp = torch.ldexp(torch.ones_like(got), e - 8)
    assert bool(((b.float() - want.float()).abs() <= ulp).all())


def test_bicubic_up_refuses_requires_grad(cuda):
    from basicsr4rs_amd.ops import convk as K
    x = torch.rand(1, 4, 4, 4, device=cuda, requires_grad=True)
    with pytest.raises(NotImplementedError, match='gradient'):
        K.bicubic_up(x, 4, torch.bfloat16)
