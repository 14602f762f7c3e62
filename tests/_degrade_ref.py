"""Float64 restatements of the degradation ops (csrc/degrade.hip), written from the documented behaviour of
``filter2D``, ``USMSharp``, ``F.interpolate``, the ``*_noise_pt`` functions and ``DiffJPEG``; formulas only.  Each
returns the value and the magnitude sums a rounding bound multiplies.  test_degrade_ref_host.py checks them against
torch on the CPU; the GPU tests compare the device with them, never with the code under test."""
import math
from types import SimpleNamespace

import torch

U = 2.0**-24


def reflect_index(n, pad):
    """Source index of every position of an axis of length n reflect-padded by pad (pad < n): -i -> i,
    n - 1 + i -> n - 1 - i."""
    i = torch.arange(-pad, n + pad)
    i = i.abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def round255(v):
    """clamp(rint(255 v), 0, 255) / 255 (rint: half to even) and the distance of 255 v from the nearest
    half-integer (the margin under which an fp32 evaluation rounds the same way)."""
    t = 255.0 * v.double()
    margin = ((t - torch.floor(t)) - 0.5).abs()
    return torch.clamp(torch.round(t), 0, 255) / 255.0, margin


# ------------------------------------------------------------------------------------------------ filter2d


def filter2d(x, kernel):
    """y[n, c, i, j] = sum_ab kernel[n or 0, a, b] x[n, c, r(i + a - p), r(j + b - p)] with r the reflection;
    returns (y, sum of |terms|)."""
    x, kernel = x.double(), kernel.double()
    B, C, H, W = x.shape
    k = kernel.shape[-1]
    p = k // 2
    xp = x[:, :, reflect_index(H, p)][:, :, :, reflect_index(W, p)]
    kb = kernel.expand(B, k, k)
    y, mag = torch.zeros_like(x), torch.zeros_like(x)
    for a in range(k):
        for b in range(k):
            w = kb[:, a, b].view(B, 1, 1, 1)
            t = w * xp[:, :, a:a + H, b:b + W]
            y += t
            mag += t.abs()
    return y, mag


# ------------------------------------------------------------------------------------------ separable blur


def gaussian_taps(radius, sigma=0.0):
    """cv2.getGaussianKernel(radius, sigma) from its definition: sigma <= 0 -> 0.3 ((radius - 1) / 2 - 1) + 0.8."""
    if sigma <= 0:
        sigma = 0.3 * ((radius - 1) * 0.5 - 1) + 0.8
    w = torch.tensor([math.exp(-((i - (radius - 1) / 2)**2) / (2 * sigma * sigma)) for i in range(radius)],
                     dtype=torch.float64)
    return w / w.sum()


def sep_blur(x, taps):
    """The blur by outer(taps, taps), reflect-padded: (blur, sum of |w x|)."""
    taps = taps.double()
    return filter2d(x, torch.outer(taps, taps)[None])


def usm(x, taps, weight=0.5, threshold=10.0):
    """USMSharp: blur, residual = x - blur, mask = |residual| 255 > threshold, soft = blur(mask),
    sharp = clip(x + weight residual, 0, 1), out = soft sharp + (1 - soft) x.  ``margin``: min over pixels of
    ||residual| 255 - threshold|."""
    x = x.double()
    r = SimpleNamespace()
    r.blur, r.blur_mag = sep_blur(x, taps)
    r.res = x - r.blur
    r.margin = ((r.res.abs() * 255.0) - threshold).abs().min().item()
    r.mask = (r.res.abs() * 255.0 > threshold).double()
    r.soft, r.soft_mag = sep_blur(r.mask, taps)
    r.sharp = torch.clamp(x + weight * r.res, 0, 1)
    r.out = r.soft * r.sharp + (1 - r.soft) * x
    return r


# -------------------------------------------------------------------------------------------------- resize

_A = -0.75


def _c1(t):
    return ((_A + 2) * t - (_A + 3)) * t * t + 1


def _c2(t):
    return ((_A * t - 5 * _A) * t + 8 * _A) * t - 4 * _A


def _dc1(t):
    return (3 * (_A + 2) * t - 2 * (_A + 3)) * t


def _dc2(t):
    return (3 * _A * t - 10 * _A) * t + 8 * _A


def resize_axis(n_in, n_out, scale, mode):
    """One axis of F.interpolate(align_corners=False): (M [n_out, n_in] weights, dM = sum of |d weight / d src| placed
    like M, src [n_out], taps).  area: the window [floor(i in / out), ceil((i + 1) in / out)) with equal weights;
    bilinear: src = max(scale (i + 0.5) - 0.5, 0), taps floor(src), min(floor(src) + 1, in - 1); bicubic: src not
    clamped, four taps floor(src) - 1 .. + 2 with clamped indices and the A = -0.75 convolution weights."""
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    dM = torch.zeros(n_out, n_in, dtype=torch.float64)
    src = torch.zeros(n_out, dtype=torch.float64)
    taps = 1
    for i in range(n_out):
        if mode == 'area':
            s, e = (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)
            M[i, s:e] = 1.0 / (e - s)
            taps = max(taps, e - s)
            continue
        s = scale * (i + 0.5) - 0.5
        if mode == 'bilinear':
            s = max(s, 0.0)
            i0 = min(int(math.floor(s)), n_in - 1)
            t = s - i0
            for idx, w, d in ((i0, 1 - t, 1.0), (min(i0 + 1, n_in - 1), t, 1.0)):
                M[i, idx] += w
                dM[i, idx] += d
            taps = 2
        else:
            i0 = int(math.floor(s))
            t = s - i0
            ws = (_c2(t + 1), _c1(t), _c1(1 - t), _c2(2 - t))
            ds = (_dc2(t + 1), _dc1(t), -_dc1(1 - t), -_dc2(2 - t))
            for j in range(4):
                idx = min(max(i0 - 1 + j, 0), n_in - 1)
                M[i, idx] += ws[j]
                dM[i, idx] += abs(ds[j])
            taps = 4
        src[i] = s
    return M, dM, src, taps


def resize(x, out_hw, scales, mode):
    """(y, bound): y = My x Mx^T per plane, and the fp32 bound of the issue: (taps + 2) U sum |w x| plus, for the
    interpolating modes, sum |dw/dt| |x| 4 U max(1, |src|) per axis."""
    x = x.double()
    My, dMy, sy, ty = resize_axis(x.shape[2], out_hw[0], scales[0], mode)
    Mx, dMx, sx, tx = resize_axis(x.shape[3], out_hw[1], scales[1], mode)

    def app(a, v, b):
        return torch.einsum('ih,nchw,jw->ncij', a, v, b)

    y = app(My, x, Mx)
    ax = x.abs()
    bound = (ty * tx + 2) * U * app(My.abs(), ax, Mx.abs())
    if mode != 'area':
        cy = (4 * U * sy.abs().clamp(min=1.0)).view(1, 1, -1, 1)
        cx = (4 * U * sx.abs().clamp(min=1.0)).view(1, 1, 1, -1)
        bound = bound + app(dMy, ax, Mx.abs()) * cy + app(My.abs(), ax, dMx) * cx
    return y, bound


def resize_geometry(n_in, scale_factor=None, size=None):
    """torch's two conventions: scale_factor s -> (floor(in s), 1 / s); size -> (size, in / size)."""
    if scale_factor is not None:
        return int(math.floor(n_in * scale_factor)), 1.0 / scale_factor
    return size, n_in / size


# --------------------------------------------------------------------------------------------------- noise


def gray_of(x):
    return 0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]


def gaussian_noise(img, normal, normal_gray, sigma, gray):
    """clamp(img + (normal sigma / 255) (1 - g) + (normal_gray sigma / 255) g, 0, 1) and the sum of |terms|."""
    img, normal, normal_gray = img.double(), normal.double(), normal_gray.double()
    s = sigma.double().view(-1, 1, 1, 1)
    g = gray.double().view(-1, 1, 1, 1)
    nc = normal * s / 255.0 * (1 - g)
    ng = normal_gray[None, None] * s / 255.0 * g
    return torch.clamp(img + nc + ng, 0, 1), img.abs() + (normal * s / 255.0).abs() + (normal_gray[None, None] * s / 255.0).abs() * g


def poisson_levels(img):
    """Quantised levels of the colour and gray images, the per-sample counts of distinct levels, vals =
    2^ceil(log2(count)), the rates level / 255 vals, and the smallest distance of 255 v from a half-integer."""
    img = img.double()
    r = SimpleNamespace()
    r.qc, mc = round255(img)
    r.qg, mg = round255(gray_of(img))
    r.margin = min(mc.min().item(), mg.min().item())
    B = img.shape[0]
    r.count_c = torch.tensor([r.qc[i].unique().numel() for i in range(B)])
    r.count_g = torch.tensor([r.qg[i].unique().numel() for i in range(B)])
    r.vals = torch.stack([2.0**torch.ceil(torch.log2(r.count_c.double())), 2.0**torch.ceil(torch.log2(r.count_g.double()))], 1)
    r.rate_c = r.qc * r.vals[:, 0].view(-1, 1, 1, 1)
    r.rate_g = r.qg * r.vals[:, 1].view(-1, 1, 1, 1)
    return r


def poisson_noise(img, lv, draw_c, draw_g, scale, gray):
    """clamp(img + ((draw_c / vals_c - q) (1 - g) + (draw_g / vals_g - q_gray) g) scale, 0, 1), sum of |terms|."""
    img = img.double()
    s, g = scale.double().view(-1, 1, 1, 1), gray.double().view(-1, 1, 1, 1)
    vc, vg = lv.vals[:, 0].view(-1, 1, 1, 1), lv.vals[:, 1].view(-1, 1, 1, 1)
    a, b = draw_c.double() / vc, draw_g.double() / vg
    noise = (a - lv.qc) * (1 - g) + (b - lv.qg) * g
    mag = img.abs() + ((a.abs() + lv.qc) * (1 - g) + (b.abs() + lv.qg) * g) * s.abs()
    return torch.clamp(img + noise * s, 0, 1), mag


# ---------------------------------------------------------------------------------------------------- JPEG

Y_TABLE_ROWS = [[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]]
C_CORNER = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]
RGB2YCC = [[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]]
YCC2RGB = [[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]]


def jpeg_tables(dtype=torch.float64):
    """(luminance table as the reference uses it: the standard table transposed; chroma table; DCT matrix
    C[j, u] = cos((2 j + 1) u pi / 16); alpha_u alpha_v), in ``dtype``."""
    yt = torch.tensor(Y_TABLE_ROWS, dtype=torch.float64).t().contiguous()
    ct = torch.full((8, 8), 99.0, dtype=torch.float64)
    ct[:4, :4] = torch.tensor(C_CORNER, dtype=torch.float64).t()
    j = torch.arange(8, dtype=torch.float64)
    cm = torch.cos((2 * j[:, None] + 1) * j[None, :] * math.pi / 16)
    al = torch.tensor([1 / math.sqrt(2)] + [1.0] * 7, dtype=torch.float64)
    return yt.to(dtype), ct.to(dtype), cm.to(dtype), torch.outer(al, al).to(dtype)


def quality_factor(q):
    """quality -> table factor: 5000 / q / 100 below 50, (200 - 2 q) / 100 from 50 (tensor in, tensor out)."""
    return torch.where(q < 50, 5000.0 / q, 200.0 - q * 2) / 100.0


def _blocks(p):
    """[B, H, W] -> [B, H/8, W/8, 8, 8]"""
    B, H, W = p.shape
    return p.reshape(B, H // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4)


def _unblocks(b):
    B, hb, wb = b.shape[:3]
    return b.permute(0, 1, 3, 2, 4).reshape(B, hb * 8, wb * 8)


def jpeg_encode(x, quality, dtype=torch.float64):
    """The pre-round coefficients (Y [B, H16/8, W16/8, 8, 8], Cb, Cr [B, H16/16, W16/16, 8, 8]) of x [B, 3, H, W] at
    ``quality`` [B], every operation in ``dtype`` (float64: the reference; float32: a replay whose distance from it
    is the scale of a correct fp32 kernel's error): zero pad to multiples of 16, x 255, YCbCr, 2 x 2 chroma mean,
    - 128, D = 0.25 alpha_u alpha_v C^T block C, / (table factor)."""
    x = x.to(dtype)
    B, _, H, W = x.shape
    x = torch.nn.functional.pad(x, (0, -W % 16, 0, -H % 16)) * 255
    m = torch.tensor(RGB2YCC, dtype=torch.float64).to(dtype)
    ycc = torch.einsum('kc,nchw->nkhw', m, x)
    ycc[:, 1:] += 128
    yt, ct, cm, al = jpeg_tables(dtype)
    f = quality_factor(quality.to(dtype)).view(B, 1, 1, 1, 1)
    out = []
    for c in range(3):
        p = ycc[:, c]
        if c:
            p = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4
        blk = _blocks(p - 128)
        d = (0.25 * al) * (cm.t() @ blk @ cm)
        out.append(d / ((yt if c == 0 else ct) * f))
    return tuple(out)


def diff_round(v):
    r = torch.round(v)
    return r + (v - r)**3


def jpeg_decode(coefs, quality, H, W):
    """Float64 decode of (rounded) coefficients: x (table factor), alpha, 0.25 C . C^T + 128, chroma replicated 2 x 2,
    YCbCr -> RGB, clamp to [0, 255], / 255, cropped to H x W; and the sum of |terms| of the IDCT and colour
    accumulation, / 255."""
    B = coefs[0].shape[0]
    yt, ct, cm, al = jpeg_tables()
    f = quality_factor(quality.double()).view(B, 1, 1, 1, 1)
    planes, mags = [], []
    for c in range(3):
        deq = coefs[c].double() * ((yt if c == 0 else ct) * f) * al
        p = _unblocks(0.25 * (cm @ deq @ cm.t()) + 128)
        mg = _unblocks(0.25 * (cm.abs() @ deq.abs() @ cm.abs().t()) + 128)
        if c:
            p, mg = (t.repeat_interleave(2, 1).repeat_interleave(2, 2) for t in (p, mg))
        planes.append(p)
        mags.append(mg)
    m = torch.tensor(YCC2RGB, dtype=torch.float64)
    ycc = torch.stack(planes, 1)
    ycc[:, 1:] -= 128
    mag = torch.stack([mags[0], mags[1] + 128, mags[2] + 128], 1)
    rgb = torch.einsum('kc,nchw->nkhw', m, ycc)
    rmag = torch.einsum('kc,nchw->nkhw', m.abs(), mag)
    return (torch.clamp(rgb, 0, 255) / 255)[:, :, :H, :W], (rmag / 255)[:, :, :H, :W]


def jpeg(x, quality, differentiable=False):
    """The whole DiffJPEG forward in float64."""
    pre = jpeg_encode(x, quality)
    rnd = diff_round if differentiable else torch.round
    return jpeg_decode(tuple(rnd(p) for p in pre), quality, x.shape[2], x.shape[3])[0]
