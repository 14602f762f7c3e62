"""Float64 restatements for the EDVR tests, written from the formulas of basicsr/archs/edvr_arch.py and
arch_util.py:237-263 (no reference code is imported): the stride-2 conv and the pooling pair through
torch.nn.functional, the temporal attention and the sigmoid modulation of TSAFusion with their backward formulas by
hand, a differentiable pure-torch modulated deformable conv, and the EDVR module tree in stock torch ops (NCHW) with
an optional ``store`` hook at every place the HIP engine keeps a feature map (the bf16-storage emulation of
tests/test_discriminator_gpu.py).  Checked on the host by tests/test_edvr_ref_host.py."""
import torch
from torch import nn
from torch.nn import functional as F

from ._fp64 import _rne_bf16
from ._gan_ref import Store  # noqa: F401  (re-export: the bf16 store of the emulation runs)

# ------------------------------------------------------------------------------------------------- kernels


def conv3s2(x, w, b=None, slope=None):
    """nn.Conv2d(cin, cout, 3, 2, 1) (+ LeakyReLU(slope)) of an NCHW map."""
    z = F.conv2d(x, w, b, stride=2, padding=1)
    return z if slope is None else torch.where(z > 0, z, z * slope)


def pool3s2(x):
    """cat([MaxPool2d(3, 2, 1), AvgPool2d(3, 2, 1)], channel) of an NCHW map."""
    return torch.cat([F.max_pool2d(x, 3, 2, 1), F.avg_pool2d(x, 3, 2, 1)], 1)


def sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def _frames(t, B):
    """[B * T, H, W, C] -> [B, T, H, W, C]."""
    return t.reshape(B, t.shape[0] // B, *t.shape[1:])


def tsa_corr(emb, emb_ref, aligned):
    """NHWC: emb / aligned [B * T, H, W, C], emb_ref [B, H, W, C] -> (out [B, H, W, T * C], prob [B, T, H, W])."""
    B, H, W, C = emb_ref.shape
    e, a = _frames(emb, B), _frames(aligned, B)
    prob = sigmoid((e * emb_ref[:, None]).sum(-1))
    out = (a * prob[..., None]).permute(0, 2, 3, 1, 4).reshape(B, H, W, -1)
    return out, prob


def tsa_corr_bwd(d_out, emb, emb_ref, aligned, prob):
    """(d_aligned, d_emb, d_emb_ref) of tsa_corr from d_out, by the written-out formulas."""
    B, H, W, C = emb_ref.shape
    e, a = _frames(emb, B), _frames(aligned, B)
    T = e.shape[1]
    g = d_out.reshape(B, H, W, T, C).permute(0, 3, 1, 2, 4)
    d_aligned = g * prob[..., None]
    dcorr = (g * a).sum(-1) * prob * (1 - prob)
    d_emb = dcorr[..., None] * emb_ref[:, None]
    d_ref = torch.zeros_like(emb_ref)
    for t in range(T):  # t ascending
        d_ref = d_ref + dcorr[:, t, ..., None] * e[:, t]
    return d_aligned.reshape(aligned.shape), d_emb.reshape(emb.shape), d_ref


def tsa_modulate(feat, attn, attn_add):
    return feat * sigmoid(attn) * 2 + attn_add


def tsa_modulate_bwd(dy, feat, attn):
    """(d_feat, d_attn, d_attn_add)."""
    s = sigmoid(attn)
    return dy * s * 2, dy * feat * 2 * s * (1 - s), dy


# ------------------------------------------------------------------------------- modulated deformable conv


def dcn(x, offset, mask, weight, bias, dg, padding=1, store=None):
    """Modulated deformable conv (stride 1, dilation 1, groups 1) in differentiable torch ops, NCHW.  offset
    [N, dg * 2 * K, Ho, Wo] with (dy, dx) interleaved per tap, mask [N, dg * K, Ho, Wo]; a sample is valid iff
    -1 < h < H and -1 < w < W, corners outside the image contribute zero.  ``store``: applied to the column matrix
    (mask * samples), which the engine keeps in the feature dtype."""
    N, C, H, W = x.shape
    Cout, _, kh, kw = weight.shape
    K = kh * kw
    Ho, Wo = H + 2 * padding - kh + 1, W + 2 * padding - kw + 1
    cpg = C // dg
    off = offset.reshape(N, dg, K, 2, Ho, Wo)
    ii = torch.arange(K) // kw
    jj = torch.arange(K) % kw
    hb = (torch.arange(Ho)[None, :, None] - padding + ii[:, None, None]).to(x.dtype)
    wb = (torch.arange(Wo)[None, None, :] - padding + jj[:, None, None]).to(x.dtype)
    h = hb + off[:, :, :, 0]
    w = wb + off[:, :, :, 1]
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    hl, wl = hl.long(), wl.long()
    xg = x.reshape(N, dg, cpg, H * W)
    val = 0
    for dy_, dx_, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        y, xx = hl + dy_, wl + dx_
        ok = valid & (y >= 0) & (y <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (y.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(N, dg, 1, -1).expand(N, dg, cpg, -1)
        v = torch.gather(xg, 3, idx).reshape(N, dg, cpg, K, Ho, Wo)
        val = val + (wt * ok)[:, :, None] * v
    cols = (val * mask.reshape(N, dg, 1, K, Ho, Wo)).reshape(N, C, K, Ho, Wo)
    if store is not None:
        cols = store(cols)
    out = torch.einsum('ock,nckhw->nohw', weight.reshape(Cout, C, K), cols)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


# --------------------------------------------------------------------------------------------- stock tree


class GradStore(torch.autograd.Function):
    """A map the bf16 engine keeps in fp32 forward while its gradient map is rounded to bf16 on the way back (the
    network's fp32 NCHW output: the last conv's backward reads its gradient as a bf16 NHWC map)."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _rne_bf16(g)


class _Mod(nn.Module):
    """A module of the stock tree: ``st`` is the store hook and ``gst`` the gradient-only store hook (identities
    unless stock_like(emulate=True) replaced them)."""

    def st(self, t):
        return t

    def gst(self, t):
        return t

    def lrelu(self, t):
        return F.leaky_relu(t, 0.1)

    def up(self, t):
        return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)


class StockResBlock(_Mod):

    def __init__(self, nf):
        super().__init__()
        self.conv1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv2 = nn.Conv2d(nf, nf, 3, 1, 1)

    def forward(self, x):
        return self.st(x + self.conv2(self.st(F.relu(self.conv1(x)))))


class StockDCNv2Pack(_Mod):

    def __init__(self, nf, dg):
        super().__init__()
        self.dg = dg
        self.weight = nn.Parameter(torch.empty(nf, nf, 3, 3))
        self.bias = nn.Parameter(torch.empty(nf))
        self.conv_offset = nn.Conv2d(nf, dg * 27, 3, 1, 1)

    def forward(self, x, feat):
        out = self.st(self.conv_offset(feat))
        o1, o2, m = torch.chunk(out, 3, dim=1)
        store = self.st if getattr(self, 'emulate', False) else None
        return self.st(dcn(x, torch.cat((o1, o2), 1), torch.sigmoid(m), self.weight, self.bias, self.dg, store=store))


class StockPCD(_Mod):

    def __init__(self, nf=64, dg=8):
        super().__init__()
        self.offset_conv1, self.offset_conv2, self.offset_conv3 = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        self.dcn_pack, self.feat_conv = nn.ModuleDict(), nn.ModuleDict()
        for i in range(3, 0, -1):
            level = f'l{i}'
            self.offset_conv1[level] = nn.Conv2d(nf * 2, nf, 3, 1, 1)
            if i == 3:
                self.offset_conv2[level] = nn.Conv2d(nf, nf, 3, 1, 1)
            else:
                self.offset_conv2[level] = nn.Conv2d(nf * 2, nf, 3, 1, 1)
                self.offset_conv3[level] = nn.Conv2d(nf, nf, 3, 1, 1)
            self.dcn_pack[level] = StockDCNv2Pack(nf, dg)
            if i < 3:
                self.feat_conv[level] = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.cas_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.cas_offset_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.cas_dcnpack = StockDCNv2Pack(nf, dg)

    def forward(self, nbr, ref):
        st, lrelu = self.st, self.lrelu
        up_offset = up_feat = None
        for i in range(3, 0, -1):
            level = f'l{i}'
            offset = st(lrelu(self.offset_conv1[level](torch.cat([nbr[i - 1], ref[i - 1]], 1))))
            if i == 3:
                offset = st(lrelu(self.offset_conv2[level](offset)))
            else:
                offset = st(lrelu(self.offset_conv2[level](torch.cat([offset, up_offset], 1))))
                offset = st(lrelu(self.offset_conv3[level](offset)))
            feat = self.dcn_pack[level](nbr[i - 1], offset)
            if i < 3:
                feat = self.feat_conv[level](torch.cat([feat, up_feat], 1))
            if i > 1:
                feat = lrelu(feat)
            feat = st(feat)
            if i > 1:
                up_offset = st(self.up(offset) * 2)
                up_feat = st(self.up(feat))
        offset = st(lrelu(self.cas_offset_conv1(torch.cat([feat, ref[0]], 1))))
        offset = st(lrelu(self.cas_offset_conv2(offset)))
        return st(lrelu(self.cas_dcnpack(feat, offset)))


class StockTSA(_Mod):

    def __init__(self, nf=64, num_frame=5, center_frame_idx=2):
        super().__init__()
        self.center_frame_idx = center_frame_idx
        self.temporal_attn1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.temporal_attn2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.feat_fusion = nn.Conv2d(num_frame * nf, nf, 1, 1)
        self.spatial_attn1 = nn.Conv2d(num_frame * nf, nf, 1)
        self.spatial_attn2 = nn.Conv2d(nf * 2, nf, 1)
        self.spatial_attn3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.spatial_attn4 = nn.Conv2d(nf, nf, 1)
        self.spatial_attn5 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.spatial_attn_l1 = nn.Conv2d(nf, nf, 1)
        self.spatial_attn_l2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.spatial_attn_l3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.spatial_attn_add1 = nn.Conv2d(nf, nf, 1)
        self.spatial_attn_add2 = nn.Conv2d(nf, nf, 1)

    def forward(self, aligned):
        st, lrelu = self.st, self.lrelu
        b, t, c, h, w = aligned.shape
        emb_ref = st(self.temporal_attn1(aligned[:, self.center_frame_idx]))
        emb = st(self.temporal_attn2(aligned.reshape(-1, c, h, w))).reshape(b, t, -1, h, w)
        prob = torch.sigmoid((emb * emb_ref[:, None]).sum(2))  # [b, t, h, w]
        weighted = st((aligned * prob[:, :, None]).reshape(b, t * c, h, w))
        feat = st(lrelu(self.feat_fusion(weighted)))
        attn = st(lrelu(self.spatial_attn1(weighted)))
        attn = st(lrelu(self.spatial_attn2(st(pool3s2(attn)))))
        level = st(lrelu(self.spatial_attn_l1(attn)))
        level = st(lrelu(self.spatial_attn_l2(st(pool3s2(level)))))
        level = st(self.up(st(lrelu(self.spatial_attn_l3(level)))))
        attn = st(lrelu(self.spatial_attn3(attn)) + level)
        attn = st(self.up(st(lrelu(self.spatial_attn4(attn)))))
        attn = st(self.spatial_attn5(attn))
        attn_add = st(self.spatial_attn_add2(st(lrelu(self.spatial_attn_add1(attn)))))
        return st(feat * torch.sigmoid(attn) * 2 + attn_add)


class StockPredeblur(_Mod):

    def __init__(self, num_in_ch=3, nf=64, hr_in=False):
        super().__init__()
        self.hr_in = hr_in
        self.conv_first = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        if hr_in:
            self.stride_conv_hr1 = nn.Conv2d(nf, nf, 3, 2, 1)
            self.stride_conv_hr2 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.stride_conv_l2 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.stride_conv_l3 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.resblock_l3 = StockResBlock(nf)
        self.resblock_l2_1 = StockResBlock(nf)
        self.resblock_l2_2 = StockResBlock(nf)
        self.resblock_l1 = nn.ModuleList([StockResBlock(nf) for _ in range(5)])

    def forward(self, x):
        st, lrelu = self.st, self.lrelu
        l1 = st(lrelu(self.conv_first(x)))
        if self.hr_in:
            l1 = st(lrelu(self.stride_conv_hr1(l1)))
            l1 = st(lrelu(self.stride_conv_hr2(l1)))
        l2 = st(lrelu(self.stride_conv_l2(l1)))
        l3 = st(lrelu(self.stride_conv_l3(l2)))
        l3 = st(self.up(self.resblock_l3(l3)))
        l2 = st(self.resblock_l2_1(l2) + l3)
        l2 = st(self.up(self.resblock_l2_2(l2)))
        for i in range(2):
            l1 = self.resblock_l1[i](l1)
        l1 = st(l1 + l2)
        for i in range(2, 5):
            l1 = self.resblock_l1[i](l1)
        return l1


class StockEDVR(_Mod):
    """The EDVR module tree with the reference's constructor arguments and state_dict keys, in stock torch ops."""

    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=5, deformable_groups=8, num_extract_block=5,
                 num_reconstruct_block=10, center_frame_idx=None, hr_in=False, with_predeblur=False, with_tsa=True):
        super().__init__()
        nf = num_feat
        self.center_frame_idx = num_frame // 2 if center_frame_idx is None else center_frame_idx
        self.hr_in, self.with_predeblur, self.with_tsa = hr_in, with_predeblur, with_tsa
        if with_predeblur:
            self.predeblur = StockPredeblur(num_in_ch, nf, hr_in)
            self.conv_1x1 = nn.Conv2d(nf, nf, 1, 1)
        else:
            self.conv_first = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        self.feature_extraction = nn.Sequential(*[StockResBlock(nf) for _ in range(num_extract_block)])
        self.conv_l2_1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.conv_l2_2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv_l3_1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.conv_l3_2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.pcd_align = StockPCD(nf, deformable_groups)
        if with_tsa:
            self.fusion = StockTSA(nf, num_frame, self.center_frame_idx)
        else:
            self.fusion = nn.Conv2d(num_frame * nf, nf, 1, 1)
        self.reconstruction = nn.Sequential(*[StockResBlock(nf) for _ in range(num_reconstruct_block)])
        self.upconv1 = nn.Conv2d(nf, nf * 4, 3, 1, 1)
        self.upconv2 = nn.Conv2d(nf, 64 * 4, 3, 1, 1)
        self.conv_hr = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = nn.Conv2d(64, 3, 3, 1, 1)

    def forward(self, x):
        st, lrelu = self.st, self.lrelu
        b, t, c, h, w = x.shape
        assert h % (16 if self.hr_in else 4) == 0 and w % (16 if self.hr_in else 4) == 0
        x_center = x[:, self.center_frame_idx]
        frames = st(x.reshape(-1, c, h, w))
        if self.with_predeblur:
            l1 = st(self.conv_1x1(self.predeblur(frames)))
            if self.hr_in:
                h, w = h // 4, w // 4
        else:
            l1 = st(lrelu(self.conv_first(frames)))
        l1 = self.feature_extraction(l1)
        l2 = st(lrelu(self.conv_l2_2(st(lrelu(self.conv_l2_1(l1))))))
        l3 = st(lrelu(self.conv_l3_2(st(lrelu(self.conv_l3_1(l2))))))
        l1 = l1.reshape(b, t, -1, h, w)
        l2 = l2.reshape(b, t, -1, h // 2, w // 2)
        l3 = l3.reshape(b, t, -1, h // 4, w // 4)
        ci = self.center_frame_idx
        ref = [l1[:, ci], l2[:, ci], l3[:, ci]]
        aligned = torch.stack([self.pcd_align([l1[:, i], l2[:, i], l3[:, i]], ref) for i in range(t)], 1)
        if self.with_tsa:
            feat = self.fusion(aligned)
        else:
            feat = st(self.fusion(aligned.reshape(b, -1, h, w)))
        out = self.reconstruction(feat)
        out = st(lrelu(F.pixel_shuffle(self.upconv1(out), 2)))
        out = st(lrelu(F.pixel_shuffle(self.upconv2(out), 2)))
        out = self.gst(self.conv_last(st(lrelu(self.conv_hr(out)))))
        base = x_center if self.hr_in else F.interpolate(x_center, scale_factor=4, mode='bilinear', align_corners=False)
        return out + base


def init_edvr(net, seed, offset_std=0.01):
    """Deterministic test initialisation: every conv He-scaled (residual-block convs x 0.1, as the engine's arch
    initialises them), small biases, and the DCN offset convs with small random weights of std ``offset_std`` instead
    of the zero init, so that the deformable convs sample off the grid."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if 'conv_offset' in name:
                p.copy_(torch.randn(p.shape, generator=g) * offset_std)
            elif p.dim() == 4:
                fan = p.shape[1] * p.shape[2] * p.shape[3]
                scale = 0.1 if ('conv1.' in name or 'conv2.' in name) and 'offset' not in name else 1.0
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan)**0.5 * scale)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return net


def stock_like(sd, cfg, dtype, emulate=False):
    """A stock tree of config ``cfg`` loaded strictly from ``sd`` in ``dtype``.  ``emulate``: the bf16-storage
    emulation -- conv and DCN weights rounded to bf16, every kept map (and its gradient map) through ``Store``."""
    net = StockEDVR(**cfg).to(dtype)
    net.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in sd.items()}, strict=True)
    if emulate:
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 4:
                    p.copy_(_rne_bf16(p.double()).to(dtype))
        for m in net.modules():
            if isinstance(m, _Mod):
                m.st = Store.apply
                m.gst = GradStore.apply
                m.emulate = True
    return net


def state_shapes(net):
    return {k: list(v.shape) for k, v in net.state_dict().items()}


# the three configurations of tests/golden/edvr_state_keys.json
GOLDEN_CONFIGS = {
    'edvr_m_tsa': dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=5, deformable_groups=8, num_extract_block=5,
                       num_reconstruct_block=10, center_frame_idx=None, hr_in=False, with_predeblur=False, with_tsa=True),
    'edvr_m_wotsa': dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=5, deformable_groups=8, num_extract_block=5,
                         num_reconstruct_block=10, center_frame_idx=None, hr_in=False, with_predeblur=False,
                         with_tsa=False),
    'edvr_predeblur_hr': dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=5, deformable_groups=8,
                              num_extract_block=5, num_reconstruct_block=10, center_frame_idx=None, hr_in=True,
                              with_predeblur=True, with_tsa=True),
}
