"""EDVR (basicsr/archs/edvr_arch.py) on the HIP engine: PCD alignment on the deformable-convolution kernels, TSA
fusion on the kernels of csrc/edvr.hip, the rest on the conv engine.

The parameter containers are the reference's ``nn.Conv2d`` / ``ModuleDict`` tree, so state_dict keys, shapes and
initialisation match and a reference checkpoint loads strictly.  The forward takes the reference's
``(b, t, c, h, w)`` NCHW frames and runs on NHWC feature maps from the first conv to the last: the concats of the
reference are channel concats of NHWC maps, the stride-2 convs are ``conv3s2``, ``upsample(offset) * 2`` is one scaled
bilinear pass, and the deformable convs take NHWC maps as they are (``DCNv2Pack.forward_nhwc``).
"""
import torch
from torch import nn as nn

from .. import _lib
from ..ops import blocks as BK
from ..ops import conv as C
from ..ops import edvr as E
from ..ops.gan import bilinear_up2
from ..utils.registry import ARCH_REGISTRY
from .arch_util import DCNv2Pack, ResidualBlockNoBN, make_layer

_LRELU = dict(act=_lib.ACT_LRELU, slope=0.1)


def _cat(a, b):
    """Channel concat of two NHWC maps."""
    return torch.cat([a, b], dim=-1)


def _check_feat(num_feat, deformable_groups=None):
    if num_feat % 8:
        raise ValueError(f'EDVR on the HIP engine needs num_feat to be a multiple of 8, got {num_feat}')
    if deformable_groups is not None and num_feat % deformable_groups:
        raise ValueError(f'num_feat {num_feat} is not divisible by deformable_groups {deformable_groups}')


class PCDAlignment(nn.Module):
    """Pyramid, cascading and deformable alignment (edvr_arch.py:9-97).  Three pyramid levels (l3: 1/4 size, l2:
    1/2, l1: full), each predicting offsets from cat(neighbour, reference) and aligning the neighbour's features
    with a DCNv2Pack, then one cascading DCN at full size."""

    def __init__(self, num_feat=64, deformable_groups=8):
        super().__init__()
        _check_feat(num_feat, deformable_groups)
        self.offset_conv1 = nn.ModuleDict()
        self.offset_conv2 = nn.ModuleDict()
        self.offset_conv3 = nn.ModuleDict()
        self.dcn_pack = nn.ModuleDict()
        self.feat_conv = nn.ModuleDict()
        for i in range(3, 0, -1):
            level = f'l{i}'
            self.offset_conv1[level] = nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1)
            if i == 3:
                self.offset_conv2[level] = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            else:
                self.offset_conv2[level] = nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1)
                self.offset_conv3[level] = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.dcn_pack[level] = DCNv2Pack(num_feat, num_feat, 3, padding=1, deformable_groups=deformable_groups)
            if i < 3:
                self.feat_conv[level] = nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1)
        self.cas_offset_conv1 = nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1)
        self.cas_offset_conv2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.cas_dcnpack = DCNv2Pack(num_feat, num_feat, 3, padding=1, deformable_groups=deformable_groups)
        self.upsample = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def forward(self, nbr_feat_l, ref_feat_l):
        """``nbr_feat_l`` / ``ref_feat_l``: [l1, l2, l3] NHWC maps [b, h, w, c] of the neighbouring and the reference
        frame.  Returns the aligned l1 features, NHWC."""
        upsampled_offset, upsampled_feat = None, None
        for i in range(3, 0, -1):
            level = f'l{i}'
            offset = C.conv3x3(_cat(nbr_feat_l[i - 1], ref_feat_l[i - 1]), self.offset_conv1[level], **_LRELU)
            if i == 3:
                offset = C.conv3x3(offset, self.offset_conv2[level], **_LRELU)
            else:
                offset = C.conv3x3(_cat(offset, upsampled_offset), self.offset_conv2[level], **_LRELU)
                offset = C.conv3x3(offset, self.offset_conv3[level], **_LRELU)
            feat = self.dcn_pack[level].forward_nhwc(nbr_feat_l[i - 1], offset)
            if i < 3:
                feat = C.conv3x3(_cat(feat, upsampled_feat), self.feat_conv[level], **(_LRELU if i > 1 else {}))
            else:
                feat = E.leaky_relu(feat, 0.1)
            if i > 1:
                # the offsets are in pixels of their own level: twice as long one level up
                upsampled_offset = bilinear_up2(offset, 2.0)
                upsampled_feat = bilinear_up2(feat)
        offset = C.conv3x3(_cat(feat, ref_feat_l[0]), self.cas_offset_conv1, **_LRELU)
        offset = C.conv3x3(offset, self.cas_offset_conv2, **_LRELU)
        return E.leaky_relu(self.cas_dcnpack.forward_nhwc(feat, offset), 0.1)


class TSAFusion(nn.Module):
    """Temporal and spatial attention fusion (edvr_arch.py:100-189): the aligned frames weighted by their
    correlation with the centre frame, fused by a 1 x 1 conv, then modulated by a three-level spatial attention."""

    def __init__(self, num_feat=64, num_frame=5, center_frame_idx=2):
        super().__init__()
        _check_feat(num_feat)
        self.center_frame_idx = center_frame_idx
        self.temporal_attn1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.temporal_attn2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.feat_fusion = nn.Conv2d(num_frame * num_feat, num_feat, 1, 1)
        self.max_pool = nn.MaxPool2d(3, stride=2, padding=1)
        self.avg_pool = nn.AvgPool2d(3, stride=2, padding=1)
        self.spatial_attn1 = nn.Conv2d(num_frame * num_feat, num_feat, 1)
        self.spatial_attn2 = nn.Conv2d(num_feat * 2, num_feat, 1)
        self.spatial_attn3 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.spatial_attn4 = nn.Conv2d(num_feat, num_feat, 1)
        self.spatial_attn5 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.spatial_attn_l1 = nn.Conv2d(num_feat, num_feat, 1)
        self.spatial_attn_l2 = nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1)
        self.spatial_attn_l3 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.spatial_attn_add1 = nn.Conv2d(num_feat, num_feat, 1)
        self.spatial_attn_add2 = nn.Conv2d(num_feat, num_feat, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)
        self.upsample = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)

    def forward(self, aligned_feat):
        """``aligned_feat``: NHWC [b, t, h, w, c].  Returns the fused features [b, h, w, c]."""
        b, t, h, w, c = aligned_feat.shape
        frames = aligned_feat.reshape(b * t, h, w, c)
        embedding_ref = C.conv3x3(aligned_feat[:, self.center_frame_idx].contiguous(), self.temporal_attn1)
        embedding = C.conv3x3(frames, self.temporal_attn2)
        # [b, h, w, t * c]: the frames times their correlation probability, in the reference's (t, c) channel order
        weighted, _ = E.tsa_corr(embedding, embedding_ref, frames)

        feat = E.conv1x1(weighted, self.feat_fusion, **_LRELU)

        attn = E.conv1x1(weighted, self.spatial_attn1, **_LRELU)
        attn = E.conv1x1(E.pool3s2(attn), self.spatial_attn2, **_LRELU)
        attn_level = E.conv1x1(attn, self.spatial_attn_l1, **_LRELU)
        attn_level = C.conv3x3(E.pool3s2(attn_level), self.spatial_attn_l2, **_LRELU)
        attn_level = bilinear_up2(C.conv3x3(attn_level, self.spatial_attn_l3, **_LRELU))

        attn = C.conv3x3(attn, self.spatial_attn3, res=attn_level, **_LRELU)
        attn = bilinear_up2(E.conv1x1(attn, self.spatial_attn4, **_LRELU))
        attn = C.conv3x3(attn, self.spatial_attn5)
        attn_add = E.conv1x1(E.conv1x1(attn, self.spatial_attn_add1, **_LRELU), self.spatial_attn_add2)
        # after initialisation, * 2 makes sigmoid(attn) * 2 close to 1
        return E.tsa_modulate(feat, attn, attn_add)


class PredeblurModule(nn.Module):
    """Pre-deblur module (edvr_arch.py:192-242): a three-level residual pyramid in front of the feature extraction."""

    def __init__(self, num_in_ch=3, num_feat=64, hr_in=False):
        super().__init__()
        _check_feat(num_feat)
        self.hr_in = hr_in
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        if self.hr_in:
            self.stride_conv_hr1 = nn.Conv2d(num_feat, num_feat, 3, 2, 1)
            self.stride_conv_hr2 = nn.Conv2d(num_feat, num_feat, 3, 2, 1)
        self.stride_conv_l2 = nn.Conv2d(num_feat, num_feat, 3, 2, 1)
        self.stride_conv_l3 = nn.Conv2d(num_feat, num_feat, 3, 2, 1)
        self.resblock_l3 = ResidualBlockNoBN(num_feat=num_feat)
        self.resblock_l2_1 = ResidualBlockNoBN(num_feat=num_feat)
        self.resblock_l2_2 = ResidualBlockNoBN(num_feat=num_feat)
        self.resblock_l1 = nn.ModuleList([ResidualBlockNoBN(num_feat=num_feat) for i in range(5)])
        self.upsample = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def forward(self, x):
        """``x``: the NHWC image map [n, h, w, pad8(num_in_ch)].  Returns NHWC features (1/4 size with ``hr_in``)."""
        feat_l1 = C.conv3x3(x, self.conv_first, **_LRELU)
        if self.hr_in:
            feat_l1 = E.conv3s2(feat_l1, self.stride_conv_hr1, **_LRELU)
            feat_l1 = E.conv3s2(feat_l1, self.stride_conv_hr2, **_LRELU)
        feat_l2 = E.conv3s2(feat_l1, self.stride_conv_l2, **_LRELU)
        feat_l3 = E.conv3s2(feat_l2, self.stride_conv_l3, **_LRELU)

        feat_l3 = bilinear_up2(self.resblock_l3(feat_l3))
        feat_l2 = self.resblock_l2_1(feat_l2) + feat_l3
        feat_l2 = bilinear_up2(self.resblock_l2_2(feat_l2))
        for i in range(2):
            feat_l1 = self.resblock_l1[i](feat_l1)
        feat_l1 = feat_l1 + feat_l2
        for i in range(2, 5):
            feat_l1 = self.resblock_l1[i](feat_l1)
        return feat_l1


@ARCH_REGISTRY.register()
class EDVR(nn.Module):
    """EDVR video super-resolution network, x4 (edvr_arch.py:245-382), with the reference's constructor arguments.
    ``num_feat`` must be a multiple of 8 and of ``deformable_groups``."""

    def __init__(self,
                 num_in_ch=3,
                 num_out_ch=3,
                 num_feat=64,
                 num_frame=5,
                 deformable_groups=8,
                 num_extract_block=5,
                 num_reconstruct_block=10,
                 center_frame_idx=None,
                 hr_in=False,
                 with_predeblur=False,
                 with_tsa=True):
        super().__init__()
        _check_feat(num_feat, deformable_groups)
        self.center_frame_idx = num_frame // 2 if center_frame_idx is None else center_frame_idx
        self.hr_in = hr_in
        self.with_predeblur = with_predeblur
        self.with_tsa = with_tsa
        self.num_in_ch = num_in_ch

        if self.with_predeblur:
            self.predeblur = PredeblurModule(num_feat=num_feat, hr_in=self.hr_in)
            self.conv_1x1 = nn.Conv2d(num_feat, num_feat, 1, 1)
        else:
            self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)

        self.feature_extraction = make_layer(ResidualBlockNoBN, num_extract_block, num_feat=num_feat)
        self.conv_l2_1 = nn.Conv2d(num_feat, num_feat, 3, 2, 1)
        self.conv_l2_2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_l3_1 = nn.Conv2d(num_feat, num_feat, 3, 2, 1)
        self.conv_l3_2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)

        self.pcd_align = PCDAlignment(num_feat=num_feat, deformable_groups=deformable_groups)
        if self.with_tsa:
            self.fusion = TSAFusion(num_feat=num_feat, num_frame=num_frame, center_frame_idx=self.center_frame_idx)
        else:
            self.fusion = nn.Conv2d(num_frame * num_feat, num_feat, 1, 1)

        self.reconstruction = make_layer(ResidualBlockNoBN, num_reconstruct_block, num_feat=num_feat)
        self.upconv1 = nn.Conv2d(num_feat, num_feat * 4, 3, 1, 1)
        self.upconv2 = nn.Conv2d(num_feat, 64 * 4, 3, 1, 1)
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.conv_hr = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = nn.Conv2d(64, 3, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def forward(self, x):
        b, t, c, h, w = x.size()
        if self.hr_in:
            assert h % 16 == 0 and w % 16 == 0, ('The height and width must be multiple of 16.')
        else:
            assert h % 4 == 0 and w % 4 == 0, ('The height and width must be multiple of 4.')
        x_center = x[:, self.center_frame_idx, :, :, :].contiguous()

        # L1: features of every frame, the frames as the batch
        frames = C.to_nhwc(x.reshape(-1, c, h, w), C.pad8(c), C.feature_dtype())
        if self.with_predeblur:
            feat_l1 = E.conv1x1(self.predeblur(frames), self.conv_1x1)
            if self.hr_in:
                h, w = h // 4, w // 4
        else:
            feat_l1 = C.conv3x3(frames, self.conv_first, **_LRELU)
        feat_l1 = self.feature_extraction(feat_l1)
        # L2, L3
        feat_l2 = C.conv3x3(E.conv3s2(feat_l1, self.conv_l2_1, **_LRELU), self.conv_l2_2, **_LRELU)
        feat_l3 = C.conv3x3(E.conv3s2(feat_l2, self.conv_l3_1, **_LRELU), self.conv_l3_2, **_LRELU)

        nf = feat_l1.shape[-1]
        levels = [feat_l1.view(b, t, h, w, nf), feat_l2.view(b, t, h // 2, w // 2, nf),
                  feat_l3.view(b, t, h // 4, w // 4, nf)]

        # PCD alignment of every frame to the centre frame
        ref_feat_l = [f[:, self.center_frame_idx].contiguous() for f in levels]
        aligned_feat = []
        for i in range(t):
            nbr_feat_l = [f[:, i].contiguous() for f in levels]
            aligned_feat.append(self.pcd_align(nbr_feat_l, ref_feat_l))

        if self.with_tsa:
            feat = self.fusion(torch.stack(aligned_feat, dim=1))  # [b, t, h, w, c]
        else:
            feat = E.conv1x1(torch.cat(aligned_feat, dim=-1), self.fusion)  # [b, h, w, t * c]

        out = self.reconstruction(feat)
        out = C.conv3x3(out, self.upconv1, out_ps=2, **_LRELU)
        out = C.conv3x3(out, self.upconv2, out_ps=2, **_LRELU)
        out = C.conv3x3(C.conv3x3(out, self.conv_hr, **_LRELU), self.conv_last, out_nchw=True)
        if self.hr_in:
            return out + x_center
        return BK.bilinear_up_add(out, x_center, 4)
