"""L2SSingleModel (basicsr/models/srrs_l2s_model.py:31-97): the Landsat-to-Sentinel model of the fork.

A batch is a dict of dicts: ``lq.rgb`` / ``lq.nss`` (the visible and the NIR / SWIR bands of the LR
tile, one resolution) and ``gt.rgb`` / ``gt.nss`` (the HR bands: RGB at the target resolution, NSS at
half of it), with ``sample_path`` and ``img_name``.  The network sees the channel concat of the two LR
groups; the ground truth is RGB next to the NSS bands upsampled x2 with
``F.interpolate(mode='bicubic')`` (align_corners=False).  That upsampling runs on every train step, so
it is a HIP kernel here (``sr_bicubic_up_hp``) that writes straight into channels 3.. of a
preallocated ground-truth tensor: the reference's ``torch.cat`` is fused away.
"""
import datetime
import os
from os import path as osp

import torch

from ..ops.convk import bicubic_up_hp
from ..utils.img_util import imwrite
from ..utils.registry import MODEL_REGISTRY
from .srrs_model import SRRSModel


@MODEL_REGISTRY.register()
class L2SSingleModel(SRRSModel):

    def feed_data(self, data):
        self.sample_path = data['sample_path']
        self.img_name = data['img_name']
        self.lq = torch.cat([data['lq']['rgb'], data['lq']['nss']], dim=1).to(self.device, non_blocking=True)
        if 'gt' in data:
            rgb = data['gt']['rgb'].to(self.device, non_blocking=True)
            nss = data['gt']['nss'].to(self.device, non_blocking=True)
            b, c_rgb, h, w = rgb.shape
            gt = torch.empty(b, c_rgb + nss.shape[1], h, w, device=self.device, dtype=torch.float32)
            gt[:, :c_rgb].copy_(rgb)
            bicubic_up_hp(nss, 2, out=gt, c0=c_rgb)
            self.gt = gt

    def log_nan_inf_loss(self, current_iter, loss):
        """The batch behind a non-finite loss, kept for inspection under
        ``<experiments_root>/loss/<iter>/`` (srrs_l2s_model.py:56-73)."""
        log_dir = osp.join(self.opt['path']['experiments_root'], 'loss', str(current_iter))
        os.makedirs(log_dir, exist_ok=True)
        loss = loss.detach()
        meta_info = {
            'iter': current_iter,
            'sample_path': self.sample_path,
            'loss': float(loss.cpu()) if torch.isfinite(loss) else str(loss),
            'timestamp': datetime.datetime.now().strftime('%Y-%m-%d %H:%M:%S'),
            'loss_type': 'NaN' if torch.isnan(loss) else 'Inf' if torch.isinf(loss) else 'Other',
        }
        torch.save(meta_info, osp.join(log_dir, f'meta_iter_{current_iter}.pt'))
        torch.save(self.lq.detach().cpu(), osp.join(log_dir, f'lq_iter_{current_iter}.pt'))
        torch.save(self.output.detach().cpu(), osp.join(log_dir, f'out_iter_{current_iter}.pt'))
        torch.save(self.gt.detach().cpu(), osp.join(log_dir, f'gt_iter_{current_iter}.pt'))

    @staticmethod
    def _extract_img_name(val_data):
        return val_data['img_name'][0]

    def _save_visuals(self, dataset, img_name, images):
        """Channels 0-2 under ``RGB/`` and 3-5 under ``NSS/`` of every visual, each file written once
        (srrs_l2s_model.py:78-97: both groups are stored as three-band colour PNGs)."""
        vis = self.opt['path']['visualization']
        for key, img in images.items():
            if img is None:
                continue
            for folder, part in (('RGB', img[..., :3]), ('NSS', img[..., 3:])):
                path = osp.join(vis, folder, dataset, img_name, f'{key}.png')
                if not osp.exists(path):
                    imwrite(part[..., ::-1], path)  # imwrite takes BGR (cv2 convention)
