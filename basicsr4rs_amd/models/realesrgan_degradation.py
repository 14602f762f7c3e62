"""The on-device second-order degradation and the training-pair pool shared by RealESRNetModel and RealESRGANModel
(the reference writes both out twice: basicsr/models/realesrnet_model.py:31-177, realesrgan_model.py:31-179).

``_degrade(gt_usm)`` keeps the reference's sequence and its order of host draws (``random.choices``,
``np.random.uniform``, ``random.choice``), so a run with the same seeds takes the reference's branches: blur, random
resize, Gaussian or Poisson noise, JPEG; blur with probability ``second_blur_prob``, random resize, noise; then
[resize back + sinc filter] and JPEG in either order; the round to 8 bits rides in the last kernel's epilogue.  Every
device step is a kernel of csrc/degrade.hip and nothing returns to the host (the reference's Poisson branch counts
distinct levels with ``torch.unique`` per sample there).
"""
import random

import numpy as np
import torch

from ..data.degradations import random_add_gaussian_noise_pt, random_add_poisson_noise_pt
from ..ops import degrade as D
from ..utils.diffjpeg import DiffJPEG
from ..utils.img_process_util import USMSharp

_MODES = ['area', 'bilinear', 'bicubic']


class DegradationMixin:

    def _init_degradation(self):
        self.jpeger = DiffJPEG(differentiable=False).to(self.device)
        self.usm_sharpener = USMSharp().to(self.device)
        self.queue_size = self.opt.get('queue_size', 180)

    @torch.no_grad()
    def _dequeue_and_enqueue(self):
        """The training-pair pool: batches fill it; once full, it is shuffled, its first b pairs leave as the batch
        and the incoming batch takes their place (degradation settings are per batch, the pool mixes them)."""
        b, c, h, w = self.lq.size()
        if not hasattr(self, 'queue_lr'):
            assert self.queue_size % b == 0, f'queue size {self.queue_size} should be divisible by batch size {b}'
            self.queue_lr = torch.zeros(self.queue_size, c, h, w, device=self.device)
            _, c, h, w = self.gt.size()
            self.queue_gt = torch.zeros(self.queue_size, c, h, w, device=self.device)
            self.queue_ptr = 0
        if self.queue_ptr == self.queue_size:
            idx = torch.randperm(self.queue_size)
            self.queue_lr = self.queue_lr[idx]
            self.queue_gt = self.queue_gt[idx]
            lq_dequeue = self.queue_lr[0:b].clone()
            gt_dequeue = self.queue_gt[0:b].clone()
            self.queue_lr[0:b] = self.lq
            self.queue_gt[0:b] = self.gt
            self.lq, self.gt = lq_dequeue, gt_dequeue
        else:
            self.queue_lr[self.queue_ptr:self.queue_ptr + b] = self.lq
            self.queue_gt[self.queue_ptr:self.queue_ptr + b] = self.gt
            self.queue_ptr = self.queue_ptr + b

    def _random_scale(self, prob, rng):
        updown_type = random.choices(['up', 'down', 'keep'], prob)[0]
        if updown_type == 'up':
            return np.random.uniform(1, rng[1])
        if updown_type == 'down':
            return np.random.uniform(rng[0], 1)
        return 1

    def _noise(self, out, suffix):
        opt = self.opt
        gray_noise_prob = opt['gray_noise_prob' + suffix]
        if np.random.uniform() < opt['gaussian_noise_prob' + suffix]:
            return random_add_gaussian_noise_pt(out, sigma_range=opt['noise_range' + suffix], clip=True, rounds=False,
                                                gray_prob=gray_noise_prob)
        return random_add_poisson_noise_pt(out, scale_range=opt['poisson_scale_range' + suffix], gray_prob=gray_noise_prob,
                                           clip=True, rounds=False)

    def _jpeg(self, out, rng, round255=False):
        jpeg_p = out.new_zeros(out.size(0)).uniform_(*rng)
        # the noise and round255 epilogues already leave [0, 1]; a resize may not (bicubic overshoots)
        return D.jpeg(torch.clamp(out, 0, 1), jpeg_p, differentiable=False, round255=round255)

    @torch.no_grad()
    def _degrade(self, gt_usm):
        """lq [b, 3, h / scale, w / scale] on the 1 / 255 grid from the (sharpened) ground truth; needs
        ``self.kernel1`` / ``self.kernel2`` / ``self.sinc_kernel``."""
        opt = self.opt
        ori_h, ori_w = gt_usm.size()[2:4]
        # ----------------------- the first degradation process -----------------------
        out = D.filter2d(gt_usm, self.kernel1)
        scale = self._random_scale(opt['resize_prob'], opt['resize_range'])
        mode = random.choice(_MODES)
        out = D.resize(out, scale_factor=scale, mode=mode)
        out = self._noise(out, '')
        out = self._jpeg(out, opt['jpeg_range'])
        # ----------------------- the second degradation process ----------------------
        if np.random.uniform() < opt['second_blur_prob']:
            out = D.filter2d(out, self.kernel2)
        scale = self._random_scale(opt['resize_prob2'], opt['resize_range2'])
        mode = random.choice(_MODES)
        out = D.resize(out, size=(int(ori_h / opt['scale'] * scale), int(ori_w / opt['scale'] * scale)), mode=mode)
        out = self._noise(out, '2')
        # [resize back + sinc filter] and JPEG in either order; the last of them rounds to 8 bits
        final = (ori_h // opt['scale'], ori_w // opt['scale'])
        if np.random.uniform() < 0.5:
            mode = random.choice(_MODES)
            out = D.resize(out, size=final, mode=mode)
            out = D.filter2d(out, self.sinc_kernel)
            return self._jpeg(out, opt['jpeg_range2'], round255=True)
        out = self._jpeg(out, opt['jpeg_range2'])
        mode = random.choice(_MODES)
        out = D.resize(out, size=final, mode=mode)
        return D.filter2d(out, self.sinc_kernel, round255=True)

    def _feed_kernels(self, data):
        self.kernel1 = data['kernel1'].to(self.device)
        self.kernel2 = data['kernel2'].to(self.device)
        self.sinc_kernel = data['sinc_kernel'].to(self.device)

    def _feed_paired(self, data):
        """Paired training or validation: no synthesis."""
        self.lq = data['lq'].to(self.device)
        if 'gt' in data:
            self.gt = data['gt'].to(self.device)
            self.gt_usm = self.usm_sharpener(self.gt)

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        # no synthetic degradation during validation
        self.is_train = False
        try:
            super().nondist_validation(dataloader, current_iter, tb_logger, save_img)
        finally:
            self.is_train = True
