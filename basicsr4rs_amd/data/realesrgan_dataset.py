"""RealESRGANDataset (basicsr/data/realesrgan_dataset.py:17-193): ground-truth images only, plus the two blur
kernels and the final sinc kernel of one second-order degradation; the degradation itself runs on the device in the
model's ``feed_data``.  Disk backend with a ``meta_info`` list (the lmdb backend needs the lmdb package, which this
image lacks: it raises with the message of the other datasets).  The host draws come in the reference's order, so a
seeded worker produces the reference's crops and kernels."""
import math
import os
import random

import numpy as np
import torch
from torch.utils import data as data

from ..utils.img_util import img2tensor, imfrombytes
from ..utils.registry import DATASET_REGISTRY
from .degradations import circular_lowpass_kernel, random_mixed_kernels
from .paired_image_dataset import FileClient
from .transforms import augment

CROP_PAD_SIZE = 400  # fixed in the reference


@DATASET_REGISTRY.register()
class RealESRGANDataset(data.Dataset):
    """Returns {'gt' [3, 400, 400] RGB in [0, 1], 'kernel1', 'kernel2', 'sinc_kernel' [21, 21] fp32, 'gt_path'}."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.file_client = None
        self.io_backend_opt = dict(opt['io_backend'])
        self.gt_folder = opt['dataroot_gt']
        if self.io_backend_opt['type'] == 'lmdb':
            raise NotImplementedError('lmdb io backend: the lmdb package is not available in this build')
        # each line of meta_info starts with the path of an image relative to dataroot_gt
        with open(opt['meta_info']) as fin:
            self.paths = [os.path.join(self.gt_folder, line.strip().split(' ')[0]) for line in fin if line.strip()]
        self.kernel_range = [2 * v + 1 for v in range(3, 11)]  # 7 .. 21, fixed in the reference
        self.pulse_tensor = torch.zeros(21, 21).float()  # the filter that leaves the image as it is
        self.pulse_tensor[10, 10] = 1

    def _blur_kernel(self, suffix):
        """One kernel of the first ('') or second ('2') degradation, zero-padded to 21 x 21."""
        opt = self.opt
        kernel_size = random.choice(self.kernel_range)
        if np.random.uniform() < opt['sinc_prob' + suffix]:
            if kernel_size < 13:
                omega_c = np.random.uniform(np.pi / 3, np.pi)
            else:
                omega_c = np.random.uniform(np.pi / 5, np.pi)
            kernel = circular_lowpass_kernel(omega_c, kernel_size, pad_to=False)
        else:
            kernel = random_mixed_kernels(opt['kernel_list' + suffix], opt['kernel_prob' + suffix], kernel_size,
                                          opt['blur_sigma' + suffix], opt['blur_sigma' + suffix], [-math.pi, math.pi],
                                          opt['betag_range' + suffix], opt['betap_range' + suffix], noise_range=None)
        pad_size = (21 - kernel_size) // 2
        return np.pad(kernel, ((pad_size, pad_size), (pad_size, pad_size)))

    @staticmethod
    def crop_or_pad(img_gt, size=CROP_PAD_SIZE):
        """Pad bottom / right by reflection without repeating the edge (BORDER_REFLECT_101) up to ``size``, then crop
        a random ``size`` x ``size`` window of what is larger."""
        h, w = img_gt.shape[0:2]
        if h < size or w < size:
            img_gt = np.pad(img_gt, ((0, max(0, size - h)), (0, max(0, size - w)), (0, 0)), mode='reflect')
        if img_gt.shape[0] > size or img_gt.shape[1] > size:
            h, w = img_gt.shape[0:2]
            top = random.randint(0, h - size)
            left = random.randint(0, w - size)
            img_gt = img_gt[top:top + size, left:left + size, ...]
        return img_gt

    def __getitem__(self, index):
        if self.file_client is None:
            opt = dict(self.io_backend_opt)
            self.file_client = FileClient(opt.pop('type'), **opt)
        gt_path = self.paths[index]
        img_gt = imfrombytes(self.file_client.get(gt_path, 'gt'), float32=True)
        img_gt = augment(img_gt, self.opt['use_hflip'], self.opt['use_rot'])
        img_gt = self.crop_or_pad(img_gt)
        kernel = self._blur_kernel('')
        kernel2 = self._blur_kernel('2')
        if np.random.uniform() < self.opt['final_sinc_prob']:
            kernel_size = random.choice(self.kernel_range)
            omega_c = np.random.uniform(np.pi / 3, np.pi)
            sinc_kernel = torch.FloatTensor(circular_lowpass_kernel(omega_c, kernel_size, pad_to=21))
        else:
            sinc_kernel = self.pulse_tensor
        img_gt = img2tensor([np.ascontiguousarray(img_gt)], bgr2rgb=True, float32=True)[0]
        return {'gt': img_gt, 'kernel1': torch.FloatTensor(kernel), 'kernel2': torch.FloatTensor(kernel2),
                'sinc_kernel': sinc_kernel, 'gt_path': gt_path}

    def __len__(self):
        return len(self.paths)
