"""SingleImageDataset (basicsr/data/single_image_dataset.py:10-68): LQ images only, for the test phase
without ground truth (options/test/ESRGAN/test_ESRGAN_x4_woGT.yml).  Paths come from a meta-info file (first
column of each line, relative to ``dataroot_lq``) or a scan of the folder; BGR -> RGB CHW float32 in [0, 1],
optional Y channel and mean/std normalisation.  ``io_backend`` 'disk' only, as PairedImageDataset."""
from os import path as osp

import torch
from torch.utils import data as data

from ..utils.img_util import img2tensor, imfrombytes, scandir
from ..utils.registry import DATASET_REGISTRY
from .paired_image_dataset import FileClient, _bgr2y


@DATASET_REGISTRY.register()
class SingleImageDataset(data.Dataset):

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.file_client = None
        self.io_backend_opt = dict(opt['io_backend'])
        self.mean = opt.get('mean')
        self.std = opt.get('std')
        self.lq_folder = opt['dataroot_lq']
        if self.io_backend_opt['type'] == 'lmdb':
            raise NotImplementedError('lmdb io backend: the lmdb package is not available in this build')
        if opt.get('meta_info_file') is not None:
            with open(opt['meta_info_file'], 'r') as fin:
                self.paths = [osp.join(self.lq_folder, line.rstrip().split(' ')[0]) for line in fin if line.strip()]
        else:
            self.paths = sorted(scandir(self.lq_folder, full_path=True))

    def __getitem__(self, index):
        if self.file_client is None:
            opt = dict(self.io_backend_opt)
            self.file_client = FileClient(opt.pop('type'), **opt)
        lq_path = self.paths[index]
        img_lq = imfrombytes(self.file_client.get(lq_path, 'lq'), float32=True)
        if self.opt.get('color') == 'y':
            img_lq = _bgr2y(img_lq)[..., None].astype('float32')
        img_lq = img2tensor(img_lq, bgr2rgb=True, float32=True)
        if self.mean is not None or self.std is not None:
            m = torch.tensor(self.mean if self.mean is not None else [0.] * img_lq.shape[0]).view(-1, 1, 1)
            s = torch.tensor(self.std if self.std is not None else [1.] * img_lq.shape[0]).view(-1, 1, 1)
            img_lq.sub_(m).div_(s)
        return {'lq': img_lq, 'lq_path': lq_path}

    def __len__(self):
        return len(self.paths)
