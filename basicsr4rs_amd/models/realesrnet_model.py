"""RealESRNet model (mirror of basicsr/models/realesrnet_model.py): SRModel trained on pairs synthesised on the
device by the second-order degradation (models/realesrgan_degradation.py).  ``gt_usm: true`` trains against the
USM-sharpened ground truth; ``high_order_degradation: false`` takes paired data as it comes."""
import torch

from ..data.transforms import paired_random_crop
from ..utils.registry import MODEL_REGISTRY
from .realesrgan_degradation import DegradationMixin
from .sr_model import SRModel


@MODEL_REGISTRY.register()
class RealESRNetModel(DegradationMixin, SRModel):
    """It is trained without GAN losses: 1. synthesise LQ images on the device, 2. optimise net_g."""

    def __init__(self, opt):
        super().__init__(opt)
        self._init_degradation()

    @torch.no_grad()
    def feed_data(self, data):
        if not (self.is_train and self.opt.get('high_order_degradation', True)):
            return self._feed_paired(data)
        self.gt = data['gt'].to(self.device)
        if self.opt['gt_usm'] is True:
            self.gt = self.usm_sharpener(self.gt)
        self._feed_kernels(data)
        self.lq = self._degrade(self.gt)
        self.gt, self.lq = paired_random_crop(self.gt, self.lq, self.opt['gt_size'], self.opt['scale'])
        self._dequeue_and_enqueue()
        self.lq = self.lq.contiguous()
        self.gt = self.gt.contiguous()
