"""RealESRGAN model (mirror of basicsr/models/realesrgan_model.py): SRGANModel trained on pairs synthesised on the
device by the second-order degradation (models/realesrgan_degradation.py).  The degradation always starts from the
USM-sharpened ground truth; ``l1_gt_usm`` / ``percep_gt_usm`` / ``gan_gt_usm`` choose, per loss, between the
sharpened and the plain ground truth of the batch that left the training-pair pool.  The step itself is
SRGANModel's: the targets travel through its ``_g_content_terms`` / ``_d_terms`` hooks.  ``dist``, ``cuda_graph`` and
``ldl_opt`` are handled as SRGANModel handles them."""
import torch

from ..data.transforms import paired_random_crop
from ..utils.registry import MODEL_REGISTRY
from .realesrgan_degradation import DegradationMixin
from .srgan_model import SRGANModel


@MODEL_REGISTRY.register()
class RealESRGANModel(DegradationMixin, SRGANModel):
    """1. synthesise LQ images on the device, 2. optimise the networks with GAN training."""

    def __init__(self, opt):
        super().__init__(opt)
        self._init_degradation()

    @torch.no_grad()
    def feed_data(self, data):
        if not (self.is_train and self.opt.get('high_order_degradation', True)):
            return self._feed_paired(data)
        self.gt = data['gt'].to(self.device)
        self.gt_usm = self.usm_sharpener(self.gt)
        self._feed_kernels(data)
        self.lq = self._degrade(self.gt_usm)
        (self.gt, self.gt_usm), self.lq = paired_random_crop([self.gt, self.gt_usm], self.lq, self.opt['gt_size'],
                                                             self.opt['scale'])
        self._dequeue_and_enqueue()
        # sharpen again: the pool may have replaced self.gt
        self.gt = self.gt.contiguous()
        self.gt_usm = self.usm_sharpener(self.gt)
        self.lq = self.lq.contiguous()

    def _target(self, key):
        return self.gt if self.opt[key] is False else self.gt_usm

    def _g_content_terms(self, loss_dict):
        return super()._g_content_terms(loss_dict, pix_gt=self._target('l1_gt_usm'),
                                        percep_gt=self._target('percep_gt_usm'))

    def _d_terms(self, loss_dict):
        return super()._d_terms(loss_dict, real=self._target('gan_gt_usm'))
