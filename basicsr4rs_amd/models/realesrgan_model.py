"""RealESRGAN model (mirror of basicsr/models/realesrgan_model.py): SRGANModel trained on pairs synthesised on the
device by the second-order degradation (models/realesrgan_degradation.py).  The degradation always starts from the
USM-sharpened ground truth; ``l1_gt_usm`` / ``percep_gt_usm`` / ``gan_gt_usm`` choose, per loss, between the
sharpened and the plain ground truth of the batch that left the training-pair pool.  The step itself is
SRGANModel's: the targets travel through its ``_g_content_terms`` / ``_d_terms`` hooks.  ``dist`` and ``cuda_graph``
are handled as SRGANModel handles them.

``train.ldl_opt`` (options/train/LDL/train_LDL_Real_x4.yml) adds the LDL term between the pixel and the perceptual
terms (realesrgan_model.py:211-226): the artifact map of the output against the plain ground truth and the EMA
network's output, then ``cri_ldl(w * output, w * gt)``.  An ``L1Loss`` with reduction mean / sum runs as the fused
term of losses/loss_util.py; any other criterion gets the map from ``get_refined_artifact_map``."""
import torch

from ..data.transforms import paired_random_crop
from ..losses.basic_loss import L1Loss
from ..losses.loss_util import get_refined_artifact_map, ldl_l1_term
from ..utils.registry import MODEL_REGISTRY
from .realesrgan_degradation import DegradationMixin
from .srgan_model import SRGANModel


@MODEL_REGISTRY.register()
class RealESRGANModel(DegradationMixin, SRGANModel):
    """1. synthesise LQ images on the device, 2. optimise the networks with GAN training."""

    def __init__(self, opt):
        super().__init__(opt)
        self._init_degradation()

    def _build_ldl(self, train_opt):
        cri_ldl = self.build_optional_loss(train_opt, 'ldl_opt')
        if cri_ldl is not None and not self.ema_decay > 0:
            # the reference reads net_g_ema, which exists only with ema_decay > 0
            raise ValueError(f'{type(self).__name__}: train.ldl_opt needs train.ema_decay > 0 (the artifact map is '
                             'taken against the EMA network\'s output)')
        return cri_ldl

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

    def _ldl_term(self):
        """The map is taken against ``self.gt``, not the USM target, as in the reference; the EMA network runs only in
        the iterations that update the generator (the reference runs it every iteration and uses it in these)."""
        with torch.no_grad(), self._amp():
            self.output_ema = self.net_g_ema(self.lq)
        cri = self.cri_ldl
        if type(cri) is L1Loss and cri.reduction in ('mean', 'sum'):
            return ldl_l1_term(self.output, self.gt, self.output_ema, cri.loss_weight, cri.reduction)
        w = get_refined_artifact_map(self.gt, self.output, self.output_ema, 7)
        return cri(w * self.output, w * self.gt)

    def _d_terms(self, loss_dict):
        return super()._d_terms(loss_dict, real=self._target('gan_gt_usm'))
