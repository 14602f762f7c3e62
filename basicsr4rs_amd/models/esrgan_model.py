"""ESRGAN model (mirror of basicsr/models/esrgan_model.py:8-83): SRGANModel with the relativistic average GAN
terms.  ``net_d`` runs five times per full step (twice in the generator half, three times in the discriminator
half), always in training mode, with the reference's detaches; the generator loss reaches ``fake_g_pred`` also
through ``mean(fake_g_pred)``.  The small ``pred - mean(other)`` arithmetic on the [N, 1] logits stays in torch."""
import torch

from ..utils.registry import MODEL_REGISTRY
from .srgan_model import SRGANModel


@MODEL_REGISTRY.register()
class ESRGANModel(SRGANModel):
    """ESRGAN model for single image super-resolution."""

    def _g_gan_term(self):
        real_d_pred = self._d(self.gt).detach()
        fake_g_pred = self._d(self.output)
        l_g_real = self.cri_gan(real_d_pred - torch.mean(fake_g_pred), False, is_disc=False)
        l_g_fake = self.cri_gan(fake_g_pred - torch.mean(real_d_pred), True, is_disc=False)
        return (l_g_real + l_g_fake) / 2

    def _d_terms(self, loss_dict):
        # the backwards for real and fake are separate, and the tensors behind the means detached, as in the
        # reference (esrgan_model.py:57-72)
        with torch.no_grad():
            fake_d_pred = self._d(self.output.detach())
        real_d_pred = self._d(self.gt)
        l_d_real = self.cri_gan(real_d_pred - torch.mean(fake_d_pred), True, is_disc=True) * 0.5
        l_d_real.backward()
        fake_d_pred = self._d(self.output.detach())
        l_d_fake = self.cri_gan(fake_d_pred - torch.mean(real_d_pred.detach()), False, is_disc=True) * 0.5
        l_d_fake.backward()
        loss_dict['l_d_real'] = l_d_real
        loss_dict['l_d_fake'] = l_d_fake
        loss_dict['out_d_real'] = torch.mean(real_d_pred.detach())
        loss_dict['out_d_fake'] = torch.mean(fake_d_pred.detach())
