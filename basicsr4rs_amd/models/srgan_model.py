"""SRGAN model (mirror of basicsr/models/srgan_model.py:11-149) on the HIP engine.

``net_g`` and the discriminator ``net_d`` each own a flat parameter vector (``flat_g`` / ``flat_d``) and a fused
Adam that runs once per network and step; the EMA covers ``net_g`` only.  The step order, the detaches and the
``requires_grad`` switches of ``net_d`` are the reference's: they decide how often BatchNorm's running statistics
move (``net_d`` runs three times per full SRGAN step, always in training mode) and, with the discriminator's
parameters frozen during the generator half, no discriminator weight gradient is launched there.  There is no
host synchronisation in the step; the loss log is reduced when read.

Out of scope: ``train.cuda_graph`` (the generator half is conditional on the iteration; one warning, the step
runs eagerly) and distributed training (``dist: true`` is refused: the discriminator's gradient and BatchNorm
buffer exchange is not built).  ``ldl_opt`` is refused here and in ESRGANModel (the reference builds the loss there
and never uses it); RealESRGANModel overrides ``_build_ldl`` (models/realesrgan_model.py).
"""
from collections import OrderedDict

import torch

from ..archs import build_network
from ..utils.flat import FlatParams, FusedAdam, ema_copy
from ..utils.logger import get_root_logger
from ..utils.registry import MODEL_REGISTRY
from .sr_model import SRModel


@MODEL_REGISTRY.register()
class SRGANModel(SRModel):
    """SRGAN model for single image super-resolution."""

    def __init__(self, opt):
        if opt.get('dist', False) and opt.get('is_train', False):
            raise NotImplementedError(f'{type(self).__name__}: distributed training is not supported (the exchange of '
                                      'the discriminator\'s gradients and BatchNorm buffers is not built)')
        super().__init__(opt)

    def init_training_settings(self):
        train_opt = self.opt['train']
        self._init_amp_state(train_opt)
        self.use_graph = False
        if train_opt.get('cuda_graph', False):
            get_root_logger().warning(f'{type(self).__name__}: train.cuda_graph is not supported (the generator half of '
                                      'the step is conditional on the iteration); the step runs eagerly')
        self.async_wgrad = False
        self._init_ema(train_opt)

        # the discriminator: its own flat parameter vector, flat_g stays the generator's
        self.net_d = build_network(self.opt['network_d']).to(self.device)
        self.flat_d = FlatParams(self.net_d)
        self.print_network(self.net_d)
        load_path = self.opt.get('path', {}).get('pretrain_network_d', None)
        if load_path is not None:
            param_key = self.opt['path'].get('param_key_d', 'params')
            self.load_network(self.net_d, load_path, self.opt['path'].get('strict_load_d', True), param_key)
        self.net_d.train()

        self.cri_pix = self.build_optional_loss(train_opt, 'pixel_opt')
        self.cri_ldl = self._build_ldl(train_opt)
        self.cri_perceptual = self.build_optional_loss(train_opt, 'perceptual_opt')
        self.cri_gan = self.build_optional_loss(train_opt, 'gan_opt')
        if self.cri_gan is None:
            raise ValueError(f'{type(self).__name__}: train.gan_opt is required')
        self.net_d_iters = train_opt.get('net_d_iters', 1)
        self.net_d_init_iters = train_opt.get('net_d_init_iters', 0)
        self.setup_optimizers()
        self.setup_schedulers()

    def _build_ldl(self, train_opt):
        """``train.ldl_opt`` -> ``cri_ldl``; only RealESRGANModel's step has the term."""
        if train_opt.get('ldl_opt'):
            raise NotImplementedError(f'{type(self).__name__}: train.ldl_opt is not supported')
        return None

    def setup_optimizers(self):
        train_opt = self.opt['train']
        optim_opt = dict(train_opt['optim_g'])
        optim_type = optim_opt.pop('type')
        self.optimizer_g = self.get_optimizer(optim_type, self.flat_g.params, **optim_opt)
        self.optimizers.append(self.optimizer_g)
        optim_opt = dict(train_opt['optim_d'])
        optim_type = optim_opt.pop('type')
        if optim_type == 'Adam':
            self.optimizer_d = FusedAdam(self.flat_d, **optim_opt)
        else:
            self.optimizer_d = self.get_optimizer(optim_type, self.flat_d.params, **optim_opt)
        self.optimizers.append(self.optimizer_d)

    def _amp(self):
        return torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.use_amp)

    def _d(self, x):
        with self._amp():
            return self.net_d(x)

    def _set_d_grad(self, flag):
        for p in self.flat_d.params:
            p.requires_grad = flag

    def _update_g(self, current_iter):
        return current_iter % self.net_d_iters == 0 and current_iter > self.net_d_init_iters

    def _g_content_terms(self, loss_dict, pix_gt=None, percep_gt=None):
        """Pixel, LDL and perceptual / style terms of the generator loss and their log entries.  ``pix_gt`` /
        ``percep_gt``: the targets in place of ``self.gt`` (models/realesrgan_model.py)."""
        l_g_total = 0
        if self.cri_pix:
            l_g_pix = self.cri_pix(self.output, self.gt if pix_gt is None else pix_gt)
            l_g_total = l_g_total + l_g_pix
            loss_dict['l_g_pix'] = l_g_pix
        if self.cri_ldl:
            l_g_ldl = self._ldl_term()
            l_g_total = l_g_total + l_g_ldl
            loss_dict['l_g_ldl'] = l_g_ldl
        l_g_total = self._perceptual_terms(l_g_total, loss_dict, keys=('l_g_percep', 'l_g_style'), gt=percep_gt)
        return l_g_total

    def _g_gan_term(self):
        fake_g_pred = self._d(self.output)
        return self.cri_gan(fake_g_pred, True, is_disc=False)

    def _d_terms(self, loss_dict, real=None):
        """The discriminator half: both backwards of the reference, in its order.  ``real``: the real sample in
        place of ``self.gt``."""
        real_d_pred = self._d(self.gt if real is None else real)
        l_d_real = self.cri_gan(real_d_pred, True, is_disc=True)
        loss_dict['l_d_real'] = l_d_real
        loss_dict['out_d_real'] = torch.mean(real_d_pred.detach())
        l_d_real.backward()
        fake_d_pred = self._d(self.output.detach())
        l_d_fake = self.cri_gan(fake_d_pred, False, is_disc=True)
        loss_dict['l_d_fake'] = l_d_fake
        loss_dict['out_d_fake'] = torch.mean(fake_d_pred.detach())
        l_d_fake.backward()

    def optimize_parameters(self, current_iter):
        # optimize net_g: net_d frozen, so its weight gradients are not launched
        self._set_d_grad(False)
        self.optimizer_g.zero_grad()
        with self._amp():
            self.output = self.net_g(self.lq)
        loss_dict = OrderedDict()
        stepped = self._update_g(current_iter)
        if stepped:
            l_g_total = self._g_content_terms(loss_dict)
            l_g_gan = self._g_gan_term()
            l_g_total = l_g_total + l_g_gan
            loss_dict['l_g_gan'] = l_g_gan
            l_g_total.backward()
            if self._fused_step():
                self.optimizer_g.step(ema=self.flat_ema if self.ema_decay > 0 else None, ema_decay=self.ema_decay)
            else:
                self.optimizer_g.step()
        # optimize net_d
        self._set_d_grad(True)
        self.optimizer_d.zero_grad()
        self._d_terms(loss_dict)
        self.optimizer_d.step()
        self.output = self.output.detach()
        self.log_dict = self.reduce_loss_dict(loss_dict)
        if self.ema_decay > 0 and not (stepped and self._fused_step()):
            # the reference averages every iteration, also when the generator did not move
            if self._fused_step():
                ema_copy(self.flat_ema, self.flat_g, self.ema_decay)
            else:
                self.model_ema(decay=self.ema_decay)
        self._eager_steps += 1

    def save(self, epoch, current_iter):
        if hasattr(self, 'net_g_ema'):
            self.save_network([self.net_g, self.net_g_ema], 'net_g', current_iter, param_key=['params', 'params_ema'])
        else:
            self.save_network(self.net_g, 'net_g', current_iter)
        self.save_network(self.net_d, 'net_d', current_iter)
        self.save_training_state(epoch, current_iter)
