"""EDVR model (mirror of basicsr/models/edvr_model.py:7-62) on top of SRModel: flat parameters, fused Adam + EMA,
``train.use_amp`` as in SRModel; ``feed_data`` takes the 5-D ``lq`` (b, t, c, h, w).

``train.dcn_lr_mul``: 1 (every shipped option file) keeps the fused optimizer; any other value builds the reference's
two parameter groups (normal first, then the names containing ``dcn``) on ``torch.optim.Adam``.
``train.tsa_iter``: as the reference, at iteration 1 every parameter whose name lacks ``fusion`` is frozen and at
iteration ``tsa_iter`` all are released, before that step runs.  With the fused optimizer the flat vector is stepped
by ranges (utils/flat.py:RangedFusedAdam: ``fusion.*`` is one contiguous range): a frozen range keeps its bits and
its step count, so after the release its Adam state is what ``torch.optim.Adam`` holds for parameters whose gradient
was ``None`` until then; the EMA follows all parameters throughout.

Not built: HIP-graph capture of the step (``DCNv2Pack``'s offset check reads the host) and video validation
(``VideoBaseModel.dist_validation`` over ``VideoTestDataset``).
"""
from ..utils.flat import RangedFusedAdam
from ..utils.logger import get_root_logger
from ..utils.registry import MODEL_REGISTRY
from .sr_model import SRModel


@MODEL_REGISTRY.register()
class EDVRModel(SRModel):

    def __init__(self, opt):
        super().__init__(opt)
        if self.is_train:
            self.train_tsa_iter = opt['train'].get('tsa_iter')

    def init_training_settings(self):
        if self.opt['train'].get('cuda_graph', False):
            raise NotImplementedError('EDVRModel: train.cuda_graph is not supported: DCNv2Pack checks the mean absolute '
                                      'offset on the host in every forward, which a captured step cannot do')
        super().init_training_settings()

    def setup_optimizers(self):
        train_opt = self.opt['train']
        dcn_lr_mul = train_opt.get('dcn_lr_mul', 1)
        get_root_logger().info(f'Multiple the learning rate for dcn with {dcn_lr_mul}.')
        optim_opt = dict(train_opt['optim_g'])
        optim_type = optim_opt.pop('type')
        net = self.get_bare_model(self.net_g)
        if dcn_lr_mul == 1:
            if optim_type == 'Adam' and train_opt.get('tsa_iter'):
                ids = [int('fusion' in name) for name, p in net.named_parameters() if p.requires_grad]
                self.optimizer_g = RangedFusedAdam(self.flat_g, ids, **optim_opt)
            else:
                self.optimizer_g = self.get_optimizer(optim_type, self.flat_g.params, **optim_opt)
        else:  # separate dcn params and normal params for different lr
            normal_params, dcn_params = [], []
            for name, param in net.named_parameters():
                (dcn_params if 'dcn' in name else normal_params).append(param)
            optim_params = [
                {'params': normal_params, 'lr': optim_opt['lr']},  # normal params first
                {'params': dcn_params, 'lr': optim_opt['lr'] * dcn_lr_mul},
            ]
            self.optimizer_g = self.get_optimizer(optim_type, optim_params, **optim_opt)
        self.optimizers.append(self.optimizer_g)

    def optimize_parameters(self, current_iter):
        if self.train_tsa_iter:
            net = self.get_bare_model(self.net_g)
            if current_iter == 1:
                get_root_logger().info(f'Only train TSA module for {self.train_tsa_iter} iters.')
                for name, param in net.named_parameters():
                    if 'fusion' not in name:
                        param.requires_grad = False
            elif current_iter == self.train_tsa_iter:
                get_root_logger().warning('Train all the parameters.')
                for param in net.parameters():
                    param.requires_grad = True
        super().optimize_parameters(current_iter)

    def sync_gradients(self):
        super().sync_gradients()
        if not self._fused_step():
            # torch.optim.Adam skips a parameter whose gradient is None; a frozen parameter's gradient is a view
            # of the flat gradient buffer (zeros), which it would step and count
            for p in self.flat_g.params:
                if not p.requires_grad:
                    p.grad = None

    def validation(self, dataloader, current_iter, tb_logger, save_img=False):
        raise NotImplementedError('EDVRModel: video validation (VideoBaseModel.dist_validation: folder-wise metrics over '
                                  'VideoTestDataset) is not built yet; it comes with the REDS / Vimeo90K / '
                                  'VideoTestDataset readers')
