"""RegisteredLoss as ``train.pixel_opt`` of a tiny model (the SRCNN 6 -> 6 x3 network and the run pattern of
tests/test_l2s_model_gpu.py; (-1, 1, 0.5, l1) on 24 x 24 ground truth): four steps with and without
``train.cuda_graph`` give the same logged ``l_pix`` and the same parameters bit for bit, and the loss decreases on a
batch whose target is a shifted copy of what the net can produce.

SRRSModel, the model the L2S option files use, reads its loss on the host every step (the reference's non-finite
check) and never captures, so with it the option changes nothing; SRModel does capture (steps 1-2 eager, step 3
captured, step 4 a replay): there the loss call -- the four launches, the selected index read back on the device and
the allocations of the autograd node -- runs inside the HIP graph."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

NET6 = dict(type='SRCNN', num_in_ch=6, num_out_ch=6, upscale=3)
PIXEL = dict(type='RegisteredLoss', start=-1, end=1, step=0.5, loss_func='l1', loss_weight=1.0, reduction='mean')


def _opt(model_type, amp, graph):
    return dict(model_type=model_type, name='registered', is_train=True, dist=False, num_gpu=1, scale=3, path={},
                network_g=dict(NET6),
                train=dict(ema_decay=0.999, use_amp=amp, cuda_graph=graph,
                           optim_g=dict(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99]),
                           scheduler=dict(type='MultiStepLR', milestones=[100], gamma=0.5), pixel_opt=dict(PIXEL)))


def _batch():
    """gt: the bicubic x3 of lq -- what SRCNN's first stage produces -- moved one pixel down and right."""
    lq = torch.rand(2, 6, 8, 8, generator=torch.Generator().manual_seed(5)) * 2 - 1
    up = F.interpolate(lq, scale_factor=3, mode='bicubic', align_corners=False)
    return {'lq': lq, 'gt': torch.roll(up, shifts=(1, 1), dims=(2, 3))}


def _run(model_type, amp, graph):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(_opt(model_type, amp, graph))
    assert type(model.cri_pix).__name__ == 'RegisteredLoss'
    losses, shifts = [], []
    for it in range(1, 5):
        model.feed_data(_batch())
        model.update_learning_rate(it)
        model.optimize_parameters(it)
        losses.append(model.get_current_log()['l_pix'])
        shifts.append(model.cri_pix.last_shift.tolist())
    net = model.get_bare_model(model.net_g)
    return model, losses, shifts, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize('amp', [False, True], ids=['fp32', 'amp'])
@pytest.mark.parametrize('model_type', ['SRRSModel', 'SRModel'])
def test_registered_loss_in_a_train_step(cuda, model_type, amp):
    eager, le, se, pe = _run(model_type, amp, False)
    graph, lg, sg, pg = _run(model_type, amp, True)
    print(f'{model_type} amp={amp}: l_pix {le}, shifts {se}')
    assert eager._graph is None and (graph._graph is not None) == (model_type == 'SRModel')
    assert le == lg and se == sg
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
    assert all(v == v and abs(v) != float('inf') and v > 0 for v in le)
    assert le[-1] < le[0]
    assert all(len(s) == 2 and all(0 <= i < 25 for i in s) for s in se)
