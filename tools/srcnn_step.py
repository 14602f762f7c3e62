#!/usr/bin/env python
"""Time the SRCNN train step at the S2N geometry (4 bands, x4, batch 32, LR 64^2 -> HR 256^2, bf16).

Default: SRRSModel + SRCNN on the HIP engine (train.use_amp, train.cuda_graph as in the request;
SRRSModel checks its loss on the host every step and so runs eagerly -- ``--model SRModel`` times the
captured step).  ``--stock``: the same three-conv net in stock PyTorch (channels_last, bf16 autocast,
torch.optim.Adam, L1 loss) on the same GPU.  The step is timed with HIP events after warm-up; one
JSON line is printed, with the per-kernel ktrace spans of one extra traced step for the HIP side.

    python tools/srcnn_step.py [--stock] [--steps 20] [--warmup 5] [--batch 32] [--lr-size 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def run_hip(a):
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    from basicsr4rs_amd.utils import ktrace
    opt = dict(model_type=a.model, is_train=True, dist=False, num_gpu=1, path={}, scale=4,
               network_g=dict(type='SRCNN', num_in_ch=a.bands, num_out_ch=a.bands, upscale=4),
               train=dict(ema_decay=0.999, use_amp=True, cuda_graph=True,
                          optim_g=dict(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99]),
                          scheduler=dict(type='MultiStepLR', milestones=[10**9], gamma=0.5),
                          pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean')))
    torch.manual_seed(0)
    model = build_model(opt)
    g = torch.Generator().manual_seed(0)
    data = {'lq': (torch.rand(a.batch, a.bands, a.lr_size, a.lr_size, generator=g) * 2 - 1).cuda(),
            'gt': (torch.rand(a.batch, a.bands, 4 * a.lr_size, 4 * a.lr_size, generator=g) * 2 - 1).cuda()}
    it = [0]

    def step():
        it[0] += 1
        model.feed_data(data)
        model.optimize_parameters(it[0])

    ms = _time_steps(step, a.steps, a.warmup)
    # one traced eager step for the per-kernel spans (events around every launch)
    graph, model._graph = model._graph, None
    use_graph, model.use_graph = model.use_graph, False
    ktrace.start()
    step()
    spans = ktrace.stop()
    model._graph, model.use_graph = graph, use_graph
    kern = {n: dict(count=d['count'], ms=round(d['ms'], 4), tflops=round(d['flops'] / d['ms'] / 1e9, 2) if d['ms'] else 0,
                    gbps=round(d['bytes'] / d['ms'] / 1e6, 1) if d['ms'] else 0) for n, d in spans.items()}
    return dict(side='hip', model=a.model, captured=graph is not None, ms_per_step=round(ms, 4), kernels=kern)


def run_stock(a):
    from torch import nn
    from torch.nn import functional as F

    class Net(nn.Module):

        def __init__(self, c):
            super().__init__()
            self.conv1 = nn.Conv2d(c, 64, 9, padding=4)
            self.conv2 = nn.Conv2d(64, 32, 5, padding=2)
            self.conv3 = nn.Conv2d(32, c, 5, padding=2)

        def forward(self, x):
            x = F.interpolate(x, scale_factor=4, mode='bicubic', align_corners=True)
            return self.conv3(F.relu(self.conv2(F.relu(self.conv1(x)))))

    torch.manual_seed(0)
    net = Net(a.bands).cuda().to(memory_format=torch.channels_last)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.9, 0.99))
    g = torch.Generator().manual_seed(0)
    lq = (torch.rand(a.batch, a.bands, a.lr_size, a.lr_size, generator=g) * 2 - 1).cuda().contiguous(
        memory_format=torch.channels_last)
    gt = (torch.rand(a.batch, a.bands, 4 * a.lr_size, 4 * a.lr_size, generator=g) * 2 - 1).cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = net(lq)
        F.l1_loss(out.float(), gt).backward()
        opt.step()

    ms = _time_steps(step, a.steps, a.warmup)
    return dict(side='stock', ms_per_step=round(ms, 4))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--stock', action='store_true')
    p.add_argument('--model', default='SRRSModel', choices=('SRRSModel', 'SRModel'))
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--lr-size', type=int, default=64)
    p.add_argument('--bands', type=int, default=4)
    a = p.parse_args()
    res = run_stock(a) if a.stock else run_hip(a)
    res.update(batch=a.batch, lr_size=a.lr_size, bands=a.bands, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
