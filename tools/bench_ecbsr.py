"""ECBSR timing at the shape of options/train/ECBSR/train_ECBSR_x4_m4c16_prelu.yml: batch 32, Y, 64^2 -> 256^2,
m4c16 (4 blocks, 16 channels, PReLU), L1 loss, Adam.

  step      SRModel train steps on the collapsed HIP path, fp32 and bf16 (``use_amp``), eager and captured
            (``train.cuda_graph``): device events around ``--steps`` steps after ``--warmup``, ``--repeats`` times;
            median and minimum of the per-step averages.
  kernels   one traced eager step (utils/ktrace.py): per kernel name the launch count, the event time, the
            algorithmic bytes and FLOPs, and the total launch count of the step's network part.
  stock     stock PyTorch (torch.nn.functional on the GPU, torch.optim.Adam) running the five-branch training form of
            tests/_ecbsr_ref.py on the same shape, fp32 and bf16 autocast, the same way.

    python tools/bench_ecbsr.py [--steps 20] [--warmup 5] [--repeats 3] [--batch 32] [--only step|kernels|stock]

One JSON line per case.  Times only: correctness is the tests' business.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from basicsr4rs_amd.models import build_model  # noqa: E402
from basicsr4rs_amd.utils import ktrace  # noqa: E402
from tests import _ecbsr_ref as R  # noqa: E402

NET = dict(type='ECBSR', num_in_ch=1, num_out_ch=1, num_block=4, num_channel=16, with_idt=False, act_type='prelu',
           scale=4)


def _opt(amp, graph):
    return dict(model_type='SRModel', is_train=True, dist=False, num_gpu=1, scale=4, path={}, network_g=dict(NET),
                train=dict(ema_decay=0, use_amp=amp, cuda_graph=graph,
                           optim_g=dict(type='Adam', lr=5e-4, weight_decay=0, betas=[0.9, 0.99]),
                           scheduler=dict(type='MultiStepLR', milestones=[1600000], gamma=0.5),
                           pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean')))


def _batch(n):
    g = torch.Generator().manual_seed(1)
    return {'lq': torch.rand(n, 1, 64, 64, generator=g), 'gt': torch.rand(n, 1, 256, 256, generator=g)}


def timed_steps(step, steps, warmup, repeats):
    for _ in range(warmup):
        step()
    per = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            step()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / steps)
    return statistics.median(per), min(per)


def bench_step(args):
    for amp in (False, True):
        for graph in (False, True):
            torch.manual_seed(0)
            model = build_model(_opt(amp, graph))
            model.feed_data(_batch(args.batch))
            it = [0]

            def step():
                it[0] += 1
                model.optimize_parameters(it[0])

            med, mn = timed_steps(step, args.steps, args.warmup, args.repeats)
            assert graph == (model._graph is not None)
            print(json.dumps(dict(case='ECBSR m4c16 x4 train step, collapsed HIP path', batch=args.batch, lq=[64, 64],
                                  dtype='bf16' if amp else 'fp32', mode='captured' if graph else 'eager',
                                  step_ms=round(med, 4), step_min_ms=round(mn, 4),
                                  l_pix=round(float(model.get_current_log()['l_pix']), 4))), flush=True)


def bench_kernels(args):
    for amp in (False, True):
        torch.manual_seed(0)
        model = build_model(_opt(amp, False))
        model.feed_data(_batch(args.batch))
        for it in range(1, 4):
            model.optimize_parameters(it)
        torch.cuda.synchronize()
        ktrace.start()
        model.optimize_parameters(4)
        recs = ktrace.stop()
        total = 0
        for name, d in sorted(recs.items()):
            total += d['launches']
            print(json.dumps(dict(case='kernel', dtype='bf16' if amp else 'fp32', name=name, calls=d['count'],
                                  launches=d['launches'], event_ms=round(d['ms'], 4),
                                  mbytes=round(d['bytes'] / 1e6, 3), gflop=round(d['flops'] / 1e9, 3),
                                  gbs=round(d['bytes'] / max(d['ms'], 1e-9) / 1e6, 1))), flush=True)
        print(json.dumps(dict(case='traced launches per step (network forward + backward; plus the layout change, '
                                   'the L1 loss and the fused Adam)', dtype='bf16' if amp else 'fp32',
                              launches=total)), flush=True)


def bench_stock(args):
    from basicsr4rs_amd.archs import build_network
    for amp in (False, True):
        torch.manual_seed(0)
        sd = {k: v.cuda() for k, v in build_network(dict(NET)).state_dict().items()}
        params = {k: (v.requires_grad_(True) if not k.endswith('.mask') else v) for k, v in sd.items()}
        opt = torch.optim.Adam([v for v in params.values() if v.requires_grad], lr=5e-4, betas=(0.9, 0.99))
        batch = {k: v.cuda() for k, v in _batch(args.batch).items()}

        def step():
            opt.zero_grad()
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                out = R.forward(params, batch['lq'], scale=4, with_idt=False)
            F.l1_loss(out.float(), batch['gt']).backward()
            opt.step()

        med, mn = timed_steps(step, args.steps, args.warmup, args.repeats)
        print(json.dumps(dict(case='ECBSR m4c16 x4 train step, stock PyTorch, five-branch form', batch=args.batch,
                              lq=[64, 64], dtype='bf16 autocast' if amp else 'fp32', mode='eager',
                              step_ms=round(med, 4), step_min_ms=round(mn, 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--only', choices=('step', 'kernels', 'stock'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ecbsr.py needs the GPU')
    for name, fn in (('step', bench_step), ('kernels', bench_kernels), ('stock', bench_stock)):
        if args.only in (None, name):
            fn(args)


if __name__ == '__main__':
    main()
