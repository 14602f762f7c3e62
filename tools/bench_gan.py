"""GAN timing: one VGGStyleDiscriminator forward + backward (to the input and every parameter) on the HIP engine
against the same modules in stock PyTorch (channels_last, bf16 autocast or fp32), and one ESRGANModel train step
(RRDBNet + discriminator + vgg19 perceptual loss with random weights) of this package, at the geometry of
options/train/ESRGAN/train_ESRGAN_x4.yml: batch 16, LR 32^2 -> HR 128^2.

Per case the median and minimum of --calls device-event timings after --warmup calls, the two discriminator paths
alternating call by call.  One JSON line per case:

    python tools/bench_gan.py [--calls 20] [--warmup 5] [--batch 16] [--no-step]

``--disc unet`` times the UNetDiscriminatorSN instead (num_feat 64, batch 12 at 256^2, the geometry of
options/train/RealESRGAN/train_realesrgan_x4plus.yml) against stock PyTorch with torch's ``spectral_norm`` and
``F.interpolate``, both in training mode, by the same method; no train step is timed for it.

``--trace`` prints instead, per dtype, the ``ktrace`` event spans of one discriminator forward + backward (after two
untraced ones): per kernel name the launches, the summed milliseconds and the algorithmic TFLOP/s and GB/s.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn as nn
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basicsr4rs_amd.archs import build_network  # noqa: E402
from basicsr4rs_amd.models import build_model  # noqa: E402
from basicsr4rs_amd.utils import ktrace  # noqa: E402


class StockDiscriminator(nn.Module):
    """The same layer list in nn modules (NCHW API; run in channels_last)."""

    def __init__(self, num_in_ch=3, nf=64):
        super().__init__()
        mult = (1, 2, 4, 8, 8)
        layers = [nn.Conv2d(num_in_ch, nf, 3, 1, 1), nn.LeakyReLU(0.2), nn.Conv2d(nf, nf, 4, 2, 1, bias=False),
                  nn.BatchNorm2d(nf), nn.LeakyReLU(0.2)]
        for s in range(1, 5):
            cin, cout = nf * mult[s - 1], nf * mult[s]
            layers += [nn.Conv2d(cin, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.2),
                       nn.Conv2d(cout, cout, 4, 2, 1, bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.2)]
        self.features = nn.Sequential(*layers)
        self.linear1, self.linear2 = nn.Linear(nf * 8 * 16, 100), nn.Linear(100, 1)

    def forward(self, x):
        h = self.features(x)
        return self.linear2(F.leaky_relu(self.linear1(h.flatten(1)), 0.2))


class StockUNetSN(nn.Module):
    """The UNetDiscriminatorSN layer list in nn modules with torch's spectral_norm (run in channels_last)."""

    def __init__(self, num_in_ch=3, nf=64):
        super().__init__()
        norm = nn.utils.spectral_norm
        self.conv0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        self.down = nn.ModuleList(norm(nn.Conv2d(nf * m, nf * m * 2, 4, 2, 1, bias=False)) for m in (1, 2, 4))
        self.up = nn.ModuleList(norm(nn.Conv2d(nf * m * 2, nf * m, 3, 1, 1, bias=False)) for m in (4, 2, 1))
        self.conv7 = norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv8 = norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(nf, 1, 3, 1, 1)

    def forward(self, x):
        act = lambda t: F.leaky_relu(t, 0.2)  # noqa: E731
        xs = [act(self.conv0(x))]
        for c in self.down:
            xs.append(act(c(xs[-1])))
        h = xs.pop()
        for c in self.up:
            h = act(c(F.interpolate(h, scale_factor=2, mode='bilinear', align_corners=False))) + xs.pop()
        return self.conv9(act(self.conv8(act(self.conv7(h)))))


def timed(fns, calls, warmup):
    ms = [[] for _ in fns]
    for i in range(warmup + calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms[k].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m)) for m in ms]


def trace(net, x):
    for amp in (True, False):
        for rep in range(3):
            if rep == 2:
                ktrace.start()
            for p in net.parameters():
                p.grad = None
            xx = x.clone().requires_grad_(True)
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                out = net(xx)
            out.sum().backward()
            torch.cuda.synchronize()
        rec = ktrace.stop()
        print(json.dumps(dict(case='discriminator fwd+bwd trace', dtype='bf16' if amp else 'fp32',
                              traced_ms=round(sum(v['ms'] for v in rec.values()), 3))))
        for k, v in sorted(rec.items(), key=lambda kv: -kv[1]['ms']):
            print(f"  {k:40s} n={v['count']:3d} ms={v['ms']:.3f} TFLOP/s={v['flops'] / max(v['ms'], 1e-9) / 1e9:.1f} "
                  f"GB/s={v['bytes'] / max(v['ms'], 1e-9) / 1e6:.0f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None, help='default 16 (--disc vgg) or 12 (--disc unet)')
    ap.add_argument('--disc', choices=['vgg', 'unet'], default='vgg')
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_gan.py needs the GPU')
    torch.manual_seed(0)
    unet = args.disc == 'unet'
    B = args.batch or (12 if unet else 16)
    if unet:
        hip = build_network(dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=64, skip_connection=True)).cuda()
        stock = StockUNetSN().cuda().to(memory_format=torch.channels_last)
        x = torch.rand(B, 3, 256, 256, device='cuda')
    else:
        hip = build_network(dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64, input_size=128)).cuda()
        stock = StockDiscriminator().cuda().to(memory_format=torch.channels_last)
        x = torch.rand(B, 3, 128, 128, device='cuda')
    if args.trace:
        trace(hip, x)
        return
    for amp in (True, False):

        def run(net, xin):

            def fn():
                for p in net.parameters():
                    p.grad = None
                xx = xin.detach().requires_grad_(True)
                with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                    out = net(xx)
                out.float().sum().backward()

            return fn

        (h_med, h_min), (s_med, s_min) = timed([run(hip, x), run(stock, x.contiguous(memory_format=torch.channels_last))],
                                               args.calls, args.warmup)
        print(json.dumps(dict(case='UNetDiscriminatorSN fwd+bwd' if unet else 'discriminator fwd+bwd', batch=B,
                              dtype='bf16' if amp else 'fp32',
                              hip_ms=round(h_med, 3), hip_min_ms=round(h_min, 3), torch_ms=round(s_med, 3),
                              torch_min_ms=round(s_min, 3))), flush=True)
    if args.no_step or unet:
        return
    for amp in (True, False):
        opt = dict(model_type='ESRGANModel', is_train=True, dist=False, num_gpu=1, path={},
                   network_g=dict(type='RRDBNet', num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32),
                   network_d=dict(type='VGGStyleDiscriminator', num_in_ch=3, num_feat=64),
                   train=dict(ema_decay=0.999, use_amp=amp,
                              optim_g=dict(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99]),
                              optim_d=dict(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99]),
                              scheduler=dict(type='MultiStepLR', milestones=[50000], gamma=0.5),
                              pixel_opt=dict(type='L1Loss', loss_weight=1e-2, reduction='mean'),
                              perceptual_opt=dict(type='PerceptualLoss', layer_weights={'conv5_4': 1}, vgg_type='vgg19',
                                                  use_input_norm=True, range_norm=False, perceptual_weight=1.0,
                                                  style_weight=0, criterion='l1', pretrained=False),
                              gan_opt=dict(type='GANLoss', gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0,
                                           loss_weight=5e-3), net_d_iters=1, net_d_init_iters=0))
        model = build_model(opt)
        model.feed_data({'lq': torch.rand(B, 3, 32, 32), 'gt': torch.rand(B, 3, 128, 128)})
        it = [0]

        def step():
            it[0] += 1
            model.optimize_parameters(it[0])

        ((med, mn), ) = timed([step], args.calls, args.warmup)
        print(json.dumps(dict(case='ESRGAN step (RRDBNet 23 blocks + D + vgg19 conv5_4)', batch=B,
                              dtype='bf16' if amp else 'fp32', hip_ms=round(med, 3), hip_min_ms=round(mn, 3))), flush=True)
        del model


if __name__ == '__main__':
    main()
