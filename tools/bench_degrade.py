"""Degradation timing: the full ``feed_data`` synthesis of RealESRGANModel (USM sharpening, the second-order
degradation, crop, training-pair pool, second USM) on the HIP kernels of csrc/degrade.hip against the same sequence
written with stock torch ops in this file (grouped ``conv2d`` with a reflect pad for filter2D, the dense 51 x 51
convolution for USM, ``F.interpolate``, ``torch.unique`` per sample for the Poisson levels, the ``tensordot`` form of
DiffJPEG), at the geometry of options/train/RealESRGAN/train_realesrgan_x4plus.yml: batch 12, gt 400^2, scale 4,
that file's probabilities and ranges.  Both sides take the same host draws (the generators are re-seeded per call),
so they run the same branches; the two alternate call by call.  Then every op alone, by the same method, and
(unless ``--no-step``) one RealESRGANModel ``optimize_parameters`` at that file's networks (RRDBNet, UNetDiscriminatorSN,
vgg19 perceptual loss with random weights; gt_size 256) for the share of a step that ``feed_data`` takes.

Per case the median and minimum of --calls device-event timings after --warmup calls.  One JSON line per case:

    python tools/bench_degrade.py [--calls 20] [--warmup 5] [--batch 12] [--no-step]
"""
import argparse
import itertools
import json
import math
import os
import random
import statistics
import sys

import numpy as np
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basicsr4rs_amd.data.degradations import circular_lowpass_kernel, random_mixed_kernels  # noqa: E402
from basicsr4rs_amd.data.transforms import paired_random_crop  # noqa: E402
from basicsr4rs_amd.models.realesrgan_degradation import DegradationMixin  # noqa: E402
from basicsr4rs_amd.ops import degrade as D  # noqa: E402

# the degradation settings of train_realesrgan_x4plus.yml
OPT = dict(scale=4, gt_size=256, queue_size=180, resize_prob=[0.2, 0.7, 0.1], resize_range=[0.15, 1.5],
           gaussian_noise_prob=0.5, noise_range=[1, 30], poisson_scale_range=[0.05, 3], gray_noise_prob=0.4,
           jpeg_range=[30, 95], second_blur_prob=0.8, resize_prob2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2],
           gaussian_noise_prob2=0.5, noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5], gray_noise_prob2=0.4,
           jpeg_range2=[30, 95])
KERNELS = dict(kernel_list=['iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso'],
               kernel_prob=[0.45, 0.25, 0.12, 0.03, 0.12, 0.03])


# ------------------------------------------------------------------------------------- the stock-torch side


def stock_filter2d(img, kernel):
    k = kernel.size(-1)
    b, c, h, w = img.size()
    img = F.pad(img, (k // 2, ) * 4, mode='reflect')
    ph, pw = img.size()[-2:]
    if kernel.size(0) == 1:
        return F.conv2d(img.view(b * c, 1, ph, pw), kernel.view(1, 1, k, k)).view(b, c, h, w)
    kernel = kernel.view(b, 1, k, k).repeat(1, c, 1, 1).view(b * c, 1, k, k)
    return F.conv2d(img.view(1, b * c, ph, pw), kernel, groups=b * c).view(b, c, h, w)


def stock_usm(img, kernel, weight=0.5, threshold=10):
    blur = stock_filter2d(img, kernel)
    residual = img - blur
    mask = (torch.abs(residual) * 255 > threshold).float()
    soft = stock_filter2d(mask, kernel)
    sharp = torch.clip(img + weight * residual, 0, 1)
    return soft * sharp + (1 - soft) * img


def _finish(out, clip=True):
    return torch.clamp(out, 0, 1) if clip else out


def stock_gaussian(img, sigma_range, gray_prob):
    b, _, h, w = img.size()
    sigma = (torch.rand(b, device=img.device) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]).view(b, 1, 1, 1)
    gray = (torch.rand(b, device=img.device) < gray_prob).float().view(b, 1, 1, 1)
    noise = torch.randn_like(img) * sigma / 255.
    if torch.sum(gray) > 0:  # a host sync, as in the reference
        noise_gray = (torch.randn(h, w, device=img.device) * sigma / 255.).view(b, 1, h, w)
        noise = noise * (1 - gray) + noise_gray * gray
    return _finish(img + noise)


def _levels(x):
    x = torch.clamp((x * 255.0).round(), 0, 255) / 255.
    vals = [2**np.ceil(np.log2(len(torch.unique(x[i])))) for i in range(x.size(0))]  # a host sync per sample
    return x, x.new_tensor(vals).view(-1, 1, 1, 1)


def stock_poisson(img, scale_range, gray_prob):
    b, _, h, w = img.size()
    scale = (torch.rand(b, device=img.device) * (scale_range[1] - scale_range[0]) + scale_range[0]).view(b, 1, 1, 1)
    gray = (torch.rand(b, device=img.device) < gray_prob).float().view(b, 1, 1, 1)
    cal_gray = torch.sum(gray) > 0
    if cal_gray:
        g, vals = _levels(0.2989 * img[:, 0:1] + 0.587 * img[:, 1:2] + 0.114 * img[:, 2:3])
        noise_gray = (torch.poisson(g * vals) / vals - g).expand(b, 3, h, w)
    q, vals = _levels(img)
    noise = torch.poisson(q * vals) / vals - q
    if cal_gray:
        noise = noise * (1 - gray) + noise_gray * gray
    return _finish(img + noise * scale)


class StockJPEG:
    """DiffJPEG.forward with the dense [8, 8, 8, 8] contraction, torch.round."""

    def __init__(self, device):
        t = np.zeros((8, 8, 8, 8), dtype=np.float32)
        for x, y, u, v in itertools.product(range(8), repeat=4):
            t[x, y, u, v] = np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)
        self.fwd = torch.from_numpy(t).to(device)
        self.inv = self.fwd.permute(2, 3, 0, 1).contiguous()
        alpha = np.array([1. / np.sqrt(2)] + [1] * 7)
        self.alpha = torch.from_numpy(np.outer(alpha, alpha)).float().to(device)
        self.scale = torch.from_numpy(np.outer(alpha, alpha) * 0.25).float().to(device)
        yt = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                       [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77],
                       [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
                       [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float32).T
        ct = np.full((8, 8), 99, dtype=np.float32)
        ct[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]).T
        self.tables = (torch.from_numpy(yt.copy()).to(device), torch.from_numpy(ct).to(device))
        self.to_ycc = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]],
                                   device=device).t()
        self.to_rgb = torch.tensor([[1., 0., 1.402], [1, -0.344136, -0.714136], [1, 1.772, 0]], device=device).t()
        self.shift = torch.tensor([0., 128., 128.], device=device)

    def __call__(self, x, quality):
        b = x.size(0)
        factor = quality.clone()
        for i in range(b):  # the reference's host loop
            factor[i] = 5000. / factor[i] / 100. if factor[i] < 50 else (200. - factor[i] * 2) / 100.
        h, w = x.size()[-2:]
        x = F.pad(x, (0, -w % 16, 0, -h % 16))
        hp, wp = x.size()[-2:]
        img = torch.tensordot((x * 255).permute(0, 2, 3, 1), self.to_ycc, dims=1) + self.shift
        comps = []
        for c in range(3):
            p, ch, cw = img[..., c], hp, wp
            if c:
                p = F.avg_pool2d(p.unsqueeze(1), 2, 2).squeeze(1)
                ch, cw = hp // 2, wp // 2
            blk = p.reshape(b, ch // 8, 8, cw // 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(b, -1, 8, 8)
            d = self.scale * torch.tensordot(blk - 128, self.fwd, dims=2)
            table = self.tables[min(c, 1)].expand(b, 1, 8, 8) * factor.view(b, 1, 1, 1)
            d = torch.round(d / table) * table
            rec = 0.25 * torch.tensordot(d * self.alpha, self.inv, dims=2) + 128
            rec = rec.view(b, ch // 8, cw // 8, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(b, ch, cw)
            if c:
                rec = rec.repeat_interleave(2, 1).repeat_interleave(2, 2)
            comps.append(rec)
        ycc = torch.stack(comps, 3) - self.shift
        rgb = torch.tensordot(ycc, self.to_rgb, dims=1).permute(0, 3, 1, 2)
        return (torch.clamp(rgb, 0, 255) / 255)[:, :, :h, :w]


class Pool:
    """The training-pair pool of the reference, for both sides."""

    def __init__(self, size):
        self.size, self.ptr = size, 0

    def __call__(self, lq, gt):
        b = lq.size(0)
        if not hasattr(self, 'lr'):
            self.lr = torch.zeros(self.size, *lq.shape[1:], device=lq.device)
            self.gt = torch.zeros(self.size, *gt.shape[1:], device=gt.device)
        if self.ptr == self.size:
            idx = torch.randperm(self.size)
            self.lr, self.gt = self.lr[idx], self.gt[idx]
            out = self.lr[0:b].clone(), self.gt[0:b].clone()
            self.lr[0:b], self.gt[0:b] = lq, gt
            return out
        self.lr[self.ptr:self.ptr + b], self.gt[self.ptr:self.ptr + b] = lq, gt
        self.ptr += b
        return lq, gt


def _scale(prob, rng):
    kind = random.choices(['up', 'down', 'keep'], prob)[0]
    return np.random.uniform(1, rng[1]) if kind == 'up' else (np.random.uniform(rng[0], 1) if kind == 'down' else 1)


def stock_feed(data, usm_kernel, jpeger, pool, o=OPT):
    gt = data['gt']
    gt_usm = stock_usm(gt, usm_kernel)
    ori_h, ori_w = gt.size()[2:4]
    out = stock_filter2d(gt_usm, data['kernel1'])
    scale = _scale(o['resize_prob'], o['resize_range'])
    out = F.interpolate(out, scale_factor=scale, mode=random.choice(['area', 'bilinear', 'bicubic']))
    if np.random.uniform() < o['gaussian_noise_prob']:
        out = stock_gaussian(out, o['noise_range'], o['gray_noise_prob'])
    else:
        out = stock_poisson(out, o['poisson_scale_range'], o['gray_noise_prob'])
    out = jpeger(torch.clamp(out, 0, 1), out.new_zeros(out.size(0)).uniform_(*o['jpeg_range']))
    if np.random.uniform() < o['second_blur_prob']:
        out = stock_filter2d(out, data['kernel2'])
    scale = _scale(o['resize_prob2'], o['resize_range2'])
    out = F.interpolate(out, size=(int(ori_h / o['scale'] * scale), int(ori_w / o['scale'] * scale)),
                        mode=random.choice(['area', 'bilinear', 'bicubic']))
    if np.random.uniform() < o['gaussian_noise_prob2']:
        out = stock_gaussian(out, o['noise_range2'], o['gray_noise_prob2'])
    else:
        out = stock_poisson(out, o['poisson_scale_range2'], o['gray_noise_prob2'])
    final = (ori_h // o['scale'], ori_w // o['scale'])
    if np.random.uniform() < 0.5:
        out = F.interpolate(out, size=final, mode=random.choice(['area', 'bilinear', 'bicubic']))
        out = stock_filter2d(out, data['sinc_kernel'])
        out = jpeger(torch.clamp(out, 0, 1), out.new_zeros(out.size(0)).uniform_(*o['jpeg_range2']))
    else:
        out = jpeger(torch.clamp(out, 0, 1), out.new_zeros(out.size(0)).uniform_(*o['jpeg_range2']))
        out = F.interpolate(out, size=final, mode=random.choice(['area', 'bilinear', 'bicubic']))
        out = stock_filter2d(out, data['sinc_kernel'])
    lq = torch.clamp((out * 255.0).round(), 0, 255) / 255.
    (gt, gt_usm), lq = paired_random_crop([gt, gt_usm], lq, o['gt_size'], o['scale'])
    lq, gt = pool(lq, gt)
    return lq.contiguous(), gt, stock_usm(gt, usm_kernel)


# ---------------------------------------------------------------------------------------------- the HIP side


class HipFeed(DegradationMixin):
    """feed_data of RealESRGANModel without the networks."""

    def __init__(self, device):
        self.opt, self.device, self.is_train = dict(OPT), device, True
        self._init_degradation()

    def feed(self, data):
        self.gt = data['gt']
        self.gt_usm = self.usm_sharpener(self.gt)
        self.kernel1, self.kernel2, self.sinc_kernel = data['kernel1'], data['kernel2'], data['sinc_kernel']
        self.lq = self._degrade(self.gt_usm)
        (self.gt, self.gt_usm), self.lq = paired_random_crop([self.gt, self.gt_usm], self.lq, self.opt['gt_size'],
                                                             self.opt['scale'])
        self._dequeue_and_enqueue()
        self.gt = self.gt.contiguous()
        self.gt_usm = self.usm_sharpener(self.gt)
        self.lq = self.lq.contiguous()


def make_batch(B, device, seed=0):
    random.seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    # a smooth image plus texture, so that the USM mask and the 8-bit levels look like a photograph's
    base = F.interpolate(torch.rand(B, 3, 25, 25, generator=g), size=(400, 400), mode='bicubic', align_corners=False)
    gt = torch.clamp(base + 0.05 * torch.randn(B, 3, 400, 400, generator=g), 0, 1)

    def blur(sigma):
        ks = [random.choice([7, 9, 11, 13, 15, 17, 19, 21]) for _ in range(B)]
        out = []
        for k in ks:
            kern = random_mixed_kernels(KERNELS['kernel_list'], KERNELS['kernel_prob'], k, sigma, sigma, [-math.pi, math.pi],
                                        [0.5, 4], [1, 2], noise_range=None)
            p = (21 - k) // 2
            out.append(torch.FloatTensor(np.pad(kern, ((p, p), (p, p)))))
        return torch.stack(out)

    sinc = torch.stack([torch.FloatTensor(circular_lowpass_kernel(np.random.uniform(np.pi / 3, np.pi), 13, pad_to=21))
                        for _ in range(B)])
    return {'gt': gt.to(device), 'kernel1': blur([0.2, 3]).to(device), 'kernel2': blur([0.2, 1.5]).to(device),
            'sinc_kernel': sinc.to(device)}


def timed(fns, calls, warmup, reseed=False):
    ms = [[] for _ in fns]
    for i in range(warmup + calls):
        for k, fn in enumerate(fns):
            if reseed:  # the same host and device draws on every side: the same branches
                random.seed(1000 + i)
                np.random.seed(1000 + i)
                torch.manual_seed(1000 + i)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms[k].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m)) for m in ms]


def report(case, names, res, **extra):
    rec = dict(case=case, **extra)
    for n, (med, mn) in zip(names, res):
        rec[f'{n}_ms_median'], rec[f'{n}_ms_min'] = round(med, 4), round(mn, 4)
    if tuple(names) == ('hip', 'stock'):
        rec['stock_over_hip'] = round(res[1][0] / res[0][0], 2)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_degrade.py needs the GPU')
    dev = torch.device('cuda')
    B = args.batch
    data = make_batch(B, dev)
    hip = HipFeed(dev)
    usm_kernel = hip.usm_sharpener.kernel
    jpeger = StockJPEG(dev)
    pool = Pool(OPT['queue_size'])
    names = ('hip', 'stock')
    with torch.no_grad():
        feed = report('feed_data', names, timed([lambda: hip.feed(data), lambda: stock_feed(data, usm_kernel, jpeger, pool)],
                                                args.calls, args.warmup, reseed=True), batch=B, gt=400, scale=4)
        x = data['gt']
        taps = hip.usm_sharpener.taps
        q = torch.full((B, ), 60.0, device=dev)
        sig, gray = torch.full((B, ), 10.0, device=dev), (torch.arange(B, device=dev) % 2).float()
        ops = [
            ('usm_sharp 400^2', lambda: D.usm_sharp(x, taps), lambda: stock_usm(x, usm_kernel)),
            ('filter2d k21 400^2', lambda: D.filter2d(x, data['kernel1']), lambda: stock_filter2d(x, data['kernel1'])),
            ('filter2d k21 100^2 shared', lambda: D.filter2d(x[..., :100, :100], data['sinc_kernel'][:1]),
             lambda: stock_filter2d(x[..., :100, :100], data['sinc_kernel'][:1])),
        ]
        for mode in ('area', 'bilinear', 'bicubic'):
            ops.append((f'resize {mode} 400^2 x0.6', lambda m=mode: D.resize(x, scale_factor=0.6, mode=m),
                        lambda m=mode: F.interpolate(x, scale_factor=0.6, mode=m)))
        ops += [
            ('gaussian noise 400^2', lambda: D.gaussian_noise(x, sig, gray), lambda: stock_gaussian(x, (10, 10), 0.5)),
            ('poisson noise 400^2', lambda: D.poisson_noise(x, sig * 0.1, gray), lambda: stock_poisson(x, (1, 1), 0.5)),
            ('jpeg 400^2', lambda: D.jpeg(x, q), lambda: jpeger(x, q)),
            ('jpeg 100^2', lambda: D.jpeg(x[..., :100, :100], q), lambda: jpeger(x[..., :100, :100].contiguous(), q)),
        ]
        for case, f_hip, f_stock in ops:
            report(case, names, timed([f_hip, f_stock], args.calls, args.warmup), batch=B)
    if args.no_step:
        return
    from basicsr4rs_amd.models import build_model
    vgg = dict(type='PerceptualLoss', layer_weights={'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1},
               vgg_type='vgg19', use_input_norm=True, perceptual_weight=1.0, style_weight=0, range_norm=False,
               criterion='l1', pretrained=False)
    adam = dict(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99])
    opt = dict(OPT, model_type='RealESRGANModel', is_train=True, dist=False, num_gpu=1, path={}, l1_gt_usm=True,
               percep_gt_usm=True, gan_gt_usm=False,
               network_g=dict(type='RRDBNet', num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32),
               network_d=dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=64, skip_connection=True),
               train=dict(ema_decay=0.999, optim_g=dict(adam), optim_d=dict(adam), use_amp=True,
                          scheduler=dict(type='MultiStepLR', milestones=[400000], gamma=0.5),
                          pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean'), perceptual_opt=vgg,
                          gan_opt=dict(type='GANLoss', gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0,
                                       loss_weight=0.1), net_d_iters=1, net_d_init_iters=0))
    model = build_model(opt)
    it = [0]

    def step():
        it[0] += 1
        model.optimize_parameters(it[0])

    model.feed_data(data)
    res = timed([lambda: model.feed_data(data), step], args.calls, args.warmup)
    report('RealESRGANModel feed_data and step (bf16 autocast)', ('feed_data', 'step'), res, batch=B)
    print(json.dumps(dict(case='share', feed_data_share_of_iteration=round(res[0][0] / (res[0][0] + res[1][0]), 4),
                          stock_feed_share_if_used=round(feed['stock_ms_median'] / (feed['stock_ms_median'] + res[1][0]), 4))))


if __name__ == '__main__':
    main()
