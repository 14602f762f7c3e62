"""EDVR timing: the kernels of csrc/edvr.hip at EDVR-M's shapes and one full EDVR-M train step.

Kernels (B * T = 20 frames of 64 features; TSA maps at batch 4):
  conv3s2 forward (bias + LeakyReLU), dgrad and wgrad at 64 x 64 and 32 x 32 inputs, 64 -> 64 channels, each beside
  the stride-1 ``conv3x3`` forward on the same input (4 x the MACs: what a stride-2 conv would otherwise cost);
  pool3s2 forward / backward at 64 x 64 and 32 x 32; tsa_corr forward / backward at 5 frames of 64 x 64;
  tsa_modulate forward / backward at 64 x 64.
A kernel is timed by device events around ``--inner`` back-to-back launches, the median and minimum over ``--calls``
such groups after ``--warmup``; with the time come the algorithmic FLOPs and bytes of the call (computed here from the
shapes) as TFLOP/s and GB/s.  These kernels run 4 to 40 us and a launch through the Python wrapper costs about 10 us
on the host, so for the short ones the event time is the launch rate, an upper bound of the kernel time: read the
kernel time itself from a profiler run of the kernel cases, one input size per run (``--hw``).

Step: ``EDVRModel`` with the ``network_g`` of options/train/EDVR/train_EDVR_M_x4_SR_REDS.yml (64 features, 5 frames,
5 + 10 blocks, TSA), batch 4, 64^2 -> 256^2, CharbonnierLoss, Adam + EMA, ``use_amp`` (bf16), every parameter
trainable; median and minimum of ``--calls`` device-event timings after ``--warmup`` steps.  For the per-kernel table
run the step alone under the profiler and read its kernel_stats.csv with tools/kstats.py or tools/kstat_table.py:

    python tools/bench_edvr.py [--calls 20] [--warmup 5] [--inner 20] [--hw 64 32] [--fp32] [--no-step | --step-only]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_edvr.py --step-only --calls 10
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_edvr.py --no-step --hw 64 --calls 5 --inner 10

One JSON line per case.  Times only: correctness is the tests' business.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basicsr4rs_amd import _lib  # noqa: E402
from basicsr4rs_amd.models import build_model  # noqa: E402
from basicsr4rs_amd.ops import conv as C  # noqa: E402
from basicsr4rs_amd.ops import edvr as E  # noqa: E402

NET_M = dict(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=5, deformable_groups=8, num_extract_block=5,
             num_reconstruct_block=10, center_frame_idx=None, hr_in=False, with_predeblur=False, with_tsa=True)


def timed(fn, calls, warmup, inner=1):
    ms = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms)


def report(case, shape, dtype, flops, nbytes, t):
    med, mn = t
    print(json.dumps(dict(case=case, shape=shape, dtype='bf16' if dtype == torch.bfloat16 else 'fp32',
                          ms=round(med, 4), min_ms=round(mn, 4), gflop=round(flops / 1e9, 3),
                          mbytes=round(nbytes / 1e6, 3),
                          tflops=round(flops / med / 1e9, 2), gbs=round(nbytes / med / 1e6, 1))), flush=True)


def bench_kernels(dtype, args):
    g = torch.Generator().manual_seed(0)
    esz = 2 if dtype == torch.bfloat16 else 4
    t = lambda fn: timed(fn, args.calls, args.warmup, args.inner)  # noqa: E731

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dtype).cuda()

    N, Cc = 20, 64
    for H in args.hw:
        Ho = E.out_size(H)
        conv = torch.nn.Conv2d(Cc, Cc, 3, 2, 1).cuda()
        conv1 = torch.nn.Conv2d(Cc, Cc, 3, 1, 1).cuda()
        x, dy = rnd(N, H, H, Cc), rnd(N, Ho, Ho, Cc)
        wf, wd = E.conv3s2_images(conv.weight, dtype)
        bias = conv.bias.detach()
        shape = [N, H, H, Cc, Cc]
        m_out, m_in, wbytes = N * Ho * Ho, N * H * H, 9 * Cc * Cc * esz
        report('conv3s2 fwd', shape, dtype, 2.0 * m_out * 9 * Cc * Cc, esz * Cc * (m_in + m_out) + wbytes,
               t(lambda: E.conv3s2_fwd_raw(x, wf, bias, Cc, _lib.ACT_LRELU, 0.1)))
        report('conv3s2 dgrad', shape, dtype, 2.0 * m_out * 9 * Cc * Cc, esz * Cc * (m_in + m_out) + wbytes,
               t(lambda: E.conv3s2_dgrad_raw(dy, wd, H, H, Cc)))
        report('conv3s2 wgrad', shape, dtype, 2.0 * m_out * 9 * Cc * Cc, esz * Cc * (m_in + m_out) + 4 * 9 * Cc * Cc,
               t(lambda: E.conv3s2_wgrad_raw(dy, x, Cc, Cc)))
        with torch.no_grad():
            report('conv3x3 stride 1 fwd (same input)', shape, dtype, 2.0 * m_in * 9 * Cc * Cc,
                   esz * Cc * 2 * m_in + wbytes, t(lambda: C.conv3x3(x, conv1, act=_lib.ACT_LRELU, slope=0.1)))
    B, T = 4, 5
    for H in args.hw:
        Ho = E.out_size(H)
        x, dy = rnd(B, H, H, Cc), rnd(B, Ho, Ho, 2 * Cc)
        report('pool3s2 fwd', [B, H, H, Cc], dtype, 18.0 * B * Ho * Ho * Cc, esz * (x.numel() + dy.numel()),
               t(lambda: E.pool3s2_fwd_raw(x)))
        report('pool3s2 bwd', [B, H, H, Cc], dtype, 18.0 * B * Ho * Ho * Cc, esz * (2 * x.numel() + dy.numel()),
               t(lambda: E.pool3s2_bwd_raw(x, dy)))
    if 64 not in args.hw:
        return
    H = 64
    emb, ali, ref, d_out = rnd(B * T, H, H, Cc), rnd(B * T, H, H, Cc), rnd(B, H, H, Cc), rnd(B, H, H, T * Cc)
    _, prob = E.tsa_corr_fwd_raw(emb, ref, ali)
    n = emb.numel()
    report('tsa_corr fwd', [B, T, H, H, Cc], dtype, 3.0 * n, esz * (3 * n + ref.numel()) + 4 * prob.numel(),
           t(lambda: E.tsa_corr_fwd_raw(emb, ref, ali)))
    report('tsa_corr bwd', [B, T, H, H, Cc], dtype, 7.0 * n, esz * (5 * n + 2 * ref.numel()) + 4 * prob.numel(),
           t(lambda: E.tsa_corr_bwd_raw(d_out, emb, ref, ali, prob)))
    feat, attn, add = rnd(B, H, H, Cc), rnd(B, H, H, Cc), rnd(B, H, H, Cc)
    n = feat.numel()
    report('tsa_modulate fwd', [B, H, H, Cc], dtype, 6.0 * n, esz * 4 * n,
           t(lambda: E.tsa_modulate_fwd_raw(feat, attn, add)))
    report('tsa_modulate bwd', [B, H, H, Cc], dtype, 8.0 * n, esz * 5 * n,
           t(lambda: E.tsa_modulate_bwd_raw(add, feat, attn)))


def bench_step(amp, args):
    opt = dict(model_type='EDVRModel', is_train=True, dist=False, num_gpu=1, scale=4, path={}, network_g=dict(NET_M),
               train=dict(ema_decay=0.999, use_amp=amp,
                          optim_g=dict(type='Adam', lr=4e-4, weight_decay=0, betas=[0.9, 0.99]),
                          scheduler=dict(type='CosineAnnealingRestartLR', periods=[600000], restart_weights=[1],
                                         eta_min=1e-7),
                          pixel_opt=dict(type='CharbonnierLoss', loss_weight=1.0, reduction='sum'), dcn_lr_mul=1))
    torch.manual_seed(0)
    model = build_model(opt)
    g = torch.Generator().manual_seed(1)
    model.feed_data({'lq': torch.rand(args.batch, 5, 3, 64, 64, generator=g),
                     'gt': torch.rand(args.batch, 3, 256, 256, generator=g)})
    it = [0]

    def step():
        it[0] += 1
        model.optimize_parameters(it[0])

    med, mn = timed(step, args.calls, args.warmup)
    print(json.dumps(dict(case='EDVR-M train step (5 frames, 5 + 10 blocks, TSA)', batch=args.batch, lq=[64, 64],
                          dtype='bf16' if amp else 'fp32', step_ms=round(med, 3), step_min_ms=round(mn, 3),
                          l_pix=round(float(model.get_current_log()['l_pix']), 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20, help='back-to-back launches per timed group of a kernel')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--hw', type=int, nargs='+', default=[64, 32],
                    help='input sizes of the kernel cases (a profiler run of one size keeps the two apart)')
    ap.add_argument('--fp32', action='store_true', help='fp32 instead of bf16')
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_edvr.py needs the GPU')
    if not args.step_only:
        bench_kernels(torch.float32 if args.fp32 else torch.bfloat16, args)
    if not args.no_step:
        bench_step(not args.fp32, args)


if __name__ == '__main__':
    main()
