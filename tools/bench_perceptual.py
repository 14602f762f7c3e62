"""One-launch times of the perceptual-loss kernels (csrc/perceptual.hip): max-pool forward / backward
(stride 2), Gram forward and Gram backward (with the residual), at NHWC [8,256,256,64] (conv1_2 of a 256^2
batch) and [8,16,16,512] (conv5_4 of it), bf16 and fp32.

Per kernel, shape and dtype: the algorithmic FLOPs and HBM bytes (the figures the ops hand to ktrace), the
mean device-event time of --reps back-to-back launches after --warmup, and the share of the roof
max(FLOPs / peak, bytes / 8 TB/s), peak = 2.5 PFLOP/s (bf16 MFMA, the bf16 Gram forward) or 157.3 TFLOP/s
(f32 MFMA: the fp32 Gram forward and the Gram backward of both dtypes); the max-pool is bandwidth only.
One JSON line per case.  For per-kernel times run it under ``rocprofv3 --kernel-trace --stats`` (the Gram
forward at [8,256,256,64] is two kernels, gram_fwd_kernel and gram_reduce_kernel, there).

    python tools/bench_perceptual.py [--reps 50] [--warmup 10] [--shape 8 16 16 512]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basicsr4rs_amd.ops import perceptual as P  # noqa: E402
from basicsr4rs_amd.utils import ktrace  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
PEAK_BF16, PEAK_F32 = 2.5e15, 157.3e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def counted(fn):
    """(name, flops, bytes) of one call, as the op reports them to ktrace."""
    ktrace.start()
    fn()
    rec = ktrace.stop()
    (name, d), = rec.items()
    return name, d['flops'], d['bytes']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--shape', type=int, nargs=4, default=None, help='N H W C: this shape only')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_perceptual.py needs the GPU')
    g = torch.Generator().manual_seed(0)
    for shape in ([tuple(args.shape)] if args.shape else [(8, 256, 256, 64), (8, 16, 16, 512)]):
        for dtype in (torch.bfloat16, torch.float32):
            N, H, W, C = shape
            x = torch.randn(shape, generator=g).to(dtype).cuda()
            res = torch.randn(shape, generator=g).to(dtype).cuda()
            dy = torch.randn(N, H // 2, W // 2, C, generator=g).to(dtype).cuda()
            dG = torch.randn(N, C, C, generator=g).cuda()
            scale = P.gram_scale(x)
            cases = [('maxpool2_fwd', lambda: P.maxpool2_fwd_raw(x, 2), None),
                     ('maxpool2_bwd', lambda: P.maxpool2_bwd_raw(x, dy, 2), None),
                     ('gram_fwd', lambda: P.gram_fwd_raw(x, scale), PEAK_BF16 if dtype == torch.bfloat16 else PEAK_F32),
                     ('gram_bwd', lambda: P.gram_bwd_raw(x, dG, scale, res=res, beta=1.0), PEAK_F32)]
            for label, fn, peak in cases:
                name, flops, nbytes = counted(fn)
                ms = timed(fn, args.reps, args.warmup)
                t_mem, t_fl = nbytes / HBM_BYTES_PER_S, (flops / peak if peak else 0.0)
                roof = max(t_mem, t_fl)
                print(json.dumps(dict(kernel=name, case=label, shape=list(shape), dtype=str(dtype).split('.')[-1],
                                      flops=flops, bytes=nbytes, us=round(ms * 1e3, 2), reps=args.reps,
                                      roof_us=round(roof * 1e6, 2), bound='bytes' if t_mem >= t_fl else 'flops',
                                      roof_share=round(roof / (ms * 1e-3), 3),
                                      tbytes_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3),
                                      tflops=round(flops / (ms * 1e-3) / 1e12, 2))), flush=True)
            del x, res, dy, dG
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
