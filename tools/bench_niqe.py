"""NIQE timing per validation image: the host metric functions (metrics/niqe.py on the ubyte image, which is
converted outside the clock) against the device path (ops/metrics.py:niqe_scores_from_device: sr_niqe_moments
launches, one copy back, niqe_from_moments on the host), for one NIQE entry per band as an L2S-style config
asks for them.

Two shapes: a 6-band 288 x 288 and a 4-band 512 x 512 image in [-1, 1].  Per shape: the median and minimum
of --calls wall-clock timings of each path after --warmup calls, host and device alternating call by call
(the device path is synchronised by its copy back), and the device-event time of the kernels alone
(sr_niqe_moments for all bands, no copy, no host part).  One JSON line per shape:

    python tools/bench_niqe.py [--calls 10] [--warmup 2] [--params tests/golden/niqe_pris_params.npz]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from basicsr4rs_amd.metrics import calculate_metric  # noqa: E402
from basicsr4rs_amd.metrics import niqe as Q  # noqa: E402
from basicsr4rs_amd.ops import metrics as M  # noqa: E402
from basicsr4rs_amd.utils.img_util import minusone_one_tensor_to_ubyte_numpy  # noqa: E402


def scene(C, s, g):
    """A smooth scene plus sensor-like noise, as tools/val_metrics_time.py makes it."""
    base = torch.nn.functional.interpolate(torch.rand(1, C, s // 8, s // 8, generator=g) * 1.6 - 0.8, size=(s, s),
                                           mode='bilinear')
    return base + 0.05 * torch.randn(1, C, s, s, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--params', default=os.path.join(ROOT, 'tests', 'golden', 'niqe_pris_params.npz'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_niqe.py needs the GPU')
    window = Q.load_niqe_params(args.params)[2]
    g = torch.Generator().manual_seed(0)
    for C, s in ((6, 288), (4, 512)):
        x = scene(C, s, g)
        xd = x.cuda()
        opt = {f'niqe_b{b}': dict(type='calculate_niqe_band', crop_border=4, band=b, params_path=args.params)
               for b in range(C)}
        host_t, dev_t, kern_t = [], [], []
        for i in range(args.warmup + args.calls):
            img = minusone_one_tensor_to_ubyte_numpy(xd.float().cpu())
            t0 = time.perf_counter()
            host = {k: calculate_metric(dict(img=img, img2=img), o) for k, o in opt.items()}
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            dev = M.niqe_scores_from_device(opt, xd)
            t3 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            M.niqe_moments_device(xd, [(0, (c,)) for c in range(C)], 4, window)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                host_t.append(t1 - t0), dev_t.append(t3 - t2), kern_t.append(a.elapsed_time(b) * 1e-3)

        def ms(v):
            return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3))

        rel = max(abs(dev[k] - host[k]) / abs(host[k]) for k in opt)
        print(json.dumps(dict(shape=[1, C, s, s], entries=C, crop_border=4, calls=args.calls, warmup=args.warmup,
                              host_per_image=ms(host_t), device_per_image=ms(dev_t), device_kernels_only=ms(kern_t),
                              speedup=round(statistics.median(host_t) / statistics.median(dev_t), 2),
                              score_max_rel_diff=rel, scores_host=[round(host[k], 4) for k in opt])), flush=True)


if __name__ == '__main__':
    main()
