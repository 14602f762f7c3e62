"""Time of the metric stage of one validation image (val.device_metrics): the 14 PSNR / SSIM
entries of the L2S option file on one 1 x 6 x 288 x 288 pair, through SRRSModel._compute_metrics (host:
numpy on the ubyte images, which are converted outside the clock) and through
SRRSModel._compute_metrics_device (one sr_val_metrics launch on the device tensors, one small copy back;
the device is synchronised before the clock stops).  Median of --repeats after --warmup, alternating the
two paths; the ubyte conversion the host path needs first is timed on its own.  One JSON line.

``--niqe`` adds the NIQE entries an L2S-style config asks for (calculate_niqe_band per band and
calculate_rs_niqe on bands [2, 1, 0]; parameter file: --niqe-params) to the metric set: the device path then
also launches sr_niqe_moments, and the line gains ``niqe_max_rel_diff``."""
import argparse
import json
import os
import statistics
import sys
import time

import pandas as pd
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L2S_YAML = os.path.join(ROOT, 'tests', 'golden', 'reference_options', 'train', 'SwinIR',
                        'train_SwinIR_L2S288_scratch.yml')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, default=288)
    ap.add_argument('--niqe', action='store_true')
    ap.add_argument('--niqe-params', default=os.path.join(ROOT, 'tests', 'golden', 'niqe_pris_params.npz'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('val_metrics_time: no HIP device (a CPU run measures nothing)')
    import basicsr4rs_amd.archs  # noqa: F401
    from basicsr4rs_amd.models import build_model
    from basicsr4rs_amd.utils.img_util import minusone_one_tensor_to_ubyte_numpy
    with open(L2S_YAML) as f:
        metrics = {k: v for k, v in yaml.safe_load(f)['val']['metrics'].items() if v['type'] != 'calculate_lpips_band'}
    if args.niqe:
        for b in range(6):
            metrics[f'niqe_b{b}'] = dict(type='calculate_niqe_band', crop_border=4, band=b, params_path=args.niqe_params)
        metrics['niqe_rgb'] = dict(type='calculate_rs_niqe', crop_border=4, input_bands=[2, 1, 0],
                                   params_path=args.niqe_params)
    opt = dict(model_type='L2SSingleModel', name='t', is_train=False, dist=False, num_gpu=1, scale=3, path={},
               network_g=dict(type='SRCNN', num_in_ch=6, num_out_ch=6, upscale=3), val=dict(metrics=metrics))
    model = build_model(opt)
    model.metric_results = {k: 0.0 for k in metrics}
    g = torch.Generator().manual_seed(0)
    s = args.size
    # a smooth scene plus sensor-like noise; sr = gt + a small error, as late in training
    base = torch.nn.functional.interpolate(torch.rand(1, 6, s // 8, s // 8, generator=g) * 1.6 - 0.8, size=(s, s),
                                           mode='bilinear')
    gt = base + 0.02 * torch.randn(1, 6, s, s, generator=g)
    sr = gt + 0.03 * torch.randn(1, 6, s, s, generator=g)
    srd, gtd = sr.cuda(), gt.cuda()
    host_t, dev_t, conv_t = [], [], []
    tables = {}
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        a, b = minusone_one_tensor_to_ubyte_numpy(srd.float().cpu()), minusone_one_tensor_to_ubyte_numpy(gtd.float().cpu())
        t1 = time.perf_counter()
        detailed = pd.DataFrame()
        model._compute_metrics('img', a, b, detailed)
        t2 = time.perf_counter()
        tables['host'] = detailed
        torch.cuda.synchronize()
        detailed = pd.DataFrame()
        t3 = time.perf_counter()
        model._compute_metrics_device('img', srd, gtd, detailed)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        tables['device'] = detailed
        if i >= args.warmup:
            conv_t.append(t1 - t0), host_t.append(t2 - t1), dev_t.append(t4 - t3)
    h, d = tables['host'].loc['img'], tables['device'].loc['img']
    psnr_equal = all(h[k] == d[k] for k in metrics if 'psnr' in k)
    ssim_diff = max(abs(h[k] - d[k]) for k in metrics if 'ssim' in k)

    def ms(v):
        v = sorted(v)
        return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * v[0], 3),
                    max_ms=round(1e3 * v[-1], 3))

    out = dict(shape=[1, 6, s, s], entries=len(metrics), repeats=args.repeats, warmup=args.warmup,
               host_compute_metrics=ms(host_t), device_compute_metrics=ms(dev_t),
               host_ubyte_conversion=ms(conv_t), psnr_equal=psnr_equal, ssim_max_abs_diff=ssim_diff,
               psnr=float(h['psnr']), ssim=float(h['ssim']))
    if args.niqe:
        out['niqe_max_rel_diff'] = max(abs(h[k] - d[k]) / abs(h[k]) for k in metrics if k.startswith('niqe'))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
