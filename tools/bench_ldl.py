"""LDL term timing: the fused HIP path (ldl_l1_term of losses/loss_util.py: sr_ldl_map_fwd / sr_ldl_map_bwd) against
the same term written with torch ops on the device -- the artifact map by an unfold of the reflect-padded residual
(49 window values per pixel) followed by L1Loss(w * out, w * gt), what the reference's step runs.

Forward + backward to the output's gradient at the shape of options/train/LDL/train_LDL_Real_x4.yml (fp32
[4,3,256,256]); per round the median of --calls device-event timings after --warmup calls, fused and torch
alternating call by call (tools/bench_loss.py's scheme).  One JSON line per round:

    python tools/bench_ldl.py [--rounds 3] [--calls 40] [--warmup 10] [--shape 4 3 256 256] [--bf16]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_loss import timed_pair  # noqa: E402

from basicsr4rs_amd.losses.loss_util import _torch_artifact_map, ldl_l1_term  # noqa: E402


def torch_term(out, gt, ema):
    w = _torch_artifact_map(gt, out, ema, 7)
    return (w * out - w * gt).abs().mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--shape', type=int, nargs=4, default=[4, 3, 256, 256])
    ap.add_argument('--bf16', action='store_true', help='the output and the EMA output in bf16 (train.use_amp)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ldl.py needs the GPU')
    g = torch.Generator().manual_seed(0)
    dt = torch.bfloat16 if args.bf16 else torch.float32
    gt = torch.rand(*args.shape, generator=g).cuda()
    out = (gt + 0.05 * torch.randn(*args.shape, generator=g).cuda()).to(dt).requires_grad_(True)
    ema = (gt + 0.05 * torch.randn(*args.shape, generator=g).cuda()).to(dt)
    for rnd in range(-1, args.rounds):  # round -1: untimed (code objects, clocks, allocator)
        pair = timed_pair(lambda: ldl_l1_term(out, gt, ema, 1.0, 'mean'), lambda: torch_term(out, gt, ema), out,
                          args.warmup if rnd < 0 else args.calls, 0 if rnd < 0 else args.warmup)
        if rnd < 0:
            continue
        (f_med, f_min, f_loss, f_grad), (t_med, t_min, t_loss, t_grad) = pair
        print(json.dumps(dict(round=rnd, term='ldl_l1', dtype=str(dt), shape=args.shape, calls=args.calls,
                              fused_ms_median=round(f_med, 4), fused_ms_min=round(f_min, 4),
                              torch_ms_median=round(t_med, 4), torch_ms_min=round(t_min, 4), speedup=round(t_med / f_med, 2),
                              loss_rel_diff=abs(f_loss.item() - t_loss.item()) / max(abs(t_loss.item()), 1e-30),
                              grad_max_abs_diff=(f_grad.float() - t_grad.float()).abs().max().item())), flush=True)


if __name__ == '__main__':
    main()
