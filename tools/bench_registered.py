"""RegisteredLoss timing and peak memory: the fused HIP path (sr_registered_loss through losses/align_loss.py) against
the torch-op composition of the same module (its fallback: the [B, S^2, C, H, W] stack of shifted images by two
convolutions, the loss map, argmin and autograd through all of it -- what the reference runs).

Forward + backward to the prediction's gradient at the L2S training shape (bf16 [12,6,192,192] predictions, fp32
targets, shifts (-2, 2, 0.5), l1); per round the median of --calls device-event timings after --warmup calls, fused
and torch alternating call by call (tools/bench_loss.py's scheme), and per path the peak of
torch.cuda.max_memory_allocated over one call above what was allocated before it.  One JSON line per round:

    python tools/bench_registered.py [--rounds 3] [--calls 20] [--warmup 5] [--shape 12 6 192 192] [--fp32]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_loss import one_call, timed_pair  # noqa: E402

from basicsr4rs_amd.losses.align_loss import RegisteredLoss, _torch_registered  # noqa: E402


def peak_bytes(fn, pred):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    one_call(fn, pred)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=4, default=[12, 6, 192, 192])
    ap.add_argument('--grid', type=float, nargs=3, default=[-2.0, 2.0, 0.5])
    ap.add_argument('--loss-func', default='l1')
    ap.add_argument('--fp32', action='store_true', help='fp32 predictions (default bf16, train.use_amp)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_registered.py needs the GPU')
    g = torch.Generator().manual_seed(0)
    dt = torch.float32 if args.fp32 else torch.bfloat16
    mod = RegisteredLoss(*args.grid, args.loss_func).cuda()
    target = (torch.rand(*args.shape, generator=g) * 2 - 1).cuda()
    pred = (torch.roll(target, shifts=(1, -1), dims=(2, 3)) + 0.05 * torch.randn(*args.shape, generator=g).cuda()).to(dt)
    pred.requires_grad_(True)
    l1 = args.loss_func.lower() == 'l1'

    def fused():
        return mod(pred, target)

    def stock():
        return _torch_registered(mod._shiftconv2d, pred.float(), target, l1, 'mean', 1.0)[0]

    S, K = mod._shiftconv2d.taps.shape
    for rnd in range(-1, args.rounds):  # round -1: untimed (code objects, clocks, allocator, convolution choice)
        pair = timed_pair(fused, stock, pred, args.warmup if rnd < 0 else args.calls, 0 if rnd < 0 else args.warmup)
        if rnd < 0:
            continue
        (f_med, f_min, f_loss, f_grad), (t_med, t_min, t_loss, t_grad) = pair
        f_peak, t_peak = peak_bytes(fused, pred), peak_bytes(stock, pred)
        print(json.dumps(dict(round=rnd, loss=args.loss_func, dtype=str(dt), shape=args.shape, grid=args.grid, S=S, K=K,
                              calls=args.calls, fused_ms_median=round(f_med, 4), fused_ms_min=round(f_min, 4),
                              torch_ms_median=round(t_med, 4), torch_ms_min=round(t_min, 4), speedup=round(t_med / f_med, 2),
                              fused_peak_mb=round(f_peak / 2**20, 2), torch_peak_mb=round(t_peak / 2**20, 2),
                              loss_rel_diff=abs(f_loss.item() - t_loss.item()) / max(abs(t_loss.item()), 1e-30),
                              grad_max_abs_diff=(f_grad.float() - t_grad.float()).abs().max().item())), flush=True)


if __name__ == '__main__':
    main()
