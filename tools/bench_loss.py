"""Pixel-loss timing: the fused HIP path (sr_pixel_loss through losses/basic_loss.py) against the same
loss written with torch ops on the device -- the reference's formula (basicsr/losses/basic_loss.py:12-24,
loss_util.py:26-55), which is also what a weighted L1Loss ran on before the kernel family existed.

Forward + backward to the prediction's gradient at the EDSR bench output shape (fp32 [32,3,256,256], weight
[32,1,256,256] where used); per case and round the median of --calls device-event timings after --warmup
calls, fused and torch alternating call by call.  One JSON line per round and case:

    python tools/bench_loss.py [--rounds 3] [--calls 40] [--warmup 10] [--shape 32 3 256 256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basicsr4rs_amd.losses import build_loss  # noqa: E402


def torch_loss(kind, pred, target, weight, eps=1e-12):
    d = pred - target
    loss = d.abs() if kind == 'L1Loss' else (d**2 if kind == 'MSELoss' else torch.sqrt(d**2 + eps))
    if weight is None:
        return loss.mean()
    loss = loss * weight
    return loss.sum() / (weight.sum() if weight.size(1) > 1 else weight.sum() * loss.size(1))


def one_call(fn, pred):
    """Device-event ms of fn() + backward, the loss and the gradient."""
    pred.grad = None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn()
    loss.backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), loss.detach(), pred.grad


def timed_pair(fused, stock, pred, calls, warmup):
    """The two paths call by call in turn, so a change of the machine's state meets both alike:
    (median, min, loss, gradient) of each over the last `calls` pairs."""
    ms = ([], [])
    for i in range(warmup + calls):
        for k, fn in enumerate((fused, stock)):
            t, loss, grad = one_call(fn, pred)
            if i >= warmup:
                ms[k].append(t)
            if i == warmup + calls - 1:
                ms[k].append((loss, grad))
    out = []
    for m in ms:
        loss, grad = m.pop()
        out.append((statistics.median(m), min(m), loss, grad))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--shape', type=int, nargs=4, default=[32, 3, 256, 256])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_loss.py needs the GPU')
    N, C, H, W = args.shape
    g = torch.Generator().manual_seed(0)
    pred = torch.rand(N, C, H, W, generator=g).cuda().requires_grad_(True)
    target = torch.rand(N, C, H, W, generator=g).cuda()
    w1 = torch.rand(N, 1, H, W, generator=g)
    w1[torch.rand(N, 1, H, W, generator=g) < 0.3] = 0
    w1 = w1.cuda()
    cases = [('L1Loss', True), ('MSELoss', False), ('MSELoss', True), ('CharbonnierLoss', False),
             ('CharbonnierLoss', True)]
    for rnd in range(-1, args.rounds):  # round -1: every case once untimed (code objects, clocks, allocator)
        for kind, weighted in cases:
            w = w1 if weighted else None
            mod = build_loss(dict(type=kind, loss_weight=1.0, reduction='mean'))
            pair = timed_pair(lambda: mod(pred, target, w), lambda: torch_loss(kind, pred, target, w), pred,
                              args.warmup if rnd < 0 else args.calls, 0 if rnd < 0 else args.warmup)
            if rnd < 0:
                continue
            (f_med, f_min, f_loss, f_grad), (t_med, t_min, t_loss, t_grad) = pair
            print(json.dumps(dict(round=rnd, loss=kind, weight='n1hw' if weighted else 'none', shape=args.shape,
                                  calls=args.calls, fused_ms_median=round(f_med, 4), fused_ms_min=round(f_min, 4),
                                  torch_ms_median=round(t_med, 4), torch_ms_min=round(t_min, 4),
                                  speedup=round(t_med / f_med, 2),
                                  loss_rel_diff=abs(f_loss.item() - t_loss.item()) / max(abs(t_loss.item()), 1e-30),
                                  grad_max_abs_diff=(f_grad - t_grad).abs().max().item())), flush=True)


if __name__ == '__main__':
    main()
