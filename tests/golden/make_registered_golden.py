"""Records tests/golden/registered_loss.npz from the reference's align losses on the CPU (fp32, one thread).

Run: python -m tests.golden.make_registered_golden <path to the reference's basicsr/losses/align_loss.py>

Only that one file is loaded (importlib, with a stub ``basicsr.utils.registry`` so that the rest of the package and
its dependencies are not imported).  Per case ``<name>.``: taps [S, K] (the K_x buffer), pred, target, and for
``l1`` / ``mse``: table [B, S^2], argmin [B], loss_mean, loss_sum, loss_none [B], and grad_mean / grad_none
(pred.grad; for 'none' under an upstream of ones).  The target of image b is shift ``picks[b]`` of pred plus noise,
so the minimum is a shift other than the identity.  ``enc.``: EncoderLoss (z, gt, lq; the loss of both strategies,
z.grad of 'lq')."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

# name: (start, end, step), shape
CASES = {
    'unit': ((-1.0, 1.0, 1.0), (1, 1, 9, 9)),
    'half': ((-1.0, 1.0, 0.5), (2, 3, 15, 18)),
    'asym': ((0.0, 1.5, 0.5), (1, 2, 14, 17)),
}


def load_reference(path):
    class _Registry:

        def register(self):
            return lambda cls: cls

    pkg, utils, registry = types.ModuleType('basicsr'), types.ModuleType('basicsr.utils'), types.ModuleType(
        'basicsr.utils.registry')
    registry.LOSS_REGISTRY = _Registry()
    sys.modules.update({'basicsr': pkg, 'basicsr.utils': utils, 'basicsr.utils.registry': registry})
    spec = importlib.util.spec_from_file_location('reference_align_loss', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(path):
    torch.set_num_threads(1)
    ref = load_reference(path)
    out = {}
    for ci, (name, (grid, shape)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(100 + ci)
        pred = torch.rand(*shape, generator=g) * 2 - 1
        shifter = ref.ShiftConv2d(*grid)
        S = shifter.K_x.shape[0]
        picks = [1, S * S - 2][:shape[0]]
        with torch.no_grad():
            stack = shifter(pred)
        target = torch.stack([stack[b, picks[b]] for b in range(shape[0])]) + 0.05 * torch.randn(*shape, generator=g)
        out[f'{name}.taps'] = shifter.K_x.reshape(S, -1).numpy()
        out[f'{name}.pred'], out[f'{name}.target'] = pred.numpy(), target.numpy()
        out[f'{name}.picks'] = np.array(picks, dtype=np.int64)
        for kind in ('l1', 'mse'):
            with torch.no_grad():
                table = ref.RegisteredLoss(*grid, kind)._shifted_loss(pred, target)
            out[f'{name}.{kind}.table'], out[f'{name}.{kind}.argmin'] = table.numpy(), table.argmin(1).numpy()
            for red in ('mean', 'sum', 'none'):
                p = pred.clone().requires_grad_(True)
                loss = ref.RegisteredLoss(*grid, kind, loss_weight=1.0, reduction=red)(p, target)
                loss.sum().backward()
                out[f'{name}.{kind}.loss_{red}'] = loss.detach().numpy()
                if red != 'sum':  # the 'sum' gradient is B times the 'mean' one: left out to keep the file small
                    out[f'{name}.{kind}.grad_{red}'] = p.grad.numpy()
    g = torch.Generator().manual_seed(7)
    lq = torch.rand(2, 6, 5, 7, generator=g) * 2 - 1
    z = (torch.rand(2, 6, 15, 21, generator=g) * 2 - 1).requires_grad_(True)
    gt = torch.rand(2, 6, 15, 21, generator=g) * 2 - 1
    for strategy in ('gt', 'lq'):
        loss = ref.EncoderLoss(loss_weight=1.0, strategy=strategy, reduction='mean')(z, gt, lq)
        out[f'enc.{strategy}.loss'] = loss.detach().numpy()
        if strategy == 'lq':
            loss.backward()
            out['enc.lq.grad'] = z.grad.numpy().copy()
    out['enc.lq'], out['enc.z'], out['enc.gt'] = lq.numpy(), z.detach().numpy(), gt.numpy()
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'registered_loss.npz')
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1])
