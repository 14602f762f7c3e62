"""Records tests/golden/ecbsr.npz from the reference's ECBSR on the CPU (fp32, one thread).

Run: python -m tests.golden.make_ecbsr_golden <path to the reference's basicsr/archs/ecbsr_arch.py>

Only that one file is loaded (importlib, with a stub ``basicsr.utils.registry`` so that the rest of the package and
its dependencies are not imported).  Per case ``<c>.`` (A: Y x4, B: RGB x2, C: all border; CASES below): ``names``
(state_dict keys in order), ``sd.<key>`` (the seeded state_dict), ``x``, ``g`` (the upstream gradient), ``out_train``,
``out_eval``, ``rep.<l>.weight / .bias`` (each block's rep_params()) and ``grad.<key>`` (every parameter gradient of
the train-mode form under ``g``).  In the seeded state every edge branch's ``scale`` and ``bias`` are multiplied by 300
(at the default 1e-3 init the edge branches would be invisible) and each ``act.weight`` is linspace(-0.3, 0.4) with
element 1 set to 0 (negative, zero and positive slopes).  ``m4c16.names / .shapes / .nparams``: the net of
train_ECBSR_x4_m4c16_prelu.yml."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

CASES = {
    'A': (dict(num_in_ch=1, num_out_ch=1, num_block=2, num_channel=16, with_idt=False, act_type='prelu', scale=4),
          (2, 1, 7, 9)),
    'B': (dict(num_in_ch=3, num_out_ch=3, num_block=1, num_channel=16, with_idt=True, act_type='prelu', scale=2),
          (1, 3, 5, 6)),
    'C': (dict(num_in_ch=1, num_out_ch=1, num_block=1, num_channel=8, with_idt=True, act_type='relu', scale=3),
          (1, 1, 1, 1)),
}
M4C16 = dict(num_in_ch=1, num_out_ch=1, num_block=4, num_channel=16, with_idt=False, act_type='prelu', scale=4)


def load_reference(path):
    class _Registry:

        def register(self):
            return lambda cls: cls

    pkg, utils, registry = types.ModuleType('basicsr'), types.ModuleType('basicsr.utils'), types.ModuleType(
        'basicsr.utils.registry')
    registry.ARCH_REGISTRY = _Registry()
    sys.modules.update({'basicsr': pkg, 'basicsr.utils': utils, 'basicsr.utils.registry': registry})
    spec = importlib.util.spec_from_file_location('reference_ecbsr_arch', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def seed_state(net):
    """The adjustments of the seeded state (see the module docstring), in place."""
    with torch.no_grad():
        for name, p in net.named_parameters():
            leaf = name.rsplit('.', 1)[-1]
            if '.conv1x1_s' in name or '.conv1x1_lpl' in name:
                if leaf in ('scale', 'bias'):
                    p.mul_(300.0)
            if name.endswith('act.weight'):
                p.copy_(torch.linspace(-0.3, 0.4, p.numel()))
                p[1] = 0.0


def main(path):
    torch.set_num_threads(1)
    ref = load_reference(path)
    out = {}
    for ci, (name, (cfg, shape)) in enumerate(CASES.items()):
        torch.manual_seed(10 + ci)
        net = ref.ECBSR(**cfg)
        seed_state(net)
        g = torch.Generator().manual_seed(20 + ci)
        x = torch.rand(*shape, generator=g)
        s = cfg['scale']
        up = torch.randn(shape[0], cfg['num_out_ch'], shape[2] * s, shape[3] * s, generator=g)
        sd = net.state_dict()
        out[f'{name}.names'] = np.array(list(sd.keys()))
        for k, v in sd.items():
            out[f'{name}.sd.{k}'] = v.detach().clone().numpy()
        out[f'{name}.x'], out[f'{name}.g'] = x.numpy(), up.numpy()
        net.train()
        y = net(x)
        (y * up).sum().backward()
        out[f'{name}.out_train'] = y.detach().numpy()
        for k, p in net.named_parameters():
            if p.requires_grad:
                out[f'{name}.grad.{k}'] = p.grad.detach().clone().numpy()
        net.eval()
        with torch.no_grad():
            out[f'{name}.out_eval'] = net(x).numpy()
            for l, blk in enumerate(net.backbone):
                w, b = blk.rep_params()
                out[f'{name}.rep.{l}.weight'], out[f'{name}.rep.{l}.bias'] = w.numpy(), b.numpy()
    torch.manual_seed(0)
    net = ref.ECBSR(**M4C16)
    sd = net.state_dict()
    out['m4c16.names'] = np.array(list(sd.keys()))
    out['m4c16.shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    out['m4c16.nparams'] = np.array(sum(p.numel() for p in net.parameters()), dtype=np.int64)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ecbsr.npz')
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1])
