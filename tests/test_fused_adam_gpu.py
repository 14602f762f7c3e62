"""Fused Adam + EMA on the GPU (sr_adam_ema_dev, sr_adam_ema, utils/flat.py FusedAdam) against the
float64 single-step reference and the derived bounds of tests/test_fused_adam_host.py (derivation in
that module's docstring), and the FusedAdam plumbing against torch.optim.Adam in float64.

Multi-step bound of the plumbing test: per step the update is good to tau_t + the 1.3e-5 of the
Python-double betas the float64 Adam uses, below 1e-4 together, and the stored parameter rounds once
per step: |p - p_ref| <= 1e-4 sum_k |D_ref,k| + t u max_k |p_ref,k|.  The EMA averages the parameter
errors (weights summing to less than 1) and rounds three times per step on values up to |ema| + |p|:
|ema - ema_ref| <= that bound + 3 t u max_k (|ema_ref,k| + |p_ref,k|).
"""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests.test_fused_adam_host import (BETAS, DECAY, EPS, GRID, LR, SWEEP, U, _id, bias_corrections, check, hyper,
                                        make_inputs)

pytestmark = pytest.mark.gpu

BIG = 2 * SWEEP + 257


def _lib():
    from basicsr4rs_amd import _lib
    return _lib


def _step_dev(cuda, inp, hp, with_ema):
    """One sr_adam_ema_dev launch on raw tensors; returns the new state as numpy arrays."""
    L = _lib()
    d = {k: torch.from_numpy(a).to(cuda) for k, a in inp.items()}
    g0 = d['g'].clone()
    hy = torch.tensor([hp['t'] - 1, hp['lr'], hp['gscale']], dtype=torch.float32, device=cuda)
    hy0 = hy.clone()
    L.check(L.load().sr_adam_ema_dev(L.ptr(d['p']), L.ptr(d['g']), L.ptr(d['m']), L.ptr(d['v']),
                                     L.ptr(d['ema'] if with_ema else None), d['p'].numel(), L.ptr(hy), hp['b1'],
                                     hp['b2'], hp['eps'], hp['decay'], L.stream()))
    torch.cuda.synchronize()
    assert hy[0].item() == hp['t'] and torch.equal(hy[1:3], hy0[1:3])
    assert torch.equal(d['g'], g0)
    return {k: d[k].cpu().numpy() for k in ('p', 'm', 'v', 'ema')}


def _step_host_scalars(cuda, inp, hp, with_ema):
    L = _lib()
    d = {k: torch.from_numpy(a).to(cuda) for k, a in inp.items()}
    bc1, bc2 = bias_corrections(hp)
    L.check(L.load().sr_adam_ema(L.ptr(d['p']), L.ptr(d['g']), L.ptr(d['m']), L.ptr(d['v']),
                                 L.ptr(d['ema'] if with_ema else None), d['p'].numel(), hp['lr'], hp['b1'], hp['b2'],
                                 hp['eps'], bc1, bc2, hp['decay'], hp['gscale'], L.stream()))
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in ('p', 'm', 'v', 'ema')}


@pytest.mark.parametrize('case', GRID, ids=_id)
def test_adam_ema_dev_single_step(cuda, case):
    t, betas, gs, with_ema = case
    inp, hp = make_inputs(1000, t), hyper(t, betas, gs)
    check(_step_dev(cuda, inp, hp, with_ema), inp, hp, f'adam_ema_dev n=1000 {_id(case)}', with_ema)


@pytest.mark.parametrize('with_ema', [True, False], ids=['ema', 'noema'])
@pytest.mark.parametrize('n', [1, 255, 257, 1000, BIG])
def test_adam_ema_dev_sizes(cuda, n, with_ema):
    """Block and grid-sweep tails; the size past two sweeps (8192 blocks x 256 threads) is checked whole."""
    inp, hp = make_inputs(n, 10), hyper(10, BETAS[0], 1.0 / 3.0)
    check(_step_dev(cuda, inp, hp, with_ema), inp, hp, f'adam_ema_dev n={n}', with_ema)


@pytest.mark.parametrize('t', [1, 1000])
@pytest.mark.parametrize('n', [257, BIG])
def test_adam_ema_host_scalar_form(cuda, n, t):
    inp, hp = make_inputs(n, t, seed=1), hyper(t, BETAS[1] if t == 1 else BETAS[0], 0.125)
    check(_step_host_scalars(cuda, inp, hp, True), inp, hp, f'adam_ema n={n} t={t}')
    if n == 257:
        check(_step_host_scalars(cuda, inp, hp, False), inp, hp, f'adam_ema n={n} t={t} no ema', False)


class _Tiny(nn.Module):

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.a = nn.Parameter(torch.randn(7, generator=g))
        self.b = nn.Parameter(torch.randn(3, 100, generator=g))


def _grads(k):
    """The fixed gradient of step k (1-based) for the 307 flat elements: independent of the parameters,
    magnitudes over five decades, a few exact zeros."""
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randn(307, generator=g) * 10.0**(-5.0 * torch.rand(307, generator=g))
    x[::19] = 0.0
    return x


def _fused(cuda, state=None):
    from basicsr4rs_amd.utils.flat import FlatParams, FusedAdam
    net, net_ema = _Tiny().to(cuda), _Tiny().to(cuda)
    flat, flat_ema = FlatParams(net), FlatParams(net_ema, with_grad=False)
    if state is not None:
        flat.flat.copy_(state['p'])
        flat_ema.flat.copy_(state['ema'])
    opt = FusedAdam(flat, lr=LR, betas=BETAS[0], eps=EPS)
    opt.grad_scale = 0.5
    if state is not None:
        opt.load_state_dict(state['opt'])
    return flat, flat_ema, opt


def _lr_of(k):
    return LR if k < 4 else 0.25 * LR


def _run_fused(cuda, flat, flat_ema, opt, steps, snap_at=None):
    out, snap = {}, None
    for k in steps:
        opt.param_groups[0]['lr'] = _lr_of(k)
        flat.grad.copy_(_grads(k))
        opt.step(ema=flat_ema, ema_decay=DECAY)
        sd = opt.state_dict()
        assert all(float(sd['state'][i]['step']) == k for i in range(2)), (k, sd['state'][0]['step'])
        out[k] = tuple(x.detach().cpu().clone() for x in (flat.flat, flat_ema.flat, opt.m, opt.v))
        if k == snap_at:
            snap = dict(p=flat.flat.clone(), ema=flat_ema.flat.clone(), opt=copy.deepcopy(sd))
    return out, snap


def test_fused_adam_plumbing_matches_float64_adam(cuda):
    flat, flat_ema, opt = _fused(cuda)
    assert flat.numels == [7, 300]
    p0 = flat.flat.detach().cpu().double()
    ref = [p0[:7].clone().requires_grad_(True), p0[7:].view(3, 100).clone().requires_grad_(True)]
    ema_ref = flat_ema.flat.detach().cpu().double().clone()
    assert torch.equal(ema_ref, p0)
    ropt = torch.optim.Adam(ref, lr=LR, betas=BETAS[0], eps=EPS)
    run, snap = _run_fused(cuda, flat, flat_ema, opt, range(1, 11), snap_at=5)
    moved = torch.zeros(307, dtype=torch.float64)
    pmax, emax = torch.zeros(307, dtype=torch.float64), torch.zeros(307, dtype=torch.float64)
    for k in range(1, 11):
        ropt.param_groups[0]['lr'] = _lr_of(k)
        g = _grads(k).double() * 0.5
        ref[0].grad, ref[1].grad = g[:7].clone(), g[7:].view(3, 100).clone()
        before = torch.cat([r.detach().reshape(-1) for r in ref]).clone()
        ropt.step()
        p_ref = torch.cat([r.detach().reshape(-1) for r in ref])
        ema_ref = DECAY * ema_ref + (1.0 - DECAY) * p_ref
        moved += (p_ref - before).abs()
        pmax = torch.maximum(pmax, p_ref.abs())
        emax = torch.maximum(emax, ema_ref.abs() + p_ref.abs())
        bp = 1e-4 * moved + k * U * pmax
        be = bp + 3 * k * U * emax
        ep = (run[k][0].double() - p_ref).abs()
        ee = (run[k][1].double() - ema_ref).abs()
        print(f'FusedAdam step {k}: p max|err| {ep.max().item():.3e} (err/bound {(ep / bp).max().item():.3f}), '
              f'ema max|err| {ee.max().item():.3e} (err/bound {(ee / be).max().item():.3f})')
        assert (ep <= bp).all(), (k, ep.max().item())
        assert (ee <= be).all(), (k, ee.max().item())
    # resume at step 5 in a fresh optimizer: steps 6-10 bitwise the uninterrupted run
    flat2, flat_ema2, opt2 = _fused(cuda, snap)
    assert opt2.nstep == 5
    run2, _ = _run_fused(cuda, flat2, flat_ema2, opt2, range(6, 11))
    for k in range(6, 11):
        for a, b, name in zip(run[k], run2[k], ('p', 'ema', 'm', 'v')):
            assert torch.equal(a, b), (k, name)
