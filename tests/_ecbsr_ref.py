"""ECBSR restated with torch functionals, driven by a state_dict, in any dtype: the five-branch training forward of
basicsr/archs/ecbsr_arch.py and the collapse formulas of its ``rep_params``.  tests/test_ecbsr_host.py pins both to
the recorded reference results (tests/golden/ecbsr.npz), so the GPU tests can use them in float64.

``stored`` wraps the maps the engine keeps in the feature dtype: every hidden layer's pre-activation ``z`` and
output ``y`` (and, through the wrapper's backward, their gradients) and the input map."""
import torch
from torch.nn import functional as F

EDGES = ('conv1x1_sbx', 'conv1x1_sby', 'conv1x1_lpl')


def num_layers(sd):
    return 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('backbone.'))


def _bias_pad(y, b):
    """Zero-pad by one pixel, then overwrite the border with the branch's own bias."""
    y = F.pad(y, (1, 1, 1, 1))
    inner = torch.zeros_like(y[:1, :1])
    inner[..., 1:-1, 1:-1] = 1.0
    return y * inner + b.view(1, -1, 1, 1) * (1.0 - inner)


def ecb_branches(sd, pre, x, with_idt):
    """Sum of the five branches of block ``pre`` (e.g. 'backbone.0.') on x, before the activation."""
    y = F.conv2d(x, sd[pre + 'conv3x3.weight'], sd[pre + 'conv3x3.bias'], padding=1)
    p = pre + 'conv1x1_3x3.'
    t = _bias_pad(F.conv2d(x, sd[p + 'k0'], sd[p + 'b0']), sd[p + 'b0'])
    y = y + F.conv2d(t, sd[p + 'k1'], sd[p + 'b1'])
    for e in EDGES:
        p = pre + e + '.'
        t = _bias_pad(F.conv2d(x, sd[p + 'k0'], sd[p + 'b0']), sd[p + 'b0'])
        y = y + F.conv2d(t, sd[p + 'scale'] * sd[p + 'mask'], sd[p + 'bias'], groups=t.shape[1])
    if with_idt and x.shape[1] == y.shape[1]:
        y = y + x
    return y


def collapse(sd, pre, with_idt):
    """(RK [Cout, Cin, 3, 3], RB [Cout]) of block ``pre`` by the collapse formulas."""
    w3 = sd[pre + 'conv3x3.weight']
    cout, cin = w3.shape[:2]
    p = pre + 'conv1x1_3x3.'
    k0, b0, k1, b1 = sd[p + 'k0'][:, :, 0, 0], sd[p + 'b0'], sd[p + 'k1'], sd[p + 'b1']
    rk = w3 + torch.einsum('omhw,mi->oihw', k1, k0)
    rb = sd[pre + 'conv3x3.bias'] + torch.einsum('omhw,m->o', k1, b0) + b1
    for e in EDGES:
        p = pre + e + '.'
        k0, b0, m = sd[p + 'k0'][:, :, 0, 0], sd[p + 'b0'], sd[p + 'mask'][:, 0]
        sc = sd[p + 'scale'].reshape(-1)
        rk = rk + (sc.view(-1, 1, 1) * m)[:, None] * k0[:, :, None, None]
        rb = rb + sc * m.sum((1, 2)) * b0 + sd[p + 'bias']
    if with_idt and cin == cout:
        idt = torch.zeros_like(rk)
        idt[torch.arange(cout), torch.arange(cout), 1, 1] = 1.0
        rk = rk + idt
    return rk, rb


def forward(sd, x, scale, with_idt, act_type='prelu', collapsed=False, stored=lambda t: t):
    """ECBSR's forward: five-branch (training) form, or every block through its collapsed conv."""
    L = num_layers(sd)
    h = stored(x)
    for l in range(L):
        pre = f'backbone.{l}.'
        if collapsed:
            rk, rb = collapse(sd, pre, with_idt)
            z = F.conv2d(h, rk, rb, padding=1)
        else:
            z = ecb_branches(sd, pre, h, with_idt)
        if l == L - 1:
            h = z
        elif act_type == 'prelu':
            # z is stored for the gate and the slope gradient (its value rounded; its gradient is the dz map,
            # rounded through y's wrapper)
            zr = z + (stored(z.detach()) - z.detach())
            h = stored(F.prelu(zr, sd[pre + 'act.weight']))
        elif act_type == 'relu':
            h = stored(F.relu(z))
        else:
            h = stored(z)
    s2 = scale * scale
    short = torch.repeat_interleave(x, s2, dim=1) if x.shape[1] > 1 else x
    return F.pixel_shuffle(h + short, scale)
