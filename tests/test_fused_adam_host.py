"""Float64 reference and derived error bounds of the fused Adam + EMA kernels (csrc/eltwise.hip:
adam_ema_kernel, adam_ema_dev_kernel), and a host-only proof that the bounds separate the kernel's
arithmetic from three wrong formulas.  tests/test_fused_adam_gpu.py imports reference and bounds.

Reference, one step from arbitrary state, float64 on the fp32 inputs with the fp32-rounded scalars the
kernel receives (lr, beta1, beta2, eps, decay, gscale; 1.f - 0.999f != 0.001, which moves the update by
about 1.3e-5 relative, so Python-double betas would not do):

    g' = g gscale                       m' = m + (1 - b1)(g' - m)        v' = b2 v + (1 - b2) g'^2
    den = sqrt(v') / sqrt(1 - b2^t) + eps                                D  = lr / (1 - b1^t) m' / den
    p' = p - D                          ema' = decay ema + (1 - decay) p'

Bounds, u = 2^-24 (one fp32 rounding is at most u relative), first order in u; every count is the
worst case without fused multiply-adds, contraction only removes roundings.  1 - b1, 1 - b2 and
1 - decay are exact in fp32 (Sterbenz: 1/2 <= b <= 2).

  gi = fl(g gscale) = g'(1 + d1).
  m:  fl(gi - m) is off by u|g'| (d1) + u(|g'| + |m|) (its rounding); times (1 - b1) and one product
      rounding: <= 3u (1 - b1)(|g'| + |m|); the final sum rounds once more, u|m'| <= u(|m| + |g'|).
          |m - m'| <= CM u (|m| + |g'|),  CM = 4    (1 + 3(1 - b1) <= 4 for any b1 >= 0)
  v:  fl(v b2): u.  fl(fl((1 - b2) gi) gi): d1 twice and two product roundings, 4u.  The sum: u.  Both
      addends are >= 0, so the relative errors do not amplify: 5u v', and 6 with the second-order terms.
      The products of tiny gradients can underflow; fp32 underflow (gradual or flushed) costs at most
      the smallest normal number TINY = 2^-126 in absolute terms.
          |v - v'| <= CV u v' + TINY,  CV = 6
  D:  relative, all factors positive except m (taken separately below):
        bc1 = fl(1 - powf(b1, t)): powf is good to 1 ulp = 2u b1^t absolute, the subtraction rounds by u:
              2u b1^t / (1 - b1^t) + u.  This is the cancellation term: at t = 1, b1 = 0.9 it is 18u.
        step_size = fl(lr / bc1): u.
        bc2s = sqrtf(bc2): half of (2u b2^t / (1 - b2^t) + u), plus u for the root.
        sqrtf(vi): half of v's 6u, plus u.   / bc2s: u.   + eps: u (both addends >= 0).
        mi / denom: u.   step_size * (.): u.
      Constant part: 1 + 1 + 1.5 + 4 + 1 + 1 + 1 + 1 = 11.5u; K = 16 leaves room for the second-order
      terms and for sqrt(TINY) = 1e-19 against eps = 1e-8.
          tau_t = K u + 2u / (1 - b1^t) + u / (1 - b2^t)      (>= the cancellation terms above)
      tau_t stays below 1e-4 at every tested t: its maximum is at t = 1, b2 = 0.999: 6.2e-5.
      The error of m enters D as (lr / bc1) |m - m'| / den.
          |p - p'| <= u |p'| + tau_t |D| + (lr / bc1) CM u (|m| + |g'|) / den
      where u |p'| is the rounding of the final subtraction.  A quarter of the test's p are exactly 0:
      there p' = -D and the update itself is checked to tau_t.
  ema: two products and a sum, each <= u of a value <= |ema| + |p'|, and the error of p scaled:
          |ema - ema'| <= 3u (|ema| + |p'|) + (1 - decay) |p - p'|

The three wrong formulas (no bias correction; (sqrt(v) + eps) / sqrt(bc2); t off by one) differ from the
kernel by more than 1e-2 in D somewhere for t <= 10, and by 3e-4 at t = 1000 with b2 = 0.999, against
tau_t <= 6.2e-5; at t = 100000 both corrections are 1 in fp32 and in float64 alike and the formulas
coincide, so the mutants are asserted to fail at t <= 10 and at (1000, b2 = 0.999) only.
"""
import numpy as np
import pytest

U = 2.0**-24
TINY = 2.0**-126
CM, CV, K = 4, 6, 16
LR, EPS, DECAY = 1e-3, 1e-8, 0.999
TS = (1, 2, 3, 10, 1000, 100000)
BETAS = ((0.9, 0.999), (0.9, 0.99))
GSCALES = (1.0, 0.125, 1.0 / 3.0)
SWEEP = 8192 * 256  # elements one sweep of the kernel's grid covers


def f32(x):
    return np.float32(x)


def make_inputs(n, t, seed=0):
    """Seeded fp32 state: p ~ N(0,1) with a quarter exactly 0; g = N(0,1) 10^U(-9,0) with exact zeros, so
    sqrt(v) crosses eps = 1e-8; m, v zero at t = 1, else of the same spread (v >= m^2); ema near p."""
    rng = np.random.default_rng(1000 * seed + 7 * t + n % 1009)

    def spread():
        return rng.standard_normal(n) * 10.0**rng.uniform(-9.0, 0.0, n)

    p = rng.standard_normal(n)
    p[rng.random(n) < 0.25] = 0.0
    g = spread()
    g[3::7] = 0.0
    if t == 1:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = 0.5 * spread()
        v = spread()**2 + m**2  # |m| <= sqrt(v), as in a real run: the update stays of the order of lr
    ema = p + 0.01 * rng.standard_normal(n)
    return {k: a.astype(np.float32) for k, a in dict(p=p, g=g, m=m, v=v, ema=ema).items()}


def hyper(t, betas=(0.9, 0.999), gscale=1.0, lr=LR, eps=EPS, decay=DECAY):
    return dict(t=int(t), lr=lr, b1=betas[0], b2=betas[1], eps=eps, decay=decay, gscale=gscale)


def bias_corrections(hp):
    """1 - beta^t in double from the fp32-rounded betas (what sr_adam_ema is handed as floats)."""
    return 1.0 - float(f32(hp['b1']))**hp['t'], 1.0 - float(f32(hp['b2']))**hp['t']


def reference(inp, hp, with_ema=True):
    """float64 single step; returns the new state and the quantities the bounds need."""
    p, g, m, v, ema = (inp[k].astype(np.float64) for k in ('p', 'g', 'm', 'v', 'ema'))
    lr, b1, b2, eps, decay, gs = (float(f32(hp[k])) for k in ('lr', 'b1', 'b2', 'eps', 'decay', 'gscale'))
    bc1, bc2 = bias_corrections(hp)
    g1 = g * gs
    m1 = m + (1.0 - b1) * (g1 - m)
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    den = np.sqrt(v1) / np.sqrt(bc2) + eps
    delta = lr / bc1 * m1 / den
    p1 = p - delta
    e1 = decay * ema + (1.0 - decay) * p1 if with_ema else ema
    tau = K * U + 2 * U / bc1 + U / bc2
    em = CM * U * (np.abs(m) + np.abs(g1))
    bp = U * np.abs(p1) + tau * np.abs(delta) + lr / bc1 * em / den
    bounds = dict(m=em, v=CV * U * v1 + TINY, p=bp,
                  ema=3 * U * (np.abs(ema) + np.abs(p1)) + (1.0 - decay) * bp if with_ema else np.zeros_like(p))
    return dict(p=p1, m=m1, v=v1, ema=e1, delta=delta, tau=tau, bounds=bounds, mterm=lr / bc1 * em / den)


def violations(got, inp, hp, with_ema=True):
    """{name: (largest |err| / bound, largest |err|, index)} of a result against the reference."""
    ref = reference(inp, hp, with_ema)
    assert ref['tau'] < 1e-4, ref['tau']
    out = {}
    for k in ('m', 'v', 'p', 'ema'):
        err = np.abs(got[k].astype(np.float64) - ref[k])
        assert np.isfinite(err).all(), k
        bound = ref['bounds'][k]
        ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
        i = int(np.argmax(ratio))
        out[k] = (float(ratio[i]), float(err.max()), i)
    # the update itself, relative to D, where p == 0 and m' has not cancelled (its error term below tau_t |D|)
    z = (inp['p'] == 0) & (ref['delta'] != 0) & (ref['mterm'] <= ref['tau'] * np.abs(ref['delta']))
    if z.any():
        rel = np.abs(got['p'].astype(np.float64)[z] - ref['p'][z]) / np.abs(ref['delta'][z])
        out['update_rel'] = float(rel.max())
    out['tau'] = ref['tau']
    return out


def check(got, inp, hp, what, with_ema=True):
    """Assert the four bounds; prints each largest error next to its bound (ratio 1 = at the bound)."""
    vio = violations(got, inp, hp, with_ema)
    print(f"{what}: err/bound m {vio['m'][0]:.3f} v {vio['v'][0]:.3f} p {vio['p'][0]:.3f} ema {vio['ema'][0]:.3f}; "
          f"max|err| m {vio['m'][1]:.3e} v {vio['v'][1]:.3e} p {vio['p'][1]:.3e} ema {vio['ema'][1]:.3e}; "
          f"update rel err at p=0, m' not cancelled {vio.get('update_rel', 0.0):.3e} (tau_t {vio['tau']:.3e})")
    for k in ('m', 'v', 'p', 'ema'):
        assert vio[k][0] <= 1.0, (what, k, vio[k])
    if not with_ema:
        assert np.array_equal(got['ema'].view(np.uint32), inp['ema'].view(np.uint32)), what
    return vio


def emulate(inp, hp, with_ema=True, variant='kernel'):
    """The kernel's statement order in numpy float32 (no fused multiply-add; powf correctly rounded).
    ``variant``: 'kernel', or one of the wrong formulas 'no_bias_correction', 'eps_inside', 'off_by_one'."""
    one = f32(1.0)
    lr, b1, b2, eps, decay, gs = (f32(hp[k]) for k in ('lr', 'b1', 'b2', 'eps', 'decay', 'gscale'))
    t = hp['t'] + (1 if variant == 'off_by_one' else 0)
    bc1 = one - f32(float(b1)**t)
    bc2 = one - f32(float(b2)**t)
    if variant == 'no_bias_correction':
        bc1 = bc2 = one
    step_size = f32(lr / bc1)
    bc2s = np.sqrt(bc2)
    p, g, m, v, ema = (inp[k] for k in ('p', 'g', 'm', 'v', 'ema'))
    gi = g * gs
    mi = m + (one - b1) * (gi - m)
    vi = v * b2 + (one - b2) * gi * gi
    if variant == 'eps_inside':
        denom = (np.sqrt(vi) + eps) / bc2s
    else:
        denom = np.sqrt(vi) / bc2s + eps
    pi = p - step_size * (mi / denom)
    out = dict(p=pi, m=mi, v=vi, ema=ema * decay + pi * (one - decay) if with_ema else ema.copy())
    assert all(a.dtype == np.float32 for a in out.values())
    return out


GRID = [(t, b, gs, e) for t in TS for b in BETAS for gs in GSCALES for e in (True, False)]
N_HOST = 4096


def _id(case):
    t, b, gs, e = case
    return f't{t}-b{b[1]}-gs{gs:.3f}-{"ema" if e else "noema"}'


@pytest.mark.parametrize('case', GRID, ids=_id)
def test_emulated_kernel_arithmetic_meets_bounds(case):
    t, betas, gs, with_ema = case
    inp, hp = make_inputs(N_HOST, t), hyper(t, betas, gs)
    assert (inp['p'] == 0).sum() > N_HOST // 8 and (inp['g'] == 0).any()
    check(emulate(inp, hp, with_ema), inp, hp, f'emulation {_id(case)}', with_ema)


@pytest.mark.parametrize('variant', ['no_bias_correction', 'eps_inside', 'off_by_one'])
@pytest.mark.parametrize('case', [c for c in GRID if c[0] <= 10 or (c[0] == 1000 and c[1][1] == 0.999)], ids=_id)
def test_wrong_formulas_violate_bounds(case, variant):
    t, betas, gs, with_ema = case
    inp, hp = make_inputs(N_HOST, t), hyper(t, betas, gs)
    vio = violations(emulate(inp, hp, with_ema, variant), inp, hp, with_ema)
    print(f"{variant} {_id(case)}: p err/bound {vio['p'][0]:.3e}, update rel err {vio['update_rel']:.3e}")
    assert vio['p'][0] > 1.0, (variant, vio)
    if with_ema:
        assert vio['ema'][0] > 1.0, (variant, vio)


def test_tau_condition():
    for t in TS:
        for betas in BETAS:
            hp = hyper(t, betas)
            assert reference(make_inputs(8, t), hp)['tau'] < 1e-4
    assert SWEEP == 2097152
