"""The conv3x3 host dispatch answers its pointer-free queries exactly as the build pinned in
tests/golden/conv_dispatch.json did (no GPU): the forward kernel name, launch count, colsum partial rows and
dot-partials query, the weight-gradient kernel name and its workspace size (which fixes the split count of
every plan), for every recorded bench-workload and test descriptor in both dtypes, under every accepted
variant and each A/B knob setting.  The test sets the variant and every knob the selection reads itself, so
SR_* variables of the caller's environment do not reach it."""
import json
import os
import re

from basicsr4rs_amd import _lib
from tests.golden import make_conv_dispatch as G


def test_dispatch_matches_pinned_build():
    fx = json.load(open(G.FIXTURE))
    assert [tuple(s) for s in fx['settings']] == list(G.SETTINGS)
    assert fx['fwd_fields'] == [n for n, _ in _lib.ConvDesc._fields_]
    assert fx['wgrad_fields'] == [n for n, _ in _lib.WgradDesc._fields_]
    assert len(fx['fwd']) >= 150 and len(fx['wgrad']) >= 75
    ans = G.query_all(_lib.load(), [r[0] for r in fx['fwd']], [r[0] for r in fx['wgrad']])
    bad = []
    for kind in ('fwd', 'wgrad'):
        for row, got in zip(fx[kind], ans[kind]):
            for dt, (base, diff), got_dt in zip(G.DTYPES, row[1:], got):
                for i, g in enumerate(got_dt):
                    want = diff.get(str(i), base)
                    want = [fx['names'][want[0]]] + want[1:]
                    if g != want:
                        bad.append((kind, dt, dict(zip(fx[kind + '_fields'], row[0])), fx['settings'][i], want, g))
    assert not bad, f'{len(bad)} queries differ from commit {fx["commit"][:7]}; first: {bad[:3]}'


def test_every_variant_is_pinned_and_named():
    """The fixture covers exactly the variants the library accepts, and _lib names each of them."""
    lib = _lib.load()
    prev = lib.sr_conv3x3_get_variant()
    try:
        accepted = [v for v in range(0, 128) if lib.sr_conv3x3_set_variant(v) == 0]
    finally:
        _lib.check(lib.sr_conv3x3_set_variant(prev))
    assert tuple(accepted) == G.VARIANTS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sr_hip.h')).read()
    named = {n: int(v) for n, v in re.findall(r'X\((SR_VARIANT_[A-Z0-9_]+), (\d+)\)', header)}
    assert sorted(named.values()) == accepted
    assert _lib.VARIANTS == named
