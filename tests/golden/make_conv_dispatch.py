"""Regenerate tests/golden/conv_dispatch.json: the kernel selection and split plans of the conv3x3 host
dispatch, recorded through its pointer-free queries (no GPU needed).

    SR_HIP_LIB=<libsr_hip.so of the commit to pin> python -m tests.golden.make_conv_dispatch \
        --commit <its hash> [--descs recorded.json ...]

The fixture pins a build that is known good (the parent of a dispatch refactor), never the code under
test; tests/test_conv_dispatch.py asserts that the current library answers every query the same.

Descriptors: --descs files hold {"fwd": [[ConvDesc fields...]], "wgrad": [[WgradDesc fields...]]} as recorded by
tests/golden/record_conv_descs.py (on the GPU) from the bench workloads (EDSR, RCAN, SwinIR-M, RRDBNet train
steps: forward, dgrad and wgrad calls) and the conv tests, pointers as 0 / 1; without --descs the descriptors of
the existing fixture are reused.  Each is queried in both dtypes, under every accepted variant and under each
knob setting below.

Row format: [descriptor fields (dtype left 0), answers as fp32, answers as bf16]; answers are [base, diff] with
base the answer of the automatic selection and diff {setting index: answer} for the settings that answer
differently; an answer is the query results in the order of "fwd_answers" / "wgrad_answers", the kernel name
as an index into "names".
"""
import argparse
import ctypes
import json
import os

from basicsr4rs_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_dispatch.json')

VARIANTS = tuple(sorted(_lib.VARIANTS.values()))  # enum sr_conv_variant (include/sr_hip.h)
KNOB_SETTINGS = (('SR_LWK', 0), ('SR_LWK_MINK', 192), ('SR_RING_WIDE', 0), ('SR_RING_WIDE', 256), ('SR_RING_PS', 0),
                 ('SR_LWG', 0), ('SR_WG_ROW3', 0))
# settings[0] is the automatic selection: variant 0, every knob at its built-in default
SETTINGS = tuple(('variant', v) for v in VARIANTS) + tuple(('knob',) + k for k in KNOB_SETTINGS)
# every knob the conv selection and its split plans read; all held at -1 (built-in default) unless a setting says so
KNOBS = ('SR_LWK', 'SR_LWK_MINK', 'SR_RING_WIDE', 'SR_RING_PS', 'SR_LWG', 'SR_LWG_T', 'SR_RING_SPLITS', 'SR_WG_ROW3',
         'SR_PPH_GRID')
DTYPES = (_lib.SR_F32, _lib.SR_BF16)

_DUMMY = ctypes.create_string_buffer(64)  # stands for a row_scale / dot operand: only its presence is looked at


def _struct(cls, vals, dtype):
    d = cls()
    for (name, ty), v in zip(cls._fields_, vals):
        setattr(d, name, (ctypes.addressof(_DUMMY) if v else None) if ty is _lib._vp else v)
    d.dtype = dtype
    return d


def _fwd(lib, d):
    return [lib.sr_conv3x3_fwd_kernel_name(d).decode(), lib.sr_conv3x3_fwd_launches(d),
            lib.sr_conv3x3_fwd_colsum_parts(d), lib.sr_conv3x3_fwd_dot_ok(d)]


def _wgrad(lib, d):
    return [lib.sr_conv3x3_wgrad_kernel_name(d).decode(), lib.sr_conv3x3_wgrad_workspace(d)]


def query_all(lib, fwd_descs, wgrad_descs):
    """answers[kind][descriptor index][dtype index][setting index], kernel names as strings; the knobs and the
    variant are put back afterwards."""
    prev_variant = lib.sr_conv3x3_get_variant()
    prev_knobs = {k: lib.sr_get_knob(k.encode()) for k in KNOBS}
    fs = [[_struct(_lib.ConvDesc, v, dt) for dt in DTYPES] for v in fwd_descs]
    ws = [[_struct(_lib.WgradDesc, v, dt) for dt in DTYPES] for v in wgrad_descs]
    out = {'fwd': [[[] for _ in DTYPES] for _ in fs], 'wgrad': [[[] for _ in DTYPES] for _ in ws]}
    try:
        for k in KNOBS:
            _lib.check(lib.sr_set_knob(k.encode(), -1, None))
        for s in SETTINGS:
            if s[0] == 'variant':
                _lib.check(lib.sr_conv3x3_set_variant(s[1]))
            else:
                _lib.check(lib.sr_conv3x3_set_variant(0))
                _lib.check(lib.sr_set_knob(s[1].encode(), s[2], None))
            for kind, structs, fn in (('fwd', fs, _fwd), ('wgrad', ws, _wgrad)):
                for i, pair in enumerate(structs):
                    for j, d in enumerate(pair):
                        out[kind][i][j].append(fn(lib, d))
            if s[0] == 'knob':
                _lib.check(lib.sr_set_knob(s[1].encode(), -1, None))
    finally:
        _lib.check(lib.sr_conv3x3_set_variant(prev_variant))
        for k, v in prev_knobs.items():
            _lib.check(lib.sr_set_knob(k.encode(), v, None))
    return out


def _unique(rows, fields, zero):
    """The descriptors without the fields in `zero` (the dtype, which every row is crossed with, and what is no
    part of a selection), floats in their shortest form that reads back as the same float32, deduplicated."""
    def short(v):
        s = float('%.7g' % v)
        return s if ctypes.c_float(s).value == ctypes.c_float(v).value else float('%.9g' % v)

    seen = set()
    for r in rows:
        r = [short(v) if isinstance(v, float) else v for v in r]
        for z in zero:
            r[fields.index(z)] = 0
        seen.add(tuple(r))
    return sorted(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit SR_HIP_LIB was built from')
    ap.add_argument('--descs', nargs='*', default=[])
    args = ap.parse_args()
    ffields = [n for n, _ in _lib.ConvDesc._fields_]
    wfields = [n for n, _ in _lib.WgradDesc._fields_]
    fwd, wg = [], []
    if args.descs:
        for p in args.descs:
            rec = json.load(open(p))
            assert rec['fwd_fields'] == ffields and rec['wgrad_fields'] == wfields, p
            fwd += rec['fwd']
            wg += rec['wgrad']
    else:
        old = json.load(open(FIXTURE))
        fwd, wg = [r[0] for r in old['fwd']], [r[0] for r in old['wgrad']]
    fwd = _unique(fwd, ffields, ('dtype',))
    wg = _unique(wg, wfields, ('dtype', 'accumulate'))
    ans = query_all(_lib.load(), fwd, wg)
    names = sorted({a[0] for kind in ans.values() for row in kind for per_dt in row for a in per_dt})

    def rows(descs, answers):
        out = []
        for d, per_dt in zip(descs, answers):
            row = [list(d)]
            for a in per_dt:
                a = [[names.index(x[0])] + x[1:] for x in a]
                row.append([a[0], {str(i): x for i, x in enumerate(a) if i and x != a[0]}])
            out.append(row)
        return out

    fixture = {'commit': args.commit, 'settings': [list(s) for s in SETTINGS], 'names': names, 'fwd_fields': ffields,
               'fwd_answers': ['kernel_name', 'launches', 'colsum_parts', 'dot_ok'], 'wgrad_fields': wfields,
               'wgrad_answers': ['kernel_name', 'workspace'], 'fwd': rows(fwd, ans['fwd']),
               'wgrad': rows(wg, ans['wgrad'])}
    with open(FIXTURE, 'w') as fh:
        fh.write('{\n')
        for k, v in fixture.items():
            if k in ('fwd', 'wgrad'):
                fh.write(f' "{k}": [\n' + ',\n'.join('  ' + json.dumps(r, separators=(',', ':')) for r in v) + '\n ]')
            else:
                fh.write(f' "{k}": {json.dumps(v)}')
            fh.write(',\n' if k != 'wgrad' else '\n')
        fh.write('}\n')
    print(f'{FIXTURE}: {len(fwd)} fwd + {len(wg)} wgrad descriptors x {len(DTYPES)} dtypes x {len(SETTINGS)} settings, '
          f'{os.path.getsize(FIXTURE)} bytes')


if __name__ == '__main__':
    main()
