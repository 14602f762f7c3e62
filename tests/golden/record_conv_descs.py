"""Record the conv / linear descriptors a run passes to libsr_hip (needs the GPU): the --descs input of
tests/golden/make_conv_dispatch.py.  Every sr_conv3x3_* call and query that takes a descriptor is wrapped; the
pointer-free fields are kept (pointers as 0 / 1), deduplicated.

    python -m tests.golden.record_conv_descs <edsr|rcan|swinir|rrdb> out.json    one bench train step of the workload
    REC_OUT=out.json python -m pytest -p tests.golden.record_conv_descs tests/test_conv_gpu.py tests/test_abi.py

The committed fixture was made from the four workloads and these two test files.
"""
import json
import os
import sys

from basicsr4rs_amd import _lib

SEEN = {'fwd': set(), 'wgrad': set()}
FWD_CALLS = ('sr_conv3x3_fwd', 'sr_linear_ln_fwd', 'sr_conv3x3_fwd_dot_ok', 'sr_conv3x3_fwd_colsum_parts',
             'sr_conv3x3_fwd_kernel_name', 'sr_conv3x3_fwd_launches')
WGRAD_CALLS = ('sr_conv3x3_wgrad', 'sr_conv3x3_wgrad_reduce', 'sr_conv3x3_wgrad_workspace',
               'sr_conv3x3_wgrad_kernel_name')


def _fields(d, cls):
    d = d._obj if hasattr(d, '_obj') else (d.contents if hasattr(d, 'contents') else d)
    vals = []
    for name, ty in cls._fields_:
        v = getattr(d, name)
        vals.append((1 if v else 0) if ty is _lib._vp else float(v) if ty is _lib._f else v)
    return tuple(vals)


def install():
    lib = _lib.load()
    for names, kind, cls in ((FWD_CALLS, 'fwd', _lib.ConvDesc), (WGRAD_CALLS, 'wgrad', _lib.WgradDesc)):
        for name in names:
            def wrapped(d, *a, _orig=getattr(lib, name), _kind=kind, _cls=cls):
                if d is not None:
                    SEEN[_kind].add(_fields(d, _cls))
                return _orig(d, *a)
            setattr(lib, name, wrapped)


def dump(out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump({'fwd_fields': [n for n, _ in _lib.ConvDesc._fields_], 'fwd': sorted(SEEN['fwd']),
                   'wgrad_fields': [n for n, _ in _lib.WgradDesc._fields_], 'wgrad': sorted(SEEN['wgrad'])}, fh)
    print(f'{out}: {len(SEEN["fwd"])} fwd + {len(SEEN["wgrad"])} wgrad descriptors')


def pytest_sessionstart(session):
    install()


def pytest_sessionfinish(session, exitstatus):
    dump(os.environ.get('REC_OUT', 'conv_descs_tests.json'))


if __name__ == '__main__':
    workload, out = sys.argv[1], sys.argv[2]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    install()
    import bench
    sys.argv = ['bench.py', '--gpus', '1', '--workload', workload, '--steps', '1', '--warmup', '3']
    try:
        bench.main()
    except SystemExit as e:
        if e.code not in (0, None):
            raise
    dump(out)
