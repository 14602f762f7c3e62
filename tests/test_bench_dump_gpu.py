"""bench.py on the GPU: a plain run measures only its timed steps, and ``--dump-outputs DIR`` writes
what the last timed step computed (small RCAN tile so the run takes seconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(cuda, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    out = tmp_path / 'dump'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '3',
                        '--workload', 'rcan', '--batch', '2', '--lr-px', '32', '--dump-outputs', str(out)],
                       env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1 and [ln for ln in p.stdout.splitlines() if ln.strip()] == lines, (p.stdout, p.stderr)
    d = json.loads(lines[0])
    assert d['steps'] == 2 and d['warmup'] == 3 and d['ms_per_step'] > 0
    assert d['unit'] == 'HR-pixels/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    assert abs(d['value'] - 2 * 128 * 128 / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    # nothing beside the timed steps was measured
    assert d['roofline'] is None and d['cpu_baseline'] is None and d['parity'] is None
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrays) == {'output', 'loss', 'params', 'params_ema', 'grads'}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays['output'].shape == (2, 3, 128, 128)
    assert arrays['loss'].shape == (1,) and abs(float(arrays['loss'][0]) - d['last_loss']) <= 1e-6 * abs(d['last_loss'])
    assert arrays['params'].shape == arrays['params_ema'].shape == arrays['grads'].shape
    assert np.abs(arrays['grads']).max() > 0
    # the EMA (decay 0.999) trails the trained parameters after 5 steps: close, not equal
    diff = np.abs(arrays['params'] - arrays['params_ema']).max()
    assert 0 < diff < 1e-2
