"""bench.py as a plain run (no --full): the headline line alone -- set-up, warm-up, the timed steps and the dump, nothing measured
beside them.  (The --full line, sub-records included, is checked by tests/test_gpu_parallel.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_prints_the_headline_line_only(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                        '--members', '4', '--dump-outputs', str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['value'] > 0 and rec['ms_per_step'] > 0 and rec['finite'] and rec['higher_is_better'] is True
    assert rec['unit'] == '6-h forecast steps/s' and rec['dtype'] == 'f32' and rec['steps'] == 2 and rec['warmup'] == 1
    assert abs(rec['value'] - 4 * 28 * 2 * 1e3 / rec['ms_per_step']) <= 1e-6 * rec['value']
    assert not {'forward', 'roofline', 'layers', 'sub_records', 'cpu_baseline'} & set(rec), sorted(rec)
    series = np.load(tmp_path / 'series.npy')
    assert rec['dump_outputs']['files'] == {'series.npy': list(series.shape)} and series.shape[1] == 4
    assert np.isfinite(series).all()
