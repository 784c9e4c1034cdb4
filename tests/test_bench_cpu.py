"""bench.py's cpu_baseline leg (the oracle's torch-CPU restatement timed beside the GPU line) on a tiny grid: the record carries the
thread-count sweep (every count's rate in the line, the best one re-measured over a longer window)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_cpu_baseline_reports_its_thread_sweep():
    import torch
    import bench
    from oracle import np_ref
    from dlwp_amd.presets import unet_layers
    grid, cin = (8, 12), 4
    weights = np_ref.init_weights(unet_layers((cin,) + grid), cin, np.random.default_rng(0))
    before = torch.get_num_threads()
    try:
        rec = bench.cpu_baseline(grid, cin, 4, weights, budget_s=0.6, warm_s=0.05, sweep_s=0.15)
    finally:
        torch.set_num_threads(before)
    assert rec['kind'] == 'port' and rec['value'] > 0 and rec['unit'] == '6-h forecast steps/s'
    counts = sorted(int(k) for k in rec['sweep'])
    ncpu = os.cpu_count() or 1
    assert counts == sorted({min(ncpu, v) for v in (8, 16, 32)}) and rec['cores'] in counts
    assert all(v > 0 for v in rec['sweep'].values())
    assert rec['sweep'][str(rec['cores'])] == max(rec['sweep'].values())


def test_dump_outputs_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: a series within the budget is written whole; a larger one as the same seeded selection on every run
    (whole members + flat elements), float32, never more than the budget."""
    import torch
    import bench
    small = torch.randn((3, 5, 8, 6, 10), generator=torch.Generator().manual_seed(1))
    rec = bench.dump_outputs(small, str(tmp_path / 'small'))
    assert rec['files'] == {'series.npy': [3, 5, 8, 6, 10]}
    assert np.array_equal(np.load(tmp_path / 'small' / 'series.npy'), small.numpy())
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 64 << 10)
    big = torch.randn((4, 40, 8, 12, 20), generator=torch.Generator().manual_seed(2))
    recs = [bench.dump_outputs(big, str(tmp_path / d)) for d in ('a', 'b')]
    assert recs[0]['files'] == recs[1]['files'] and recs[0]['members'] == recs[1]['members']
    total = 0
    for name in recs[0]['files']:
        a, b = np.load(tmp_path / 'a' / name), np.load(tmp_path / 'b' / name)
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / 'a' / name)
    assert total <= 64 << 10
    members = recs[0]['members']
    assert members == sorted(members) and 0 < len(members) < 40
    assert np.array_equal(np.load(tmp_path / 'a' / 'series_members.npy'), big[:, members].numpy())
    sample = np.load(tmp_path / 'a' / 'series_sample.npy')
    assert np.isin(sample, big.numpy().ravel()).all()
