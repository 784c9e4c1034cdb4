#!/usr/bin/env python3
"""The wrapper's scaler and imputer on the MI355X (csrc/scale.hip): HIP-event time and GB/s of the two kernels at 256 samples of
20 736 features (the reference's feed-forward model on its own grid: 36 x 144 x 2 variables x 2 time steps), every scaler kind,
with and without the imputer, in place and out of place; and predict_timeseries steps/s of a scaled feed-forward wrapper
(StandardScaler, Dense tanh -> Dropout -> Dense) on the host path (DLWP_SCALER_HOST=1: sklearn around every model call, one
upload and one download per forecast step) against the device path (the scaler inside the model call, one captured hipGraph).
Writes profiles/bench_scaler_rollout.json (with the kernel source hash).  GPU only.

Bound quoted: a launch reads and writes n x f float32 values once (the float64 parameters, 8 f bytes each, stay in the L2) against
8 TB/s; the yardstick for a pure streaming kernel here is what the pad kernels reach, 0.57-0.70 of that.  Each figure is the
median of `repeats` event-bracketed runs of `iters` launches after a warm-up; the spread (min, max) is kept in the file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402

PEAK_GBS = 8000.0


def timeit(fn, iters, repeats=5):
    """(median, min, max) ms per call over `repeats` event-bracketed runs of `iters` calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms), max(ms)


def kernels(n, f, iters):
    rows = []
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((n, f)).astype(np.float32)).cuda()
    holes = x.clone()
    holes[torch.rand_like(holes) < 0.1] = float('nan')
    y = torch.empty_like(x)
    shift = torch.from_numpy(rng.standard_normal(f)).cuda()
    scale = torch.from_numpy(np.abs(rng.standard_normal(f)) + 0.5).cuda()
    fill = torch.from_numpy(rng.standard_normal(f)).cuda()
    nbytes = 8.0 * n * f                                    # one float32 read and one write per element
    work = x.clone()
    for kind in ('standard', 'minmax'):
        for name, fn in (
                ('scale_fwd', lambda: ops.scale_fwd(x, kind, None, shift, scale, out=y)),
                ('scale_fwd + impute', lambda: ops.scale_fwd(holes, kind, fill, shift, scale, out=y)),
                ('scale_fwd in place', lambda: ops.scale_fwd(work, kind, None, shift, None, out=work)),
                ('scale_inv', lambda: ops.scale_inv(x, kind, shift, scale, out=y)),
                ('scale_inv in place', lambda: ops.scale_inv(work, kind, shift, None, out=work))):
            med, lo, hi = timeit(fn, iters)
            gbs = nbytes / med / 1e6
            rows.append({'kernel': name, 'kind': kind, 'n': n, 'f': f, 'us': 1e3 * med, 'us_min': 1e3 * lo, 'us_max': 1e3 * hi,
                         'gbs': gbs, 'fraction_of_hbm_peak': gbs / PEAK_GBS})
            print('%-20s %-8s %4d x %6d  %8.1f us (%.1f - %.1f)  %7.0f GB/s  %.2f of the HBM peak'
                  % (name, kind, n, f, 1e3 * med, 1e3 * lo, 1e3 * hi, gbs, gbs / PEAK_GBS), flush=True)
    return rows


def rollout(f, n, steps, repeats):
    """predict_timeseries of a StandardScaler wrapper: steps/s = members x forecast steps per second, numpy in, numpy out"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    rng = np.random.default_rng(1)
    d = DLWPNeuralNet(is_convolutional=False, is_recurrent=False, time_dim=2)           # the reference's default: StandardScaler
    d.build_model((('Dense', (f // 2,), {'activation': 'tanh', 'input_shape': (f,)}), ('Dropout', (0.25,), None),
                   ('Dense', (f,), None)), loss='mse', optimizer='adam')
    fit = (rng.standard_normal((n, f)) * 3 + 5).astype(np.float32)
    d.init_fit(fit, fit)
    x = (rng.standard_normal((n, f)) * 3 + 5).astype(np.float32)

    def use(path):
        if path == 'host':
            os.environ['DLWP_SCALER_HOST'] = '1'
        else:
            os.environ.pop('DLWP_SCALER_HOST', None)
            assert d._device_io(x), 'the wrapper is not eligible for the device path'

    def run(path):
        use(path)
        out = d.predict_timeseries(x, steps, return_device=(path == 'device_resident'))
        if path == 'device_resident':
            torch.cuda.synchronize()
        return out
    paths = ('host', 'device', 'device_resident')       # device_resident: return_device=True, the series stays in HBM
    last, ts = {}, {p: [] for p in paths}
    for p in paths:
        run(p)                                              # warm-up: allocations, the graph capture
    for _ in range(repeats):                                # the paths alternate: other work shares the host
        for p in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[p] = run(p)
            ts[p].append(time.perf_counter() - t0)
    res = {}
    for p in paths:
        med = statistics.median(ts[p])
        res[p] = {'seconds': med, 'seconds_min': min(ts[p]), 'seconds_max': max(ts[p]), 'steps_per_s': n * steps / med,
                  'all_ms': [round(1e3 * t, 2) for t in ts[p]], 'series': last[p]}
        print('predict_timeseries, %-15s path: %d members x %d steps of %d features  %.1f ms (%.1f - %.1f)  %.0f steps/s'
              % (p, n, steps, f, 1e3 * med, 1e3 * min(ts[p]), 1e3 * max(ts[p]), res[p]['steps_per_s']), flush=True)
    os.environ.pop('DLWP_SCALER_HOST', None)
    res['device_resident'].pop('series')
    same = np.array_equal(res['host'].pop('series').view(np.int32), res['device'].pop('series').view(np.int32))
    print('device series == host series bit for bit: %s;  device / host: %.1f x' %
          (same, res['device']['steps_per_s'] / res['host']['steps_per_s']))
    return dict(res, members=n, steps=steps, features=f, bit_identical=bool(same),
                speedup=res['device']['steps_per_s'] / res['host']['steps_per_s'])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--features', type=int, default=20736)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--members', type=int, default=64)
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--no-rollout', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_scaler_rollout.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scaler_rollout.py needs a GPU')
    rows = kernels(args.samples, args.features, args.iters)
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0)},
           'kernels': rows}
    if not args.no_rollout:
        res['predict_timeseries'] = rollout(args.features, args.members, args.steps, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
