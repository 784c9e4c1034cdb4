#!/usr/bin/env python3
"""The HBM-resident series feed on the MI355X (csrc/series.hip, DeviceLoader's 'resident' mode).

1. The kernel alone: HIP-event time, GB/s over read + written bytes and the fraction of the 8 TB/s HBM peak of
   dlwp_series_window_gather on batches of 8 / 64 / 256 shuffled samples of a two-field 88 x 180 series, in the two shapes a
   SeriesDataGenerator is trained with -- examples/train_functional.py's (input_time_steps=2, output_time_steps=2, sequence=6,
   add_insolation=True: 1.9 MB per sample) and the same without sequence and insolation (0.5 MB per sample) -- each beside
   dlwp_gather_rows_fill moving the same number of bytes as whole states in the same run, alternating.
2. What a caller sees: fit_generator ms per step of the 64-sample U-Net (presets.unet_layers on 4 x 88 x 180) with the host feed
   (DLWP_SERIES_HOST=1: generate() in numpy, pinned copy, upload -- every batch's path before), with the device feed, and
   Trainer.fit on arrays that already are in HBM (batches cut there by index_select): alternating repetitions, median and spread.
   No preset builds the multi-output functional model of train_functional.py, so that shape is measured as a kernel only.
Writes profiles/bench_series_feed.json (with the kernel source hash).  GPU only."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402
from dlwp_amd.model import DLWPNeuralNet, SeriesDataGenerator, SeriesDataset  # noqa: E402
from dlwp_amd.presets import unet_layers  # noqa: E402
from tools.bench_verify import PEAK_GBS, timeit  # noqa: E402

GRID = (88, 180)
FIELDS = 2
LL = ctypes.c_longlong
SHAPES = {'train_functional': dict(input_time_steps=2, output_time_steps=2, sequence=6, add_insolation=True),
          'plain': dict(input_time_steps=2, output_time_steps=2)}


def dataset(T, seed=0):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((T, FIELDS, 1) + GRID, dtype=np.float32)
    times = np.datetime64('1979-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
    return SeriesDataset(s, {'sample': times, 'variable': np.array(['z', 't']), 'level': np.array([500]),
                             'lat': np.linspace(-87, 87, GRID[0]), 'lon': np.arange(GRID[1]) * 2.0},
                         ('sample', 'variable', 'level', 'lat', 'lon'))


def net():
    np.random.seed(0)
    return DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)


def kernel_rows(ds, iters, rounds):
    out = []
    m = net()
    for name, kw in SHAPES.items():
        gen = SeriesDataGenerator(m, ds, batch_size=64, shuffle=True, **kw)
        plan = gen.window_plan()
        srcs = [torch.from_numpy(a).cuda() for a in plan.sources]
        state = srcs[0]                                   # (T, one state): the yardstick gathers whole states
        per_sample = sum(plan.rows)
        assert per_sample % state.shape[1] == 0
        for n in (8, 64, 256):
            bufs = [torch.empty((n, r), device='cuda') for r in plan.rows]
            tables = ops.SeriesTables(srcs, bufs, plan.segments)
            samples = torch.from_numpy(np.random.default_rng(n).permutation(gen._n_sample)[:n].astype(np.int64)).cuda()
            k = n * per_sample // state.shape[1]
            rows = torch.from_numpy(np.random.default_rng(n + 1).integers(0, state.shape[0], k).astype(np.int64)).cuda()
            dst = torch.empty((k, state.shape[1]), device='cuda')
            h = _lib.handle(0)

            def yard():
                _lib.check(_lib.lib.dlwp_gather_rows_fill(h, state.data_ptr(), LL(state.shape[0]), LL(state.shape[1]), rows.data_ptr(), LL(k),
                                                          dst.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            (ms, sp), (yms, ysp) = timeit([lambda: tables.launch(samples, n), yard], iters, rounds)
            nbytes = 8.0 * n * per_sample
            r = {'shape': name, 'samples': n, 'segments': int(len(plan.segments)), 'vec': bool(tables.vec),
                 'turns': n * ops.series_chunks(plan.segments, tables.vec), 'grid_cap': ops.series_grid_cap(), 'bytes': nbytes,
                 'us': 1e3 * ms, 'spread': sp, 'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS,
                 'gather_rows_fill_us': 1e3 * yms, 'gather_rows_fill_spread': ysp, 'gather_rows_fill_gbs': nbytes / yms / 1e6}
            r['of_gather_rows_fill'] = r['gbs'] / r['gather_rows_fill_gbs']
            print('%-16s %3d samples %7.1f MB: %8.1f us %5.0f GB/s %5.3f of peak (spread %4.1f %%) | dlwp_gather_rows_fill on the same bytes '
                  '%8.1f us %5.0f GB/s (spread %4.1f %%) | ratio %.2f' % (name, n, nbytes / 1e6, r['us'], r['gbs'], r['of_peak'], 100 * sp,
                                                                         r['gather_rows_fill_us'], r['gather_rows_fill_gbs'], 100 * ysp,
                                                                         r['of_gather_rows_fill']), flush=True)
            out.append(r)
            del bufs, dst
        del srcs
        torch.cuda.empty_cache()
    return out


def feed_rows(ds, steps, reps):
    bs = 64
    cs = (2 * FIELDS,) + GRID
    d = net()
    from dlwp_amd.training import Adam
    d.build_model(unet_layers(cs), loss='mse', optimizer=Adam(lr=1e-4), metrics=['mae'])
    gen = SeriesDataGenerator(d, ds, batch_size=bs, shuffle=True, **SHAPES['plain'])
    assert gen.window_plan() is not None and len(gen) >= steps
    X, y = gen.generate(np.arange(steps * bs))
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    tr = d.model._need_trainer()

    from dlwp_amd.custom import Callback

    class EpochClock(Callback):
        """wall time of every epoch of a call, device drained at both ends"""

        def __init__(self):
            self.ms = []

        def on_epoch_begin(self, epoch, logs=None):
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()

        def on_epoch_end(self, epoch, logs=None):
            torch.cuda.synchronize()
            self.ms.append(1e3 * (time.perf_counter() - self.t0) / steps)

    epochs = 3                               # per call; the first one carries the call's set-up (the loader, the upload of the series)

    def run_feed(host):
        if host:
            os.environ['DLWP_SERIES_HOST'] = '1'
        else:
            os.environ.pop('DLWP_SERIES_HOST', None)
        clock = EpochClock()
        d.fit_generator(gen, steps_per_epoch=steps, epochs=epochs, verbose=0, callbacks=[clock])
        return clock.ms

    def run_fit():
        clock = EpochClock()
        tr.fit(Xd, yd, batch_size=bs, epochs=epochs, verbose=0, shuffle=True, callbacks=[clock])
        return clock.ms

    runs = {'host_feed': lambda: run_feed(True), 'device_feed': lambda: run_feed(False), 'resident_arrays': run_fit}
    for fn in runs.values():                 # warm-up: the step is recorded here
        fn()
    ms, first = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(reps):                    # calls alternate over the three feeds; epochs 2 .. of every call are the steady state
        for k, fn in runs.items():
            t = fn()
            first[k].append(t[0])
            ms[k] += t[1:]
    os.environ.pop('DLWP_SERIES_HOST', None)
    res = {'model': 'unet_layers %r' % (cs,), 'samples': bs, 'steps': steps, 'reps': reps, 'epochs_per_call': epochs,
           'step_form': str(tr._graph_ok(bs)),
           'first_epoch_ms_per_step': {k: float(np.median(v)) for k, v in first.items()}}
    for k, v in ms.items():
        res[k + '_ms_per_step'] = float(np.median(v))
        res[k + '_spread'] = (max(v) - min(v)) / float(np.median(v))
        res[k + '_all'] = [float('%.4f' % t) for t in v]
    res['gather_cost_ms_per_step'] = res['device_feed_ms_per_step'] - res['resident_arrays_ms_per_step']
    print('fit_generator, %d samples, %d steps x %d: host feed %.3f ms per step (spread %.1f %%), device feed %.3f (%.1f %%), fit on resident '
          'arrays %.3f (%.1f %%)' % (bs, steps, reps, res['host_feed_ms_per_step'], 100 * res['host_feed_spread'],
                                     res['device_feed_ms_per_step'], 100 * res['device_feed_spread'], res['resident_arrays_ms_per_step'],
                                     100 * res['resident_arrays_spread']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--states', type=int, default=2920, help='states of the series (two years at six hours: 370 MB)')
    ap.add_argument('--steps', type=int, default=24, help='fit_generator steps per repetition')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_series_feed.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_series_feed.py needs a GPU')
    ds = dataset(args.states)
    kernels = kernel_rows(ds, args.iters, args.rounds)
    feed = feed_rows(ds, args.steps, args.reps)
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds, 'states': args.states, 'grid': list(GRID), 'fields': FIELDS,
                     'host_threads': os.cpu_count()},
           'kernels': kernels, 'fit_generator': feed}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
