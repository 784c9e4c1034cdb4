#!/usr/bin/env python3
"""Dense kernels on the MI355X (csrc/dense.hip): HIP-event time, GB/s of weight traffic and TFLOP/s of forward, data gradient and
weight gradient at the two layer shapes of the reference's feed-forward model on its own grid (examples/train_generator.py:224-233;
36 x 144 x 2 variables x 2 time steps: 20 736 -> 10 368 -> 20 736) and batch 1, 8, 32, 64, 256; beside each,
torch.nn.functional.linear (and its autograd) in the same process as an outside yardstick; and the whole feed-forward training step
at batch 64.  Writes profiles/bench_dense.json (with the kernel source hash).  GPU only.

Bounds quoted: a launch reads (forward, data gradient) or writes (weight gradient) the k x n float32 weights once -- 8 TB/s -- and
multiplies 2 m k n FLOP on the float32 matrix instruction -- 157.3 TFLOP/s.  Each figure is the median of `repeats` event-bracketed
runs of `iters` launches after a warm-up; the spread (min, max) is kept in the file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402

PEAK_GBS, PEAK_TFLOPS = 8000.0, 157.3


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


def kernels(shapes, batches, iters):
    rows = []
    for k, n in shapes:
        w = (torch.rand((k, n), device='cuda') - 0.5) * (2.0 * (6.0 / (k + n)) ** 0.5)
        wt = w.t().contiguous()              # torch.nn.functional.linear takes (out, in)
        b = torch.zeros(n, device='cuda')
        dw, db = torch.empty_like(w), torch.empty_like(b)
        for m in batches:
            x = torch.randn((m, k), device='cuda')
            dy = torch.randn((m, n), device='cuda')
            y = ops.dense_fwd(x, w, b, 'tanh')
            dx = torch.empty_like(x)
            xt = x.clone().requires_grad_(True)
            wp = wt.clone().requires_grad_(True)
            yt = torch.nn.functional.linear(xt, wp, b)
            flop = 2.0 * m * k * n
            wbytes = 4.0 * k * n
            its = max(3, iters // (1 + m // 64))
            for name, fn, ref in (
                    ('dense_fwd', lambda: ops.dense_fwd(x, w, b, 'tanh', out=y),
                     lambda: torch.tanh(torch.nn.functional.linear(x, wt, b))),
                    ('dense_bwd_data', lambda: ops.dense_bwd_data(dy, y, w, 'tanh', out=dx),
                     lambda: torch.autograd.grad(yt, xt, dy, retain_graph=True)),
                    ('dense_bwd_weight', lambda: ops.dense_bwd_weight(x, dy, y, dw, db, 'tanh'),
                     lambda: torch.autograd.grad(yt, wp, dy, retain_graph=True))):
                med, lo, hi = timeit(fn, its)
                tmed, tlo, thi = timeit(ref, its)
                bound = 'weights' if m <= 32 else 'matrix'
                frac = (wbytes / med / 1e6) / PEAK_GBS if bound == 'weights' else (flop / med / 1e9) / PEAK_TFLOPS
                rows.append({'kernel': name, 'm': m, 'k': k, 'n': n, 'us': 1e3 * med, 'us_min': 1e3 * lo, 'us_max': 1e3 * hi,
                             'weight_gbs': wbytes / med / 1e6, 'tflops': flop / med / 1e9, 'bound': bound, 'fraction_of_bound': frac,
                             'torch_us': 1e3 * tmed, 'torch_us_min': 1e3 * tlo, 'torch_us_max': 1e3 * thi})
                print('%-17s m %3d  %5d -> %5d  %9.1f us %7.0f GB/s %6.1f TFLOP/s  %4.1f %% of the %s bound   torch %9.1f us'
                      % (name, m, k, n, 1e3 * med, wbytes / med / 1e6, flop / med / 1e9, 100 * frac, bound, 1e3 * tmed), flush=True)
            del xt, wp, yt
        del w, wt, dw
        torch.cuda.empty_cache()
    return rows


def step_ms(f, n, steps, warmup):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.regularizers import l2
    from dlwp_amd.training import Adam
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=False, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model((('Dense', (f // 2,), {'activation': 'tanh', 'kernel_regularizer': l2(1e-4), 'input_shape': (f,)}),
                   ('Dropout', (0.25,), None),
                   ('Dense', (f,), None)), loss='mse', optimizer=Adam(lr=1e-4))
    tr = d.model._trainer
    x = torch.randn((n, f), device='cuda')
    y = torch.randn((n, f), device='cuda')
    for _ in range(warmup):
        tr.train_on_shard(x, y, n, return_device=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            tr.train_on_shard(x, y, n, return_device=True)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return statistics.median(ms), min(ms), max(ms), d.model.count_params()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--features', type=int, default=20736)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 32, 64, 256])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_dense.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dense.py needs a GPU')
    f = args.features
    rows = kernels(((f, f // 2), (f // 2, f)), args.batches, args.iters)
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'peak_tflops': PEAK_TFLOPS,
                     'device': torch.cuda.get_device_name(0), 'features': f}, 'kernels': rows}
    if not args.no_step:
        med, lo, hi, params = step_ms(f, 64, args.steps, args.warmup)
        print('feed-forward training step (Dense tanh l2 -> Dropout -> Dense, Adam), 64 samples, %d parameters: %.2f ms (%.2f - %.2f)'
              % (params, med, lo, hi))
        res['step'] = {'samples': 64, 'parameters': params, 'ms': med, 'ms_min': lo, 'ms_max': hi}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
