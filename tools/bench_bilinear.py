#!/usr/bin/env python3
"""Bilinear UpSampling2D(2) on the MI355X (csrc/halo.hip): HIP-event time, ALGORITHMIC GB/s (tensors in + tensors out) and the
fraction of the 8 TB/s HBM peak of dlwp_upsample2_bilinear_fwd / _bwd at the U-Net's two up-sampling maps -- M x 128 x 22 x 45 ->
44 x 90 (odd W: 8-byte (even, odd) pairs) and M x 64 x 44 x 90 -> 88 x 180 (even W: 16-byte accesses) with M = 8, 64 and 256
members -- beside the nearest dlwp_upsample2_fwd / _bwd on the same tensors in the same run (the yardstick: the same bytes),
alternating, with the spread over the rounds.  Then what the launch costs a model: the config-3 training step and the 28-call
rollout of the U-Net with bilinear against nearest decoders (nearest up-sampling is read lazily by the next convolution; a bilinear
layer is a launch and a stored tensor of its own).  Writes profiles/bench_bilinear.json (with the kernel source hash).  GPU only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402
from dlwp_amd.presets import unet_layers  # noqa: E402

PEAK_GBS = 8000.0          # the HBM peak DESIGN.md section 5.4 quotes its fractions against
MAPS = ((128, 22, 45), (64, 44, 90))
MEMBERS = (8, 64, 256)


def timeit(fns, iters, rounds=5):
    """[(median ms per call, (max - min) / median)] of every function: `rounds` rounds that ALTERNATE over the functions, each an
    event-bracketed run of `iters` calls, after a warm-up of every function"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    return [(float(np.median(m)), (max(m) - min(m)) / float(np.median(m))) for m in ms]


def kernels(shape, iters, rounds):
    n, c, h, w = shape
    x = torch.randn(shape, device='cuda')
    y = torch.empty((n, c, 2 * h, 2 * w), device='cuda')
    dy, dx = torch.randn_like(y), torch.empty_like(x)
    nbytes = 4.0 * (x.numel() + y.numel())
    cases = (('dlwp_upsample2_bilinear_fwd', lambda: ops.upsample2_bilinear(x, out=y)),
             ('dlwp_upsample2_fwd', lambda: ops.upsample2(x, out=y)),
             ('dlwp_upsample2_bilinear_bwd', lambda: ops.upsample2_bilinear_bwd(dy, shape, out=dx)),
             ('dlwp_upsample2_bwd', lambda: ops.upsample2_bwd(dy)))                 # (allocates its dx from torch's cache)
    route = '16-byte' if w % 2 == 0 else '8-byte pairs'
    rows = []
    for (name, fn), (ms, spread) in zip(cases, timeit([cs[1] for cs in cases], iters, rounds)):
        rows.append({'kernel': name, 'shape': list(shape), 'route': route if 'bilinear' in name else None, 'us': 1e3 * ms,
                     'spread': spread, 'bytes': nbytes, 'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS})
    return rows


def build(interpolation):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    specs = tuple((name, args, dict(kw, interpolation=interpolation) if name == 'UpSampling2D' else kw)
                  for name, args, kw in unet_layers((4, 88, 180)))
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(specs, loss='mse', optimizer=Adam(lr=1e-4), metrics=['mae'])
    return d


def model_costs(n, steps, warmup, calls):
    """nearest and bilinear U-Net, alternating: the training step, then the rollout"""
    kinds = ('nearest', 'bilinear')
    nets = [build(k) for k in kinds]
    x = torch.randn((n, 4, 88, 180), device='cuda')
    y = torch.randn_like(x)
    for d in nets:
        for _ in range(warmup):                    # (the step is recorded and replayed from its third call on)
            d.model._trainer.train_on_shard(x, y, n, return_device=True)
        d.model.rollout_on_device(x, calls)
    step = timeit([lambda d=d: d.model._trainer.train_on_shard(x, y, n, return_device=True) for d in nets], steps, rounds=5)
    roll = timeit([lambda d=d: d.model.rollout_on_device(x, calls) for d in nets], 3, rounds=5)
    return [{'interpolation': kind, 'samples': n, 'step_ms': step[k][0], 'step_spread': step[k][1],
             'step_form': str(d.model._trainer._graph_ok(n)), 'launches_training_plan': len(d.model.plan.ops),
             'launches_inference_plan': len(d.model.infer_plan.ops), 'rollout_calls': calls, 'rollout_ms': roll[k][0],
             'rollout_spread': roll[k][1], 'rollout_steps_per_s': n * calls * 2 / (roll[k][0] * 1e-3)}
            for k, (kind, d) in enumerate(zip(kinds, nets))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--members', type=int, default=64, help='samples of the training step and members of the rollout')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=28, help='model calls of the rollout (28 = 14 days of 2 x 6 h)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_bilinear.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_bilinear.py needs a GPU')
    rows = []
    for m in MEMBERS:
        for cmap in MAPS:
            rows += kernels((m,) + cmap, args.iters, args.rounds)
    for r in rows:
        print('%-28s %-18s %-13s %8.1f us %7.0f GB/s %5.3f of peak  spread %4.1f %%' % (
            r['kernel'], 'x'.join(map(str, r['shape'])), r['route'] or '', r['us'], r['gbs'], r['of_peak'], 100 * r['spread']))
    models = model_costs(args.members, args.steps, args.warmup, args.calls)
    for m in models:
        print('U-Net, %-8s decoders: step of %d samples %.3f ms (%s, %d launches planned, spread %.1f %%); rollout of %d calls '
              '%.3f ms = %.0f steps/s (%d launches per call, spread %.1f %%)' % (
                  m['interpolation'], m['samples'], m['step_ms'], m['step_form'], m['launches_training_plan'],
                  100 * m['step_spread'], m['rollout_calls'], m['rollout_ms'], m['rollout_steps_per_s'],
                  m['launches_inference_plan'], 100 * m['rollout_spread']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds}, 'kernels': rows, 'models': models}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
