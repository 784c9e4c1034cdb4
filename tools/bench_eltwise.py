#!/usr/bin/env python3
"""Activation and merge layers on the MI355X (csrc/eltwise.hip): HIP-event time, ALGORITHMIC GB/s (operands in + results out) and
the fraction of the 8 TB/s HBM peak of each kernel at 8 / 64 / 256 x 32 x 88 x 180 (the last does not fit the 256 MiB cache),
torch's own leaky_relu / add / maximum on the same tensors in the same run, the spread over the repeats -- and what the unfused
launch costs a model: the config-3 training step and the 64-member rollout of the U-Net with `activation='tanh'` fused into its
convolutions against the same net as linear convolutions + Activation('tanh') layers.  Writes profiles/bench_eltwise.json (with
the kernel source hash).  GPU only."""
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
SHAPE = (32, 88, 180)


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


def kernels(n, iters):
    a = torch.randn((n,) + SHAPE, device='cuda') * 3.0
    b, dy = torch.randn_like(a), torch.randn_like(a)
    y, d0, d1 = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    F = torch.nn.functional
    cases = (
        ('activation_fwd leaky_relu', lambda: ops.activation_fwd(a, 'relu', 0.1, out=y), 2),
        ('activation_fwd relu(10, 0.1)', lambda: ops.activation_fwd(a, 'relu', 0.1, 10.0, out=y), 2),
        ('activation_fwd tanh', lambda: ops.activation_fwd(a, 'tanh', out=y), 2),
        ('activation_fwd elu', lambda: ops.activation_fwd(a, 'elu', 1.0, out=y), 2),
        ('activation_bwd leaky_relu', lambda: ops.activation_bwd(a, dy, 'relu', 0.1, out=d0), 3),
        ('activation_bwd tanh', lambda: ops.activation_bwd(a, dy, 'tanh', out=d0), 3),
        ('merge_fwd add (2)', lambda: ops.merge_fwd('add', [a, b], out=y), 3),
        ('merge_fwd maximum (2)', lambda: ops.merge_fwd('maximum', [a, b], out=y), 3),
        ('merge_fwd average (4)', lambda: ops.merge_fwd('average', [a, b, dy, d1], out=y), 5),
        ('merge_bwd add (2)', lambda: ops.merge_bwd('add', [a, b], dy, outs=[d0, d1]), 3),     # (reads dy alone)
        ('merge_bwd multiply (2)', lambda: ops.merge_bwd('multiply', [a, b], dy, outs=[d0, d1]), 5),
        ('merge_bwd maximum (2)', lambda: ops.merge_bwd('maximum', [a, b], dy, outs=[d0, d1]), 5),
        ('torch leaky_relu (allocates)', lambda: F.leaky_relu(a, 0.1), 2),
        ('torch tanh (out=)', lambda: torch.tanh(a, out=y), 2),
        ('torch add (out=)', lambda: torch.add(a, b, out=y), 3),
        ('torch maximum (out=)', lambda: torch.maximum(a, b, out=y), 3),
    )
    d1.copy_(b)
    rows = []
    for (name, fn, arrays), (ms, spread) in zip(cases, timeit([c[1] for c in cases], iters)):
        nbytes = 4.0 * arrays * a.numel()
        rows.append({'kernel': name, 'shape': [n] + list(SHAPE), 'us': 1e3 * ms, 'spread': spread, 'bytes': nbytes,
                     'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS})
    return rows


def unet_specs(split):
    """the config-3 U-Net; split: every Conv2D(activation='tanh') as a linear Conv2D followed by Activation('tanh')"""
    specs = []
    for name, args, kw in unet_layers((4, 88, 180)):
        if split and name == 'Conv2D' and kw.get('activation') == 'tanh':
            specs += [(name, args, dict(kw, activation='linear')), ('Activation', ('tanh',), None)]
        else:
            specs.append((name, args, kw))
    return tuple(specs)


def build(split):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(unet_specs(split), loss='mse', optimizer=Adam(lr=1e-4), metrics=['mae'])
    return d


def model_costs(n, steps, warmup, calls):
    """fused and split U-Net, alternating: the training step, then the rollout"""
    nets = [build(split) for split in (False, True)]
    x = torch.randn((n, 4, 88, 180), device='cuda')
    y = torch.randn_like(x)
    for d in nets:
        for _ in range(warmup):                    # (the step is recorded and replayed from its third call on)
            d.model._trainer.train_on_shard(x, y, n, return_device=True)
        d.model.rollout_on_device(x, calls)
    step = timeit([lambda d=d: d.model._trainer.train_on_shard(x, y, n, return_device=True) for d in nets], steps, rounds=3)
    roll = timeit([lambda d=d: d.model.rollout_on_device(x, calls) for d in nets], 3, rounds=3)
    return [{'split': split, 'samples': n, 'step_ms': step[k][0], 'step_spread': step[k][1],
             'step_form': str(d.model._trainer._graph_ok(n)), 'launches_training_plan': len(d.model.plan.ops),
             'launches_inference_plan': len(d.model.infer_plan.ops), 'rollout_calls': calls, 'rollout_ms': roll[k][0],
             'rollout_spread': roll[k][1], 'rollout_steps_per_s': n * calls * 2 / (roll[k][0] * 1e-3)}
            for k, (split, d) in enumerate(zip((False, True), nets))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 64, 256])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--members', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=28, help='model calls of the rollout (28 = 14 days of 2 x 6 h)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_eltwise.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_eltwise.py needs a GPU')
    rows = []
    for n in args.batches:
        rows += kernels(n, args.iters)
    for r in rows:
        print('%-30s %-20s %9.1f us %7.0f GB/s %5.3f of peak  spread %4.1f %%' % (
            r['kernel'], r['shape'], r['us'], r['gbs'], r['of_peak'], 100 * r['spread']))
    models = model_costs(args.members, args.steps, args.warmup, args.calls)
    for m in models:
        print('U-Net %-28s step of %d samples %.3f ms (%s, %d launches planned, spread %.1f %%); rollout of %d calls %.3f ms = %.0f '
              'steps/s (%d launches per call, spread %.1f %%)' % (
                  'linear + Activation(tanh):' if m['split'] else "activation='tanh' fused:", m['samples'], m['step_ms'],
                  m['step_form'], m['launches_training_plan'], 100 * m['step_spread'], m['rollout_calls'], m['rollout_ms'],
                  m['rollout_steps_per_s'], m['launches_inference_plan'], 100 * m['rollout_spread']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0)},
           'kernels': rows, 'models': models}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
