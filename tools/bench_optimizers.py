#!/usr/bin/env python3
"""The Keras optimizers on the MI355X (csrc/optimizers.hip): HIP-event time and ALGORITHMIC GB/s of dlwp_optimizer_step for every kind
and of the clip pass (dlwp_grad_clip_factor), at the U-Net's 188 996 parameters (launch latency: us only) and at the 215 000 000 of
the dense model of tools/bench_dense.py (an HBM stream), with dlwp_adam_keras -- the kernel of unclipped Adam, untouched -- in the
SAME run, alternating round by round with the new kernels.  Writes profiles/optimizers.json (with the kernel source hash).  GPU only.

Algorithmic bytes: 4 n (arrays read + arrays written): p and every slot are read and written, g is read -- 4 n (2 (1 + slots) + 1);
the clip pass reads g: 4 n.  At 215 M each kind's GB/s is held against 0.9 x Adam's (same traffic pattern; the margin covers the
2-5 % run-to-run spread)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402

KINDS = ('sgd', 'sgd_nesterov', 'rmsprop', 'adagrad', 'adadelta', 'adam', 'adam_amsgrad', 'adamax', 'nadam')
PEAK_GBS = 8000.0


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench(n, iters, rounds):
    p = torch.randn(n, device='cuda')
    g = torch.randn(n, device='cuda') * 1e-3
    slots = [torch.zeros(n, device='cuda') for _ in range(3)]
    factor = torch.ones(3, device='cuda')
    hyper = dict(lr=1e-3, h1=0.9, h2=0.999, epsilon=1e-7, schedule_decay=0.004)
    cases = {'dlwp_adam_keras': (lambda: ops.adam_keras(p, slots[0], slots[1], g, 7), 7)}
    for k, name in enumerate(KINDS):
        ns = ops.OPT_SLOTS[k]
        cases[name] = (lambda k=k, ns=ns: ops.optimizer_step(k, p, slots[:ns], g, 7, m_schedule=0.5, **hyper), 2 * (1 + ns) + 1)
    # the clipped update (factor from the device, clamp) moves the same bytes as the plain one
    cases['adam + clipnorm factor + clipvalue'] = (
        lambda: ops.optimizer_step(ops.OPT_ADAM, p, slots[:2], g, 7, clipvalue=1.0, factor=factor, **hyper), 7)
    cases['clip pass (dlwp_grad_clip_factor)'] = (lambda: ops.grad_clip_factor(g, 1.0, 1.0, out=factor), 1)
    times = {name: [] for name in cases}
    for fn, _ in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):                 # alternate: every round times every kernel once, dlwp_adam_keras among them
        for name, (fn, _) in cases.items():
            times[name].append(event_ms(fn, iters))
    rows = []
    for name, (_, arrays) in cases.items():
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        nbytes = 4.0 * n * arrays
        rows.append({'kernel': name, 'n': n, 'arrays': arrays, 'us': 1e3 * med, 'us_min': 1e3 * ts[0], 'us_max': 1e3 * ts[-1],
                     'bytes': nbytes, 'gbs': nbytes / med / 1e6, 'fraction_of_peak': nbytes / med / 1e6 / PEAK_GBS})
    adam = rows[0]['gbs']
    for r in rows:
        r['gbs_vs_adam_keras'] = r['gbs'] / adam
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--small', type=int, default=188996)
    ap.add_argument('--large', type=int, default=215000000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optimizers.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_optimizers.py needs a GPU')
    small = bench(args.small, 200, args.rounds)
    large = bench(args.large, 5, args.rounds)
    print('n = %d (launch latency)' % args.small)
    for r in small:
        print('  %-40s %8.2f us (%.2f - %.2f)' % (r['kernel'], r['us'], r['us_min'], r['us_max']))
    print('n = %d (HBM stream; peak %.0f GB/s)' % (args.large, PEAK_GBS))
    for r in large:
        print('  %-40s %9.1f us %7.0f GB/s  %4.1f %% of peak  %.3f x dlwp_adam_keras' % (
            r['kernel'], r['us'], r['gbs'], 100 * r['fraction_of_peak'], r['gbs_vs_adam_keras']))
    slow = [r['kernel'] for r in large if r['kernel'] != 'clip pass (dlwp_grad_clip_factor)' and r['gbs_vs_adam_keras'] < 0.9]
    print('below 0.9 x dlwp_adam_keras at n = %d: %s' % (args.large, ', '.join(slow) if slow else 'none'))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'rounds': args.rounds, 'below_0.9x_adam_keras': slow},
           'small': small, 'large': large}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
