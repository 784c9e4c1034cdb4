#!/usr/bin/env python3
"""BatchNormalization(axis=1) on the MI355X (csrc/batchnorm.hip): HIP-event time and ALGORITHMIC GB/s of each entry point at the
config-3 training shapes (64 samples; the five sites behind the tanh Conv2D layers of examples/train.py:159-219: 32 / 64 / 128 /
64 / 32 channels at 88 x 180, 44 x 90, 22 x 45, 44 x 90, 88 x 180), and the config-3 training step with BatchNormalization at all
five sites against the same model without it.  Writes profiles/bench_batchnorm.json (with the kernel source hash).  GPU only.

Algorithmic bytes per element (float32): training forward 12 (statistics pass reads x, the affine pass reads x and writes y),
inference 8, backward 20 (the sums read x and dy, the element pass reads both again and writes dx)."""
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

SITES = ((32, 88, 180), (64, 44, 90), (128, 22, 45), (64, 44, 90), (32, 88, 180))


def timeit(fn, iters, repeats=3):
    """ms per call: the best of `repeats` event-bracketed runs of `iters` calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        best = ms if best is None else min(best, ms)
    return best


def kernels(n, iters):
    rows = []
    for c, h, w in SITES:
        x = torch.randn((n, c, h, w), device='cuda') * 2.0 + 1.0
        dy = torch.randn_like(x)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        g, b = torch.ones(c, device='cuda'), torch.zeros(c, device='cuda')
        mm, mv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
        sm, si = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
        dg, db = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
        ws = torch.zeros(ops.batchnorm_workspace_bytes(ops.batchnorm_desc(x)), dtype=torch.uint8, device='cuda')
        elems = float(x.numel())
        for name, fn, per in (
                ('fwd_train', lambda: ops.batchnorm_fwd_train(x, g, b, mm, mv, sm, si, ws, out=y), 12),
                ('fwd_infer', lambda: ops.batchnorm_fwd_infer(x, g, b, mm, mv, out=y), 8),
                ('bwd', lambda: ops.batchnorm_bwd(x, dy, g, sm, si, ws, dgamma=dg, dbeta=db, dx=dx), 20)):
            ms = timeit(fn, iters)
            rows.append({'kernel': 'batchnorm_' + name, 'shape': [n, c, h, w], 'ms': ms, 'us': 1e3 * ms,
                         'bytes': per * elems, 'gbs': per * elems / ms / 1e6})
    return rows


def step_ms(with_bn, n, steps, warmup):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    cs = (4, 88, 180)
    specs = []
    for spec in unet_layers(cs):
        specs.append(spec)
        if with_bn and spec[0] == 'Conv2D' and spec[2].get('activation') == 'tanh':
            specs.append(('BatchNormalization', None, {'axis': 1}))
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(tuple(specs), loss='mse', optimizer=Adam(lr=1e-4), metrics=['mae'])
    tr = d.model._trainer
    x = torch.randn((n,) + cs, device='cuda')
    y = torch.randn((n,) + cs, device='cuda')
    for _ in range(warmup):
        tr.train_on_shard(x, y, n, return_device=True)
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            tr.train_on_shard(x, y, n, return_device=True)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        best = ms if best is None else min(best, ms)
    return best, tr._graph_ok(n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_batchnorm.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_batchnorm.py needs a GPU')
    rows = kernels(args.n, args.iters)
    for r in rows:
        print('%-20s %-22s %8.1f us %7.0f GB/s' % (r['kernel'], r['shape'], r['us'], r['gbs']))
    plain, form0 = step_ms(False, args.n, args.steps, args.warmup)
    bn, form1 = step_ms(True, args.n, args.steps, args.warmup)
    print('config-3 training step, %d samples: %.3f ms without BatchNormalization (%s), %.3f ms with it at 5 sites (%s): +%.3f ms'
          % (args.n, plain, form0, bn, form1, bn - plain))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'samples': args.n, 'peak_gbs': 8000.0,
                     'device': torch.cuda.get_device_name(0)},
           'kernels': rows,
           'step': {'ms_without_bn': plain, 'ms_with_bn': bn, 'delta_ms': bn - plain, 'form_without_bn': str(form0),
                    'form_with_bn': str(form1)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
