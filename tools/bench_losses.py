#!/usr/bin/env python3
"""The Keras regression losses on the MI355X (csrc/losses.hip): HIP-event time and ALGORITHMIC GB/s of dlwp_loss_elementwise (value +
gradient) per kind, plain and on a restated output layer's phase channels (dlwp_loss_elementwise_phase), and of one
dlwp_loss_metrics pass with every metric, at the config-3 output (64, 4, 88, 180) and the 8-sample shape; then the config-3
training step at 64 samples with loss='mse', 'mae' and 'logcosh', alternated in one process.  Writes
profiles/bench_losses.json (with the kernel source hash).  GPU only.

Algorithmic bytes per element (float32): value + gradient 12 (read yp, yt, write dy), metrics 8 (read yp, yt)."""
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

KINDS = ('mse', 'mae', 'mape', 'msle', 'logcosh')
CS = (4, 88, 180)


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
    f, hh, ww = CS
    yp = torch.randn((n,) + CS, device='cuda')
    yt = torch.randn_like(yp)
    dy = torch.empty_like(yp)
    yph = torch.randn((n, 4 * f, hh // 2, ww // 2), device='cuda')
    dz = torch.empty_like(yph)
    db = torch.empty(4 * f, device='cuda')
    out = torch.zeros(8, device='cuda')
    elems = float(yp.numel())
    for kind, name in enumerate(KINDS):
        for form, fn in (('plain', lambda k=kind: ops.loss_elementwise(yp, yt, out[:1], dy, 1.0, k)),
                         ('phase', lambda k=kind: ops.loss_elementwise_phase(yph, yt, out[:1], dz, db, 1.0, k))):
            ms = timeit(fn, iters)
            rows.append({'kernel': 'loss_elementwise' + ('_phase' if form == 'phase' else ''), 'kind': name,
                         'shape': [n] + list(CS), 'ms': ms, 'us': 1e3 * ms, 'bytes': 12 * elems, 'gbs': 12 * elems / ms / 1e6})
    mask = 0x1f | _lib.METRIC_ACC_SUMS
    for form, fn in (('plain', lambda: ops.loss_metrics(yp, yt, out, mask)),
                     ('phase', lambda: ops.loss_metrics(yph, yt, out, mask, phase=True))):
        ms = timeit(fn, iters)
        rows.append({'kernel': 'loss_metrics' + ('_phase' if form == 'phase' else ''), 'kind': 'all 5 + ACC sums',
                     'shape': [n] + list(CS), 'ms': ms, 'us': 1e3 * ms, 'bytes': 8 * elems, 'gbs': 8 * elems / ms / 1e6})
    return rows


def build(loss):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(unet_layers(CS), loss=loss, optimizer=Adam(lr=1e-4), metrics=['mae'])
    return d.model._trainer


def steps_ms(n, steps, warmup, rounds):
    """the config-3 step per loss, the losses alternated round by round in one process: best of `rounds` per loss"""
    losses = ('mse', 'mae', 'logcosh')
    trs = {loss: build(loss) for loss in losses}
    x = torch.randn((n,) + CS, device='cuda')
    y = torch.randn((n,) + CS, device='cuda')
    for tr in trs.values():
        for _ in range(warmup):
            tr.train_on_shard(x, y, n, return_device=True)
    torch.cuda.synchronize()
    best = {}
    for _ in range(rounds):
        for loss, tr in trs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                tr.train_on_shard(x, y, n, return_device=True)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / steps
            best[loss] = min(best.get(loss, ms), ms)
    return {loss: {'ms': best[loss], 'form': str(trs[loss]._graph_ok(n)), 'phase_loss': bool(trs[loss]._phase_outputs())}
            for loss in losses}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_losses.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_losses.py needs a GPU')
    rows = kernels(64, args.iters) + kernels(8, args.iters)
    for r in rows:
        print('%-24s %-8s %-20s %8.1f us %7.0f GB/s' % (r['kernel'], r['kind'], r['shape'], r['us'], r['gbs']))
    step = steps_ms(64, args.steps, args.warmup, args.rounds)
    for loss, r in step.items():
        print('config-3 training step, 64 samples, loss=%-8r %.3f ms (%s, loss on phase channels: %s)'
              % (loss, r['ms'], r['form'], r['phase_loss']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': 8000.0, 'device': torch.cuda.get_device_name(0)},
           'kernels': rows, 'step_b64': step}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
