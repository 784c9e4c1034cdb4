#!/usr/bin/env python3
"""AveragePooling2D(2) on the MI355X (csrc/halo.hip): HIP-event time, ALGORITHMIC GB/s (tensors in + tensors out) and the fraction
of the 8 TB/s HBM peak of dlwp_avgpool2_fwd / _bwd at the U-Net's three maps with 256 members -- 256 x 32 x 88 x 180 (two windows
per thread), 256 x 64 x 44 x 90 (one window, 8-byte accesses), 256 x 128 x 22 x 45 (scalar) -- beside dlwp_maxpool2_fwd / _bwd on
the same tensors in the same run (the yardstick: the same bytes forward, x read as well backward), alternating, with the spread
over the repeats.  The first shape moves 649 MB forward and does not fit the 256 MiB cache; the last (162 MB forward) does, so its
rate is a cache rate, for both poolings alike.  Writes profiles/bench_avgpool.json (with the kernel source hash).  GPU only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402

PEAK_GBS = 8000.0          # the HBM peak DESIGN.md section 5.4 quotes its fractions against
SHAPES = ((256, 32, 88, 180), (256, 64, 44, 90), (256, 128, 22, 45))
ROUTES = {0: 'scalar', 2: 'one window, 8-byte', 4: 'two windows, 16-byte'}


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
    y = torch.empty((n, c, h // 2, w // 2), device='cuda')
    dy, dx = torch.randn_like(y), torch.empty_like(x)
    big, small = 4.0 * x.numel(), 4.0 * y.numel()
    cases = (('dlwp_avgpool2_fwd', lambda: ops.avgpool2(x, out=y), big + small),
             ('dlwp_maxpool2_fwd', lambda: ops.maxpool2(x, out=y), big + small),
             ('dlwp_avgpool2_bwd', lambda: ops.avgpool2_bwd(dy, shape, out=dx), small + big),
             ('dlwp_maxpool2_bwd', lambda: ops.maxpool2_bwd(x, dy), big + small + big))     # (allocates its dx from torch's cache)
    route = ROUTES[4 if w % 4 == 0 else (2 if w % 2 == 0 else 0)]
    rows = []
    for (name, fn, nbytes), (ms, spread) in zip(cases, timeit([cs[1] for cs in cases], iters, rounds)):
        rows.append({'kernel': name, 'shape': list(shape), 'route': route if 'avgpool' in name else None, 'us': 1e3 * ms,
                     'spread': spread, 'bytes': nbytes, 'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_avgpool.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_avgpool.py needs a GPU')
    rows = []
    for shape in SHAPES:
        rows += kernels(shape, args.iters, args.rounds)
    for r in rows:
        print('%-18s %-20s %-21s %9.1f us %7.0f GB/s %5.3f of peak  spread %4.1f %%' % (
            r['kernel'], 'x'.join(map(str, r['shape'])), r['route'] or '', r['us'], r['gbs'], r['of_peak'], 100 * r['spread']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds}, 'kernels': rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
