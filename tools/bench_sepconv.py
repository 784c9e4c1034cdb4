#!/usr/bin/env python3
"""DepthwiseConv2D / SeparableConv2D on the MI355X (csrc/sepconv.hip) with M = 8, 64 and 256 members on the U-Net's maps and channel
counts (32 x 88 x 180, 64 x 44 x 90, 128 x 22 x 45):

  kernels  all six kernels in us, ALGORITHMIC GB/s (tensors in + tensor out; the weights are noise) and share of the HBM peak.
           The depthwise forward runs in the same alternating rounds as dlwp_avgpool2_fwd and dlwp_activation_fwd on the same input
           (the project's bandwidth yardsticks), and with a wrap (columns) + zero (rows) halo of 1 against dlwp_pad2d_fwd + itself
           unhaloed.  The pointwise forward, data gradient and weight gradient run beside the parent commit's route for the same
           product: dlwp_conv2d_fwd / _bwd_data / _bwd_weight with a 1 x 1 kernel on the same tensors.
           HIP events around `iters` calls, `rounds` rounds that alternate over the kernels, the spread (max - min) / median over the
           rounds stated.  The rule of DESIGN.md 5.26: a gap is real above three run-to-run spreads.
  layers   SeparableConv2D(64 -> 64, 3, 'same', tanh) forward (predict_on_device) and a whole eager training step beside Conv2D(64, 3)
           on the same 64 x 44 x 90 input; a U-Net (two levels, 32 / 64 channels on 4 x 88 x 180 states) with separable against dense
           3 x 3 layers: eager training step and a captured rollout of 14 days (56 six-hourly steps of a 2-step model = 28 calls).

Writes profiles/bench_sepconv.json (with the kernel source hash), prints the tables to stderr and ONE JSON line to stdout.  GPU only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402
from dlwp_amd import layers as L  # noqa: E402

PEAK_GBS = 8000.0          # the HBM peak DESIGN.md section 5.4 quotes its fractions against
SHAPES = ((32, 88, 180), (64, 44, 90), (128, 22, 45))
MEMBERS = (8, 64, 256)
CF = {'data_format': 'channels_first'}


def log(*a):
    print(*a, file=sys.stderr)


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


def rows_of(cases, members, shape, iters, rounds, **extra):
    out = []
    for (name, _, nbytes, nl), (ms, sp) in zip(cases, timeit([cs[1] for cs in cases], iters, rounds)):
        out.append(dict(kernel=name, members=members, shape=list(shape), launches=nl, us=1e3 * ms, spread=sp, bytes=nbytes,
                        gbs=nbytes / ms / 1e6, of_peak=nbytes / ms / 1e6 / PEAK_GBS, **extra))
    return out


# -- kernels ---------------------------------------------------------------------------------------------------------------------------- #
def depthwise_kernels(members, c, h, w, iters, rounds):
    x = torch.randn((members, c, h, w), device='cuda')
    k = torch.randn((3, 3, c, 1), device='cuda')
    b = torch.randn((c,), device='cuda')
    halo = ops.make_pad(1, 1, 1, 1, ops.PAD_ZERO, ops.PAD_WRAP)
    d0, d1 = ops.make_depthwise(3, 3), ops.make_depthwise(3, 3, halo=halo)
    y0 = torch.empty((members, c, h - 2, w - 2), device='cuda')
    y1, padded = torch.empty_like(x), torch.empty((members, c, h + 2, w + 2), device='cuda')
    g0, g1, dx, dk = torch.randn_like(y0), torch.randn_like(y1), torch.empty_like(x), torch.empty_like(k)
    pooled, act = torch.empty((members, c, h // 2, w // 2), device='cuda'), torch.empty_like(x)

    def unfused():
        ops.pad2d(x, halo, out=padded)
        ops.depthwise2d(padded, k, b, d0, out=y1)
    nb0, nb1 = 4.0 * (x.numel() + y0.numel()), 8.0 * x.numel()
    cases = [('dlwp_depthwise2d_fwd', lambda: ops.depthwise2d(x, k, b, d0, out=y0), nb0, 1),
             ('dlwp_avgpool2_fwd (yardstick)', lambda: ops.avgpool2(x, out=pooled), 4.0 * (x.numel() + pooled.numel()), 1),
             ('dlwp_activation_fwd (yardstick)', lambda: ops.activation_fwd(x, 'tanh', out=act), nb1, 1),
             ('dlwp_depthwise2d_fwd, wrap + zero halo of 1', lambda: ops.depthwise2d(x, k, b, d1, out=y1), nb1, 1),
             ('dlwp_pad2d_fwd + dlwp_depthwise2d_fwd', unfused, nb1, 2),
             ('dlwp_depthwise2d_bwd_data', lambda: ops.depthwise2d_bwd_data(g0, k, d0, h, w, out=dx), nb0, 1),
             ('dlwp_depthwise2d_bwd_data, wrap + zero halo of 1', lambda: ops.depthwise2d_bwd_data(g1, k, d1, h, w, out=dx), nb1, 1),
             ('dlwp_depthwise2d_bwd_weight', lambda: ops.depthwise2d_bwd_weight(x, g0, dk, d0), nb0, 2)]
    return rows_of(cases, members, (c, h, w), iters, rounds)


def pointwise_kernels(members, c, h, w, iters, rounds):
    """q = o = c: the pointwise stage of SeparableConv2D(c -> c) beside Conv2D(c, 1) on the same tensors"""
    x = torch.randn((members, c, h, w), device='cuda')
    p = torch.randn((1, 1, c, c), device='cuda')
    b = torch.randn((c,), device='cuda')
    y, g, dx, dp = torch.empty_like(x), torch.randn_like(x), torch.empty_like(x), torch.empty_like(p)
    d, cd = ops.make_pointwise(c, c), ops.make_conv(c, 1, 1)
    xs = _lib.Shape4(members, c, h, w)
    nb = 8.0 * x.numel()
    cases = [('dlwp_pointwise2d_fwd', lambda: ops.pointwise2d(x, p, b, d, out=y), nb, 1),
             ('dlwp_conv2d_fwd 1 x 1 (parent route)', lambda: ops.conv2d(x, p, b, cd, out=y), nb, 1),
             ('dlwp_pointwise2d_bwd_data', lambda: ops.pointwise2d_bwd_data(g, p, d, out=dx), nb, 1),
             ('dlwp_conv2d_bwd_data 1 x 1 (parent route)', lambda: ops.conv2d_bwd_data(g, p, cd, xs, dx), nb, 1),
             ('dlwp_pointwise2d_bwd_weight', lambda: ops.pointwise2d_bwd_weight(x, g, dp, d), nb, 2),
             ('dlwp_conv2d_bwd_weight 1 x 1 (parent route)', lambda: ops.conv2d_bwd_weight(x, g, dp, cd, xs), nb, 1)]
    kept, refused = [], {}
    for k, cs in enumerate(cases):          # a parent route without a kernel for this product is left out and named
        try:
            cs[1]()
            kept.append(cs)
        except _lib.DlwpError as e:
            refused[cases[k - 1][0]] = str(e)
    torch.cuda.synchronize()
    rows = rows_of(kept, members, (c, h, w), iters, rounds)
    for r in rows:
        if r['kernel'] in refused:
            r['parent_route_refused'] = refused[r['kernel']]
    return rows


def verdict(rows):
    """per (members, shape): each pointwise kernel against the parent route, three-spreads rule"""
    out = []
    for i, r in enumerate(rows):
        if not r['kernel'].startswith('dlwp_pointwise2d') or i + 1 >= len(rows) or 'parent route' not in rows[i + 1]['kernel']:
            continue
        parent = rows[i + 1]
        spread_us = max(r['spread'] * r['us'], parent['spread'] * parent['us'])
        out.append({'kernel': r['kernel'], 'members': r['members'], 'shape': r['shape'], 'us': r['us'], 'parent_us': parent['us'],
                    'spread_us': spread_us, 'ahead_of_parent_beyond_three_spreads': bool(parent['us'] - r['us'] > 3 * spread_us),
                    'behind_parent_beyond_three_spreads': bool(r['us'] - parent['us'] > 3 * spread_us)})
    return out


# -- layers ----------------------------------------------------------------------------------------------------------------------------- #
def one_layer_model(kind, cin, f, h, w):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0 = L.Input(shape=(cin, h, w))
    cls = L.SeparableConv2D if kind == 'separable' else L.Conv2D
    m = Model(inputs=x0, outputs=cls(f, 3, padding='same', activation='tanh', **CF)(x0), seed=1)
    m.compile(optimizer=Adam(lr=1e-4), loss='mse')
    return m


def unet(kind, c_in=4, h=88, w=180):
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    cls = L.SeparableConv2D if kind == 'separable' else L.Conv2D

    def conv(t, f, act='tanh'):
        t = L.ZeroPadding2D((1, 0), **CF)(PeriodicPadding2D((0, 1), **CF)(t))
        return cls(f, 3, activation=act, **CF)(t)
    x0 = L.Input(shape=(c_in, h, w))
    e1 = conv(x0, 32)
    e2 = conv(L.MaxPooling2D(2, **CF)(e1), 64)
    mid = conv(L.MaxPooling2D(2, **CF)(e2), 128)
    d2 = conv(L.concatenate([L.UpSampling2D(2, **CF)(mid), e2], axis=1), 64)
    d1 = conv(L.concatenate([L.UpSampling2D(2, **CF)(d2), e1], axis=1), 32)
    m = Model(inputs=x0, outputs=conv(d1, c_in, None), seed=1)
    m.compile(optimizer=Adam(lr=1e-4), loss='mse')
    return m


def layers(members, iters, rounds, c=64, h=44, w=90):
    kinds = ('separable', 'dense 3 x 3')
    os.environ['DLWP_TRAIN_GRAPH'] = '0'              # the eager step: launch by launch, the same form for both
    rows = []
    try:
        nets = [one_layer_model(k, c, c, h, w) for k in kinds]
        x, y = torch.randn((members, c, h, w), device='cuda'), torch.randn((members, c, h, w), device='cuda')
        fwd = timeit([lambda m=m: m.predict_on_device(x) for m in nets], iters, rounds)
        step = timeit([lambda m=m: m._need_trainer().train_on_shard(x, y, members, return_device=True) for m in nets],
                      max(3, iters // 3), rounds)
        for k, (kind, m) in enumerate(zip(kinds, nets)):
            rows.append({'layer': '%s 64 -> 64' % kind, 'members': members, 'map': [h, w], 'fwd_us': 1e3 * fwd[k][0],
                         'fwd_spread': fwd[k][1], 'step_us': 1e3 * step[k][0], 'step_spread': step[k][1],
                         'training_plan': [op.kind for op in m.plan.ops]})
        nets = [unet(k) for k in kinds]
        x, y = torch.randn((members, 4, 88, 180), device='cuda'), torch.randn((members, 4, 88, 180), device='cuda')
        step = timeit([lambda m=m: m._need_trainer().train_on_shard(x, y, members, return_device=True) for m in nets],
                      max(3, iters // 3), rounds)
        roll = timeit([lambda m=m: m.rollout_on_device(x, 28) for m in nets], max(2, iters // 5), rounds)
        for k, (kind, m) in enumerate(zip(kinds, nets)):
            rows.append({'layer': 'U-Net, %s layers' % kind, 'members': members, 'map': [88, 180], 'step_us': 1e3 * step[k][0],
                         'step_spread': step[k][1], 'rollout_14_days_us': 1e3 * roll[k][0], 'rollout_spread': roll[k][1],
                         'parameters': int(sum(int(np.prod(a.shape)) for a in m.get_weights())),
                         'launches': len(m.infer_plan.ops)})
    finally:
        del os.environ['DLWP_TRAIN_GRAPH']
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--layer-members', type=int, nargs='*', default=[8, 64])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_sepconv.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sepconv.py needs a GPU')
    krows = []
    for m in MEMBERS:
        for c, h, w in SHAPES:
            krows += depthwise_kernels(m, c, h, w, args.iters, args.rounds)
            krows += pointwise_kernels(m, c, h, w, args.iters, args.rounds)
            torch.cuda.empty_cache()
    for r in krows:
        log('%-50s M = %3d %-12s %9.1f us %7.0f GB/s %5.3f of peak  spread %4.1f %%' % (
            r['kernel'], r['members'], 'x'.join(map(str, r['shape'])), r['us'], r['gbs'], r['of_peak'], 100 * r['spread']))
    rule = verdict(krows)
    for v in rule:
        log('%-30s M = %3d %-12s %9.1f us, parent route %9.1f us, spread %6.1f us%s' % (
            v['kernel'], v['members'], 'x'.join(map(str, v['shape'])), v['us'], v['parent_us'], v['spread_us'],
            '  AHEAD' if v['ahead_of_parent_beyond_three_spreads'] else ('  BEHIND' if v['behind_parent_beyond_three_spreads'] else '')))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds},
           'kernels': krows, 'against_parent_route': rule, 'layers': []}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    save()                          # (the kernel rows are kept even where a layer row fails)
    for m in args.layer_members:
        res['layers'] += layers(m, args.iters, args.rounds)
        torch.cuda.empty_cache()
        save()
    for r in res['layers']:
        log(json.dumps(r))
    log('wrote', args.out)
    print(json.dumps({'bench': 'sepconv', 'kernel_cases': len(krows),
                      'pointwise_ahead_of_parent_beyond_three_spreads': sum(v['ahead_of_parent_beyond_three_spreads'] for v in rule),
                      'pointwise_behind_parent_beyond_three_spreads': sum(v['behind_parent_beyond_three_spreads'] for v in rule),
                      'of': len(rule), 'layers': [{k: r[k] for k in r if k.endswith('_us') or k in ('layer', 'members')}
                                                  for r in res['layers']], 'out': args.out}))


if __name__ == '__main__':
    main()
