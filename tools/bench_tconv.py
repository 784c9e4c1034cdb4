#!/usr/bin/env python3
"""Conv2DTranspose(strides=2) and its cropping interleave on the MI355X (csrc/tconv.hip), at the U-Net's two decoder steps --
128 -> 64 channels, 22 x 45 -> 44 x 90, and 64 -> 32 channels, 44 x 90 -> 88 x 180 -- with M = 8, 64 and 256 members:

  layers   the forward (predict_on_device) and a whole training step (forward + 'mse' + backward + Adam, the eager step) of a
           one-layer model: Conv2DTranspose(k = 2), Conv2DTranspose(k = 4, 'same') and the reference U-Net's layer at the same place,
           UpSampling2D(2) -> periodic / zero padding -> Conv2D(3) (dilation 1 at the first step, 2 at the second), alternating in
           one run; HIP-event time in us and the spread over the rounds;
  kernels  dlwp_depth_to_space2_crop / dlwp_space_to_depth2_fill in us and ALGORITHMIC GB/s (tensor in + tensor out) next to
           dlwp_depth_to_space2 / dlwp_space_to_depth2 on the same bytes (nothing cropped), and -- on the phase tensors of k = 4,
           'same' (a crop of one row and column on every side) -- next to the TWO launches they replace: interleave +
           dlwp_pad2d_bwd, dlwp_pad2d_fwd + inverse interleave.  The rule of DESIGN.md 5.26: a gap is real above three
           run-to-run spreads; the fused kernels stay only if they are not slower than the two launches;
  models   the config-3 training step and the 28-call rollout of the U-Net with transposed decoders (each UpSampling2D + padding +
           Conv2D(3) replaced by Conv2DTranspose(filters, 2, tanh)) against the nearest decoders.

Writes profiles/bench_tconv.json (with the kernel source hash).  GPU only."""
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
from dlwp_amd.presets import unet_layers  # noqa: E402

PEAK_GBS = 8000.0          # the HBM peak DESIGN.md section 5.4 quotes its fractions against
STEPS = ((128, 64, 22, 45, 1), (64, 32, 44, 90, 2))       # cin, filters, h, w, dilation of the reference layer's Conv2D(3)
MEMBERS = (8, 64, 256)
CF = {'data_format': 'channels_first'}


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


# -- layers ----------------------------------------------------------------------------------------------------------------------------- #
def one_layer_model(kind, cin, f, h, w, dil):
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0 = L.Input(shape=(cin, h, w))
    if kind == 'tconv_k2':
        out = L.Conv2DTranspose(f, 2, activation='tanh', **CF)(x0)
    elif kind == 'tconv_k4_same':
        out = L.Conv2DTranspose(f, 4, padding='same', activation='tanh', **CF)(x0)
    else:                    # the reference U-Net's decoder layer (dlwp_amd.presets._block behind an UpSampling2D)
        t = L.ZeroPadding2D((dil, 0), **CF)(PeriodicPadding2D((0, dil), **CF)(L.UpSampling2D(2, **CF)(x0)))
        out = L.Conv2D(f, 3, dilation_rate=dil, activation='tanh', **CF)(t)
    m = Model(inputs=x0, outputs=out, seed=1)
    m.compile(optimizer=Adam(lr=1e-4), loss='mse')
    return m


def layers(members, iters, rounds):
    rows = []
    kinds = ('tconv_k2', 'tconv_k4_same', 'upsample_pad_conv3')
    os.environ['DLWP_TRAIN_GRAPH'] = '0'              # the eager step: launch by launch, the same form for the three layers
    try:
        for cin, f, h, w, dil in STEPS:
            nets = [one_layer_model(k, cin, f, h, w, dil) for k in kinds]
            # k = 2 with the ONE tap it needs instead of 3 x 3 stored taps (DLWP_TCONV_TAPS=exact: a 1 x 1 convolution on the
            # library's direct kernel; it has no weight gradient, so only the forward is timed)
            os.environ['DLWP_TCONV_TAPS'] = 'exact'
            try:
                exact = one_layer_model('tconv_k2', cin, f, h, w, dil)
                assert exact.infer_plan.ops[1].conv_geometry[1] == (1, 1)
            finally:
                del os.environ['DLWP_TCONV_TAPS']
            x = torch.randn((members, cin, h, w), device='cuda')
            y = torch.randn((members, f, 2 * h, 2 * w), device='cuda')
            fwd = timeit([lambda m=m: m.predict_on_device(x) for m in nets + [exact]], iters, rounds)
            step = timeit([lambda m=m: m._need_trainer().train_on_shard(x, y, members, return_device=True) for m in nets],
                          max(3, iters // 3), rounds)
            for k, (kind, m) in enumerate(zip(kinds, nets)):
                rows.append({'layer': kind, 'members': members, 'cin': cin, 'filters': f, 'map': [h, w],
                             'fwd_us': 1e3 * fwd[k][0], 'fwd_spread': fwd[k][1], 'step_us': 1e3 * step[k][0],
                             'step_spread': step[k][1], 'inference_plan': [op.kind for op in m.infer_plan.ops],
                             'training_plan': [op.kind for op in m.plan.ops]})
            rows.append({'layer': 'tconv_k2, one stored tap', 'members': members, 'cin': cin, 'filters': f, 'map': [h, w],
                         'fwd_us': 1e3 * fwd[3][0], 'fwd_spread': fwd[3][1], 'step_us': None, 'step_spread': None,
                         'inference_plan': [op.kind for op in exact.infer_plan.ops], 'training_plan': None})
            del nets, exact
            torch.cuda.empty_cache()
    finally:
        del os.environ['DLWP_TRAIN_GRAPH']
    return rows


# -- kernels ---------------------------------------------------------------------------------------------------------------------------- #
def row(name, what, shape, ms, spread, nbytes, launches=1):
    return {'kernel': name, 'case': what, 'phase_shape': list(shape), 'launches': launches, 'us': 1e3 * ms, 'spread': spread,
            'bytes': nbytes, 'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS}


def interleaves(members, f, h, w, iters, rounds):
    rows = []
    # nothing cropped (k = 2): the phase tensor of the layer's input map, against the plain interleaves on the same bytes
    ph = torch.randn((members, 4 * f, h, w), device='cuda')
    y = torch.empty((members, f, 2 * h, 2 * w), device='cuda')
    dy, dph = torch.randn_like(y), torch.empty_like(ph)
    nb = 4.0 * (ph.numel() + y.numel())
    cases = (('dlwp_depth_to_space2_crop', lambda: ops.depth_to_space2_crop(ph, f, 0, 0, 2 * h, 2 * w, out=y)),
             ('dlwp_depth_to_space2', lambda: ops.depth_to_space2(ph, f, out=y)),
             ('dlwp_space_to_depth2_fill', lambda: ops.space_to_depth2_fill(dy, f, h, w, 0, 0, out=dph)),
             ('dlwp_space_to_depth2', lambda: ops.space_to_depth2(dy, f)))           # (allocates its result from torch's cache)
    for (name, _), (ms, sp) in zip(cases, timeit([c[1] for c in cases], iters, rounds)):
        rows.append(row(name, 'no crop', ph.shape, ms, sp, nb))
    # k = 4, 'same': the phase map is one row and column larger, one row / column is cropped on every side
    hp, wp = h + 1, w + 1
    ph = torch.randn((members, 4 * f, hp, wp), device='cuda')
    whole = torch.empty((members, f, 2 * hp, 2 * wp), device='cuda')
    dph = torch.empty_like(ph)
    crop = ops.make_pad(1, 1, 1, 1)
    nb = 4.0 * (ph.numel() + y.numel())

    def two_fwd():
        ops.depth_to_space2(ph, f, out=whole)
        ops.crop2d(whole, crop, out=y)

    def two_bwd():
        ops.pad2d(dy, crop, out=whole)
        ops.space_to_depth2(whole, f)
    cases = (('dlwp_depth_to_space2_crop', lambda: ops.depth_to_space2_crop(ph, f, 1, 1, 2 * h, 2 * w, out=y), 1),
             ('dlwp_depth_to_space2 + dlwp_pad2d_bwd', two_fwd, 2),
             ('dlwp_space_to_depth2_fill', lambda: ops.space_to_depth2_fill(dy, f, hp, wp, 1, 1, out=dph), 1),
             ('dlwp_pad2d_fwd + dlwp_space_to_depth2', two_bwd, 2))
    for (name, _, nl), (ms, sp) in zip(cases, timeit([c[1] for c in cases], iters, rounds)):
        rows.append(row(name, "crop (1, 1) of k = 4, 'same'", ph.shape, ms, sp, nb, nl))
    return rows


def verdict(rows):
    """the rule about the fused interleave, over every cropped case: slower than the two launches by more than three spreads?"""
    out = []
    for i in range(0, len(rows)):
        r = rows[i]
        if r['launches'] != 1 or not r['case'].startswith('crop'):
            continue
        two = rows[i + 1]
        spread_us = max(r['spread'] * r['us'], two['spread'] * two['us'])
        out.append({'kernel': r['kernel'], 'phase_shape': r['phase_shape'], 'fused_us': r['us'], 'two_launch_us': two['us'],
                    'spread_us': spread_us, 'fused_slower_beyond_three_spreads': bool(r['us'] - two['us'] > 3 * spread_us)})
    return out


# -- models ----------------------------------------------------------------------------------------------------------------------------- #
def transposed_unet_layers(cs):
    """the U-Net of dlwp_amd.presets with every UpSampling2D + padding + Conv2D(3, tanh) replaced by Conv2DTranspose(filters, 2, tanh)"""
    src = list(unet_layers(cs))
    out, i = [], 0
    while i < len(src):
        if src[i][0] == 'UpSampling2D':
            conv = src[i + 3]
            out.append(('Conv2DTranspose', (conv[1][0], 2), dict(CF, strides=2, activation=conv[2]['activation'])))
            i += 4
        else:
            out.append(src[i])
            i += 1
    return tuple(out)


def build(kind):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    specs = unet_layers((4, 88, 180)) if kind == 'nearest' else transposed_unet_layers((4, 88, 180))
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(specs, loss='mse', optimizer=Adam(lr=1e-4), metrics=['mae'])
    return d


def model_costs(n, steps, warmup, calls):
    """nearest and transposed U-Net, alternating: the training step, then the rollout"""
    kinds = ('nearest', 'transposed')
    nets = [build(k) for k in kinds]
    x = torch.randn((n, 4, 88, 180), device='cuda')
    y = torch.randn_like(x)
    for d in nets:
        for _ in range(warmup):                    # (the step is recorded and replayed from its third call on)
            d.model._trainer.train_on_shard(x, y, n, return_device=True)
        d.model.rollout_on_device(x, calls)
    step = timeit([lambda d=d: d.model._trainer.train_on_shard(x, y, n, return_device=True) for d in nets], steps, rounds=5)
    roll = timeit([lambda d=d: d.model.rollout_on_device(x, calls) for d in nets], 3, rounds=5)
    return [{'decoders': kind, 'samples': n, 'parameters': int(d.model.count_params()), 'step_ms': step[k][0],
             'step_spread': step[k][1], 'step_form': str(d.model._trainer._graph_ok(n)),
             'launches_training_plan': len(d.model.plan.ops), 'launches_inference_plan': len(d.model.infer_plan.ops),
             'rollout_calls': calls, 'rollout_ms': roll[k][0], 'rollout_spread': roll[k][1],
             'rollout_steps_per_s': n * calls * 2 / (roll[k][0] * 1e-3)}
            for k, (kind, d) in enumerate(zip(kinds, nets))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--members', type=int, default=64, help='samples of the training step and members of the rollout')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=28, help='model calls of the rollout (28 = 14 days of 2 x 6 h)')
    ap.add_argument('--skip-models', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_tconv.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_tconv.py needs a GPU')
    krows = []
    for m in MEMBERS:
        for cin, f, h, w, _ in STEPS:
            krows += interleaves(m, f, h, w, args.iters, args.rounds)
            torch.cuda.empty_cache()
    for r in krows:
        print('%-40s %-30s %-20s %8.1f us %7.0f GB/s %5.3f of peak  spread %4.1f %%' % (
            r['kernel'], r['case'], 'x'.join(map(str, r['phase_shape'])), r['us'], r['gbs'], r['of_peak'], 100 * r['spread']))
    rule = verdict(krows)
    keep = not any(v['fused_slower_beyond_three_spreads'] for v in rule)
    for v in rule:
        print('%-28s %-20s fused %8.1f us, two launches %8.1f us, spread %6.1f us%s' % (
            v['kernel'], 'x'.join(map(str, v['phase_shape'])), v['fused_us'], v['two_launch_us'], v['spread_us'],
            '  SLOWER' if v['fused_slower_beyond_three_spreads'] else ''))
    print('the fused interleave %s' % ('stays' if keep else 'is slower than the two launches it replaces'))
    lrows = []
    for m in MEMBERS:
        lrows += layers(m, args.iters, args.rounds)
    for r in lrows:
        print('%-26s M = %3d  %3d -> %3d channels on %2d x %2d: forward %8.1f us (spread %4.1f %%)' % (
            r['layer'], r['members'], r['cin'], r['filters'], r['map'][0], r['map'][1], r['fwd_us'], 100 * r['fwd_spread']) +
              (', training step %8.1f us (spread %4.1f %%)' % (r['step_us'], 100 * r['step_spread']) if r['step_us'] else ''))
    models = [] if args.skip_models else model_costs(args.members, args.steps, args.warmup, args.calls)
    for m in models:
        print('U-Net, %-10s decoders (%d parameters): step of %d samples %.3f ms (%s, %d launches planned, spread %.1f %%); rollout '
              'of %d calls %.3f ms = %.0f steps/s (%d launches per call, spread %.1f %%)' % (
                  m['decoders'], m['parameters'], m['samples'], m['step_ms'], m['step_form'], m['launches_training_plan'],
                  100 * m['step_spread'], m['rollout_calls'], m['rollout_ms'], m['rollout_steps_per_s'],
                  m['launches_inference_plan'], 100 * m['rollout_spread']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds},
           'kernels': krows, 'fused_interleave_rule': rule, 'fused_interleave_stays': keep, 'layers': lrows, 'models': models}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
