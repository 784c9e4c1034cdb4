#!/usr/bin/env python3
"""Conv2D(strides=2) and its padded space-to-depth pass on the MI355X (csrc/sconv.hip), with M = 8, 64 and 256 members on
32 x 88 x 180 and 64 x 44 x 90, without a halo, with the reference's wrap (columns) + zero (rows) halo of 2, and in the launch of
Conv2D(3, strides=2, 'same') itself (on 88 x 180 the 16-byte route; every other row is the element route):

  kernels  dlwp_space_to_depth2_pad and dlwp_space_to_depth2_pad_bwd in us, ALGORITHMIC GB/s (tensor in + tensor out) and share of
           the HBM peak, in the same alternating rounds as
             - dlwp_space_to_depth2_fill, the parent kernel: on the same bytes where there is no halo or only zeros below / right
               (it fills those itself), on the already padded tensor (the same output bytes) under the wrap halo -- the yardstick;
             - the launches the fused pass replaces: dlwp_pad2d_fwd + dlwp_space_to_depth2_fill, and for the adjoint
               dlwp_depth_to_space2_crop + dlwp_pad2d_bwd.
           HIP events around `iters` calls, `rounds` rounds that alternate over the kernels, the spread (max - min) / median over
           the rounds stated.  The rule of DESIGN.md 5.26: a gap is real above three run-to-run spreads.
  layers   Conv2D(32 -> 64, 3, strides=2, 'same', tanh): forward (predict_on_device) and a whole eager training step, beside
           Conv2D(32 -> 64, 3, 'same', tanh) + MaxPooling2D(2) on the same 88 x 180 map; the multiplies the stored 3 x 3 taps on
           4 cin channels spend against the layer's own k x k.

Writes profiles/bench_sconv.json (with the kernel source hash), prints the tables to stderr and ONE JSON line to stdout.  GPU only."""
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
SHAPES = ((32, 88, 180), (64, 44, 90))
MEMBERS = (8, 64, 256)
# (name, halo, modes (rows, columns), rows / columns of the phase tensor beyond the cover of the padded image)
HALOS = (('none', (0, 0, 0, 0), (0, 0), 0), ('wrap + zero halo of 2', (2, 2, 2, 2), (0, 1), 0),
         # what Conv2D(3, strides=2, 'same') itself launches: zeros (0, 1, 0, 1), 3 x 3 stored taps -> (h / 2 + 2) x (w / 2 + 2); on
         # 88 x 180 that is wp = 92: the 16-byte route of both directions (47 columns on 44 x 90: the element route)
         ("'same' zeros of k = 3, stored taps", (0, 1, 0, 1), (0, 0), 1))
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


# -- kernels ---------------------------------------------------------------------------------------------------------------------------- #
def kernels(members, c, h, w, halo, iters, rounds):
    name, pad, modes, extra = halo
    d = ops.make_pad(*pad, *modes)
    ph, pw = h + pad[0] + pad[1], w + pad[2] + pad[3]
    hp, wp = (ph + 1) // 2 + extra, (pw + 1) // 2 + extra
    x = torch.randn((members, c, h, w), device='cuda')
    p = torch.empty((members, 4 * c, hp, wp), device='cuda')
    g, dx = torch.randn_like(p), torch.empty_like(x)
    padded = torch.randn((members, c, ph, pw), device='cuda')
    dpadded = torch.empty_like(padded)
    nb = 4.0 * (x.numel() + p.numel())
    nb_padded = 4.0 * (padded.numel() + p.numel())

    def unfused_fwd():
        ops.pad2d(x, d, out=padded)
        ops.space_to_depth2_fill(padded, c, hp, wp, 0, 0, out=p)

    def unfused_bwd():
        ops.depth_to_space2_crop(g, c, 0, 0, ph, pw, out=dpadded)
        ops.pad2d_bwd(dpadded, (members, c, h, w), d)          # (allocates its result from torch's cache)
    cases = [('dlwp_space_to_depth2_pad', lambda: ops.space_to_depth2_pad(x, c, d, hp, wp, out=p), nb, 1),
             ('dlwp_space_to_depth2_pad_bwd', lambda: ops.space_to_depth2_pad_bwd(g, c, h, w, d, out=dx), nb, 1),
             ('dlwp_space_to_depth2_fill (parent)', lambda: ops.space_to_depth2_fill(padded, c, hp, wp, 0, 0, out=p), nb_padded, 1)]
    if extra:         # zeros below / right only: the parent kernel gives the same tensor from the unpadded source -- the same bytes
        cases[2] = ('dlwp_space_to_depth2_fill (parent)', lambda: ops.space_to_depth2_fill(x, c, hp, wp, 0, 0, out=p), nb, 1)
    elif any(pad):
        cases += [('dlwp_pad2d_fwd + dlwp_space_to_depth2_fill', unfused_fwd, nb, 2),
                  ('dlwp_depth_to_space2_crop + dlwp_pad2d_bwd', unfused_bwd, nb, 2)]
    rows = []
    for (kname, _, nbytes, nl), (ms, sp) in zip(cases, timeit([cs[1] for cs in cases], iters, rounds)):
        rows.append({'kernel': kname, 'halo': name, 'members': members, 'shape': [c, h, w], 'phase_shape': [4 * c, hp, wp],
                     'route': '16-byte' if (wp % 4 == 0 and pad[2] % 4 == 0 and w % 4 == 0) else 'element',
                     'launches': nl, 'us': 1e3 * ms, 'spread': sp, 'bytes': nbytes, 'gbs': nbytes / ms / 1e6,
                     'of_peak': nbytes / ms / 1e6 / PEAK_GBS})
    return rows


def verdict(rows):
    """per (members, shape, halo): the fused pass and its adjoint against the parent kernel, three-spreads rule"""
    out = []
    for i in range(len(rows)):
        r = rows[i]
        if r['kernel'] != 'dlwp_space_to_depth2_pad':
            continue
        bwd, parent = rows[i + 1], rows[i + 2]
        for k in (r, bwd):
            spread_us = max(k['spread'] * k['us'], parent['spread'] * parent['us'])
            out.append({'kernel': k['kernel'], 'halo': k['halo'], 'members': k['members'], 'shape': k['shape'], 'us': k['us'],
                        'parent_us': parent['us'], 'gbs': k['gbs'], 'parent_gbs': parent['gbs'], 'spread_us': spread_us,
                        'behind_parent_beyond_three_spreads': bool(k['us'] - parent['us'] > 3 * spread_us)})
    return out


# -- layers ----------------------------------------------------------------------------------------------------------------------------- #
def one_layer_model(kind, cin, f, h, w):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0 = L.Input(shape=(cin, h, w))
    if kind == 'conv3_strides2_same':
        out = L.Conv2D(f, 3, strides=2, padding='same', activation='tanh', **CF)(x0)
    else:
        out = L.MaxPooling2D(2, **CF)(L.Conv2D(f, 3, padding='same', activation='tanh', **CF)(x0))
    m = Model(inputs=x0, outputs=out, seed=1)
    m.compile(optimizer=Adam(lr=1e-4), loss='mse')
    return m


def layers(members, iters, rounds, cin=32, f=64, h=88, w=180):
    kinds = ('conv3_strides2_same', 'conv3_same + maxpool2')
    os.environ['DLWP_TRAIN_GRAPH'] = '0'              # the eager step: launch by launch, the same form for both
    rows = []
    try:
        nets = [one_layer_model(k, cin, f, h, w) for k in kinds]
        x = torch.randn((members, cin, h, w), device='cuda')
        y = torch.randn((members, f, h // 2, w // 2), device='cuda')
        fwd = timeit([lambda m=m: m.predict_on_device(x) for m in nets], iters, rounds)
        step = timeit([lambda m=m: m._need_trainer().train_on_shard(x, y, members, return_device=True) for m in nets],
                      max(3, iters // 3), rounds)
        for k, (kind, m) in enumerate(zip(kinds, nets)):
            conv = [op for op in m.plan.ops if op.kind == 'conv'][0]
            _, (sh, sw), _ = conv.conv_geometry
            rows.append({'layer': kind, 'members': members, 'cin': cin, 'filters': f, 'map': [h, w],
                         'fwd_us': 1e3 * fwd[k][0], 'fwd_spread': fwd[k][1], 'step_us': 1e3 * step[k][0],
                         'step_spread': step[k][1], 'inference_plan': [op.kind for op in m.infer_plan.ops],
                         'training_plan': [op.kind for op in m.plan.ops],
                         'multiplies_per_output_own': 9 * cin * f, 'multiplies_per_output_run': sh * sw * conv.xs[0] * f,
                         'outputs_per_sample': int(np.prod(conv.out_shape))})
    finally:
        del os.environ['DLWP_TRAIN_GRAPH']
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--layer-members', type=int, nargs='*', default=[8, 64])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_sconv.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sconv.py needs a GPU')
    krows = []
    for m in MEMBERS:
        for c, h, w in SHAPES:
            for halo in HALOS:
                krows += kernels(m, c, h, w, halo, args.iters, args.rounds)
                torch.cuda.empty_cache()
    for r in krows:
        log('%-46s %-22s M = %3d %-12s %9.1f us %7.0f GB/s %5.3f of peak  spread %4.1f %%' % (
            r['kernel'], r['halo'], r['members'], 'x'.join(map(str, r['shape'])), r['us'], r['gbs'], r['of_peak'], 100 * r['spread']))
    rule = verdict(krows)
    for v in rule:
        log('%-30s %-22s M = %3d %-12s %9.1f us, parent %9.1f us, spread %6.1f us%s' % (
            v['kernel'], v['halo'], v['members'], 'x'.join(map(str, v['shape'])), v['us'], v['parent_us'], v['spread_us'],
            '  BEHIND' if v['behind_parent_beyond_three_spreads'] else ''))
    lrows = []
    for m in args.layer_members:
        lrows += layers(m, args.iters, args.rounds)
        torch.cuda.empty_cache()
    for r in lrows:
        log('%-24s M = %3d  %3d -> %3d channels on %2d x %3d: forward %8.1f us (spread %4.1f %%), training step %8.1f us (spread '
            '%4.1f %%); %d multiplies per output run, %d its own' % (
                r['layer'], r['members'], r['cin'], r['filters'], r['map'][0], r['map'][1], r['fwd_us'], 100 * r['fwd_spread'],
                r['step_us'], 100 * r['step_spread'], r['multiplies_per_output_run'], r['multiplies_per_output_own']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds},
           'kernels': krows, 'against_parent_kernel': rule, 'layers': lrows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    log('wrote', args.out)
    behind = [v for v in rule if v['behind_parent_beyond_three_spreads']]
    print(json.dumps({'bench': 'sconv', 'kernel_cases': len(krows), 'behind_parent_beyond_three_spreads': len(behind),
                      'of': len(rule), 'worst_ratio_to_parent': max(v['us'] / v['parent_us'] for v in rule),
                      'layers': [{k: r[k] for k in ('layer', 'members', 'fwd_us', 'step_us')} for r in lrows], 'out': args.out}))


if __name__ == '__main__':
    main()
