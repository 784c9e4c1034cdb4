#!/usr/bin/env python3
"""Per-grid-point forecast skill on the MI355X (csrc/skill_map.hip): HIP-event time, GB/s (8 bytes read per pair: both operands once,
the climatology table and the maps written not counted) and the fraction of the 8 TB/s HBM peak of dlwp_verify_skill_map on the
56-lead x 256-sample series of the 4 x 88 x 180 state -- both layouts of `valid`, with and without the 12-month table, scores only and
sums + scores -- each beside dlwp_verify_skill_sums (no weights, one group) on the same operands in the same run, alternating, with the
ratio of the two: the yardstick reads the same 8 bytes per pair.  Then what a caller sees: the wall time of verify.forecast_skill_map
on the resident series (the maps stay on the device) against the host path for the same arrays, the download included.  Every timed
step runs in a child process under its own time limit; a step that fails ends the run.  Writes profiles/bench_skill_map.json (with the
kernel source hash).  GPU only."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_skill import LAYOUTS, LEADS, PEAK_GBS, STATE, operands, raw_skill, timeit  # noqa: E402


def raw_map(plan, t, table, labels, with_sums):
    """the C entry point on preallocated outputs: what the launch costs, without the wrapper's checks, uploads and allocations"""
    import torch
    from dlwp_amd import _lib
    fc, ob = t[plan.fc], t[plan.ob]
    h = _lib.handle(fc.device.index)
    row = plan.run
    ws = torch.empty(max(_lib.lib.dlwp_verify_skill_map_workspace(h, plan.leads, plan.count0, row, 0), 8), dtype=torch.uint8,
                     device=fc.device)
    sums = torch.empty((plan.leads, 9, row), dtype=torch.float64, device=fc.device) if with_sums else None
    scores = torch.empty((plan.leads, 6, row), dtype=torch.float32, device=fc.device)
    counts = torch.empty((plan.leads, row), dtype=torch.int32, device=fc.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    LL = ctypes.c_longlong
    ptr = lambda x: ctypes.c_void_p(0 if x is None else x.data_ptr())      # noqa: E731

    def fn():
        _lib.check(_lib.lib.dlwp_verify_skill_map(
            h, ptr(fc), LL(plan.fc_strides[0]), LL(plan.fc_strides[1]), plan.fc_strides[2], ptr(ob), LL(plan.ob_strides[0]),
            LL(plan.ob_strides[1]), plan.ob_strides[2], plan.leads, plan.count0, plan.count_dec, LL(row), ptr(table),
            0 if table is None else int(table.shape[0]), ptr(labels), LL(plan.label_strides[0]), plan.label_strides[1], 0, ptr(sums),
            ptr(scores), ptr(counts), ptr(ws), ws.numel(), stream))
    return fn, counts, (fc, ob, ws, sums, scores)


def step_kernels(layout, members, iters, rounds):
    """one child process: the four kernel cases of one layout"""
    import torch
    from dlwp_amd.model import verify
    forecast, valid = operands(layout, members)
    t = {'forecast': forecast, 'valid': valid}
    table = (0.5 * torch.randn((12,) + STATE, device='cuda')).contiguous()
    rng = np.random.default_rng(1)
    label_shape = (LEADS, members) if layout == 'per_lead' else (members,)
    labels = torch.from_numpy(rng.integers(0, 12, label_shape).astype(np.int32)).cuda()
    row = int(np.prod(STATE))
    plan = verify.plan_forecast_skill(forecast.shape, valid.shape, None)
    pairs = sum(max(plan.count0 - f * plan.count_dec, 0) for f in range(LEADS))      # sample rows compared
    nbytes = 8.0 * pairs * row
    written = {False: LEADS * row * 28.0, True: LEADS * row * 100.0}
    out = []
    for use_c in (False, True):
        yard_fn, yard_sums, _keep_y = raw_skill(plan, t, table if use_c else None, labels if use_c else None, None)
        for with_sums in (False, True):
            fn, counts, _keep = raw_map(plan, t, table if use_c else None, labels if use_c else None, with_sums)
            (m_ms, m_sp), (y_ms, y_sp) = timeit([fn, yard_fn], iters, rounds)
            assert counts.sum().item() == int(yard_sums[..., 9].sum().item())      # the same pairs
            out.append({'layout': layout, 'members': members, 'climatology': use_c, 'sums': with_sums, 'pairs_of_rows': pairs,
                        'bytes': nbytes, 'bytes_written': written[with_sums], 'map_us': 1e3 * m_ms, 'map_spread': m_sp,
                        'map_gbs': nbytes / m_ms / 1e6, 'map_of_peak': nbytes / m_ms / 1e6 / PEAK_GBS, 'skill_sums_us': 1e3 * y_ms,
                        'skill_sums_spread': y_sp, 'skill_sums_gbs': nbytes / y_ms / 1e6, 'ratio_to_skill_sums': m_ms / y_ms})
            r = out[-1]
            print('%-12s %s %s %6.0f MB: map %8.1f us %5.0f GB/s %5.3f of peak (spread %4.1f %%) | skill_sums %8.1f us %5.0f GB/s | '
                  'ratio %.3f' % (layout, 'c' if use_c else '-', 'sums+scores' if with_sums else 'scores     ', nbytes / 1e6, r['map_us'],
                                  r['map_gbs'], r['map_of_peak'], 100 * m_sp, r['skill_sums_us'], r['skill_sums_gbs'],
                                  r['ratio_to_skill_sums']), flush=True)
    return out


def step_wall(members, host_reps):
    """one child process: forecast_skill_map as a caller sees it, device (maps left in HBM, and downloaded) against host (download of
    the series included), with the 12-month table"""
    import torch
    from dlwp_amd.model import verify
    out = []
    for layout in LAYOUTS:
        forecast, valid = operands(layout, members)
        table = (0.5 * torch.randn((12,) + STATE, device='cuda')).contiguous()
        label_shape = (LEADS, members) if layout == 'per_lead' else (members,)
        labels = np.random.default_rng(2).integers(0, 12, label_shape).astype(np.int32)

        def wall(fn, reps):
            took = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                took.append(time.perf_counter() - t0)
            return float(np.median(took))
        verify.forecast_skill_map(forecast, valid, table, labels)
        dev = wall(lambda: verify.forecast_skill_map(forecast, valid, table, labels), 5)
        down = wall(lambda: [v.cpu() for v in verify.forecast_skill_map(forecast, valid, table, labels)], 5)
        host = wall(lambda: verify.forecast_skill_map(forecast.cpu().numpy(), valid.cpu().numpy(), table.cpu().numpy(), labels),
                    host_reps)
        out.append({'layout': layout, 'members': members, 'device_path_wall_ms': 1e3 * dev, 'device_path_with_maps_downloaded_ms': 1e3 * down,
                    'host_path_wall_ms': 1e3 * host})
        print('%-12s %d members: forecast_skill_map wall: device %8.3f ms, with the maps downloaded %8.3f ms, host with the download of '
              'the series %9.1f ms' % (layout, members, 1e3 * dev, 1e3 * down, 1e3 * host), flush=True)
        del forecast, valid
        torch.cuda.empty_cache()
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_skill_map.py needs a GPU')
    if args.step == 'wall':
        res = step_wall(args.wall_members, args.host_reps)
    else:
        res = step_kernels(args.step, args.members, args.iters, args.rounds)
    from dlwp_amd import _lib
    print('RESULT ' + json.dumps({'rows': res, 'source_sha': _lib.kernel_source_hash(), 'device': torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--members', type=int, default=256)
    ap.add_argument('--wall-members', type=int, default=64, help='samples of the wall-time comparison (the host path takes seconds)')
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds each child process may take')
    ap.add_argument('--step', choices=LAYOUTS + ('wall',), help='(internal) run one step in this process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_skill_map.json'))
    args = ap.parse_args()
    if args.step:
        return child(args)
    res = {'_meta': {'peak_gbs': PEAK_GBS, 'iters': args.iters, 'rounds': args.rounds, 'leads': LEADS, 'state': list(STATE),
                     'bytes_counted': 'both operands once; the table and the maps written are not',
                     'yardstick': 'dlwp_verify_skill_sums, no weights, one group, the same table', 'host_threads': os.cpu_count()}}
    for step in LAYOUTS + ('wall',):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--iters', str(args.iters), '--rounds', str(args.rounds),
               '--members', str(args.members), '--wall-members', str(args.wall_members), '--host-reps', str(args.host_reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit('step %s ran into its time limit of %d s: nothing further is started' % (step, args.step_timeout))
        lines = p.stdout.splitlines()
        print('\n'.join(ln for ln in lines if not ln.startswith('RESULT ')), flush=True)
        if p.returncode != 0:
            raise SystemExit('step %s ended with status %d: nothing further is started' % (step, p.returncode))
        got = json.loads([ln for ln in lines if ln.startswith('RESULT ')][-1][len('RESULT '):])
        res['_meta'].update(source_sha=got['source_sha'], device=got['device'])
        res['wall' if step == 'wall' else step] = got['rows']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
