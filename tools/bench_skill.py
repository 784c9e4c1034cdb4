#!/usr/bin/env python3
"""Latitude-weighted forecast skill on the MI355X (csrc/skill.hip): HIP-event time, GB/s (8 bytes read per pair: both operands once,
the climatology table not counted) and the fraction of the 8 TB/s HBM peak of dlwp_verify_skill_sums on the 56-lead x 256-sample
series of the 4 x 88 x 180 state -- both layouts of `valid`, with and without the latitude weights, with and without the 12-month
table, axis=None and per variable -- each beside dlwp_verify_error_sums on the same operands in the same run, alternating, with the
ratio of the two.  Then what a caller sees: the wall time of verify.forecast_skill on the resident series against the host path for
the same arrays, the download included.  Every timed step runs in a child process under its own time limit; a step that fails ends
the run.  Writes profiles/bench_skill.json (with the kernel source hash).  GPU only."""
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

PEAK_GBS = 8000.0
STATE = (4, 88, 180)
LEADS = 56
LAYOUTS = ('per_lead', 'plain_series')


def timeit(fns, iters, rounds):
    """[(median ms per call, (max - min) / median)] of every function: `rounds` rounds that ALTERNATE over the functions, each an
    event-bracketed run of `iters` calls, after a warm-up of every function"""
    import torch
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


def raw_skill(plan, t, table, labels, weights):
    """the C entry point on preallocated outputs: what the kernel pair costs, without the wrapper's checks, uploads and allocations"""
    import torch
    from dlwp_amd import _lib
    fc, ob = t[plan.fc], t[plan.ob]
    h = _lib.handle(fc.device.index)
    ws = torch.empty(_lib.lib.dlwp_verify_skill_workspace(h, plan.leads, plan.groups), dtype=torch.uint8, device=fc.device)
    sums = torch.empty((plan.leads, plan.groups, 10), dtype=torch.float64, device=fc.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    LL = ctypes.c_longlong
    ptr = lambda x: ctypes.c_void_p(0 if x is None else x.data_ptr())      # noqa: E731

    def fn():
        _lib.check(_lib.lib.dlwp_verify_skill_sums(
            h, ptr(fc), LL(plan.fc_strides[0]), LL(plan.fc_strides[1]), plan.fc_strides[2], ptr(ob), LL(plan.ob_strides[0]),
            LL(plan.ob_strides[1]), plan.ob_strides[2], plan.leads, plan.count0, plan.count_dec, plan.groups, LL(plan.run), ptr(table),
            0 if table is None else int(table.shape[0]), ptr(labels), LL(plan.label_strides[0]), plan.label_strides[1], ptr(weights),
            0 if weights is None else int(weights.numel()), LL(STATE[2]), ptr(sums), ptr(ws), ws.numel(), stream))
    return fn, sums, (fc, ob, ws)


def raw_error(plan, t):
    """dlwp_verify_error_sums on the same operands, strides and grid rule: the yardstick"""
    import torch
    from dlwp_amd import _lib
    fc, ob = t[plan.fc], t[plan.ob]
    h = _lib.handle(fc.device.index)
    ws = torch.empty(_lib.lib.dlwp_verify_error_workspace(h, plan.leads, plan.groups), dtype=torch.uint8, device=fc.device)
    sums = torch.empty((plan.leads, plan.groups, 3), dtype=torch.float64, device=fc.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    LL = ctypes.c_longlong

    def fn():
        _lib.check(_lib.lib.dlwp_verify_error_sums(
            h, fc.data_ptr(), LL(plan.fc_strides[0]), LL(plan.fc_strides[1]), plan.fc_strides[2], ob.data_ptr(), LL(plan.ob_strides[0]),
            LL(plan.ob_strides[1]), plan.ob_strides[2], plan.leads, plan.count0, plan.count_dec, plan.groups, LL(plan.run),
            sums.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return fn, sums, ws


def operands(layout, members):
    import torch
    forecast = torch.randn((LEADS, members) + STATE, device='cuda')
    valid = torch.randn((LEADS, members) + STATE, device='cuda')
    return forecast, (valid if layout == 'per_lead' else valid[0].contiguous())


def step_kernels(layout, members, iters, rounds):
    """one child process: the eight kernel cases of one layout"""
    import torch
    from dlwp_amd.model import verify
    forecast, valid = operands(layout, members)
    t = {'forecast': forecast, 'valid': valid}
    table = (0.5 * torch.randn((12,) + STATE, device='cuda')).contiguous()
    rng = np.random.default_rng(1)
    label_shape = (LEADS, members) if layout == 'per_lead' else (members,)
    labels = torch.from_numpy(rng.integers(0, 12, label_shape).astype(np.int32)).cuda()
    weights = torch.from_numpy(verify.area_weights(np.linspace(-87.0, 87.0, STATE[1]))).cuda()
    row = int(np.prod(STATE))
    out = []
    for per_variable in (False, True):
        axis = None if not per_variable else ((1, 3, 4) if layout == 'per_lead' else (0, 2, 3))
        plan = verify.plan_forecast_skill(forecast.shape, valid.shape, axis)
        pairs = sum(max(plan.count0 - f * plan.count_dec, 0) for f in range(LEADS))      # sample rows compared
        nbytes = 8.0 * pairs * row
        err_fn, err_sums, _keep_e = raw_error(plan, t)
        for use_w in (False, True):
            for use_c in (False, True):
                fn, sums, _keep = raw_skill(plan, t, table if use_c else None, labels if use_c else None, weights if use_w else None)
                (s_ms, s_sp), (e_ms, e_sp) = timeit([fn, err_fn], iters, rounds)
                if not use_w and not use_c:          # the same pairs: the counts agree with the yardstick's
                    assert torch.equal(sums[..., 9], err_sums[..., 2])
                out.append({'layout': layout, 'members': members, 'per_variable': per_variable, 'weights': use_w, 'climatology': use_c,
                            'pairs_of_rows': pairs, 'bytes': nbytes, 'skill_us': 1e3 * s_ms, 'skill_spread': s_sp,
                            'skill_gbs': nbytes / s_ms / 1e6, 'skill_of_peak': nbytes / s_ms / 1e6 / PEAK_GBS,
                            'error_sums_us': 1e3 * e_ms, 'error_sums_spread': e_sp, 'error_sums_gbs': nbytes / e_ms / 1e6,
                            'ratio_to_error_sums': s_ms / e_ms})
                r = out[-1]
                print('%-12s %s %s %s %6.0f MB: skill %8.1f us %5.0f GB/s %5.3f of peak (spread %4.1f %%) | error_sums %8.1f us '
                      '%5.0f GB/s | ratio %.3f' % (layout, 'per-var' if per_variable else 'all    ', 'w' if use_w else '-',
                                                   'c' if use_c else '-', nbytes / 1e6, r['skill_us'], r['skill_gbs'], r['skill_of_peak'],
                                                   100 * s_sp, r['error_sums_us'], r['error_sums_gbs'], r['ratio_to_error_sums']),
                      flush=True)
    return out


def step_wall(members, host_reps):
    """one child process: forecast_skill as a caller sees it, device against host (download included), weights and table given"""
    import torch
    from dlwp_amd.model import verify
    out = []
    for layout in LAYOUTS:
        forecast, valid = operands(layout, members)
        table = (0.5 * torch.randn((12,) + STATE, device='cuda')).contiguous()
        label_shape = (LEADS, members) if layout == 'per_lead' else (members,)
        labels = np.random.default_rng(2).integers(0, 12, label_shape).astype(np.int32)
        weights = verify.area_weights(np.linspace(-87.0, 87.0, STATE[1]))

        def wall(fn, reps):
            took = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                took.append(time.perf_counter() - t0)
            return float(np.median(took))
        verify.forecast_skill(forecast, valid, table, labels, weights)
        dev = wall(lambda: verify.forecast_skill(forecast, valid, table, labels, weights), 5)
        host = wall(lambda: verify.forecast_skill(forecast.cpu().numpy(), valid.cpu().numpy(), table.cpu().numpy(), labels, weights),
                    host_reps)
        out.append({'layout': layout, 'members': members, 'device_path_wall_ms': 1e3 * dev, 'host_path_wall_ms': 1e3 * host})
        print('%-12s %d members: forecast_skill wall: device %8.3f ms, host with the download %9.1f ms' % (layout, members, 1e3 * dev,
                                                                                                         1e3 * host), flush=True)
        del forecast, valid
        torch.cuda.empty_cache()
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_skill.py needs a GPU')
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_skill.json'))
    args = ap.parse_args()
    if args.step:
        return child(args)
    res = {'_meta': {'peak_gbs': PEAK_GBS, 'iters': args.iters, 'rounds': args.rounds, 'leads': LEADS, 'state': list(STATE),
                     'bytes_counted': 'both operands once, the table not', 'host_threads': os.cpu_count()}}
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
