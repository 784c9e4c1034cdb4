#!/usr/bin/env python3
"""Forecast verification on the MI355X (csrc/verify.hip): HIP-event time, GB/s (8 bytes read per pair) and the fraction of the 8 TB/s
HBM peak of dlwp_verify_error_sums on a 56-lead series of the 4 x 88 x 180 state with 8, 64 and 256 members, for both layouts of
`valid` (per lead: (F, N, ...); plain series: (N, ...), lead f compares valid[i + f]) -- beside dlwp_loss_metrics (mse + mae) on the
same number of bytes in the same run, alternating (the closest existing kernel: two operands, reduction only).  Then what a caller
sees: the wall time of verify.forecast_error on the resident series (launches, the download of the sums, the finish on the host)
against the host path for the same arrays, the download of the series included.  Writes profiles/bench_verify.json (with the kernel
source hash).  GPU only."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dlwp_amd import _lib, ops  # noqa: E402
from dlwp_amd.model import verify  # noqa: E402

PEAK_GBS = 8000.0
STATE = (4, 88, 180)
LEADS = 56
MEMBERS = (8, 64, 256)


def timeit(fns, iters, rounds):
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


def raw_verify(plan, t):
    """the C entry point on preallocated outputs: what the kernel pair costs, without the wrapper's allocations"""
    a, b = t[plan.a], t[plan.b]
    h = _lib.handle(a.device.index)
    ws = torch.empty(_lib.lib.dlwp_verify_error_workspace(h, plan.leads, plan.groups), dtype=torch.uint8, device=a.device)
    sums = torch.empty((plan.leads, plan.groups, 3), dtype=torch.float64, device=a.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    LL = ctypes.c_longlong

    def fn():
        _lib.check(_lib.lib.dlwp_verify_error_sums(h, a.data_ptr(), LL(plan.a_strides[0]), LL(plan.a_strides[1]), plan.a_strides[2],
                                                   b.data_ptr(), LL(plan.b_strides[0]), LL(plan.b_strides[1]), plan.b_strides[2],
                                                   plan.leads, plan.count0, plan.count_dec, plan.groups, LL(plan.run), sums.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), stream))
    return fn


def raw_metrics(x, y, rows):
    """dlwp_loss_metrics (mse + mae) on the first `rows` state rows of x and y: the same bytes as the verification call"""
    out = torch.empty(8, dtype=torch.float32, device=x.device)
    xs, ys = x.view(-1)[:rows * x[0, 0].numel()].view((rows,) + STATE), y.view(-1)[:rows * x[0, 0].numel()].view((rows,) + STATE)
    return lambda: ops.loss_metrics(xs, ys, out, (1 << _lib.LOSS_MSE) | (1 << _lib.LOSS_MAE), ws_key='bench_verify')


def wall(fn, reps):
    best = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        best.append(time.perf_counter() - t0)
    return float(np.median(best))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=1, help='repetitions of the host path (seconds each at 256 members)')
    ap.add_argument('--members', type=int, nargs='*', default=list(MEMBERS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_verify.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_verify.py needs a GPU')
    row = int(np.prod(STATE))
    rows = []
    for m in args.members:
        forecast = torch.randn((LEADS, m) + STATE, device='cuda')
        per_lead = torch.randn((LEADS, m) + STATE, device='cuda')
        for layout, valid in (('per_lead', per_lead), ('plain_series', per_lead[0])):
            plan = verify.plan_forecast(forecast.shape, valid.shape, None)
            pairs = sum(max(plan.count0 - f * plan.count_dec, 0) for f in range(LEADS))      # sample rows compared
            nbytes = 8.0 * pairs * row
            t = {'forecast': forecast, 'valid': valid}
            (v_ms, v_sp), (l_ms, l_sp) = timeit([raw_verify(plan, t), raw_metrics(forecast, per_lead, pairs)], args.iters, args.rounds)
            grouped = verify.plan_forecast(forecast.shape, valid.shape, (1, 3, 4) if layout == 'per_lead' else (0, 2, 3))
            (g_ms, g_sp), = timeit([raw_verify(grouped, t)], args.iters, args.rounds)
            dev_wall = wall(lambda: verify.forecast_error(forecast, valid), 5)
            # (numpy refuses a lead beyond a plain verification series, where the device reports NaN: the host gets the leads with
            #  pairs only -- the same rows the device reads)
            host_leads = LEADS if layout == 'per_lead' else min(LEADS, m)
            host_wall = wall(lambda: verify.forecast_error(forecast[:host_leads].cpu().numpy(), valid.cpu().numpy()), args.host_reps)
            rows.append({'members': m, 'layout': layout, 'pairs_of_rows': pairs, 'bytes': nbytes,
                         'verify_us': 1e3 * v_ms, 'verify_spread': v_sp, 'verify_gbs': nbytes / v_ms / 1e6,
                         'verify_of_peak': nbytes / v_ms / 1e6 / PEAK_GBS,
                         'verify_groups4_us': 1e3 * g_ms, 'verify_groups4_spread': g_sp, 'verify_groups4_gbs': nbytes / g_ms / 1e6,
                         'loss_metrics_us': 1e3 * l_ms, 'loss_metrics_spread': l_sp, 'loss_metrics_gbs': nbytes / l_ms / 1e6,
                         'loss_metrics_of_peak': nbytes / l_ms / 1e6 / PEAK_GBS,
                         'device_path_wall_ms': 1e3 * dev_wall, 'host_path_wall_ms': 1e3 * host_wall, 'host_path_leads': host_leads})
            r = rows[-1]
            print('%3d members %-12s %6.0f MB: verify %8.1f us %5.0f GB/s %5.3f of peak (spread %4.1f %%; 4 groups %8.1f us) | '
                  'loss_metrics %8.1f us %5.0f GB/s %5.3f | forecast_error wall: device %8.3f ms, host %9.1f ms' % (
                      m, layout, nbytes / 1e6, r['verify_us'], r['verify_gbs'], r['verify_of_peak'], 100 * v_sp, r['verify_groups4_us'],
                      r['loss_metrics_us'], r['loss_metrics_gbs'], r['loss_metrics_of_peak'], r['device_path_wall_ms'],
                      r['host_path_wall_ms']), flush=True)
        del forecast, per_lead
        torch.cuda.empty_cache()
    # climo_error's two launches at the largest size: the mean over samples, then the error pass against it
    m = max(args.members)
    valid = torch.randn((m,) + STATE, device='cuda')
    (n_ms, n_sp), = timeit([lambda: ops.verify_nanmean_samples(valid)], args.iters, args.rounds)
    climo = {'members': m, 'nanmean_us': 1e3 * n_ms, 'nanmean_spread': n_sp, 'nanmean_gbs': 4.0 * valid.numel() / n_ms / 1e6,
             'climo_error_wall_ms': 1e3 * wall(lambda: verify.climo_error(valid, LEADS), 5)}
    print('climo: nanmean over %d samples %.1f us (%.0f GB/s), climo_error(%d leads) wall %.3f ms' % (
        m, climo['nanmean_us'], climo['nanmean_gbs'], LEADS, climo['climo_error_wall_ms']))
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds, 'leads': LEADS, 'state': list(STATE), 'host_threads': os.cpu_count()},
           'forecast_error': rows, 'climo': climo}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
