#!/usr/bin/env python3
"""Ensemble verification on the MI355X (csrc/ensemble.hip): HIP-event time, GB/s and the fraction of the 8 TB/s HBM peak of
dlwp_ens_mean_spread and dlwp_ens_score_sums on the benchmark's 56-lead series of the 4 x 88 x 180 state with 256 rows per lead, read
as (samples, members) = (1, 256), (8, 32) and (32, 8) in both member layouts -- beside dlwp_verify_error_sums on the same bytes in
the same run, alternating (the two halves of every lead as its two operands: the yardstick for "the achievable HBM rate" of a
reduction here).  Then what a caller sees: the wall time of ensemble.ensemble_scores on the resident series (launches, the download
of the sums and the histogram, the finish on the host) against the host path for the same arrays, the download of the series
included.  The host path takes seconds per lead, so both are timed on the first --host-leads leads (the device path on all 56 too).
Writes profiles/bench_ensemble.json (with the kernel source hash).  GPU only."""
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
from dlwp_amd.model import ensemble  # noqa: E402

PEAK_GBS = 8000.0
STATE = (4, 88, 180)
LEADS = 56
ROWS = 256                                   # sample rows per lead: samples x members
POINTS = ((1, 256), (8, 32), (32, 8))
LL = ctypes.c_longlong


def timeit(fns, iters, rounds):
    """[(median ms per call, (max - min) / median)] of every function: `rounds` rounds that ALTERNATE over the functions, each an
    event-bracketed run of `iters` calls, after a warm-up of every function"""
    for fn in fns:
        for _ in range(2):
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


def raw_mean_spread(x, st, samples, members, row):
    """the C entry points on preallocated outputs: what the kernels cost, without the wrapper's allocations"""
    h = _lib.handle(x.device.index)
    mean = torch.empty((LEADS, samples, row), dtype=torch.float32, device=x.device)
    spread = torch.empty_like(mean)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(_lib.lib.dlwp_ens_mean_spread(h, x.data_ptr(), LEADS, samples, members, LL(st[0]), LL(st[1]), LL(st[2]),
                                                            LL(row), 1, mean.data_ptr(), spread.data_ptr(), stream))


def raw_scores(x, st, y, samples, members, row, field):
    h = _lib.handle(x.device.index)
    ws = torch.empty(_lib.lib.dlwp_ens_score_workspace(h, LEADS, 1, members), dtype=torch.uint8, device=x.device)
    sums = torch.empty((LEADS, 1, 6), dtype=torch.float64, device=x.device)
    hist = torch.empty((LEADS, 1, members + 1), dtype=torch.int64, device=x.device)
    crps = torch.empty((LEADS, samples, row), dtype=torch.float32, device=x.device) if field else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(_lib.lib.dlwp_ens_score_sums(h, x.data_ptr(), LL(st[0]), LL(st[1]), LL(st[2]), y.data_ptr(), LEADS, samples,
                                                           members, 1, LL(row), sums.data_ptr(), hist.data_ptr(),
                                                           crps.data_ptr() if field else None, ws.data_ptr(), ws.numel(), stream))


def raw_verify_same_bytes(x, row):
    """dlwp_verify_error_sums over the series' own bytes: rows 0 .. 127 of every lead against rows 128 .. 255"""
    half = ROWS // 2
    a, b = x.view(-1), x.view(-1)[half * row:]
    h = _lib.handle(x.device.index)
    ws = torch.empty(_lib.lib.dlwp_verify_error_workspace(h, LEADS, 1), dtype=torch.uint8, device=x.device)
    sums = torch.empty((LEADS, 1, 3), dtype=torch.float64, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(_lib.lib.dlwp_verify_error_sums(h, a.data_ptr(), LL(ROWS * row), LL(row), 0, b.data_ptr(), LL(ROWS * row),
                                                              LL(row), 0, LEADS, half, 0, 1, LL(row), sums.data_ptr(), ws.data_ptr(),
                                                              ws.numel(), stream))


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
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-leads', type=int, default=4, help='leads the host path is timed on (seconds per lead)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_ensemble.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ensemble.py needs a GPU')
    row = int(np.prod(STATE))
    base = torch.randn((LEADS, 1) + STATE, device='cuda')
    series = base + 0.05 * torch.randn((LEADS, ROWS) + STATE, device='cuda')      # every row of a lead: one state + a perturbation
    x_bytes = 4.0 * series.numel()
    hl = max(1, min(args.host_leads, LEADS))
    rows = []
    for samples, members in POINTS:
        valid = (base + 0.05 * torch.randn((LEADS, samples) + STATE, device='cuda')).contiguous()
        for member_axis in (2, 1):
            st = ops.ens_strides(samples, members, row, member_axis)
            shape = (LEADS, samples, members) + STATE if member_axis == 2 else (LEADS, members, samples) + STATE
            view = series.view(shape)
            fns = [raw_mean_spread(series, st, samples, members, row), raw_scores(series, st, valid, samples, members, row, False),
                   raw_scores(series, st, valid, samples, members, row, True), raw_verify_same_bytes(series, row)]
            (m_ms, m_sp), (s_ms, s_sp), (f_ms, f_sp), (v_ms, v_sp) = timeit(fns, args.iters, args.rounds)
            out_bytes = 4.0 * LEADS * samples * row
            m_bytes, s_bytes, f_bytes = x_bytes + 2 * out_bytes, x_bytes + out_bytes, x_bytes + 2 * out_bytes
            dev_wall = wall(lambda: ensemble.ensemble_scores(view, valid, member_axis=member_axis), 5)
            dev_wall_hl = wall(lambda: ensemble.ensemble_scores(view[:hl], valid[:hl], member_axis=member_axis), 5)
            host_wall = wall(lambda: ensemble.ensemble_scores(view[:hl].cpu().numpy(), valid[:hl].cpu().numpy(), member_axis=member_axis), 1)
            r = {'samples': samples, 'members': members, 'member_axis': member_axis, 'series_bytes': x_bytes,
                 'mean_spread_us': 1e3 * m_ms, 'mean_spread_spread': m_sp, 'mean_spread_gbs': m_bytes / m_ms / 1e6,
                 'mean_spread_of_peak': m_bytes / m_ms / 1e6 / PEAK_GBS,
                 'score_sums_us': 1e3 * s_ms, 'score_sums_spread': s_sp, 'score_sums_gbs': s_bytes / s_ms / 1e6,
                 'score_sums_of_peak': s_bytes / s_ms / 1e6 / PEAK_GBS,
                 'score_sums_crps_field_us': 1e3 * f_ms, 'score_sums_crps_field_spread': f_sp, 'score_sums_crps_field_gbs': f_bytes / f_ms / 1e6,
                 'verify_error_sums_us': 1e3 * v_ms, 'verify_error_sums_spread': v_sp, 'verify_error_sums_gbs': x_bytes / v_ms / 1e6,
                 'verify_error_sums_of_peak': x_bytes / v_ms / 1e6 / PEAK_GBS,
                 'device_path_wall_ms': 1e3 * dev_wall, 'host_leads': hl, 'device_path_wall_host_leads_ms': 1e3 * dev_wall_hl,
                 'host_path_wall_host_leads_ms': 1e3 * host_wall}
            rows.append(r)
            print('S %2d M %3d axis %d: mean_spread %8.1f us %5.0f GB/s %5.3f of peak | score_sums %8.1f us %5.0f GB/s %5.3f (crps field '
                  '%8.1f us) | verify_error_sums %8.1f us %5.0f GB/s %5.3f | ensemble_scores wall: device %8.3f ms (56 leads), on %d '
                  'leads device %8.3f ms, host %9.1f ms' % (
                      samples, members, member_axis, r['mean_spread_us'], r['mean_spread_gbs'], r['mean_spread_of_peak'],
                      r['score_sums_us'], r['score_sums_gbs'], r['score_sums_of_peak'], r['score_sums_crps_field_us'],
                      r['verify_error_sums_us'], r['verify_error_sums_gbs'], r['verify_error_sums_of_peak'], r['device_path_wall_ms'], hl,
                      r['device_path_wall_host_leads_ms'], r['host_path_wall_host_leads_ms']), flush=True)
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds, 'leads': LEADS, 'rows_per_lead': ROWS, 'state': list(STATE),
                     'host_threads': os.cpu_count()},
           'ensemble': rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
