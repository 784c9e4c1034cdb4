#!/usr/bin/env python3
"""Ensemble event verification on the MI355X (csrc/events.hip): HIP-event time, GB/s and the fraction of the 8 TB/s HBM peak of
dlwp_ens_event_counts on the benchmark's 56-lead series of the 4 x 88 x 180 state with 256 rows per lead, read as (samples, members)
= (1, 256), (8, 32) and (32, 8) in both member layouts, with K = 1, 3, 8 thresholds in two regimes -- a TAIL threshold (every column
in the bin n = 0, o = 0) and thresholds around the MEDIAN of a wide ensemble (the bins spread) -- with and without the probability
field.  Beside it, in the same run and alternating: dlwp_ens_mean_spread on the same tensor and layout (the yardstick: the same
member bytes in one pass) and dlwp_verify_error_sums on the same bytes.  `ratio` is events / mean_spread without the probability
field; the target is <= 1.25 for M <= 32 in both regimes (M = 256 is reported, not gated).  Then what a caller sees: the wall time of
ensemble.event_scores on the resident series against the host path with the download, on the first --host-leads leads.
Writes profiles/bench_events.json (with the kernel source hash).  GPU only."""
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
THRESHOLDS = (1, 3, 8)
TARGET = 1.25
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


def raw_events(x, st, y, thr, samples, members, row, prob):
    """thr: float32 device tensor (K, 1), one group; prob: a preallocated (K, leads, samples, row) tensor or None"""
    h = _lib.handle(x.device.index)
    k_n = int(thr.shape[0])
    ws = torch.empty(_lib.lib.dlwp_ens_event_workspace(h, LEADS, 1, members, k_n), dtype=torch.uint8, device=x.device)
    table = torch.empty((LEADS, 1, k_n, members + 1, 2), dtype=torch.int64, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(_lib.lib.dlwp_ens_event_counts(h, x.data_ptr(), LL(st[0]), LL(st[1]), LL(st[2]), y.data_ptr(), thr.data_ptr(),
                                                             0, 0, LEADS, samples, members, 1, LL(row), k_n, table.data_ptr(),
                                                             prob.data_ptr() if prob is not None else None, ws.data_ptr(), ws.numel(),
                                                             stream)), table


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


def regime_thresholds(regime, k_n):
    """tail: far above every value; median: K ascending values around 0, the median of the series below"""
    if regime == 'tail':
        return np.full(k_n, 1e30, np.float32)
    return (np.linspace(-0.5, 0.5, k_n) if k_n > 1 else np.zeros(1)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-leads', type=int, default=2, help='leads the host path is timed on')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_events.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_events.py needs a GPU')
    row = int(np.prod(STATE))
    # a WIDE ensemble: every row of a lead is a small common state plus unit noise, so the members of a column straddle the median
    base = 0.3 * torch.randn((LEADS, 1) + STATE, device='cuda')
    series = base + torch.randn((LEADS, ROWS) + STATE, device='cuda')
    x_bytes = 4.0 * series.numel()
    hl = max(1, min(args.host_leads, LEADS))
    rows = []
    for samples, members in POINTS:
        valid = (base + torch.randn((LEADS, samples) + STATE, device='cuda')).contiguous()
        y_bytes = 4.0 * valid.numel()
        probs = {k_n: torch.empty((k_n, LEADS, samples, row), dtype=torch.float32, device='cuda') for k_n in THRESHOLDS}
        for member_axis in (2, 1):
            st = ops.ens_strides(samples, members, row, member_axis)
            shape = (LEADS, samples, members) + STATE if member_axis == 2 else (LEADS, members, samples) + STATE
            view = series.view(shape)
            fns, keys, tables = [raw_mean_spread(series, st, samples, members, row), raw_verify_same_bytes(series, row)], [], {}
            for regime in ('tail', 'median'):
                for k_n in THRESHOLDS:
                    thr = torch.from_numpy(regime_thresholds(regime, k_n)[:, None].copy()).cuda()
                    for field in (False, True):
                        fn, table = raw_events(series, st, valid, thr, samples, members, row, probs[k_n] if field else None)
                        fns.append(fn)
                        keys.append((regime, k_n, field))
                        tables[(regime, k_n, field)] = table
            times = timeit(fns, args.iters, args.rounds)
            (m_ms, m_sp), (v_ms, v_sp) = times[:2]
            m_bytes = x_bytes + 2 * 4.0 * LEADS * samples * row
            r = {'samples': samples, 'members': members, 'member_axis': member_axis, 'series_bytes': x_bytes,
                 'mean_spread_us': 1e3 * m_ms, 'mean_spread_spread': m_sp, 'mean_spread_gbs': m_bytes / m_ms / 1e6,
                 'mean_spread_of_peak': m_bytes / m_ms / 1e6 / PEAK_GBS,
                 'verify_error_sums_us': 1e3 * v_ms, 'verify_error_sums_spread': v_sp, 'verify_error_sums_gbs': x_bytes / v_ms / 1e6,
                 'verify_error_sums_of_peak': x_bytes / v_ms / 1e6 / PEAK_GBS, 'gated': members <= 32, 'events': []}
            for (regime, k_n, field), (e_ms, e_sp) in zip(keys, times[2:]):
                e_bytes = x_bytes + y_bytes + (k_n * y_bytes if field else 0.0)
                table = tables[(regime, k_n, field)][:, 0, 0].sum(dim=0)             # threshold 0: (M + 1, 2) over all leads
                e = {'regime': regime, 'thresholds': k_n, 'prob_field': field, 'us': 1e3 * e_ms, 'spread': e_sp, 'gbs': e_bytes / e_ms / 1e6,
                     'of_peak': e_bytes / e_ms / 1e6 / PEAK_GBS, 'ratio_to_mean_spread': e_ms / m_ms,
                     'bins_hit_threshold_0': int((table > 0).sum()), 'largest_bin_share_threshold_0': float(table.max()) / float(table.sum())}
                if not field:
                    e['within_target'] = bool(e_ms / m_ms <= TARGET)
                r['events'].append(e)
                print('S %2d M %3d axis %d %-6s K %d %s: %8.1f us (+-%4.1f%%) %5.0f GB/s %5.3f of peak, %5.2f x mean_spread (%8.1f us), '
                      'verify_error_sums %8.1f us; %3d bins hit, largest %5.3f'
                      % (samples, members, member_axis, regime, k_n, 'prob ' if field else 'table', e['us'], 100 * e_sp, e['gbs'], e['of_peak'],
                         e['ratio_to_mean_spread'], r['mean_spread_us'], r['verify_error_sums_us'], e['bins_hit_threshold_0'],
                         e['largest_bin_share_threshold_0']), flush=True)
            thr3 = regime_thresholds('median', 3)
            r['device_path_wall_ms'] = 1e3 * wall(lambda: ensemble.event_scores(view, valid, thr3, member_axis=member_axis), 5)
            r['host_leads'] = hl
            r['device_path_wall_host_leads_ms'] = 1e3 * wall(lambda: ensemble.event_scores(view[:hl], valid[:hl], thr3, member_axis=member_axis), 5)
            r['host_path_wall_host_leads_ms'] = 1e3 * wall(lambda: ensemble.event_scores(view[:hl].cpu().numpy(), valid[:hl].cpu().numpy(), thr3,
                                                                                      member_axis=member_axis), 1)
            print('S %2d M %3d axis %d event_scores (K = 3) wall: device %8.3f ms (56 leads), on %d leads device %8.3f ms, host with the '
                  'download %9.1f ms' % (samples, members, member_axis, r['device_path_wall_ms'], hl, r['device_path_wall_host_leads_ms'],
                                         r['host_path_wall_host_leads_ms']), flush=True)
            rows.append(r)
    gated = [e['ratio_to_mean_spread'] for r in rows if r['gated'] for e in r['events'] if not e['prob_field']]
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds, 'leads': LEADS, 'rows_per_lead': ROWS, 'state': list(STATE),
                     'target_ratio': TARGET, 'worst_gated_ratio': max(gated), 'host_threads': os.cpu_count()},
           'events': rows}
    print('worst gated ratio (M <= 32, table only): %.3f (target %.2f)' % (max(gated), TARGET))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
