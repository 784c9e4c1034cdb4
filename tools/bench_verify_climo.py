#!/usr/bin/env python3
"""Month-aware climatology and verification windows on the MI355X (csrc/verify.hip): HIP-event time, GB/s and the fraction of the
8 TB/s HBM peak of dlwp_verify_label_nanmean on a ten-year six-hourly record of the 4 x 88 x 180 state (14 608 states, 3.7 GB), of
dlwp_verify_label_error_sums on 256 validation times of it (with and without the anomaly output) and of dlwp_gather_rows_fill on
the 56 x 256 verification windows (3.6 GB written) -- each beside dlwp_verify_error_sums on the same number of bytes in the same
run, alternating.  Then what a caller sees: the wall time of verify.monthly_climo_error and verify.verification_from_series on the
host path against the device path (upload included; verification_tensor leaves out the download), on a one-year record by default.
Writes profiles/bench_verify_climo.json (with the kernel source hash).  GPU only."""
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
from dlwp_amd.model.generators import LabeledArray, SeriesDataset  # noqa: E402
from tools.bench_verify import PEAK_GBS, STATE, timeit, wall  # noqa: E402

LEADS, MEMBERS = 56, 256
LL = ctypes.c_longlong


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_error_sums(a, b, count, row):
    """dlwp_verify_error_sums over `count` pairs of rows of a and b, one lead, one group: the yardstick, 8 bytes read per pair"""
    h = _lib.handle(a.device.index)
    ws = torch.empty(_lib.lib.dlwp_verify_error_workspace(h, 1, 1), dtype=torch.uint8, device=a.device)
    sums = torch.empty(3, dtype=torch.float64, device=a.device)
    return lambda: _lib.check(_lib.lib.dlwp_verify_error_sums(h, a.data_ptr(), LL(0), LL(row), 0, b.data_ptr(), LL(0), LL(row), 0, 1, count, 0,
                                                              1, LL(row), sums.data_ptr(), ws.data_ptr(), ws.numel(), stream()))


def raw_label_nanmean(x, labels, n_labels):
    count, row = x.shape[0], x[0].numel()
    h = _lib.handle(x.device.index)
    offsets, index = ops.label_lists(labels, n_labels)
    index_d = torch.from_numpy(index).to(x.device)
    ws = torch.empty(ops.verify_label_nanmean_workspace(x, n_labels), dtype=torch.uint8, device=x.device)
    mean = torch.empty((n_labels,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    off_p = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def fn():
        _lib.check(_lib.lib.dlwp_verify_label_nanmean(h, x.data_ptr(), count, LL(row), off_p, index_d.data_ptr(), n_labels, mean.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), stream()))
    fn.keep = (offsets, index_d, ws)
    return fn, mean, ws.numel() // (n_labels * row * 12)


def raw_label_error(x, rows, labels, table, anomaly):
    count, row, m = x.shape[0], x[0].numel(), len(rows)
    h = _lib.handle(x.device.index)
    rows_d = torch.from_numpy(np.asarray(rows, np.int32)).to(x.device)
    labels_d = torch.from_numpy(np.asarray(labels, np.int32)).to(x.device)
    ws = torch.empty(_lib.lib.dlwp_verify_error_workspace(h, 1, 1), dtype=torch.uint8, device=x.device)
    sums = torch.empty(3, dtype=torch.float64, device=x.device)
    out = torch.empty((m,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device) if anomaly else None
    return lambda: _lib.check(_lib.lib.dlwp_verify_label_error_sums(h, x.data_ptr(), count, LL(row), rows_d.data_ptr(), labels_d.data_ptr(), m,
                                                                    table.data_ptr(), table.shape[0], out.data_ptr() if anomaly else None,
                                                                    sums.data_ptr(), ws.data_ptr(), ws.numel(), stream()))


def raw_gather(src, rows, dst):
    h = _lib.handle(src.device.index)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int64).reshape(-1)).to(src.device)
    return lambda: _lib.check(_lib.lib.dlwp_gather_rows_fill(h, src.data_ptr(), LL(src.shape[0]), LL(src[0].numel()), rows_d.data_ptr(),
                                                             LL(rows_d.numel()), dst.data_ptr(), stream()))


def entry(name, nbytes, ms, spread, yard_ms, yard_spread, **more):
    r = {'kernel': name, 'bytes': nbytes, 'us': 1e3 * ms, 'spread': spread, 'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS,
         'error_sums_us': 1e3 * yard_ms, 'error_sums_spread': yard_spread, 'error_sums_gbs': nbytes / yard_ms / 1e6,
         'error_sums_of_peak': nbytes / yard_ms / 1e6 / PEAK_GBS}
    r['of_error_sums'] = r['gbs'] / r['error_sums_gbs']
    r.update(more)
    print('%-34s %8.1f MB: %9.1f us %5.0f GB/s %5.3f of peak (spread %4.1f %%) | dlwp_verify_error_sums on the same bytes %9.1f us '
          '%5.0f GB/s %5.3f | ratio %.2f' % (name, nbytes / 1e6, r['us'], r['gbs'], r['of_peak'], 100 * spread, r['error_sums_us'],
                                             r['error_sums_gbs'], r['error_sums_of_peak'], r['of_error_sums']), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--count', type=int, default=14608, help='states of the record (ten years at six hours)')
    ap.add_argument('--host-count', type=int, default=1460, help='states of the record of the host / device path comparison')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_verify_climo.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_verify_climo.py needs a GPU')
    row = int(np.prod(STATE))
    count = args.count
    times = np.datetime64('1979-01-01T00') + np.arange(count) * np.timedelta64(6, 'h')
    months = verify._months(times)
    x = torch.empty((count,) + STATE, device='cuda')
    for lo in range(0, count, 1024):
        x[lo:lo + 1024].normal_()
    kernels = []
    # the climatology: the whole record once
    half = count // 2
    fn, table, split = raw_label_nanmean(x, months, 12)
    (ms, sp), (yms, ysp) = timeit([fn, raw_error_sums(x[:half], x[half:], half, row)], args.iters, args.rounds)
    kernels.append(entry('label_nanmean %d states' % count, 8.0 * half * row, ms, sp, yms, ysp, split=int(split), states=count))
    # the anomaly of 256 validation times: x rows and table rows, 8 bytes per pair (+ 4 written with the anomaly output)
    val = np.sort(np.random.default_rng(0).choice(count, MEMBERS, replace=False))
    yard = raw_error_sums(x[:MEMBERS], x[MEMBERS:2 * MEMBERS], MEMBERS, row)
    for anomaly in (False, True):
        (ms, sp), (yms, ysp) = timeit([raw_label_error(x, val, months[val], table, anomaly), yard], 4 * args.iters, args.rounds)
        kernels.append(entry('label_error_sums %d times%s' % (MEMBERS, ' + anomaly' if anomaly else ''), 8.0 * MEMBERS * row, ms, sp, yms, ysp,
                             bytes_written=4.0 * MEMBERS * row if anomaly else 0.0))
    # the verification windows: 56 leads x 256 dates, read once and written once
    init = np.sort(np.random.default_rng(1).choice(count - LEADS - 1, MEMBERS, replace=False))
    rows = verify.window_rows(times, times[init], LEADS, 6, 1)
    dst = torch.empty((LEADS, MEMBERS) + STATE, device='cuda')
    n = LEADS * MEMBERS
    (ms, sp), (yms, ysp) = timeit([raw_gather(x, rows, dst), raw_error_sums(dst, x, n, row)], args.iters, args.rounds)
    kernels.append(entry('gather_rows_fill %d x %d windows' % (LEADS, MEMBERS), 8.0 * n * row, ms, sp, yms, ysp))
    assert torch.equal(dst[3, 5].view(torch.int32), x[int(rows[3, 5])].view(torch.int32))
    del dst
    torch.cuda.empty_cache()
    # what a caller sees
    hc = min(args.host_count, count)
    xh = x[:hc].cpu().numpy()
    da = LabeledArray(xh, {'time': times[:hc]}, ('time', 'varlev', 'lat', 'lon'))
    val_set = times[:hc][::max(hc // MEMBERS, 1)][:MEMBERS]
    ds_all = SeriesDataset(xh, {'sample': times[:hc]}, ('sample', 'varlev', 'lat', 'lon'))
    ds = SeriesDataset(xh[:MEMBERS], {'sample': times[:MEMBERS]}, ('sample', 'varlev', 'lat', 'lon'))
    resident = LabeledArray(x[:hc], {'time': times[:hc]}, ('time', 'varlev', 'lat', 'lon'))
    caller = {
        'states': hc, 'validation_times': len(val_set), 'leads': LEADS, 'dates': MEMBERS,
        'monthly_climo_error_host_ms': 1e3 * wall(lambda: verify.monthly_climo_error(da, val_set), 1),
        'monthly_climo_error_device_upload_ms': 1e3 * wall(lambda: verify.monthly_climo_error(da, val_set, device='cuda'), 3),
        'monthly_climo_error_device_resident_ms': 1e3 * wall(lambda: verify.monthly_climo_error(resident, val_set), 3),
        'verification_from_series_host_ms': 1e3 * wall(lambda: verify.verification_from_series(ds, ds_all, LEADS, 6), 1),
        'verification_from_series_device_ms': 1e3 * wall(lambda: verify.verification_from_series(ds, ds_all, LEADS, 6, device='cuda'), 1),
        'verification_tensor_ms': 1e3 * wall(lambda: verify.verification_tensor(ds, ds_all, LEADS, 6), 3)}
    t0 = time.perf_counter()
    host, dev = verify.monthly_climo_error(da, val_set), verify.monthly_climo_error(resident, val_set)
    caller['device_over_host_minus_1'] = dev / host - 1.0
    caller['check_s'] = time.perf_counter() - t0
    print('caller, %d states: monthly_climo_error host %.0f ms, device with upload %.1f ms, resident %.2f ms | verification_from_series '
          '%d x %d: host %.0f ms, device with upload and download %.0f ms, verification_tensor %.1f ms' % (
              hc, caller['monthly_climo_error_host_ms'], caller['monthly_climo_error_device_upload_ms'],
              caller['monthly_climo_error_device_resident_ms'], LEADS, MEMBERS, caller['verification_from_series_host_ms'],
              caller['verification_from_series_device_ms'], caller['verification_tensor_ms']), flush=True)
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds, 'state': list(STATE), 'host_threads': os.cpu_count()},
           'kernels': kernels, 'caller': caller}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
