#!/usr/bin/env python3
"""Climatological quantiles on the MI355X (csrc/quantile.hip): HIP-event time and GB/s over the bytes of the record read ONCE of
dlwp_verify_label_quantiles on the ten-year six-hourly record of tools/bench_verify_climo.py (14 608 states of 4 x 88 x 180, 3.7 GB),
with labels='month' (lists of about 1 240 rows: the LDS route at 16 columns) and labels=None (one list of 14 608 rows: the streaming
route), at K = 1, 3, 8 with 'linear' and 'lower' -- each beside dlwp_verify_label_nanmean on the same operands in the same run,
alternating: the one-pass floor, the same gather with a float64 add where this kernel selects.  Then what a caller sees: the wall
time of verify.climatological_quantiles on a resident record against the host path with the download, on a one-year record by default.
Every step runs in a child process under its own time limit; a step that fails or runs out of time ends the run.
Writes profiles/bench_quantiles.json (with the kernel source hash).  GPU only."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ('month', 'whole', 'wall')
KS = {1: (0.5,), 3: (1.0 / 3.0, 0.5, 2.0 / 3.0), 8: (0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.9, 0.95)}
METHODS = ('linear', 'lower')
LL = ctypes.c_longlong


def record(count):
    import torch
    from tools.bench_verify import STATE
    times = np.datetime64('1979-01-01T00') + np.arange(count) * np.timedelta64(6, 'h')
    x = torch.empty((count,) + STATE, device='cuda')
    for lo in range(0, count, 1024):
        x[lo:lo + 1024].normal_()
    return x, times


def raw_quantiles(x, labels, n_labels, q, method, route):
    """the C entry point on preallocated outputs: what the kernel costs, without the wrapper's allocations and upload"""
    import torch
    from dlwp_amd import _lib, ops
    count, row = x.shape[0], x[0].numel()
    h = _lib.handle(x.device.index)
    offsets, index = ops.label_lists(labels, n_labels)
    index_d = torch.from_numpy(index).to(x.device)
    qs = np.ascontiguousarray(q, dtype=np.float64)
    ws = torch.empty(_lib.lib.dlwp_verify_label_quantiles_workspace(h, count, row, n_labels, qs.size), dtype=torch.uint8, device=x.device)
    out = torch.empty((qs.size, n_labels) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    off_p, q_p = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), qs.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    m = ops.quantile_method(method)

    def fn():
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib.dlwp_verify_label_quantiles(h, x.data_ptr(), count, LL(row), off_p, index_d.data_ptr(), n_labels, q_p, qs.size, m,
                                                        route, out.data_ptr(), None, ws.data_ptr(), ws.numel(), stream))
    fn.keep = (offsets, index_d, qs, ws)
    return fn, out


def step_kernels(step, count, iters, rounds):
    from dlwp_amd import ops
    from dlwp_amd.model import verify
    from tools.bench_verify import PEAK_GBS, timeit
    from tools.bench_verify_climo import raw_label_nanmean
    x, times = record(count)
    row = x[0].numel()
    labels, n_labels = (verify.month_labels(times), 12) if step == 'month' else (np.zeros(count, np.int32), 1)
    max_len = int(np.bincount(labels, minlength=n_labels).max())
    route, cols = ops.verify_label_quantiles_plan(max_len, row)
    nbytes = 4.0 * count * row
    mean_fn = raw_label_nanmean(x, labels, n_labels)[0]
    rows = []
    for k, q in KS.items():
        for method in METHODS:
            fn, out = raw_quantiles(x, labels, n_labels, q, method, 0)
            (ms, sp), (yms, ysp) = timeit([fn, mean_fn], iters, rounds)
            ranks = (2 if method == 'linear' else 1) * k
            r = {'labels': step, 'k': k, 'method': method, 'ranks': ranks, 'route': route, 'cols': cols, 'max_len': max_len, 'states': count,
                 'bytes': nbytes, 'us': 1e3 * ms, 'spread': sp, 'gbs': nbytes / ms / 1e6, 'of_peak': nbytes / ms / 1e6 / PEAK_GBS,
                 'label_nanmean_us': 1e3 * yms, 'label_nanmean_spread': ysp, 'label_nanmean_gbs': nbytes / yms / 1e6,
                 'over_label_nanmean': ms / yms}
            rows.append(r)
            print('%-5s K %d %-6s (route %d, %3d columns, lists <= %5d): %10.1f us %6.0f GB/s (spread %4.1f %%) | label_nanmean %8.1f us '
                  '%5.0f GB/s (spread %4.1f %%) | %6.1f x' % (step, k, method, route, cols, max_len, r['us'], r['gbs'], 100 * sp,
                                                             r['label_nanmean_us'], r['label_nanmean_gbs'], 100 * ysp,
                                                             r['over_label_nanmean']), flush=True)
    return rows


def step_wall(count):
    import torch
    from dlwp_amd.model import verify
    from dlwp_amd.model.generators import LabeledArray
    from tools.bench_verify import wall
    x, times = record(count)
    dims = ('time', 'varlev', 'lat', 'lon')
    resident = LabeledArray(x, {'time': times}, dims)
    q = KS[3]
    out = {'states': count, 'k': 3, 'method': 'linear', 'labels': 'month'}
    out['device_resident_ms'] = 1e3 * wall(lambda: verify.climatological_quantiles(resident, q).cpu(), 3)

    def host():
        return verify.climatological_quantiles(LabeledArray(x.cpu().numpy(), {'time': times}, dims), q)
    out['host_with_download_ms'] = 1e3 * wall(host, 1)
    same = torch.equal(verify.climatological_quantiles(resident, q).cpu().view(torch.int32), torch.from_numpy(host()).view(torch.int32))
    out['same_bits'] = bool(same)
    print('caller, %d states, monthly terciles and median: device (resident record, result downloaded) %.1f ms, host with the download '
          '%.0f ms, same bits: %s' % (count, out['device_resident_ms'], out['host_with_download_ms'], same), flush=True)
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_quantiles.py needs a GPU')
    res = step_wall(args.host_count) if args.step == 'wall' else step_kernels(args.step, args.count, args.iters, args.rounds)
    from dlwp_amd import _lib
    print('RESULT ' + json.dumps({'rows': res, 'source_sha': _lib.kernel_source_hash(), 'device': torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--count', type=int, default=14608, help='states of the record (ten years at six hours)')
    ap.add_argument('--host-count', type=int, default=1460, help='states of the record of the host / device path comparison')
    ap.add_argument('--step-timeout', type=int, default=300, help='seconds each child process may take')
    ap.add_argument('--steps', nargs='*', default=list(STEPS), choices=STEPS)
    ap.add_argument('--step', choices=STEPS, help='(internal) run one step in this process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_quantiles.json'))
    args = ap.parse_args()
    if args.step:
        return child(args)
    from tools.bench_verify import PEAK_GBS, STATE
    res = {'_meta': {'peak_gbs': PEAK_GBS, 'iters': args.iters, 'rounds': args.rounds, 'state': list(STATE),
                     'bytes_counted': 'the record once', 'host_threads': os.cpu_count()}}
    for step in args.steps:
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--iters', str(args.iters), '--rounds', str(args.rounds),
               '--count', str(args.count), '--host-count', str(args.host_count)]
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
        res[step] = got['rows']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
