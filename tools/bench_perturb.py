#!/usr/bin/env python3
"""The ensemble member generator on the MI355X (csrc/perturb.hip): HIP-event time, GB/s over input plus output bytes and the share
of the 8 TB/s HBM peak of dlwp_ens_perturb for (samples, members) = (1, 256), (8, 32), (32, 8) of the 4 x 88 x 180 state, white
(L = 0) and smoothed (L = 2, R = 6) -- beside dlwp_dropout_fwd, which runs the same Philox-4x32-10 once per four elements, on the
same output bytes in the same alternating rounds.  Then the front end a caller sees: perturb_members on the device (launch to
synchronised result) against drawing the normals with numpy, adding and uploading.  Writes profiles/bench_perturb.json (with the
kernel source hash).  GPU only."""
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
POINTS = ((1, 256), (8, 32), (32, 8))
LENGTHS = (0.0, 2.0)


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


def raw_perturb(x, sigma, out, members, length, member_axis=2):
    """the C entry point on a preallocated output: what the kernels cost, without the wrapper's allocation"""
    s_n, k_n, h_n, w_n = x.shape
    taps = ensemble.smoothing_taps(length)[1]
    _, ss, ms = ops.ens_strides(s_n, members, k_n * h_n * w_n, member_axis)
    d = ops.ens_perturb_desc(s_n, k_n, h_n, w_n, members, 0, 2016, taps, taps, True, False, ss, ms)
    h = _lib.handle(x.device.index)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(_lib.lib.dlwp_ens_perturb(h, x.data_ptr(), sigma.data_ptr(), out.data_ptr(), d, stream))


def raw_dropout(src, out):
    h = _lib.handle(src.device.index)
    d = ops.dropout_desc(0.25, 2016, 0, 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(_lib.lib.dlwp_dropout_fwd(h, src.data_ptr(), out.data_ptr(), ctypes.c_longlong(src.numel()), d, stream))


def wall(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def host_front_end(x, members, stddev):
    """what a caller did before: S M C H W normals in numpy, the sum, the upload"""
    rng = np.random.default_rng(2016)
    noise = rng.standard_normal((x.shape[0], members) + x.shape[1:], dtype=np.float32)
    batch = (x[:, None] + np.float32(stddev) * noise).reshape((-1,) + x.shape[1:])
    return torch.from_numpy(batch).cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_perturb.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_perturb.py needs a GPU')
    rows = []
    for samples, members in POINTS:
        x = torch.randn((samples,) + STATE, device='cuda')
        sigma = torch.full((STATE[0],), 0.05, device='cuda')
        out = torch.empty((samples * members,) + STATE, device='cuda')
        src = torch.randn_like(out)
        drop = torch.empty_like(out)
        in_bytes, out_bytes = 4.0 * x.numel(), 4.0 * out.numel()
        fns = [raw_perturb(x, sigma, out, members, length) for length in LENGTHS] + [raw_dropout(src, drop)]
        (w_ms, w_sp), (s_ms, s_sp), (d_ms, d_sp) = timeit(fns, args.iters, args.rounds)
        xh = x.cpu().numpy()
        dev_white = wall(lambda: ensemble.perturb_members(x, members, stddev=0.05, seed=1), 5)
        dev_smooth = wall(lambda: ensemble.perturb_members(x, members, stddev=0.05, length=2.0, seed=1), 5)
        dev_upload = wall(lambda: ensemble.perturb_members(xh, members, stddev=0.05, length=2.0, seed=1, device='cuda'), 5)
        host = wall(lambda: host_front_end(xh, members, 0.05), 3)
        gbs = lambda ms: (in_bytes + out_bytes) / ms / 1e6          # noqa: E731
        r = {'samples': samples, 'members': members, 'input_bytes': in_bytes, 'output_bytes': out_bytes,
             'white_us': 1e3 * w_ms, 'white_spread': w_sp, 'white_gbs': gbs(w_ms), 'white_of_peak': gbs(w_ms) / PEAK_GBS,
             'smoothed_us': 1e3 * s_ms, 'smoothed_spread': s_sp, 'smoothed_gbs': gbs(s_ms), 'smoothed_of_peak': gbs(s_ms) / PEAK_GBS,
             'dropout_fwd_us': 1e3 * d_ms, 'dropout_fwd_spread': d_sp, 'dropout_fwd_gbs': 2.0 * out_bytes / d_ms / 1e6,
             'dropout_fwd_of_peak': 2.0 * out_bytes / d_ms / 1e6 / PEAK_GBS,
             'white_over_dropout': w_ms / d_ms, 'smoothed_over_dropout': s_ms / d_ms,
             'front_end_device_white_ms': 1e3 * dev_white, 'front_end_device_smoothed_ms': 1e3 * dev_smooth,
             'front_end_device_smoothed_numpy_in_ms': 1e3 * dev_upload, 'front_end_host_white_ms': 1e3 * host}
        rows.append(r)
        print('S %2d M %3d: white %7.1f us %5.0f GB/s %5.3f of peak (+-%.2f) | smoothed L=2 %7.1f us %5.0f GB/s %5.3f (+-%.2f) | '
              'dropout_fwd %7.1f us %5.0f GB/s %5.3f (+-%.2f) | x dropout: %.2f, %.2f | front end: device %.3f / %.3f ms, host %.1f ms'
              % (samples, members, r['white_us'], r['white_gbs'], r['white_of_peak'], w_sp, r['smoothed_us'], r['smoothed_gbs'],
                 r['smoothed_of_peak'], s_sp, r['dropout_fwd_us'], r['dropout_fwd_gbs'], r['dropout_fwd_of_peak'], d_sp,
                 r['white_over_dropout'], r['smoothed_over_dropout'], r['front_end_device_white_ms'], r['front_end_device_smoothed_ms'],
                 r['front_end_host_white_ms']), flush=True)
    res = {'_meta': {'source_sha': _lib.kernel_source_hash(), 'peak_gbs': PEAK_GBS, 'device': torch.cuda.get_device_name(0),
                     'iters': args.iters, 'rounds': args.rounds, 'state': list(STATE), 'lengths': list(LENGTHS)},
           'perturb': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
