#!/usr/bin/env python3
"""Zonal power spectra on the MI355X (csrc/spectrum.hip): HIP-event time of dlwp_verify_spectrum_sums on the 56-lead x 256-sample
series of the 4 x 88 x 180 state -- both layouts of `valid`, with and without the latitude weights, axis=None and per variable --
beside dlwp_verify_skill_sums on the same operands in the same run, alternating, with the ratio of the two.  Per case: us, GB/s (8
bytes read per pair: both operands once) and the share of the 8 TB/s HBM peak; the fp32 multiply-adds the kernel ISSUES on the matrix
cores (padding included and stated: rows to 32-row tiles, wavenumbers to 32-wavenumber tiles, the folded length K to an even number)
as TFLOP/s and as a share of the 157.3 TF fp32 matrix peak, beside the share of the multiplies a folded transform NEEDS (2 transforms
x 2 parts x K x K per row); and the two floors -- bytes over the HBM peak, issued flops over the matrix peak -- with the one that
binds.  Then what a caller sees: the wall time of verify.forecast_spectrum on the resident series against the host path for the same
arrays, the download included.  Every timed step runs in a child process under its own time limit; a step that fails ends the run.
Writes profiles/bench_spectrum.json (with the kernel source hash).  GPU only."""
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
PEAK_TFLOPS = 157.3                 # fp32 matrix: 64 FLOP / clk / SIMD
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


def matrix_work(plan, width):
    """(flops the kernel issues on the matrix cores, flops a folded transform needs) for a plan: per 32-row tile and 32-wavenumber tile
    four products of ceil(K / 2) instructions of 32 x 32 x 2 multiply-adds; needed: 2 transforms x 2 parts x K x K multiply-adds a row"""
    k = width // 2 + 1
    n_t, steps = -(-k // 32), -(-k // 2)
    rpr = plan.run // width
    issued = needed = 0
    for f in range(plan.leads):
        rows = max(plan.count0 - f * plan.count_dec, 0) * rpr
        issued += plan.groups * -(-rows // 32) * n_t * 4 * steps * (32 * 32 * 2 * 2)
        needed += plan.groups * rows * 4 * k * k * 2
    return float(issued), float(needed)


def raw_spectrum(plan, t, weights, width):
    """the C entry point on preallocated outputs: what the kernel pair costs, without the wrapper's checks, uploads and allocations"""
    import torch
    from dlwp_amd import _lib, ops
    fc, ob = t[plan.fc], t[plan.ob]
    h = _lib.handle(fc.device.index)
    k = width // 2 + 1
    ws = torch.empty(_lib.lib.dlwp_verify_spectrum_workspace(h, plan.leads, plan.groups, width), dtype=torch.uint8, device=fc.device)
    sums = torch.empty((plan.leads, plan.groups, 4, k), dtype=torch.float64, device=fc.device)
    norm = torch.empty((plan.leads, plan.groups, 2), dtype=torch.float64, device=fc.device)
    tw = torch.from_numpy(ops.spectrum_twiddles(width)).to(fc.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    LL = ctypes.c_longlong
    ptr = lambda x: ctypes.c_void_p(0 if x is None else x.data_ptr())      # noqa: E731

    def fn():
        _lib.check(_lib.lib.dlwp_verify_spectrum_sums(
            h, ptr(fc), LL(plan.fc_strides[0]), LL(plan.fc_strides[1]), plan.fc_strides[2], ptr(ob), LL(plan.ob_strides[0]),
            LL(plan.ob_strides[1]), plan.ob_strides[2], plan.leads, plan.count0, plan.count_dec, plan.groups, LL(plan.run), width,
            ptr(weights), 0 if weights is None else int(weights.numel()), ptr(tw), ptr(sums), ptr(norm), ptr(ws), ws.numel(), stream))
    return fn, (sums, norm), (fc, ob, ws, tw)


def raw_skill(plan, t, weights):
    """dlwp_verify_skill_sums on the same operands, strides and weights, without a climatology: the sibling"""
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
            LL(plan.ob_strides[1]), plan.ob_strides[2], plan.leads, plan.count0, plan.count_dec, plan.groups, LL(plan.run), ptr(None), 0,
            ptr(None), LL(0), 0, ptr(weights), 0 if weights is None else int(weights.numel()), LL(STATE[2]), ptr(sums), ptr(ws),
            ws.numel(), stream))
    return fn, sums, (fc, ob, ws)


def operands(layout, members):
    import torch
    forecast = torch.randn((LEADS, members) + STATE, device='cuda')
    valid = torch.randn((LEADS, members) + STATE, device='cuda')
    return forecast, (valid if layout == 'per_lead' else valid[0].contiguous())


def step_kernels(layout, members, iters, rounds):
    """one child process: the four kernel cases of one layout"""
    import torch
    from dlwp_amd.model import verify
    forecast, valid = operands(layout, members)
    t = {'forecast': forecast, 'valid': valid}
    weights = torch.from_numpy(verify.area_weights(np.linspace(-87.0, 87.0, STATE[1]))).cuda()
    row, width = int(np.prod(STATE)), STATE[2]
    out = []
    for per_variable in (False, True):
        axis = None if not per_variable else ((1, 3, 4) if layout == 'per_lead' else (0, 2, 3))
        plan = verify.plan_forecast_skill(forecast.shape, valid.shape, axis)
        pairs = sum(max(plan.count0 - f * plan.count_dec, 0) for f in range(LEADS))      # sample rows compared
        nbytes = 8.0 * pairs * row
        issued, needed = matrix_work(plan, width)
        for use_w in (False, True):
            fn, (sums, norm), _keep = raw_spectrum(plan, t, weights if use_w else None, width)
            sk_fn, sk_sums, _keep_s = raw_skill(plan, t, weights if use_w else None)
            (s_ms, s_sp), (k_ms, k_sp) = timeit([fn, sk_fn], iters, rounds)
            # the same pairs: W longitudes per counted row; Parseval: the error power sums to the sibling's sum w d^2
            assert torch.equal(norm[..., 1] * width, sk_sums[..., 9])
            assert torch.allclose(sums[:, :, 1].sum(dim=-1), sk_sums[..., 2] / width, rtol=1e-5, atol=0)
            hbm_floor, mat_floor = nbytes / PEAK_GBS / 1e6, issued / PEAK_TFLOPS / 1e9            # ms
            out.append({'layout': layout, 'members': members, 'per_variable': per_variable, 'weights': use_w, 'pairs_of_rows': pairs,
                        'bytes': nbytes, 'spectrum_us': 1e3 * s_ms, 'spectrum_spread': s_sp, 'spectrum_gbs': nbytes / s_ms / 1e6,
                        'spectrum_of_hbm_peak': nbytes / s_ms / 1e6 / PEAK_GBS, 'matrix_flops_issued': issued,
                        'matrix_flops_needed': needed, 'padding_factor': issued / needed, 'matrix_tflops_issued': issued / s_ms / 1e9,
                        'matrix_of_peak_issued': issued / s_ms / 1e9 / PEAK_TFLOPS,
                        'matrix_of_peak_needed': needed / s_ms / 1e9 / PEAK_TFLOPS, 'hbm_floor_us': 1e3 * hbm_floor,
                        'matrix_floor_us': 1e3 * mat_floor, 'binding_floor': 'matrix' if mat_floor > hbm_floor else 'hbm',
                        'of_binding_floor': max(hbm_floor, mat_floor) / s_ms, 'skill_sums_us': 1e3 * k_ms, 'skill_sums_spread': k_sp,
                        'skill_sums_gbs': nbytes / k_ms / 1e6, 'ratio_to_skill_sums': s_ms / k_ms})
            r = out[-1]
            print('%-12s %s %s %6.0f MB: spectrum %8.1f us %5.0f GB/s %5.3f of HBM peak, %5.1f TF issued %5.3f of matrix peak (needed '
                  '%5.3f, padding x%.3f; spread %4.1f %%) | floors: HBM %6.1f us, matrix %6.1f us | skill_sums %8.1f us | ratio %.2f'
                  % (layout, 'per-var' if per_variable else 'all    ', 'w' if use_w else '-', nbytes / 1e6, r['spectrum_us'],
                     r['spectrum_gbs'], r['spectrum_of_hbm_peak'], r['matrix_tflops_issued'], r['matrix_of_peak_issued'],
                     r['matrix_of_peak_needed'], r['padding_factor'], 100 * s_sp, r['hbm_floor_us'], r['matrix_floor_us'],
                     r['skill_sums_us'], r['ratio_to_skill_sums']), flush=True)
    return out


def step_wall(members, host_reps):
    """one child process: forecast_spectrum as a caller sees it, device against host (download included), weights given"""
    import torch
    from dlwp_amd.model import verify
    out = []
    for layout in LAYOUTS:
        forecast, valid = operands(layout, members)
        weights = verify.area_weights(np.linspace(-87.0, 87.0, STATE[1]))

        def wall(fn, reps):
            took = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                took.append(time.perf_counter() - t0)
            return float(np.median(took))
        verify.forecast_spectrum(forecast, valid, weights)
        dev = wall(lambda: verify.forecast_spectrum(forecast, valid, weights), 5)
        host = wall(lambda: verify.forecast_spectrum(forecast.cpu().numpy(), valid.cpu().numpy(), weights), host_reps)
        out.append({'layout': layout, 'members': members, 'device_path_wall_ms': 1e3 * dev, 'host_path_wall_ms': 1e3 * host})
        print('%-12s %d members: forecast_spectrum wall: device %8.3f ms, host with the download %9.1f ms'
              % (layout, members, 1e3 * dev, 1e3 * host), flush=True)
        del forecast, valid
        torch.cuda.empty_cache()
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_spectrum.py needs a GPU')
    if args.step == 'wall':
        res = step_wall(args.wall_members, args.host_reps)
    else:
        res = step_kernels(args.step, args.members, args.iters, args.rounds)
    from dlwp_amd import _lib
    print('RESULT ' + json.dumps({'rows': res, 'source_sha': _lib.kernel_source_hash(), 'device': torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--members', type=int, default=256)
    ap.add_argument('--wall-members', type=int, default=16, help='samples of the wall-time comparison (the host path takes seconds)')
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds each child process may take')
    ap.add_argument('--step', choices=LAYOUTS + ('wall',), help='(internal) run one step in this process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_spectrum.json'))
    args = ap.parse_args()
    if args.step:
        return child(args)
    res = {'_meta': {'peak_gbs': PEAK_GBS, 'peak_matrix_tflops': PEAK_TFLOPS, 'iters': args.iters, 'rounds': args.rounds,
                     'leads': LEADS, 'state': list(STATE), 'bytes_counted': 'both operands once',
                     'flops_counted': 'issued: 32-row x 32-wavenumber tiles, ceil(K / 2) steps of 32x32x2, four products; '
                                      'needed: 2 transforms x 2 parts x K x K multiply-adds per row', 'host_threads': os.cpu_count()}}
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
