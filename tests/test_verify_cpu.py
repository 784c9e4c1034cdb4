"""Forecast verification on the device, the part that needs none: the C ABI of csrc/verify.hip (symbols, refusals, workspace size), the
mapping of dlwp_amd.model.verify from (shapes, axis) to the strides of ONE dlwp_verify_error_sums call -- replayed by a numpy loop
over the pairs it describes and compared with the host functions --, the fall-back to the host path, the argument checks, and the
unchanged bits of the host path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ('mse', 'mae', 'rmse')
LL = ctypes.c_longlong
FAKE = ctypes.c_void_p(4096)         # a non-null address for refusals that come before any launch; never dereferenced
NULL = ctypes.c_void_p(0)


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------- #
def test_symbols_are_declared_exported_and_bound():
    names = _lib.declared_symbols()
    for n in ('dlwp_verify_error_workspace', 'dlwp_verify_error_sums', 'dlwp_verify_nanmean_samples'):
        assert n in names, n
        assert getattr(_lib.lib, n).argtypes is not None, n
    assert _lib.lib.dlwp_verify_error_workspace.restype is ctypes.c_size_t
    assert len(_lib.lib.dlwp_verify_error_sums.argtypes) == 18


def _sums(h=NULL, a=FAKE, b=FAKE, leads=2, count0=4, count_dec=1, groups=3, run=8, sums=FAKE, ws=FAKE, ws_bytes=1 << 20,
          strides=(0, 24, 1, 96, 24, 0)):
    return _lib.lib.dlwp_verify_error_sums(h, a, LL(strides[0]), LL(strides[1]), strides[2], b, LL(strides[3]), LL(strides[4]),
                                           strides[5], leads, count0, count_dec, groups, LL(run), sums, ws, ws_bytes, NULL)


def _refused(rc, text):
    assert rc == _lib.EINVAL, rc
    assert text in _lib.lib.dlwp_last_error().decode(), _lib.lib.dlwp_last_error()


def test_error_sums_refuses_without_a_launch():
    """every refusal comes before the handle is looked at (include/dlwp_hip.h gives the order): none of these reaches a device"""
    for kw in (dict(leads=0), dict(groups=0), dict(run=0), dict(leads=-3)):
        _refused(_sums(**kw), 'must all be >= 1')
    _refused(_sums(count_dec=-1), 'negative')
    _refused(_sums(strides=(0, -24, 1, 96, 24, 0)), 'negative')
    for kw in (dict(a=NULL), dict(b=NULL), dict(sums=NULL), dict(ws=NULL)):
        _refused(_sums(**kw), 'null pointer')
    _refused(_sums(leads=1 << 12, groups=1 << 9), 'cells')
    _refused(_sums(ws_bytes=0), 'workspace too small')
    # 2 leads x 3 groups, rows of 8 floats as 2 quads: lead 0 has 4 x 2 = 8 units -> one block per cell, 6 x 24 bytes
    _refused(_sums(ws_bytes=6 * 24 - 1), 'workspace too small (143 < 144)')
    _refused(_sums(ws_bytes=6 * 24), 'null handle')
    # no lead has pairs: nothing is needed in the workspace, and still no launch without a handle
    _refused(_sums(count0=0, ws_bytes=0), 'null handle')


def test_nanmean_samples_refuses_without_a_launch():
    f = _lib.lib.dlwp_verify_nanmean_samples
    _refused(f(NULL, FAKE, 0, LL(5), FAKE, NULL), 'must be >= 1')
    _refused(f(NULL, FAKE, 3, LL(0), FAKE, NULL), 'must be >= 1')
    _refused(f(NULL, NULL, 3, LL(5), FAKE, NULL), 'null pointer')
    _refused(f(NULL, FAKE, 3, LL(5), NULL, NULL), 'null pointer')
    _refused(f(NULL, FAKE, 3, LL(5), FAKE, NULL), 'null handle')


@pytest.mark.parametrize('leads, groups', [(1, 1), (56, 1), (56, 4), (5, 3), (3000, 2)])
def test_workspace_is_at_least_the_documented_product(leads, groups):
    """leads * groups * B * 24 bytes with B = ceil(8 * CUs / (leads * groups)); without a handle 256 CUs are counted"""
    got = _lib.lib.dlwp_verify_error_workspace(NULL, leads, groups)
    assert got == leads * groups * -(-2048 // (leads * groups)) * 24
    assert got >= leads * groups * 3 * 8
    assert _lib.lib.dlwp_verify_error_workspace(NULL, 0, groups) == 0 and _lib.lib.dlwp_verify_error_workspace(NULL, leads, 0) == 0


@pytest.mark.parametrize('leads, groups, count0, count_dec', [(56, 1, 8, 1), (56, 1, 256, 1), (56, 4, 8, 1), (56, 1, 64, 0), (5, 3, 3, 1),
                                                              (3000, 2, 7, 1), (7, 1, 1, 1), (56, 1, 100, 3)])
def test_workspace_covers_every_count_of_active_leads(leads, groups, count0, count_dec):
    """a launch spreads its blocks over the leads that HAVE pairs (8 of 56 for 8 members against a plain series), so it can use
    more blocks per cell than leads * groups would get: the size the workspace function names is enough for all of them -- the call
    gets as far as the handle check"""
    ws = _lib.lib.dlwp_verify_error_workspace(NULL, leads, groups)
    row = groups * 63360 // 4 * 4
    _refused(_sums(leads=leads, groups=groups, count0=count0, count_dec=count_dec, run=row // groups, ws_bytes=ws,
                   strides=(0, row, 1, 300 * row, row, 0)), 'null handle')


def test_kernel_source_keeps_its_promises():
    """structural: no atomics, no host synchronisation, no allocation in csrc/verify.hip; both stream-taking exports mark the tape"""
    src = open(os.path.join(ROOT, 'dlwp_amd', 'csrc', 'verify.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    for word in ('atomic', 'Synchronize', 'hipMalloc', 'hipMemcpy', '__threadfence'):
        assert word not in code, word
    assert 'DLWP_UNTAPED(dlwp_verify_error_sums)' in code and 'DLWP_UNTAPED(dlwp_verify_nanmean_samples)' in code


# -- the mapping, replayed ----------------------------------------------------------------------------------------------------------- #
def replay(plan, arrays):
    """the (leads, groups, 3) sums of the pairs `plan` describes, by the header's addressing rule on the flat operands:
    row i of x at lead f starts at f * lead_stride + (i + f * shift) * sample_stride; d in float32, NaN skipped"""
    a, b = (np.ascontiguousarray(arrays[k], np.float32).ravel() for k in (plan.a, plan.b))
    assert ops.verify_extent(plan.a_strides, plan.leads, plan.count0, plan.count_dec, plan.groups, plan.run) <= a.size
    assert ops.verify_extent(plan.b_strides, plan.leads, plan.count0, plan.count_dec, plan.groups, plan.run) <= b.size
    out = np.zeros((plan.leads, plan.groups, 3))
    for f in range(plan.leads):
        for i in range(max(plan.count0 - f * plan.count_dec, 0)):
            for g in range(plan.groups):
                oa = f * plan.a_strides[0] + (i + f * plan.a_strides[2]) * plan.a_strides[1] + g * plan.run
                ob = f * plan.b_strides[0] + (i + f * plan.b_strides[2]) * plan.b_strides[1] + g * plan.run
                d = a[oa:oa + plan.run] - b[ob:ob + plan.run]
                assert d.dtype == np.float32 and d.size == plan.run
                d = d[~np.isnan(d)].astype(np.float64)
                out[f, g] += ((d * d).sum(), np.abs(d).sum(), d.size)
    return out


def series(shape, seed, nan_every=37):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) + 0.5).astype(np.float32)
    x.ravel()[seed % nan_every::nan_every] = np.nan
    return x


def close_to_host(got, want, terms):
    """the host path sums float32 terms: its own rounding is at most terms * 2^-24 relative (sequential worst case); a wrong
    index moves a result by its own size"""
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= (terms + 4) * 2.0 ** -24 * np.abs(want[ok])).all()


INNER = [(2, 3, 5), (3, 4), (2, 2, 3, 4)]


@pytest.mark.parametrize('inner', INNER, ids=[str(len(i)) + 'd' for i in INNER])
@pytest.mark.parametrize('grouped', [False, True], ids=['all', 'groups'])
def test_mapping_of_the_five_uses_against_the_host_functions(inner, grouped):
    F, N, NV = 4, 7, 6
    row = int(np.prod(inner))
    groups, run = (inner[0], row // inner[0]) if grouped else (1, row)
    fc, va, va5 = series((F, N) + inner, 1), series((NV,) + inner, 2), series((F, N) + inner, 3)
    va[2] = np.nan                                               # a whole NaN sample row
    ax_plain = (0,) + tuple(range(2, 1 + len(inner))) if grouped else None
    ax_steps = (1,) + tuple(range(3, 2 + len(inner))) if grouped else None
    terms = N * row

    p = verify.plan_forecast(fc.shape, va5.shape, ax_steps)
    assert p == verify.Plan('forecast', 'valid', (N * row, row, 0), (N * row, row, 0), F, N, 0, groups, run)
    q = verify.plan_forecast(fc.shape, va.shape, ax_plain)
    assert q == verify.Plan('valid', 'forecast', (0, row, 1), (N * row, row, 0), F, NV, 1, groups, run)
    r = verify.plan_persistence(fc[0].shape, va.shape, 3, ax_plain)
    assert r == verify.Plan('valid', 'predictors', (0, row, 1), (0, row, 0), 3, NV, 1, groups, run)
    c = verify.plan_climo(va.shape, 3, ax_plain)
    assert c == verify.Plan('valid', 'mean', (0, row, 0), (0, 0, 0), 3, NV, 1, groups, run)
    with np.errstate(all='ignore'):
        mean = np.nanmean(va, axis=0)
        for method in METHODS:
            close_to_host(verify.finish(replay(p, {'forecast': fc, 'valid': va5}), method, grouped),
                          verify.forecast_error(fc, va5, method=method, axis=ax_steps), terms)
            close_to_host(verify.finish(replay(q, {'forecast': fc, 'valid': va}), method, grouped),
                          verify.forecast_error(fc, va, method=method, axis=ax_plain), terms)
            close_to_host(verify.finish(replay(r, {'predictors': fc[0], 'valid': va}), method, grouped),
                          verify.persistence_error(fc[0], va, 3, method=method, axis=ax_plain), terms)
            close_to_host(verify.finish(replay(c, {'mean': mean, 'valid': va}), method, grouped),
                          verify.climo_error(va, 3, method=method, axis=ax_plain), terms)


def test_axis_forms_are_normalised_and_everything_else_goes_to_the_host():
    f5, v4 = (5, 9, 2, 6, 8), (9, 2, 6, 8)
    assert verify.plan_forecast(f5, v4, (0, 2, 3)) == verify.plan_forecast(f5, v4, [3, -2, 0]) is not None
    assert verify.plan_forecast(f5, f5, (1, 3, 4)) == verify.plan_forecast(f5, f5, (-1, 1, -2)) is not None
    assert verify.plan_forecast(f5, v4, (0, 2, 3)).groups == 2 and verify.plan_forecast(f5, v4, None).groups == 1
    for axis in (0, (0,), (0, 1), (0, 1, 2, 3), (1, 2, 3), (0, 2), (0, 2, 3, 4), (0, 2, 7)):
        assert verify.plan_forecast(f5, v4, axis) is None, axis
        assert verify.plan_persistence(v4, v4, 4, axis) is None, axis
        assert verify.plan_climo(v4, 3, axis) is None, axis
    for axis in (0, (1,), (1, 2, 3, 4), (0, 3, 4), (0, 2, 3)):
        assert verify.plan_forecast(f5, f5, axis) is None, axis
    assert verify.plan_forecast((5, 9, 6), (9, 6), (0,)) is None                 # one inner axis: nothing behind the group axis
    assert verify.plan_forecast((5, 9, 6), (9, 6), None).run == 6
    assert verify.plan_forecast((0, 9, 2, 6), (9, 2, 6), None) is None            # no lead: the host path returns the empty array
    assert verify.plan_persistence(v4, v4, 0, None) is None and verify.plan_climo(v4, 0, None) is None
    assert verify.plan_forecast((5, 9, 2, 1, 8), (5, 9, 2, 6, 8), None) is None   # numpy broadcasts these: the host path does
    assert verify.plan_forecast((5, 12, 2, 6, 8), v4, None).count0 == 9           # N > Nv
    p = verify.plan_forecast((5, 3, 2, 6, 8), (3, 2, 6, 8), None)                 # leads 3 and 4 have no pairs
    assert (p.leads, p.count0, p.count_dec) == (5, 3, 1)
    assert ops.verify_extent(p.a_strides, 5, 3, 1, 1, 96) == 3 * 96 and ops.verify_extent(p.b_strides, 5, 3, 1, 1, 96) == 2 * 288 + 96


def test_finish_divides_in_float64_and_marks_empty_leads():
    s = np.array([[[8.0, 4.0, 2.0]], [[0.0, 0.0, 0.0]], [[np.inf, np.inf, 3.0]]])
    assert verify.finish(s, 'mse', False).tolist()[::2] == [4.0, np.inf] and np.isnan(verify.finish(s, 'mse', False)[1])
    assert verify.finish(s, 'mae', False).tolist()[0] == 2.0 and verify.finish(s, 'rmse', False).tolist()[0] == 2.0
    out = verify.finish(s, 'rmse', True)
    assert out.shape == (3, 1) and out.dtype == np.float32
    third = verify.finish(np.array([[[1.0, 1.0, 3.0]]]), 'mse', False)
    assert third[0] == np.float32(1.0 / 3.0)                                      # one rounding of the float64 quotient


# -- fall-back, refusals, the host path's bits ------------------------------------------------------------------------------------- #
def test_unsupported_axes_run_the_host_code_whatever_the_device_keyword(golden):
    g = golden('verify')
    fc, va = g['forecast'], g['valid']
    for method in METHODS:
        got = verify.persistence_error(fc[0], va, 4, method=method, axis=0, device='cuda')
        assert np.array_equal(got, g['pe_axis_%s' % method], equal_nan=True)
        got = verify.forecast_error(fc, va, method=method, axis=(0, 1), device='cuda')
        assert np.array_equal(got, verify.forecast_error(fc, va, method=method, axis=(0, 1)), equal_nan=True)
        got = verify.climo_error(va, 3, method=method, axis=(0,), device='cuda')
        assert np.array_equal(got, verify.climo_error(va, 3, method=method, axis=(0,)), equal_nan=True)


def test_host_path_keeps_its_bits_without_the_keyword(golden):
    g = golden('verify')
    fc, va, va5 = g['forecast'], g['valid'], g['valid_steps']
    for method in METHODS:
        cases = {'fe_series_%s': verify.forecast_error(fc, va, method=method),
                 'fe_series_axis_%s': verify.forecast_error(fc, va, method=method, axis=(0, 2, 3), device=None),
                 'fe_steps_%s': verify.forecast_error(fc, va5, method=method),
                 'fe_steps_axis_%s': verify.forecast_error(fc, va5, method=method, axis=(1, 3, 4)),
                 'pe_%s': verify.persistence_error(fc[0], va, 4, method=method, device=None),
                 'ce_%s': verify.climo_error(va, 3, method=method, device=None)}
        for key, got in cases.items():
            want = g[key % method]
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), key % method


def test_type_errors_name_the_argument():
    x = np.zeros((3, 4, 2, 3, 4), np.float32)
    for bad in (torch.zeros(x.shape), torch.zeros(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.bfloat16)):
        with pytest.raises(TypeError, match="'forecast' must be a CUDA float32 tensor"):
            verify.forecast_error(bad, x)
        with pytest.raises(TypeError, match="'valid' must be a CUDA float32 tensor"):
            verify.forecast_error(x, bad, device='cuda')
        with pytest.raises(TypeError, match="'predictors' must be a CUDA float32 tensor"):
            verify.persistence_error(bad[0], x[0], 2)
        with pytest.raises(TypeError, match="'valid' must be a CUDA float32 tensor"):
            verify.climo_error(bad[0], 2)
    with pytest.raises(TypeError, match="'valid' must be float32 on the device path, got float64"):
        verify.forecast_error(x, x.astype(np.float64), device='cuda')
    with pytest.raises(ValueError, match="'method' must be"):                     # the method is looked at first
        verify.forecast_error(torch.zeros(x.shape), x, method='bias')


def test_value_errors_come_before_any_launch():
    x = np.zeros((3, 4, 2, 3, 4), np.float32)
    with pytest.raises(ValueError, match='do not match'):
        verify.forecast_error(x, np.zeros((3, 4, 2, 3, 5), np.float32), device='cuda')
    with pytest.raises(ValueError, match='do not match'):
        verify.forecast_error(x, np.zeros((4, 2, 5, 4), np.float32), device='cuda')
    with pytest.raises(ValueError, match='do not match'):                         # N = 4 forecasts for Nv = 6: numpy refuses step 0
        verify.forecast_error(x, np.zeros((6, 2, 3, 4), np.float32), device='cuda')
    with pytest.raises(ValueError, match='do not match'):
        verify.persistence_error(x[0, :3], x[0], 2, device='cuda')
    with pytest.raises(ValueError, match='CUDA device'):
        verify.forecast_error(x, x, device='cpu')
    cuda = [torch.device('cuda', 0), torch.device('cuda', 1)]
    with pytest.raises(ValueError, match='different devices: cuda:0, cuda:1'):
        verify._common_device(cuda, None)
    with pytest.raises(ValueError, match='different devices'):
        verify._common_device(cuda[:1], 'cuda:1')
    assert verify._common_device(cuda[:1], 'cuda') == cuda[0] and verify._common_device(cuda[1:], 'cuda:1') == cuda[1]
    assert verify._common_device([], None) is None


def test_wrapper_checks_the_addressed_extent_without_a_device():
    assert ops.verify_extent((0, 24, 1), 4, 7, 1, 3, 8) == 7 * 24            # valid[f:]: the same last row at every lead
    assert ops.verify_extent((7 * 24, 24, 0), 4, 7, 1, 3, 8) == 3 * 168 + 4 * 24
    assert ops.verify_extent((0, 0, 0), 4, 7, 1, 3, 8) == 24                    # the climatology's one row
    assert ops.verify_extent((0, 24, 1), 5, 0, 1, 3, 8) == 0
    with pytest.raises(RuntimeError, match='device'):
        ops.verify_error_sums(torch.zeros(8), (0, 8, 0), torch.zeros(8), (0, 8, 0), 1, 1, 0, 1, 8)
