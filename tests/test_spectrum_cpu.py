"""Zonal power spectra without a device: the host path of verify.forecast_spectrum / persistence_spectrum against the float64
restatement of tests/spectrum_cases.py, finish_spectrum against its formulas, the identities of the definition (Parseval against
forecast_skill's mse, a perfect forecast, a pure wave, chunks that add), the arithmetic of csrc/spectrum.hip restated in float32 inside
the derived bound, and every refusal that comes before a launch -- those of the C entry point in the order include/dlwp_hip.h gives.

Host path against restatement is float64 against float64: 1e-12 relative to the value on every one of the four sums, and equal
counts."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import verify
from tests.spectrum_cases import CASES, U, axis_of, case, check_spectrum, check_sums, cosine, data, offset, red

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
FAKE = ctypes.c_void_p(4096)         # a non-null address for refusals that come before any launch; never dereferenced
NULL = ctypes.c_void_p(0)


def host_sums(name):
    fc, va, weights, grouped, n_fhour, ref = case(name)
    sums, norm = verify.spectrum_sums(fc, va, weights, axis_of(fc, va, grouped, n_fhour), n_fhour=n_fhour or None)
    return sums, norm, ref


# -- the host path against the restatement ------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('name', sorted(CASES))
def test_host_sums_are_the_restatement(name):
    sums, norm, ref = host_sums(name)
    assert sums.dtype == np.float64 and norm.dtype == np.float64 and sums.shape == ref.sums.shape
    assert np.array_equal(norm[..., 1], ref.norm[..., 1])
    assert np.allclose(norm[..., 0], ref.norm[..., 0], rtol=1e-12, atol=0)
    for q in range(4):
        tol = 1e-12 * np.abs(ref.sums[..., q, :])
        err = np.abs(sums[..., q, :] - ref.sums[..., q, :])
        assert (err <= tol).all(), (name, q, float((err / np.where(tol > 0, tol, 1)).max()))
    check_sums(sums, norm, ref, 'host ' + name)


@pytest.mark.parametrize('name', ['w5', 'w180_red', 'series', 'series_groups', 'persistence', 'offset', 'nonfinite'])
def test_host_spectrum_is_the_finished_restatement(name):
    fc, va, weights, grouped, n_fhour, ref = case(name)
    axis = axis_of(fc, va, grouped, n_fhour)
    got = (verify.persistence_spectrum(fc, va, n_fhour, weights, axis) if n_fhour else verify.forecast_spectrum(fc, va, weights, axis))
    check_spectrum(got, ref, grouped, 'host ' + name)
    if name.startswith('series'):
        assert (got.count[5:] == 0).all() and np.isnan(got.power_valid[5:]).all() and np.isnan(got.coherence[5:]).all()
    if name == 'nonfinite':
        # lead 0: rows (0,0,0,1) [both], (1,1,2) [inf], (2,0,5) [overflow of d]; lead 1: (2,1,0), (1,0,3), (0,1,4) -- of 3 x 6 per group
        assert got.count.tolist() == [[16, 17], [17, 16]]


def test_nonfinite_rows_are_skipped_whole_and_counted_out():
    fc, va, weights, grouped, _, ref = case('nonfinite')
    sums, norm = verify.spectrum_sums(fc, va, weights, axis_of(fc, va, grouped))
    assert np.isfinite(sums).all() and norm[..., 1].tolist() == [[16, 17], [17, 16]]
    # the same spectrum as the series without those rows: zero weight on them is not enough (0 * inf), dropping them is
    with np.errstate(invalid='ignore', over='ignore'):
        keep = np.isfinite(fc).all(axis=-1) & np.isfinite(va).all(axis=-1) & np.isfinite(fc - va).all(axis=-1)
    fc2, va2 = np.where(keep[..., None], fc, np.float32(0)), np.where(keep[..., None], va, np.float32(0))
    sums2, _ = verify.spectrum_sums(fc2, va2, weights, axis_of(fc, va, grouped))
    assert np.allclose(sums, sums2, rtol=1e-13, atol=0)


# -- finish_spectrum ----------------------------------------------------------------------------------------------------------------- #
def test_finish_spectrum_formulas_nan_rules_and_added_tables():
    rng = np.random.default_rng(5)
    s0, s1 = rng.uniform(1, 2, (3, 2, 6)), rng.uniform(0.1, 0.3, (3, 2, 6))
    s2, s3 = rng.uniform(-0.2, 0.2, (3, 2, 6)), rng.uniform(-0.2, 0.2, (3, 2, 6))
    sums = np.stack([s0, s1, s2, s3], axis=2) * 7.0
    norm = np.zeros((3, 2, 2))
    norm[..., 0], norm[..., 1] = 7.0, 40
    norm[2, 1] = (0.0, 40)               # sum w = 0
    norm[1, 0] = (7.0, 0)                # nothing counted
    sums[0, 0, 0, 3] = 0.0               # no power of the truth at one wavenumber: ratio and coherence NaN there
    got = verify.finish_spectrum(sums, norm)
    assert isinstance(got, verify.Spectrum) and got._fields == ('wavenumber', 'power_forecast', 'power_valid', 'power_error', 'ratio',
                                                                'coherence', 'count')
    assert got.wavenumber.tolist() == list(range(6)) and got.count.dtype == np.int64 and got.count[0].tolist() == [40, 40]
    s0[0, 0, 3] = 0.0
    p_f = s0 + s1 + 2 * s2
    with np.errstate(all='ignore'):
        want = {'power_forecast': p_f, 'power_valid': s0, 'power_error': s1, 'ratio': p_f / s0,
                'coherence': ((s0 + s2) ** 2 + s3 ** 2) / (p_f * s0)}
    for name, w in want.items():
        w = w.copy()
        w[2, 1], w[1, 0] = np.nan, np.nan
        if name in ('ratio', 'coherence'):
            w[0, 0, 3] = np.nan
        g = getattr(got, name)
        assert g.dtype == np.float32 and g.shape == (3, 2, 6)
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= 2.0 ** -23 * np.abs(w[ok])).all(), name
    assert got.count[2, 1] == 40 and got.count[1, 0] == 0
    # tables add before the finish; grouped=False drops a groups axis of one
    twice = verify.finish_spectrum(sums + sums, norm + norm)
    for a, b in zip(got[1:6], twice[1:6]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(twice.count, 2 * got.count)
    flat = verify.finish_spectrum(sums[:, :1], norm[:, :1], grouped=False)
    assert flat.power_valid.shape == (3, 6) and flat.count.shape == (3,)
    assert np.array_equal(flat.ratio, got.ratio[:, 0], equal_nan=True) and flat.count.tolist() == got.count[:, 0].tolist()
    with pytest.raises(ValueError, match='finish_spectrum'):
        verify.finish_spectrum(sums[:, :, :3], norm)
    with pytest.raises(ValueError, match='finish_spectrum'):
        verify.finish_spectrum(sums, norm[:, :1])


# -- identities ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
@pytest.mark.parametrize('width', [10, 9])
def test_parseval_the_error_power_sums_to_the_weighted_mse(axis, width):
    inner = (2, 6, width)
    fc, va, w = data((3, 4) + inner, 51), data((3, 4) + inner, 52), cosine(6)
    spec = verify.forecast_spectrum(fc, va, w, axis)
    skill = verify.forecast_skill(fc, va, weights=w, axis=axis)
    total = spec.power_error.astype(np.float64).sum(axis=-1)
    assert total.shape == skill.mse.shape
    # K float32 casts of the spectrum (2^-24 each, one sign), one of the mse, float64 behind them
    assert (np.abs(total - skill.mse) <= 2.0 ** -20 * skill.mse).all(), np.abs(total / skill.mse - 1).max() / 2.0 ** -20
    # and the other two powers: the weighted means of fc^2 and ob^2
    wk = np.broadcast_to(w.astype(np.float64)[:, None], inner)
    for field, x in ((spec.power_forecast, fc), (spec.power_valid, va)):
        x64 = x.astype(np.float64)
        ax = (1, 2, 3, 4) if axis is None else (1, 3, 4)
        mean = (wk * x64 ** 2).sum(axis=ax) / np.broadcast_to(wk, x.shape).sum(axis=ax)
        assert np.allclose(field.astype(np.float64).sum(axis=-1), mean, rtol=2.0 ** -20, atol=0)


def test_a_perfect_forecast_has_ratio_and_coherence_one_and_no_error_power():
    va = data((2, 3, 2, 6, 12), 53)
    got = verify.forecast_spectrum(va, va, cosine(6))
    assert np.array_equal(got.ratio, np.ones_like(got.ratio)) and np.array_equal(got.coherence, np.ones_like(got.coherence))
    assert np.array_equal(got.power_error, np.zeros_like(got.power_error))
    assert np.array_equal(got.power_forecast, got.power_valid) and got.count.tolist() == [36, 36]


@pytest.mark.parametrize('width, k0', [(12, 3), (12, 6), (9, 4), (180, 45), (5, 1)])
def test_a_pure_wave_puts_its_power_at_its_wavenumber_only(width, k0):
    j = np.arange(width)
    row = np.cos(2 * np.pi * k0 * j / width)
    va = np.broadcast_to(row, (1, 2, 1, 3, width)).astype(np.float32)
    got = verify.forecast_spectrum(np.zeros_like(va), va)                   # forecast 0: error power = power of the truth
    want = np.zeros(width // 2 + 1)
    want[k0] = 1.0 if 2 * k0 == width else 0.5                              # cos(pi j) = +-1 has mean square 1
    for field in (got.power_valid, got.power_error):
        assert field.shape == (1, width // 2 + 1)
        assert np.abs(field[0] - want).max() < 1e-6, field
    assert got.count.tolist() == [6]


def test_sums_of_two_sample_chunks_add_to_the_whole():
    fc, va, w = data((3, 7, 2, 6, 10), 55), data((3, 7, 2, 6, 10), 56), cosine(6)
    whole = verify.spectrum_sums(fc, va, w, (1, 3, 4))
    a, b = verify.spectrum_sums(fc[:, :3], va[:, :3], w, (1, 3, 4)), verify.spectrum_sums(fc[:, 3:], va[:, 3:], w, (1, 3, 4))
    assert np.allclose(a[0] + b[0], whole[0], rtol=1e-13, atol=1e-13 * np.abs(whole[0]).max())
    assert np.array_equal(a[1][..., 1] + b[1][..., 1], whole[1][..., 1]) and np.allclose(a[1] + b[1], whole[1], rtol=1e-14)
    one = verify.finish_spectrum(a[0] + b[0], a[1] + b[1])
    for x, y in zip(one[1:6], verify.forecast_spectrum(fc, va, w, (1, 3, 4))[1:6]):
        assert np.allclose(x, y, rtol=2.0 ** -22, atol=0, equal_nan=True)


def test_both_forms_of_valid_and_persistence_pair_the_same_rows():
    """a plain series and the per-lead array cut from it give the same sums lead by lead; persistence is forecast_spectrum of the
    repeated predictors"""
    inner = (2, 4, 8)
    series, fc = data((6,) + inner, 57), data((3, 4) + inner, 58)
    plain = verify.spectrum_sums(fc, series[:4], None, None)                # 4, 3, 2 pairs
    for f in range(3):
        cnt = 4 - f
        per = verify.spectrum_sums(fc[f:f + 1, :cnt], series[None, f:f + cnt], None, None)
        assert np.allclose(per[0][0], plain[0][f], rtol=1e-13, atol=0) and np.array_equal(per[1][0], plain[1][f])
    pers = verify.persistence_spectrum(series, series[:5], 3, axis=(0, 2, 3))
    rep = np.stack([series[:5]] * 3)
    same = verify.forecast_spectrum(rep, series[:5], axis=(0, 2, 3))
    for x, y in zip(pers, same):
        assert np.array_equal(x, y, equal_nan=True)
    assert pers.count[:, 0].tolist() == [20, 16, 12] and np.array_equal(pers.power_error[0], np.zeros_like(pers.power_error[0]))


# -- the arithmetic of the kernel, restated in float32 -------------------------------------------------------------------------------- #
def kernel_row(x, tw):
    """csrc/spectrum.hip on one row, in numpy float32: the float64 row sum, the mean out, the fold in place (e_j at j, o_j at W - j), a
    j-ordered fused chain of K products per part padded to an even number, twiddles by the running index (j k) mod W.  Returns X_k"""
    w = x.size
    k = w // 2 + 1
    total = float(np.sum(x.astype(np.float64)))
    m = np.float32(total / w)
    buf = np.zeros(w + 2, np.float32)
    buf[:w] = x
    half = (w - 1) // 2
    for j in range(1, half + 1):
        a, b = np.float32(buf[j] - m), np.float32(buf[w - j] - m)
        buf[j], buf[w - j] = np.float32(a + b), np.float32(a - b)
    buf[0] = np.float32(buf[0] - m)
    if w % 2 == 0:
        buf[w // 2] = np.float32(buf[w // 2] - m)
    kw = np.arange(k)
    re, im = np.zeros(k, np.float32), np.zeros(k, np.float32)
    idx = np.zeros(k, np.int64)
    for j in range(2 * ((k + 1) // 2)):
        e = buf[j] if j < k else np.float32(0)
        o = buf[w - j] if (j > 0 and 2 * j < w) else np.float32(0)
        assert np.array_equal(idx, (j * kw) % w)
        # fmaf: the product exact in float64 (24 x 24 bits), one rounding of the sum
        re = (np.float64(e) * tw[idx].astype(np.float64) + re.astype(np.float64)).astype(np.float32)
        im = (np.float64(o) * tw[w + idx].astype(np.float64) + im.astype(np.float64)).astype(np.float32)
        idx = idx + kw
        idx = np.where(idx >= w, idx - w, idx)
    out = re.astype(np.float64) - 1j * im.astype(np.float64)
    out[0] = total
    return out


@pytest.mark.parametrize('width', [4, 5, 6, 7, 9, 30, 45, 180, 360, 511, 512])
@pytest.mark.parametrize('gen', [data, red, offset], ids=['white', 'red', 'offset'])
def test_kernel_arithmetic_restated_in_float32_stays_inside_the_bound(width, gen):
    """the fold, the index walk and the select rules of the kernel, on the host: every coefficient of every row within delta_x of
    np.fft.rfft, with room (the issue's emulation stayed below 0.35 of the bound)"""
    tw = ops.spectrum_twiddles(width)
    assert tw.dtype == np.float32 and tw.shape == (2 * width,) and tw[0] == 1 and tw[width] == 0
    rows = gen((3, width), 100 + width)
    n = width // 2 + 1
    assert n <= (width - 1) // 2 + 2
    worst = 0.0
    for x in rows:
        x64 = x.astype(np.float64)
        want = np.fft.rfft(x64)
        got = kernel_row(x, tw)
        delta = (n + 4) * U * (np.abs(x64 - x64.mean()).sum() + width * U * abs(x64.mean()))
        err = np.abs(got - want)
        assert err[0] <= 2.0 ** -45 * np.abs(x64).sum()
        worst = max(worst, float(err[1:].max() / delta))
    print('W %d %s: |X^ - X| / delta_x = %.3f' % (width, gen.__name__, worst))
    assert worst <= 0.5


# -- refusals ------------------------------------------------------------------------------------------------------------------------ #
def test_refusals_of_the_public_functions():
    inner = (2, 6, 10)
    fc, va, w = data((3, 5) + inner, 61), data((3, 5) + inner, 62), cosine(6)
    bad = w.copy()
    bad[2] = -0.25
    with pytest.raises(ValueError, match='>= 0'):
        verify.forecast_spectrum(fc, va, bad)
    bad[2] = np.inf
    with pytest.raises(ValueError, match='finite'):
        verify.forecast_spectrum(fc, va, bad)
    with pytest.raises(ValueError, match='all zero'):
        verify.forecast_spectrum(fc, va, np.zeros(6, np.float32))
    with pytest.raises(ValueError, match="'weights' must hold one weight per row"):
        verify.forecast_spectrum(fc, va, np.ones(10, np.float32))                      # the longitude axis
    with pytest.raises(ValueError, match="'weights' must hold one weight per row"):
        verify.forecast_spectrum(fc[:, :, 0], va[:, :, 0], w, axis=(1, 3))              # per latitude row: no latitude left in a group
    with pytest.raises(ValueError, match="'axis' must be None"):
        verify.forecast_spectrum(fc, va, axis=(1, 2, 3))
    with pytest.raises(ValueError, match="'axis' must be None"):
        verify.forecast_spectrum(fc, va, axis=0, device='cuda')
    with pytest.raises(ValueError, match='do not match'):
        verify.forecast_spectrum(fc, va[:, :4])
    with pytest.raises(ValueError, match='do not match'):
        verify.persistence_spectrum(fc[0, :3], va[0], 2)
    with pytest.raises(ValueError, match="'n_fhour' must be >= 1"):
        verify.persistence_spectrum(va[0], va[0], 0)
    with pytest.raises(ValueError, match='latitude and a longitude axis'):
        verify.forecast_spectrum(fc[:, :, 0, 0], va[:, :, 0, 0])
    with pytest.raises(ValueError, match='at least 4'):
        verify.forecast_spectrum(fc[..., :3], va[..., :3])
    wide = np.zeros((1, 1, 2, 513), np.float32)
    with pytest.raises(ValueError, match='at most 512'):
        verify.forecast_spectrum(wide, wide, device='cuda')                               # refused before anything is uploaded
    assert verify.forecast_spectrum(wide, wide).power_valid.shape == (1, 257)             # the host path has no limit
    with pytest.raises(TypeError, match="'valid' must be a CUDA float32 tensor"):
        verify.forecast_spectrum(fc, torch.zeros(va.shape))
    with pytest.raises(ValueError, match='do not match'):
        verify.forecast_spectrum(fc.tolist(), va[:, :4].tolist())                         # array-likes are taken as arrays
    assert np.array_equal(verify.forecast_spectrum(fc.tolist(), va.tolist()).power_error,
                          verify.forecast_spectrum(fc.astype(np.float64), va).power_error)
    with pytest.raises(TypeError, match="'forecast' must be float32"):
        verify.forecast_spectrum(fc.astype(np.float64), va, device='cuda')


def _call(h=NULL, fc=FAKE, ob=FAKE, leads=2, count0=4, count_dec=1, groups=3, run=24, width=8, weights=NULL, w_len=0, tw=FAKE,
          sums=FAKE, norm=FAKE, ws=FAKE, ws_bytes=1 << 20, strides=(288, 72, 0, 0, 72, 1)):
    return _lib.lib.dlwp_verify_spectrum_sums(h, fc, LL(strides[0]), LL(strides[1]), strides[2], ob, LL(strides[3]), LL(strides[4]),
                                              strides[5], leads, count0, count_dec, groups, LL(run), width, weights, w_len, tw, sums,
                                              norm, ws, ws_bytes, NULL)


def _refused(rc, text):
    assert rc == _lib.EINVAL, rc
    assert text in _lib.lib.dlwp_last_error().decode(), _lib.lib.dlwp_last_error()


def test_entry_point_refuses_in_the_documented_order_without_a_launch():
    """every refusal comes before the handle is looked at, each with the later ones provoked as well: the earlier one is reported"""
    names = _lib.declared_symbols()
    assert 'dlwp_verify_spectrum_sums' in names and 'dlwp_verify_spectrum_workspace' in names
    header = open(os.path.join(ROOT, 'include', 'dlwp_hip.h')).read()
    assert 'int dlwp_verify_spectrum_sums(' in header and 'size_t dlwp_verify_spectrum_workspace(' in header
    assert len(_lib.lib.dlwp_verify_spectrum_sums.argtypes) == 23 and _lib.lib.dlwp_verify_spectrum_workspace.restype is ctypes.c_size_t
    _refused(_call(leads=0, count_dec=-1), 'must all be >= 1')
    _refused(_call(run=0, fc=NULL), 'must all be >= 1')
    _refused(_call(count_dec=-1, width=3), 'negative')
    _refused(_call(strides=(288, 72, 0, 0, -72, 1), fc=NULL), 'negative')
    _refused(_call(width=3, run=24, fc=NULL), 'width 3')
    _refused(_call(width=513, run=513, weights=FAKE, w_len=0), 'width 513')
    _refused(_call(width=5, sums=NULL), 'width 5')                                        # does not divide a run of 24
    _refused(_call(weights=FAKE, w_len=0, fc=NULL), 'do not divide')
    _refused(_call(weights=FAKE, w_len=2, norm=NULL), 'do not divide')                    # 3 longitude rows in a run
    _refused(_call(weights=FAKE, w_len=6), 'do not divide')
    for kw in (dict(fc=NULL), dict(ob=NULL), dict(sums=NULL), dict(norm=NULL), dict(tw=NULL)):
        _refused(_call(leads=1 << 12, groups=1 << 9, **kw), 'null pointer')
    _refused(_call(leads=1 << 12, groups=(1 << 8) + 1, ws_bytes=0), 'cells')
    _refused(_call(count0=1 << 30, run=512, width=4, ws_bytes=0), 'longitude rows in a cell')
    _refused(_call(ws_bytes=0), 'workspace too small')
    # 2 leads x 3 groups, 4 samples x 3 rows = 12 rows: one tile, one block per cell; K = 5: 22 doubles
    _refused(_call(ws_bytes=6 * 22 * 8 - 1), 'workspace too small (1055 < 1056)')
    _refused(_call(ws=NULL), 'workspace too small')
    _refused(_call(ws=ctypes.c_void_p(4100)), '8-byte aligned')
    _refused(_call(ws_bytes=6 * 22 * 8, weights=FAKE, w_len=3), 'null handle')
    # no lead has pairs: nothing is needed in the workspace, and still no launch without a handle
    _refused(_call(count0=0, ws=NULL, ws_bytes=0), 'null handle')


@pytest.mark.parametrize('leads, groups, width', [(1, 1, 180), (56, 1, 180), (56, 4, 360), (5, 3, 45), (3000, 2, 512)])
def test_workspace_is_the_documented_product_and_covers_fewer_active_leads(leads, groups, width):
    got = _lib.lib.dlwp_verify_spectrum_workspace(NULL, leads, groups, width)
    assert got == leads * groups * -(-2048 // (leads * groups)) * (4 * (width // 2 + 1) + 2) * 8
    for bad in ((0, groups, width), (leads, 0, width), (leads, groups, 3), (leads, groups, 513)):
        assert _lib.lib.dlwp_verify_spectrum_workspace(NULL, *bad) == 0
    run = 88 * width
    row = groups * run
    for count0 in (1, 8, 256):
        _refused(_call(leads=leads, groups=groups, count0=count0, run=run, width=width, ws_bytes=got,
                       strides=(300 * row, row, 0, 0, row, 1)), 'null handle')


def test_wrapper_refuses_before_the_device_is_looked_at():
    with pytest.raises(RuntimeError, match='device'):
        ops.verify_spectrum_sums(torch.zeros(64), (0, 32, 0), torch.zeros(64), (0, 32, 0), 1, 2, 0, 2, 16, 8)


def test_kernel_source_keeps_its_promises():
    """structural: no atomics, no host synchronisation, no allocation, no device sincos in csrc/spectrum.hip; the stream-taking export
    marks the tape; the product runs on the exact float32 matrix instruction"""
    src = open(os.path.join(ROOT, 'dlwp_amd', 'csrc', 'spectrum.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    for word in ('atomic', 'Synchronize', 'hipMalloc', 'hipMemcpy', '__threadfence', 'sincos', 'cosf(', 'sinf(', 'asm'):
        assert word not in code, word
    assert 'DLWP_UNTAPED(dlwp_verify_spectrum_sums)' in code and '__builtin_amdgcn_mfma_f32_32x32x2f32' in code
