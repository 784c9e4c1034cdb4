"""Host side of the second half of dlwp_amd.model.verify: the row-index function behind verification_from_samples / _series and its
numpy executor, the two reshaping helpers, and monthly_climo_error's host path against a float64 restatement
(tests/verify_climo_cases.py; the reference's functions need xarray and cannot be run here).

A note on the climatology record: 40 states at 11-day spacing put at least two states into every calendar month, so the case "one
month has a single state" is covered by a second record without 2001-11-21, beside the full one."""
import numpy as np
import pytest

from dlwp_amd import _lib
from dlwp_amd.model import verify
from dlwp_amd.model.generators import LabeledArray, SeriesDataset
from tests.verify_climo_cases import (BOUND, GAP_AT, GAP_LEN, INNER, METHODS, bits, climo_record, gap_record, month_of, monthly64,
                                      same_bits_nan_exact)

DIMS = ('sample', 'varlev', 'lat', 'lon')
H6 = np.timedelta64(6, 'h')


def series_ds(times, values):
    return SeriesDataset(values, {'sample': times, 'varlev': np.array(['z500', 't2m']), 'lat': np.arange(3.), 'lon': np.arange(4.)}, DIMS)


def samples_ds(times, values):
    """a file of samples: predictors and targets carry a time_step axis of 2; targets.isel(time_step=0) is `values`"""
    dims = ('sample', 'time_step') + DIMS[1:]
    coords = {'sample': times, 'varlev': np.array(['z500', 't2m']), 'lat': np.arange(3.), 'lon': np.arange(4.)}
    targets = np.stack([values, values + np.float32(100)], axis=1)
    return SeriesDataset(np.stack([values - np.float32(100), values - np.float32(50)], axis=1), coords, dims, targets=targets)


def padded(full, extra):
    return np.concatenate([full, np.full((extra,) + full.shape[1:], np.nan, np.float32)])


# -- the ABI-visible names --------------------------------------------------------------------------------------------------------------- #
def test_new_exports_are_declared_and_bound():
    names = _lib.declared_symbols()
    for n in ('dlwp_verify_label_nanmean_workspace', 'dlwp_verify_label_nanmean', 'dlwp_verify_label_error_sums', 'dlwp_gather_rows_fill'):
        assert n in names and getattr(_lib.lib, n).argtypes is not None, n
    for n in ('monthly_climo_error', 'verification_from_samples', 'verification_from_series', 'predictors_to_time_series',
              'add_metadata_to_forecast', 'verification_tensor', 'window_rows'):
        assert callable(getattr(verify, n)), n


# -- the row-index function ------------------------------------------------------------------------------------------------------------------ #
def test_window_rows_gap_end_of_record_and_foreign_dates():
    times, values, full, all_times = gap_record()
    pos = np.arange(GAP_LEN)
    pos = np.where(pos < GAP_AT, pos, pos - 1)           # row of the record that holds regular time k ...
    pos[GAP_AT] = -1                                     # ... and none at the gap
    ext = np.concatenate([pos, np.full(8, -1)])
    rows = verify.window_rows(times, all_times, 5, 6, 1)
    assert rows.dtype == np.int64 and rows.shape == (5, GAP_LEN)
    for f in range(5):
        assert np.array_equal(rows[f], ext[1 + f:1 + f + GAP_LEN]), f
    assert (rows[:, -1] == -1).all() and rows[4, -5] == -1 and rows[3, -5] == 22          # windows that run past the end
    assert np.array_equal(verify.window_rows(times, all_times, 5, 6, 0)[1:], rows[:4])
    # dates between the states, before the record and after it are nowhere; dt = 12 takes every other state
    off = verify.window_rows(times, all_times + np.timedelta64(3, 'h'), 3, 6, 0)
    assert (off == -1).all()
    early = verify.window_rows(times, np.array([all_times[0] - 2 * H6, all_times[-1] + H6]), 4, 6, 0)
    assert early.tolist() == [[-1, -1], [-1, -1], [0, -1], [1, -1]]
    assert np.array_equal(verify.window_rows(times, all_times[:4], 3, 12, 1), ext[[2, 4, 6]][:, None] + np.arange(4)[None, :])
    # an unsorted record gives positions in the record as it is stored
    perm = np.random.default_rng(1).permutation(times.size)
    back = verify.window_rows(times[perm], all_times, 2, 6, 0)
    assert np.array_equal(np.where(back >= 0, perm[np.maximum(back, 0)], -1), verify.window_rows(times, all_times, 2, 6, 0))
    assert verify.window_rows(times[:0], all_times[:2], 2, 6, 0).tolist() == [[-1, -1], [-1, -1]]


def test_host_executor_copies_bits_and_fills_quiet_nans():
    src = np.arange(12, dtype=np.float32).reshape(4, 3)
    src.view(np.uint32)[1, 1] = 0x7fc12345               # a NaN with a payload stays as it is
    rows = np.array([[3, -1], [1, 1]], np.int64)
    out = verify.take_rows_fill_host(src, rows)
    assert out.dtype == np.float32 and out.shape == (2, 2, 3)
    assert np.array_equal(bits(out[0, 0]), bits(src[3])) and np.array_equal(bits(out[1, 0]), bits(src[1]))
    assert (bits(out[0, 1]) == 0x7fc00000).all() and bits(out)[1, 1, 1] == 0x7fc12345


# -- verification_from_series / _samples ----------------------------------------------------------------------------------------------------- #
def test_verification_from_series_on_the_record_with_a_gap():
    times, values, full, all_times = gap_record()
    ds = series_ds(times, values)
    steps = 5
    got = verify.verification_from_series(ds, forecast_steps=steps, dt=6)
    assert isinstance(got, LabeledArray) and got.dims == ('f_hour', 'time', 'varlev', 'lat', 'lon')
    assert got.values.dtype == np.float32 and got.shape == (steps, 23) + INNER
    assert got.coords['f_hour'].dtype == np.dtype('timedelta64[h]')
    assert got.coords['f_hour'].astype(int).tolist() == [6, 12, 18, 24, 30]
    assert np.array_equal(got.coords['time'], times) and np.array_equal(got.coords['lat'], np.arange(3.))
    assert got.f_hour.values is got.coords['f_hour']
    keep = np.arange(GAP_LEN) != GAP_AT
    ext = padded(full, steps + 1)
    for f in range(steps):          # lead f of the date at regular position k is the state at k + 1 + f: a slice, then the dates we have
        same_bits_nan_exact(got.values[f], ext[1 + f:1 + f + GAP_LEN][keep])
    assert np.isnan(got.values[0, GAP_AT - 1]).all() and np.isnan(got.values[4, -5:]).all() and not np.isnan(got.values[3, -5]).any()


def test_samples_and_series_differ_by_exactly_one_lead():
    times, values, full, all_times = gap_record()
    sm = verify.verification_from_samples(samples_ds(times, values), forecast_steps=5, dt=6)
    sr = verify.verification_from_series(series_ds(times, values), forecast_steps=4, dt=6)
    assert sm.dims == sr.dims == ('f_hour', 'time', 'varlev', 'lat', 'lon')
    assert np.array_equal(bits(sm.values[1:]), bits(sr.values))
    same_bits_nan_exact(sm.values[0], values)            # the first lead of `samples` is the date itself
    assert sm.coords['f_hour'].astype(int).tolist() == [6, 12, 18, 24, 30]


def test_dates_outside_the_record_with_and_without_all_ds():
    times, values, full, all_times = gap_record()
    all_ds = series_ds(times, values)
    # a validation file of its own: regular positions 9 .. 12, the time of the gap among them, values of its own
    own = np.random.default_rng(9).standard_normal((4,) + INNER).astype(np.float32)
    ds = series_ds(all_times[9:13], own)
    alone = verify.verification_from_series(ds, forecast_steps=3, dt=6).values
    ext_own = padded(own, 4)
    for f in range(3):
        same_bits_nan_exact(alone[f], ext_own[1 + f:1 + f + 4])
    wide = verify.verification_from_series(ds, all_ds=all_ds, forecast_steps=3, dt=6)
    assert np.array_equal(wide.coords['time'], all_times[9:13])
    ext = padded(full, 4)
    for f in range(3):              # the date of the gap is no state of all_ds, its window is
        same_bits_nan_exact(wide.values[f], ext[10 + f:14 + f])
    assert np.isnan(wide.values[1, 0]).all() and not np.isnan(wide.values[0, 2]).any()
    sm = verify.verification_from_samples(samples_ds(all_times[9:13], own), all_ds=samples_ds(times, values), forecast_steps=2, dt=6)
    for f in range(2):
        same_bits_nan_exact(sm.values[f], ext[9 + f:13 + f])
    # dates three hours off every state: nothing but NaN
    shifted = verify.verification_from_series(series_ds(all_times[:3] + np.timedelta64(3, 'h'), own[:3]), all_ds=all_ds, forecast_steps=2)
    assert np.isnan(shifted.values).all() and shifted.shape == (2, 3) + INNER


def test_verification_refusals():
    times, values, _, _ = gap_record()
    ds = series_ds(times, values)
    for fn in (verify.verification_from_series, verify.verification_from_samples):
        with pytest.raises(ValueError, match="'forecast_steps' must be an integer >= 1"):
            fn(ds, forecast_steps=0)
        with pytest.raises(ValueError, match="'dt' must be an integer >= 1"):
            fn(ds, forecast_steps=2, dt=0)
    with pytest.raises(ValueError, match='does not match'):
        verify.verification_from_series(ds, all_ds=SeriesDataset(values[:, :1], {'sample': times}, DIMS), forecast_steps=2)
    with pytest.raises(ValueError, match="'kind'"):
        verify.verification_tensor(ds, kind='other')


# -- reshaping helpers ----------------------------------------------------------------------------------------------------------------------- #
class _Meta(object):
    """what predictors_to_time_series / add_metadata_to_forecast read of a dataset: dims and coordinates"""

    class _C(object):
        def __init__(self, values):
            self.values = values

    def __init__(self, **coords):
        self.dims = {k: len(v) for k, v in coords.items()}
        for k, v in coords.items():
            setattr(self, k, _Meta._C(np.asarray(v)))


def test_predictors_to_time_series():
    rng = np.random.default_rng(3)
    p = rng.standard_normal((5, 3, 4, 2, 6)).astype(np.float32)          # (sample, time_step, varlev, lat, lon)
    assert np.array_equal(verify.predictors_to_time_series(p, 3), p[:, -1])
    assert np.array_equal(verify.predictors_to_time_series(p, 3, use_first_step=True), p[:, 0])
    flat = p.reshape(5, 12, 2, 6)
    assert np.array_equal(verify.predictors_to_time_series(flat, 3, has_time_dim=False), p[:, -1])
    assert np.array_equal(verify.predictors_to_time_series(flat, 3, has_time_dim=False, use_first_step=True), p[:, 0])
    t = np.datetime64('2003-01-01T00') + np.arange(5) * H6
    varlev = _Meta(sample=t, varlev=['a', 'b', 'c', 'd'], lat=[0., 1.], lon=np.arange(6.))
    out = verify.predictors_to_time_series(p, 3, meta_ds=varlev)
    assert isinstance(out, LabeledArray) and out.dims == ('time', 'varlev', 'lat', 'lon') and np.array_equal(out.values, p[:, -1])
    assert np.array_equal(out.coords['time'], t) and out.coords['varlev'].tolist() == ['a', 'b', 'c', 'd']
    level = _Meta(sample=t, variable=['z', 't'], level=[500, 850], lat=[0., 1.], lon=np.arange(6.))
    out = verify.predictors_to_time_series(flat, 3, has_time_dim=False, use_first_step=True, meta_ds=level)
    assert out.dims == ('time', 'variable', 'level', 'lat', 'lon') and out.shape == (5, 2, 2, 2, 6)
    assert np.array_equal(out.values, p[:, 0].reshape(5, 2, 2, 2, 6)) and out.coords['level'].tolist() == [500, 850]
    # a SeriesDataset serves as meta_ds as it is
    sds = SeriesDataset(p[:, 0], {'sample': t, 'varlev': np.arange(4), 'lat': np.arange(2.), 'lon': np.arange(6.)}, DIMS)
    assert np.array_equal(verify.predictors_to_time_series(p, 3, meta_ds=sds).coords['time'], t)


def test_add_metadata_to_forecast():
    rng = np.random.default_rng(4)
    fc = rng.standard_normal((3, 5, 4, 2, 6)).astype(np.float32)
    t = np.datetime64('2003-01-01T00') + np.arange(5) * H6
    f_hour = np.arange(6, 19, 6).astype('timedelta64[h]')
    varlev = _Meta(sample=t, varlev=['a', 'b', 'c', 'd'], lat=[0., 1.], lon=np.arange(6.))
    out = verify.add_metadata_to_forecast(fc, f_hour, varlev)
    assert out.dims == ('f_hour', 'time', 'varlev', 'lat', 'lon') and np.array_equal(out.values, fc)
    assert np.array_equal(out.coords['f_hour'], f_hour) and np.array_equal(out.coords['time'], t)
    level = _Meta(sample=t, variable=['z', 't'], level=[500, 850], lat=[0., 1.], lon=np.arange(6.))
    out = verify.add_metadata_to_forecast(fc, f_hour, level)
    assert out.dims == ('f_hour', 'time', 'variable', 'level', 'lat', 'lon') and out.shape == (3, 5, 2, 2, 2, 6)
    assert np.array_equal(out.values.reshape(fc.shape), fc)
    for meta in (varlev, level):
        with pytest.raises(ValueError, match="'f_hour' coordinate must have same size as the first axis of 'forecast'"):
            verify.add_metadata_to_forecast(fc, f_hour[:2], meta)


# -- monthly_climo_error, host path ---------------------------------------------------------------------------------------------------------- #
def test_the_climatology_record_has_the_cases_it_is_meant_to_have():
    times, x = climo_record()
    months = month_of(times)
    assert times.size == 40 and np.unique(np.diff(times)).tolist() == [np.timedelta64(11 * 24, 'h')]
    years = times.astype('datetime64[Y]').astype(int) + 1970
    assert sorted(set(years.tolist())) == [2000, 2001, 2002]
    for m in (11, 0, 1):             # December, January, February: states of two different years
        assert len(set(years[months == m].tolist())) == 2
    assert np.bincount(months, minlength=12).min() == 2
    assert np.isnan(x[months == 2][:, 1, 0, 2]).all() and np.isnan(x[20]).all()
    assert np.bincount(month_of(climo_record(single_month=True)[0]), minlength=12).min() == 1
    assert np.array_equal(verify._months(times), months)


@pytest.mark.parametrize('single_month', [False, True], ids=['forty_states', 'one_state_in_november'])
@pytest.mark.parametrize('dyadic', [False, True], ids=['gaussian', 'dyadic'])
@pytest.mark.parametrize('time_dim', ['sample', 'time'])
def test_monthly_climo_error_host_path(time_dim, dyadic, single_month):
    times, x = climo_record(dyadic=dyadic, single_month=single_month)
    da = LabeledArray(x, {time_dim: times, 'lat': np.arange(3.)}, (time_dim, 'varlev', 'lat', 'lon'))
    val_rows = np.arange(1, times.size, 3)               # a strided subset
    val_set = list(times[val_rows])
    for method in METHODS:
        want, d = monthly64(x, times, val_rows, method)
        got, an = verify.monthly_climo_error(da, val_set, method=method, return_da=True)
        assert isinstance(got, float)
        print('%s %s %s: relative error %.3g of %.3g' % (time_dim, 'dyadic' if dyadic else 'gaussian', method, abs(got - want) / want,
                                                         BOUND))
        assert abs(got - want) <= BOUND * abs(want)
        if dyadic:
            assert got == want
        assert isinstance(an, LabeledArray) and an.dims == da.dims and an.values.dtype == np.float32
        assert np.array_equal(bits(an.values), bits(d)) and np.isnan(d).any() and not np.isnan(d).all()
        assert np.array_equal(an.coords[time_dim], times[val_rows]) and np.array_equal(an.coords['lat'], np.arange(3.))
        assert verify.monthly_climo_error(da, val_set, method=method) == got
        many = verify.monthly_climo_error(da, np.array(val_set), n_fhour=4, method=method)
        assert isinstance(many, np.ndarray) and many.shape == (4,) and (many == got).all()
    if single_month:                 # the only November state is its own climatology: zero anomaly wherever it is a number
        nov = int(np.flatnonzero(month_of(times) == 10)[0])
        _, an = verify.monthly_climo_error(da, [times[nov]], return_da=True)
        assert (an.values[~np.isnan(x[nov:nov + 1])] == 0).all()


def test_monthly_climo_error_with_the_time_axis_second():
    times, x = climo_record()
    da = LabeledArray(np.ascontiguousarray(np.moveaxis(x, 0, 1)), {'time': times}, ('varlev', 'time', 'lat', 'lon'))
    val_rows = np.arange(0, 40, 4)
    want, d = monthly64(x, times, val_rows, 'mse')
    got, an = verify.monthly_climo_error(da, times[val_rows], return_da=True)
    assert abs(got - want) <= BOUND * want and an.shape == (2, 10, 3, 4) and np.array_equal(bits(np.moveaxis(an.values, 1, 0)), bits(d))


def test_monthly_climo_error_refusals():
    times, x = climo_record()
    da = LabeledArray(x, {'time': times}, ('time', 'varlev', 'lat', 'lon'))
    with pytest.raises(ValueError, match="'method' must be 'mse', 'rmse', or 'mae'"):
        verify.monthly_climo_error(da, times[:3], method='bias')
    with pytest.raises(KeyError):
        verify.monthly_climo_error(da, [times[0], times[1] + np.timedelta64(1, 'h')])
    with pytest.raises(KeyError):
        verify.monthly_climo_error(da, [np.datetime64('1999-01-01T00')])
