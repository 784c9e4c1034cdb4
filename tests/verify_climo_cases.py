"""Records and float64 restatements shared by tests/test_verify_windows_cpu.py and tests/test_gpu_verify_climo.py.

The value oracle of both files is a numpy restatement of the definitions in dlwp_amd/model/verify.py (the reference's own functions
need xarray, which is not installed): nothing here imports the code under test."""
import numpy as np

BOUND = 2.0 ** -22          # tests/test_gpu_verify.py: d rounded once in float32, float64 sums, one float32 cast
METHODS = ('mse', 'mae', 'rmse')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits_nan_exact(got, want):
    """NaN exactly where `want` has NaN, every other element with equal bits"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])


# -- a six-hourly record with one gap -------------------------------------------------------------------------------------------------- #
GAP_LEN, GAP_AT, INNER = 24, 11, (2, 3, 4)


def gap_record(seed=5):
    """(times (23,), values (23,) + INNER, full (24,) + INNER with a NaN row at the missing time)"""
    rng = np.random.default_rng(seed)
    full = rng.standard_normal((GAP_LEN,) + INNER).astype(np.float32)
    full[3, 1, 2, 0] = np.nan                       # a NaN that belongs to the data
    times = np.datetime64('2001-01-01T00') + np.arange(GAP_LEN) * np.timedelta64(6, 'h')
    keep = np.arange(GAP_LEN) != GAP_AT
    values = full[keep].copy()
    full[GAP_AT] = np.nan
    return times[keep], values, full, times


# -- the climatology record -------------------------------------------------------------------------------------------------------------- #
def month_of(times):
    """calendar month - 1 through Python's datetime, not through the arithmetic the code under test uses"""
    return np.array([d.month - 1 for d in np.asarray(times).astype('datetime64[s]').tolist()], np.int32)


def climo_record(dyadic=False, single_month=False, seed=7):
    """40 states at 11-day spacing from 2000-12-15: December, January and February come round twice, the year changes twice.
    Eleven days put at least two states into every month, so `single_month` drops 2001-11-21: November keeps one state.
    NaNs are sprinkled in, one column is NaN in every March state, one state is NaN throughout."""
    times = np.datetime64('2000-12-15T00') + np.arange(40) * np.timedelta64(11 * 24, 'h')
    rng = np.random.default_rng(seed)
    shape = (40, 2, 3, 4)
    if dyadic:
        x = (rng.integers(-(1 << 16) + 1, 1 << 16, shape) / 64.0).astype(np.float32)     # multiples of 2^-6 below 2^10
    else:
        x = (rng.standard_normal(shape) * 3.0 + 1.0).astype(np.float32)
    x.reshape(-1)[5::37] = np.nan
    months = month_of(times)
    x[months == 2, 1, 0, 2] = np.nan
    x[20] = np.nan
    if single_month:
        keep = times != np.datetime64('2001-11-21T00')
        times, x = times[keep], x[keep]
        assert (month_of(times) == 10).sum() == 1
    return times, x


def label_mean64(x, labels, n_labels):
    """float64 (n_labels,) + x.shape[1:]: NaN-skipping mean of the rows of each label; NaN where there is none"""
    out = np.full((n_labels,) + x.shape[1:], np.nan)
    x64 = x.astype(np.float64)
    for l in range(n_labels):
        sel = x64[labels == l]
        ok = ~np.isnan(sel)
        n = ok.sum(axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            out[l] = np.where(n > 0, np.where(ok, sel, 0.0).sum(axis=0) / n, np.nan)
    return out


def monthly64(x, times, val_rows, method):
    """(value in float64, anomaly float32) of the month-aware climatology error: climatology in float64 rounded once to float32,
    d = x - climatology in float32, the mean of d^2 or |d| in float64 over the non-NaN d"""
    months = month_of(times)
    climo = label_mean64(x, months, 12).astype(np.float32)
    with np.errstate(invalid='ignore'):
        d = x[val_rows] - climo[months[val_rows]]
    d64 = d.astype(np.float64)
    n = np.count_nonzero(~np.isnan(d64))
    v = (np.nansum(np.abs(d64)) if method == 'mae' else np.nansum(d64 * d64)) / n
    return (float(np.sqrt(v)) if method == 'rmse' else float(v)), d


def error_sums64(d):
    """(sum d^2, sum |d|, count) in float64 over the non-NaN elements of float32 d"""
    d64 = d.astype(np.float64)
    ok = ~np.isnan(d64)
    z = np.where(ok, d64, 0.0)
    return np.array([(z * z).sum(), np.abs(z).sum(), float(ok.sum())])
