"""Forecast verification on the device (csrc/verify.hip behind dlwp_amd.model.verify) against a float64 restatement of the same
definition: d = float64(a) - float64(b), NaN pairs skipped, mean / sqrt in float64.

Bound (derived): the device rounds d once in float32 (2^-24 relative per term), so d^2 is off by about 2^-23, sums of
non-negative terms keep the relative bound, float64 accumulation adds n * 2^-53, the final cast 2^-24:
|device - float64| <= 2^-22 * |float64| for every method.  Where the float64 value is 0, NaN or infinite the result is equal to it.
Run with -s to see error / bound of every case."""
import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import verify
from tests.nets import cnn2_layers

pytestmark = pytest.mark.gpu

METHODS = ('mse', 'mae', 'rmse')
BOUND = 2.0 ** -22


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


# -- the float64 restatement --------------------------------------------------------------------------------------------------------- #
def measure64(diff, grouped):
    """diff: float64 (count, groups, ...) -> (sum d^2, sum |d|, count) over everything (grouped: everything but axis 1), NaN skipped"""
    ax = tuple(a for a in range(diff.ndim) if not (grouped and a == 1))
    ok = ~np.isnan(diff)
    z = np.where(ok, diff, 0.0)
    return np.stack([(z * z).sum(axis=ax), np.abs(z).sum(axis=ax), ok.sum(axis=ax).astype(np.float64)], axis=-1)


def value64(s, method):
    with np.errstate(all='ignore'):
        v = np.where(s[..., 2] > 0, s[..., 1 if method == 'mae' else 0] / s[..., 2], np.nan)
        return np.sqrt(v) if method == 'rmse' else v


def forecast64(fc, va, grouped):
    """(F, [groups,] 3) sums of forecast_error in float64; leads beyond the verification series have no pairs"""
    fc, va = fc.astype(np.float64), va.astype(np.float64)
    with np.errstate(invalid='ignore'):
        if fc.ndim == va.ndim:
            return np.stack([measure64(va[f] - fc[f], grouped) for f in range(fc.shape[0])])
        nv = va.shape[0]
        return np.stack([measure64(va[f:f + max(nv - f, 0)] - fc[f, :max(nv - f, 0)], grouped) for f in range(fc.shape[0])])


def persistence64(pr, va, n_fhour, grouped):
    pr, va = pr.astype(np.float64), va.astype(np.float64)
    nv = va.shape[0]
    with np.errstate(invalid='ignore'):
        return np.stack([measure64(va[f:f + max(nv - f, 0)] - pr[:max(nv - f, 0)], grouped) for f in range(n_fhour)])


def nanmean64(va):
    """the mean the device stores: non-NaN samples summed in float64 in sample order, divided, rounded to float32 once"""
    s, n = np.zeros(va.shape[1:]), np.zeros(va.shape[1:])
    with np.errstate(invalid='ignore'):
        for row in va.astype(np.float64):
            ok = ~np.isnan(row)
            s = s + np.where(ok, row, 0.0)
            n = n + ok
        with np.errstate(divide='ignore'):
            return np.where(n > 0, s / n, np.nan)


def climo64(va, n_fhour, grouped):
    mean = nanmean64(va).astype(np.float32).astype(np.float64)
    va, nv = va.astype(np.float64), va.shape[0]
    with np.errstate(invalid='ignore'):
        return np.stack([measure64(va[:max(nv - f, 0)] - mean, grouped) for f in range(n_fhour)])


def within(got, want, what, allowance=None):
    """got: the float32 result; want: float64.  NaN where want is NaN, equal where want is 0 or infinite, else inside the bound"""
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    exact = np.isinf(want) | (want == 0)
    assert np.array_equal(got[exact].astype(np.float64), want[exact]), what
    ok = ~np.isnan(want) & ~exact
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    bound = BOUND * np.abs(want[ok]) + (0.0 if allowance is None else allowance[ok])
    print('%s: error / bound %.3f over %d values' % (what, float((err / bound).max()) if err.size else 0.0, err.size))
    assert (err <= bound).all(), (what, float((err / bound).max()))


def data(shape, seed, nan_every=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 3.0 + 1.0).astype(np.float32)
    if nan_every:
        x.ravel()[seed % nan_every::nan_every] = np.nan
    return x


def cuda(x, misalign=False):
    """x on the device; misalign: the same values one float into a storage, so the address is 4 (mod 16)"""
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if not misalign:
        assert t.data_ptr() % 16 == 0
        return t
    store = torch.empty(t.numel() + 4, dtype=torch.float32, device='cuda')
    assert store.data_ptr() % 16 == 0
    out = store[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def check_forecast(fc, va, axis, what, misalign=False, **kw):
    want = forecast64(fc, va, axis is not None)
    f, v = cuda(fc, misalign), cuda(va, misalign)
    for method in METHODS:
        got = verify.forecast_error(f, v, method=method, axis=axis, **kw)
        within(got, value64(want, method), '%s %s' % (what, method))
    return want


# -- routes -------------------------------------------------------------------------------------------------------------------------- #
#: inner shapes: a run of 108 (one group) or 54 (two) is a multiple of neither 4 nor the block -> scalar loads; 4 x 8 = 32 -> 16-byte loads
ROUTES = [((2, 6, 9), None, False, 'scalar_run108'), ((2, 6, 9), 'groups', False, 'scalar_run54'), ((1, 4, 8), None, False, 'vector_run32'),
          ((1, 4, 8), None, True, 'vector_shape_misaligned')]


@pytest.mark.parametrize('inner, grouped, misalign, name', ROUTES, ids=[r[3] for r in ROUTES])
def test_routes_plain_series_and_per_lead(inner, grouped, misalign, name):
    """F = 4, N = Nv = 7 (7, 6, 5, 4 pairs of rows), N = 9 > Nv = 7, and the per-lead layout F = 3, N = 5"""
    fc, va = data((4, 7) + inner, 11, 29), data((7,) + inner, 12, 31)
    check_forecast(fc, va, (0, 2, 3) if grouped else None, name + ' series', misalign)
    check_forecast(data((4, 9) + inner, 13, 29), va, (0, 2, 3) if grouped else None, name + ' series N=9', misalign)
    check_forecast(data((3, 5) + inner, 14, 23), data((3, 5) + inner, 15, 19), (1, 3, 4) if grouped else None, name + ' per lead', misalign)


def test_misaligned_operands_agree_with_each_other_bit_for_bit():
    """one float into the storage the 16-byte route is not allowed: whichever operand is misaligned, the scalar route runs, and the
    scalar route's bits do not depend on which one it was"""
    fc, va = data((3, 5, 1, 4, 8), 21, 17), data((3, 5, 1, 4, 8), 22)
    row = 32
    args = ((5 * row, row, 0), (5 * row, row, 0), 3, 5, 0, 1, row)
    sums = [ops.verify_error_sums(cuda(fc, ma), args[0], cuda(va, mb), *args[1:]) for ma, mb in ((True, True), (True, False), (False, True))]
    assert torch.equal(sums[0].view(torch.int64), sums[1].view(torch.int64)) and torch.equal(sums[0].view(torch.int64), sums[2].view(torch.int64))
    want = forecast64(fc, va, False)
    assert np.array_equal(sums[0].cpu().numpy()[:, 0, 2], want[:, 2])
    aligned = ops.verify_error_sums(cuda(fc), args[0], cuda(va), *args[1:]).cpu().numpy()
    assert np.array_equal(aligned[:, 0, 2], want[:, 2])
    for k in (0, 1):      # the sums themselves: 2^-23 from the rounding of d, the float64 tree far below
        assert (np.abs(aligned[:, 0, k] - want[:, k]) <= BOUND * want[:, k]).all()


def test_leads_beyond_the_verification_series_have_no_pairs():
    """F = 5 with Nv = 3: leads 3 and 4 launch no work and come out NaN with a count of 0"""
    fc, va = data((5, 3, 2, 6, 9), 31), data((3, 2, 6, 9), 32)
    want = check_forecast(fc, va, None, 'F=5 Nv=3')
    assert want[:, 2].tolist() == [3 * 108, 2 * 108, 108, 0, 0]
    got = verify.forecast_error(cuda(fc), cuda(va))
    assert np.isnan(got[3:]).all() and not np.isnan(got[:3]).any()
    plan = verify.plan_forecast(fc.shape, va.shape, (0, 2, 3))
    sums = ops.verify_error_sums(cuda(va), plan.a_strides, cuda(fc), plan.b_strides, 5, 3, 1, 2, 54).cpu().numpy()
    assert sums.shape == (5, 2, 3) and (sums[3:] == 0).all() and sums[:3, :, 2].tolist() == [[162, 162], [108, 108], [54, 54]]
    pe = verify.persistence_error(cuda(fc[0]), cuda(va), 5)
    assert np.isnan(pe[3:]).all() and not np.isnan(pe[:3]).any()


# -- groups, NaN, infinity ----------------------------------------------------------------------------------------------------------- #
def test_groups_with_an_all_nan_group_in_one_lead():
    """both axis tuples with V = 3; group 1 of lead 1 is NaN in every pair: that cell is NaN with count 0, its neighbours untouched"""
    inner = (3, 4, 8)
    fc, va, va5 = data((3, 5) + inner, 41), data((5,) + inner, 42), data((3, 5) + inner, 43)
    fc[1, :, 1] = np.nan
    for valid, axis, what in ((va, (0, 2, 3), 'series'), (va5, (1, 3, 4), 'per lead')):
        want = check_forecast(fc, valid, axis, 'groups ' + what)
        assert want[1, 1, 2] == 0 and (np.delete(want[..., 2].ravel(), 4) > 0).all()
        got = verify.forecast_error(cuda(fc), cuda(valid), axis=axis)
        assert got.shape == (3, 3) and np.isnan(got[1, 1]) and np.isnan(got).sum() == 1
        clean = fc.copy()
        clean[1, :, 1] = 0.0
        ref = verify.forecast_error(cuda(clean), cuda(valid), axis=axis)
        keep = np.ones((3, 3), bool)
        keep[1, 1] = False
        assert np.array_equal(got[keep], ref[keep])            # the neighbours' bits do not see the NaN group


def test_nan_and_infinity_handling_with_exact_counts():
    inner = (2, 4, 8)
    row = 64
    fc, va = data((3, 4) + inner, 51), data((4,) + inner, 52)
    fc[0, 1, 0, 2, 3] = np.nan               # one NaN element in the forecast
    va[2] = np.nan                           # a whole NaN sample row in valid
    plan = verify.plan_forecast(fc.shape, va.shape, None)

    def counts(f, v):
        return ops.verify_error_sums(cuda(v), plan.a_strides, cuda(f), plan.b_strides, 3, 4, 1, 1, row).cpu().numpy()[:, 0]
    want = check_forecast(fc, va, None, 'nan')
    s = counts(fc, va)
    # lead 0: rows 0..3, row 2 of valid NaN, one NaN element; lead 1: valid[1:] has the NaN row; lead 2: valid[2:] has it
    assert s[:, 2].tolist() == want[:, 2].tolist() == [3 * row - 1, 2 * row, row]
    fi, vi = fc.copy(), va.copy()
    fi[1, 0, 1, 0, 0] = np.inf               # an inf in one operand: lead 1 is inf, its count whole
    fi[2, 1, 0, 1, 1] = np.inf               # inf - inf: skipped (pairs with valid[3])
    vi[3, 0, 1, 1] = np.inf
    want = check_forecast(fi, vi, None, 'inf')
    for method in METHODS:
        got = verify.forecast_error(cuda(fi), cuda(vi), method=method)
        assert np.isinf(got[1]) and got[1] > 0 and np.isfinite(got[2])
    s = counts(fi, vi)
    assert s[:, 2].tolist() == want[:, 2].tolist() == [3 * row - 1, 2 * row, row - 1]
    assert np.isinf(s[0, 0]) and np.isinf(s[1, 1]) and np.isfinite(s[2, :2]).all()          # lead 0 sees valid[3]'s inf too


# -- the reduction tree -------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('misalign', [False, True], ids=['vector', 'scalar'])
def test_reduction_tree_many_partials_few_rows_and_repeatable_bits(misalign):
    """F = 3, N = 33, rows of 2 x 64 x 96: every block of the launch has work and the second kernel sums hundreds of partials per
    cell; N = 2: fewer rows than blocks.  Two calls on the same inputs give identical float64 bits.  (One shape per route: routes are
    not compared with each other.)"""
    inner = (2, 64, 96)
    row = 2 * 64 * 96
    for n, seed in ((33, 61), (2, 62)):
        fc, va = data((3, n) + inner, seed, 1013), data((3, n) + inner, seed + 5)
        want = forecast64(fc, va, False)
        f, v = cuda(fc, misalign), cuda(va, misalign)
        st = (n * row, row, 0)
        one = ops.verify_error_sums(f, st, v, st, 3, n, 0, 1, row)
        two = ops.verify_error_sums(f, st, v, st, 3, n, 0, 1, row)
        assert torch.equal(one.view(torch.int64), two.view(torch.int64))
        s = one.cpu().numpy()[:, 0]
        assert np.array_equal(s[:, 2], want[:, 2])
        for method in METHODS:
            within(verify.finish(s[:, None], method, False), value64(want, method), 'tree n=%d %s' % (n, method))
        grouped = ops.verify_error_sums(f, st, v, st, 3, n, 0, 2, row // 2).cpu().numpy()
        for method in METHODS:
            within(verify.finish(grouped, method, True), value64(forecast64(fc, va, True), method), 'tree groups n=%d %s' % (n, method))


# -- persistence, climatology -------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('inner', [(2, 6, 9), (3, 4, 8)], ids=['scalar', 'vector'])
def test_persistence_and_climo_against_float64(inner):
    pr, va = data((8,) + inner, 71, 41), data((6,) + inner, 72, 43)
    va[:, 1, 2, 3] = np.nan                   # a column of valid that is NaN in every sample
    va[4] = np.nan
    for axis in (None, (0, 2, 3)):
        grouped = axis is not None
        for method in METHODS:
            want = value64(persistence64(pr, va, 4, grouped), method)
            within(verify.persistence_error(cuda(pr), cuda(va), 4, method=method, axis=axis), want, 'persistence %s' % method)
            want = value64(climo64(va, 3, grouped), method)
            within(verify.climo_error(cuda(va), 3, method=method, axis=axis), want, 'climo %s' % method)
    # numpy arguments with the keyword, and a mixed pair: the numpy one follows the tensor
    want = value64(persistence64(pr, va, 4, False), 'mse')
    within(verify.persistence_error(pr, va, 4, device='cuda'), want, 'persistence numpy')
    within(verify.persistence_error(cuda(pr), va, 4), want, 'persistence mixed')
    within(verify.persistence_error(pr, cuda(va), 4, device=torch.device('cuda', 0)), want, 'persistence mixed 2')
    # a non-contiguous tensor is made contiguous
    wide = cuda(np.concatenate([pr, pr], axis=-1))
    assert not wide[..., :inner[-1]].is_contiguous()
    within(verify.persistence_error(wide[..., :inner[-1]], cuda(va), 4), want, 'persistence strided')


@pytest.mark.parametrize('shape', [(5, 2, 6, 9), (1, 7), (9, 3, 4, 8), (300, 513)], ids=str)
def test_nanmean_samples_alone(shape):
    """one float32 rounding of a float64 mean (2^-24) and a margin of one more ulp for the float64 sums: 2^-23"""
    x = data(shape, 81, 7)
    x[:, 0] = np.nan                           # columns without a sample
    if shape[0] > 1:
        x[1] = np.nan
    got = ops.verify_nanmean_samples(cuda(x)).cpu().numpy()
    want = nanmean64(x)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0]).all()
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    print('nanmean %s: error / bound %.3f' % (shape, float((err / (2.0 ** -23 * np.abs(want[ok]))).max())))
    assert (err <= 2.0 ** -23 * np.abs(want[ok])).all()


def test_nanmean_samples_follows_ieee_on_infinities():
    x = np.array([[np.inf, np.inf, -np.inf, 1.0], [1.0, 1.0, 1.0, np.nan], [-np.inf, np.inf, 2.0, 3.0]], np.float32)
    got = ops.verify_nanmean_samples(cuda(x)).cpu().numpy()
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == -np.inf and got[3] == 2.0


# -- the golden file ----------------------------------------------------------------------------------------------------------------- #
def test_golden_file_through_the_device_path(golden):
    """every fe_*, pe_* and ce_* array of tests/golden/verify.npz with device='cuda'.  The fixture holds the reference's float32
    results, which are not within 2^-22 of float64 themselves: the allowance is 2^-22 plus the fixture's own distance from the
    float64 restatement of its stored inputs (a triangle inequality).  pe_axis_* (axis=0) runs the host code: equal bits."""
    g = golden('verify')
    fc, va, va5 = g['forecast'], g['valid'], g['valid_steps']
    assert fc.dtype == va.dtype == va5.dtype == np.float32
    for method in METHODS:
        cases = {
            'fe_series_%s': (verify.forecast_error(fc, va, method=method, device='cuda'), forecast64(fc, va, False)),
            'fe_series_axis_%s': (verify.forecast_error(fc, va, method=method, axis=(0, 2, 3), device='cuda'), forecast64(fc, va, True)),
            'fe_steps_%s': (verify.forecast_error(fc, va5, method=method, device='cuda'), forecast64(fc, va5, False)),
            'fe_steps_axis_%s': (verify.forecast_error(fc, va5, method=method, axis=(1, 3, 4), device='cuda'), forecast64(fc, va5, True)),
            'pe_%s': (verify.persistence_error(fc[0], va, 4, method=method, device='cuda'), persistence64(fc[0], va, 4, False)),
            'ce_%s': (verify.climo_error(va, 3, method=method, device='cuda'), climo64(va, 3, False))}
        for key, (got, sums) in cases.items():
            want64, fixture = value64(sums, method), g[key % method]
            assert got.shape == fixture.shape and got.dtype == fixture.dtype, key % method
            assert np.array_equal(np.isnan(fixture), np.isnan(want64)), key % method
            own = np.abs(np.nan_to_num(fixture.astype(np.float64)) - np.nan_to_num(want64))
            within(got, want64, key % method)
            err = np.abs(np.nan_to_num(got.astype(np.float64)) - np.nan_to_num(fixture.astype(np.float64)))
            assert (err <= BOUND * np.abs(np.nan_to_num(want64)) + own).all(), key % method
        host = verify.persistence_error(fc[0], va, 4, method=method, axis=0, device='cuda')
        assert np.array_equal(host, g['pe_axis_%s' % method], equal_nan=True)
        assert np.array_equal(verify.persistence_error(cuda(fc[0]), cuda(va), 4, method=method, axis=0), g['pe_axis_%s' % method],
                              equal_nan=True)


# -- end to end ---------------------------------------------------------------------------------------------------------------------- #
def test_rollout_series_verified_where_it_is():
    """a small convolutional DLWPNeuralNet: 3 samples, 4 channels, 8 x 12, 5 leads; predict_timeseries(..., return_device=True) goes
    into forecast_error as it is.  Device and host path are both within 2^-22 of the float64 restatement on the downloaded series."""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    d.build_model(cnn2_layers((4, 8, 12)), loss='mse', optimizer='adam')
    rng = np.random.default_rng(91)
    x = rng.standard_normal((3, 4, 8, 12)).astype(np.float32)
    series = d.predict_timeseries(x, 5, return_device=True)
    assert series.is_cuda and tuple(series.shape) == (5, 3, 4, 8, 12)
    valid = rng.standard_normal((5, 3, 4, 8, 12)).astype(np.float32)
    host_series = series.cpu().numpy()
    for axis in (None, (1, 3, 4)):
        sums = forecast64(host_series, valid, axis is not None)
        for method in METHODS:
            want = value64(sums, method)
            within(verify.forecast_error(series, valid, method=method, axis=axis), want, 'rollout device %s' % method)
            within(verify.forecast_error(host_series, valid, method=method, axis=axis, device='cuda'), want, 'rollout upload %s' % method)
            within(np.asarray(verify.forecast_error(host_series, valid, method=method, axis=axis)), want, 'rollout host %s' % method)
    # the plain verification series: leads 3 and 4 reach beyond its 3 samples
    plain = rng.standard_normal((3, 4, 8, 12)).astype(np.float32)
    within(verify.forecast_error(series, cuda(plain)), value64(forecast64(host_series, plain, False), 'mse'), 'rollout plain series')
