"""Latitude-weighted forecast skill on the device (csrc/skill.hip behind verify.forecast_skill / persistence_skill) against the float64
restatement of tests/skill_cases.py, inside the bounds derived there: 2^-22 relative for mse / rmse / mae,
2^-23 mae + 2^-24 |bias| for the bias, 2^-21 absolute for acc, 2^-21 kappa for the centred form (kappa <= 2 asserted), equal counts,
equality where the reference is 0, NaN or infinite.  Shapes are the smallest at which each route can go wrong: 16-byte units that
straddle latitude rows (W = 10), the weight index wrapping per channel, scalar loads (odd rows, misaligned storage), a cell of many
blocks.  Run with -s to see error / bound of every case."""
import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import verify
from dlwp_amd.model.generators import LabeledArray, SeriesDataset
from tests.nets import cnn2_layers
from tests.skill_cases import check_skill, cosine, data, forecast64, labels_of, persistence64, table_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


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


def check_forecast(fc, va, table, labels, weights, axis, what, misalign=False):
    ref = forecast64(fc, va, table, labels, weights, axis is not None)
    got = verify.forecast_skill(cuda(fc, misalign), cuda(va, misalign), None if table is None else cuda(table, misalign), labels, weights,
                                axis=axis)
    check_skill(got, ref, what)
    return got


# -- routes -------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_per_lead_valid_units_straddle_latitude_rows(axis):
    """F = 3, N = 5, C = 2, H = 6, W = 10: W % 4 != 0, so the weight is looked up per element; with axis=None the run holds both
    channels and the weight index wraps; 150 (75 per group) units for 256 threads"""
    inner = (2, 6, 10)
    check_forecast(data((3, 5) + inner, 31), data((3, 5) + inner, 32), table_of(inner, 33), labels_of((3, 5), 34), cosine(6), axis,
                   'per lead %s' % (axis,))


@pytest.mark.parametrize('axis', [None, (0, 2, 3)], ids=['all', 'groups'])
def test_plain_series_shrinking_counts_and_leads_without_pairs(axis):
    """F = 7, Nv = 5, N = 6: 5, 4, .. 1 pairs of rows, leads 5 and 6 none; labels (Nv,)"""
    inner = (2, 6, 10)
    got = check_forecast(data((7, 6) + inner, 35), data((5,) + inner, 36), table_of(inner, 37), labels_of((5,), 38), cosine(6), axis,
                         'plain series %s' % (axis,))
    assert (got.count[5:] == 0).all() and np.isnan(got.acc[5:]).all() and np.isnan(got.rmse[5:]).all()


@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['run90', 'run45'])
def test_scalar_route_odd_rows(axis):
    inner = (2, 5, 9)
    check_forecast(data((3, 5) + inner, 39), data((3, 5) + inner, 40), table_of(inner, 41), labels_of((3, 5), 42), cosine(5), axis,
                   'scalar %s' % (axis,))


@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_scalar_route_misaligned_storage(axis):
    inner = (2, 6, 10)
    check_forecast(data((3, 5) + inner, 31), data((3, 5) + inner, 32), table_of(inner, 33), labels_of((3, 5), 34), cosine(6), axis,
                   'misaligned %s' % (axis,), misalign=True)


@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_vector_route_one_weight_per_unit(axis):
    """W = 12: a 16-byte unit lies inside one latitude row and the weight is looked up once per unit"""
    inner = (2, 6, 12)
    check_forecast(data((3, 5) + inner, 43), data((3, 5) + inner, 44), table_of(inner, 45), labels_of((3, 5), 46), cosine(6), axis,
                   'unit weight %s' % (axis,))


# -- NaN handling -------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_nan_pairs_nan_table_rows_absent_and_skipped_labels(axis):
    """every 7th forecast and every 11th truth element NaN; table row 4 all NaN (its pairs are skipped and counted out); label 9
    absent; one label -1; every pair of lead 2 skipped (labels 4 and -1 only)"""
    inner = (2, 6, 10)
    fc, va = data((4, 5) + inner, 47, 7), data((4, 5) + inner, 48, 11)
    table = table_of(inner, 49)
    table[4] = np.nan
    labels = labels_of((4, 5), 50)
    labels[labels == 9] = 3
    labels[0, 1], labels[1, 0], labels[3, 4] = 4, 4, -1
    labels[2] = [4, -1, 4, 4, -1]
    got = check_forecast(fc, va, table, labels, cosine(6), axis, 'nan %s' % (axis,))
    assert (got.count[2] == 0).all() and np.isnan(got.mse[2]).all() and np.isnan(got.acc_centered[2]).all()
    full = 2 * 6 * 10 // (1 if axis is None else 2) * 5
    assert (got.count[[0, 1, 3]] > 0).all() and (got.count < full * 4 // 5).all()


def test_infinities_follow_ieee():
    inner = (1, 4, 8)
    fc, va = data((2, 3) + inner, 51), data((2, 3) + inner, 52)
    fc[0, 1, 0, 2, 3] = np.inf                      # d = fa = inf: the sums of lead 0 that hold them become inf, S6 = inf * oa
    fc[1, 0, 0, 1, 1], va[1, 0, 0, 1, 1] = np.inf, np.inf          # d = inf - inf = NaN: skipped
    ref = forecast64(fc, va)
    got = verify.forecast_skill(cuda(fc), cuda(va))
    assert got.count.tolist() == ref.count.tolist() == [96, 95]
    assert np.isinf(got.mse[0]) and np.isinf(got.mae[0]) and np.isinf(got.bias[0]) and np.isnan(got.acc[0])
    check_skill(got, ref, 'infinities')


# -- optional arguments -------------------------------------------------------------------------------------------------------------- #
def test_optional_arguments_each_alone_and_all_absent():
    inner = (2, 6, 10)
    fc, va = data((3, 5) + inner, 53, 13), data((3, 5) + inner, 54)
    table, labels, w = table_of(inner, 55), labels_of((3, 5), 56), cosine(6)
    for axis in (None, (1, 3, 4)):
        check_forecast(fc, va, None, None, None, axis, 'bare %s' % (axis,))
        check_forecast(fc, va, table, labels, None, axis, 'no weights %s' % (axis,))
        check_forecast(fc, va, None, None, w, axis, 'no climatology %s' % (axis,))
        check_forecast(fc, va, table[5], None, w, axis, 'one field %s' % (axis,))


# -- the tree ------------------------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope='module')
def large():
    """one lead, N = 160 samples of 4 x 44 x 92 (10.4 MB per operand): every thread's loop runs more than once, many blocks per cell"""
    inner = (4, 44, 92)
    fc, va = data((1, 160) + inner, 57, 1013), data((1, 160) + inner, 58)
    table, labels, w = table_of(inner, 59), labels_of((1, 160), 60), cosine(44)
    refs = {grouped: forecast64(fc, va, table, labels, w, grouped) for grouped in (False, True)}
    return cuda(fc), cuda(va), cuda(table), labels, w, refs


@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_cells_of_many_blocks(large, axis):
    fc, va, table, labels, w, refs = large
    check_skill(verify.forecast_skill(fc, va, table, labels, w, axis=axis), refs[axis is not None], 'many blocks %s' % (axis,))


def test_repeated_calls_give_identical_bits(large):
    fc, va, table, labels, w, _ = large
    row = 4 * 44 * 92
    st = (160 * row, row, 0)
    args = dict(climo=table, labels=labels, label_strides=(160, 0), weights=w, w_inner=92)
    one = ops.verify_skill_sums(fc, st, va, st, 1, 160, 0, 1, row, **args)
    two = ops.verify_skill_sums(fc, st, va, st, 1, 160, 0, 1, row, **args)
    assert one.shape == (1, 1, 10) and one.dtype == torch.float64 and torch.equal(one, two)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))


@pytest.mark.parametrize('inner, misalign', [((4, 44, 92), False), ((2, 6, 10), False), ((2, 5, 9), False), ((2, 6, 10), True)],
                         ids=['many_blocks', 'vector', 'scalar', 'misaligned'])
def test_against_the_parent_kernel_without_weights_and_climatology(inner, misalign):
    """sum d^2, sum |d| and the count are those of dlwp_verify_error_sums: two float64 trees over fewer than 2^23 non-negative terms
    differ by at most n 2^-53 each, far below 2^-30; the counts are equal"""
    n = 40 if inner[1] == 44 else 5
    fc, va = cuda(data((3, n) + inner, 61, 17), misalign), cuda(data((3, n) + inner, 62, 19), misalign)
    row = int(np.prod(inner))
    st = (n * row, row, 0)
    for groups in (1, inner[0]):
        mine = ops.verify_skill_sums(fc, st, va, st, 3, n, 0, groups, row // groups).cpu().numpy()
        parent = ops.verify_error_sums(fc, st, va, st, 3, n, 0, groups, row // groups).cpu().numpy()
        assert np.array_equal(mine[..., 9], parent[..., 2]) and np.array_equal(mine[..., 0], mine[..., 9])
        for k, j in ((2, 0), (3, 1)):
            assert (np.abs(mine[..., k] - parent[..., j]) <= 2.0 ** -30 * parent[..., j]).all(), (groups, k)


# -- persistence --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('axis', [None, (0, 2, 3)], ids=['all', 'groups'])
def test_persistence_skill(axis):
    inner = (2, 6, 10)
    pr, va = data((6,) + inner, 63), data((6,) + inner, 64, 23)
    table, labels, w = table_of(inner, 65), labels_of((6,), 66), cosine(6)
    got = verify.persistence_skill(cuda(pr), cuda(va), 4, cuda(table), labels, w, axis=axis)
    check_skill(got, persistence64(pr, va, 4, table, labels, w, axis is not None), 'persistence %s' % (axis,))
    again = verify.persistence_skill(pr, va, 4, table, labels, w, axis=axis, device='cuda')
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))


# -- end to end ---------------------------------------------------------------------------------------------------------------------- #
def test_rollout_scored_where_it_is_against_a_monthly_climatology():
    """2 initial dates, 3 leads, a 2 x 8 x 12 state: predict_timeseries(..., return_device=True), verification_tensor and the monthly
    table stay in HBM; the device scores lie inside the bounds of the float64 restatement on the downloaded arrays, and so does the
    host path; numpy arguments with device='cuda' give the values of the tensor arguments"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    d.build_model(cnn2_layers((2, 8, 12)), loss='mse', optimizer='adam')
    rng = np.random.default_rng(67)
    times = np.datetime64('2010-01-25T00') + (np.arange(12) * 6).astype('timedelta64[h]') + np.repeat([0, 40], 6).astype('timedelta64[D]')
    record = rng.standard_normal((12, 2, 8, 12)).astype(np.float32)
    dims = ('sample', 'varlev', 'lat', 'lon')
    all_ds = SeriesDataset(record, {'sample': times}, dims)
    ds = SeriesDataset(record[:2], {'sample': times[:2]}, dims)
    series = d.predict_timeseries(record[:2], 3, return_device=True)
    vt = verify.verification_tensor(ds, all_ds=all_ds, forecast_steps=3, dt=6)
    assert series.is_cuda and vt.is_cuda and tuple(series.shape) == tuple(vt.shape) == (3, 2, 2, 8, 12)
    da = LabeledArray(torch.from_numpy(record).cuda(), {'sample': times}, dims)
    table = verify.monthly_climatology(da)
    assert isinstance(table, torch.Tensor) and table.is_cuda and tuple(table.shape) == (12, 2, 8, 12)
    host_table = verify.monthly_climatology(LabeledArray(record, {'sample': times}, dims))
    assert np.array_equal(table.cpu().numpy().view(np.int32), host_table.view(np.int32))
    uploaded = verify.monthly_climatology(LabeledArray(record, {'sample': times}, dims), device='cuda')
    assert isinstance(uploaded, np.ndarray) and np.array_equal(uploaded.view(np.int32), host_table.view(np.int32))
    valid_times = times[:2][None, :] + ((np.arange(3) + 1) * 6).astype('timedelta64[h]')[:, None]
    labels = verify.month_labels(valid_times)
    assert labels.shape == (3, 2) and set(labels.ravel().tolist()) == {0}          # January; the record's other half lies in March
    labels[2, 1] = 2
    w = verify.area_weights(np.linspace(-70, 70, 8))
    host_series, host_valid = series.cpu().numpy(), vt.cpu().numpy()
    for axis in (None, (1, 3, 4)):
        ref = forecast64(host_series, host_valid, host_table, labels, w, axis is not None)
        got = verify.forecast_skill(series, vt, table, labels, w, axis=axis)
        check_skill(got, ref, 'rollout device %s' % (axis,))
        check_skill(verify.forecast_skill(host_series, host_valid, host_table, labels, w, axis=axis), ref, 'rollout host %s' % (axis,))
        again = verify.forecast_skill(host_series, host_valid, host_table, labels, w, axis=axis, device='cuda')
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))


# -- refusals ------------------------------------------------------------------------------------------------------------------------ #
def test_wrapper_refusals_launch_nothing():
    row = 2 * 6 * 10
    fc, va = cuda(data((3, 5, 2, 6, 10), 68)), cuda(data((3, 5, 2, 6, 10), 69))
    table, labels, w = cuda(table_of((2, 6, 10), 70)), labels_of((3, 5), 71), cosine(6)
    st = (5 * row, row, 0)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='operand ob holds 1800 elements, the strides address 2040'):
        ops.verify_skill_sums(fc, st, va, (5 * row, row, 1), 3, 5, 0, 1, row)
    with pytest.raises(ValueError, match='operand fc holds'):
        ops.verify_skill_sums(fc[:2], st, va, st, 3, 5, 0, 1, row)
    with pytest.raises(ValueError, match='15 labels, the strides address 17'):
        ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 1, row, climo=table, labels=labels, label_strides=(5, 1))
    with pytest.raises(ValueError, match='labels without'):
        ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 1, row, labels=labels, label_strides=(5, 0))
    with pytest.raises(ValueError, match='do not divide a run of 60'):
        ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 2, row // 2, weights=w, w_inner=20)
    with pytest.raises(ValueError, match='do not divide'):
        ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 1, row, weights=np.ones(7, np.float32), w_inner=10)
    with pytest.raises(ValueError, match=r'\[-1, 12\)'):
        ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 1, row, climo=table, labels=labels + 12, label_strides=(5, 0))
    with pytest.raises(ValueError, match='table rows of 60 floats'):
        ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 1, row, climo=table.view(24, 60))
    # and the same arguments, valid, run
    out = ops.verify_skill_sums(fc, st, va, st, 3, 5, 0, 1, row, climo=table, labels=labels, label_strides=(5, 0), weights=w, w_inner=10)
    assert tuple(out.shape) == (3, 1, 10) and (out[..., 9] == 5 * row).all()
