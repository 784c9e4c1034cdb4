"""Per-grid-point forecast skill on the device (csrc/skill_map.hip behind verify.forecast_skill_map / persistence_skill_map /
skill_map_sums / finish_skill_map) against the float64 restatement of tests/skill_map_cases.py, inside the bounds derived in
tests/skill_cases.py and asserted per point: 2^-22 relative for mse / rmse / mae, 2^-23 mae + 2^-24 |bias| for the bias, 2^-21 absolute
for acc, 2^-21 kappa for the centred form (kappa <= 2 asserted), equal counts, equality where the reference is 0, NaN or infinite.
Shapes are the smallest at which each route can go wrong: fewer 16-byte units than lanes, scalar loads (odd rows, misaligned storage),
several blocks per lead, every chunk count.  A lead has 0, 1 or at least 63 samples.  Run with -s to see error / bound of every case."""
import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import verify
from dlwp_amd.model.generators import LabeledArray, SeriesDataset
from tests.nets import cnn2_layers
from tests.skill_cases import cosine, data, labels_of, table_of
from tests.skill_map_cases import check_skill_map, forecast_map64, persistence_map64, term_magnitudes, weighted_plane_sums

pytestmark = pytest.mark.gpu
N = 64


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


def check_forecast(fc, va, table, labels, what, misalign=False):
    ref = forecast_map64(fc, va, table, labels)
    got = verify.forecast_skill_map(cuda(fc, misalign), cuda(va, misalign), None if table is None else cuda(table, misalign), labels)
    return check_skill_map(got, ref, what, on_device=True)


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# -- routes -------------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope='module')
def small():
    """2 leads x 64 samples of 2 x 6 x 10 with a 12-month table: 30 units of 16 bytes for 64 lanes"""
    inner = (2, 6, 10)
    fc, va = data((2, N) + inner, 31), data((2, N) + inner, 32)
    table, labels = table_of(inner, 33), labels_of((2, N), 34)
    return fc, va, table, labels, forecast_map64(fc, va, table, labels)


def test_per_lead_valid_fewer_units_than_lanes(small):
    fc, va, table, labels, ref = small
    got = check_skill_map(verify.forecast_skill_map(cuda(fc), cuda(va), cuda(table), labels), ref, 'per lead', on_device=True)
    assert got.rmse.shape == (2, 2, 6, 10) and (got.count == N).all()


def test_scalar_route_odd_rows():
    inner = (2, 5, 9)
    check_forecast(data((2, N) + inner, 39), data((2, N) + inner, 40), table_of(inner, 41), labels_of((2, N), 42), 'scalar, odd rows')


def test_scalar_route_misaligned_storage_has_the_bits_of_the_vector_route(small):
    """every operand one float into its storage; a point adds the same samples in the same order on either route"""
    fc, va, table, labels, ref = small
    check_skill_map(verify.forecast_skill_map(cuda(fc, True), cuda(va, True), cuda(table, True), labels), ref, 'misaligned', True)
    a = verify.skill_map_sums(cuda(fc, True), cuda(va, True), cuda(table, True), labels, split=1)
    b = verify.skill_map_sums(cuda(fc), cuda(va), cuda(table), labels, split=1)
    assert torch.equal(bits(a), bits(b))


def test_several_blocks_per_lead():
    """4 x 44 x 92 = 16192 points: 16 blocks of 16-byte units per lead and chunk.  The table lies around the mean of the data (1), as a
    climatology does: among 32384 points of 64 samples kappa would pass 2 somewhere otherwise"""
    inner = (4, 44, 92)
    table = table_of(inner, 59) + np.float32(1)
    check_forecast(data((2, N) + inner, 57, 1013), data((2, N) + inner, 58), table, labels_of((2, N), 60), 'several blocks')


def test_plain_series_shrinking_counts():
    """70 verification times, 8 leads: 70 .. 63 samples per point, labels (Nv,)"""
    inner = (2, 6, 10)
    fc, va = data((8, 72) + inner, 35), data((70,) + inner, 36)
    got = check_forecast(fc, va, table_of(inner, 37), labels_of((70,), 38), 'plain series')
    assert [int(c) for c in got.count[:, 1, 2, 3]] == [70, 69, 68, 67, 66, 65, 64, 63]
    check_forecast(fc, va, None, None, 'plain series bare')


def test_one_sample_and_two_leads_beyond_the_series():
    """one verification time, three leads: lead 0 has exactly one pair per point -- a variance of exactly zero on both sides, so the
    centred correlation is NaN and the errors are not; leads 1 and 2 lie beyond the series: zero sums, NaN scores, count 0"""
    inner = (2, 6, 10)
    fc, va = data((3, 2) + inner, 43), data((1,) + inner, 44)
    got = check_forecast(fc, va, None, None, 'one sample')
    assert (got.count[0] == 1).all() and (got.count[1:] == 0).all() and np.isnan(got.acc_centered).all()
    assert not np.isnan(got.rmse[0]).any() and np.isnan(got.rmse[1:]).all() and np.isnan(got.acc[1:]).all()
    sums = verify.skill_map_sums(cuda(fc), cuda(va))
    assert sums.is_cuda and tuple(sums.shape) == (3, 9) + inner and (sums[1:] == 0).all() and (sums[0, 8] == 1).all()


# -- chunks of the sample axis ------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('split', [1, 2, 3, N, 0])
def test_every_split_is_inside_the_bounds_and_repeats_its_bits(small, split):
    """3 chunks of 64 samples are uneven (21, 21, 22); 64 chunks hold one sample each; 0 lets the library choose (2 leads x 1 tile do
    not fill a chip: it splits)"""
    fc, va, table, labels, ref = small
    args = (cuda(fc), cuda(va), cuda(table), labels)
    one = verify.skill_map_sums(*args, split=split)
    two = verify.skill_map_sums(*args, split=split)
    assert one.dtype == torch.float64 and tuple(one.shape) == (2, 9, 2, 6, 10) and torch.equal(bits(one), bits(two))
    check_skill_map(verify.finish_skill_map(one), ref, 'split %d' % split, on_device=True)
    check_skill_map(verify.finish_skill_map(one.cpu().numpy()), ref, 'split %d, host finish' % split, on_device=False)
    assert torch.equal(one[:, 8], torch.full_like(one[:, 8], N))
    # the scores of the same launch
    row = 2 * 6 * 10
    st = (N * row, row, 0)
    _, scores, counts = ops.verify_skill_map(args[0], st, args[1], st, 2, N, 0, row, climo=args[2], labels=labels, label_strides=(N, 0),
                                             split=split, want_sums=False)
    again = ops.verify_skill_map(args[0], st, args[1], st, 2, N, 0, row, climo=args[2], labels=labels, label_strides=(N, 0),
                                 split=split, want_sums=False)
    assert torch.equal(bits(scores), bits(again[1])) and torch.equal(counts, again[2])
    got = verify.Skill(*([scores[:, k].reshape(2, 2, 6, 10) for k in range(6)] + [counts.reshape(2, 2, 6, 10).to(torch.int64)]))
    check_skill_map(got, ref, 'split %d, scores only' % split, on_device=True)


# -- NaN handling -------------------------------------------------------------------------------------------------------------------- #
def test_nan_pairs_nan_table_rows_absent_and_skipped_labels():
    """every 7th forecast and every 11th truth element NaN; table row 4 all NaN (its pairs are skipped and counted out); label 9
    absent; labels -1; every pair of lead 2 skipped (labels 4 and -1 only); 160 samples keep at least 64 counted at every point"""
    inner = (2, 6, 10)
    n = 160
    fc, va = data((3, n) + inner, 47, 7), data((3, n) + inner, 48, 11)
    table = table_of(inner, 49)
    table[4] = np.nan
    labels = labels_of((3, n), 50)
    labels[labels == 9] = 3
    labels[0, 1], labels[1, 0], labels[1, 159] = -1, -1, -1
    labels[2] = np.where(np.arange(n) % 3 == 0, -1, 4)
    got = check_forecast(fc, va, table, labels, 'nan')
    assert (got.count[2] == 0).all() and np.isnan(got.mse[2]).all() and np.isnan(got.acc_centered[2]).all()
    assert (got.count[:2] >= 64).all() and (got.count[:2] < n).all() and len(np.unique(got.count[:2])) > 1


def test_infinities_follow_ieee():
    inner = (1, 4, 8)
    fc, va = data((2, N) + inner, 51), data((2, N) + inner, 52)
    fc[0, 1, 0, 2, 3] = np.inf                      # d = fa = inf: the sums of that point that hold them become inf
    fc[1, 0, 0, 1, 1], va[1, 0, 0, 1, 1] = np.inf, np.inf          # d = inf - inf = NaN: skipped at that point only
    ref = forecast_map64(fc, va)
    got = check_skill_map(verify.forecast_skill_map(cuda(fc), cuda(va)), ref, 'infinities', on_device=True)
    assert got.count[1, 0, 1, 1] == N - 1 and (got.count.sum() == 2 * N * 32 - 1)
    assert np.isinf(got.mse[0, 0, 2, 3]) and np.isinf(got.bias[0, 0, 2, 3]) and np.isnan(got.acc[0, 0, 2, 3])
    assert np.isfinite(got.mse).sum() == got.mse.size - 1


# -- arguments and outputs ----------------------------------------------------------------------------------------------------------- #
def test_optional_arguments_each_alone_and_all_absent():
    inner = (2, 6, 10)
    fc, va = data((2, N) + inner, 53, 13), data((2, N) + inner, 54)
    table, labels = table_of(inner, 55), labels_of((2, N), 56)
    check_forecast(fc, va, None, None, 'bare')
    check_forecast(fc, va, table, labels, 'table and labels')
    near = table + np.float32(1)                    # around the mean of the data: one row for every sample must not push kappa past 2
    check_forecast(fc, va, near[5], None, 'one field')
    check_forecast(fc, va, near[:1], np.zeros((2, N), np.int64), 'a table of one row with labels')


def test_output_selection_and_device_scores_against_the_finished_table(small):
    """sums only, scores only, and the device scores against finish_skill_map of the downloaded sums: mse, mae, bias and the count are
    one float64 division and a cast each -- the same bits; the others are held to the bounds"""
    fc, va, table, labels, ref = small
    row = 2 * 6 * 10
    st = (N * row, row, 0)
    args = dict(climo=cuda(table), labels=labels, label_strides=(N, 0), split=1)
    fcd, vad = cuda(fc), cuda(va)
    sums, none_a, none_b = ops.verify_skill_map(fcd, st, vad, st, 2, N, 0, row, want_scores=False, **args)
    assert none_a is None and none_b is None and tuple(sums.shape) == (2, 9, row) and sums.dtype == torch.float64
    none_c, scores, counts = ops.verify_skill_map(fcd, st, vad, st, 2, N, 0, row, want_sums=False, **args)
    assert none_c is None and tuple(scores.shape) == (2, 6, row) and scores.dtype == torch.float32 and counts.dtype == torch.int32
    host = verify.finish_skill_map(sums.cpu().numpy().reshape(2, 9, 2, 6, 10))
    dev = scores.cpu().numpy().reshape(2, 6, 2, 6, 10)
    for k, name in ((0, 'mse'), (2, 'mae'), (3, 'bias')):
        assert np.array_equal(dev[:, k].view(np.int32), getattr(host, name).view(np.int32)), name
    assert np.array_equal(counts.cpu().numpy().reshape(2, 2, 6, 10), host.count)
    check_skill_map(verify.Skill(*([dev[:, k] for k in range(6)] + [host.count])), ref, 'scores only', on_device=False)
    # the device's own finish of the same table: the same kernel code, the same bits as the fused launch
    fin_scores, fin_counts = ops.verify_skill_map_finish(sums)
    assert torch.equal(bits(fin_scores), bits(scores)) and torch.equal(fin_counts, counts)


def test_added_tables_finish_on_the_device():
    inner = (2, 6, 10)
    fc, va = data((2, 2 * N) + inner, 61, 17), data((2, 2 * N) + inner, 62)
    table, labels = table_of(inner, 63), labels_of((2, 2 * N), 64)
    a = verify.skill_map_sums(cuda(fc[:, :N]), cuda(va[:, :N]), cuda(table), labels[:, :N])
    b = verify.skill_map_sums(cuda(fc[:, N:]), cuda(va[:, N:]), cuda(table), labels[:, N:])
    check_skill_map(verify.finish_skill_map(a + b), forecast_map64(fc, va, table, labels), 'added tables', on_device=True)


def test_weighted_planes_add_up_to_the_sums_of_the_per_lead_kernel():
    """sum over points of w_e x plane k against dlwp_verify_skill_sums on the same tensors, within n 2^-52 sum |term|"""
    inner = (2, 6, 10)
    fc, va = data((2, N) + inner, 65, 13), data((2, N) + inner, 66)
    table, labels, w = table_of(inner, 67), labels_of((2, N), 68), cosine(6)
    labels[0, 5] = -1
    row = 2 * 6 * 10
    st = (N * row, row, 0)
    fcd, vad, td = cuda(fc), cuda(va), cuda(table)
    want = ops.verify_skill_sums(fcd, st, vad, st, 2, N, 0, 1, row, climo=td, labels=labels, label_strides=(N, 0), weights=w,
                                 w_inner=10).cpu().numpy()[:, 0]
    w_e = np.broadcast_to(w.astype(np.float64).reshape(1, 6, 1), inner)
    got = weighted_plane_sums(verify.skill_map_sums(fcd, vad, td, labels).cpu().numpy(), w_e)
    bound = N * row * 2.0 ** -52 * term_magnitudes(fc, va, table, labels, w_e)
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
    assert np.array_equal(got[:, 9], want[:, 9])


# -- persistence --------------------------------------------------------------------------------------------------------------------- #
def test_persistence_skill_map():
    inner = (2, 6, 10)
    pr, va = data((70,) + inner, 69), data((68,) + inner, 70, 23)
    table, labels = table_of(inner, 71), labels_of((68,), 72)
    got = verify.persistence_skill_map(cuda(pr), cuda(va), 4, cuda(table), labels)
    got = check_skill_map(got, persistence_map64(pr, va, 4, table, labels), 'persistence', on_device=True)
    again = verify.persistence_skill_map(pr, va, 4, table, labels, device='cuda')
    assert all(isinstance(v, np.ndarray) for v in again)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))


# -- end to end ---------------------------------------------------------------------------------------------------------------------- #
def test_rollout_mapped_where_it_is_against_a_monthly_climatology():
    """64 initial dates, 2 leads, a 2 x 8 x 12 state: predict_timeseries(..., return_device=True), verification_tensor and the monthly
    table stay in HBM and so do the maps; device and host path lie inside the bounds of the float64 restatement on the downloaded
    arrays; numpy arguments with device='cuda' give the values of the tensor arguments, as numpy arrays"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    d.build_model(cnn2_layers((2, 8, 12)), loss='mse', optimizer='adam')
    rng = np.random.default_rng(67)
    n = 64
    times = np.datetime64('2010-01-10T00') + (np.arange(n + 2) * 6).astype('timedelta64[h]')      # 16.5 days: January only
    record = rng.standard_normal((n + 2, 2, 8, 12)).astype(np.float32)
    # kappa <= 2 is a condition on the inputs: an untrained net answers N(0, 1) states with fields of a standard deviation near 0.2
    # around zero, so the climatology (the mean of the record: every time lies in January) has to be small beside that.  The record
    # is centred and given a mean field of 0.02 N(0, 1): kappa is about 1 + (0.02 z)^2 / 0.03 at every point
    record -= record.mean(axis=0, keepdims=True)
    record += np.float32(0.02) * rng.standard_normal((2, 8, 12)).astype(np.float32)
    dims =('sample', 'varlev', 'lat', 'lon')
    all_ds = SeriesDataset(record, {'sample': times}, dims)
    ds = SeriesDataset(record[:n], {'sample': times[:n]}, dims)
    series = d.predict_timeseries(record[:n], 2, return_device=True)
    vt = verify.verification_tensor(ds, all_ds=all_ds, forecast_steps=2, dt=6)
    assert series.is_cuda and vt.is_cuda and tuple(series.shape) == tuple(vt.shape) == (2, n, 2, 8, 12)
    table = verify.monthly_climatology(LabeledArray(torch.from_numpy(record).cuda(), {'sample': times}, dims))
    assert isinstance(table, torch.Tensor) and table.is_cuda and tuple(table.shape) == (12, 2, 8, 12)
    valid_times = times[:n][None, :] + ((np.arange(2) + 1) * 6).astype('timedelta64[h]')[:, None]
    labels = verify.month_labels(valid_times)
    assert labels.shape == (2, n) and set(labels.ravel().tolist()) == {0}
    host_series, host_valid, host_table = series.cpu().numpy(), vt.cpu().numpy(), table.cpu().numpy()
    ref = forecast_map64(host_series, host_valid, host_table, labels)
    got = check_skill_map(verify.forecast_skill_map(series, vt, table, labels), ref, 'rollout device', on_device=True)
    check_skill_map(verify.forecast_skill_map(host_series, host_valid, host_table, labels), ref, 'rollout host', on_device=False)
    again = verify.forecast_skill_map(host_series, host_valid, host_table, labels, device='cuda')
    assert all(isinstance(v, np.ndarray) for v in again)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))


# -- refusals ------------------------------------------------------------------------------------------------------------------------ #
def test_wrapper_refusals_launch_nothing():
    row = 2 * 6 * 10
    fc, va = cuda(data((3, 5, 2, 6, 10), 68)), cuda(data((3, 5, 2, 6, 10), 69))
    table, labels = cuda(table_of((2, 6, 10), 70)), labels_of((3, 5), 71)
    st = (5 * row, row, 0)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='operand ob holds 1800 elements, the strides address 2040'):
        ops.verify_skill_map(fc, st, va, (5 * row, row, 1), 3, 5, 0, row)
    with pytest.raises(ValueError, match='operand fc holds'):
        ops.verify_skill_map(fc[:2], st, va, st, 3, 5, 0, row)
    with pytest.raises(ValueError, match='15 labels, the strides address 17'):
        ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, climo=table, labels=labels, label_strides=(5, 1))
    with pytest.raises(ValueError, match='labels without'):
        ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, labels=labels, label_strides=(5, 0))
    with pytest.raises(ValueError, match=r'\[-1, 12\)'):
        ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, climo=table, labels=labels + 12, label_strides=(5, 0))
    with pytest.raises(ValueError, match='table rows of 60 floats'):
        ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, climo=table.view(24, 60))
    with pytest.raises(ValueError, match='split must be >= 0'):
        ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, split=-1)
    with pytest.raises(ValueError, match='neither sums nor scores'):
        ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, want_sums=False, want_scores=False)
    with pytest.raises(ValueError, match='leads and row must be >= 1'):
        ops.verify_skill_map(fc, st, va, st, 0, 5, 0, row)
    # and the same arguments, valid, run
    sums, scores, counts = ops.verify_skill_map(fc, st, va, st, 3, 5, 0, row, climo=table, labels=labels, label_strides=(5, 0))
    assert tuple(sums.shape) == (3, 9, row) and tuple(scores.shape) == (3, 6, row) and (counts == 5).all() and (sums[:, 8] == 5).all()
