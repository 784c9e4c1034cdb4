"""dlwp_amd.model.ensemble without a GPU: the host path against the brute-force float64 restatement of tests/ensemble_cases.py (its
docstring derives the bound), closed forms, both member layouts, the NaN rule, ties, argument errors and the axis rule."""
import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import ensemble
from tests.ensemble_cases import (check_scores, ensemble as make_ensemble, member_order_mean32, scores64, spread_field64, verification,
                                  within)


@pytest.mark.parametrize('members', [2, 3, 5, 32, 33, 100])
def test_host_path_against_the_brute_force_restatement(members):
    x = make_ensemble((3, 2, members, 2, 5, 7), 100 + members)
    y = verification(x, 200 + members)
    for axis, grouped in ((None, False), ((1, 3, 4), True)):
        res = ensemble.ensemble_scores(x, y, axis=axis, crps_field=True)
        assert isinstance(res.crps_field, np.ndarray) and res.rank_hist.shape == ((3, 2) if grouped else (3,)) + (members + 1,)
        check_scores(res, scores64(x, y, grouped), 'host M=%d grouped=%s' % (members, grouped), res.crps_field)
        assert (res.count == (2 * 35 if grouped else 2 * 70)).all()
        ratio = res.spread.astype(np.float64) / res.rmse_mean.astype(np.float64)
        assert np.allclose(res.spread_skill, ratio, rtol=2.0 ** -22, atol=0)
    assert ensemble.ensemble_scores(x, y).crps_field is None
    for ddof in (0, 1):
        mean, spread = ensemble.ensemble_mean_spread(x, ddof=ddof)
        assert mean.dtype == spread.dtype == np.float32 and mean.shape == spread.shape == (3, 2, 2, 5, 7)
        assert np.array_equal(mean, member_order_mean32(x))
        want, allowance = spread_field64(x, ddof)
        within(spread, want, allowance, 'host spread field M=%d ddof=%d' % (members, ddof))
        res = ensemble.ensemble_scores(x, y, ddof=ddof)
        within(res.spread, *scores64(x, y, False, ddof)['spread'], 'host spread M=%d ddof=%d' % (members, ddof))


def test_closed_forms():
    # M = 2: members a, b and y: A = (|a - y| + |b - y|) / 2, B = |a - b|, var_1 = (a - b)^2 / 2
    a, b, yv = np.float32(1.5), np.float32(-0.25), np.float32(0.75)
    x = np.empty((1, 1, 2, 1, 1, 3), np.float32)
    x[:, :, 0], x[:, :, 1] = a, b
    y = np.full((1, 1, 1, 1, 3), yv, np.float32)
    res = ensemble.ensemble_scores(x, y, crps_field=True)
    A, B = (abs(a - yv) + abs(b - yv)) / 2.0, abs(float(a) - float(b))
    assert res.crps[0] == np.float32(A - B / 4.0) and res.fair_crps[0] == np.float32(A - B / 2.0)
    assert res.rmse_mean[0] == res.mae_mean[0] == np.float32(abs((float(a) + float(b)) / 2.0 - yv))
    assert res.spread[0] == np.float32(np.sqrt((float(a) - float(b)) ** 2 / 2.0))
    assert res.rank_hist[0].tolist() == [0, 3, 0] and res.count[0] == 3
    assert np.array_equal(res.crps_field, np.full(y.shape, np.float32(A - B / 4.0)))
    # all members equal to y: crps 0, rank 0, spread 0
    x = np.full((2, 3, 7, 2, 3, 4), np.float32(0.3), np.float32)
    y = np.full((2, 3, 2, 3, 4), np.float32(0.3), np.float32)
    res = ensemble.ensemble_scores(x, y)
    assert (res.crps == 0).all() and (res.fair_crps == 0).all() and (res.spread == 0).all() and (res.rmse_mean == 0).all()
    assert (res.rank_hist[:, 0] == 72).all() and (res.rank_hist[:, 1:] == 0).all()
    assert np.isnan(res.spread_skill).all()                     # 0 / 0
    mean, spread = ensemble.ensemble_mean_spread(x)
    assert (spread == 0).all() and np.array_equal(mean, member_order_mean32(x))
    # y below / above every member: rank 0 / M
    x = make_ensemble((2, 2, 9, 1, 4, 5), 7, spread=1.0)
    for yv, r in ((x.min() - 1, 0), (x.max() + 1, 9)):
        res = ensemble.ensemble_scores(x, np.full((2, 2, 1, 4, 5), yv, np.float32))
        assert (res.rank_hist[:, r] == 40).all() and res.rank_hist.sum() == 80
    # fair_crps - crps = B / (M^2 (M - 1)) per column, so for the means too
    y = verification(x, 8, spread=1.0)
    res = ensemble.ensemble_scores(x, y)
    xd = x.astype(np.float64)
    B = sum(np.abs(xd[:, :, i] - xd[:, :, j]) for i in range(9) for j in range(i + 1, 9))
    want = -(B / (81.0 * 8.0)).mean(axis=(1, 2, 3, 4))
    got = res.fair_crps.astype(np.float64) - res.crps.astype(np.float64)
    assert np.abs(got - want).max() <= 2.0 ** -22 * np.abs(res.crps).max()


def test_both_member_layouts_give_equal_results():
    x = make_ensemble((3, 2, 5, 2, 4, 6), 11)
    y = verification(x, 12)
    xt = np.ascontiguousarray(np.moveaxis(x, 2, 1))             # (T, M, S, ...)
    for axis in (None, (1, 3, 4)):
        one = ensemble.ensemble_scores(x, y, axis=axis, crps_field=True)
        two = ensemble.ensemble_scores(xt, y, member_axis=1, axis=axis, crps_field=True)
        for a, b in zip(one, two):
            assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(ensemble.ensemble_mean_spread(x), ensemble.ensemble_mean_spread(xt, member_axis=1)):
        assert np.array_equal(a, b)
    # the free views of what predict_timeseries returns
    flat = x.reshape(3, 10, 2, 4, 6)
    assert np.array_equal(ensemble.ensemble_scores(flat.reshape(3, 2, 5, 2, 4, 6), y).crps, ensemble.ensemble_scores(x, y).crps)


def test_nan_rule_and_count():
    x = make_ensemble((3, 2, 6, 2, 3, 5), 21)
    y = verification(x, 22)
    x[0, 1, 4, 1, 2, 3] = np.nan                                 # one member of one column
    x[1, 0, 0, 0, 0, 0] = np.nan                                 # member 0: the shift itself
    y[1, 1, 1, 0, 1] = np.nan
    y[2] = np.nan                                                # a lead whose columns are all skipped
    res = ensemble.ensemble_scores(x, y, crps_field=True)
    assert res.count.tolist() == [59, 58, 0] and res.rank_hist.sum(axis=1).tolist() == [59, 58, 0]
    for v in res[:6]:
        assert np.isnan(v[2]) and not np.isnan(v[:2]).any()
    check_scores(res, scores64(x, y, False), 'host nan', res.crps_field)
    assert np.isnan(res.crps_field[0, 1, 1, 2, 3]) and np.isnan(res.crps_field[2]).all() and np.isnan(res.crps_field).sum() == 3 + 30 + 30
    mean, spread = ensemble.ensemble_mean_spread(x)
    bad = np.isnan(x).any(axis=2)
    assert bad.sum() == 2 and np.array_equal(np.isnan(mean), bad) and np.array_equal(np.isnan(spread), bad)
    grouped = ensemble.ensemble_scores(x, y, axis=(1, 3, 4))
    assert grouped.count.tolist() == [[30, 29], [29, 29], [0, 0]]


def test_ties_count_as_not_below():
    rng = np.random.default_rng(31)
    x = rng.integers(-3, 4, (2, 3, 12, 2, 4, 5)).astype(np.float32)
    y = rng.integers(-3, 4, (2, 3, 2, 4, 5)).astype(np.float32)
    res = ensemble.ensemble_scores(x, y, crps_field=True)
    want = scores64(x, y, False)
    check_scores(res, want, 'host ties', res.crps_field)
    assert np.array_equal(res.rank_hist, want['rank_hist']) and res.rank_hist[:, 12].sum() < res.rank_hist.sum() / 4
    again = ensemble.ensemble_scores(x, y)
    assert np.array_equal(again.rank_hist, res.rank_hist)      # no randomisation


def test_argument_errors():
    x = make_ensemble((2, 2, 3, 1, 2, 2), 41)
    y = verification(x, 42)
    with pytest.raises(ValueError, match='at least 2 members'):
        ensemble.ensemble_scores(x[:, :, :1], y)
    with pytest.raises(ValueError, match='at least 2 members'):
        ensemble.ensemble_mean_spread(x[:, :, :1])
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match='member_axis'):
            ensemble.ensemble_scores(x, y, member_axis=bad)
        with pytest.raises(ValueError, match='member_axis'):
            ensemble.ensemble_mean_spread(x, member_axis=bad)
    with pytest.raises(ValueError, match='do not match'):
        ensemble.ensemble_scores(x, y[:, :1])
    with pytest.raises(ValueError, match='do not match'):
        ensemble.ensemble_scores(x, y, member_axis=1)             # read as (T, M, S, ...): 3 samples against 2
    with pytest.raises(ValueError, match='field axis'):
        ensemble.ensemble_mean_spread(x.reshape(2, 2, 12))
    with pytest.raises(ValueError, match='ddof'):
        ensemble.ensemble_scores(x, y, ddof=2)
    with pytest.raises(ValueError, match="'axis'"):
        ensemble.ensemble_scores(x, y, axis=(0, 1))
    # device operands must be CUDA float32 tensors: refused before any device is touched
    with pytest.raises(TypeError, match="'forecast' must be a CUDA float32 tensor"):
        ensemble.ensemble_scores(torch.from_numpy(x), y)
    with pytest.raises(TypeError, match="'valid' must be float32 on the device path"):
        ensemble.ensemble_scores(x, y.astype(np.float64), device='cuda')
    with pytest.raises(TypeError, match="'forecast' must be float32 on the device path"):
        ensemble.ensemble_mean_spread(x.astype(np.float64), device='cuda')
    with pytest.raises(ValueError, match='CUDA device'):
        ensemble.ensemble_scores(x, y, device='cpu')


def test_axis_rule_covered_axes_and_host_fallback():
    from dlwp_amd.model.verify import _groups_run
    field = (2, 3, 5)
    assert _groups_run(field, None, 1) == (1, 30)
    assert _groups_run(field, (1, 3, 4), 1) == (2, 15) and _groups_run(field, (-1, 1, -2), 1) == (2, 15)
    for axis in ((1,), (1, 2, 3), (3, 4), 1):
        assert _groups_run(field, axis, 1) is None
    x = make_ensemble((2, 3, 4) + field, 51)
    y = verification(x, 52)
    # an uncovered axis runs the host code: samples only -> one value per lead and field point
    res = ensemble.ensemble_scores(x, y, axis=(1,))
    assert res.crps.shape == (2,) + field and res.rank_hist.shape == (2,) + field + (5,) and (res.count == 3).all()
    whole = ensemble.ensemble_scores(x, y)
    assert np.array_equal(res.rank_hist.sum(axis=(1, 2, 3)), whole.rank_hist)
    assert np.allclose(res.crps.astype(np.float64).mean(axis=(1, 2, 3)), whole.crps, rtol=1e-6)
    # the strides of the two layouts, and the extent check in front of a launch
    assert ops.ens_strides(3, 4, 30, 2) == (360, 120, 30) and ops.ens_strides(3, 4, 30, 1) == (360, 30, 90)
    assert ops.ens_extent((360, 120, 30), 2, 3, 4, 30) == 720 == ops.ens_extent((360, 30, 90), 2, 3, 4, 30)


def test_abi_declares_binds_and_untapes_the_new_entry_points():
    names = ('dlwp_ens_mean_spread', 'dlwp_ens_score_workspace', 'dlwp_ens_score_sums')
    declared = _lib.declared_symbols()
    for n in names:
        assert n in declared and getattr(_lib.lib, n).argtypes is not None
    src = open(_lib.os.path.join(_lib._HERE, 'csrc', 'ensemble.hip')).read()
    for n in (names[0], names[2]):
        assert 'DLWP_UNTAPED(%s)' % n in src
    # the workspace query needs no device: sizes outside the ranges give 0, a null handle counts an MI355X
    ws = _lib.lib.dlwp_ens_score_workspace
    assert ws(None, 0, 1, 8) == ws(None, 1, 0, 8) == ws(None, 1, 1, 1) == ws(None, 1, 1, 257) == 0
    assert ws(None, 56, 1, 256) == 56 * (256 * 2 // 56) * (48 + 257 * 8)
    assert ws(None, 3, 2, 5) == 6 * (256 * 28 // 6) * (48 + 6 * 8)
    # argument checks come before any launch (and before the handle is looked at)
    assert _lib.lib.dlwp_ens_score_sums(None, None, 0, 0, 0, None, 1, 1, 300, 1, 1, None, None, None, None, 0, None) != 0
    assert b'members 300' in _lib.lib.dlwp_last_error()
    assert _lib.lib.dlwp_ens_mean_spread(None, None, 1, 1, 1, 0, 0, 0, 1, 1, None, None, None) != 0
    assert b'members 1' in _lib.lib.dlwp_last_error()
