"""Ensemble verification on the device (csrc/ensemble.hip behind dlwp_amd.model.ensemble) against the brute-force float64 restatement
of tests/ensemble_cases.py on the same float32 inputs: np.mean / np.var, the O(M^2) pairwise B, (x < y).sum for the ranks.

Required: rank_hist and count exactly equal; the mean field equal to float32(float64 member-order sum / M) bit for bit; spread,
rmse_mean, mae_mean, crps, fair_crps and the crps field within
    |device - float64| <= 2^-23 |float64| + 2^-40 * (the magnitudes that cancel)
-- the cast to float32, and float64 sums in another order ((M + n) * 2^-53 of what enters them).  tests/ensemble_cases.py derives the
second term per score (DESIGN.md 5.35 repeats it); nothing in it comes from the device's output.  Ensembles are base + 0.01 * noise,
so the shifted sums are what is exercised.  Run with -s to see error / bound of every case."""
import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import ensemble
from tests.ensemble_cases import (check_scores, columns64, ensemble as make_ensemble, member_order_mean32, scores64, spread_field64,
                                  verification, within)
from tests.nets import cnn2_layers

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
    out = store[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def members_first(x):
    """(T, S, M, ...) -> contiguous (T, M, S, ...)"""
    return np.ascontiguousarray(np.moveaxis(x, 2, 1))


def check_all_layouts(x, y, what):
    """both member axes x grouped / ungrouped, the crps field on in half of them; the reference is computed once"""
    c = columns64(x, y)
    want = {False: scores64(x, y, False, c=c), True: scores64(x, y, True, c=c)}
    yd = cuda(y)
    for member_axis, xd in ((2, cuda(x)), (1, cuda(members_first(x)))):
        for grouped in (False, True):
            field = grouped == (member_axis == 2)
            res = ensemble.ensemble_scores(xd, yd, member_axis=member_axis, axis=(1, 3, 4) if grouped else None, crps_field=field)
            assert (res.crps_field is not None) == field
            if field:
                assert res.crps_field.is_cuda and tuple(res.crps_field.shape) == y.shape
            check_scores(res, want[grouped], '%s axis %d %s' % (what, member_axis, 'grouped' if grouped else 'whole'),
                         res.crps_field.cpu().numpy() if field else None)
    return want


#: run = 35 (70 ungrouped): scalar loads and a tail shorter than a wave; 8 x 32: 16-byte loads in the field kernel, whole 64-point tiles;
#: 9 x 31 = 279: several tiles with a ragged last one
FIELDS = [(2, 5, 7), (2, 8, 32), (1, 9, 31)]
#: both ends, every register instance (2, 4, 8, 32 keys) with and without padding, 2, 4 and 8 runs in LDS with a ragged last run
MEMBERS = [2, 3, 5, 31, 32, 33, 64, 100, 256]


@pytest.mark.parametrize('field', FIELDS, ids=lambda f: 'x'.join(map(str, f)))
@pytest.mark.parametrize('members', MEMBERS)
def test_scores_on_every_route(members, field):
    samples = 1 + (members + len(FIELDS) + FIELDS.index(field)) % 2          # S = 1 and S = 2 alternate over the cases
    x = make_ensemble((3, samples, members) + field, 1000 + members)
    y = verification(x, 2000 + members)
    check_all_layouts(x, y, 'M=%d S=%d %s' % (members, samples, field))


@pytest.mark.parametrize('field', FIELDS, ids=lambda f: 'x'.join(map(str, f)))
@pytest.mark.parametrize('members', [2, 5, 33, 256])
def test_mean_and_spread_fields(members, field):
    x = make_ensemble((3, 2, members) + field, 3000 + members)
    x[1, 1, members // 2, 0, 1, 2] = np.nan
    want_mean = member_order_mean32(x)
    for member_axis, xd in ((2, cuda(x)), (1, cuda(members_first(x)))):
        for ddof in (1, 0):
            mean, spread = ensemble.ensemble_mean_spread(xd, member_axis=member_axis, ddof=ddof)
            assert mean.is_cuda and spread.is_cuda and tuple(mean.shape) == tuple(spread.shape) == (3, 2) + field
            assert np.array_equal(mean.cpu().numpy(), want_mean, equal_nan=True)
            assert np.isnan(want_mean).sum() == 1
            within(spread.cpu().numpy(), *spread_field64(x, ddof), 'spread field M=%d axis %d ddof %d %s' % (members, member_axis, ddof, field))
    # numpy in, numpy out
    mean, spread = ensemble.ensemble_mean_spread(x, device='cuda')
    assert isinstance(mean, np.ndarray) and np.array_equal(mean, want_mean, equal_nan=True)
    # one float into the storage the 16-byte route is not allowed: the scalar route gives the same bits
    row = int(np.prod(field))
    st = ops.ens_strides(2, members, row, 2)
    for got, ref in zip(ops.ens_mean_spread(cuda(x, True), st, 3, 2, members, row), ops.ens_mean_spread(cuda(x), st, 3, 2, members, row)):
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    only = ops.ens_mean_spread(cuda(x), st, 3, 2, members, row, want_mean=False)
    assert only[0] is None and torch.equal(only[1].view(torch.int32), ref.view(torch.int32))


def test_nan_members_nan_valid_and_a_lead_without_columns():
    x = make_ensemble((3, 2, 33, 2, 5, 7), 41)
    y = verification(x, 42)
    x[0, 1, 4, 1, 2, 3] = np.nan
    x[0, 0, 32, 0, 0, 0] = np.nan                                # the last member: the ragged run
    x[1, 0, 0, 0, 4, 6] = np.nan                                 # member 0: the shift itself
    y[1, 1, 1, 0, 1] = np.nan
    y[2] = np.nan                                                # every column of lead 2 is skipped
    want = check_all_layouts(x, y, 'nan')
    assert want[False]['count'].tolist() == [138, 138, 0] and want[True]['count'].tolist() == [[69, 69], [69, 69], [0, 0]]
    res = ensemble.ensemble_scores(cuda(x), cuda(y), crps_field=True)
    for v in res[:6]:
        assert np.isnan(v[2]) and not np.isnan(v[:2]).any()
    assert (res.rank_hist[2] == 0).all() and res.count[2] == 0
    assert torch.isnan(res.crps_field[2]).all() and int(torch.isnan(res.crps_field[:2]).sum()) == 4


@pytest.mark.parametrize('members', [12, 70])
def test_integer_valued_ties(members):
    rng = np.random.default_rng(51 + members)
    x = rng.integers(-3, 4, (3, 2, members, 2, 5, 7)).astype(np.float32)
    y = rng.integers(-3, 4, (3, 2, 2, 5, 7)).astype(np.float32)
    x[0, :, :, 0, 0, 0] = 2.0                                    # every member equal to y: rank 0, crps 0
    y[0, :, 0, 0, 0] = 2.0
    want = check_all_layouts(x, y, 'ties M=%d' % members)
    res = ensemble.ensemble_scores(cuda(x), cuda(y), crps_field=True)
    assert np.array_equal(res.rank_hist, want[False]['rank_hist']) and res.rank_hist[:, members].sum() < res.rank_hist.sum() / 4
    assert (res.crps_field[0, :, 0, 0, 0] == 0).all()


@pytest.mark.parametrize('members', [8, 33])
def test_many_partials_per_cell_and_repeatable_bits(members):
    """rows of 2 x 64 x 96 and 2 samples: every block of the launch has work and the second kernel adds hundreds of partials per cell.
    Two launches on the same input return identical bits."""
    field = (2, 64, 96)
    x = make_ensemble((3, 2, members) + field, 61 + members)
    y = verification(x, 62 + members, nan_every=1013)
    check_all_layouts(x, y, 'tree M=%d' % members)
    xd, yd = cuda(x), cuda(y)
    row = int(np.prod(field))
    st = ops.ens_strides(2, members, row, 2)
    for groups in (1, 2):
        one = ops.ens_score_sums(xd, st, yd, 3, 2, members, groups, row // groups, crps_field=True)
        two = ops.ens_score_sums(xd, st, yd, 3, 2, members, groups, row // groups, crps_field=True)
        assert torch.equal(one[0].view(torch.int64), two[0].view(torch.int64)) and torch.equal(one[1], two[1])
        assert torch.equal(one[2].view(torch.int32), two[2].view(torch.int32))
    a, b = ensemble.ensemble_mean_spread(xd), ensemble.ensemble_mean_spread(xd)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_numpy_operands_large_ensembles_and_uncovered_axes():
    x = make_ensemble((3, 2, 6, 2, 5, 7), 71)
    y = verification(x, 72)
    want = scores64(x, y, False)
    res = ensemble.ensemble_scores(x, y, crps_field=True, device='cuda')       # numpy in: a numpy field out
    assert isinstance(res.crps_field, np.ndarray)
    check_scores(res, want, 'numpy operands', res.crps_field)
    check_scores(ensemble.ensemble_scores(cuda(x), y), want, 'mixed operands')
    # an axis the device path does not cover, and more than 256 members: the host code on downloaded arrays, equal to the host path
    host = ensemble.ensemble_scores(x, y, axis=(1,))
    dev = ensemble.ensemble_scores(cuda(x), cuda(y), axis=(1,))
    for a, b in zip(host[:8], dev[:8]):
        assert np.array_equal(a, b, equal_nan=True)
    big = make_ensemble((2, 1, 257, 1, 3, 5), 73)
    yb = verification(big, 74)
    host, dev = ensemble.ensemble_scores(big, yb), ensemble.ensemble_scores(cuda(big), cuda(yb))
    for a, b in zip(host[:8], dev[:8]):
        assert np.array_equal(a, b, equal_nan=True)
    with pytest.raises(ValueError, match='the strides address'):
        ops.ens_score_sums(cuda(x), ops.ens_strides(2, 7, 70, 2), cuda(y), 3, 2, 7, 1, 70)
    with pytest.raises(TypeError, match="'forecast' must be a CUDA float32 tensor"):
        ensemble.ensemble_scores(cuda(x).double(), cuda(y))


def test_rollout_ensemble_scored_where_it_is():
    """a small convolutional DLWPNeuralNet rolled out on 2 samples x 4 perturbed members with return_device=True; the series is viewed
    as (T, 2, 4, ...) and scored against a synthetic verification: equal to the host path on the downloaded series within the bound,
    with equal histograms"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    d.build_model(cnn2_layers((4, 8, 12)), loss='mse', optimizer='adam')
    rng = np.random.default_rng(91)
    base = rng.standard_normal((2, 1, 4, 8, 12))
    x0 = (base + 0.05 * rng.standard_normal((2, 4, 4, 8, 12))).astype(np.float32).reshape(8, 4, 8, 12)
    series = d.predict_timeseries(x0, 5, return_device=True)
    assert series.is_cuda and tuple(series.shape) == (5, 8, 4, 8, 12)
    ens = series.view(5, 2, 4, 4, 8, 12)
    host_ens = ens.cpu().numpy()
    valid = (host_ens.mean(axis=2) + 0.05 * rng.standard_normal((5, 2, 4, 8, 12))).astype(np.float32)
    c = columns64(host_ens, valid)
    for axis in (None, (1, 3, 4)):
        want = scores64(host_ens, valid, axis is not None, c=c)
        res = ensemble.ensemble_scores(ens, cuda(valid), axis=axis, crps_field=True)
        check_scores(res, want, 'rollout device', res.crps_field.cpu().numpy())
        host = ensemble.ensemble_scores(host_ens, valid, axis=axis, crps_field=True)
        check_scores(host, want, 'rollout host', host.crps_field)
        assert np.array_equal(res.rank_hist, host.rank_hist) and np.array_equal(res.count, host.count)
    mean, spread = ensemble.ensemble_mean_spread(ens)
    assert np.array_equal(mean.cpu().numpy(), member_order_mean32(host_ens))
    within(spread.cpu().numpy(), *spread_field64(host_ens), 'rollout spread field')
