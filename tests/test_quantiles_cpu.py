"""Climatological quantiles on the host: dlwp_amd.model.verify.label_quantiles_host (the definition the device kernel is compared with,
bit for bit, in tests/test_gpu_quantiles.py) against the column-by-column restatement of tests/quantile_cases.py and against
numpy.nanquantile, its identities, the refusals that need no device, and climatological_quantiles on LabeledArrays.

Against numpy.  np.nanquantile(x.astype(float64), q, method=...) rounded to float32 is compared on 400 columns of 1 .. 301 samples x 32
probabilities = 12 800 quantiles per method (quantile_cases.numpy_columns, fixed seed).  The three order-statistic methods return a
sample, so they compare ==.  'linear' is bounded by one float32 ulp -- numpy evaluates a lerp of its own in float64, whose last bit may
differ before the rounding to float32 -- and on these fixed inputs numpy (2.2.6) gives zero differences, which is asserted; run with -s
for the share."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import verify
from dlwp_amd.model.generators import LabeledArray
from tests.quantile_cases import (KINDS, METHODS, ORDER_METHODS, Q_SETS, QNAN, QS, bits, labels_for, make_data, numpy_columns,
                                  numpy_quantiles, quantiles_restated, same_bits)


@pytest.mark.parametrize('method', METHODS)
def test_host_definition_has_the_bits_of_the_restatement(method):
    for kind in KINDS:
        if kind == 'inf' and method == 'linear':
            continue
        for count, n_labels, inner in ((1, 1, (5,)), (2, 2, (7,)), (37, 3, (2, 5)), (61, 12, (9,))):
            x = make_data((count,) + inner, kind, 7 * count + n_labels)
            lab = labels_for(count, n_labels, count)
            got, n = verify.label_quantiles_host(x, lab, n_labels, QS, method, return_count=True)
            want, n_want = quantiles_restated(x, lab, n_labels, QS, method)
            same_bits(got, want)
            same_bits(n, n_want)


def test_linear_between_infinities_is_the_one_nan():
    x = np.array([[-np.inf, np.inf, 1.0], [np.inf, np.inf, np.inf], [-np.inf, np.inf, np.nan]], np.float32)
    got = verify.label_quantiles_host(x, np.zeros(3, np.int32), 1, [0.25, 0.5], 'linear')
    same_bits(got, quantiles_restated(x, np.zeros(3, np.int32), 1, [0.25, 0.5], 'linear')[0])
    assert bits(got)[0, 0, 0] == QNAN and bits(got)[0, 0, 1] == QNAN           # inf - inf, of either sign
    assert got[1, 0, 0] == -np.inf and got[1, 0, 1] == np.inf and got[1, 0, 2] == np.inf      # whole h; 1 + inf / 2


@pytest.mark.parametrize('method', METHODS)
def test_against_numpy_nanquantile(method):
    x, q = numpy_columns()
    got = verify.label_quantiles_host(x, np.zeros(x.shape[0], np.int32), 1, q, method)[:, 0]
    want = numpy_quantiles(x, q, method)
    assert got.shape == want.shape == (32, 400)
    if method in ORDER_METHODS:
        assert np.array_equal(got, want)
        return
    ulp = np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))
    share = float(np.count_nonzero(ulp)) / ulp.size
    print('linear against numpy %s: %.5f of %d quantiles differ, at most %d ulp' % (np.__version__, share, ulp.size, ulp.max()))
    assert ulp.max() <= 1
    assert share == 0.0


def test_identities():
    count, n_labels = 53, 3
    x = make_data((count, 11), 'gauss', 3)
    ties = make_data((count, 11), 'ties', 4)
    lab = labels_for(count, n_labels, 5)
    lab[lab == 2] = 1                                        # label 2 has no rows
    for data in (x, ties):
        ends, n = verify.label_quantiles_host(data, lab, n_labels, [0.0, 1.0], 'linear', return_count=True)
        res = {m: verify.label_quantiles_host(data, lab, n_labels, QS, m) for m in METHODS}
        for l in range(2):
            rows = data[lab == l]
            # (not np.nanmin: its fmin reduction goes wrong on the signalling NaNs of make_data)
            lo = np.where(np.isnan(rows), np.float32(np.inf), rows).min(axis=0)
            hi = np.where(np.isnan(rows), np.float32(-np.inf), rows).max(axis=0)
            ok = ~np.isnan(rows).all(axis=0)
            assert np.array_equal(ends[0, l][ok], lo[ok]) and np.array_equal(ends[1, l][ok], hi[ok])
            assert np.array_equal(n[l], np.count_nonzero(~np.isnan(rows), axis=0))
        ok = ~np.isnan(res['linear'])
        assert np.all(res['lower'][ok] <= res['linear'][ok]) and np.all(res['linear'][ok] <= res['higher'][ok])
        # column 0 is all NaN: NaN with count 0; label 2 has no rows: NaN everywhere
        for m in METHODS:
            assert np.all(bits(res[m][:, :, 0]) == QNAN) and np.all(n[:, 0] == 0)
            assert np.all(bits(res[m][:, 2]) == QNAN) and np.all(n[2] == 0)
        # the rows of a label in another order
        perm = np.random.default_rng(6).permutation(count)
        for m in METHODS:
            same_bits(verify.label_quantiles_host(data[perm], lab[perm], n_labels, QS, m), res[m])
    # n == 1: the sample for every q, whatever the method, with its bits (-0.0 stays -0.0)
    one = np.array([[np.nan, -0.0, 3.5], [2.0, np.nan, np.nan]], np.float32)
    for m in METHODS:
        got = verify.label_quantiles_host(one, np.zeros(2, np.int32), 1, QS, m)
        same_bits(got, np.broadcast_to(np.array([2.0, -0.0, 3.5], np.float32), (len(QS), 1, 3)).copy())
    # -0.0 sorts below +0.0
    z = np.array([[0.0], [-0.0], [0.0], [-0.0]], np.float32)
    got = verify.label_quantiles_host(z, np.zeros(4, np.int32), 1, [0.0, 1.0], 'lower')
    assert bits(got).reshape(-1).tolist() == [0x80000000, 0x00000000]


def test_refusals_without_a_device():
    x = make_data((5, 8), 'gauss', 1)
    lab = np.array([0, 1, 0, 1, 1], np.int32)
    for bad in ([1.5], [-0.1], [np.nan], [np.inf], [], [[0.5]]):
        with pytest.raises(ValueError, match='q must|every q'):
            verify.label_quantiles_host(x, lab, 2, bad)
    with pytest.raises(ValueError, match='method'):
        verify.label_quantiles_host(x, lab, 2, 0.5, 'midpoint')
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 2\)'):
        verify.label_quantiles_host(x, np.array([0, 1, 2, 0, 0]), 2, 0.5)
    with pytest.raises(TypeError, match='float32'):
        verify.label_quantiles_host(np.zeros((5, 8)), lab, 2, 0.5)
    assert verify.label_quantiles_host(x, lab, 2, np.linspace(0, 1, 9)).shape == (9, 2, 8)       # any K on the host
    # ops refuses on the host arrays before it touches a device: a CPU tensor gets as far as the device look-up
    t = torch.from_numpy(x)
    with pytest.raises(ValueError, match='every q'):
        ops.verify_label_quantiles(t, lab, 2, [0.5, 1.01])
    with pytest.raises(ValueError, match='at least one'):
        ops.verify_label_quantiles(t, lab, 2, [])
    with pytest.raises(ValueError, match='9 probabilities, at most 8'):
        ops.verify_label_quantiles(t, lab, 2, np.linspace(0, 1, 9))
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 2\)'):
        ops.verify_label_quantiles(t, np.array([0, 1, -1, 0, 0]), 2, 0.5)
    with pytest.raises(ValueError, match='4 labels for 5 samples'):
        ops.verify_label_quantiles(t, lab[:4], 2, 0.5)
    with pytest.raises(ValueError, match='method'):
        ops.verify_label_quantiles(t, lab, 2, 0.5, method='median_unbiased')
    with pytest.raises(ValueError, match='route'):
        ops.verify_label_quantiles(t, lab, 2, 0.5, route=3)
    with pytest.raises(ValueError, match='float32'):
        ops.verify_label_quantiles(t.double(), lab, 2, 0.5)
    with pytest.raises(RuntimeError, match='device'):
        ops.verify_label_quantiles(t, lab, 2, 0.5)
    # climatological_quantiles with device='cuda' checks before it looks for a device
    times = np.datetime64('2001-01-01T00') + np.arange(5) * np.timedelta64(6, 'h')
    da = LabeledArray(x, {'time': times}, ('time', 'lon'))
    with pytest.raises(ValueError, match='9 probabilities, at most 8'):
        verify.climatological_quantiles(da, np.linspace(0, 1, 9), device='cuda')
    with pytest.raises(ValueError, match='every q'):
        verify.climatological_quantiles(da, [2.0], device='cuda')
    with pytest.raises(ValueError, match='labels must lie'):
        verify.climatological_quantiles(da, 0.5, labels=np.array([0, 1, 2, 0, 0]), n_labels=2, device='cuda')
    with pytest.raises(ValueError, match='needs n_labels'):
        verify.climatological_quantiles(da, 0.5, labels=lab)
    with pytest.raises(TypeError, match='float32 on the device path'):
        verify.climatological_quantiles(LabeledArray(np.zeros((5, 8)), {'time': times}, ('time', 'lon')), 0.5, device='cuda')


def test_planner_and_c_refusals_without_a_device():
    """dlwp_verify_label_quantiles_plan is host logic: the widest of 64 / 32 / 16 columns whose image of round_up(max_len, 256 / cols)
    rows fits 80 KiB, else the streaming route; the sizes come from the header's rule, not from the kernel"""
    budget = 80 * 1024

    def rule(max_len):
        for cols in (64, 32, 16):
            t = 256 // cols
            if (max_len + t - 1) // t * t * cols * 4 <= budget:
                return 1, cols
        return 2, 64
    for max_len in (1, 2, 319, 320, 321, 639, 640, 641, 1240, 1279, 1280, 1281, 14608):
        assert ops.verify_label_quantiles_plan(max_len, 108) == rule(max_len), max_len
        assert ops.verify_label_quantiles_plan(max_len, 108, route=2) == (2, 64)
    assert ops.verify_label_quantiles_plan(1280, 7, route=1) == (1, 16)
    with pytest.raises(_lib.DlwpError, match='LDS route holds at most 1280 rows'):
        ops.verify_label_quantiles_plan(1281, 7, route=1)
    with pytest.raises(_lib.DlwpError, match='route 3'):
        ops.verify_label_quantiles_plan(5, 7, route=3)
    with pytest.raises(_lib.DlwpError, match='must be >= 1'):
        ops.verify_label_quantiles_plan(0, 7)
    ws = _lib.lib.dlwp_verify_label_quantiles_workspace
    assert ws(None, 5, ctypes.c_longlong(8), 2, 3) == 64 and ws(None, 5, ctypes.c_longlong(7), 3, 1) == 96
    assert ws(None, 5, ctypes.c_longlong(8), 65, 3) == 0 and ws(None, 5, ctypes.c_longlong(8), 2, 9) == 0 and ws(None, 0, 8, 2, 1) == 0
    src = open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'quantile.hip')).read()
    assert 'DLWP_UNTAPED(dlwp_verify_label_quantiles)' in src and '#pragma clang fp contract(off)' in src


def test_climatological_quantiles_on_labeled_arrays():
    rng = np.random.default_rng(11)
    times = np.datetime64('2003-11-20T00') + np.arange(120) * np.timedelta64(18, 'h')       # November .. February
    x = (rng.standard_normal((120, 2, 3, 4)) * 2.0).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.nan
    months = verify.month_labels(times)
    da = LabeledArray(x, {'time': times}, ('time', 'varlev', 'lat', 'lon'))
    got, n = verify.climatological_quantiles(da, [1.0 / 3.0, 2.0 / 3.0], return_count=True)
    want, n_want = verify.label_quantiles_host(x, months, 12, [1.0 / 3.0, 2.0 / 3.0], 'linear', return_count=True)
    assert got.shape == (2, 12, 2, 3, 4) and n.shape == (12, 2, 3, 4) and n.dtype == np.int32
    same_bits(got, want)
    same_bits(n, n_want)
    assert np.isnan(got[:, 5]).all() and not np.isnan(got[:, 0]).any()                      # no June in the record
    # a 'sample' axis that is not the leading one, a scalar q, another method
    moved = LabeledArray(np.moveaxis(x, 0, 2).copy(), {'sample': times}, ('varlev', 'lat', 'sample', 'lon'))
    upper = verify.climatological_quantiles(moved, 2.0 / 3.0, method='higher')
    assert upper.shape == (1, 12, 2, 3, 4)
    same_bits(upper, verify.label_quantiles_host(x, months, 12, 2.0 / 3.0, 'higher'))
    # the whole record as one label; seasons as a grouping of one's own
    whole = verify.climatological_quantiles(da, [0.05, 0.95], labels=None)
    assert whole.shape == (2, 1, 2, 3, 4)
    assert np.array_equal(whole[:, 0], numpy_quantiles(x, [0.05, 0.95], 'linear'))
    seasons = ((months + 1) % 12 // 3).astype(np.int32)
    by_season = verify.climatological_quantiles(da, 0.5, labels=seasons, n_labels=4, method='nearest')
    same_bits(by_season, verify.label_quantiles_host(x, seasons, 4, 0.5, 'nearest'))
    with pytest.raises(ValueError, match="expected 'month'"):
        verify.climatological_quantiles(da, 0.5, labels='season')
    for k, qs in Q_SETS.items():
        assert verify.climatological_quantiles(da, qs, labels=None).shape[0] == k
