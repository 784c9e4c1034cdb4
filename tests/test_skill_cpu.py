"""Latitude-weighted forecast skill without a device: the host path of verify.forecast_skill / persistence_skill against the float64
restatement of tests/skill_cases.py (bounds derived there), the identities of the definition, the helpers, the planner, and every
refusal that comes before a launch -- those of the C entry point in the order include/dlwp_hip.h gives."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import verify
from dlwp_amd.model.generators import LabeledArray
from tests.skill_cases import check_skill, cosine, data, forecast64, labels_of, persistence64, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
FAKE = ctypes.c_void_p(4096)         # a non-null address for refusals that come before any launch; never dereferenced
NULL = ctypes.c_void_p(0)
INNER = (2, 6, 10)


# -- the host path against the restatement ------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_host_path_per_lead_valid_with_table_and_weights(axis):
    fc, va = data((3, 5) + INNER, 1, 7), data((3, 5) + INNER, 2, 11)
    table, labels, w = table_of(INNER, 3), labels_of((3, 5), 4), cosine(6)
    labels[1, 2] = -1
    got = verify.forecast_skill(fc, va, table, labels, w, axis=axis)
    check_skill(got, forecast64(fc, va, table, labels, w, axis is not None), 'host per lead')


@pytest.mark.parametrize('axis', [None, (0, 2, 3)], ids=['all', 'groups'])
def test_host_path_plain_series_and_leads_beyond_it(axis):
    """F = 7 leads against Nv = 5 times: leads 5 and 6 have no pairs -> NaN and count 0"""
    fc, va = data((7, 6) + INNER, 5), data((5,) + INNER, 6)
    table, labels, w = table_of(INNER, 7), labels_of((5,), 8), cosine(6)
    got = verify.forecast_skill(fc, va, table, labels, w, axis=axis)
    check_skill(got, forecast64(fc, va, table, labels, w, axis is not None), 'host plain series')
    assert (got.count[5:] == 0).all() and (got.count[:5] > 0).all()
    for name in ('mse', 'rmse', 'mae', 'bias', 'acc', 'acc_centered'):
        assert np.isnan(getattr(got, name)[5:]).all() and not np.isnan(getattr(got, name)[:5]).any(), name


def test_host_path_optional_arguments_each_alone_and_persistence():
    fc, va = data((3, 5) + INNER, 9), data((3, 5) + INNER, 10)
    table, labels, w = table_of(INNER, 11), labels_of((3, 5), 12), cosine(6)
    check_skill(verify.forecast_skill(fc, va), forecast64(fc, va), 'host bare')
    check_skill(verify.forecast_skill(fc, va, weights=w), forecast64(fc, va, weights=w), 'host weights only')
    check_skill(verify.forecast_skill(fc, va, table, labels), forecast64(fc, va, table, labels), 'host table only')
    check_skill(verify.forecast_skill(fc, va, table[3]), forecast64(fc, va, table[3]), 'host one field')
    pr, pv, pl = data((6,) + INNER, 13), data((6,) + INNER, 14), labels_of((6,), 15)
    check_skill(verify.persistence_skill(pr, pv, 4, table, pl, w), persistence64(pr, pv, 4, table, pl, w), 'host persistence')
    check_skill(verify.persistence_skill(pr, pv, 4, table, pl, w, axis=(0, 2, 3)), persistence64(pr, pv, 4, table, pl, w, True),
                'host persistence groups')


def test_unweighted_errors_are_those_of_forecast_error_in_float64():
    """no weights, no climatology: mse, mae, rmse within 2^-22 of the float64 value of forecast_error's definition (nanmean of d^2, |d|)"""
    fc, va = data((4, 7) + INNER, 16, 29), data((7,) + INNER, 17, 31)
    got = verify.forecast_skill(fc, va)
    for f in range(4):
        d = va[f:].astype(np.float64) - fc[f, :7 - f].astype(np.float64)
        want = {'mse': np.nanmean(d * d), 'mae': np.nanmean(np.abs(d)), 'rmse': np.sqrt(np.nanmean(d * d))}
        for name, v in want.items():
            assert abs(float(getattr(got, name)[f]) - v) <= 2.0 ** -22 * v, (f, name)
        assert got.count[f] == np.count_nonzero(~np.isnan(d))


# -- identities ---------------------------------------------------------------------------------------------------------------------- #
def test_identities_of_the_definition():
    va = data((3, 5) + INNER, 18)
    table, labels, w = table_of(INNER, 19), labels_of((3, 5), 20), cosine(6)
    same = verify.forecast_skill(va.copy(), va, table, labels, w)
    assert (same.acc == 1).all() and (same.bias == 0).all() and (same.rmse == 0).all() and (same.mae == 0).all()
    # fa = -oa exactly: no climatology, the forecast is the negated truth.  sqrt(fl(x * x)) == |x| in binary arithmetic
    assert (verify.forecast_skill(-va, va, weights=w).acc == -1).all()
    # forecast = fl(valid + 2), |valid + 2| < 32: the sum is off by at most half an ulp there (2^-20), d = fl(forecast - valid) by
    # 2^-23 more, the cast by 2^-23: a mean of such terms is within 2^-19 of 2
    assert np.abs(va + 2).max() < 32
    shifted = verify.forecast_skill(va + np.float32(2), va, table, labels, w)
    assert (np.abs(shifted.bias.astype(np.float64) - 2.0) <= 2.0 ** -19).all()
    assert (np.abs(shifted.rmse.astype(np.float64) - 2.0) <= 2.0 ** -19).all()


@pytest.mark.parametrize('axis', [None, (1, 3, 4)], ids=['all', 'groups'])
def test_doubling_the_weights_changes_no_bit(axis):
    """S and S0 scale by exactly 2 in binary, so S / S0, S6 / sqrt(S7 S8) and the centred form keep their bits"""
    fc, va = data((3, 5) + INNER, 21, 13), data((3, 5) + INNER, 22)
    table, labels, w = table_of(INNER, 23), labels_of((3, 5), 24), cosine(6)
    one = verify.forecast_skill(fc, va, table, labels, w, axis=axis)
    two = verify.forecast_skill(fc, va, table, labels, 2 * w, axis=axis)
    for a, b in zip(one, two):
        bits = np.int32 if a.dtype == np.float32 else np.int64
        assert np.array_equal(a.view(bits), b.view(bits))


# -- helpers ------------------------------------------------------------------------------------------------------------------------- #
def test_area_weights_are_never_negative():
    w = verify.area_weights(np.linspace(-90, 90, 91))
    assert w.dtype == np.float32 and w.shape == (91,) and (w >= 0).all() and w[0] == 0 and w[-1] == 0 and w[45] == 1
    from dlwp_amd import custom
    assert custom.latitude_weights(np.linspace(-90, 90, 91), 'cosine').min() < 0          # what the clamp is for


def test_month_labels_match_the_private_helper():
    times = np.datetime64('2001-11-20T00') + np.arange(0, 40 * 24 * 6, 24 * 6).astype('timedelta64[h]')
    assert np.array_equal(verify.month_labels(times), verify._months(times))
    got = verify.month_labels(times.reshape(4, 10))
    assert got.shape == (4, 10) and got.dtype == np.int32 and got[0, 0] == 10 and set(got.ravel().tolist()) <= set(range(12))
    with pytest.raises(TypeError, match='datetime64'):
        verify.month_labels(np.arange(4))


def test_monthly_climatology_on_the_host_is_label_nanmean_host():
    times = np.datetime64('2003-01-05T00') + np.arange(0, 30 * 24 * 13, 24 * 13).astype('timedelta64[h]')
    x = data((30, 2, 3, 4), 25, 17)
    want = verify.label_nanmean_host(x, verify._months(times), 12)
    got = verify.monthly_climatology(LabeledArray(x, {'time': times}, ('time', 'varlev', 'lat', 'lon')))
    assert got.dtype == np.float32 and got.shape == (12, 2, 3, 4) and np.array_equal(got.view(np.int32), want.view(np.int32))
    # the time axis need not lead
    moved = LabeledArray(np.moveaxis(x, 0, 1).copy(), {'sample': times}, ('varlev', 'sample', 'lat', 'lon'))
    assert np.array_equal(verify.monthly_climatology(moved).view(np.int32), want.view(np.int32))


def test_planner_strides_for_both_forms_of_valid():
    row = 2 * 6 * 10
    p = verify.plan_forecast_skill((3, 5, 2, 6, 10), (3, 5, 2, 6, 10), None)
    assert p == verify.SkillPlan('forecast', 'valid', (5 * row, row, 0), (5 * row, row, 0), (5, 0), 3, 5, 0, 1, row)
    p = verify.plan_forecast_skill((3, 5, 2, 6, 10), (3, 5, 2, 6, 10), (1, 3, 4))
    assert (p.groups, p.run, p.label_strides) == (2, 60, (5, 0))
    p = verify.plan_forecast_skill((7, 6, 2, 6, 10), (5, 2, 6, 10), None)
    assert p == verify.SkillPlan('forecast', 'valid', (6 * row, row, 0), (0, row, 1), (0, 1), 7, 5, 1, 1, row)
    assert verify.plan_forecast_skill((7, 6, 2, 6, 10), (5, 2, 6, 10), (0, -2, -1))[-2:] == (2, 60)
    p = verify.plan_persistence_skill((8, 2, 6, 10), (6, 2, 6, 10), 4, None)
    assert p == verify.SkillPlan('predictors', 'valid', (0, row, 0), (0, row, 1), (0, 1), 4, 6, 1, 1, row)
    q = verify.plan_persistence((8, 2, 6, 10), (6, 2, 6, 10), 4, None)                   # the same pairs as persistence_error
    assert (p.fc_strides, p.ob_strides) == (q.b_strides, q.a_strides) and p[5:] == q[4:]
    for f_shape, v_shape in (((3, 5, 2, 6, 10), (3, 5, 2, 6, 9)), ((3, 4, 2, 6, 10), (6, 2, 6, 10)), ((3, 5, 6), (6,))):
        with pytest.raises(ValueError, match='do not match'):
            verify.plan_forecast_skill(f_shape, v_shape, None)
    assert ops.verify_label_extent((5, 0), 3, 5, 0) == 15 and ops.verify_label_extent((0, 1), 7, 5, 1) == 5
    assert ops.verify_label_extent((0, 1), 7, 0, 1) == 0


def test_finish_skill_of_added_tables_and_of_empty_cells():
    rng = np.random.default_rng(26)
    a, b = rng.random((4, 3, 10)) + 0.5, rng.random((4, 3, 10)) + 0.5
    for t in (a, b):          # a consistent table: Cauchy-Schwarz holds, the counts are integers
        t[..., 7], t[..., 8], t[..., 9] = 4 * t[..., 7], 4 * t[..., 8], np.floor(10 * t[..., 9])
    a[1] = 0                  # a lead without pairs
    a[2, 1, 0] = 0            # pairs, but every weight zero
    whole = verify.finish_skill(a + b)
    assert whole.mse.shape == (4, 3) and whole.count.dtype == np.int64 and whole.mse.dtype == np.float32
    s = a + b
    assert np.array_equal(whole.mse, (s[..., 2] / s[..., 0]).astype(np.float32))
    assert np.array_equal(whole.acc, (s[..., 6] / np.sqrt(s[..., 7] * s[..., 8])).astype(np.float32))
    assert np.array_equal(whole.count, s[..., 9].astype(np.int64))
    alone = verify.finish_skill(a)
    for name in ('mse', 'rmse', 'mae', 'bias', 'acc', 'acc_centered'):
        v = getattr(alone, name)
        assert np.isnan(v[1]).all() and np.isnan(v[2, 1]) and not np.isnan(v[0]).any(), name
    assert (alone.count[1] == 0).all() and alone.count[2, 1] > 0
    flat = verify.finish_skill(s[:, :1], grouped=False)
    assert flat.mse.shape == (4,) and np.array_equal(flat.mse, whole.mse[:, 0])
    # a zero denominator: no anomaly at all
    z = np.zeros((1, 1, 10))
    z[..., 0] = z[..., 9] = 5
    assert np.isnan(verify.finish_skill(z).acc).all() and np.isnan(verify.finish_skill(z).acc_centered).all()
    assert (verify.finish_skill(z).mse == 0).all()


# -- refusals ------------------------------------------------------------------------------------------------------------------------ #
def test_refusals_of_the_public_functions():
    fc, va = data((3, 5) + INNER, 27), data((3, 5) + INNER, 28)
    table, labels, w = table_of(INNER, 29), labels_of((3, 5), 30), cosine(6)
    bad = w.copy()
    bad[2] = -0.25
    with pytest.raises(ValueError, match='>= 0'):
        verify.forecast_skill(fc, va, weights=bad)
    bad[2] = np.inf
    with pytest.raises(ValueError, match='finite'):
        verify.forecast_skill(fc, va, weights=bad)
    bad[2] = np.nan
    with pytest.raises(ValueError, match='finite'):
        verify.forecast_skill(fc, va, weights=bad)
    with pytest.raises(ValueError, match='all zero'):
        verify.forecast_skill(fc, va, weights=np.zeros(6, np.float32))
    big = labels.copy()
    big[2, 4] = 12
    with pytest.raises(ValueError, match=r'\[-1, 12\)'):
        verify.forecast_skill(fc, va, table, big)
    big[2, 4] = -2
    with pytest.raises(ValueError, match=r'\[-1, 12\)'):
        verify.forecast_skill(fc, va, table, big)
    with pytest.raises(ValueError, match='integers'):
        verify.forecast_skill(fc, va, table, labels.astype(np.float32))
    with pytest.raises(ValueError, match="'weights' must hold one weight per row"):
        verify.forecast_skill(fc, va, weights=np.ones(10, np.float32))                    # the longitude axis
    with pytest.raises(ValueError, match="'axis' must be None"):
        verify.forecast_skill(fc, va, axis=(1, 2, 3))
    with pytest.raises(ValueError, match="'axis' must be None"):
        verify.forecast_skill(fc, va, axis=0, device='cuda')                             # the device path has no other axis either
    with pytest.raises(ValueError, match="'labels' must have shape"):
        verify.forecast_skill(fc, va, table, labels[0])
    with pytest.raises(ValueError, match="needs 'labels'"):
        verify.forecast_skill(fc, va, table)
    with pytest.raises(ValueError, match='without a climatology'):
        verify.forecast_skill(fc, va, labels=labels)
    with pytest.raises(ValueError, match="'climatology' must have the shape"):
        verify.forecast_skill(fc, va, table[:, :1], labels)
    with pytest.raises(TypeError, match="'valid' must be a CUDA float32 tensor"):
        verify.forecast_skill(fc, torch.zeros(va.shape))
    with pytest.raises(TypeError, match="'climatology' must be float32"):
        verify.forecast_skill(fc, va, table.astype(np.float64), labels, device='cuda')
    with pytest.raises(ValueError, match='do not match'):
        verify.persistence_skill(fc[0, :3], va[0], 2)
    # the wrapper's own checks come before the device is looked at
    with pytest.raises(ValueError, match='all zero'):
        ops.skill_weights(np.zeros(3))
    with pytest.raises(ValueError, match='1-D'):
        ops.skill_weights(np.ones((2, 3)))
    assert ops.skill_labels(np.array([[0, -1], [3, 2]], np.int64), 4).tolist() == [0, -1, 3, 2]


def _call(h=NULL, fc=FAKE, ob=FAKE, leads=2, count0=4, count_dec=1, groups=3, run=8, climo=NULL, n_labels=0, labels=NULL, lab=(0, 1),
          weights=NULL, w_len=0, w_inner=1, sums=FAKE, ws=FAKE, ws_bytes=1 << 20, strides=(96, 24, 0, 0, 24, 1)):
    return _lib.lib.dlwp_verify_skill_sums(h, fc, LL(strides[0]), LL(strides[1]), strides[2], ob, LL(strides[3]), LL(strides[4]),
                                           strides[5], leads, count0, count_dec, groups, LL(run), climo, n_labels, labels, LL(lab[0]),
                                           lab[1], weights, w_len, LL(w_inner), sums, ws, ws_bytes, NULL)


def _refused(rc, text):
    assert rc == _lib.EINVAL, rc
    assert text in _lib.lib.dlwp_last_error().decode(), _lib.lib.dlwp_last_error()


def test_entry_point_refuses_in_the_documented_order_without_a_launch():
    """every refusal comes before the handle is looked at, each with the later ones provoked as well: the earlier one is reported"""
    names = _lib.declared_symbols()
    assert 'dlwp_verify_skill_sums' in names and 'dlwp_verify_skill_workspace' in names
    assert len(_lib.lib.dlwp_verify_skill_sums.argtypes) == 26 and _lib.lib.dlwp_verify_skill_workspace.restype is ctypes.c_size_t
    _refused(_call(leads=0, count_dec=-1), 'must all be >= 1')
    _refused(_call(run=0, fc=NULL), 'must all be >= 1')
    _refused(_call(count_dec=-1, climo=FAKE, n_labels=65), 'negative')
    _refused(_call(lab=(-1, 0), fc=NULL), 'negative')
    _refused(_call(strides=(96, 24, 0, 0, -24, 1)), 'negative')
    _refused(_call(climo=FAKE, n_labels=65, labels=FAKE, fc=NULL), 'n_labels 65')
    _refused(_call(climo=FAKE, n_labels=0), 'n_labels 0')
    _refused(_call(labels=FAKE, weights=FAKE, w_len=0), 'labels without')
    _refused(_call(weights=FAKE, w_len=0, w_inner=4, fc=NULL), 'do not divide')
    _refused(_call(weights=FAKE, w_len=2, w_inner=0), 'do not divide')
    _refused(_call(weights=FAKE, w_len=3, w_inner=2, sums=NULL), 'do not divide')          # run 8, period 6
    _refused(_call(weights=FAKE, w_len=2, w_inner=1 << 62), 'do not divide')               # no overflow on the way
    for kw in (dict(fc=NULL), dict(ob=NULL), dict(sums=NULL)):
        _refused(_call(leads=1 << 12, groups=1 << 9, **kw), 'null pointer')
    _refused(_call(leads=1 << 12, groups=(1 << 8) + 1, ws_bytes=0), 'cells')
    _refused(_call(ws_bytes=0), 'workspace too small')
    # 2 leads x 3 groups, rows of 8 floats as 2 quads: lead 0 has 4 x 2 = 8 units -> one block per cell, 6 x 80 bytes
    _refused(_call(ws_bytes=6 * 80 - 1), 'workspace too small (479 < 480)')
    _refused(_call(ws=NULL), 'workspace too small')
    _refused(_call(ws=ctypes.c_void_p(4100)), '8-byte aligned')
    _refused(_call(ws_bytes=6 * 80, weights=FAKE, w_len=2, w_inner=4, climo=FAKE, n_labels=64, labels=FAKE), 'null handle')
    # no lead has pairs: nothing is needed in the workspace, and still no launch without a handle
    _refused(_call(count0=0, ws=NULL, ws_bytes=0), 'null handle')


@pytest.mark.parametrize('leads, groups', [(1, 1), (56, 1), (56, 4), (5, 3), (3000, 2)])
def test_workspace_is_the_documented_product_and_covers_fewer_active_leads(leads, groups):
    got = _lib.lib.dlwp_verify_skill_workspace(NULL, leads, groups)
    assert got == leads * groups * -(-2048 // (leads * groups)) * 80
    assert _lib.lib.dlwp_verify_skill_workspace(NULL, 0, groups) == 0 and _lib.lib.dlwp_verify_skill_workspace(NULL, leads, 0) == 0
    row = groups * 63360
    for count0 in (1, 8, 256):
        _refused(_call(leads=leads, groups=groups, count0=count0, run=63360, ws_bytes=got, strides=(300 * row, row, 0, 0, row, 1)),
                 'null handle')


def test_the_walk_of_a_cell_visits_every_unit_once_and_finds_its_weights():
    """csrc/skill.hip walks a cell by integer arithmetic alone: (row, col) advanced by the host's (step_row, step_col) with one carry,
    the position inside the weight period by (step_wrow, step_wcol) with two carries and no division.  The same arithmetic restated
    here must visit every unit exactly once and give every element the weight index (e // w_inner) % w_len, for 16-byte and scalar
    units, one block and several, periods that a unit straddles, w_inner = 1 and a period as long as the run."""
    def walk(cnt, run, vec, bpc, w_len, w_inner):
        W = 4 if vec else 1
        units, step, period = run // W, bpc * 256, w_inner * w_len
        step_row, step_col = divmod(step, units)
        step_wrow, step_wcol = divmod((step_col * W) % period, w_inner)
        seen = set()
        for q in range(bpc * 256):
            row, col = divmod(q, units)
            wrow, wcol = divmod((W * col) % period, w_inner)
            while row < cnt:
                assert col < units and (row, col) not in seen
                seen.add((row, col))
                er, ec = wrow, wcol
                for k in range(W):
                    assert er == ((W * col + k) // w_inner) % w_len
                    ec += 1
                    if ec == w_inner:
                        ec, er = 0, (0 if er + 1 == w_len else er + 1)
                row, col = row + step_row, col + step_col
                if col >= units:
                    row, col = row + 1, col - units
                wrow, wcol = wrow + step_wrow, wcol + step_wcol
                if wcol >= w_inner:
                    wrow, wcol = wrow + 1, wcol - w_inner
                if wrow >= w_len:
                    wrow -= w_len
        assert len(seen) == cnt * units
    for run, w_len, w_inner in ((120, 6, 10), (60, 6, 10), (144, 6, 12), (90, 5, 9), (45, 5, 9), (8, 2, 1), (8, 8, 1), (24, 3, 2),
                                (4048, 44, 92)):
        for vec in (False, True):
            if vec and run % 4:
                continue
            for cnt in (1, 5, 37):
                for bpc in (1, 2, 3, 7):
                    walk(cnt, run, vec, bpc, w_len, w_inner)


def test_wrapper_refuses_before_the_device_is_looked_at():
    with pytest.raises(RuntimeError, match='device'):
        ops.verify_skill_sums(torch.zeros(8), (0, 8, 0), torch.zeros(8), (0, 8, 0), 1, 1, 0, 1, 8)


def test_kernel_source_keeps_its_promises():
    """structural: no atomics, no host synchronisation, no allocation in csrc/skill.hip; the stream-taking export marks the tape"""
    src = open(os.path.join(ROOT, 'dlwp_amd', 'csrc', 'skill.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    for word in ('atomic', 'Synchronize', 'hipMalloc', 'hipMemcpy', '__threadfence'):
        assert word not in code, word
    assert 'DLWP_UNTAPED(dlwp_verify_skill_sums)' in code
