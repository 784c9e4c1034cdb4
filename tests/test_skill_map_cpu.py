"""Per-grid-point forecast skill without a device: the host path of verify.forecast_skill_map / persistence_skill_map / skill_map_sums
/ finish_skill_map against the float64 restatement of tests/skill_map_cases.py (bounds derived in tests/skill_cases.py), the
identities of the definition, consistency with the merged per-lead scores, every refusal of the public functions, those of the C
entry points in the order include/dlwp_hip.h gives, and the chunk arithmetic of csrc/skill_map.hip restated in integers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import verify
from tests.skill_cases import cosine, data, labels_of, table_of
from tests.skill_map_cases import check_skill_map, forecast_map64, persistence_map64, term_magnitudes, weighted_plane_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
FAKE = ctypes.c_void_p(4096)         # a non-null address for refusals that come before any launch; never dereferenced
NULL = ctypes.c_void_p(0)
INNER = (2, 6, 10)
N = 64                               # samples per lead: kappa <= 2 needs a sample of this size (tests/skill_map_cases.py)


# -- the host path against the restatement ------------------------------------------------------------------------------------------- #
def test_host_path_per_lead_valid_with_table():
    fc, va = data((2, N) + INNER, 1, 7), data((2, N) + INNER, 2, 11)
    table, labels = table_of(INNER, 3), labels_of((2, N), 4)
    labels[1, 2] = -1
    got = verify.forecast_skill_map(fc, va, table, labels)
    got = check_skill_map(got, forecast_map64(fc, va, table, labels), 'host per lead', on_device=False)
    assert got.rmse.shape == (2,) + INNER and got.count.dtype == np.int64 and got.count.max() <= N


def test_host_path_plain_series_one_field_and_bare():
    """6 leads against 70 times: 70 .. 65 samples per point"""
    fc, va = data((6, 72) + INNER, 5), data((70,) + INNER, 6)
    field = table_of(INNER, 7)[3]
    check_skill_map(verify.forecast_skill_map(fc, va, field), forecast_map64(fc, va, field), 'host plain series, one field', False)
    got = check_skill_map(verify.forecast_skill_map(fc, va), forecast_map64(fc, va), 'host plain series, bare', False)
    assert [int(c) for c in got.count[:, 0, 0, 0]] == [70, 69, 68, 67, 66, 65]
    table, labels = table_of(INNER, 8), labels_of((70,), 9)
    check_skill_map(verify.forecast_skill_map(fc, va, table, labels), forecast_map64(fc, va, table, labels), 'host plain series, table',
                    False)


def test_host_path_one_sample_and_leads_beyond_the_series():
    """one verification time, three leads: lead 0 has exactly one pair per point (both variances exactly zero: the correlations are
    NaN, the errors are not), leads 1 and 2 have none (NaN, count 0, zero sums)"""
    fc, va = data((3, 2) + INNER, 10), data((1,) + INNER, 11)
    got = check_skill_map(verify.forecast_skill_map(fc, va), forecast_map64(fc, va), 'host one sample', False)
    assert (got.count[0] == 1).all() and (got.count[1:] == 0).all()
    assert np.isnan(got.acc_centered).all() and not np.isnan(got.rmse[0]).any() and not np.isnan(got.acc[0]).any()
    for name in ('mse', 'rmse', 'mae', 'bias', 'acc'):
        assert np.isnan(getattr(got, name)[1:]).all(), name
    sums = verify.skill_map_sums(fc, va)
    assert sums.shape == (3, 9) + INNER and sums.dtype == np.float64 and (sums[1:] == 0).all()


def test_host_path_persistence():
    pr, va = data((70,) + INNER, 13), data((68,) + INNER, 14, 23)
    table, labels = table_of(INNER, 15), labels_of((68,), 16)
    got = verify.persistence_skill_map(pr, va, 4, table, labels)
    check_skill_map(got, persistence_map64(pr, va, 4, table, labels), 'host persistence', False)
    check_skill_map(verify.persistence_skill_map(pr, va, 2), persistence_map64(pr, va, 2), 'host persistence bare', False)


# -- identities ---------------------------------------------------------------------------------------------------------------------- #
def test_identities_of_the_definition():
    va = data((2, N) + INNER, 18)
    table, labels = table_of(INNER, 19), labels_of((2, N), 20)
    same = verify.forecast_skill_map(va.copy(), va, table, labels)
    assert (same.acc == 1).all() and (same.bias == 0).all() and (same.rmse == 0).all() and (same.mae == 0).all()
    # fa = -oa exactly: no climatology, the forecast is the negated truth.  sqrt(fl(x * x)) == |x| in binary arithmetic
    assert (verify.forecast_skill_map(-va, va).acc == -1).all()
    # forecast = fl(valid + 2), |valid + 2| < 32: the sum is off by at most half an ulp there (2^-20), d = fl(forecast - valid) by
    # 2^-23 more, the cast by 2^-23: a mean of such terms is within 2^-19 of 2
    assert np.abs(va + 2).max() < 32
    shifted = verify.forecast_skill_map(va + np.float32(2), va, table, labels)
    assert (np.abs(shifted.bias.astype(np.float64) - 2.0) <= 2.0 ** -19).all()
    assert (np.abs(shifted.rmse.astype(np.float64) - 2.0) <= 2.0 ** -19).all()


# -- consistency with the merged per-lead scores ------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'area_weights'])
def test_planes_add_up_to_the_sums_of_forecast_skill(weighted):
    """sum over points of w_e x plane k is S_k of the per-lead definition: two float64 orders of addition over n terms differ by at
    most n 2^-52 sum |term|; the counts add exactly"""
    fc, va = data((2, N) + INNER, 21, 13), data((2, N) + INNER, 22)
    table, labels = table_of(INNER, 23), labels_of((2, N), 24)
    labels[0, 5] = -1
    w = cosine(6) if weighted else None
    w_e = np.broadcast_to((np.ones(6) if w is None else w.astype(np.float64)).reshape(1, 6, 1), INNER)
    plan = verify.plan_forecast_skill(fc.shape, va.shape, None)
    flat = ops.skill_labels(labels, 12)
    want = verify._skill_host(lambda f, cnt: fc[f, :cnt], lambda f, cnt: va[f, :cnt], plan, INNER, table, flat, w)[:, 0]
    got = weighted_plane_sums(verify.skill_map_sums(fc, va, table, labels), w_e)
    n = N * int(np.prod(INNER))
    bound = n * 2.0 ** -52 * term_magnitudes(fc, va, table, labels, w_e)
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
    assert np.array_equal(got[:, 9], want[:, 9]) and (want[:, 9] < n).all() and (want[:, 9] > 0).all()


def test_finish_skill_map_of_added_tables_is_the_table_of_all_samples():
    fc, va = data((2, 2 * N) + INNER, 25, 17), data((2, 2 * N) + INNER, 26)
    table, labels = table_of(INNER, 27), labels_of((2, 2 * N), 28)
    a = verify.skill_map_sums(fc[:, :N], va[:, :N], table, labels[:, :N])
    b = verify.skill_map_sums(fc[:, N:], va[:, N:], table, labels[:, N:])
    got = check_skill_map(verify.finish_skill_map(a + b), forecast_map64(fc, va, table, labels), 'added tables', False)
    assert np.array_equal(got.count, (a[:, 8] + b[:, 8]).astype(np.int64))
    whole = verify.forecast_skill_map(fc, va, table, labels)
    assert np.array_equal(got.count, whole.count) and np.array_equal(got.mae.shape, whole.mae.shape)
    # a table with an empty lead and with a single sample finishes to NaN where finish_skill does
    z = np.zeros((2, 9, 3))
    z[1, 8], z[1, 0], z[1, 1], z[1, 2] = 1, 2, 4, 2
    fin = verify.finish_skill_map(z)
    assert np.isnan(fin.mse[0]).all() and (fin.count[0] == 0).all() and (fin.mse[1] == 4).all() and (fin.bias[1] == 2).all()
    assert np.isnan(fin.acc).all() and np.isnan(fin.acc_centered).all()


# -- refusals ------------------------------------------------------------------------------------------------------------------------ #
def test_refusals_of_the_public_functions():
    fc, va = data((3, 5) + INNER, 27), data((3, 5) + INNER, 28)
    table, labels = table_of(INNER, 29), labels_of((3, 5), 30)
    big = labels.copy()
    big[2, 4] = 12
    with pytest.raises(ValueError, match=r'\[-1, 12\)'):
        verify.forecast_skill_map(fc, va, table, big)
    big[2, 4] = -2
    with pytest.raises(ValueError, match=r'\[-1, 12\)'):
        verify.skill_map_sums(fc, va, table, big)
    with pytest.raises(ValueError, match='integers'):
        verify.forecast_skill_map(fc, va, table, labels.astype(np.float32))
    with pytest.raises(ValueError, match="'labels' must have shape"):
        verify.forecast_skill_map(fc, va, table, labels[0])
    with pytest.raises(ValueError, match="needs 'labels'"):
        verify.forecast_skill_map(fc, va, table)
    with pytest.raises(ValueError, match='without a climatology'):
        verify.forecast_skill_map(fc, va, labels=labels)
    with pytest.raises(ValueError, match="need a \\(L, ...\\) climatology table"):
        verify.forecast_skill_map(fc, va, table[0], labels)
    with pytest.raises(ValueError, match="'climatology' must have the shape"):
        verify.forecast_skill_map(fc, va, table[:, :1], labels)
    with pytest.raises(ValueError, match='do not match'):
        verify.forecast_skill_map(fc, va[:, :, :1])
    with pytest.raises(ValueError, match='do not match'):
        verify.forecast_skill_map(fc[:, :4], va[0])                                       # fewer forecasts than verification times
    with pytest.raises(ValueError, match='do not match'):
        verify.persistence_skill_map(fc[0, :3], va[0], 2)
    with pytest.raises(ValueError, match="'n_fhour' must be >= 1"):
        verify.persistence_skill_map(fc[0], va[0], 0)
    with pytest.raises(ValueError, match="'split' must be >= 0"):
        verify.skill_map_sums(fc, va, split=-1)
    with pytest.raises(TypeError, match="'valid' must be a CUDA float32 tensor"):
        verify.forecast_skill_map(fc, torch.zeros(va.shape))
    with pytest.raises(TypeError, match="'climatology' must be float32"):
        verify.forecast_skill_map(fc, va, table.astype(np.float64), labels, device='cuda')
    with pytest.raises(TypeError, match="'forecast' must be float32"):
        verify.skill_map_sums(fc.astype(np.float64), va, device='cuda')
    with pytest.raises(ValueError, match="'device' must be a CUDA device"):
        verify.forecast_skill_map(fc, va, device='cpu')
    with pytest.raises(ValueError, match=r'\(leads, 9, \.\.\.\)'):
        verify.finish_skill_map(np.zeros((3, 10, 4)))
    with pytest.raises(ValueError, match=r'\(leads, 9, \.\.\.\)'):
        verify.finish_skill_map(np.zeros((3, 9)))
    # the wrappers' own checks come before the device is looked at
    with pytest.raises(RuntimeError, match='device'):
        ops.verify_skill_map(torch.zeros(8), (0, 8, 0), torch.zeros(8), (0, 8, 0), 1, 1, 0, 8)
    with pytest.raises(RuntimeError, match='device'):
        ops.verify_skill_map_finish(torch.zeros((1, 9, 4), dtype=torch.float64))
    with pytest.raises(TypeError, match='float64'):
        ops.verify_skill_map_finish(torch.zeros((1, 9, 4)))
    with pytest.raises(ValueError, match=r'\(leads >= 1, 9, \.\.\.\)'):
        ops.verify_skill_map_finish(torch.zeros((1, 8, 4), dtype=torch.float64))


def _call(h=NULL, fc=FAKE, ob=FAKE, leads=2, count0=4, count_dec=1, row=24, climo=NULL, n_labels=0, labels=NULL, lab=(0, 1), split=1,
          sums=FAKE, scores=FAKE, counts=FAKE, ws=FAKE, ws_bytes=1 << 20, strides=(96, 24, 0, 0, 24, 1)):
    return _lib.lib.dlwp_verify_skill_map(h, fc, LL(strides[0]), LL(strides[1]), strides[2], ob, LL(strides[3]), LL(strides[4]),
                                          strides[5], leads, count0, count_dec, LL(row), climo, n_labels, labels, LL(lab[0]), lab[1],
                                          split, sums, scores, counts, ws, ws_bytes, NULL)


def _refused(rc, text):
    assert rc == _lib.EINVAL, rc
    assert text in _lib.lib.dlwp_last_error().decode(), _lib.lib.dlwp_last_error()


def test_entry_point_refuses_in_the_documented_order_without_a_launch():
    """every refusal comes before the handle is looked at, each with a later one provoked as well: the earlier one is reported"""
    names = _lib.declared_symbols()
    assert {'dlwp_verify_skill_map', 'dlwp_verify_skill_map_workspace', 'dlwp_verify_skill_map_finish'} <= set(names)
    assert len(_lib.lib.dlwp_verify_skill_map.argtypes) == 25 and _lib.lib.dlwp_verify_skill_map_workspace.restype is ctypes.c_size_t
    none = dict(sums=NULL, scores=NULL, counts=NULL)
    _refused(_call(leads=0, count_dec=-1), 'must be >= 1')
    _refused(_call(row=0, fc=NULL), 'must be >= 1')
    _refused(_call(count_dec=-1, climo=FAKE, n_labels=65), 'negative')
    _refused(_call(lab=(-1, 0), fc=NULL), 'negative')
    _refused(_call(lab=(0, -1), split=-1), 'negative')
    _refused(_call(strides=(96, 24, 0, 0, -24, 1)), 'negative')
    _refused(_call(strides=(96, 24, -1, 0, 24, 1), **none), 'negative')
    _refused(_call(climo=FAKE, n_labels=65, labels=FAKE, fc=NULL), 'n_labels 65')
    _refused(_call(climo=FAKE, n_labels=0, **none), 'n_labels 0')
    _refused(_call(labels=FAKE, **none), 'labels without')
    _refused(_call(labels=FAKE, split=-1), 'labels without')
    for kw in (dict(fc=NULL), dict(ob=NULL), none):
        _refused(_call(split=-1, **kw), 'no output at all')
    _refused(_call(split=-1, ws_bytes=0), 'split -1')
    _refused(_call(split=-5, row=1 << 40), 'split -5')
    # 2^30 scalar columns (the strides are odd) are 2^22 tiles; 256 leads x 2 chunks x 2^22 tiles = 2^31 blocks
    _refused(_call(leads=256, count0=4, count_dec=0, split=2, row=1 << 30, ws_bytes=0, strides=(0, 1, 0, 0, 1, 0)), 'too long')
    _refused(_call(leads=256, count0=4, count_dec=0, split=7, row=1 << 30, ws_bytes=0, strides=(0, 1, 0, 0, 1, 0)), 'in 4 chunks')
    # 2 leads x 2 chunks x 9 planes x 24 points x 8 bytes
    _refused(_call(split=2, ws_bytes=0), 'workspace too small (0 < 6912)')
    _refused(_call(split=2, ws_bytes=6911), 'workspace too small (6911 < 6912)')
    _refused(_call(split=9, ws_bytes=4 * 3456 - 1), 'workspace too small (13823 < 13824)')      # capped at count0 = 4 chunks
    _refused(_call(split=2, ws=NULL), 'workspace too small')
    _refused(_call(split=2, ws=ctypes.c_void_p(4100)), '8-byte aligned')
    _refused(_call(split=2, ws_bytes=6912, climo=FAKE, n_labels=64, labels=FAKE), 'null handle')
    # one chunk needs no workspace; each output alone is enough; no lead with pairs still launches nothing without a handle
    _refused(_call(split=1, ws=NULL, ws_bytes=0), 'null handle')
    for keep in ('sums', 'scores', 'counts'):
        _refused(_call(ws=NULL, ws_bytes=0, **{k: v for k, v in none.items() if k != keep}), 'null handle')
    _refused(_call(count0=0, split=0, ws=NULL, ws_bytes=0), 'null handle')
    _refused(_call(count0=-3, split=5, ws=NULL, ws_bytes=0), 'null handle')


def test_finish_entry_point_refuses_in_the_documented_order():
    fin = _lib.lib.dlwp_verify_skill_map_finish
    assert len(fin.argtypes) == 6
    _refused(fin(NULL, NULL, LL(0), NULL, NULL, NULL), 'cells 0 must be >= 1')
    _refused(fin(NULL, NULL, LL(8), FAKE, FAKE, NULL), 'no output at all')
    _refused(fin(NULL, FAKE, LL(8), NULL, NULL, NULL), 'no output at all')
    _refused(fin(NULL, FAKE, LL(1 << 40), FAKE, NULL, NULL), 'too long')
    _refused(fin(NULL, FAKE, LL(8), FAKE, NULL, NULL), 'null handle')
    _refused(fin(NULL, FAKE, LL(8), NULL, FAKE, NULL), 'null handle')


@pytest.mark.parametrize('leads, count0, row', [(1, 256, 63360), (56, 256, 63360), (2, 64, 120), (2, 3, 120), (3, 64, 45), (1, 0, 8)])
def test_workspace_is_the_documented_product(leads, count0, row):
    """split = 0 without a handle: min(max(1, 8 * 256 / (leads * tiles)), count0) chunks with the tiles of the 16-byte route where the
    row allows it; one chunk needs no workspace; a positive split is taken as given and capped at count0"""
    ws = _lib.lib.dlwp_verify_skill_map_workspace
    tiles = -(-(row // 4 if row % 4 == 0 else row) // 256)
    auto = max(1, min(max(1, 2048 // (leads * tiles)), count0))
    assert ws(NULL, leads, count0, LL(row), 0) == (leads * auto * 9 * row * 8 if auto > 1 else 0)
    assert ws(NULL, leads, count0, LL(row), 1) == 0
    for split in (2, 3, 300):
        s = max(1, min(split, count0))
        assert ws(NULL, leads, count0, LL(row), split) == (leads * s * 9 * row * 8 if s > 1 else 0)
        if count0 > 0:
            _refused(_call(leads=leads, count0=count0, count_dec=0, row=row, split=split, ws_bytes=ws(NULL, leads, count0, LL(row), split),
                           strides=(count0 * row, row, 0, count0 * row, row, 0)), 'null handle')
    assert ws(NULL, 0, count0, LL(row), 0) == 0 and ws(NULL, leads, count0, LL(0), 0) == 0 and ws(NULL, leads, count0, LL(row), -1) == 0
    assert (auto > 1) == (leads * tiles <= 1024 and count0 > 1)         # the samples are split only when the chip is not filled


def test_every_sample_of_every_lead_falls_in_exactly_one_chunk():
    """csrc/skill_map.hip cuts the cnt_f samples of lead f into chunks [cnt_f k / split, cnt_f (k + 1) / split) with split capped at
    count0: restated in integers, the chunks of a lead are disjoint, in order, and cover 0 .. cnt_f - 1, for every count 0 .. 70, every
    split 1 .. count and the shrinking counts of a plain series; a walk in steps of U with a clamped tail visits the same samples"""
    for count0 in range(0, 71):
        for split in range(1, max(count0, 1) + 1):
            chunks = max(1, min(split, count0))
            assert chunks == split or count0 == 0
            for cnt in {count0, max(count0 - 3, 0), max(count0 - 69, 0), min(count0, 1)}:
                seen = []
                for k in range(chunks):
                    lo, end = cnt * k // chunks, cnt * (k + 1) // chunks
                    assert 0 <= lo <= end <= cnt
                    for unroll in (2, 4):
                        walked = []
                        for i in range(lo, end, unroll):
                            for u in range(unroll):
                                r = i + u if i + u < end else end - 1
                                assert lo <= r < end                     # what is loaded is a row of this chunk
                                if i + u < end:
                                    walked.append(r)
                        assert walked == list(range(lo, end))
                    seen += list(range(lo, end))
                assert seen == list(range(cnt)), (count0, split, cnt)


def test_kernel_source_keeps_its_promises():
    """structural: no atomics, no host synchronisation, no allocation in csrc/skill_map.hip; both stream-taking exports mark the tape;
    the finishing arithmetic is compiled without contraction"""
    src = open(os.path.join(ROOT, 'dlwp_amd', 'csrc', 'skill_map.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    for word in ('atomic', 'Synchronize', 'hipMalloc', 'hipMemcpy', '__threadfence'):
        assert word not in code, word
    assert 'DLWP_UNTAPED(dlwp_verify_skill_map)' in code and 'DLWP_UNTAPED(dlwp_verify_skill_map_finish)' in code
    assert '#pragma clang fp contract(off)' in code
