"""Ensemble event verification on the device (csrc/events.hip behind dlwp_amd.model.ensemble) against the brute-force restatement of
tests/event_cases.py on the same float32 inputs.  Every comparison is an EQUALITY: the table is integer, the probability field is
float32(n / M) with all its bits defined, and the derived scores come from the same table through the same finish_events as the host
path, so they must match it bit for bit.  The cases cover every kernel instance (one or four columns per lane, 1 / 2 / 4 / 8
counters, both events, thresholds per group and per point), both table updates (plain LDS adds on 16 or 32 replicas; wave
aggregation where the table leaves room for fewer: K (M + 1) 2 > 640 bins), ragged tiles and the strided tile loop."""
import ctypes

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import ensemble
from tests.event_cases import check_case, events64, inputs, per_point, same_bits, thresholds

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
    return np.ascontiguousarray(np.moveaxis(x, 2, 1))


def device_counts(xd, yd, thr, below, grouped, member_axis, dims, misalign_thr=False):
    """dlwp_ens_event_counts through ops on device tensors: (table numpy (T[, G], K, M + 1, 2), prob numpy (K, T, S, *field))"""
    t_n, s_n, m, field = dims
    groups, run = (field[0], int(np.prod(field[1:]))) if grouped else (1, int(np.prod(field)))
    thr = np.asarray(thr, np.float32)
    pp = thr.ndim > 1
    thr_d = cuda(thr if pp else np.repeat(thr[:, None], groups, axis=1), misalign_thr)
    table, prob = ops.ens_event_counts(xd, ops.ens_strides(s_n, m, groups * run, member_axis), yd, thr_d, pp, below, t_n, s_n, m, groups,
                                       run, want_table=True, want_prob=True)
    assert table.dtype == torch.int64 and prob.dtype == torch.float32
    table = table.cpu().numpy()
    return (table if grouped else table[:, 0]), prob.cpu().numpy().reshape((thr.shape[0], t_n, s_n) + tuple(field))


def check_all(x, y, thr_kinds, what, wide=True, quality=True):
    """both events x grouped / ungrouped x the given thresholds x both member layouts: table equal, prob bit-equal.  The restatement
    is computed once per (event, grouping, thresholds) and shared by the layouts."""
    dims = (x.shape[0], x.shape[1], x.shape[2], x.shape[3:])
    columns = int(np.prod(y.shape))
    yd = cuda(y)
    layouts = ((2, cuda(x)), (1, cuda(members_first(x))))
    for kind, thr in thr_kinds:
        for below in (False, True):
            for grouped in (False, True):
                want = events64(x, y, thr, below, grouped, derived=False)
                if quality:
                    check_case(want, columns, wide)
                for member_axis, xd in layouts:
                    tag = '%s %s below=%s grouped=%s axis %d' % (what, kind, below, grouped, member_axis)
                    table, prob = device_counts(xd, yd, thr, below, grouped, member_axis, dims)
                    assert np.array_equal(table, want['table']), tag
                    assert same_bits(prob, want['prob']), tag


#: (4, 5, 7): ungrouped run = 140, four columns per lane in one ragged tile; grouped run = 35 < 64, one column per lane
@pytest.mark.parametrize('members', [2, 3, 8, 31, 32, 33, 256])
@pytest.mark.parametrize('k_n', [1, 3, 8])
def test_table_and_probability_equal_the_restatement(members, k_n):
    x, y = inputs((2, 3, members, 4, 5, 7), 4000 + members)
    check_all(x, y, (('per group', thresholds(k_n)), ('per point', per_point(k_n, (4, 5, 7), 7))), 'M=%d K=%d' % (members, k_n))


@pytest.mark.parametrize('members', [2, 8, 33, 256])
def test_a_sharp_ensemble_puts_a_wave_in_one_bin(members):
    x, y = inputs((2, 3, members, 4, 5, 7), 5000 + members, spread=0.01)
    check_all(x, y, (('per group', thresholds(3)),), 'sharp M=%d' % members, wide=False)


#: (4, 8, 16): whole quads, run = 128 / 512; (1, 1, 129): row not a multiple of 4, run = 2 * 64 + 1; (2, 3, 171): one column per lane over
#: 2 * 256 + 1 and 4 * 256 + 2 points (several tiles, a one-point tail); (2, 4, 257): four columns per lane over 1024 + 4 and
#: 2 * 1024 + 8 points (several tiles, a one-quad tail)
@pytest.mark.parametrize('field', [(4, 8, 16), (1, 1, 129), (2, 3, 171), (2, 4, 257)])
def test_field_sizes_and_tails(field):
    for members, k_n in ((3, 3), (40, 8)):
        x, y = inputs((2, 2, members) + field, 6000 + members + field[-1])
        check_all(x, y, (('per group', thresholds(k_n)), ('per point', per_point(k_n, field, 8))), 'field %r M=%d' % (field, members),
                  quality=False)


def test_a_misaligned_base_falls_back_to_one_column_per_lane():
    field = (4, 8, 16)
    x, y = inputs((2, 3, 8) + field, 6100)
    dims = (2, 3, 8, field)
    for thr in (thresholds(3), per_point(3, field, 9)):
        want = events64(x, y, thr, False, True, derived=False)
        for off_x, off_y, off_t in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
            table, prob = device_counts(cuda(x, off_x), cuda(y, off_y), thr, False, True, 2, dims, misalign_thr=off_t)
            assert np.array_equal(table, want['table']) and same_bits(prob, want['prob']), (off_x, off_y, off_t)


def _tail_case(vec):
    """More tiles per cell than blocks per cell.  The grid cap is (CUs * blocks per CU) / cells blocks per cell, which the workspace
    query reports: bytes / (cells * K (M + 1) 2 * 4).  One column per lane: 16 leads x 8 groups = 128 cells (cap 20 on 256 CUs),
    3 samples x ceil(1793 / 256) = 24 tiles per cell.  Four columns per lane: 64 x 8 = 512 cells (cap 5), 2 samples x
    ceil(2052 / 1024) = 6 tiles per cell.  M = 2, K = 1: 5.5 MB and 16.8 MB."""
    leads, samples, groups, run, tile = (64, 2, 8, 2052, 1024) if vec else (16, 3, 8, 1793, 256)
    cells, tiles = leads * groups, samples * -(-run // tile)
    cap = ops.ens_event_workspace(torch.cuda.current_device(), leads, groups, 2, 1) // (cells * 3 * 2 * 4)
    assert 1 <= cap < tiles, (cap, tiles)
    x, y = inputs((leads, samples, 2, groups, 1, run), 7000 + run)
    return x, y, (leads, samples, 2, (groups, 1, run))


@pytest.mark.parametrize('vec', [False, True])
def test_strided_tile_loop(vec):
    x, y, dims = _tail_case(vec)
    thr = thresholds(1)
    want = events64(x, y, thr, False, True, derived=False)
    check_case(want, int(np.prod(y.shape)), True)
    table, prob = device_counts(cuda(x), cuda(y), thr, False, True, 2, dims)
    assert np.array_equal(table, want['table']) and same_bits(prob, want['prob'])


@pytest.mark.parametrize('members,k_n', [(8, 8), (40, 8), (256, 3)])
def test_both_update_regimes(members, k_n):
    """(8, 8): 144 bins on 32 replicas, plain adds; (40, 8) and (256, 3): 656 bins on 8 and 1542 on 4 replicas, wave aggregation"""
    dims = (1, 1, members, (1, 1, 1000))
    # every column in one bin: a threshold far in the tail, n = 0 and the event never verified
    x, y = inputs((1, 1, members, 1, 1, 1000), 8000 + members)
    counted = int((~(np.isnan(y) | np.isnan(x).any(axis=2))).sum())
    assert 500 < counted < 1000
    thr = np.full(k_n, 1e30, np.float32)
    table, _ = device_counts(cuda(x), cuda(y), thr, False, False, 2, dims)
    assert (table[0, :, 0, 0] == counted).all() and table.sum() == k_n * counted
    table, _ = device_counts(cuda(x), cuda(y), -thr, False, False, 2, dims)          # and n = M, verified
    assert (table[0, :, members, 1] == counted).all() and table.sum() == k_n * counted
    # neighbouring lanes in different bins: point p has exactly p mod (M + 1) members above the threshold
    n = np.arange(1000) % (members + 1)
    x = (np.arange(members)[:, None] < n[None, :]).astype(np.float32).reshape(1, 1, members, 1, 1, 1000)
    y = (np.arange(1000) % 2).astype(np.float32).reshape(1, 1, 1, 1, 1000)
    thr = np.full(k_n, 0.5, np.float32)
    want = events64(x, y, thr, False, False, derived=False)
    assert (want['table'].sum(axis=-1) > 0).all() and (want['table'][0, 0].sum(axis=-1) == np.bincount(n, minlength=members + 1)).all()
    for scalar in (False, True):                                                   # four columns per lane; one (a misaligned base)
        table, prob = device_counts(cuda(x, scalar), cuda(y), thr, False, False, 2, dims)
        assert np.array_equal(table, want['table']) and same_bits(prob, want['prob'])


def test_repeated_calls_give_identical_tables():
    x, y, dims = _tail_case(False)
    xd, yd = cuda(x), cuda(y)
    thr = torch.from_numpy(np.repeat(thresholds(3)[:, None], 8, axis=1)).cuda()
    st = ops.ens_strides(dims[1], 2, 8 * 1793, 2)
    one = ops.ens_event_counts(xd, st, yd, thr, False, False, dims[0], dims[1], 2, 8, 1793, want_prob=True)
    two = ops.ens_event_counts(xd, st, yd, thr, False, False, dims[0], dims[1], 2, 8, 1793, want_prob=True)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1].view(torch.int32), two[1].view(torch.int32))
    only = ops.ens_event_counts(xd, st, None, thr, False, False, dims[0], dims[1], 2, 8, 1793, want_table=False, want_prob=True)
    assert only[0] is None and torch.equal(only[1].view(torch.int32), one[1].view(torch.int32))


def test_a_workspace_one_byte_short_is_refused_without_a_launch():
    x, y, dims = _tail_case(False)                               # more tiles than the cap: the call needs all the query reports
    xd, yd = cuda(x), cuda(y)
    thr = torch.zeros((1, 8), dtype=torch.float32, device='cuda')
    dev = torch.cuda.current_device()
    need = ops.ens_event_workspace(dev, 16, 8, 2, 1)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    table = torch.full((16, 8, 1, 3, 2), -7, dtype=torch.int64, device='cuda')
    st = ops.ens_strides(3, 2, 8 * 1793, 2)
    LL = ctypes.c_longlong

    def call(ws_bytes):
        return _lib.lib.dlwp_ens_event_counts(_lib.handle(dev), xd.data_ptr(), LL(st[0]), LL(st[1]), LL(st[2]), yd.data_ptr(), thr.data_ptr(),
                                              0, 0, 16, 3, 2, 8, LL(1793), 1, table.data_ptr(), None, ws.data_ptr(), ws_bytes,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(need - 1) != 0 and b'workspace too small' in _lib.lib.dlwp_last_error()
    torch.cuda.synchronize()
    assert (table == -7).all()                                   # nothing ran
    assert call(need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), events64(x, y, np.zeros(1, np.float32), False, True, derived=False)['table'])
    with pytest.raises(ValueError, match='workspace holds'):
        ops.ens_event_counts(xd, st, yd, thr, False, False, 16, 3, 2, 8, 1793, ws=ws[:need - 1])


def _same_scores(dev, host, prob):
    for name, a, b in zip(dev._fields[:-1], dev[:-1], host[:-1]):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, name
        if a.dtype == np.float32:
            assert same_bits(a, b), name
        else:
            assert np.array_equal(a, b), name
    if prob:
        assert dev.prob_field.is_cuda and same_bits(dev.prob_field.cpu().numpy(), host.prob_field)
    else:
        assert dev.prob_field is None and host.prob_field is None


@pytest.mark.parametrize('members', [3, 8, 40])
def test_event_scores_on_the_device_equal_the_host_path_bit_for_bit(members):
    field = (4, 8, 16)
    x, y = inputs((2, 3, members) + field, 9000 + members)
    thr_kinds = (thresholds(3), per_point(3, field, 10), thresholds(8)[:, None, None, None] + np.zeros((1, 4, 1, 1), np.float32))
    for member_axis, xh in ((2, x), (1, members_first(x))):
        xd, yd = cuda(xh), cuda(y)
        for thr in thr_kinds:
            for event in ('above', 'below'):
                for axis in (None, (1, 3, 4)):
                    prob = axis is None
                    dev = ensemble.event_scores(xd, yd, thr, member_axis=member_axis, axis=axis, event=event, prob_field=prob)
                    host = ensemble.event_scores(xh, y, thr, member_axis=member_axis, axis=axis, event=event, prob_field=prob)
                    _same_scores(dev, host, prob)
            got = ensemble.ensemble_exceedance(xd, thr, member_axis=member_axis, event='below')
            assert got.is_cuda and same_bits(got.cpu().numpy(), ensemble.ensemble_exceedance(xh, thr, member_axis=member_axis, event='below'))
    # numpy operands with device='cuda' come back as numpy; an axis the device does not cover runs the host code on a download
    dev = ensemble.event_scores(x, y, thresholds(3), prob_field=True, device='cuda')
    host = ensemble.event_scores(x, y, thresholds(3), prob_field=True)
    assert isinstance(dev.prob_field, np.ndarray) and same_bits(dev.prob_field, host.prob_field) and np.array_equal(dev.table, host.table)
    assert np.array_equal(ensemble.event_scores(cuda(x), cuda(y), thresholds(3), axis=(1,)).table,
                          ensemble.event_scores(x, y, thresholds(3), axis=(1,)).table)
    with pytest.raises(ValueError, match='9 thresholds'):
        ensemble.event_scores(cuda(x), cuda(y), np.linspace(0.0, 1.0, 9))


def test_generate_and_score_without_a_host_array():
    """perturb_members makes 3 x 8 members on the device, event_scores reads them where they are; the downloaded ensemble gives the
    same scores through the host path"""
    rng = np.random.default_rng(17)
    state = torch.from_numpy((rng.standard_normal((3, 4, 8, 16)) * 3.0 + 1.0).astype(np.float32)).cuda()
    for member_axis in (2, 1):
        ens = ensemble.perturb_members(state, 8, stddev=1.0, length=1.0, seed=5, member_axis=member_axis)
        assert ens.is_cuda and tuple(ens.shape) == (24, 4, 8, 16)
        fc = ens.view((1, 3, 8, 4, 8, 16) if member_axis == 2 else (1, 8, 3, 4, 8, 16))
        valid = (state + torch.from_numpy(rng.standard_normal((3, 4, 8, 16)).astype(np.float32)).cuda()).view(1, 3, 4, 8, 16)
        for axis in (None, (1, 3, 4)):
            dev = ensemble.event_scores(fc, valid, thresholds(3), member_axis=member_axis, axis=axis, prob_field=True)
            host = ensemble.event_scores(fc.cpu().numpy(), valid.cpu().numpy(), thresholds(3), member_axis=member_axis, axis=axis,
                                         prob_field=True)
            _same_scores(dev, host, True)
            assert (dev.count == (1536 if axis is None else 384)).all() and (dev.fcst_hist[..., 1:-1].sum(axis=-1) > 0).all()
