"""The label kernels and the row gather of csrc/verify.hip on the device, and the functions of dlwp_amd.model.verify built on them,
against the float64 restatement of tests/verify_climo_cases.py (not the reference run: its functions need xarray).

Bounds.  A table entry is one float64 sum divided once and rounded once to float32; on dyadic data (multiples of 2^-6 below 2^10,
at most 301 of them) every partial sum is exact, so the table has the restatement's bits whatever the chunks are.  On Gaussian data
the chunked float64 sum can differ from the sequential one in its last bits, which can move the float32 rounding by one ulp: that is
the bound, and the share of elements that differ is printed, not gated.  The error sums carry the 2^-22 of tests/test_gpu_verify.py
(d rounded once in float32, float64 behind it) and are compared with the restatement evaluated on the device's own downloaded table.
Run with -s to see the figures."""
import ctypes

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import verify
from dlwp_amd.model.generators import LabeledArray, SeriesDataset
from tests.nets import cnn2_layers
from tests.verify_climo_cases import (BOUND, INNER, METHODS, bits, climo_record, error_sums64, gap_record, label_mean64, month_of,
                                      monthly64, same_bits_nan_exact)

pytestmark = pytest.mark.gpu

LL = ctypes.c_longlong
FAKE = ctypes.c_void_p(4096)         # a non-null address for refusals that come before any launch; never dereferenced
NULL = ctypes.c_void_p(0)
# 108 = 4 x 27 and 32 take the 16-byte route (27 quads: no multiple of the block), 4 x 8 x 12 with an inner shape; 107 is no multiple
# of 4 and takes scalar loads, as every offset view below does
ROWS = [(108,), (107,), (32,), (4, 8, 12)]
COUNTS = [1, 37, 301]
LABELS = [1, 2, 12, 64]


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def cuda(x, misalign=False):
    """x on the device; misalign: an offset view one float into a larger buffer, so the address is 4 (mod 16)"""
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if not misalign:
        assert t.data_ptr() % 16 == 0
        return t
    store = torch.empty(t.numel() + 4, dtype=torch.float32, device='cuda')
    out = store[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def data(shape, seed, dyadic):
    rng = np.random.default_rng(seed)
    if dyadic:
        x = (rng.integers(-(1 << 16) + 1, 1 << 16, shape) / 64.0).astype(np.float32)
    else:
        x = (rng.standard_normal(shape) * 3.0 + 1.0).astype(np.float32)
    x.reshape(-1)[seed % 7::11] = np.nan
    return x


def labels_for(count, n_labels, seed):
    """half of the samples carry label 0 (a long list), the rest are spread; the last label of three or more carries none"""
    rng = np.random.default_rng(seed)
    top = n_labels - 1 if n_labels >= 3 else n_labels
    lab = rng.integers(0, top, count).astype(np.int32)
    lab[rng.random(count) < 0.5] = 0
    return lab


def split_of(x, n_labels):
    """the chunks per label, from the workspace size: n_labels * split * row * 12 bytes"""
    row = int(x[0].numel())
    nbytes = ops.verify_label_nanmean_workspace(x, n_labels)
    assert nbytes % (n_labels * row * 12) == 0
    return nbytes // (n_labels * row * 12)


def ulps(got, want32):
    return np.abs(bits(got).astype(np.int64) - bits(want32).astype(np.int64))


# -- dlwp_verify_label_nanmean --------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope='module')
def mean_cases():
    """every (row, count, labels) case once: inputs, labels and the float64 table, for dyadic and Gaussian data"""
    cases = {}
    for r, row in enumerate(ROWS):
        for count in COUNTS:
            for dy in (True, False):
                x = data((count,) + row, 100 + 10 * r + count % 7 + dy, dy)
                if count > 2:
                    x[:, 0] = np.nan                      # a column without a sample in every label
                for n_labels in LABELS:
                    lab = labels_for(count, n_labels, 3 * count + n_labels)
                    cases[(row, count, n_labels, dy)] = (x, lab, label_mean64(x, lab, n_labels))
    return cases


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('row', ROWS, ids=str)
def test_label_nanmean_bit_equal_on_dyadic_one_ulp_on_gaussian(mean_cases, row, count):
    for n_labels in LABELS:
        for dy in (True, False):
            x, lab, want = mean_cases[(row, count, n_labels, dy)]
            xd = cuda(x)
            got = ops.verify_label_nanmean(xd, lab, n_labels)
            again = ops.verify_label_nanmean(xd, lab, n_labels)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n_labels,) + row
            assert torch.equal(got.view(torch.int32), again.view(torch.int32))              # two launches, identical bits
            got, want32 = got.cpu().numpy(), want.astype(np.float32)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            empty = np.bincount(lab, minlength=n_labels) == 0
            assert np.isnan(got[empty]).all()
            if n_labels >= 3:
                assert empty[-1]                                                            # a label with no sample at all
            if dy:
                same_bits_nan_exact(got, want32)
            else:
                ok = ~np.isnan(want)
                off = ulps(got[ok], want32[ok])
                print('label_nanmean %s count %d labels %d split %d: %.4f of %d elements differ by one ulp' % (
                    row, count, n_labels, split_of(xd, n_labels), float((off > 0).mean()) if off.size else 0.0, off.size))
                assert (off <= 1).all()


def test_label_nanmean_time_split_empty_chunks_and_ragged_boundaries():
    """few labels and a short row: the sample axis must be split (read off the workspace size).  Label 1 has fewer samples than there
    are chunks, so most of its chunks are empty; with 64 labels and rows of 108 the split is smaller than label 0's list and does not
    divide it."""
    count = 301
    x = data((count, 32), 41, True)
    lab = np.zeros(count, np.int32)
    lab[[5, 200]] = 1
    xd = cuda(x)
    split = split_of(xd, 2)
    assert split > 2, split
    got = ops.verify_label_nanmean(xd, lab, 2).cpu().numpy()
    same_bits_nan_exact(got, label_mean64(x, lab, 2).astype(np.float32))
    x = data((count, 108), 42, True)
    lab = labels_for(count, 64, 43)
    xd = cuda(x)
    split, len0 = split_of(xd, 64), int((lab == 0).sum())
    assert 1 < split < len0 and len0 % split != 0, (split, len0)
    same_bits_nan_exact(ops.verify_label_nanmean(xd, lab, 64).cpu().numpy(), label_mean64(x, lab, 64).astype(np.float32))
    # a long row on few labels still splits; the longest case of this file, 301 x 4096 floats
    x = data((count, 4096), 44, True)
    lab = labels_for(count, 2, 45)
    xd = cuda(x)
    assert split_of(xd, 2) > 1
    same_bits_nan_exact(ops.verify_label_nanmean(xd, lab, 2).cpu().numpy(), label_mean64(x, lab, 2).astype(np.float32))


def test_label_nanmean_follows_ieee_on_nan_and_infinities():
    inf = np.inf
    x = np.array([[inf, inf, -inf, 1.0, np.nan, 4.0, 2.0, 8.0],
                  [1.0, 1.0, 1.0, np.nan, np.nan, 4.0, 2.0, 8.0],
                  [-inf, inf, 2.0, 3.0, np.nan, 5.0, -inf, 8.0]], np.float32)
    got = ops.verify_label_nanmean(cuda(x), np.array([0, 0, 0], np.int32), 1).cpu().numpy()[0]
    assert np.isnan(got[0]) and got[1] == inf and got[2] == -inf and got[3] == 2.0 and np.isnan(got[4]) and got[7] == 8.0
    two = ops.verify_label_nanmean(cuda(x), np.array([1, 0, 1], np.int32), 2).cpu().numpy()
    assert np.isnan(two[1, 0]) and two[0, 0] == 1.0 and two[1, 6] == -inf and two[0, 6] == 2.0 and np.isnan(two[:, 4]).all()


@pytest.mark.parametrize('row', [(32,), (4, 8, 12)], ids=str)
def test_label_nanmean_offset_view_falls_back_to_scalar_loads(row):
    """one float into a larger buffer the 16-byte route is not allowed; the table keeps its bits on dyadic data"""
    x = data((37,) + row, 51, True)
    lab = labels_for(37, 12, 52)
    want = label_mean64(x, lab, 12).astype(np.float32)
    same_bits_nan_exact(ops.verify_label_nanmean(cuda(x, misalign=True), lab, 12).cpu().numpy(), want)
    same_bits_nan_exact(ops.verify_label_nanmean(cuda(x), lab, 12).cpu().numpy(), want)


# -- dlwp_verify_label_error_sums ------------------------------------------------------------------------------------------------------------ #
def close(got, want):
    assert got[2] == want[2] and got[2] == np.floor(got[2])                                 # counts are exact integers
    for k in (0, 1):
        if np.isfinite(want[k]) and want[k] != 0:
            assert abs(got[k] - want[k]) <= BOUND * abs(want[k]), (k, got[k], want[k])
        else:
            assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k]))


@pytest.mark.parametrize('m', [1, 129])
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('row', ROWS, ids=str)
def test_label_error_sums_and_anomaly(row, count, m):
    rng = np.random.default_rng(7 * count + m)
    x = data((count,) + row, 61 + count, False)
    for n_labels in LABELS:
        lab = labels_for(count, n_labels, 62 + n_labels)
        xd = cuda(x)
        table = ops.verify_label_nanmean(xd, lab, n_labels)
        rows = np.sort(rng.integers(0, count, m))[::-1].copy()                              # descending, with repeats once m > count
        if m > 1:
            rows[1] = rows[0]
        tab = table.cpu().numpy()                                                           # the device's own table
        with np.errstate(invalid='ignore'):
            d = x[rows] - tab[lab[rows]]
        want = error_sums64(d)
        sums, an = ops.verify_label_error_sums(xd, rows, lab[rows], table, anomaly=True)
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (3,) and tuple(an.shape) == (m,) + row
        close(sums.cpu().numpy(), want)
        same_bits_nan_exact(an.cpu().numpy(), d)
        bare = ops.verify_label_error_sums(xd, rows, lab[rows], table)                      # a null anomaly: the same sums bit for bit
        assert torch.equal(bare.view(torch.int64), sums.view(torch.int64))
        assert torch.equal(ops.verify_label_error_sums(xd, rows, lab[rows], table).view(torch.int64), bare.view(torch.int64))
        off = ops.verify_label_error_sums(cuda(x, misalign=True), rows, lab[rows], cuda(tab, misalign=True))
        close(off.cpu().numpy(), want)
        close(off.cpu().numpy(), sums.cpu().numpy())


def test_label_error_sums_many_blocks_and_infinities():
    """129 rows of 4096 floats: more 256-thread slices than one block; an infinity on either side follows IEEE"""
    x = data((37, 4096), 71, False)
    lab = labels_for(37, 2, 72)
    rows = np.arange(129) % 37
    xd = cuda(x)
    table = ops.verify_label_nanmean(xd, lab, 2)
    tab = table.cpu().numpy()
    with np.errstate(invalid='ignore'):
        d = x[rows] - tab[lab[rows]]
    sums, an = ops.verify_label_error_sums(xd, rows, lab[rows], table, anomaly=True)
    close(sums.cpu().numpy(), error_sums64(d))
    same_bits_nan_exact(an.cpu().numpy(), d)
    x[3, 9], tab[lab[4], 10] = np.inf, np.inf
    x[4, 10] = np.inf                                      # inf - inf: skipped
    with np.errstate(invalid='ignore'):
        d = x[rows] - tab[lab[rows]]
    got = ops.verify_label_error_sums(cuda(x), rows, lab[rows], cuda(tab)).cpu().numpy()
    want = error_sums64(d)
    assert np.isinf(got[0]) and np.isinf(got[1]) and got[2] == want[2]


# -- dlwp_gather_rows_fill ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('misalign', [False, True], ids=['aligned', 'offset_view'])
@pytest.mark.parametrize('n', [0, 1, 300])
@pytest.mark.parametrize('row', [1, 45, 64])
def test_gather_rows_fill(row, n, misalign):
    rng = np.random.default_rng(row + n)
    src = rng.standard_normal((23, row)).astype(np.float32)
    v = src.view(np.uint32)
    v[2, 0], v[5, row - 1], v[7, row // 2] = 0x7fc12345, 0xffc00001, 0x7f800001             # NaNs with payloads, one signalling
    rows = rng.integers(0, 23, n).astype(np.int64)
    if n == 1:
        variants = [rows, np.array([-1], np.int64)]
    elif n:
        rows[[0, n // 2, n - 1]] = -1                      # absent rows at the first, a middle and the last position
        rows[[3, 4, 5]] = 2                                # repeats, of the row with a payload
        rows[10] = 22
        variants = [rows, rows.reshape(3, 100)]
    else:
        variants = [rows]
    for r in variants:
        got = ops.gather_rows_fill(cuda(src, misalign), r)
        assert tuple(got.shape) == tuple(r.shape) + (row,) and got.dtype == torch.float32
        want = verify.take_rows_fill_host(src, r)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))      # bits, payloads included
        if r.size:
            assert np.isnan(got.cpu().numpy()[r < 0]).all() and (got.cpu().numpy().view(np.uint32)[r < 0] == 0x7fc00000).all()


def test_gather_rows_fill_many_blocks():
    """56 x 40 windows of rows of 1 x 88 x 180 floats: 142 MB, a full grid with several turns per thread"""
    src = np.random.default_rng(5).standard_normal((50, 88 * 180)).astype(np.float32)
    rows = (np.arange(56)[:, None] + np.arange(40)[None, :]).astype(np.int64)
    rows[rows >= 50] = -1
    got = ops.gather_rows_fill(cuda(src), rows).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), verify.take_rows_fill_host(src, rows).view(np.uint32))


def test_gather_rows_fill_refuses_an_index_past_the_source_without_a_launch():
    src = cuda(np.zeros((4, 8), np.float32))
    with pytest.raises(ValueError, match='row index 4, the source has 4 rows'):
        ops.gather_rows_fill(src, np.array([0, 4], np.int64))
    with pytest.raises(ValueError, match='integers'):
        ops.gather_rows_fill(src, np.array([0.0]))


# -- the functions, end to end ----------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('dyadic', [False, True], ids=['gaussian', 'dyadic'])
def test_monthly_climo_error_device_against_host(dyadic):
    times, x = climo_record(dyadic=dyadic)
    da = LabeledArray(x, {'sample': times}, ('sample', 'varlev', 'lat', 'lon'))
    val_rows = np.arange(1, 40, 3)
    months = month_of(times)
    host_table = verify.label_nanmean_host(x, months, 12)
    dev_table = ops.verify_label_nanmean(cuda(x), months, 12).cpu().numpy()
    same_table = bits(host_table) == bits(dev_table)
    if dyadic:
        assert same_table.all()
    for method in METHODS:
        host, host_an = verify.monthly_climo_error(da, times[val_rows], method=method, return_da=True)
        want, _ = monthly64(x, times, val_rows, method)
        for arg, kw in ((da, dict(device='cuda')), (LabeledArray(cuda(x), da.coords, da.dims), {})):
            got, an = verify.monthly_climo_error(arg, times[val_rows], method=method, return_da=True, **kw)
            print('monthly_climo_error %s %s: device / host - 1 = %.3g' % ('dyadic' if dyadic else 'gaussian', method, got / host - 1))
            assert isinstance(got, float) and abs(got - host) <= BOUND * abs(host) and abs(got - want) <= BOUND * abs(want)
            values = an.values.cpu().numpy() if isinstance(an.values, torch.Tensor) else an.values
            assert isinstance(an.values, torch.Tensor) == (not kw) and an.dims == da.dims
            assert np.array_equal(an.coords['sample'], times[val_rows])
            same = same_table[months[val_rows]]
            assert np.array_equal(bits(values)[same], bits(host_an.values)[same])
            assert np.array_equal(np.isnan(values), np.isnan(host_an.values))
        many = verify.monthly_climo_error(da, times[val_rows], n_fhour=3, method=method, device='cuda')
        assert many.shape == (3,) and (many == got).all()
    with pytest.raises(KeyError):
        verify.monthly_climo_error(da, [np.datetime64('1999-01-01T00')], device='cuda')


def test_verification_from_series_device_bit_equal_to_host():
    times, values, full, all_times = gap_record()
    coords = {'sample': times, 'lat': np.arange(3.)}
    ds = SeriesDataset(values, coords, ('sample', 'varlev', 'lat', 'lon'))
    host = verify.verification_from_series(ds, forecast_steps=5, dt=6)
    dev = verify.verification_from_series(ds, forecast_steps=5, dt=6, device='cuda')
    assert isinstance(dev.values, np.ndarray) and dev.dims == host.dims and np.isnan(host.values).any()
    assert np.array_equal(bits(dev.values), bits(host.values))
    assert np.array_equal(dev.coords['f_hour'], host.coords['f_hour']) and np.array_equal(dev.coords['time'], host.coords['time'])
    sub = SeriesDataset(values[4:9], {'sample': times[4:9]}, ('sample', 'varlev', 'lat', 'lon'))
    h = verify.verification_from_series(sub, all_ds=ds, forecast_steps=3).values
    t = verify.verification_tensor(sub, all_ds=ds, forecast_steps=3)
    assert t.is_cuda and t.dtype == torch.float32 and np.array_equal(bits(t.cpu().numpy()), bits(h))


def test_verification_tensor_scores_a_device_rollout_without_a_host_array():
    """2 members, 3 leads, a 1 x 8 x 12 state: predict_timeseries(..., return_device=True) against verification_tensor, both in HBM;
    the same numbers as the float64 restatement on the all-host arrays, inside the bound of tests/test_gpu_verify.py"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    d.build_model(cnn2_layers((1, 8, 12)), loss='mse', optimizer='adam')
    rng = np.random.default_rng(17)
    record = rng.standard_normal((4, 1, 8, 12)).astype(np.float32)
    times = np.datetime64('2005-03-01T00') + np.arange(4) * np.timedelta64(6, 'h')
    dims = ('sample', 'varlev', 'lat', 'lon')
    all_ds = SeriesDataset(record, {'sample': times}, dims)
    ds = SeriesDataset(record[:2], {'sample': times[:2]}, dims)
    series = d.predict_timeseries(record[:2], 3, return_device=True)
    assert series.is_cuda and tuple(series.shape) == (3, 2, 1, 8, 12)
    vt = verify.verification_tensor(ds, all_ds=all_ds, forecast_steps=3, dt=6)
    assert vt.is_cuda and tuple(vt.shape) == (3, 2, 1, 8, 12)
    host_valid = verify.verification_from_series(ds, all_ds=all_ds, forecast_steps=3, dt=6).values
    assert np.array_equal(bits(vt.cpu().numpy()), bits(host_valid)) and np.isnan(host_valid[2, 1]).all()     # 2005-03-02T00 is past the record
    host_series = series.cpu().numpy()
    with np.errstate(invalid='ignore'):
        diff = host_valid.astype(np.float64) - host_series.astype(np.float64)
    for method in METHODS:
        got = verify.forecast_error(series, vt, method=method)
        host = np.asarray(verify.forecast_error(host_series, host_valid, method=method))
        assert got.dtype == np.float32 and got.shape == (3,)
        for f in range(3):
            v = np.nanmean(np.abs(diff[f])) if method == 'mae' else np.nanmean(diff[f] ** 2)
            v = np.sqrt(v) if method == 'rmse' else v
            assert abs(float(got[f]) - v) <= BOUND * v, (method, f, got[f], v)
            assert abs(float(host[f]) - v) <= 4 * BOUND * v              # the host path's float32 mean over 96 or 192 numbers


# -- argument refusals, without a launch --------------------------------------------------------------------------------------------------- #
def _refused(rc, text):
    assert rc == _lib.EINVAL, rc
    assert text in _lib.lib.dlwp_last_error().decode(), _lib.lib.dlwp_last_error()


def test_label_nanmean_refusals():
    off = (ctypes.c_int * 3)(0, 2, 5)
    index = FAKE

    def call(h=NULL, x=FAKE, count=5, row=8, offsets=off, index=index, n_labels=2, mean=FAKE, ws=FAKE, ws_bytes=1 << 20):
        return _lib.lib.dlwp_verify_label_nanmean(h, x, count, LL(row), offsets, index, n_labels, mean, ws, ws_bytes, NULL)
    _refused(call(count=0), 'must be >= 1')
    _refused(call(row=0), 'must be >= 1')
    _refused(call(n_labels=65), 'n_labels 65')
    _refused(call(n_labels=0), 'n_labels 0')
    for kw in (dict(x=NULL), dict(index=NULL), dict(mean=NULL), dict(ws=NULL), dict(offsets=None)):
        _refused(call(**kw), 'null pointer')
    _refused(call(offsets=(ctypes.c_int * 3)(0, 2, 4)), 'offsets must run from 0 to count')
    _refused(call(offsets=(ctypes.c_int * 3)(0, 6, 5)), 'offsets decrease')
    # 256 CUs without a handle: 2 labels x 1 tile -> 1024 chunks allowed, 5 samples -> split 5; 2 * 5 * 8 * 12 bytes
    assert _lib.lib.dlwp_verify_label_nanmean_workspace(NULL, 5, LL(8), 2) == 960
    assert _lib.lib.dlwp_verify_label_nanmean_workspace(NULL, 5, LL(8), 65) == 0
    _refused(call(ws_bytes=959), 'workspace too small (959 < 960)')
    _refused(call(ws_bytes=960), 'null handle')
    x = cuda(np.zeros((5, 8), np.float32))
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 2\)'):
        ops.verify_label_nanmean(x, np.array([0, 1, 2, 0, 0]), 2)
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 2\)'):
        ops.verify_label_nanmean(x, np.array([0, 1, -1, 0, 0]), 2)
    with pytest.raises(ValueError, match='n_labels 65'):
        ops.verify_label_nanmean(x, np.zeros(5, np.int32), 65)
    with pytest.raises(ValueError, match='4 labels for 5 samples'):
        ops.verify_label_nanmean(x, np.zeros(4, np.int32), 2)
    with pytest.raises(_lib.DlwpError, match='workspace too small'):
        ops.verify_label_nanmean(x, np.zeros(5, np.int32), 2, ws=torch.empty(64, dtype=torch.uint8, device='cuda'))


def test_label_error_sums_refusals():
    def call(h=NULL, x=FAKE, count_x=5, row=8, rows=FAKE, labels=FAKE, m=3, table=FAKE, n_labels=2, anomaly=NULL, sums=FAKE, ws=FAKE,
             ws_bytes=1 << 20):
        return _lib.lib.dlwp_verify_label_error_sums(h, x, count_x, LL(row), rows, labels, m, table, n_labels, anomaly, sums, ws, ws_bytes,
                                                     NULL)
    for kw in (dict(count_x=0), dict(m=0), dict(row=0)):
        _refused(call(**kw), 'must all be >= 1')
    _refused(call(n_labels=65), 'n_labels 65')
    for kw in (dict(x=NULL), dict(rows=NULL), dict(labels=NULL), dict(table=NULL), dict(sums=NULL), dict(ws=NULL)):
        _refused(call(**kw), 'null pointer')
    _refused(call(ws_bytes=23), 'workspace too small (23 < 24)')         # 3 rows of 2 quads: one block
    _refused(call(ws_bytes=24), 'null handle')
    x, table = cuda(np.zeros((5, 8), np.float32)), cuda(np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 2\)'):
        ops.verify_label_error_sums(x, np.array([0, 1]), np.array([0, 2]), table)
    with pytest.raises(ValueError, match=r'rows must lie in \[0, 5\)'):
        ops.verify_label_error_sums(x, np.array([0, 5]), np.array([0, 1]), table)
    with pytest.raises(ValueError, match='at most 64'):
        ops.verify_label_error_sums(x, np.array([0]), np.array([0]), cuda(np.zeros((65, 8), np.float32)))
    with pytest.raises(_lib.DlwpError, match='workspace too small'):
        ops.verify_label_error_sums(x, np.array([0]), np.array([0]), table, ws=torch.empty(8, dtype=torch.uint8, device='cuda'))


def test_gather_rows_fill_refusals():
    def call(h=NULL, src=FAKE, src_rows=4, row=8, rows=FAKE, n=3, dst=FAKE):
        return _lib.lib.dlwp_gather_rows_fill(h, src, LL(src_rows), LL(row), rows, LL(n), dst, NULL)
    _refused(call(src_rows=0), 'must be >= 1')
    _refused(call(row=0), 'must be >= 1')
    _refused(call(n=-1), 'must be >= 1')
    for kw in (dict(src=NULL), dict(rows=NULL), dict(dst=NULL)):
        _refused(call(**kw), 'null pointer')
    _refused(call(), 'null handle')
    assert call(n=0, src=NULL, rows=NULL, dst=NULL) == _lib.OK            # nothing to do
