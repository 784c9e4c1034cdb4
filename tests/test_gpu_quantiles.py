"""dlwp_verify_label_quantiles (csrc/quantile.hip) on the device against dlwp_amd.model.verify.label_quantiles_host, which
tests/test_quantiles_cpu.py pins to a column-by-column restatement and to numpy.nanquantile.

The bound is equality of bits, NaNs included (every NaN of the definition is 0x7fc00000): selection counts integers, the order
statistics are samples with their bits, and the interpolation of 'linear' is three float64 operations rounded one by one on both sides
and one rounding to float32.  Both routes (LDS and streaming) are held to it on every case.  The list lengths that land on each tile
width, on the last length the LDS route holds and on the first it does not come from dlwp_verify_label_quantiles_plan."""
import ctypes

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, ops
from dlwp_amd.model import ensemble, verify
from dlwp_amd.model.generators import LabeledArray
from tests.quantile_cases import KINDS, METHODS, Q_SETS, QNAN, bits, labels_for, make_data, same_bits

pytestmark = pytest.mark.gpu

LL = ctypes.c_longlong
FAKE = ctypes.c_void_p(4096)         # a non-null, 16-byte aligned address for refusals that come before any launch; never dereferenced
NULL = ctypes.c_void_p(0)
# 108 = 4 x 27 and 32 take 16-byte loads (108: a ragged last tile at every width), 4 x 8 x 12 = 384 has an inner shape and fills whole
# tiles; 107 is no multiple of 4 and takes scalar loads, as every offset view does
ROWS = [(108,), (107,), (32,), (4, 8, 12)]
COUNTS = [1, 2, 37, 301]
LABELS = [1, 2, 12, 64]
COMBOS = [(k, m) for k in (1, 3, 8) for m in METHODS]


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


def check(xd, x, lab, n_labels, qs, method, routes):
    want, n_want = verify.label_quantiles_host(x, lab, n_labels, qs, method, return_count=True)
    for route in routes:
        got, n = ops.verify_label_quantiles(xd, lab, n_labels, qs, method, route=route, want_count=True)
        assert got.shape == (len(qs), n_labels) + x.shape[1:] and got.dtype == torch.float32 and n.dtype == torch.int32
        same_bits(got.cpu().numpy(), want)
        same_bits(n.cpu().numpy(), n_want)
    return want


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('row', ROWS)
def test_quantiles_have_the_hosts_bits(row, count):
    """every K and method on every row shape and count, planner's route and streaming; the label counts and the kinds of data (Gaussian,
    ties, zeros of both signs with subnormals, infinities -- all with NaNs of both signs and payloads, an all-NaN column, a constant
    column) rotate through the combinations"""
    turn = ROWS.index(row) + COUNTS.index(count)
    data = {kind: make_data((count,) + row, kind, 100 + 7 * turn + i) for i, kind in enumerate(KINDS)}
    dev = {kind: cuda(x) for kind, x in data.items()}
    for i, n_labels in enumerate(LABELS):
        lab = labels_for(count, n_labels, 3 * count + n_labels)
        for j, (k, method) in enumerate(COMBOS):
            kind = KINDS[(turn + i + j) % len(KINDS)]
            check(dev[kind], data[kind], lab, n_labels, Q_SETS[k], method, (0, 2))


@pytest.mark.parametrize('kind', KINDS)
def test_every_kind_of_data_with_every_method(kind):
    x = make_data((301, 108), kind, 5)
    xd = cuda(x)
    lab = labels_for(301, 12, 9)
    for method in METHODS:
        want = check(xd, x, lab, 12, Q_SETS[8], method, (1, 2))
        assert np.all(bits(want[:, :, 0]) == QNAN)                       # the all-NaN column
        assert np.all(want[:, :11, 1] == np.float32(-2.5))               # the constant column


@pytest.mark.parametrize('row', [(108,), (32,)])
def test_offset_view_takes_scalar_loads(row):
    x = make_data((37,) + row, 'gauss', 41)
    lab = labels_for(37, 12, 42)
    for k, method in ((3, 'linear'), (8, 'lower')):
        want = check(cuda(x, misalign=True), x, lab, 12, Q_SETS[k], method, (1, 2))
        same_bits(ops.verify_label_quantiles(cuda(x), lab, 12, Q_SETS[k], method).cpu().numpy(), want)


def planner_lengths():
    """from the planner alone: per tile width the longest list it takes, and the first list the LDS route does not hold"""
    last = {}
    for max_len in range(1, 1 << 13):
        route, cols = ops.verify_label_quantiles_plan(max_len, 108)
        if route == 2:
            return last, max_len
        last[cols] = max_len
    raise AssertionError('the planner never leaves the LDS route')


def test_list_lengths_at_every_planner_boundary():
    """the longest list of each tile width (the widest first), the last one the LDS route holds and the first it does not: label 0 has
    exactly that many rows, label 1 seven, in shuffled order; every case on the planner's route, forced through streaming, and forced
    through LDS where that fits"""
    last, first_stream = planner_lengths()
    assert len(last) >= 2 and sorted(last.values()) == [last[c] for c in sorted(last, reverse=True)]
    lengths = sorted(set(list(last.values()) + [v + 1 for v in last.values()] + [first_stream]))
    assert first_stream == max(last.values()) + 1 and lengths[-1] == first_stream and lengths[-1] <= 4096
    for i, length in enumerate(lengths):
        rng = np.random.default_rng(length)
        lab = np.zeros(length + 7, np.int32)
        lab[:7] = 1
        lab = lab[rng.permutation(lab.size)]
        x = make_data((length + 7, 108), ('gauss', 'ties')[i % 2], 50 + i)
        xd = cuda(x)
        fits = length < first_stream
        assert ops.verify_label_quantiles_plan(length, 108)[0] == (1 if fits else 2)
        check(xd, x, lab, 2, Q_SETS[3], 'linear', (0, 1, 2) if fits else (0, 2))
        check(xd, x, lab, 2, Q_SETS[8], 'nearest', (0, 2))
        if not fits:
            with pytest.raises(_lib.DlwpError, match='LDS route holds at most'):
                ops.verify_label_quantiles(xd, lab, 2, 0.5, route=1)


def test_both_routes_give_identical_bits():
    x = make_data((301, 4, 8, 12), 'ties', 77)
    xd = cuda(x)
    lab = labels_for(301, 12, 78)
    for k, method in ((8, 'linear'), (3, 'higher')):
        a, na = ops.verify_label_quantiles(xd, lab, 12, Q_SETS[k], method, route=1, want_count=True)
        b, nb = ops.verify_label_quantiles(xd, lab, 12, Q_SETS[k], method, route=2, want_count=True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(na, nb)
        again = ops.verify_label_quantiles(xd, lab, 12, Q_SETS[k], method, route=1)
        assert torch.equal(a.view(torch.int32), again.view(torch.int32))


def _refused(rc, text):
    assert rc == _lib.EINVAL, rc
    assert text in _lib.lib.dlwp_last_error().decode(), _lib.lib.dlwp_last_error()


def test_c_refusals_arrive_in_the_documented_order():
    off = (ctypes.c_int * 3)(0, 2, 5)
    qs = (ctypes.c_double * 2)(0.25, 0.5)

    def call(h=NULL, x=FAKE, count=5, row=8, offsets=off, index=FAKE, n_labels=2, q=qs, k=2, method=0, route=0, out=FAKE, counts=NULL,
             ws=FAKE, ws_bytes=1 << 20):
        return _lib.lib.dlwp_verify_label_quantiles(h, x, count, LL(row), offsets, index, n_labels, q, k, method, route, out, counts, ws,
                                                    ws_bytes, NULL)
    # each call breaks one rule and every rule behind it in the order: the first one is reported
    bad_q = (ctypes.c_double * 2)(0.25, 1.5)
    bad_off = (ctypes.c_int * 3)(0, 6, 5)
    later = dict(ws_bytes=0)
    _refused(call(count=0, n_labels=0, **later), 'must be >= 1')
    _refused(call(row=0, n_labels=0, **later), 'must be >= 1')
    _refused(call(n_labels=65, k=0, **later), 'n_labels 65')
    _refused(call(n_labels=0, k=0, **later), 'n_labels 0')
    _refused(call(k=0, q=bad_q, **later), 'k 0')
    _refused(call(k=9, q=bad_q, **later), 'k 9')
    _refused(call(q=None, method=7, **later), 'null pointer (q)')
    _refused(call(q=bad_q, method=7, **later), 'q[1] = 1.5')
    _refused(call(q=(ctypes.c_double * 2)(float('nan'), 0.5), method=7, **later), 'q[0]')
    _refused(call(q=(ctypes.c_double * 2)(-1e-9, 0.5), method=7, **later), 'q[0]')
    _refused(call(method=4, route=3, **later), 'unknown method 4')
    _refused(call(method=-1, route=3, **later), 'unknown method -1')
    _refused(call(route=3, x=NULL, **later), 'route 3')
    for kw in (dict(x=NULL), dict(index=NULL), dict(out=NULL), dict(ws=NULL), dict(offsets=None)):
        _refused(call(**kw, **later), 'null pointer')
    _refused(call(offsets=(ctypes.c_int * 3)(0, 2, 4), **later), 'offsets must run from 0 to count')
    _refused(call(offsets=bad_off, **later), 'offsets decrease')
    _refused(call(row=(1 << 31) * 16, n_labels=1, offsets=(ctypes.c_int * 2)(0, 5), **later), 'too long')
    long_off = (ctypes.c_int * 3)(0, 2, 5000)
    _refused(call(count=5000, offsets=long_off, route=1, **later), 'LDS route holds at most')
    need = _lib.lib.dlwp_verify_label_quantiles_workspace(NULL, 5, LL(8), 2, 2)
    assert need == 64
    _refused(call(ws_bytes=63), 'workspace too small (63 < 64)')
    _refused(call(ws=ctypes.c_void_p(4104), ws_bytes=64), '16-byte aligned')
    _refused(call(ws_bytes=64), 'null handle')
    _refused(call(count=5000, offsets=long_off, route=2), 'null handle')             # streaming has no limit on the list
    x = cuda(np.zeros((5, 8), np.float32))
    with pytest.raises(_lib.DlwpError, match='workspace too small'):
        ops.verify_label_quantiles(x, np.zeros(5, np.int32), 2, 0.5, ws=torch.empty(16, dtype=torch.uint8, device='cuda'))


def test_index_outside_the_record_is_skipped():
    """the C entry point with a list that names rows beyond the record and a negative one: skipped, never read, not counted"""
    x = make_data((7, 32), 'gauss', 8, nan_share=0.0)
    xd = cuda(x)
    index = np.array([3, 40, 0, -1, 6, 7, 5], np.int32)
    off = (ctypes.c_int * 2)(0, index.size)
    index_d = torch.from_numpy(index).cuda()
    qs = (ctypes.c_double * 3)(*Q_SETS[3])
    h = _lib.handle(0)
    want, n_want = verify.label_quantiles_host(x[[3, 0, 6, 5]], np.zeros(4, np.int32), 1, Q_SETS[3], 'linear', return_count=True)
    for route in (1, 2):
        out = torch.empty((3, 1, 32), dtype=torch.float32, device='cuda')
        n = torch.empty((1, 32), dtype=torch.int32, device='cuda')
        ws = torch.empty(256, dtype=torch.uint8, device='cuda')
        _lib.check(_lib.lib.dlwp_verify_label_quantiles(h, ctypes.c_void_p(xd.data_ptr()), 7, LL(32), off,
                                                        ctypes.c_void_p(index_d.data_ptr()), 1, qs, 3, 0, route,
                                                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(n.data_ptr()),
                                                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), NULL))
        torch.cuda.synchronize()
        same_bits(out.cpu().numpy(), want)
        same_bits(n.cpu().numpy(), n_want)


def test_climatological_quantiles_on_the_device_and_as_event_thresholds():
    """a tiny ensemble scored against the terciles of a record that lives on the device: climatological_quantiles returns a CUDA tensor
    with the host's bits, and event_scores takes it as it stands and returns what it returns for the host-made thresholds"""
    rng = np.random.default_rng(21)
    field = (2, 6, 8)
    times = np.datetime64('2002-01-01T00') + np.arange(200) * np.timedelta64(6, 'h')
    record = (rng.standard_normal((200,) + field) * 2.0).astype(np.float32)
    record[rng.random(record.shape) < 0.03] = np.nan
    dims = ('sample', 'varlev', 'lat', 'lon')
    on_host = LabeledArray(record, {'sample': times}, dims)
    on_device = LabeledArray(torch.from_numpy(record).cuda(), {'sample': times}, dims)
    terciles = [1.0 / 3.0, 2.0 / 3.0]
    host = verify.climatological_quantiles(on_host, terciles, labels=None)
    dev = verify.climatological_quantiles(on_device, terciles, labels=None)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and tuple(dev.shape) == (2, 1) + field
    same_bits(dev.cpu().numpy(), host)
    uploaded, n = verify.climatological_quantiles(on_host, terciles, labels=None, return_count=True, device='cuda')
    assert isinstance(uploaded, np.ndarray) and n.dtype == np.int32
    same_bits(uploaded, host)
    monthly = verify.climatological_quantiles(on_device, 0.95, method='higher')
    same_bits(monthly.cpu().numpy(), verify.climatological_quantiles(on_host, 0.95, method='higher'))
    t_n, s_n, m = 2, 3, 5
    forecast = (rng.standard_normal((t_n, s_n, m) + field) * 2.0).astype(np.float32)
    valid = (rng.standard_normal((t_n, s_n) + field) * 2.0).astype(np.float32)
    fd, vd = torch.from_numpy(forecast).cuda(), torch.from_numpy(valid).cuda()
    a = ensemble.event_scores(fd, vd, dev[:, 0])
    b = ensemble.event_scores(fd, vd, host[:, 0])
    for name, u, v in zip(a._fields, a, b):
        if u is None and v is None:
            continue
        u, v = np.asarray(u), np.asarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape, name
        assert u.tobytes() == v.tobytes(), name
