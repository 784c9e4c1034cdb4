"""The HBM-resident series feed on the device: dlwp_series_window_gather (csrc/series.hip) against its numpy restatement
ops.series_window_gather_host, bit for bit; DeviceLoader's 'resident' mode against SeriesDataGenerator.__getitem__ on the golden
cases of the reference's generator (tests/golden/series.npz; DLWP/model/generators.py:323-629); fit_generator and
evaluate_generator with the device feed against the host feed (DLWP_SERIES_HOST=1, the path every batch took before).

Everything here is a copy, so every comparison is bit equality -- except training, which carries the tolerance of
tests/test_gpu_train_steps.py for fit_generator against train_on_batch (2e-7 per step on the weights, 1e-5 relative on losses)."""
import os
import threading

import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import DLWPNeuralNet, SeriesDataGenerator, SeriesDataset
from dlwp_amd.model.generators import DeviceLoader, WindowPlan
from dlwp_amd.presets import unet_layers
from tests.test_gpu_model import _build, _weights_of

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'series.npz'))
DATES = G['dates'].astype('datetime64[s]')
QNAN = 0x7fc00000
GUARD = 0x5a5a5a5a

CASES = {
    'a': dict(rec=False, kw=dict(input_time_steps=2, output_time_steps=2, batch_size=4)),
    'b': dict(rec=True, kw=dict(input_time_steps=2, output_time_steps=2, batch_size=4)),
    'c': dict(rec=False, kw=dict(input_sel={'variable': ['z']}, output_sel={'variable': ['t'], 'level': [850]},
                                 input_time_steps=3, output_time_steps=1, interval=2, batch_size=5)),
    'd': dict(rec=False, kw=dict(input_time_steps=2, output_time_steps=2, add_insolation=True, batch_size=4)),
    'e': dict(rec=True, kw=dict(input_time_steps=2, output_time_steps=2, add_insolation=True, batch_size=4)),
    'f': dict(rec=False, kw=dict(input_time_steps=2, output_time_steps=2, sequence=3, batch_size=3)),
    'g': dict(rec=False, kw=dict(input_time_steps=1, output_time_steps=1, batch_size=6, shuffle=True)),
}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


@pytest.fixture(autouse=True)
def _device_feed(monkeypatch):
    monkeypatch.delenv('DLWP_SERIES_HOST', raising=False)


def _ds(series=None, lat=None, lon=None):
    s = G['S'] if series is None else series
    return SeriesDataset(s, {'sample': DATES[:s.shape[0]], 'variable': np.array(['z', 't']), 'level': np.array([500, 850]),
                             'lat': G['lat'] if lat is None else lat, 'lon': G['lon'] if lon is None else lon},
                         ('sample', 'variable', 'level', 'lat', 'lon'))


def _gen(tag, ds=None, model=None, **kw):
    case = CASES[tag]
    m = model or DLWPNeuralNet(is_convolutional=True, is_recurrent=case['rec'], time_dim=case['kw']['input_time_steps'],
                               scaler_type=None, scale_targets=False)
    np.random.seed(7)
    return SeriesDataGenerator(m, ds or _ds(), **dict(case['kw'], **kw))


def bits(a):
    if isinstance(a, torch.Tensor):
        torch.cuda.synchronize()
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _flat(batch):
    X, y = batch
    return [X] + (list(y) if isinstance(y, (list, tuple)) else [y])


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


def series(T, row, seed):
    """(T, row) floats with a NaN payload in every row, so a float move instead of a word move would show"""
    s = np.random.default_rng(seed).standard_normal((T, row)).astype(np.float32)
    s.view(np.uint32)[:, row // 2] = 0x7fc12345
    return s


def run(plan, samples, misalign=(), vec=None):
    """the kernel on `plan`, every destination between guard words; returns the destinations as host arrays after checking the
    guards and -- when `vec` is given -- the path the host picks"""
    srcs = [cuda(a, misalign=(k in misalign)) for k, a in enumerate(plan.sources)]
    samples = np.asarray(samples, dtype=np.int64)
    n = samples.size
    stores, outs = [], []
    for r in plan.rows:                        # 4 guard floats in front (keeps the 16-byte alignment), 4 behind
        st = torch.full((4 + max(n, 1) * r + 4,), 0.0, dtype=torch.float32, device='cuda')
        st.view(torch.int32).fill_(GUARD)
        stores.append(st)
        outs.append(st[4:4 + max(n, 1) * r].view(max(n, 1), r))
    if vec is not None:
        assert ops.SeriesTables(srcs, outs, plan.segments).vec == vec
    ops.series_window_gather(srcs, plan.segments, plan.shapes, samples, out=outs)
    got = []
    for st, r, shp in zip(stores, plan.rows, plan.shapes):
        b = bits(st)
        assert (b[:4] == GUARD).all() and (b[4 + n * r:] == GUARD).all()
        got.append(b[4:4 + n * r].view(np.float32).reshape((n,) + shp))
    return got


def check(plan, samples, **kw):
    want = ops.series_window_gather_host(plan, samples)
    got = run(plan, samples, **kw)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return got


def window(T, row, hw_ins, t_in, t_out, blocks, seed):
    """a hand-made plan of the generator's layout: t_in states (+ an insolation plane of hw_ins floats behind each when > 0), then
    `blocks` target blocks of t_out states"""
    from dlwp_amd.model.generators import merge_segments
    srcs = [series(T, row, seed)] + ([series(T, hw_ins, seed + 1)] if hw_ins else [])
    pieces = []
    for m in range(t_in):
        pieces.append((0, 0, m, 0, m * (row + hw_ins), row))
        if hw_ins:
            pieces.append((1, 0, m, 0, m * (row + hw_ins) + row, hw_ins))
    for k in range(blocks):
        pieces += [(0, 1 + k, t_in + t_out * k + m, 0, m * row, row) for m in range(t_out)]
    shapes = [(t_in * (row + hw_ins),)] + [(t_out * row,)] * blocks
    return WindowPlan(srcs, shapes, merge_segments(pieces, [s.shape[1] for s in srcs]), blocks > 1)


# -- the kernel against the restatement --------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('tag', sorted(CASES))
def test_kernel_on_the_golden_grid_takes_the_vector_path(tag):
    g = _gen(tag)                                                       # hw = 48
    check(g.window_plan(), np.arange(g._n_sample), vec=True)
    check(g.window_plan(), g._indices[:1], vec=True)                    # n = 1


def test_kernel_on_a_5_by_7_grid_takes_the_scalar_path():
    hw = 35
    check(window(20, 4 * hw, hw, 2, 2, 3, 1), np.arange(20 - 8 + 1), vec=False)
    check(window(20, 3 * hw, 0, 2, 2, 1, 2), [3], vec=False)              # three fields: 105 floats a state


def test_one_16_byte_unit_per_segment():
    # hw = 4, one-plane segments: channels 0 and 2 of the input, channel 1 of the target
    src = series(9, 16, 3)
    plan = WindowPlan([src], [(8,), (4,)], [[0, 0, 0, 0, 0, 4], [0, 0, 0, 8, 4, 4], [0, 1, 1, 4, 0, 4]])
    check(plan, np.arange(8), vec=True)


def test_a_source_offset_by_one_float_takes_the_scalar_path_and_stays_exact():
    g = _gen('d')
    for k in range(2):
        check(g.window_plan(), np.arange(g._n_sample), misalign=(k,), vec=False)


def test_a_non_contiguous_channel_selection_cannot_merge():
    hw = 48
    src = series(12, 4 * hw, 4)
    pieces = [[0, 0, m, c * hw, (2 * m + j) * hw, hw] for m in range(2) for j, c in enumerate((0, 2))]
    pieces += [[0, 1, 2, 3 * hw, 0, hw]]
    from dlwp_amd.model.generators import merge_segments
    segs = merge_segments(pieces, [4 * hw])
    assert len(segs) == 5
    check(WindowPlan([src], [(4 * hw,), (hw,)], segs), np.arange(10), vec=True)


def test_n_one_past_a_multiple_of_the_blocks_reach_and_the_last_time_exactly():
    # a block moves 1024 units a turn: segments of exactly 1024 and of 1025 units on both paths, n = 1 and n = 2 x reach + 1 samples
    for row, vec in ((4096, True), (4100, True), (1024, False), (1025, False)):
        T = 12
        plan = window(T, row, 0, 1, 1, 1, row)
        srcs_misaligned = () if vec else (0,)
        check(plan, [T - 2], misalign=srcs_misaligned, vec=vec)         # sample + shift == T - 1 exactly: the last state is read
        check(plan, np.arange(T - 1)[::-1], misalign=srcs_misaligned, vec=vec)
    cap = ops.series_grid_cap()
    plan = window(5, 8, 0, 1, 1, 1, 9)                                  # two chunks per sample: n = cap / 2 is one pass of the grid
    assert ops.series_chunks(plan.segments, True) == 2 and cap % 2 == 0
    rng = np.random.default_rng(10)
    for n in (cap // 2, cap // 2 + 1, cap + 1):
        check(plan, rng.integers(0, 4, n), vec=True)


def test_a_launch_larger_than_one_pass_of_the_capped_grid():
    """the train_functional.py batch: 64 samples of 2 x (2 variables + insolation) in, 6 blocks of 2 x 2 variables out, on 88 x 180"""
    hw = 88 * 180
    plan = window(64 + 13, 2 * hw, hw, 2, 2, 6, 11)
    n = 64
    turns = n * ops.series_chunks(plan.segments, True)
    assert turns > ops.series_grid_cap(), (turns, ops.series_grid_cap())          # the grid strides: more than one turn per block
    srcs = [cuda(a) for a in plan.sources]
    samples = np.random.default_rng(12).permutation(n)
    got = ops.series_window_gather(srcs, plan.segments, plan.shapes, samples)
    want = ops.series_window_gather_host(plan, samples)
    for a, b in zip(got, want):
        assert tuple(a.shape) == b.shape and np.array_equal(bits(a), bits(b))


def test_times_outside_the_series_are_quiet_nans_and_the_neighbours_exact():
    for hw, vec in ((48, True), (35, False)):
        T = 10
        plan = window(T, 2 * hw, hw, 2, 1, 2, hw)                       # states s, s + 1 in; s + 2 and s + 3 out
        samples = np.array([0, -1, 1, T - 3, T - 4, T - 2, 5, T, -7])
        got = check(plan, samples, vec=vec)
        X, y0, y1 = [bits(a) for a in got]
        # start -1: the first input step (its variables and its insolation plane) is missing, state 0 behind it and the targets are not
        assert (X[1, :3 * hw] == QNAN).all() and not (X[1, 3 * hw:] == QNAN).any() and not (y0[1] == QNAN).any()
        assert (y1[3] == QNAN).all() and not (X[3] == QNAN).any() and not (y0[3] == QNAN).any()      # sample + shift == T
        assert (y0[5] == QNAN).all() and (y1[5] == QNAN).all() and not (X[5] == QNAN).any()          # states T - 2, T - 1 | T, T + 1
        for i in (0, 2, 4, 6):                                           # the neighbours are whole (sample 4 ends on state T - 1)
            assert not (X[i] == QNAN).any() and not (y0[i] == QNAN).any() and not (y1[i] == QNAN).any()
        assert all((a[7] == QNAN).all() and (a[8] == QNAN).all() for a in (X, y0, y1))
    # a merged run is one unit: its second state missing blanks the run
    merged = window(6, 8, 0, 2, 1, 1, 5)
    assert len(merged.segments) == 2
    (X, y) = check(merged, [5, 3, 4, -1], vec=True)
    assert (bits(X[0]) == QNAN).all() and not (bits(X[1]) == QNAN).any() and (bits(X[3]) == QNAN).all()


def test_wrapper_refusals_and_the_empty_batch():
    src = cuda(series(6, 8, 1))
    segs = [[0, 0, 0, 0, 0, 8]]
    out = ops.series_window_gather([src], segs, [(8,)], np.zeros(0, np.int64))
    assert tuple(out[0].shape) == (0, 8)
    with pytest.raises(ValueError, match='integers'):
        ops.series_window_gather([src], segs, [(8,)], np.array([0.5]))
    with pytest.raises(ValueError, match='leaves its rows'):
        ops.series_window_gather([src], [[0, 0, 0, 4, 0, 16]], [(8,)], [0])
    with pytest.raises(ValueError, match='into destinations of 1 rows'):
        ops.series_window_gather([src], segs, [(8,)], [0, 1], out=[torch.empty((1, 8), device='cuda')])


# -- the loader ---------------------------------------------------------------------------------------------------------------------------- #
def _same_batch(got, want):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert tuple(a.shape) == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize('tag', sorted(CASES))
def test_loader_serves_two_epochs_from_the_resident_series(tag):
    g = _gen(tag)
    loader = DeviceLoader(g, torch.device('cuda'))
    orders = []
    for epoch in range(2):
        orders.append(g._indices.copy())
        seen = 0
        threads = threading.active_count()
        for i, (X, y, n_global) in enumerate(loader.iter_batches()):
            assert loader.mode == 'resident' and threading.active_count() == threads        # no worker thread in this mode
            want = g[i]
            _same_batch((X, y), want)
            assert isinstance(y, list) == isinstance(want[1], list) and n_global == want[0].shape[0]
            seen += n_global
        assert i == len(g) - 1 and seen == g._n_sample                  # the ragged last batch included
        g.on_epoch_end()
    if CASES[tag]['kw'].get('shuffle'):
        assert not np.array_equal(orders[0], orders[1])                 # the second epoch read re-uploaded indices
    assert tag == 'c' or g._n_sample % g.batch_size != 0                # (every case but c ends on a ragged batch)


def test_host_feed_switch_gives_the_same_values(monkeypatch):
    g = _gen('d')
    monkeypatch.setenv('DLWP_SERIES_HOST', '1')
    loader = DeviceLoader(g, torch.device('cuda'))
    for i, (X, y, _) in enumerate(loader.iter_batches()):
        assert loader.mode == 'generate'
        _same_batch((X, y), g[i])
    assert i == len(g) - 1


def test_two_shards_in_one_process_are_the_two_halves_of_the_batch():
    from dlwp_amd.parallel import shard_bounds
    g = _gen('f', batch_size=5)
    loaders = [DeviceLoader(g, torch.device('cuda'), shard=(r, 2)) for r in range(2)]
    its = [ld.iter_batches() for ld in loaders]
    for i in range(len(g)):
        want = _flat(g[i])
        n = want[0].shape[0]
        for r in range(2):
            X, y, n_global = next(its[r])
            lo, hi = shard_bounds(n, r, 2)
            assert loaders[r].mode == 'resident' and n_global == n and X.shape[0] == hi - lo
            _same_batch((X, y), (want[0][lo:hi], [t[lo:hi] for t in want[1:]]))
    for it in its:
        with pytest.raises(StopIteration):
            next(it)


def test_a_series_that_does_not_fit_leaves_the_resident_mode():
    g = _gen('a')
    loader = DeviceLoader(g, torch.device('cuda'))
    loader.resident_fraction = 0
    for i, (X, y, _) in enumerate(loader.iter_batches()):
        assert loader.mode == 'generate'
        _same_batch((X, y), g[i])
    assert i == len(g) - 1 and loader._resident['tables'] is None


# -- training and evaluation --------------------------------------------------------------------------------------------------------------- #
def _train(monkeypatch, host):
    """three epochs of case a's generator on the golden series tiled 2 x 2 (a 12 x 16 grid: two poolings) through a small U-Net"""
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if host:
        monkeypatch.setenv('DLWP_SERIES_HOST', '1')
    else:
        monkeypatch.delenv('DLWP_SERIES_HOST', raising=False)
    S = np.ascontiguousarray(np.tile(G['S'], (1, 1, 1, 2, 2)))
    ds = _ds(S, lat=np.linspace(-80, 80, 12), lon=np.arange(16) * 22.5)
    cs = (8, 12, 16)
    d = _build(unet_layers(cs, widths=(8, 16, 16, 16, 8)), time_dim=2, seed=9)
    _weights_of(d.model, np.random.default_rng(90))
    g = _gen('a', ds=ds, model=d)
    assert g.window_plan() is not None and tuple(g.convolution_shape) == cs
    hist = d.fit_generator(g, epochs=3, verbose=0)
    tr = d.model._trainer
    torch.cuda.synchronize()
    replayed = any(k[0] == g.batch_size and e.get('step') is not None for k, e in tr._graphs.items())
    val = tr.evaluate_generator(g)
    return dict(weights=d.model.get_weights(), loss=list(hist.history['loss']), form=tr._graph_ok(g.batch_size), replayed=replayed,
                val=val, steps=3 * len(g), iterations=d.model.optimizer.iterations)


def test_fit_generator_and_evaluate_generator_device_feed_against_host_feed(monkeypatch):
    dev = _train(monkeypatch, host=False)
    ref = _train(monkeypatch, host=True)
    assert dev['iterations'] == ref['iterations'] == dev['steps']
    # the step runs in the form it runs in with the host feed, and it was replayed: the untaped gather launches between the steps
    assert dev['form'] == ref['form'] == 'graph' and dev['replayed'] and ref['replayed']
    for a, b in zip(dev['weights'], ref['weights']):
        print('weights: max difference %.3g of %.3g' % (np.abs(a - b).max(), 2e-7 * dev['steps']))
        assert np.abs(a - b).max() <= 2e-7 * dev['steps']
    assert dev['loss'] == pytest.approx(ref['loss'], rel=1e-5)
    assert dev['val'] == pytest.approx(ref['val'], rel=1e-5)
