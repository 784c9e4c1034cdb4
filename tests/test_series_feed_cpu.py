"""Host side of the HBM-resident series feed: SeriesDataGenerator.window_plan (the segment table of what generate() copies),
its numpy executor ops.series_window_gather_host against generate() on the golden cases of the reference's generator
(tests/golden/series.npz; DLWP/model/generators.py:323-629), the cases without a plan, and every argument refusal of
dlwp_series_window_gather that needs no device.  (The helpers are this file's own copies of tests/test_series_generator.py's.)"""
import ctypes
import os

import numpy as np
import pytest

from dlwp_amd import _lib, ops
from dlwp_amd.model import DLWPNeuralNet, SeriesDataGenerator, SeriesDataset
from dlwp_amd.model.generators import WindowPlan, merge_segments

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'series.npz'))
DATES = G['dates'].astype('datetime64[s]')

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
HW = 48                             # the golden 6 x 8 grid
ROW = 4 * HW                        # two variables on two levels


def _ds(series=None):
    s = G['S'] if series is None else series
    return SeriesDataset(s, {'sample': DATES[:s.shape[0]], 'variable': np.array(['z', 't']), 'level': np.array([500, 850]),
                             'lat': G['lat'], 'lon': G['lon']}, ('sample', 'variable', 'level', 'lat', 'lon'))


def _model(tag, **kw):
    case = CASES[tag]
    args = dict(is_convolutional=True, is_recurrent=case['rec'], time_dim=case['kw']['input_time_steps'], scaler_type=None,
                scale_targets=False)
    args.update(kw)
    return DLWPNeuralNet(**args)


def _gen(tag, ds=None, model=None, cls=SeriesDataGenerator, **kw):
    np.random.seed(7)
    return cls(model or _model(tag), ds or _ds(), **dict(CASES[tag]['kw'], **kw))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _flat(batch):
    X, y = batch
    return [X] + (list(y) if isinstance(y, (list, tuple)) else [y])


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# -- the plan against generate() -------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('tag', sorted(CASES))
def test_the_restated_table_equals_generate_on_the_golden_cases(tag):
    g = _gen(tag)
    plan = g.window_plan()
    assert isinstance(plan, WindowPlan) and g.window_plan() is plan                      # cached: the same object
    assert plan.y_list == (CASES[tag]['kw'].get('sequence') is not None)
    assert all(s.ndim == 2 and s.dtype == np.float32 and s.shape[0] == 14 for s in plan.sources)
    bs = g.batch_size
    for b in (0, len(g) - 1):
        samples = g._indices[b * bs:(b + 1) * bs]
        got = ops.series_window_gather_host(plan, samples)
        _same(got, _flat(g[b]))
        assert np.array_equal(got[0], G['%s_X%d' % (tag, b)])                           # ... which is the reference's batch
        X, y = plan.as_batch(got)
        assert isinstance(y, list) == plan.y_list
    _same(ops.series_window_gather_host(plan, np.arange(g._n_sample)), _flat(g.generate([])))
    assert np.array_equal(ops.series_window_gather_host(plan, np.arange(g._n_sample))[0], G['%s_Xall' % tag])


def test_segment_counts_and_shifts():
    # a: no insolation, the whole state: X is one run of two states, y one run of two states two steps on; one shared source
    pa = _gen('a').window_plan()
    assert len(pa.sources) == 1 and pa.shapes == [(8, 6, 8), (8, 6, 8)]
    assert pa.segments.tolist() == [[0, 0, 0, 0, 0, 2 * ROW], [0, 1, 2, 0, 0, 2 * ROW]]
    # b: the recurrent shapes over the same memory
    pb = _gen('b').window_plan()
    assert pb.shapes == [(2, 4, 6, 8), (2, 4, 6, 8)] and np.array_equal(pb.segments, pa.segments)
    # d: insolation is one more plane behind each input step's channels: two segments per input step, from two sources
    pd = _gen('d').window_plan()
    assert len(pd.sources) == 2 and pd.sources[1].shape == (14, HW) and pd.shapes[0] == (10, 6, 8)
    assert pd.segments.tolist() == [[0, 0, 0, 0, 0, ROW], [1, 0, 0, 0, ROW, HW],
                                    [0, 0, 1, 0, ROW + HW, ROW], [1, 0, 1, 0, 2 * ROW + HW, HW],
                                    [0, 1, 2, 0, 0, 2 * ROW]]
    # c: z on both levels in, t850 out, three input steps, one output step, interval 2: the target is 3 + 2 - 1 steps on
    pc = _gen('c').window_plan()
    assert [s.shape for s in pc.sources] == [(14, 2 * HW), (14, HW)] and pc.shapes == [(6, 6, 8), (1, 6, 8)]
    assert pc.segments.tolist() == [[0, 0, 0, 0, 0, 6 * HW], [1, 1, 4, 0, 0, HW]]
    # f: three target blocks of two states each, one run per block
    pf = _gen('f').window_plan()
    assert pf.y_list and len(pf.shapes) == 4
    assert pf.segments.tolist() == [[0, 0, 0, 0, 0, 2 * ROW]] + [[0, 1 + k, 2 + 2 * k, 0, 0, 2 * ROW] for k in range(3)]
    # the train_functional.py shape: 2 x 2 input segments and six blocks
    gt = _gen('a', sequence=6, add_insolation=True, batch_size=2)
    assert gt._n_sample == 1                                            # 2 + 6 * 2 = 14 states: exactly the golden series
    pt = gt.window_plan()
    assert len(pt.segments) == 4 + 6 and pt.segments[-1].tolist() == [0, 6, 12, 0, 0, 2 * ROW]
    _same(ops.series_window_gather_host(pt, [0]), _flat(gt.generate([0])))


def test_merge_segments_joins_only_what_is_contiguous_on_both_sides():
    row = 12
    # two states in a row, then a gap in the destination, then a gap in the source, then another source
    pieces = [(0, 0, 0, 0, 0, row), (0, 0, 1, 0, row, row), (0, 0, 2, 0, 2 * row + 1, row), (0, 1, 0, 0, 0, 4), (0, 1, 0, 8, 4, 4),
              (1, 1, 0, 0, 8, 4), (1, 1, 0, 4, 12, 4)]
    assert merge_segments(pieces, [row, 8]).tolist() == [[0, 0, 0, 0, 0, 2 * row], [0, 0, 2, 0, 2 * row + 1, row], [0, 1, 0, 0, 0, 4],
                                                        [0, 1, 0, 8, 4, 4], [1, 1, 0, 0, 8, 8]]


def test_out_of_range_times_are_quiet_nans_and_payloads_survive():
    src = np.arange(5 * 8, dtype=np.float32).reshape(5, 8)
    src.view(np.uint32)[2, 3] = 0x7fc12345
    plan = WindowPlan([src], [(8,), (4,)], [[0, 0, 0, 0, 0, 8], [0, 1, 1, 2, 0, 4]])
    X, y = ops.series_window_gather_host(plan, [-1, 2, 4, 5, 1])
    assert (bits(X[0]) == 0x7fc00000).all() and np.array_equal(bits(y[0]), bits(src[0, 2:6]))
    assert bits(X[1])[3] == 0x7fc12345 and np.array_equal(bits(X[2]), bits(src[4]))
    assert (bits(y[2]) == 0x7fc00000).all() and (bits(X[3]) == 0x7fc00000).all() and bits(y[4])[1] == 0x7fc12345
    # a run over two times is one unit: the second time missing blanks all of it
    two = WindowPlan([src], [(16,)], [[0, 0, 0, 0, 0, 16]])
    (Z,) = ops.series_window_gather_host(two, [3, 4])
    assert np.array_equal(bits(Z[0]), bits(src[3:5].reshape(-1))) and (bits(Z[1]) == 0x7fc00000).all()


# -- no plan ------------------------------------------------------------------------------------------------------------------------------ #
def test_no_plan_when_generate_is_more_than_copies():
    s = G['S'].copy()
    s[5, 0, 0, 1, 1] = np.nan
    assert _gen('a', _ds(s)).window_plan() is None                      # samples may be dropped
    g = _gen('a', _ds(s), remove_nan=False)
    plan = g.window_plan()
    assert plan is not None
    got = ops.series_window_gather_host(plan, g._indices[4:8])          # ... and the NaN is copied like any other float
    _same(got, _flat(g[1]))
    assert np.isnan(got[0]).sum() == 2 and np.isnan(got[1]).sum() == 0   # state 5 is an input of samples 4 and 5 ...
    got = ops.series_window_gather_host(plan, g._indices[0:4])
    _same(got, _flat(g[0]))
    assert np.isnan(got[0]).sum() == 0 and np.isnan(got[1]).sum() == 2   # ... and a target of samples 2 and 3
    assert _gen('a', model=_model('a', scaler_type='StandardScaler')).window_plan() is None
    assert _gen('a', model=_model('a', impute_missing=True)).window_plan() is None
    assert _gen('a', _ds(G['S'].astype(np.float64))).window_plan() is None
    assert _gen('d', _ds(G['S'].astype(np.float64))).window_plan() is None

    class Augmented(SeriesDataGenerator):
        def generate(self, samples, scale_and_impute=True):
            X, y = SeriesDataGenerator.generate(self, samples, scale_and_impute)
            return X[:, :, ::-1], y

    assert _gen('a', cls=Augmented).window_plan() is None
    assert _gen('a').window_plan() is not None


def test_the_plan_follows_the_model_switches_it_was_made_from():
    g = _gen('a')
    assert g.window_plan() is not None
    g.model.scaler_type = 'StandardScaler'
    assert g.window_plan() is None
    g.model.scaler_type = None
    assert g.window_plan() is not None


# -- the entry point's refusals ---------------------------------------------------------------------------------------------------------- #
def test_new_exports_are_declared_and_bound():
    names = _lib.declared_symbols()
    for n in ('dlwp_series_window_gather', 'dlwp_series_gather_grid_cap'):
        assert n in names and getattr(_lib.lib, n).argtypes is not None, n
    assert ctypes.sizeof(_lib.SeriesSrc) == 24 and ctypes.sizeof(_lib.SeriesDst) == 16 and ctypes.sizeof(_lib.SeriesSeg) == 40
    code = open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'series.hip')).read()
    assert 'DLWP_UNTAPED(dlwp_series_window_gather)' in code
    assert _lib.lib.dlwp_series_gather_grid_cap(None) == 0


def test_entry_point_refusals_without_a_device():
    """every refusal of dlwp_series_window_gather comes before the launch and before the handle is looked at: with fake (never
    dereferenced) device addresses and a null handle the messages can be read on a machine without a GPU"""
    FAKE = 0x10000
    LL = ctypes.c_longlong

    def call(srcs=((FAKE, 10, 16),), dsts=((FAKE, 16),), segs=((0, 0, 0, 0, 0, 16),), samples=FAKE, n=4, n_src=None, n_dst=None,
             n_seg=None, null=()):
        s = (_lib.SeriesSrc * max(len(srcs), 1))(*[_lib.SeriesSrc(*v) for v in srcs])
        d = (_lib.SeriesDst * max(len(dsts), 1))(*[_lib.SeriesDst(*v) for v in dsts])
        g = (_lib.SeriesSeg * max(len(segs), 1))(*[_lib.SeriesSeg(*v) for v in segs])
        rc = _lib.lib.dlwp_series_window_gather(None, None if 'srcs' in null else s, len(srcs) if n_src is None else n_src,
                                                None if 'dsts' in null else d, len(dsts) if n_dst is None else n_dst,
                                                None if 'segs' in null else g, len(segs) if n_seg is None else n_seg,
                                                ctypes.c_void_p(samples), LL(n), None)
        return rc, _lib.lib.dlwp_last_error().decode()

    def refused(match, **kw):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and match in msg, (kw, rc, msg)

    refused('n_src 0', n_src=0)
    refused('n_src 5', n_src=5)
    refused('n_dst 0', n_dst=0)
    refused('n_dst 33', n_dst=33)
    refused('n_seg 0', n_seg=0)
    refused('n_seg 65', n_seg=65)
    refused('n -1', n=-1)
    for table in ('srcs', 'dsts', 'segs'):
        refused('null pointer', null=(table,))
    refused('null pointer (source 0)', srcs=((0, 10, 16),))
    refused('null pointer (destination 1)', dsts=((FAKE, 16), (0, 16)))
    refused('rows 0', srcs=((FAKE, 0, 16),))
    refused('row 0', srcs=((FAKE, 10, 0),))
    refused('row -4', dsts=((FAKE, -4),))
    refused('floats overflow', srcs=((FAKE, 1 << 40, 1 << 40),))
    refused('floats overflow', dsts=((FAKE, 1 << 50),), n=1 << 20)
    refused('source 1 of 1', segs=((1, 0, 0, 0, 0, 16),))
    refused('source -1 of 1', segs=((-1, 0, 0, 0, 0, 16),))
    refused('destination 1 of 1', segs=((0, 1, 0, 0, 0, 16),))
    refused('len 0', segs=((0, 0, 0, 0, 0, 0),))
    refused('src_at 16 leaves the source row', segs=((0, 0, 0, 16, 0, 4),))
    refused('src_at -1 leaves the source row', segs=((0, 0, 0, -1, 0, 4),))
    refused('dst_at 13 + len 4 leaves the destination row', segs=((0, 0, 0, 0, 13, 4),))
    refused('dst_at -1', segs=((0, 0, 0, 0, -1, 4),))
    refused('overflow', segs=((0, 0, 1 << 41, 0, 0, 4),))
    refused('len 2305843009213693943 or shift 0 overflow', dsts=((FAKE, (1 << 61) - 1),), segs=((0, 0, 0, 0, 0, (1 << 61) - 9),), n=1)
    refused('source rows overflows', dsts=((FAKE, 1 << 50),), segs=((0, 0, 0, 0, 0, 1 << 50),), n=1)
    refused('chunks', srcs=((FAKE, 2, 1 << 50),), dsts=((FAKE, 1 << 50),), segs=((0, 0, 0, 0, 0, 1 << 50),), n=1)
    refused('null pointer (samples)', samples=0)
    refused('null handle')
    # n == 0 is a no-op once the tables are in order -- and only then
    assert call(n=0, samples=0)[0] == _lib.OK
    refused('len 0', segs=((0, 0, 0, 0, 0, 0),), n=0)
    # a run over the end of its source row is what a merged window is: accepted up to the null handle
    refused('null handle', segs=((0, 0, 0, 8, 0, 16),))


def test_tables_object_refuses_on_the_host_what_the_arrays_cannot_hold():
    class T(object):
        """no tensor: SeriesTables must refuse the counts before it touches one"""
    with pytest.raises(ValueError, match='at most 4, 32, 64'):
        ops.SeriesTables([T()] * 5, [T()], [[0, 0, 0, 0, 0, 1]])
    with pytest.raises(ValueError, match='at least one'):
        ops.SeriesTables([T()], [T()], np.zeros((0, 6), np.int64))
    assert ops.series_chunks([[0, 0, 0, 0, 0, 4096], [0, 0, 0, 0, 0, 4100], [0, 1, 0, 0, 0, 4]], True) == 1 + 2 + 1
    assert ops.series_chunks([[0, 0, 0, 0, 0, 4096], [0, 0, 0, 0, 0, 5]], False) == 4 + 1
