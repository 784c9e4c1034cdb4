"""AveragePooling2D(2) on the GPU (csrc/halo.hip: dlwp_avgpool2_fwd / _bwd through every layer of the stack).

Kernels, through dlwp_amd.ops in the guarded slabs of tests/test_gpu_train_ops.py (outputs start as NaN between guard elements that
must keep their bits).  The stated arithmetic is demanded to the bit: forward ((a + b) + (c + d)) * 0.25f, bfloat16 storage the same
expression on the widened values rounded to nearest-even once, backward 0.25f * dy inside a window and +0 on an odd last row /
column.  The shapes reach the two-window (W % 4 == 0), one-window (W even) and scalar routes, odd edges and odd plane bases, and
every tensor is also placed 0 ... 3 floats past a 16-byte boundary: every placement must give the bits of the aligned call.

Models (batch 3, 4 channels, 8 x 12 unless stated) against float64 torch on the CPU: predict, one training step against autograd,
the recorded / replayed step against the eager one, the captured rollout against the host loop, model files in both formats, a
hand-written Keras checkpoint, and bfloat16 activation storage."""
import itertools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from tests.test_gpu_batchnorm import _bits, _grads_of, _host, _randomise, _ref_params
from tests.test_gpu_convlstm_bwd import BWD_TOL
from tests.test_gpu_dense import TOL
from tests.test_gpu_model import FWD_TOL
from tests.test_gpu_train_ops import Slab, same_bits

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
# (n, c, H, W): W = 2 and 10 take the one-window route, 8, 4 and 12 the two-window route, 7 the scalar one; H = 5, 3 and 7 leave a
# row over, W = 7 a column; 5 x 7 and 3 x 4 ... planes start at odd / non-multiple-of-4 element offsets
SHAPES = [(3, 1, 2, 2), (2, 3, 5, 7), (2, 3, 6, 10), (1, 2, 4, 8), (2, 5, 3, 4), (1, 3, 7, 12)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------------------------------------------------- #
# restatements
# ----------------------------------------------------------------------------------------------------------------------- #
def windows(x):
    """a, b, c, d of every 2 x 2 window, row-major"""
    h2, w2 = x.shape[2] // 2, x.shape[3] // 2
    return (x[:, :, 0:2 * h2:2, 0:2 * w2:2], x[:, :, 0:2 * h2:2, 1:2 * w2:2], x[:, :, 1:2 * h2:2, 0:2 * w2:2],
            x[:, :, 1:2 * h2:2, 1:2 * w2:2])


def np_fwd(x):
    """the stated float32 expression: three additions and one multiplication, each rounded once (numpy float32 is IEEE)"""
    a, b, c, d = windows(np.asarray(x, np.float32))
    return ((a + b) + (c + d)) * np.float32(0.25)


def np_bwd(dy, shape):
    n, c, h, w = shape
    h2, w2 = h // 2, w // 2
    dx = np.zeros(shape, np.float32)
    g = np.float32(0.25) * np.asarray(dy, np.float32).reshape(n, c, h2, w2)
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        dx[:, :, i:2 * h2:2, j:2 * w2:2] = g
    return dx


def to_bf16_bits(v):
    """float32 -> bfloat16 bits, round to nearest even (finite values)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def reals(shape, seed):
    """normal float32 values over a few decades, both signs"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


def run_fwd(ops, x, ax=0, ay=0):
    n, c, h, w = x.shape
    xs, ys = Slab(x, ax), Slab(None, ay, shape=(n, c, h // 2, w // 2))
    ops.avgpool2(xs.t, out=ys.t)
    got = ys.read()
    assert xs.unchanged()
    return got


def run_bwd(ops, dy, shape, ady=0, adx=0):
    ds, xs = Slab(dy, ady), Slab(None, adx, shape=shape)           # dx starts as NaN: every element must be written
    ops.avgpool2_bwd(ds.t, shape, out=xs.t)
    got = xs.read()
    assert ds.unchanged()
    return got


# ----------------------------------------------------------------------------------------------------------------------- #
# kernels
# ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_float32_bits_bound_and_exact_integers(ops, shape):
    x = reals(shape, 1)
    assert np.isfinite(x).all() and (np.abs(x[x != 0]) > 1e-30).all()
    got = run_fwd(ops, x)
    assert got.shape == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
    assert same_bits(got, np_fwd(x))
    # three roundings of relative size 2^-24 each: (a + b), (c + d), their sum; the multiplication by 0.25 is exact in the normal
    # range.  |error| <= 2^-24 (|a + b| + |c + d| + |a + b + c + d|) / 4 (1 + small) <= 2^-23 mean(|a|, |b|, |c|, |d|)
    a, b, c, d = [v.astype(np.float64) for v in windows(x)]
    mean = (a + b + c + d) / 4.0
    bound = 2.0 ** -23 * (np.abs(a) + np.abs(b) + np.abs(c) + np.abs(d)) / 4.0
    err = np.abs(got.astype(np.float64) - mean)
    print('\nMEASURED forward %r: worst error / bound %.3f' % (shape, float((err / bound).max())))
    assert (err <= bound).all()
    # small integers: every sum is exact, and so is the quarter
    xi = np.random.default_rng(2).integers(-64, 65, shape).astype(np.float32)
    ai, bi, ci, di = [v.astype(np.float64) for v in windows(xi)]
    assert np.array_equal(run_fwd(ops, xi).astype(np.float64), (ai + bi + ci + di) / 4.0)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_every_alignment_gives_the_bits_of_the_aligned_call(ops, shape):
    """x / dx and y / dy 0 ... 3 floats past a 16-byte boundary: whichever route the host picks, the same bits, inside the guards"""
    x = reals(shape, 3)
    dy = reals((shape[0], shape[1], shape[2] // 2, shape[3] // 2), 4)
    fwd0, bwd0 = run_fwd(ops, x), run_bwd(ops, dy, shape)
    assert same_bits(fwd0, np_fwd(x)) and same_bits(bwd0, np_bwd(dy, shape))
    for ax, ay in itertools.product(range(4), range(4)):
        if (ax, ay) != (0, 0):
            assert same_bits(run_fwd(ops, x, ax, ay), fwd0), ('forward', ax, ay)
            assert same_bits(run_bwd(ops, dy, shape, ay, ax), bwd0), ('backward', ax, ay)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_bfloat16_bits_and_one_ulp(ops, shape):
    xb = to_bf16_bits(reals(shape, 5))
    xw = from_bf16_bits(xb)                                               # the widened values
    x = torch.from_numpy(xb.view(np.int16)).cuda().view(torch.bfloat16)
    y = ops.avgpool2(x)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
    torch.cuda.synchronize()
    got = y.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, to_bf16_bits(np_fwd(xw)))
    a, b, c, d = [v.astype(np.float64) for v in windows(xw)]
    mean = (a + b + c + d) / 4.0
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(mean), 1e-300))) - 7)      # bfloat16: 8 significant bits
    err = np.abs(from_bf16_bits(got).astype(np.float64) - mean)
    print('\nMEASURED bf16 forward %r: worst error %.3f ulp' % (shape, float((err / ulp).max())))
    assert (err <= ulp).all()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_writes_everything_quarter_gradients_and_plus_zero_on_the_odd_edge(ops, shape):
    n, c, h, w = shape
    h2, w2 = h // 2, w // 2
    dy = reals((n, c, h2, w2), 6)
    got = run_bwd(ops, dy, shape)
    assert not np.isnan(got).any(), 'elements of dx were left unwritten'
    q = np.float32(0.25) * dy
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert same_bits(got[:, :, i:2 * h2:2, j:2 * w2:2], q)
    assert not got[:, :, 2 * h2:, :].view(np.uint32).any() and not got[:, :, :, 2 * w2:].view(np.uint32).any()      # +0, not -0
    assert same_bits(got, np_bwd(dy, shape))
    # the adjoint of the forward, exactly, on integer data
    rng = np.random.default_rng(7)
    xi, di = rng.integers(-32, 33, shape).astype(np.float32), (4 * rng.integers(-32, 33, (n, c, h2, w2))).astype(np.float32)
    lhs = (run_fwd(ops, xi).astype(np.float64) * di).sum()
    rhs = (xi.astype(np.float64) * run_bwd(ops, di, shape).astype(np.float64)).sum()
    assert lhs == rhs


def test_no_members_and_maps_of_one_row_or_column(ops):
    x = torch.empty((0, 3, 4, 4), device='cuda')
    assert tuple(ops.avgpool2(x).shape) == (0, 3, 2, 2)
    assert tuple(ops.avgpool2_bwd(torch.empty((0, 3, 2, 2), device='cuda'), (0, 3, 4, 4)).shape) == (0, 3, 4, 4)
    for shape in ((1, 1, 1, 5), (1, 1, 5, 1), (2, 3, 1, 8), (2, 3, 6, 1)):
        y = ops.avgpool2(torch.ones(shape, device='cuda'))
        assert y.numel() == 0 and tuple(y.shape) == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
        for adx in range(4):
            got = run_bwd(ops, np.zeros(tuple(y.shape), np.float32), shape, 0, adx)
            assert not got.view(np.uint32).any(), shape


def test_library_refuses_bad_arguments_without_a_launch(ops):
    import ctypes
    from dlwp_amd import _lib
    h = _lib.handle(torch.cuda.current_device())
    dy, dx = Slab(np.ones((1, 2, 2, 3), np.float32)), Slab(None, shape=(1, 2, 4, 6))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                           # noqa: E731
    S = _lib.Shape4
    bad = [(_lib.lib.dlwp_avgpool2_bwd, (h, p(dy.t), p(dx.t), S(1, 0, 4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (h, p(dy.t), p(dx.t), S(1, 2, -4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (h, p(dy.t), p(dx.t), S(-1, 2, 4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (h, p(dy.t), p(dx.t), S(1, 2, 4, 6), _lib.BF16, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (h, p(dy.t), p(dx.t), S(1, 2, 4, 6), 7, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (h, None, p(dx.t), S(1, 2, 4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (h, p(dy.t), None, S(1, 2, 4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_bwd, (None, p(dy.t), p(dx.t), S(1, 2, 4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_fwd, (h, p(dx.t), p(dy.t), S(1, 2, 4, 0), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_fwd, (h, p(dx.t), p(dy.t), S(1, 2, 4, 6), 7, stream)),
           (_lib.lib.dlwp_avgpool2_fwd, (h, None, p(dy.t), S(1, 2, 4, 6), _lib.F32, stream)),
           (_lib.lib.dlwp_avgpool2_fwd, (h, p(dx.t), None, S(1, 2, 4, 6), _lib.F32, stream))]
    for fn, args in bad:
        assert fn(*args) == _lib.EINVAL, args[3:5]
        assert _lib.lib.dlwp_last_error()
    assert np.isnan(dx.read()).all() and dy.unchanged()                   # nothing ran
    # ... and the same pointers with good arguments do
    assert _lib.lib.dlwp_avgpool2_bwd(h, p(dy.t), p(dx.t), S(1, 2, 4, 6), _lib.F32, stream) == _lib.OK
    assert same_bits(dx.read(), np.full((1, 2, 4, 6), 0.25, np.float32))


def test_nan_poisons_its_own_window_only(ops):
    for shape in ((1, 2, 5, 7), (1, 2, 4, 8), (1, 2, 6, 10)):
        x = reals(shape, 8)
        x[0, 1, 3, 2] = np.nan                                            # window (1, 1) of plane 1
        x[0, 0, -1, -1] = np.nan if shape[2] % 2 else x[0, 0, -1, -1]     # the odd edge belongs to no window
        got = run_fwd(ops, x)
        want = np.zeros(got.shape, bool)
        want[0, 1, 1, 1] = True
        assert np.array_equal(np.isnan(got), want), shape
        xb = torch.from_numpy(x).cuda().to(torch.bfloat16)
        assert np.array_equal(np.isnan(_host(ops.avgpool2(xb).float())), want), shape
        dy = reals(got.shape, 9)
        dy[0, 0, 0, 1] = np.nan
        gb = run_bwd(ops, dy, shape)
        wantb = np.zeros(shape, bool)
        wantb[0, 0, 0:2, 2:4] = True
        assert np.array_equal(np.isnan(gb), wantb), shape


# ----------------------------------------------------------------------------------------------------------------------- #
# models
# ----------------------------------------------------------------------------------------------------------------------- #
def _pads(t):
    from dlwp_amd.custom import PeriodicPadding2D
    return L.ZeroPadding2D(((1, 1), (0, 0)), **CF)(PeriodicPadding2D(((0, 0), (1, 1)), **CF)(t))


def _pads_ref(t):
    return F.pad(torch.cat([t[..., -1:], t, t[..., :1]], dim=-1), (0, 0, 1, 1))


def _conv_ref(t, lay, p, pad=True):
    t = F.conv2d(_pads_ref(t) if pad else t, p[(lay.name, 'kernel')], padding=0 if pad else 1)
    t = t + p[(lay.name, 'bias')].view(1, -1, 1, 1)
    return torch.tanh(t) if lay.activation == 'tanh' else t


def net_a(cs=(4, 8, 12)):
    """periodic / zero padding + conv(8, tanh) -> AveragePooling2D -> conv(16, tanh) -> UpSampling2D -> concatenate with the skip
    -> conv(4, linear)"""
    x0 = L.Input(shape=cs)
    skip = L.Conv2D(8, 3, activation='tanh', **CF)(_pads(x0))
    t = L.Conv2D(16, 3, activation='tanh', **CF)(_pads(L.AveragePooling2D(2, **CF)(skip)))
    t = L.concatenate([L.UpSampling2D(2, **CF)(t), skip], axis=1)
    return x0, L.Conv2D(cs[0], 3, **CF)(_pads(t))


def net_a_ref(model, x, p):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    skip = _conv_ref(x, convs[0], p)
    t = _conv_ref(F.avg_pool2d(skip, 2), convs[1], p)
    t = torch.cat([F.interpolate(t, scale_factor=2, mode='nearest'), skip], dim=1)
    return _conv_ref(t, convs[2], p)


def net_b(cs=(4, 7, 9)):
    """sequential, an odd edge in both directions, no skip: conv(8, tanh, 'same') -> AveragePooling2D -> conv(4, 'same')"""
    x0 = L.Input(shape=cs)
    t = L.AveragePooling2D((2, 2), strides=(2, 2), **CF)(L.Conv2D(8, 3, padding='same', activation='tanh', **CF)(x0))
    return x0, L.Conv2D(cs[0], 3, padding='same', **CF)(t)


def net_b_ref(model, x, p):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    return _conv_ref(F.avg_pool2d(_conv_ref(x, convs[0], p, pad=False), 2), convs[1], p, pad=False)


def net_c(cs=(4, 8, 12)):
    """slice_layer -> AveragePooling2D as the model's output: a channel window as input, the output buffer as target"""
    from dlwp_amd.custom import slice_layer
    x0 = L.Input(shape=cs)
    return x0, L.AveragePooling2D(2, **CF)(slice_layer(1, 3, axis=1)(x0))


def net_c_ref(model, x, p):
    return F.avg_pool2d(x[:, 1:3], 2)


NETS = {'a': (net_a, net_a_ref, (4, 8, 12)), 'b': (net_b, net_b_ref, (4, 7, 9)), 'c': (net_c, net_c_ref, (4, 8, 12))}


def _model(which, seed=1, lr=1e-3):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0, out = NETS[which][0]()
    m = Model(inputs=x0, outputs=out, seed=seed)
    if which != 'c':                                                      # (net c has nothing to train)
        m.compile(optimizer=Adam(lr=lr), loss='mse')
    _randomise(m, np.random.default_rng(seed + 100))
    return m


def _data(cs, seed, n=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n,) + cs).astype(np.float32), rng.standard_normal((n,) + cs).astype(np.float32))


@pytest.mark.parametrize('which', ['a', 'b', 'c'])
def test_predict_against_float64(which):
    m = _model(which)
    cs = NETS[which][2]
    assert [op.kind for op in m.infer_plan.ops].count('avgpool') == 1
    x, _ = _data(cs, 11)
    with torch.no_grad():
        want = NETS[which][1](m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False)).numpy()
    got = m.predict(x)
    assert got.shape == want.shape
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print('\nMEASURED predict net %s: error %.3g of scale %.3g = %.3g' % (which, err, scale, err / scale))
    assert err <= FWD_TOL * scale


def test_training_step_against_float64_autograd(monkeypatch):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model('a', seed=2)
    cs = NETS['a'][2]
    assert [op.kind for op in m.plan.ops].count('avgpool') == 1
    x, y = _data(cs, 12)
    p = _ref_params(m)
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    ref = ((net_a_ref(m, torch.tensor(x, dtype=torch.float64), p) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    ref.backward()
    print('\nMEASURED step net a: loss %.8g against %.8g' % (loss, float(ref.detach())))
    got = _grads_of(m._trainer)
    assert len(got) == sum(1 for t in p.values() if t.requires_grad) == 6
    worst = 0.0
    for (lname, nm), g in sorted(got.items()):
        r = p[(lname, nm)].grad.numpy()
        r = r.transpose(2, 3, 1, 0) if nm == 'kernel' else r
        ratio = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-6))
        worst = max(worst, ratio)
        print('MEASURED   %s/%s gradient error %.3g of its scale' % (lname, nm, ratio))
    assert loss == pytest.approx(float(ref.detach()), rel=TOL)
    assert worst <= BWD_TOL, worst


def _run_steps(monkeypatch, form, batches):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)
    m = _model('a', seed=5)
    logs = [m.train_on_batch(x, y) for x, y in batches]
    torch.cuda.synchronize()
    tr = m._trainer
    if form != 'eager':
        n = batches[0][0].shape[0]
        ents = [e for k, e in tr._graphs.items() if k[0] == n and e.get('step') is not None]
        assert len(ents) == 1, 'the step of %d samples was not recorded (refused: %r)' % (n, tr._no_tape)
    return logs, [w.copy() for w in m.get_weights()], [s.cpu().numpy() for s in tr.opt_state]


def test_replayed_step_equals_the_eager_step(monkeypatch):
    """2 eager steps, then the recorded (and validated) one and 2 replayed ones: nothing marks the tape foreign"""
    batches = [_data(NETS['a'][2], 600 + i) for i in range(5)]
    ref = _run_steps(monkeypatch, 'eager', batches)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, form, batches)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
            assert np.array_equal(_bits(a), _bits(b)), form


def test_captured_rollout_equals_the_host_loop():
    from dlwp_amd.model import DLWPFunctional
    cs = NETS['a'][2]
    m = _model('a', seed=6)
    d = DLWPFunctional(is_convolutional=True, is_recurrent=False, time_dim=2)
    d.model = d.base_model = m
    x, _ = _data(cs, 15, n=5)
    assert d._device_rollout_ok(x)
    kept = d.predict_timeseries(x, 8, keep_time_dim=True)            # one hipGraph of 4 forwards
    state, want = x, []
    for _ in range(4):
        state = m.predict(state)
        want.append(state)
    want = np.stack(want)
    assert np.isfinite(want).all() and kept.shape == (4, 5, 2, 2) + cs[1:]
    assert np.array_equal(_bits(kept), _bits(want.reshape(kept.shape)))
    ser = _host(m.rollout_on_device(torch.from_numpy(x).cuda(), 4, graph_cache=False))
    assert np.array_equal(_bits(ser), _bits(want))


@pytest.mark.parametrize('fmt', ['keras', 'npz'])
def test_saved_and_reloaded_model_predicts_and_trains_the_same_bits(tmp_path, monkeypatch, fmt):
    from dlwp_amd import serialization
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    cs = NETS['a'][2]
    batches = [_data(cs, 800 + i) for i in range(4)]
    m = _model('a', seed=7)
    for x, y in batches[:2]:
        m.train_on_batch(x, y)
    path = str(tmp_path / ('a.%s' % fmt))
    m.save(path, format=fmt)
    m2 = serialization.load_model_file(path)
    assert [type(lay).__name__ for lay in m2.layers] == [type(lay).__name__ for lay in m.layers]
    pool = [lay for lay in m2.layers if isinstance(lay, L.AveragePooling2D)]
    assert len(pool) == 1 and pool[0].get_config() == [lay for lay in m.layers if isinstance(lay, L.AveragePooling2D)][0].get_config()
    assert np.array_equal(_bits(m2.predict(batches[0][0])), _bits(m.predict(batches[0][0])))
    for x, y in batches[2:]:
        a, b = m.train_on_batch(x, y), m2.train_on_batch(x, y)
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(_bits(a), _bits(b))


def test_hand_written_keras_checkpoint_imports(tmp_path):
    """a Sequential as Keras 2.2 writes it: the pooling layer with pool_size / strides as lists, padding 'valid'"""
    from dlwp_amd import hdf5_lite, serialization
    rng = np.random.default_rng(21)
    cs = (4, 8, 12)

    def conv(name, filters, first=False):
        c = {'name': name, 'trainable': True, 'filters': filters, 'kernel_size': [3, 3], 'strides': [1, 1], 'padding': 'same',
             'data_format': 'channels_first', 'dilation_rate': [1, 1], 'activation': 'tanh' if first else 'linear', 'use_bias': True,
             'kernel_initializer': {'class_name': 'VarianceScaling',
                                    'config': {'scale': 1.0, 'mode': 'fan_avg', 'distribution': 'uniform', 'seed': None}},
             'bias_initializer': {'class_name': 'Zeros', 'config': {}}, 'kernel_regularizer': None, 'bias_regularizer': None,
             'activity_regularizer': None, 'kernel_constraint': None, 'bias_constraint': None}
        if first:
            c.update(batch_input_shape=[None] + list(cs), dtype='float32')
        return {'class_name': 'Conv2D', 'config': c}
    pool = {'class_name': 'AveragePooling2D',
            'config': {'name': 'average_pooling2d_1', 'trainable': True, 'pool_size': [2, 2], 'padding': 'valid', 'strides': [2, 2],
                       'data_format': 'channels_first'}}
    config = {'class_name': 'Sequential', 'config': {'name': 'sequential_1', 'layers': [conv('conv2d_1', 8, True), pool,
                                                                                       conv('conv2d_2', 4)]}}
    weights = {'conv2d_1': [(0.3 * rng.standard_normal((3, 3, 4, 8))).astype(np.float32), (0.1 * rng.standard_normal(8)).astype(np.float32)],
               'conv2d_2': [(0.3 * rng.standard_normal((3, 3, 8, 4))).astype(np.float32), (0.1 * rng.standard_normal(4)).astype(np.float32)]}
    root = hdf5_lite.GroupSpec()
    root.attrs['keras_version'] = b'2.2.4'
    root.attrs['backend'] = b'tensorflow'
    root.attrs['model_config'] = json.dumps(config).encode('utf-8')
    mw = root.create_group('model_weights')
    mw.attrs['layer_names'] = np.array([b'conv2d_1', b'average_pooling2d_1', b'conv2d_2'])
    for name in ('conv2d_1', 'average_pooling2d_1', 'conv2d_2'):
        g = mw.create_group(name)
        if name in weights:
            g.attrs['weight_names'] = np.array([('%s/kernel:0' % name).encode(), ('%s/bias:0' % name).encode()])
            g.create_dataset('%s/kernel:0' % name, weights[name][0])
            g.create_dataset('%s/bias:0' % name, weights[name][1])
    path = str(tmp_path / 'avgpool.h5')
    hdf5_lite.write_file(path, root)
    m = serialization.import_keras_hdf5(path)
    assert [type(lay).__name__ for lay in m.layers if not isinstance(lay, L.InputLayer)] == ['Conv2D', 'AveragePooling2D', 'Conv2D']
    assert [op.kind for op in m.infer_plan.ops] == ['conv', 'avgpool', 'conv']
    x, _ = _data(cs, 22)
    k1, b1, k2, b2 = [torch.tensor(a.astype(np.float64)) for a in weights['conv2d_1'] + weights['conv2d_2']]
    t = torch.tanh(F.conv2d(torch.tensor(x, dtype=torch.float64), k1.permute(3, 2, 0, 1), b1, padding=1))
    want = F.conv2d(F.avg_pool2d(t, 2), k2.permute(3, 2, 0, 1), b2, padding=1).numpy()
    got = m.predict(x)
    assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()


def test_bfloat16_activation_storage():
    """conv -> AveragePooling2D -> conv at 16 x 24 (the second convolution reads the pooled buffer through a lazy up-sampling, so
    that the output has the input's shape and the model can be rolled out): the convolution's output and its pooled image are
    stored as bfloat16; the bounds are those of tests/test_gpu_configs.py for the project's bf16 mode, against the float64
    reference of the float32 mode"""
    from dlwp_amd.engine import Model
    from dlwp_amd.model import DLWPFunctional
    cs = (4, 16, 24)
    x0 = L.Input(shape=cs)
    t = L.AveragePooling2D(2, **CF)(L.Conv2D(16, 3, activation='tanh', **CF)(_pads(x0)))
    m = Model(inputs=x0, outputs=L.Conv2D(cs[0], 3, **CF)(_pads(L.UpSampling2D(2, **CF)(t))), seed=9)
    _randomise(m, np.random.default_rng(31))
    x, _ = _data(cs, 32, n=5)
    p = _ref_params(m, requires_grad=False)
    convs = [lay for lay in m.layers if isinstance(lay, L.Conv2D)]
    with torch.no_grad():
        t64 = F.avg_pool2d(_conv_ref(torch.tensor(x, dtype=torch.float64), convs[0], p), 2)
        want = _conv_ref(F.interpolate(t64, scale_factor=2, mode='nearest'), convs[1], p).numpy()
    got32 = m.predict(x)
    assert np.abs(got32 - want).max() <= FWD_TOL * np.abs(want).max()
    m.set_activation_dtype('bfloat16')
    pool = [op for op in m.infer_plan.ops if op.kind == 'avgpool']
    assert len(pool) == 1
    bufs = m.executor.scratch(5)
    assert bufs[pool[0].src].dtype == torch.bfloat16 and bufs[pool[0].dst].dtype == torch.bfloat16
    assert {pool[0].src, pool[0].dst} <= set(m.infer_plan.bf16_buffers())
    got = m.predict(x)
    scale = max(1.0, float(np.abs(want).max()))
    rel, mean = float(np.abs(got - want).max()) / scale, float(np.abs(got - want).mean())
    print('\nMEASURED bf16 storage: max error %.3g of scale, mean error %.3g (scale %.3g)' % (rel, mean, scale))
    assert rel < 1e-2
    assert mean < 1e-3 * scale
    # a two-step captured rollout replays exactly that forward
    d = DLWPFunctional(is_convolutional=True, is_recurrent=False, time_dim=2)
    d.model = d.base_model = m
    series = np.asarray(d.predict_timeseries(x, 4, keep_time_dim=True))
    second = m.predict(got)
    assert series.shape == (2, 5, 2, 2) + cs[1:]
    assert np.array_equal(_bits(series[0].reshape(got.shape)), _bits(got))
    assert np.array_equal(_bits(series[1].reshape(got.shape)), _bits(second))
    m.set_activation_dtype('float32')
    assert np.array_equal(_bits(m.predict(x)), _bits(got32))
