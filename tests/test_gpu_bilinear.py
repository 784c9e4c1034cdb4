"""UpSampling2D(2, interpolation='bilinear') on the GPU (csrc/halo.hip: dlwp_upsample2_bilinear_fwd / _bwd through every layer of the
stack).

Kernels, through dlwp_amd.ops in the guarded slabs of tests/test_gpu_train_ops.py (outputs start as NaN between guard elements that
must keep their bits).  The stated arithmetic is demanded to the bit, against the numpy restatements of tests/test_bilinear_cpu.py:
forward a + (b - a) * 0.5f along the rows and then the columns with the last neighbour clamped, bfloat16 storage the same
expression on the widened values rounded to nearest-even once, backward the gather-form adjoint (v0 + 0.5f vm) + 0.5f vp along
both axes.  The shapes reach one row, one column, clamped edges, the 16-byte (W even), 8-byte and scalar routes and planes at odd
element offsets, and every tensor is also placed 0 ... 3 floats past a 16-byte boundary: every placement must give the bits of the
aligned call.

Models (batch 3, 4 channels, 8 x 12 and 6 x 9) against a float64 torch restatement built from the interpolation matrices (torch's
own interpolate uses half-pixel centres): predict, one training step against autograd, the recorded / replayed step against the
eager one, the captured rollout against the host loop, model files in both formats, a hand-written Keras checkpoint, and bfloat16
activation storage.

Measured on an MI355X (error / bound): kernels forward <= 0.66 and backward <= 0.62 of the rounding bound; predict 0.053 (net a at
8 x 12), 0.042 (net a at 6 x 9) and 0.004 (net b) of FWD_TOL; the training step's loss 0.005 of TOL, its gradients <= 0.037 of BWD_TOL;
bfloat16 storage 3.3e-3 of scale (max) and 1.0e-3 (mean)."""
import itertools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from tests.test_bilinear_cpu import ROUNDING, bwd64, fwd64, matrix, np_bwd, np_fwd, reals
from tests.test_gpu_avgpool import from_bf16_bits, to_bf16_bits
from tests.test_gpu_batchnorm import _bits, _grads_of, _host, _randomise, _ref_params
from tests.test_gpu_convlstm_bwd import BWD_TOL
from tests.test_gpu_dense import TOL
from tests.test_gpu_model import FWD_TOL
from tests.test_gpu_train_ops import Slab, same_bits

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
# (n, c, H, W): one element; one row; one column; odd x odd (planes of 35 floats: odd element offsets, 8-byte and scalar routes);
# W = 8, 4, 12, 10 take the 16-byte route when the pointers allow it; 3 x 4 ... planes that start off a 16-byte boundary
SHAPES = [(3, 1, 1, 1), (2, 3, 1, 5), (2, 3, 4, 1), (2, 3, 5, 7), (1, 2, 4, 8), (2, 5, 3, 4), (1, 3, 7, 12), (2, 3, 6, 10)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def up(shape):
    return (shape[0], shape[1], 2 * shape[2], 2 * shape[3])


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def run_fwd(ops, x, ax=0, ay=0):
    xs, ys = Slab(x, ax), Slab(None, ay, shape=up(x.shape))               # y starts as NaN: every element must be written
    ops.upsample2_bilinear(xs.t, out=ys.t)
    got = ys.read()
    assert xs.unchanged()
    return got


def run_bwd(ops, dy, shape, ady=0, adx=0):
    ds, xs = Slab(dy, ady), Slab(None, adx, shape=shape)                  # dx starts as NaN: every element must be written
    ops.upsample2_bilinear_bwd(ds.t, shape, out=xs.t)
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
    assert got.shape == up(shape) and not np.isnan(got).any(), 'elements of y were left unwritten'
    assert same_bits(got, np_fwd(x))
    assert same_bits(got[:, :, 0::2, 0::2], x)                            # the bits are copied
    err, bound = np.abs(got.astype(np.float64) - fwd64(x)), ROUNDING * fwd64(np.abs(x))
    print('\nMEASURED forward %r: worst error / bound %.3f' % (shape, float((err / bound).max())))
    assert (err <= bound).all()
    xi = np.random.default_rng(2).integers(-64, 65, shape).astype(np.float32)
    assert np.array_equal(run_fwd(ops, xi).astype(np.float64), fwd64(xi))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_float32_bits_bound_and_the_exact_adjoint(ops, shape):
    dy = reals(up(shape), 6)
    got = run_bwd(ops, dy, shape)
    assert got.shape == shape and not np.isnan(got).any(), 'elements of dx were left unwritten'
    assert same_bits(got, np_bwd(dy, shape))
    err, bound = np.abs(got.astype(np.float64) - bwd64(dy, shape)), ROUNDING * bwd64(np.abs(dy), shape)
    print('\nMEASURED backward %r: worst error / bound %.3f' % (shape, float((err / bound).max())))
    assert (err <= bound).all()
    # the adjoint of the forward, exactly, on integer data
    rng = np.random.default_rng(7)
    xi, di = rng.integers(-32, 33, shape).astype(np.float32), (4 * rng.integers(-32, 33, up(shape))).astype(np.float32)
    gi = run_bwd(ops, di, shape)
    assert np.array_equal(gi.astype(np.float64), bwd64(di, shape))
    assert (run_fwd(ops, xi).astype(np.float64) * di).sum() == (xi.astype(np.float64) * gi.astype(np.float64)).sum()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_every_alignment_gives_the_bits_of_the_aligned_call(ops, shape):
    """x / dx and y / dy 0 ... 3 floats past a 16-byte boundary: whichever route the host picks, the same bits, inside the guards"""
    x, dy = reals(shape, 3), reals(up(shape), 4)
    fwd0, bwd0 = run_fwd(ops, x), run_bwd(ops, dy, shape)
    assert same_bits(fwd0, np_fwd(x)) and same_bits(bwd0, np_bwd(dy, shape))
    for ax, ay in itertools.product(range(4), range(4)):
        if (ax, ay) != (0, 0):
            assert same_bits(run_fwd(ops, x, ax, ay), fwd0), ('forward', ax, ay)
            assert same_bits(run_bwd(ops, dy, shape, ay, ax), bwd0), ('backward', ax, ay)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_bfloat16_bits(ops, shape):
    xb = to_bf16_bits(reals(shape, 5))
    xw = from_bf16_bits(xb)                                               # the widened values
    want = to_bf16_bits(np_fwd(xw))
    for off in (0, 1):                                                    # 4-byte aligned and 2 bytes past it
        xbuf = torch.zeros(xb.size + 2, dtype=torch.int16, device='cuda')
        ybuf = torch.full((want.size + 2,), 0x7fc0, dtype=torch.int16, device='cuda')
        xbuf[off:off + xb.size] = torch.from_numpy(xb.view(np.int16).reshape(-1)).cuda()
        x = xbuf[off:off + xb.size].view(torch.bfloat16).view(shape)
        y = ybuf[off:off + want.size].view(torch.bfloat16).view(up(shape))
        assert ops.upsample2_bilinear(x, out=y) is y and y.dtype == torch.bfloat16
        torch.cuda.synchronize()
        whole = ybuf.cpu().numpy().view(np.uint16)
        assert np.array_equal(whole[off:off + want.size].reshape(want.shape), want), off
        assert (np.delete(whole, np.s_[off:off + want.size]) == 0x7fc0).all()         # nothing outside the tensor
    assert np.array_equal(want[:, :, 0::2, 0::2], xb)
    y = ops.upsample2_bilinear(torch.from_numpy(xb.view(np.int16)).cuda().view(torch.bfloat16))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == up(shape)
    assert np.array_equal(y.view(torch.int16).cpu().numpy().view(np.uint16), want)


def test_nan_poisons_the_outputs_whose_stencil_holds_it(ops):
    for shape, (i, j) in (((1, 2, 5, 7), (3, 2)), ((1, 2, 4, 8), (0, 7)), ((1, 2, 6, 10), (5, 0)), ((1, 2, 1, 5), (0, 4)),
                          ((1, 2, 4, 1), (2, 0))):
        x = reals(shape, 8)
        x[0, 1, i, j] = np.nan
        got = run_fwd(ops, x)
        want = np.zeros(got.shape, bool)
        want[0, 1, max(2 * i - 1, 0):2 * i + 2, max(2 * j - 1, 0):2 * j + 2] = True      # the clipped 3 x 3 block around (2i, 2j)
        assert np.array_equal(np.isnan(got), want), shape
        xb = torch.from_numpy(x).cuda().to(torch.bfloat16)
        assert np.array_equal(np.isnan(_host(ops.upsample2_bilinear(xb).float())), want), shape
        # backward: a NaN at dy[r][s] reaches the dx elements whose 3 x 3 block holds it
        dy = reals(up(shape), 9)
        dy[0, 0, 2 * i, 2 * j] = np.nan
        wantb = np.zeros(shape, bool)
        wantb[0, 0, i, j] = True
        assert np.array_equal(np.isnan(run_bwd(ops, dy, shape)), wantb), shape


def test_no_members(ops):
    x = torch.empty((0, 3, 4, 4), device='cuda')
    assert tuple(ops.upsample2_bilinear(x).shape) == (0, 3, 8, 8)
    assert tuple(ops.upsample2_bilinear(x.to(torch.bfloat16)).shape) == (0, 3, 8, 8)
    assert tuple(ops.upsample2_bilinear_bwd(torch.empty((0, 3, 8, 8), device='cuda'), (0, 3, 4, 4)).shape) == (0, 3, 4, 4)
    torch.cuda.synchronize()


def test_library_refuses_bad_arguments_without_a_launch(ops):
    import ctypes
    from dlwp_amd import _lib
    h = _lib.handle(torch.cuda.current_device())
    dy, dx = Slab(np.ones((1, 2, 4, 6), np.float32)), Slab(None, shape=(1, 2, 2, 3))
    x, y = Slab(np.ones((1, 2, 2, 3), np.float32)), Slab(None, shape=(1, 2, 4, 6))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)              # noqa: E731
    S = _lib.Shape4
    bwd, fwd = _lib.lib.dlwp_upsample2_bilinear_bwd, _lib.lib.dlwp_upsample2_bilinear_fwd
    bad = [(bwd, (h, p(dy.t), p(dx.t), S(1, 0, 2, 3), _lib.F32, stream)),
           (bwd, (h, p(dy.t), p(dx.t), S(1, 2, -2, 3), _lib.F32, stream)),
           (bwd, (h, p(dy.t), p(dx.t), S(-1, 2, 2, 3), _lib.F32, stream)),
           (bwd, (h, p(dy.t), p(dx.t), S(1, 2, 2, 3), _lib.BF16, stream)),
           (bwd, (h, p(dy.t), p(dx.t), S(1, 2, 2, 3), 7, stream)),
           (bwd, (h, None, p(dx.t), S(1, 2, 2, 3), _lib.F32, stream)),
           (bwd, (h, p(dy.t), None, S(1, 2, 2, 3), _lib.F32, stream)),
           (bwd, (None, p(dy.t), p(dx.t), S(1, 2, 2, 3), _lib.F32, stream)),
           (bwd, (h, p(dy.t, 2), p(dx.t), S(1, 2, 2, 3), _lib.F32, stream)),          # not a float32 address
           (fwd, (h, p(x.t), p(y.t), S(1, 2, 2, 0), _lib.F32, stream)),
           (fwd, (h, p(x.t), p(y.t), S(1, 2, 2, 3), 7, stream)),
           (fwd, (h, None, p(y.t), S(1, 2, 2, 3), _lib.F32, stream)),
           (fwd, (h, p(x.t), None, S(1, 2, 2, 3), _lib.F32, stream)),
           (fwd, (None, p(x.t), p(y.t), S(1, 2, 2, 3), _lib.F32, stream)),
           (fwd, (h, p(x.t), p(y.t, 2), S(1, 2, 2, 3), _lib.F32, stream)),
           (fwd, (h, p(x.t), p(y.t, 1), S(1, 2, 2, 3), _lib.BF16, stream))]
    for fn, args in bad:
        assert fn(*args) == _lib.EINVAL, args[3:5]
        assert _lib.lib.dlwp_last_error()
    assert np.isnan(dx.read()).all() and np.isnan(y.read()).all() and dy.unchanged() and x.unchanged()      # nothing ran
    # ... and the same pointers with good arguments do
    assert bwd(h, p(dy.t), p(dx.t), S(1, 2, 2, 3), _lib.F32, stream) == _lib.OK
    assert same_bits(dx.read(), np_bwd(np.ones((1, 2, 4, 6), np.float32), (1, 2, 2, 3)))
    assert fwd(h, p(x.t), p(y.t), S(1, 2, 2, 3), _lib.F32, stream) == _lib.OK
    assert same_bits(y.read(), np.ones((1, 2, 4, 6), np.float32))


# ----------------------------------------------------------------------------------------------------------------------- #
# models
# ----------------------------------------------------------------------------------------------------------------------- #
def _pads(t):
    from dlwp_amd.custom import PeriodicPadding2D
    return L.ZeroPadding2D(((1, 1), (0, 0)), **CF)(PeriodicPadding2D(((0, 0), (1, 1)), **CF)(t))


def _pads_ref(t):
    return F.pad(torch.cat([t[..., -1:], t, t[..., :1]], dim=-1), (0, 0, 1, 1))


def _conv_ref(t, lay, p):
    t = F.conv2d(_pads_ref(t), p[(lay.name, 'kernel')]) + p[(lay.name, 'bias')].view(1, -1, 1, 1)
    return torch.tanh(t) if lay.activation == 'tanh' else t


def bilinear_ref(t):
    """float64, from the interpolation matrices (differentiable)"""
    ah, aw = torch.tensor(matrix(t.shape[2])), torch.tensor(matrix(t.shape[3]))
    return torch.einsum('ri,ncij,sj->ncrs', ah, t, aw)


def net_a(cs):
    """padded conv(8, tanh) -> MaxPooling2D -> padded conv(16, tanh) -> bilinear UpSampling2D -> padded conv(4, linear)"""
    x0 = L.Input(shape=cs)
    t = L.Conv2D(8, 3, activation='tanh', **CF)(_pads(x0))
    t = L.Conv2D(16, 3, activation='tanh', **CF)(_pads(L.MaxPooling2D(2, **CF)(t)))
    t = L.UpSampling2D(2, interpolation='bilinear', **CF)(t)
    return x0, L.Conv2D(cs[0], 3, **CF)(_pads(t))


def net_a_ref(model, x, p):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    t = _conv_ref(F.max_pool2d(_conv_ref(x, convs[0], p), 2), convs[1], p)
    return _conv_ref(bilinear_ref(t), convs[2], p)


def net_b(cs):
    """slice_layer -> bilinear UpSampling2D as the model's output: a channel window as input, the output buffer as target"""
    from dlwp_amd.custom import slice_layer
    x0 = L.Input(shape=cs)
    return x0, L.UpSampling2D(2, interpolation='bilinear', **CF)(slice_layer(1, 3, axis=1)(x0))


def net_b_ref(model, x, p):
    return bilinear_ref(x[:, 1:3])


NETS = {'a': (net_a, net_a_ref), 'b': (net_b, net_b_ref)}
# 8 x 12: the decoder's map is 4 x 6; 6 x 9: net a pools to 3 x 4 and gives 6 x 8 (the odd column is lost in the pooling), net b
# interpolates 9 columns (the 8-byte route)
CASES = [('a', (4, 8, 12)), ('a', (4, 6, 9)), ('b', (4, 8, 12)), ('b', (4, 6, 9))]


def _model(which, cs=(4, 8, 12), seed=1, lr=1e-3):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0, out = NETS[which][0](cs)
    m = Model(inputs=x0, outputs=out, seed=seed)
    if which != 'b':                                                      # (net b has nothing to train)
        m.compile(optimizer=Adam(lr=lr), loss='mse')
    _randomise(m, np.random.default_rng(seed + 100))
    return m


def _data(cs, seed, n=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n,) + cs).astype(np.float32), rng.standard_normal((n,) + cs).astype(np.float32))


@pytest.mark.parametrize('which, cs', CASES, ids=['%s-%dx%d' % (w, c[1], c[2]) for w, c in CASES])
def test_predict_against_float64(which, cs):
    m = _model(which, cs)
    assert [op.kind for op in m.infer_plan.ops].count('bilinear') == 1
    x, _ = _data(cs, 11)
    with torch.no_grad():
        want = NETS[which][1](m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False)).numpy()
    got = m.predict(x)
    assert got.shape == want.shape
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print('\nMEASURED predict net %s %r: error %.3g of scale %.3g = %.3g, error / bound %.3g'
          % (which, cs, err, scale, err / scale, err / (FWD_TOL * scale)))
    assert err <= FWD_TOL * scale


@pytest.mark.parametrize('cs', [(4, 8, 12), (4, 6, 9)], ids=['8x12', '6x9'])
def test_training_step_against_float64_autograd(monkeypatch, cs):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model('a', cs, seed=2)
    assert [op.kind for op in m.plan.ops].count('bilinear') == 1
    x, y = _data(cs, 12)
    y = y[..., :2 * (cs[2] // 2)]                                         # (an odd column is lost in the pooling)
    p = _ref_params(m)
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    ref = ((net_a_ref(m, torch.tensor(x, dtype=torch.float64), p) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    ref.backward()
    print('\nMEASURED step net a %r: loss %.8g against %.8g, error / bound %.3g'
          % (cs, loss, float(ref.detach()), abs(loss - float(ref.detach())) / (TOL * abs(float(ref.detach())))))
    got = _grads_of(m._trainer)
    assert len(got) == sum(1 for t in p.values() if t.requires_grad) == 6
    worst = 0.0
    for (lname, nm), g in sorted(got.items()):
        r = p[(lname, nm)].grad.numpy()
        r = r.transpose(2, 3, 1, 0) if nm == 'kernel' else r
        ratio = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-6))
        worst = max(worst, ratio)
        print('MEASURED   %s/%s gradient error %.3g of its scale, error / bound %.3g' % (lname, nm, ratio, ratio / BWD_TOL))
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
    batches = [_data((4, 8, 12), 600 + i) for i in range(5)]
    ref = _run_steps(monkeypatch, 'eager', batches)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, form, batches)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
            assert np.array_equal(_bits(a), _bits(b)), form


def test_captured_rollout_equals_the_host_loop():
    from dlwp_amd.model import DLWPFunctional
    cs = (4, 8, 12)
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
    cs = (4, 8, 12)
    batches = [_data(cs, 800 + i) for i in range(4)]
    m = _model('a', seed=7)
    for x, y in batches[:2]:
        m.train_on_batch(x, y)
    path = str(tmp_path / ('a.%s' % fmt))
    m.save(path, format=fmt)
    m2 = serialization.load_model_file(path)
    assert [type(lay).__name__ for lay in m2.layers] == [type(lay).__name__ for lay in m.layers]
    ups = [lay for lay in m2.layers if isinstance(lay, L.UpSampling2D)]
    assert len(ups) == 1 and ups[0].interpolation == 'bilinear'
    assert ups[0].get_config() == [lay for lay in m.layers if isinstance(lay, L.UpSampling2D)][0].get_config()
    assert [op.kind for op in m2.infer_plan.ops].count('bilinear') == 1
    assert np.array_equal(_bits(m2.predict(batches[0][0])), _bits(m.predict(batches[0][0])))
    for x, y in batches[2:]:
        a, b = m.train_on_batch(x, y), m2.train_on_batch(x, y)
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(_bits(a), _bits(b))


def test_hand_written_keras_checkpoint_imports(tmp_path):
    """a Sequential as Keras 2.2.4 writes it: the up-sampling layer with size as a list and its interpolation key"""
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
    pool = {'class_name': 'MaxPooling2D',
            'config': {'name': 'max_pooling2d_1', 'trainable': True, 'pool_size': [2, 2], 'padding': 'valid', 'strides': [2, 2],
                       'data_format': 'channels_first'}}
    ups = {'class_name': 'UpSampling2D',
           'config': {'name': 'up_sampling2d_1', 'trainable': True, 'size': [2, 2], 'data_format': 'channels_first',
                      'interpolation': 'bilinear'}}
    names = ['conv2d_1', 'max_pooling2d_1', 'up_sampling2d_1', 'conv2d_2']
    config = {'class_name': 'Sequential', 'config': {'name': 'sequential_1', 'layers': [conv('conv2d_1', 8, True), pool, ups,
                                                                                       conv('conv2d_2', 4)]}}
    weights = {'conv2d_1': [(0.3 * rng.standard_normal((3, 3, 4, 8))).astype(np.float32), (0.1 * rng.standard_normal(8)).astype(np.float32)],
               'conv2d_2': [(0.3 * rng.standard_normal((3, 3, 8, 4))).astype(np.float32), (0.1 * rng.standard_normal(4)).astype(np.float32)]}
    root = hdf5_lite.GroupSpec()
    root.attrs['keras_version'] = b'2.2.4'
    root.attrs['backend'] = b'tensorflow'
    root.attrs['model_config'] = json.dumps(config).encode('utf-8')
    mw = root.create_group('model_weights')
    mw.attrs['layer_names'] = np.array([n.encode() for n in names])
    for name in names:
        g = mw.create_group(name)
        if name in weights:
            g.attrs['weight_names'] = np.array([('%s/kernel:0' % name).encode(), ('%s/bias:0' % name).encode()])
            g.create_dataset('%s/kernel:0' % name, weights[name][0])
            g.create_dataset('%s/bias:0' % name, weights[name][1])
    path = str(tmp_path / 'bilinear.h5')
    hdf5_lite.write_file(path, root)
    m = serialization.import_keras_hdf5(path)
    assert [type(lay).__name__ for lay in m.layers if not isinstance(lay, L.InputLayer)] == \
        ['Conv2D', 'MaxPooling2D', 'UpSampling2D', 'Conv2D']
    assert [op.kind for op in m.infer_plan.ops].count('bilinear') == 1 and 'upsample' not in [op.kind for op in m.infer_plan.ops]
    x, _ = _data(cs, 22)
    k1, b1, k2, b2 = [torch.tensor(a.astype(np.float64)) for a in weights['conv2d_1'] + weights['conv2d_2']]
    t = torch.tanh(F.conv2d(torch.tensor(x, dtype=torch.float64), k1.permute(3, 2, 0, 1), b1, padding=1))
    want = F.conv2d(bilinear_ref(F.max_pool2d(t, 2)), k2.permute(3, 2, 0, 1), b2, padding=1).numpy()
    got = m.predict(x)
    assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()


def test_bfloat16_activation_storage():
    """conv -> bilinear UpSampling2D -> conv on a pooled source at 16 x 24 (so that the output has the input's shape and the model
    can be rolled out): the convolution's output and its interpolated image are stored as bfloat16; the bounds are those of
    tests/test_gpu_configs.py for the project's bf16 mode, against the float64 reference of the float32 mode"""
    from dlwp_amd.engine import Model
    from dlwp_amd.model import DLWPFunctional
    cs = (4, 16, 24)
    x0 = L.Input(shape=cs)
    t = L.Conv2D(16, 3, activation='tanh', **CF)(_pads(L.MaxPooling2D(2, **CF)(x0)))
    t = L.UpSampling2D(2, interpolation='bilinear', **CF)(t)
    m = Model(inputs=x0, outputs=L.Conv2D(cs[0], 3, **CF)(_pads(t)), seed=9)
    _randomise(m, np.random.default_rng(31))
    x, _ = _data(cs, 32, n=5)
    p = _ref_params(m, requires_grad=False)
    convs = [lay for lay in m.layers if isinstance(lay, L.Conv2D)]
    with torch.no_grad():
        t64 = _conv_ref(F.max_pool2d(torch.tensor(x, dtype=torch.float64), 2), convs[0], p)
        want = _conv_ref(bilinear_ref(t64), convs[1], p).numpy()
    got32 = m.predict(x)
    assert np.abs(got32 - want).max() <= FWD_TOL * np.abs(want).max()
    m.set_activation_dtype('bfloat16')
    ups = [op for op in m.infer_plan.ops if op.kind == 'bilinear']
    assert len(ups) == 1
    bufs = m.executor.scratch(5)
    assert bufs[ups[0].src].dtype == torch.bfloat16 and bufs[ups[0].dst].dtype == torch.bfloat16
    assert {ups[0].src, ups[0].dst} <= set(m.infer_plan.bf16_buffers())
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
