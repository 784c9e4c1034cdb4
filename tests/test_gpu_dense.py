"""Dense / Flatten / Dropout on the GPU (csrc/dense.hip): the kernels against the float64 restatement, bit reproducibility and
batch independence, the Dropout mask against its numpy restatement, training steps against float64 autograd, the recorded step, the
wrapper end to end with a StandardScaler, the captured rollout, two ranks, model files."""
import math
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd import ops
from dlwp_amd.regularizers import l2
from oracle import torch_ref
from tests.test_dense_cpu import (conv_dense_layers, feed_forward_layers, np_dense_backward, np_dense_forward, np_dropout_apply,
                                  np_dropout_mask)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # the project's FWD_TOL / CONV_RTOL: max |got - want| <= TOL * max |want|


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _close(got, want, what, tol=TOL):
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('%s: error %.3g of scale %.3g (%.3g relative)' % (what, err, scale, err / scale))
    assert err <= tol * scale, '%s: error %.3g of scale %.3g' % (what, err, scale)


def _off(a, off):
    """a device copy of `a` that starts `off` floats behind a 16-byte boundary"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device='cuda')
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    assert t.data_ptr() % 16 == 4 * (off % 4)
    return t


def _case(m, k, n, seed):
    rng = np.random.default_rng(seed)
    limit = math.sqrt(6.0 / (k + n))
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = rng.uniform(-limit, limit, (k, n)).astype(np.float32)
    b = (0.1 * rng.standard_normal(n)).astype(np.float32)
    dy = rng.standard_normal((m, n)).astype(np.float32)
    return x, w, b, dy


def _run_kernels(x, w, b, dy, act, offs=(0, 0, 0, 0)):
    xd, wd, dyd = _off(x, offs[0]), _off(w, offs[1]), _off(dy, offs[2])
    bd = _off(b, offs[3]) if b is not None else None
    y = ops.dense_fwd(xd, wd, bd, act)
    dx = ops.dense_bwd_data(dyd, y, wd, act)
    dw = torch.full(w.shape, float('nan'), device='cuda')
    db = torch.full((w.shape[1],), float('nan'), device='cuda') if b is not None else None
    ops.dense_bwd_weight(xd, dyd, y, dw, db, act)
    return [_host(t) if t is not None else None for t in (y, dx, dw, db)]


def _check_kernels(m, k, n, act, bias, seed, offs=(0, 0, 0, 0)):
    x, w, b, dy = _case(m, k, n, seed)
    if not bias:
        b = None
    y, dx, dw, db = _run_kernels(x, w, b, dy, act, offs)
    want_y = np_dense_forward(x, w, b, act)
    tag = '(m %d, k %d, n %d, %s, bias %s, offsets %r)' % (m, k, n, act, bias, offs)
    _close(y, want_y, 'forward ' + tag)
    # the gradients' restatement takes the kernel's own y (float32): the backward is defined on the stored activation
    want_dx, want_dw, want_db = np_dense_backward(x, w, y, dy, act)
    _close(dx, want_dx, 'data gradient ' + tag)
    _close(dw, want_dw, 'weight gradient ' + tag)
    if bias:
        _close(db, want_db, 'bias gradient ' + tag)


# every M, K and N of the issue at least once with each activation; ragged against every tile edge (32 / 64 / 128)
KERNEL_CASES = [(m, k, n, act, bias)
                for i, (m, k, n) in enumerate([(1, 7, 1), (3, 50, 5), (64, 192, 96), (100, 1037, 1030), (256, 192, 1030),
                                               (1, 1037, 96), (3, 7, 1030), (64, 50, 1), (100, 192, 5), (256, 1037, 96),
                                               (64, 1037, 1030), (256, 7, 5)])
                for act, bias in ((('linear', True), ('tanh', True), ('relu', False)) if i % 2 == 0 else
                                  (('linear', False), ('tanh', False), ('relu', True)))]


@pytest.mark.parametrize('m, k, n, act, bias', KERNEL_CASES)
def test_kernels_against_float64(m, k, n, act, bias):
    _check_kernels(m, k, n, act, bias, seed=m * 7 + k * 3 + n)


@pytest.mark.parametrize('offs', [(1, 1, 1, 1), (3, 2, 1, 0), (0, 3, 0, 2), (2, 0, 3, 1)])
def test_kernels_on_tensors_off_16_byte_boundaries(offs):
    for act in ('linear', 'tanh', 'relu'):
        _check_kernels(100, 192, 96, act, True, seed=11, offs=offs)     # (k and n multiples of 4: the float4 path is at stake)
        _check_kernels(3, 50, 1030, act, True, seed=12, offs=offs)


def test_full_size_layer_against_float64():
    """the reference's own layer 1: 64 x 20 736 -> 10 368 (860 MB of weights)"""
    m, k, n = 64, 20736, 10368
    x, w, b, dy = _case(m, k, n, 5)
    xd, wd, bd, dyd = _dev(x), _dev(w), _dev(b), _dev(dy)
    y = ops.dense_fwd(xd, wd, bd, 'tanh')
    yh = _host(y)
    _close(yh, np_dense_forward(x, w, b, 'tanh'), 'full-size forward')
    zl = _host(ops.dense_fwd(xd, wd, bd, None))
    _close(zl, np_dense_forward(x, w, b, None), 'full-size forward, linear')
    g = dy.astype(np.float64) * (1.0 - yh.astype(np.float64) ** 2)
    dx = _host(ops.dense_bwd_data(dyd, y, wd, 'tanh'))
    _close(dx, g @ w.astype(np.float64).T, 'full-size data gradient')
    del dx
    dw = torch.empty((k, n), device='cuda')
    db = torch.empty(n, device='cuda')
    ops.dense_bwd_weight(xd, dyd, y, dw, db, 'tanh')
    _close(_host(db), g.sum(axis=0), 'full-size bias gradient')
    rows = np.array([0, 1, 31, 32, 4097, 20735])
    _close(_host(dw[torch.from_numpy(rows).cuda()]), x.astype(np.float64).T[rows] @ g, 'full-size weight gradient (6 rows)')
    cols = np.array([0, 33, 10367])
    _close(_host(dw[:, torch.from_numpy(cols).cuda()]), x.astype(np.float64).T @ g[:, cols], 'full-size weight gradient (3 columns)')


def test_two_runs_give_the_same_bits_and_a_row_does_not_depend_on_its_batch():
    k, n = 1037, 1030
    x, w, b, dy = _case(256, k, n, 21)
    wd, bd = _dev(w), _dev(b)
    for act in ('tanh', 'linear'):
        runs = {}
        for m in (256, 64, 1):
            xd, dyd = _dev(x[:m]), _dev(dy[:m])
            y = ops.dense_fwd(xd, wd, bd, act)
            y2 = ops.dense_fwd(xd, wd, bd, act)
            yfull = _dev(np_dense_forward(x, w, b, act)[:m])            # (one y for every batch: dx must not depend on the batch)
            dx = ops.dense_bwd_data(dyd, yfull, wd, act)
            dx2 = ops.dense_bwd_data(dyd, yfull, wd, act)
            dw, dw2 = torch.empty((k, n), device='cuda'), torch.empty((k, n), device='cuda')
            db, db2 = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
            ops.dense_bwd_weight(xd, dyd, y, dw, db, act)
            ops.dense_bwd_weight(xd, dyd, y, dw2, db2, act)
            for a, c in ((y, y2), (dx, dx2), (dw, dw2), (db, db2)):
                assert np.array_equal(_bits(_host(a)), _bits(_host(c))), (act, m)
            runs[m] = (_host(y), _host(dx))
        for i in (0, 1):
            assert np.array_equal(_bits(runs[256][i][:64]), _bits(runs[64][i])), (act, i)
            assert np.array_equal(_bits(runs[256][i][:1]), _bits(runs[1][i])), (act, i)
        # row 200 of 256 alone
        y1 = _host(ops.dense_fwd(_dev(x[200:201]), wd, bd, act))
        assert np.array_equal(_bits(y1), _bits(runs[256][0][200:201]))


# ----------------------------------------------------------------------------------------------------------------------- #
# Dropout
# ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('n, off', [(1 << 20, 0), (4099, 0), (4099, 1), (3, 2), (1 << 20, 3)])
def test_dropout_mask_equals_the_numpy_restatement(n, off):
    rng = np.random.default_rng(n + off)
    x = (rng.standard_normal(n) + 3.0).astype(np.float32)              # (no zeros: the mask can be read off the output)
    for rate, seed, layer, step in ((0.25, 1234, 0, 7), (0.5, (1 << 40) + 17, 3, 1 << 20)):
        xd = _off(x, off)
        y = _host(ops.dropout_fwd(xd, rate, seed, layer, step))
        want = np_dropout_apply(x, rate, seed, layer, step)
        assert np.array_equal(_bits(y), _bits(want)), (rate, seed, layer, step)
        keep, _ = np_dropout_mask(n, rate, seed, layer, step)
        assert np.array_equal(y != 0, keep)
        if n >= 1 << 20:
            sd = math.sqrt(rate * (1 - rate) / n)
            assert abs(float((y != 0).mean()) - (1 - rate)) < 4 * sd
        dy = rng.standard_normal(n).astype(np.float32)
        dx = _host(ops.dropout_bwd(_off(dy, off), rate, seed, layer, step))       # the backward uses the forward's mask
        assert np.array_equal(_bits(dx), _bits(np_dropout_apply(dy, rate, seed, layer, step)))
        again = _host(ops.dropout_fwd(xd, rate, seed, layer, step))
        assert np.array_equal(_bits(again), _bits(y))
        assert not np.array_equal(_host(ops.dropout_fwd(xd, rate, seed, layer, step + 1)) != 0, keep) or n < 16
    assert np.array_equal(_bits(_host(ops.dropout_fwd(_off(x, off), 0.0, 1, 0, 0))), _bits(x))


# ----------------------------------------------------------------------------------------------------------------------- #
# training steps against float64 autograd
# ----------------------------------------------------------------------------------------------------------------------- #
def _build(specs, seed=0, lr=1e-3, loss='mse', conv=False, **kw):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    np.random.seed(seed)
    d = DLWPNeuralNet(is_convolutional=conv, is_recurrent=False, time_dim=2, scaler_type=kw.pop('scaler_type', None),
                      scale_targets=kw.pop('scale_targets', False))
    d.build_model(specs, loss=loss, optimizer=Adam(lr=lr), metrics=['mae'], **kw)
    return d


def _randomise_biases(model, rng):
    for lay in model.layers:
        if isinstance(lay, (L.Dense, L.Conv2D)) and lay.bias is not None:
            k, b = lay.get_weights()
            lay.set_weights([k, (0.1 * rng.standard_normal(b.shape)).astype(np.float32)])


def _ref_params(model):
    return {(lay.name, nm): torch.tensor(a.astype(np.float64), requires_grad=True)
            for lay in model.layers for (nm, _), a in zip(lay._weights, lay.get_weights())}


def _ref_forward(model, x, p, step=None):
    """float64 torch restatement of the layer stack; step: the training step whose Dropout masks apply (None: inference)"""
    t = x
    n_drop = 0
    for lay in model.layers:
        if isinstance(lay, L.Conv2D):
            wk = p[(lay.name, 'kernel')].permute(3, 2, 0, 1)
            t = torch.nn.functional.conv2d(t, wk, p[(lay.name, 'bias')], padding='same')
            t = torch.tanh(t) if lay.activation == 'tanh' else t
        elif isinstance(lay, L.Flatten):
            t = t.reshape(t.shape[0], -1)
        elif isinstance(lay, L.Reshape):
            t = t.reshape((t.shape[0],) + tuple(lay.target_shape))
        elif isinstance(lay, L.Dense):
            t = t @ p[(lay.name, 'kernel')]
            if lay.bias is not None:
                t = t + p[(lay.name, 'bias')]
            t = torch.tanh(t) if lay.activation == 'tanh' else (torch.relu(t) if lay.activation == 'relu' else t)
        elif isinstance(lay, L.Dropout):
            if step is not None:
                keep, scale = np_dropout_mask(t.numel(), lay.rate, lay.mask_seed, n_drop, step)
                t = t * torch.tensor(keep.reshape(tuple(t.shape)).astype(np.float64) * float(scale))
            n_drop += 1
        else:
            raise AssertionError(type(lay))
    return t


def _ref_loss(model, out, y, p, loss):
    d = out - torch.tensor(y, dtype=torch.float64).reshape(out.shape)
    val = (d ** 2).mean() if loss == 'mse' else d.abs().mean()
    for lay in model.layers:
        reg = getattr(lay, 'kernel_regularizer', None)
        if reg is not None:
            val = val + reg.l2 * (p[(lay.name, 'kernel')] ** 2).sum()
    return val


def _grads_of(trainer):
    g = trainer.flat_grads.cpu().numpy()
    return {(lay.name, nm): g[off:off + numel].reshape(shape) for lay, nm, off, numel, shape in trainer.entries}


@pytest.mark.parametrize('loss', ['mse', 'mae'])
@pytest.mark.parametrize('reg', [0.0, 1e-3])
def test_feed_forward_training_step_against_float64_autograd(monkeypatch, loss, reg):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    f, n = 192, 64
    d = _build(feed_forward_layers(f, reg=reg, seed=77), seed=3, loss=loss)
    rng = np.random.default_rng(31)
    _randomise_biases(d.model, rng)
    x = rng.standard_normal((n, f)).astype(np.float32)
    y = rng.standard_normal((n, f)).astype(np.float32)
    p = _ref_params(d.model)
    slots = {k: (torch.zeros_like(t), torch.zeros_like(t)) for k, t in p.items()}
    for it in range(4):                      # the first step's gradients, then three more Adam steps
        logs = d.model.train_on_batch(x, y)
        torch.cuda.synchronize()
        for t in p.values():
            t.grad = None
        val = _ref_loss(d.model, _ref_forward(d.model, torch.tensor(x, dtype=torch.float64), p, step=it), y, p, loss)
        val.backward()
        assert logs[0] == pytest.approx(float(val.detach()), rel=2e-5), it
        if it == 0:
            got = _grads_of(d.model._trainer)
            assert sorted(got) == sorted(p)
            for key, g in got.items():
                ref = p[key].grad.numpy()
                err = np.abs(g - ref).max()
                print(key, 'gradient error %.3g of %.3g' % (err, np.abs(ref).max()))
                assert err <= 3e-4 * max(np.abs(ref).max(), 1e-6), (key, err, np.abs(ref).max())
        with torch.no_grad():
            for key, (m_, v_) in slots.items():
                torch_ref.adam_keras_step(p[key], m_, v_, p[key].grad, it, lr=1e-3, epsilon=1e-7)
    for lay in d.model.layers:
        for (nm, _), a in zip(lay._weights, lay.get_weights()):
            want = p[(lay.name, nm)].detach().numpy()
            assert np.abs(a - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (lay.name, nm)
    # consecutive steps drew different masks; predict is the identity through Dropout
    pred = d.model.predict(x)
    want = _ref_forward(d.model, torch.tensor(x, dtype=torch.float64), _ref_params(d.model)).detach().numpy()
    _close(pred, want, 'predict through Dropout')


def test_the_same_seed_gives_the_same_run_twice_and_steps_differ(monkeypatch):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16, 48)).astype(np.float32)
    y = rng.standard_normal((16, 48)).astype(np.float32)
    runs = []
    for seed in (9, 9, 10):
        d = _build(feed_forward_layers(48, reg=0.0, seed=seed), seed=1)
        logs = [d.model.train_on_batch(x, y)[0] for _ in range(3)]
        ex = d.model.train_executor
        drop = [k for k, op in enumerate(d.model.plan.ops) if op.kind == 'dropout'][0]
        kept = _host(ex.scratch(16)[d.model.plan.ops[drop].dst]) != 0
        runs.append((logs, d.model.get_weights(), kept))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert runs[0][0][1:] != runs[2][0][1:] or not np.array_equal(runs[0][2], runs[2][2])
    assert not np.array_equal(runs[0][2], runs[2][2])
    want, _ = np_dropout_mask(16 * 24, 0.25, 9, 0, 2)                    # the third step's mask (step = optimizer iteration 2)
    assert np.array_equal(runs[0][2].reshape(-1), want)


def test_conv_front_dense_head_step_and_predict(monkeypatch):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    c, h, w, n = 2, 8, 12, 8
    d = _build(conv_dense_layers(c, h, w), seed=2, conv=True)
    rng = np.random.default_rng(8)
    _randomise_biases(d.model, rng)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    y = rng.standard_normal((n, c, h, w)).astype(np.float32)
    p = _ref_params(d.model)
    pred = d.model.predict(x)
    assert pred.shape == (n, c, h, w)
    _close(pred, _ref_forward(d.model, torch.tensor(x, dtype=torch.float64), p).detach().numpy(), 'conv front + dense head predict')
    logs = d.model.train_on_batch(x, y)
    torch.cuda.synchronize()
    val = _ref_loss(d.model, _ref_forward(d.model, torch.tensor(x, dtype=torch.float64), p, step=0), y, p, 'mse')
    val.backward()
    assert logs[0] == pytest.approx(float(val.detach()), rel=2e-5)
    for key, g in _grads_of(d.model._trainer).items():
        ref = p[key].grad.numpy()
        assert np.abs(g - ref).max() <= 3e-4 * max(np.abs(ref).max(), 1e-6), (key, np.abs(g - ref).max(), np.abs(ref).max())


# ----------------------------------------------------------------------------------------------------------------------- #
# the recorded / replayed step
# ----------------------------------------------------------------------------------------------------------------------- #
def _run_steps(monkeypatch, n, form, batches, specs):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)
    d = _build(specs, seed=5)
    _randomise_biases(d.model, np.random.default_rng(50))
    logs = [d.model.train_on_batch(x, y) for x, y in batches]
    torch.cuda.synchronize()
    tr = d.model._trainer
    if form != 'eager':
        ents = [e for k, e in tr._graphs.items() if k[0] == n and e.get('step') is not None]
        assert len(ents) == 1, 'the step of %d samples was not recorded (refused: %r)' % (n, tr._no_tape)
    return logs, [w.copy() for w in d.model.get_weights()], [s.cpu().numpy() for s in tr.opt_state]


def test_replayed_step_equals_the_eager_step(monkeypatch):
    f, n = 192, 64
    specs = feed_forward_layers(f, reg=0.0)[::2]          # Dense -> Dense: what _graph_ok replays (no Dropout, no regulariser)
    rng = np.random.default_rng(600)
    batches = [(rng.standard_normal((n, f)).astype(np.float32), rng.standard_normal((n, f)).astype(np.float32)) for _ in range(5)]
    ref = _run_steps(monkeypatch, n, 'eager', batches, specs)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, n, form, batches, specs)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
            assert np.array_equal(_bits(a), _bits(b)), form


def test_models_with_dropout_or_a_regulariser_stay_on_the_eager_step():
    d = _build(feed_forward_layers(48, reg=0.0))
    assert d.model._trainer._graph_ok(16) is False
    d = _build(feed_forward_layers(48, reg=0.0)[::2])
    assert d.model._trainer._graph_ok(16) in ('graph', 'lanes')


# ----------------------------------------------------------------------------------------------------------------------- #
# the wrapper end to end
# ----------------------------------------------------------------------------------------------------------------------- #
def _series(n, shape, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n,) + shape).astype(np.float32)
    base = (base * rng.uniform(0.5, 4.0, (1,) + shape) + rng.uniform(-10, 10, (1,) + shape)).astype(np.float32)
    return base, (0.8 * base + 1.0).astype(np.float32)


def test_wrapper_with_standard_scaler_end_to_end():
    from dlwp_amd.model import DataGenerator
    from dlwp_amd.model.generators import ArrayDataset
    shape = (2, 2, 4, 6)                        # (time_step, variable, lat, lon): n_features = 96
    f = int(np.prod(shape))
    p, t = _series(96, shape, 3)
    d = _build(feed_forward_layers(f, reg=1e-4, seed=4), seed=6, lr=2e-3, scaler_type='StandardScaler', scale_targets=True)
    assert d.is_convolutional is False
    gen = DataGenerator(d, ArrayDataset(p.reshape((96, 2, 2, 4, 6)), t.reshape((96, 2, 2, 4, 6))), batch_size=32)
    assert gen.dense_shape == (f,)
    xa, ya = gen.generate([], scale_and_impute=False)
    assert xa.shape == (96, f)
    with pytest.raises(AttributeError):
        d.fit_generator(gen, epochs=1, verbose=0)
    d.init_fit(xa, ya)
    h = d.fit_generator(gen, epochs=6, verbose=0)
    assert h.history['loss'][-1] < h.history['loss'][0]
    h2 = d.fit(xa, ya, initialize=False, batch_size=32, epochs=2, verbose=0)
    assert all(np.isfinite(h2.history['loss']))
    # predict = scaler -> restatement -> inverse scaler
    pr = _ref_params(d.model)

    def ref_predict(a):
        z = d.scaler.transform(a.reshape(a.shape[0], -1))
        out = _ref_forward(d.model, torch.tensor(z, dtype=torch.float64), pr).detach().numpy()
        return d.scaler_y.inverse_transform(out)
    pred = d.predict(xa)
    assert pred.shape == (96, f)
    _close(pred, ref_predict(xa), 'wrapper predict', tol=2e-5)          # (two float32 scaler passes on top of the kernels)
    ev = d.evaluate(xa, ya, verbose=0)
    assert np.isfinite(ev[0])
    # predict_timeseries: the reference's loop (models.py:247-301) restated on the host
    steps = 6
    series = d.predict_timeseries(xa[:5], steps)
    assert series.shape == (steps, 5, f // 2) and series.dtype == np.float32
    state = xa[:5].astype(np.float64)
    want = []
    for _ in range(steps // 2):
        state = ref_predict(state)
        want.append(state.reshape(5, 2, -1))
    want = np.stack(want).transpose(0, 2, 1, 3).reshape(steps, 5, -1)
    _close(series[:4], want[:4], 'predict_timeseries, first two calls', tol=1e-4)
    kept = d.predict_timeseries(xa[:5], steps, keep_time_dim=True)
    assert kept.shape == (steps // 2, 5, 2, f // 2)


def test_captured_rollout_equals_the_host_loop():
    f = 96
    d = _build(feed_forward_layers(f, reg=0.0), seed=8)
    _randomise_biases(d.model, np.random.default_rng(2))
    x = np.random.default_rng(3).standard_normal((7, f)).astype(np.float32)
    assert d._device_rollout_ok(x)
    got = d.predict_timeseries(x, 6)
    kept = d.predict_timeseries(x, 6, keep_time_dim=True)
    state, want = x, []
    for _ in range(3):
        state = d.model.predict(state)
        want.append(state)
    want = np.stack(want)
    assert np.array_equal(_bits(kept), _bits(want.reshape(3, 7, 2, f // 2)))
    assert np.array_equal(_bits(got), _bits(want.reshape(3, 7, 2, f // 2).transpose(0, 2, 1, 3).reshape(6, 7, f // 2)))


# ----------------------------------------------------------------------------------------------------------------------- #
# two ranks
# ----------------------------------------------------------------------------------------------------------------------- #
def _dp_specs():
    return feed_forward_layers(96, reg=0.0)[::2]


def _dp_data():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((64, 96)).astype(np.float32)
    return x, (0.5 * x + 0.1 * rng.standard_normal(x.shape)).astype(np.float32)


def _dp_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DLWP_SHARE_GPUS='1', DLWP_DIST_BACKEND='gloo')
    from dlwp_amd import parallel
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    parallel.init()
    np.random.seed(1000 + 17 * rank)
    d = DLWPNeuralNet(is_convolutional=False, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(_dp_specs(), loss='mse', optimizer=Adam(lr=1e-3), gpus=world)
    w0 = [w.copy() for w in d.model.get_weights()]
    x, y = _dp_data()
    logs = [d.model.train_on_batch(x, y) for _ in range(3)]
    torch.cuda.synchronize()
    ret[rank] = {'w0': w0, 'w1': d.model.get_weights(), 'logs': logs}
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_step_equals_the_single_process_step_on_the_whole_batch():
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    from tests.test_gpu_parallel import _free_port
    ctx = mp.get_context('spawn')
    port = _free_port()
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, ret)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            if p.is_alive():
                p.kill()
                pytest.fail('data-parallel worker timed out')
            assert p.exitcode == 0, 'data-parallel worker failed'
        res = dict(ret)
    assert res[0]['logs'] == res[1]['logs']
    for a, b in zip(res[0]['w1'], res[1]['w1']):
        assert np.array_equal(a, b)
    d = DLWPNeuralNet(is_convolutional=False, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(_dp_specs(), loss='mse', optimizer=Adam(lr=1e-3))
    d.model.set_weights(res[0]['w0'])
    x, y = _dp_data()
    logs = [d.model.train_on_batch(x, y) for _ in range(3)]
    for got, want in zip(res[0]['logs'], logs):
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (got, want)
    for a, b in zip(res[0]['w1'], d.model.get_weights()):
        assert np.abs(a - b).max() <= 1e-6 * 3, np.abs(a - b).max()


def test_parallel_build_with_dropout_is_refused():
    from dlwp_amd.model import DLWPNeuralNet
    d = DLWPNeuralNet(is_convolutional=False, scaler_type=None, scale_targets=False)
    with pytest.raises(NotImplementedError, match='Dropout'):
        d.build_model(feed_forward_layers(48), loss='mse', gpus=2)


# ----------------------------------------------------------------------------------------------------------------------- #
# model files
# ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('fmt', ['keras', 'npz'])
def test_saved_and_reloaded_training_continues_bit_identically(tmp_path, monkeypatch, fmt):
    from dlwp_amd import serialization
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    f = 48
    rng = np.random.default_rng(12)
    batches = [(rng.standard_normal((16, f)).astype(np.float32), rng.standard_normal((16, f)).astype(np.float32)) for _ in range(5)]
    specs = feed_forward_layers(f, reg=1e-3)               # (no seed given: the one the model drew is what the file must carry)
    d = _build(specs, seed=2)
    w0 = d.model.get_weights()
    full = [d.model.train_on_batch(x, y) for x, y in batches]
    want = d.model.get_weights()
    seed = d.model.layers[1].mask_seed
    d = _build(specs, seed=2)
    assert d.model.layers[1].mask_seed == seed
    d.model.set_weights(w0)
    first = [d.model.train_on_batch(x, y) for x, y in batches[:3]]
    path = str(tmp_path / ('m.' + fmt))
    d.model.save(path, format=fmt)
    m2 = serialization.load_model_file(path)
    assert [type(lay).__name__ for lay in m2.layers if not isinstance(lay, L.InputLayer)] == ['Dense', 'Dropout', 'Dense']
    assert m2.layers[-2].mask_seed == seed and m2.layers[-3].kernel_regularizer.l2 == pytest.approx(1e-3)
    for a, b in zip(m2.get_weights(), d.model.get_weights()):
        assert np.array_equal(_bits(a), _bits(b))
    rest = [m2.train_on_batch(x, y) for x, y in batches[3:]]
    assert m2.optimizer.iterations == 5
    for a, b in zip(first + rest, full):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
    for a, b in zip(m2.get_weights(), want):
        assert np.array_equal(_bits(a), _bits(b))
