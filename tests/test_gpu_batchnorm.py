"""BatchNormalization(axis=1) on the GPU (csrc/batchnorm.hip through every layer): the kernels against float64, deterministic bits
and the moving-statistics recursion; the reference U-Net with its five commented-out BatchNormalization lines switched on
(examples/train.py:170-210) -- one training step against torch autograd in float64, three Adam steps, the recorded / replayed
step against the eager one, inference with the moving statistics (predict, evaluate, the hipGraph rollout, the fed rollout of
TimeSeriesEstimator), a functional skip-connection U-Net, model files; and the errors of what is out of scope."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from dlwp_amd import ops
from oracle import torch_ref
from tests.test_batchnorm_cpu import bn_layers, np_bn_backward, np_bn_forward

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
MOM, EPS = 0.99, 1e-3


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


# ----------------------------------------------------------------------------------------------------------------------- #
# kernels
# ----------------------------------------------------------------------------------------------------------------------- #
SHAPES = [(1, 1, 7, 9), (2, 3, 5, 7), (64, 1, 3, 5), (2, 32, 9, 11), (64, 32, 22, 45), (2, 128, 11, 13), (1, 128, 88, 180),
          (64, 3, 88, 180), (8, 32, 88, 180)]


class _Kern(object):
    def __init__(self, n, c, h, w, seed):
        rng = np.random.default_rng(seed)
        self.x = (rng.standard_normal((n, c, h, w)) * rng.uniform(0.5, 3.0, (1, c, 1, 1)) + rng.uniform(-20, 20, (1, c, 1, 1)))
        self.dy = rng.standard_normal((n, c, h, w))
        self.gamma, self.beta = rng.uniform(0.5, 2.0, c), rng.standard_normal(c)
        self.mm, self.mv = rng.standard_normal(c), rng.uniform(0.5, 2.0, c)
        self.x32 = self.x.astype(np.float32)
        self.dy32 = self.dy.astype(np.float32)
        d = ops.batchnorm_desc(torch.empty((n, c, h, w)))
        self.ws = torch.zeros(ops.batchnorm_workspace_bytes(d), dtype=torch.uint8, device='cuda')

    def run(self):
        c = self.x.shape[1]
        x = _dev(self.x32)
        g, b, mm, mv = _dev(self.gamma), _dev(self.beta), _dev(self.mm), _dev(self.mv)
        sm = torch.zeros(c, device='cuda')
        si = torch.zeros(c, device='cuda')
        y = ops.batchnorm_fwd_train(x, g, b, mm, mv, sm, si, self.ws, MOM, EPS)
        dg, db = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
        dx = ops.batchnorm_bwd(x, _dev(self.dy32), g, sm, si, self.ws, dgamma=dg, dbeta=db)
        yi = ops.batchnorm_fwd_infer(x, g, b, mm, mv, EPS)
        return [_host(t) for t in (y, sm, si, mm, mv, dx, dg, db, yi)]


def _close(got, want, what, tol=1e-5):
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= tol * scale, '%s: error %.3g of scale %.3g' % (what, err, scale)


@pytest.mark.parametrize('shape', SHAPES)
def test_kernels_against_float64(shape):
    k = _Kern(*shape, seed=sum(shape))
    y, sm, si, mm, mv, dx, dg, db, yi = k.run()
    x = k.x32.astype(np.float64)
    y_ref, mean, invstd, mm_ref, mv_ref = np_bn_forward(x, k.gamma.astype(np.float32).astype(np.float64),
                                                        k.beta.astype(np.float32).astype(np.float64),
                                                        k.mm.astype(np.float32).astype(np.float64),
                                                        k.mv.astype(np.float32).astype(np.float64), MOM, EPS)
    _close(y, y_ref, 'y %r' % (shape,))
    _close(sm, mean, 'mean')
    _close(si, invstd, 'invstd')
    _close(mm, mm_ref, 'moving mean')
    _close(mv, mv_ref, 'moving variance')
    g64 = k.gamma.astype(np.float32).astype(np.float64)
    dx_ref, dg_ref, db_ref = np_bn_backward(x, k.dy32.astype(np.float64), g64, mean, invstd)
    _close(dx, dx_ref, 'dx %r' % (shape,))
    _close(dg, dg_ref, 'dgamma')
    _close(db, db_ref, 'dbeta')
    # inference: the UPDATED moving statistics (the forward above ran first)
    yi_ref = g64[None, :, None, None] * (x - mm_ref[None, :, None, None]) / np.sqrt(mv_ref[None, :, None, None] + EPS) + \
        k.beta.astype(np.float32)[None, :, None, None]
    _close(yi, yi_ref, 'inference y')
    # two runs: the same bits
    again = k.run()
    for a, b in zip(again, (y, sm, si, mm, mv, dx, dg, db, yi)):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize('off_x, off_y', [(1, 1), (3, 3), (1, 2), (0, 3)])
def test_kernels_on_tensors_off_16_byte_boundaries(off_x, off_y):
    """views that start inside a 16-byte unit (a sliced device batch, a member group of a rollout): the same values"""
    n, c, h, w = 3, 5, 9, 13
    k = _Kern(n, c, h, w, seed=77)
    want = k.run()

    def view(a, off):
        buf = torch.zeros(a.size + 8, device='cuda')
        t = buf[off:off + a.size].view(a.shape)
        t.copy_(_dev(a))
        return t
    x, dy = view(k.x32, off_x), view(k.dy32, off_y)
    y, dx = view(np.zeros_like(k.x32), off_y), view(np.zeros_like(k.x32), off_x)
    g, b, mm, mv = _dev(k.gamma), _dev(k.beta), _dev(k.mm), _dev(k.mv)
    sm, si, dg, db = (torch.zeros(c, device='cuda') for _ in range(4))
    ops.batchnorm_fwd_train(x, g, b, mm, mv, sm, si, k.ws, MOM, EPS, out=y)
    ops.batchnorm_bwd(x, dy, g, sm, si, k.ws, dgamma=dg, dbeta=db, dx=dx)
    for got, ref in zip((y, sm, si, mm, mv, dx, dg, db), want[:8]):
        _close(_host(got), ref.astype(np.float64), 'offsets %d / %d' % (off_x, off_y), tol=2e-6)


def test_moving_statistics_follow_the_recursion():
    rng = np.random.default_rng(5)
    n, c, h, w = 4, 6, 22, 45
    mm, mv = np.zeros(c), np.ones(c)
    mm_d, mv_d = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    g, b = torch.ones(c, device='cuda'), torch.zeros(c, device='cuda')
    ws = torch.zeros(ops.batchnorm_workspace_bytes(ops.batchnorm_desc(torch.empty(n, c, h, w))), dtype=torch.uint8, device='cuda')
    sm, si = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
    for step in range(5):
        x = (rng.standard_normal((n, c, h, w)) * (1 + step) + step).astype(np.float32)
        ops.batchnorm_fwd_train(_dev(x), g, b, mm_d, mv_d, sm, si, ws, 0.9, 1e-5)
        _, _, _, mm, mv = np_bn_forward(x.astype(np.float64), np.ones(c), np.zeros(c), mm, mv, 0.9, 1e-5)
        _close(_host(mm_d), mm, 'moving mean, step %d' % step)
        _close(_host(mv_d), mv, 'moving variance, step %d' % step)


# ----------------------------------------------------------------------------------------------------------------------- #
# models: the float64 reference (oracle/torch_ref.py between the normalisations, F.batch_norm at them)
# ----------------------------------------------------------------------------------------------------------------------- #
def _build(specs, seed=0, lr=1e-3):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    np.random.seed(seed)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(specs, loss='mse', optimizer=Adam(lr=lr), metrics=['mae'])
    return d


def _randomise(model, rng):
    """biases and every BatchNormalization weight drawn at random, so that all of them are tested"""
    for lay in model.layers:
        if isinstance(lay, L.Conv2D):
            k, b = lay.get_weights()
            lay.set_weights([k, (0.1 * rng.standard_normal(b.shape)).astype(np.float32)])
        elif isinstance(lay, L.BatchNormalization):
            c = lay.moving_mean.shape[0]
            lay.set_weights([rng.uniform(0.5, 1.5, c).astype(np.float32), (0.1 * rng.standard_normal(c)).astype(np.float32),
                             (0.1 * rng.standard_normal(c)).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)])


def _ref_params(model, requires_grad=True):
    """{(layer, weight name): float64 torch tensor}; conv kernels in OIHW"""
    out = {}
    for lay in model.layers:
        for (nm, _), a in zip(lay._weights, lay.get_weights()):
            a = a.astype(np.float64)
            if nm == 'kernel':
                a = np.ascontiguousarray(a.transpose(3, 2, 0, 1))
            trainable = nm not in getattr(lay, 'non_trainable_names', ())
            out[(lay.name, nm)] = torch.tensor(a, requires_grad=requires_grad and trainable)
    return out


def _ref_forward(model, specs, x, p, training):
    seg, segw = [], []
    for lay, spec in zip(model.layers, specs):
        if isinstance(lay, L.BatchNormalization):
            x = torch_ref.run_layers(seg, x, segw) if seg else x
            seg, segw = [], []
            x = F.batch_norm(x, p[(lay.name, 'moving_mean')], p[(lay.name, 'moving_variance')], p[(lay.name, 'gamma')],
                             p[(lay.name, 'beta')], training=training, momentum=1 - MOM, eps=EPS)
            continue
        seg.append(spec)
        if isinstance(lay, L.Conv2D):
            segw.append((p[(lay.name, 'kernel')], p[(lay.name, 'bias')]))
    return torch_ref.run_layers(seg, x, segw) if seg else x


def _grads_of(trainer):
    g = trainer.flat_grads.cpu().numpy()
    return {(lay.name, nm): g[off:off + numel].reshape(shape) for lay, nm, off, numel, shape in trainer.entries}


def _check_step(d, specs, x, y, p, tol=3e-4, first_kernel_tol=None):
    """one train_on_batch against float64 autograd: loss, every gradient, the moving statistics.  first_kernel_tol: the bound of
    the first layer's kernel gradient.  That layer reads the 4-channel model input; its weight gradient is a sum over every
    position of the batch, and at 64 samples of the 88 x 180 grid the library's 4-channel weight-gradient kernel misses the
    float64 sum by ~4e-5 of its size already without normalisation (2e-7 on every other layer).  That is round-off, not a wrong
    term: tests/test_gpu_conv_grads.py holds this kernel bit-equal to float64 on integer inputs at this size and measures its error on
    random reals at 0.04 u A (A = sum |x| |dz|, u = 2^-24; 4e-7 of max |dw| where max |dw| is 5e-3 of A); here x is the independent
    model input, the sum cancels to ~1e-4 of A, and the same 0.04 u A is 4e-5 of what is left.  Behind a normalisation the
    gradient of that layer's output has the batch mean and the correlation with the normalised tensor projected out: the sum
    cancels ~20x more, the same absolute error is ~1e-3 of it."""
    logs = d.model.train_on_batch(x, y)
    torch.cuda.synchronize()
    out = _ref_forward(d.model, specs, torch.tensor(x, dtype=torch.float64), p, True)
    loss = ((out - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    loss.backward()
    assert logs[0] == pytest.approx(float(loss.detach()), rel=2e-5)
    got = _grads_of(d.model._trainer)
    assert len(got) == sum(1 for t in p.values() if t.requires_grad)
    first = [lay for lay in d.model.layers if isinstance(lay, L.Conv2D)][0].name
    for (lname, nm), g in got.items():
        ref = p[(lname, nm)].grad.numpy()
        if nm == 'kernel':
            ref = ref.transpose(2, 3, 1, 0)
        t = first_kernel_tol if (first_kernel_tol and (lname, nm) == (first, 'kernel')) else tol
        assert np.abs(g - ref).max() <= t * max(np.abs(ref).max(), 1e-6), (lname, nm, np.abs(g - ref).max(), np.abs(ref).max())
    for lay in d.model.layers:
        if isinstance(lay, L.BatchNormalization):
            for nm in ('moving_mean', 'moving_variance'):
                want = p[(lay.name, nm)].numpy()
                assert np.abs(_host(getattr(lay, nm)) - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0), (lay.name, nm)


@pytest.mark.parametrize('n', [8, 64])
def test_reference_stack_training_step_against_float64_autograd(monkeypatch, n):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    cs = (4, 88, 180)
    specs = bn_layers(cs)
    d = _build(specs, seed=3)
    rng = np.random.default_rng(30 + n)
    _randomise(d.model, rng)
    p = _ref_params(d.model)
    x = rng.standard_normal((n,) + cs).astype(np.float32)
    y = rng.standard_normal((n,) + cs).astype(np.float32)
    _check_step(d, specs, x, y, p, first_kernel_tol=2e-3 if n == 64 else None)


def test_three_adam_steps():
    cs = (4, 32, 48)
    specs = bn_layers(cs)
    d = _build(specs, seed=4, lr=1e-3)
    rng = np.random.default_rng(40)
    _randomise(d.model, rng)
    p = _ref_params(d.model)
    slots = {k: (torch.zeros_like(t), torch.zeros_like(t)) for k, t in p.items() if t.requires_grad}
    for it in range(3):
        x = rng.standard_normal((8,) + cs).astype(np.float32)
        y = rng.standard_normal((8,) + cs).astype(np.float32)
        d.model.train_on_batch(x, y)
        for t in p.values():
            t.grad = None
        out = _ref_forward(d.model, specs, torch.tensor(x, dtype=torch.float64), p, True)
        ((out - torch.tensor(y, dtype=torch.float64)) ** 2).mean().backward()
        with torch.no_grad():
            for k, (m, v) in slots.items():
                torch_ref.adam_keras_step(p[k], m, v, p[k].grad, it, lr=1e-3, epsilon=1e-7)
    for lay in d.model.layers:
        for (nm, _), a in zip(lay._weights, lay.get_weights()):
            want = p[(lay.name, nm)].detach().numpy()
            if nm == 'kernel':
                want = want.transpose(2, 3, 1, 0)
            assert np.abs(a - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (lay.name, nm)


# ----------------------------------------------------------------------------------------------------------------------- #
# the recorded / replayed step (csrc/tape.hip) against the eager step
# ----------------------------------------------------------------------------------------------------------------------- #
def _run_steps(monkeypatch, n, form, batches):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)
    cs = batches[0][0].shape[1:]
    d = _build(bn_layers(cs), seed=5)
    _randomise(d.model, np.random.default_rng(50))
    logs = [d.model.train_on_batch(x, y) for x, y in batches]
    torch.cuda.synchronize()
    tr = d.model._trainer
    if form != 'eager':
        ents = [e for k, e in tr._graphs.items() if k[0] == n and e.get('step') is not None]
        assert len(ents) == 1, 'the step of %d samples was not recorded (refused: %r)' % (n, tr._no_tape)
    return logs, [w.copy() for w in d.model.get_weights()], [s.cpu().numpy() for s in tr.opt_state]


@pytest.mark.parametrize('n', [12, 64])
def test_replayed_step_equals_the_eager_step(monkeypatch, n):
    rng = np.random.default_rng(600 + n)
    cs = (4, 88, 180)
    batches = [(rng.standard_normal((n,) + cs).astype(np.float32), rng.standard_normal((n,) + cs).astype(np.float32))
               for _ in range(5)]                  # 2 eager, 1 recorded (and validated), 2 replayed
    ref = _run_steps(monkeypatch, n, 'eager', batches)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, n, form, batches)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):       # weights (moving statistics included) and Adam slots
            assert np.array_equal(_bits(a), _bits(b)), form


# ----------------------------------------------------------------------------------------------------------------------- #
# inference: the moving statistics
# ----------------------------------------------------------------------------------------------------------------------- #
def test_predict_evaluate_and_rollouts_use_the_moving_statistics():
    cs = (4, 32, 48)
    specs = bn_layers(cs)
    d = _build(specs, seed=6)
    rng = np.random.default_rng(60)
    _randomise(d.model, rng)
    x = rng.standard_normal((5,) + cs).astype(np.float32)
    y = rng.standard_normal((5,) + cs).astype(np.float32)

    def oracle():
        p = _ref_params(d.model, requires_grad=False)
        with torch.no_grad():
            return _ref_forward(d.model, specs, torch.tensor(x, dtype=torch.float64), p, False).numpy()
    want = oracle()
    got = d.predict(x)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    ev = d.model.evaluate(x, y, verbose=0)
    assert ev[0] == pytest.approx(float(((want - y) ** 2).mean()), rel=1e-4)
    mm0 = [_host(lay.moving_mean).copy() for lay in d.model.layers if isinstance(lay, L.BatchNormalization)]
    d.predict(x)
    d.model.evaluate(x, y, verbose=0)                         # inference never touches the moving statistics
    assert all(np.array_equal(a, _host(lay.moving_mean)) for a, lay in
               zip(mm0, [lay for lay in d.model.layers if isinstance(lay, L.BatchNormalization)]))

    def eager_loop(steps):
        p_, out = x, []
        for _ in range(steps):
            p_ = d.predict(p_)
            out.append(p_)
        return np.stack(out)
    ts = d.predict_timeseries(x, 6)                        # one hipGraph: 3 model calls of 2 time steps each
    loop = eager_loop(3)
    assert np.array_equal(_bits(ts[4:6].transpose(1, 0, 2, 3, 4).reshape(5, 4, 32, 48)), _bits(loop[-1]))
    # new moving statistics (set_weights, then a training step): the cached graph reads them, it is not stale
    for lay in d.model.layers:
        if isinstance(lay, L.BatchNormalization):
            g, b, mm, mv = lay.get_weights()
            lay.set_weights([g, b, mm + 0.25, mv * 1.5])
    ts2 = d.predict_timeseries(x, 6)
    assert not np.array_equal(ts2, ts)
    assert np.array_equal(_bits(ts2[4:6].transpose(1, 0, 2, 3, 4).reshape(5, 4, 32, 48)), _bits(eager_loop(3)[-1]))
    d.model.train_on_batch(x, y)
    ts3 = d.predict_timeseries(x, 6)
    assert np.array_equal(_bits(ts3[4:6].transpose(1, 0, 2, 3, 4).reshape(5, 4, 32, 48)), _bits(eager_loop(3)[-1]))
    d.host_stream_bytes = 0                               # the streamed rollout: the same bits
    assert np.array_equal(_bits(d.predict_timeseries(x, 6)), _bits(ts3))


def test_fed_rollout_of_the_estimator_equals_the_host_loop(monkeypatch):
    from dlwp_amd.model import SeriesDataGenerator, TimeSeriesEstimator
    from tests.test_gpu_estimator import _series_dataset
    rng = np.random.default_rng(7)
    h, w = 16, 24
    ds = _series_dataset(rng, 20, h, w)
    specs = []
    from dlwp_amd.presets import unet_layers
    for spec in unet_layers((6, h, w), widths=(8, 16, 16, 16, 8), cout=4):
        specs.append(spec)
        if spec[0] == 'Conv2D' and spec[2].get('activation') == 'tanh':
            specs.append(('BatchNormalization', None, {'axis': 1}))
    d = _build(tuple(specs), seed=8)
    _randomise(d.model, rng)
    gen = SeriesDataGenerator(d, ds, input_time_steps=2, output_time_steps=2, add_insolation=True, interval=1, batch_size=4)
    est = TimeSeriesEstimator(d, gen)
    calls = []
    real = d.model._fed_entry
    monkeypatch.setattr(d.model, '_fed_entry', lambda *a, **k: calls.append(1) or real(*a, **k))
    out = est.predict(7)
    assert calls
    monkeypatch.setenv('DLWP_ESTIMATOR_HOST', '1')
    host = est.predict(7)
    assert np.array_equal(_bits(out.values), _bits(host.values))


# ----------------------------------------------------------------------------------------------------------------------- #
# functional use, model files, out of scope
# ----------------------------------------------------------------------------------------------------------------------- #
def _functional_unet(cs):
    from dlwp_amd.custom import PeriodicPadding2D

    def conv(t, f, act='tanh'):
        t = L.ZeroPadding2D(((1, 1), (0, 0)), **CF)(PeriodicPadding2D(((0, 0), (1, 1)), **CF)(t))
        return L.Conv2D(f, 3, activation=act, **CF)(t)
    x0 = L.Input(shape=cs)
    c1 = L.BatchNormalization(axis=1)(conv(x0, 8))
    c2 = L.BatchNormalization(axis=1)(conv(L.MaxPooling2D(2, **CF)(c1), 16))
    u1 = L.UpSampling2D(2, **CF)(c2)
    c3 = L.BatchNormalization(axis=1)(conv(L.concatenate([u1, c1], axis=1), 8))
    return x0, conv(c3, cs[0], act='linear')


def _functional_ref(model, x, p, training):
    def pads(t):
        t = torch.cat([t[..., -1:], t, t[..., :1]], dim=-1)
        return F.pad(t, (0, 0, 1, 1))

    def conv(t, lay, act=True):
        t = F.conv2d(pads(t), p[(lay.name, 'kernel')]) + p[(lay.name, 'bias')].view(1, -1, 1, 1)
        return torch.tanh(t) if act else t

    def bn(t, lay):
        return F.batch_norm(t, p[(lay.name, 'moving_mean')], p[(lay.name, 'moving_variance')], p[(lay.name, 'gamma')],
                            p[(lay.name, 'beta')], training=training, momentum=1 - MOM, eps=EPS)
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    bns = [lay for lay in model.layers if isinstance(lay, L.BatchNormalization)]
    c1 = bn(conv(x, convs[0]), bns[0])
    c2 = bn(conv(F.max_pool2d(c1, 2), convs[1]), bns[1])
    u1 = F.interpolate(c2, scale_factor=2, mode='nearest')
    c3 = bn(conv(torch.cat([u1, c1], dim=1), convs[2]), bns[2])
    return conv(c3, convs[3], act=False)


def test_functional_skip_unet_with_batchnorm(monkeypatch):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    cs = (4, 16, 24)
    x0, out = _functional_unet(cs)
    m = Model(inputs=x0, outputs=out, seed=1)
    m.compile(optimizer=Adam(lr=1e-3), loss='mse')
    rng = np.random.default_rng(11)
    _randomise(m, rng)
    x = rng.standard_normal((6,) + cs).astype(np.float32)
    y = rng.standard_normal((6,) + cs).astype(np.float32)
    p = _ref_params(m, requires_grad=False)
    with torch.no_grad():
        want = _functional_ref(m, torch.tensor(x, dtype=torch.float64), p, False).numpy()
    assert np.abs(m.predict(x) - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    p = _ref_params(m)
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    ref = ((_functional_ref(m, torch.tensor(x, dtype=torch.float64), p, True) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    ref.backward()
    assert loss == pytest.approx(float(ref), rel=2e-5)
    for (lname, nm), g in _grads_of(m._trainer).items():
        r = p[(lname, nm)].grad.numpy()
        r = r.transpose(2, 3, 1, 0) if nm == 'kernel' else r
        assert np.abs(g - r).max() <= 3e-4 * max(np.abs(r).max(), 1e-6), (lname, nm)
    for lay in m.layers:
        if isinstance(lay, L.BatchNormalization):
            assert np.abs(_host(lay.moving_variance) - p[(lay.name, 'moving_variance')].numpy()).max() <= 1e-5


def test_model_files_round_trip(tmp_path):
    from dlwp_amd.serialization import load_model_file
    cs = (4, 32, 48)
    d = _build(bn_layers(cs), seed=9)
    rng = np.random.default_rng(90)
    _randomise(d.model, rng)
    x = rng.standard_normal((3,) + cs).astype(np.float32)
    d.model.train_on_batch(x, x)                          # moving statistics away from their initial values
    want = d.predict(x)
    for fmt in ('keras', 'npz'):
        path = str(tmp_path / ('bn_%s.keras' % fmt))
        d.model.save(path, format=fmt)
        m2 = load_model_file(path)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(d.model.get_weights(), m2.get_weights()))
        assert np.array_equal(_bits(m2.predict(x)), _bits(want))


def test_out_of_scope_errors():
    cs = (4, 16, 24)
    d = _build(bn_layers(cs), seed=10)
    with pytest.raises(NotImplementedError, match='bfloat16'):
        d.model.set_activation_dtype('bfloat16')
    from dlwp_amd.model import DLWPNeuralNet
    d2 = DLWPNeuralNet(is_convolutional=True, scaler_type=None, scale_targets=False)
    with pytest.raises(NotImplementedError, match='gpus > 1'):
        d2.build_model(bn_layers(cs), gpus=2, loss='mse', optimizer='adam')
    assert os.environ.get('LOCAL_RANK') is None           # (no worker was started)
