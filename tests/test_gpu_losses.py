"""The Keras regression losses beyond 'mse' on the GPU (csrc/losses.hip): the three entry points against float64 formulas, the
fused phase-channel path against the separate passes, one Adam step per loss against torch float64 autograd, the logs of fit /
evaluate, data-parallel training and model files."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests.nets import cnn2_layers, unet_layers
from tests.test_gpu_model import FWD_TOL, _build, _weights_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-7
KINDS = (0, 1, 2, 3, 4)          # mse, mae, mape, msle, logcosh (include/dlwp_hip.h: DLWP_LOSS_*)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ref_terms(kind, p, t):
    """float64 element values and d value / d p (Keras 2.2 / TF gradient conventions)."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    x = p - t
    if kind == 0:
        return x * x, 2 * x
    if kind == 1:
        return np.abs(x), np.sign(x)
    if kind == 2:
        den = np.maximum(np.abs(t), EPS)
        return 100 * np.abs(x) / den, 100 * np.sign(x) / den
    if kind == 3:
        pc = np.maximum(p, EPS)
        d = np.log1p(pc) - np.log1p(np.maximum(t, EPS))
        return d * d, np.where(p < EPS, 0.0, 2 * d / (pc + 1))
    ax = np.abs(x)
    return ax + np.log1p(np.exp(-2 * ax)) - np.log(2.0), np.tanh(x)


def ref_loss(kind, yp, yt, w=None, loss_weight=1.0):
    """value and loss_weight * dL/dyp of mean(term(w yp, w yt)), w per row (axis -2).  The weighted operands are float32
    tensors in the reference (y_true * w, y_pred * w): rounded to float32 here too, the rest in float64."""
    w32 = np.ones(yp.shape[-2], np.float32) if w is None else np.asarray(w, np.float32)
    w32 = w32[:, None]
    v, g = ref_terms(kind, w32 * yp.astype(np.float32), w32 * yt.astype(np.float32))
    return v.mean(), loss_weight * w32.astype(np.float64) * g / v.size


def torch_loss(kind, out, yt, w=None):
    """the same loss on torch float64 tensors (for autograd through the network)."""
    if w is not None:
        wt = torch.tensor(np.asarray(w, np.float64))[:, None]
        out, yt = out * wt, yt * wt
    x = out - yt
    if kind == 0:
        return (x * x).mean()
    if kind == 1:
        return x.abs().mean()
    if kind == 2:
        return 100 * (x.abs() / yt.abs().clamp(min=EPS)).mean()
    if kind == 3:
        return ((out.clamp(min=EPS) + 1).log() - (yt.clamp(min=EPS) + 1).log()).pow(2).mean()
    return (x + torch.nn.functional.softplus(-2 * x) - np.log(2.0)).mean()


def edge_data(shape, seed):
    rng = np.random.default_rng(seed)
    yp = rng.standard_normal(shape).astype(np.float32)
    yt = (0.6 * yp + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    flat_p, flat_t = yp.reshape(-1), yt.reshape(-1)
    k = flat_p.size
    idx = rng.permutation(k)[:64]
    flat_t[idx[:8]] = 0.0                                    # mape: the clip of |yt| at eps
    flat_p[idx[8:16]] = 3e-8                                 # msle: both below eps
    flat_t[idx[8:16]] = -2e-8
    flat_t[idx[16:24]] = flat_p[idx[16:24]]                  # mae: x = 0, gradient exactly 0
    flat_p[idx[24:28]] = flat_t[idx[24:28]] + 100.0          # logcosh: |x| = 100 stays finite
    flat_p[idx[28:32]] = flat_t[idx[28:32]] - 100.0
    return yp, yt


def lat_weights(h, which):
    from dlwp_amd import custom as C
    lats = np.linspace(-88.0, 88.0, h)
    if which == 'function':
        return C.latitude_weights(lats, 'midlatitude')
    if which == 'class':
        return C.LatitudeWeightedLoss('mae', lats, weighting='midlatitude').row_weights
    return None


@pytest.mark.parametrize('shape', [(3, 5, 37, 71), (64, 4, 88, 180)])
@pytest.mark.parametrize('weights', [None, 'function', 'class'])
def test_elementwise_kernel_values_gradients_and_repeatability(shape, weights):
    from dlwp_amd import ops
    yp, yt = edge_data(shape, 11 + len(shape) + shape[0])
    w = lat_weights(shape[2], weights)
    p, t = dev(yp), dev(yt)
    wd = None if w is None else dev(w)
    for kind in KINDS:
        out = torch.full((1,), float('nan'), device='cuda')
        dy = torch.full_like(p, float('nan'))
        ops.loss_elementwise(p, t, out, dy, 0.7, kind, wd)
        torch.cuda.synchronize()
        v_ref, g_ref = ref_loss(kind, yp, yt, w, 0.7)
        got = float(out.cpu())
        assert np.isfinite(got) and abs(got - v_ref) <= FWD_TOL * abs(v_ref), (kind, got, v_ref)
        g = dy.cpu().numpy()
        assert np.all(np.isfinite(g))
        assert np.abs(g - g_ref).max() <= 1e-5 * np.abs(g_ref).max(), kind
        if kind == 1:
            same = (yp == yt)
            assert same.sum() >= 8 and np.all(g[same] == 0.0)
        out2, dy2 = torch.empty_like(out), torch.empty_like(dy)
        ops.loss_elementwise(p, t, out2, dy2, 0.7, kind, wd)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(dy, dy2)
        out3 = torch.empty_like(out)
        ops.loss_elementwise(p, t, out3, None, 0.7, kind, wd)         # value only: the same bits
        assert torch.equal(out, out3)


@pytest.mark.parametrize('shape', [(3, 5, 37, 71), (64, 4, 88, 180)])
def test_metrics_pass_equals_the_per_kind_values(shape):
    from dlwp_amd import _lib, ops
    yp, yt = edge_data(shape, 5)
    p, t = dev(yp), dev(yt)
    mask = 0x1f | _lib.METRIC_ACC_SUMS
    out = torch.full((8,), float('nan'), device='cuda')
    ops.loss_metrics(p, t, out, mask)
    again = torch.empty_like(out)
    ops.loss_metrics(p, t, again, mask)
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    got = out.cpu().numpy().astype(np.float64)
    for kind in KINDS:
        one = torch.empty(1, device='cuda')
        ops.loss_elementwise(p, t, one, None, 1.0, kind)
        assert got[kind] == pytest.approx(float(one.cpu()), rel=1e-6)
        assert got[kind] == pytest.approx(ref_loss(kind, yp, yt)[0], rel=FWD_TOL)
    p64, t64 = yp.astype(np.float64), yt.astype(np.float64)
    for k, want in enumerate(((p64 * t64).mean(), (p64 * p64).mean(), (t64 * t64).mean())):
        assert got[5 + k] == pytest.approx(want, rel=FWD_TOL)
    # a subset lands compactly, in kind order
    sub = torch.full((4,), float('nan'), device='cuda')
    ops.loss_metrics(p, t, sub, (1 << 4) | (1 << 2))
    torch.cuda.synchronize()
    assert sub[:2].cpu().numpy() == pytest.approx([got[2], got[4]], rel=1e-6) and torch.isnan(sub[2:]).all()
    # the function form of the metric
    from dlwp_amd import custom as C
    acc = float(C.anomaly_correlation(t, p).cpu())
    assert acc == pytest.approx(((p64 - t64) ** 2).mean() - (p64 * t64).mean() / np.sqrt((p64 ** 2).mean() * (t64 ** 2).mean()),
                                rel=1e-5)


def _d2s(yph):
    n, f4, h, w = yph.shape
    f = f4 // 4
    return yph.reshape(n, 2, 2, f, h, w).transpose(0, 3, 4, 1, 5, 2).reshape(n, f, 2 * h, 2 * w)


@pytest.mark.parametrize('shape', [(3, 5, 22, 36), (64, 4, 44, 90)])
def test_phase_kernel_equals_the_unfused_kernel(shape):
    from dlwp_amd import _lib, ops
    n, f, h, w = shape
    rng = np.random.default_rng(3)
    yph = rng.standard_normal((n, 4 * f, h, w)).astype(np.float32)
    yt = (0.5 * _d2s(yph) + 0.5 * rng.standard_normal((n, f, 2 * h, 2 * w))).astype(np.float32)
    yt.reshape(-1)[:5] = 0.0
    wts = lat_weights(2 * h, 'class')
    for kind in KINDS:
        for wd in (None, dev(wts)):
            out = torch.empty(1, device='cuda')
            dz = torch.empty((n, 4 * f, h, w), device='cuda')
            db = torch.empty(4 * f, device='cuda')
            ops.loss_elementwise_phase(dev(yph), dev(yt), out, dz, db, 0.9, kind, wd)
            ref_out = torch.empty(1, device='cuda')
            ref_dy = torch.empty((n, f, 2 * h, 2 * w), device='cuda')
            ops.loss_elementwise(dev(_d2s(yph)), dev(yt), ref_out, ref_dy, 0.9, kind, wd)
            torch.cuda.synchronize()
            assert float(out.cpu()) == pytest.approx(float(ref_out.cpu()), rel=1e-6), kind
            g = _d2s(dz.cpu().numpy())
            assert np.abs(g - ref_dy.cpu().numpy()).max() <= 1e-6 * np.abs(ref_dy.cpu().numpy()).max(), kind
            dbr = dz.cpu().numpy().astype(np.float64).sum(axis=(0, 2, 3))
            assert np.abs(db.cpu().numpy() - dbr).max() <= 1e-5 * max(np.abs(dbr).max(), 1e-6), kind
    # the metrics pass on the phase layout
    out = torch.empty(8, device='cuda')
    ref = torch.empty(8, device='cuda')
    mask = 0x1f | _lib.METRIC_ACC_SUMS
    ops.loss_metrics(dev(yph), dev(yt), out, mask, phase=True)
    ops.loss_metrics(dev(_d2s(yph)), dev(yt), ref, mask)
    torch.cuda.synchronize()
    assert out.cpu().numpy() == pytest.approx(ref.cpu().numpy(), rel=1e-6)


def _losses():
    return [('mae', 1, None), ('mape', 2, None), ('msle', 3, None), ('logcosh', 4, None),
            ('lat_mae', 1, 'class')]


def _loss_object(name, h):
    from dlwp_amd import custom as C
    if name == 'lat_mae':
        return C.LatitudeWeightedLoss('mae', np.linspace(-88.0, 88.0, h), weighting='midlatitude')
    return name


@pytest.mark.parametrize('net', ['unet', 'cnn73'])
@pytest.mark.parametrize('name,kind,wsel', _losses())
def test_one_adam_step_matches_float64_autograd(monkeypatch, net, name, kind, wsel):
    from oracle import np_ref
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    rng = np.random.default_rng(21 + kind)
    cs = (4, 16, 24) if net == 'unet' else (2, 73, 144)
    layers = unet_layers(cs) if net == 'unet' else cnn2_layers(cs, hidden=16)
    loss = _loss_object(name, cs[1])
    d = _build(layers, time_dim=2, loss=loss, metrics=['mae', 'logcosh'])
    weights = _weights_of(d.model, rng)
    x = rng.standard_normal((6,) + cs).astype(np.float32)
    y = rng.standard_normal((6,) + cs).astype(np.float32)
    w = None if wsel is None else loss.row_weights
    tw = torch_ref.to_torch_weights(weights, dtype=torch.float64, requires_grad=True)
    out = torch_ref.run_layers(layers, torch.tensor(x, dtype=torch.float64), tw)
    yt = torch.tensor(y, dtype=torch.float64)
    lref = torch_loss(kind, out, yt, w)
    lref.backward()
    o64 = out.detach().numpy()
    tr = d.model._trainer
    assert bool(tr._phase_outputs()) == (net == 'unet')          # the new kinds keep the fused output-layer path
    vals = d.model.train_on_batch(x, y)
    torch.cuda.synchronize()
    assert vals[0] == pytest.approx(float(lref), rel=2e-5)
    assert vals[1] == pytest.approx(np.abs(o64 - y).mean(), rel=2e-5)
    assert vals[2] == pytest.approx(ref_terms(4, o64, y)[0].mean(), rel=2e-5)
    off = 0
    new_ref = []
    for (wt, bt), (w0, b0) in zip(tw, weights):
        for g_ref, p0 in ((wt.grad.numpy().transpose(2, 3, 1, 0), w0), (bt.grad.numpy(), b0)):
            g = tr.flat_grads[off:off + g_ref.size].cpu().numpy().reshape(g_ref.shape)
            off += g_ref.size
            assert np.abs(g - g_ref).max() <= 2e-4 * max(np.abs(g_ref).max(), 1e-6), (name, g_ref.shape)
            # Adam on the step's own gradient (a sign flip of a near-zero float32 gradient moves a weight by ~lr either way)
            new_ref.append(np_ref.adam_keras_step(p0.astype(np.float64), np.zeros_like(g_ref), np.zeros_like(g_ref),
                                                  g.astype(np.float64), 0)[0])
    for w_new, w_ref in zip(d.model.get_weights(), new_ref):
        assert np.abs(w_new - w_ref).max() < 5e-6


@pytest.mark.parametrize('name', ['mae', 'logcosh', 'lat_mae'])
def test_recorded_step_replays_the_eager_step(monkeypatch, name):
    cs = (4, 16, 24)
    rng = np.random.default_rng(4)
    batches = [(rng.standard_normal((8,) + cs).astype(np.float32), rng.standard_normal((8,) + cs).astype(np.float32))
               for _ in range(5)]
    res = {}
    for form in ('0', '1'):
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', form)
        d = _build(unet_layers(cs), time_dim=2, seed=3, loss=_loss_object(name, cs[1]),
                   metrics=['mape', 'anomaly_correlation'])
        _weights_of(d.model, np.random.default_rng(30))
        logs = [d.model.train_on_batch(x, y) for x, y in batches]
        torch.cuda.synchronize()
        tr = d.model._trainer
        if form == '1':
            assert any(e.get('step') is not None for e in tr._graphs.values()), tr._no_tape
        res[form] = (logs, d.model.get_weights(), tr.flat_grads.cpu().numpy().copy())
    # the recorded step was validated against a launch-by-launch run at recording time (DLWP_TAPE_VALIDATE); the replayed
    # form may pair launches the eager step issues apart (csrc/conv_pair.hip): float32 round-off, as test_gpu_train_steps.py
    for a, b in zip(res['0'][0], res['1'][0]):
        assert np.allclose(a, b, rtol=1e-5, atol=1e-7), (a, b)
    for a, b in zip(res['0'][1], res['1'][1]):
        assert np.abs(a - b).max() <= 2e-7 * len(batches)
    assert np.abs(res['0'][2] - res['1'][2]).max() <= 1e-5 * np.abs(res['0'][2]).max()


def test_fit_and_evaluate_logs_match_float64_on_the_predictions():
    from dlwp_amd import custom as C
    cs = (4, 16, 24)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((40,) + cs).astype(np.float32)
    y = (0.5 * x + 0.3 * rng.standard_normal((40,) + cs)).astype(np.float32)
    d = _build(unet_layers(cs), time_dim=2, loss='logcosh',
               metrics=['mae', 'mape', 'msle', C.anomaly_correlation, 'mse', C.latitude_weighted_loss('mae', np.linspace(-80, 80, 16))])
    _weights_of(d.model, rng)
    assert d.model.metrics_names == ['loss', 'mean_absolute_error', 'mean_absolute_percentage_error',
                                     'mean_squared_logarithmic_error', 'anomaly_correlation', 'mean_squared_error', 'lat_loss']
    p = d.model.predict(x).astype(np.float64)
    y64 = y.astype(np.float64)
    ev = d.model.evaluate(x, y, batch_size=40, verbose=0)
    wl = np.cos(np.deg2rad(np.linspace(-80, 80, 16)))[:, None]
    want = [ref_terms(4, p, y64)[0].mean(), np.abs(p - y64).mean(), ref_terms(2, p, y64)[0].mean(), ref_terms(3, p, y64)[0].mean(),
            ((p - y64) ** 2).mean() - (p * y64).mean() / np.sqrt((p * p).mean() * (y64 * y64).mean()), ((p - y64) ** 2).mean(),
            np.abs(wl * p - wl * y64).mean()]
    assert ev == pytest.approx(want, rel=2e-5)
    # fit: the epoch's log keys and, with one batch per epoch, the values of the step's predictions (before the update)
    h = d.fit(x, y, batch_size=40, epochs=1, verbose=0, shuffle=False)
    assert sorted(h.history) == sorted(d.model.metrics_names)
    assert [h.history[k][0] for k in d.model.metrics_names] == pytest.approx(want, rel=2e-5)
    # two outputs with loss weights (DLWPFunctional)
    from dlwp_amd import layers as L
    from dlwp_amd.engine import Model
    from dlwp_amd.model import DLWPFunctional
    x0 = L.Input(shape=cs)
    c1 = L.Conv2D(4, 3, padding='same', activation='tanh', data_format='channels_first', name='first')
    c2 = L.Conv2D(4, 3, padding='same', data_format='channels_first', name='second')
    o1 = c1(x0)
    m = Model(inputs=x0, outputs=[o1, c2(o1)])
    f = DLWPFunctional(is_convolutional=True, time_dim=2)
    f.build_model(m, loss='mae', loss_weights=[0.25, 0.75], optimizer='adam', metrics=['logcosh', C.anomaly_correlation])
    assert m.metrics_names == ['loss', 'first_loss', 'second_loss', 'first_logcosh', 'first_anomaly_correlation',
                               'second_logcosh', 'second_anomaly_correlation']
    y2 = [y, (0.2 * y).astype(np.float32)]
    preds = [a.astype(np.float64) for a in m.predict(x)]
    ev = m.evaluate(x, y2, batch_size=40, verbose=0)
    per = [np.abs(pp - t).mean() for pp, t in zip(preds, y2)]
    mets = []
    for pp, t in zip(preds, y2):
        t = t.astype(np.float64)
        mets += [ref_terms(4, pp, t)[0].mean(),
                 ((pp - t) ** 2).mean() - (pp * t).mean() / np.sqrt((pp * pp).mean() * (t * t).mean())]
    assert ev == pytest.approx([0.25 * per[0] + 0.75 * per[1]] + per + mets, rel=2e-5)


def _dp_worker(rank, world, port, ret, extra_env):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DLWP_SHARE_GPUS='1', DLWP_DIST_BACKEND='gloo')
    os.environ.update(extra_env)
    from dlwp_amd import custom as C
    from dlwp_amd import parallel
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    parallel.init()
    np.random.seed(1000 + 17 * rank)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(unet_layers((4, 16, 24), widths=(8, 16, 16, 16, 8)), loss='mae', optimizer=Adam(lr=1e-3),
                  metrics=['logcosh', C.anomaly_correlation], gpus=world)
    w0 = [w.copy() for w in d.model.get_weights()]
    x, y = _dp_data()
    logs = [d.model.train_on_batch(x, y) for _ in range(3)]
    torch.cuda.synchronize()
    ret[rank] = {'w0': w0, 'w1': d.model.get_weights(), 'logs': logs,
                 'oneshot': bool(getattr(d.model._trainer.dp, '_xchg', None))}
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _dp_data():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((8, 4, 16, 24)).astype(np.float32)
    y = (0.5 * x + 0.25 * np.roll(x, 1, axis=-1) + 0.1 * rng.standard_normal(x.shape)).astype(np.float32)
    return x, y


@pytest.mark.parametrize('transport', ['gloo', 'oneshot'])
def test_two_rank_training_with_the_new_loss_and_metrics_equals_the_single_process_run(transport):
    from dlwp_amd import custom as C
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    from tests.test_gpu_parallel import _free_port
    extra = {'DLWP_ALLREDUCE': 'oneshot'} if transport == 'oneshot' else {}
    ctx = mp.get_context('spawn')
    port = _free_port()
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, ret, extra)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            if p.is_alive():
                p.kill()
                pytest.fail('data-parallel worker timed out')
            assert p.exitcode == 0, 'data-parallel worker failed'
        res = dict(ret)
    assert res[0]['oneshot'] == res[1]['oneshot'] == (transport == 'oneshot')
    assert res[0]['logs'] == res[1]['logs']
    for a, b in zip(res[0]['w1'], res[1]['w1']):
        assert np.array_equal(a, b)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(unet_layers((4, 16, 24), widths=(8, 16, 16, 16, 8)), loss='mae', optimizer=Adam(lr=1e-3),
                  metrics=['logcosh', C.anomaly_correlation])
    d.model.set_weights(res[0]['w0'])
    x, y = _dp_data()
    logs = [d.model.train_on_batch(x, y) for _ in range(3)]
    assert d.model.metrics_names == ['loss', 'logcosh', 'anomaly_correlation']
    for got, want in zip(res[0]['logs'], logs):
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (got, want)
    for a, b in zip(res[0]['w1'], d.model.get_weights()):
        assert np.abs(a - b).max() <= 1e-6 * 3, np.abs(a - b).max()


@pytest.mark.parametrize('fmt', ['keras', 'npz'])
@pytest.mark.parametrize('name', ['logcosh', 'lat_mae'])
def test_saved_and_reloaded_training_continues_as_if_uninterrupted(tmp_path, monkeypatch, fmt, name):
    from dlwp_amd import custom as C
    from dlwp_amd import serialization
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    cs = (4, 16, 24)
    rng = np.random.default_rng(12)
    batches = [(rng.standard_normal((8,) + cs).astype(np.float32), rng.standard_normal((8,) + cs).astype(np.float32))
               for _ in range(5)]
    metrics = ['mape', C.anomaly_correlation]
    d = _build(unet_layers(cs), time_dim=2, seed=2, loss=_loss_object(name, cs[1]), metrics=metrics)
    w0 = d.model.get_weights()
    full = [d.model.train_on_batch(x, y) for x, y in batches]
    want = d.model.get_weights()
    d = _build(unet_layers(cs), time_dim=2, seed=2, loss=_loss_object(name, cs[1]), metrics=metrics)
    d.model.set_weights(w0)
    first = [d.model.train_on_batch(x, y) for x, y in batches[:3]]
    path = str(tmp_path / ('m.' + fmt))
    d.model.save(path, format=fmt)
    m2 = serialization.load_model_file(path)
    assert m2.metrics_names == ['loss', 'mean_absolute_percentage_error', 'anomaly_correlation']
    rest = [m2.train_on_batch(x, y) for x, y in batches[3:]]
    assert m2.optimizer.iterations == 5
    for a, b in zip(first + rest, full):
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7), (a, b)
    for a, b in zip(m2.get_weights(), want):
        assert np.abs(a - b).max() <= 1e-6


def test_build_model_with_mae_and_a_logcosh_metric_trains():
    """DLWPNeuralNet.build_model(unet, loss='mae', metrics=['logcosh']) followed by fit: refused before these losses existed."""
    cs = (4, 16, 24)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((16,) + cs).astype(np.float32)
    y = (0.5 * x).astype(np.float32)
    d = _build(unet_layers(cs), time_dim=2, loss='mae', metrics=['logcosh'])
    h = d.fit(x, y, batch_size=8, epochs=2, verbose=0)
    assert sorted(h.history) == ['logcosh', 'loss'] and all(np.isfinite(h.history['loss']))
    assert h.history['loss'][1] < h.history['loss'][0] * 1.5
