"""Dense / Flatten / Dropout without a GPU: the layers' Keras surface, their lowering into the plan, the refusals, and the numpy
restatements the GPU tests compare against (tests/test_gpu_dense.py): the float64 dense layer and its gradients, and the Dropout
mask generator bit for bit."""
import math

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd.engine import Model, Sequential
from dlwp_amd.regularizers import l2

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')


def feed_forward_layers(f, rate=0.25, reg=1e-4, seed=None):
    """the 'Feed-forward dense neural network' block of the reference's examples/train_generator.py:224-233"""
    return (
        ('Dense', (f // 2,), {'activation': 'tanh', 'kernel_regularizer': l2(reg) if reg else None, 'input_shape': (f,)}),
        ('Dropout', (rate,), {'seed': seed} if seed is not None else None),
        ('Dense', (f,), None),
    )


def conv_dense_layers(c, h, w, filters=6):
    """a convolutional front with a dense head (examples/train_generator.py:138-140: ... -> Flatten -> Dense -> Reshape)"""
    return (
        ('Conv2D', (filters, 3), dict(CF, padding='same', activation='tanh', input_shape=(c, h, w))),
        ('Flatten', None, None),
        ('Dense', (c * h * w,), None),
        ('Reshape', ((c, h, w),), None),
    )


def build(specs, device=CPU, seed=3):
    net = Sequential(device=device, seed=seed)
    for name, args, kwargs in specs:
        net.add(getattr(L, name)(*(args or ()), **(kwargs or {})))
    return net


# -- float64 restatements ---------------------------------------------------------------------------------------------------- #
def np_act(z, act):
    return np.tanh(z) if act == 'tanh' else (np.maximum(z, 0.0) if act == 'relu' else z)


def np_act_grad(y, act):
    return 1.0 - y * y if act == 'tanh' else ((y > 0).astype(np.float64) if act == 'relu' else np.ones_like(y))


def np_dense_forward(x, w, b, act):
    z = np.asarray(x, np.float64) @ np.asarray(w, np.float64)
    if b is not None:
        z = z + np.asarray(b, np.float64)[None, :]
    return np_act(z, act)


def np_dense_backward(x, w, y, dy, act):
    """(dx, dw, db) of y = act(x w + b) for the output gradient dy; y is the forward's output"""
    g = np.asarray(dy, np.float64) * np_act_grad(np.asarray(y, np.float64), act)
    return g @ np.asarray(w, np.float64).T, np.asarray(x, np.float64).T @ g, g.sum(axis=0)


# -- the Dropout mask: Philox-4x32-10, counter (q lo, q hi, step, layer), key (seed lo, seed hi) ------------------------------------ #
def np_philox4x32_10(c0, c1, c2, c3, k0, k1):
    u64, u32 = np.uint64, np.uint32
    c0, c1, c2, c3 = (np.asarray(c, dtype=u32) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0 = c0.astype(u64) * u64(0xD2511F53)
        p1 = c2.astype(u64) * u64(0xCD9E8D57)
        hi0, lo0 = (p0 >> u64(32)).astype(u32), (p0 & u64(0xffffffff)).astype(u32)
        hi1, lo1 = (p1 >> u64(32)).astype(u32), (p1 & u64(0xffffffff)).astype(u32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ u32(k0), lo1, hi0 ^ c3 ^ u32(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def np_dropout_words(n, seed, layer, step):
    """the 32-bit word that decides each of n elements: word i % 4 of block i // 4"""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    z = np.zeros(q.shape, dtype=np.uint32)
    words = np_philox4x32_10((q & np.uint64(0xffffffff)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                             z + np.uint32(int(step) & 0xffffffff), z + np.uint32(int(layer) & 0xffffffff),
                             int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    return np.stack(words, axis=1).reshape(-1)[:n]


def np_dropout_mask(n, rate, seed, layer, step):
    """(keep as bool, scale as float32): an element is kept when its word >= floor(rate 2^32); kept values are multiplied by
    float32(1 / (1 - rate)), dropped ones are +0"""
    thr = min(int(float(rate) * 4294967296.0), 4294967295)
    return np_dropout_words(n, seed, layer, step) >= np.uint32(thr), np.float32(1.0 / (1.0 - float(rate)))


def np_dropout_apply(x, rate, seed, layer, step):
    x = np.asarray(x, np.float32)
    keep, scale = np_dropout_mask(x.size, rate, seed, layer, step)
    return np.where(keep.reshape(x.shape), x * scale, np.float32(0.0)).astype(np.float32)


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors: zero, all ones, digits of pi)"""
    got = np_philox4x32_10([0], [0], [0], [0], 0, 0)
    assert [int(v[0]) for v in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = np_philox4x32_10([0xffffffff], [0xffffffff], [0xffffffff], [0xffffffff], 0xffffffff, 0xffffffff)
    assert [int(v[0]) for v in got] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = np_philox4x32_10([0x243f6a88], [0x85a308d3], [0x13198a2e], [0x03707344], 0xa4093822, 0x299f31d0)
    assert [int(v[0]) for v in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_mask_restatement_properties():
    n = 1 << 20
    for rate in (0.25, 0.5):
        keep, scale = np_dropout_mask(n, rate, seed=1234, layer=0, step=7)
        sd = math.sqrt(rate * (1 - rate) / n)
        assert abs(keep.mean() - (1 - rate)) < 4 * sd
        assert scale == np.float32(1.0 / (1.0 - rate))
    a = np_dropout_mask(4099, 0.25, 5, 0, 1)[0]
    assert np.array_equal(a, np_dropout_mask(4099, 0.25, 5, 0, 1)[0])
    for other in ((6, 0, 1), (5, 1, 1), (5, 0, 2)):
        assert not np.array_equal(a, np_dropout_mask(4099, 0.25, *other)[0])
    assert np_dropout_mask(100, 0.0, 1, 0, 0)[0].all()
    x = np.linspace(-1, 1, 37, dtype=np.float32)
    assert np.array_equal(np_dropout_apply(x, 0.0, 9, 0, 0), x)


# -- layer surface ----------------------------------------------------------------------------------------------------------- #
def test_dense_defaults_weights_and_config():
    lay = L.Dense(7)
    assert (lay.units, lay.activation, lay.use_bias, lay.kernel_initializer, lay.kernel_regularizer) == \
        (7, 'linear', True, 'glorot_uniform', None)
    x0 = L.Input(shape=(50,))
    d = L.Dense(30, activation='tanh', kernel_regularizer=l2(1e-3))
    m = Model(inputs=x0, outputs=d(x0), device=CPU, seed=1)
    assert [nm for nm, _ in d._weights] == ['kernel', 'bias']
    k, b = d.get_weights()
    assert k.shape == (50, 30) and b.shape == (30,) and k.dtype == np.float32
    limit = math.sqrt(6.0 / (50 + 30))
    assert np.abs(k).max() <= limit and np.abs(k).max() > 0.9 * limit and np.all(b == 0)
    assert d.count_params() == 50 * 30 + 30 == m.count_params()
    assert m.output_shape == (None, 30) and d.output_shape == (None, 30) and d.input_shape == (None, 50)
    cfg = d.get_config()
    assert (cfg['units'], cfg['activation'], cfg['use_bias']) == (30, 'tanh', True)
    nb = L.Dense(4, use_bias=False, input_shape=(9,))
    s = build((('Dense', (4,), {'use_bias': False, 'input_shape': (9,)}),))
    assert [nm for nm, _ in s.layers[0]._weights] == ['kernel'] and s.count_params() == 36 and nb.batch_input_shape == (None, 9)


def test_flatten_and_dropout_surface():
    f = L.Flatten()
    assert f.data_format == 'channels_last' and f.compute_output_shape((3, 4, 5)) == (60,)
    assert f.get_config()['data_format'] == 'channels_last'
    d = L.Dropout(0.25)
    assert (d.rate, d.noise_shape, d.seed) == (0.25, None, None)
    assert d.compute_output_shape((11,)) == (11,) and d.count_params() == 0
    cfg = L.Dropout(0.5, seed=3).get_config()
    assert (cfg['rate'], cfg['noise_shape'], cfg['seed']) == (0.5, None, 3)


def test_refusals():
    with pytest.raises(NotImplementedError):
        L.Dense(4)(L.Input(shape=(3, 5)))                    # Keras: the last axis; no reference call site
    with pytest.raises(NotImplementedError):
        L.Dense(4, activation='sigmoid')
    with pytest.raises(NotImplementedError, match='channels-last order'):
        L.Flatten(data_format='channels_first')
    with pytest.raises(NotImplementedError):
        L.Dropout(0.25, noise_shape=(None, 1))
    with pytest.raises(ValueError):
        L.Dropout(1.0)
    net = build(feed_forward_layers(24))
    with pytest.raises(NotImplementedError, match='Dense'):
        net.set_activation_dtype('bfloat16')


def test_parallel_dropout_is_refused_before_any_worker_starts():
    from dlwp_amd.model.models import _refuse_parallel_dropout
    with pytest.raises(NotImplementedError, match='Dropout'):
        _refuse_parallel_dropout(build(feed_forward_layers(24)))
    _refuse_parallel_dropout(build(feed_forward_layers(24)[::2]))     # Dense alone is an ordinary data-parallel model


# -- lowering ------------------------------------------------------------------------------------------------------------------ #
def test_feed_forward_plan():
    net = build(feed_forward_layers(24))
    assert net.plan._in_store == (24, 1, 1) and net.plan.output_store == [(24, 1, 1)] and net.plan.output_shapes == [(24,)]
    assert [op.kind for op in net.plan.ops] == ['dense', 'dropout', 'dense']          # training: the mask has a launch
    assert [op.kind for op in net.infer_plan.ops] == ['dense', 'dense']               # predict / rollouts: none
    d1, d2 = net.infer_plan.ops
    assert d1.src == -1 and d2.src == d1.dst and d2.dst == -2 and d1.xs == (24, 1, 1) and d2.xs == (12, 1, 1)
    assert d1.act == 1 and d2.act == 0
    assert net.plan.dense_layers == [net.layers[0], net.layers[2]] and net.plan.dropout_layers == [net.layers[1]]
    assert net.count_params() == 24 * 12 + 12 + 12 * 24 + 24


def test_conv_front_dense_head_plan():
    net = build(conv_dense_layers(2, 4, 6))
    for plan in (net.plan, net.infer_plan):
        assert [op.kind for op in plan.ops] == ['conv', 'dense']                      # Flatten and Reshape are views
        conv, dense = plan.ops
        assert dense.src == conv.dst and dense.xs == (6, 4, 6) and dense.dst == -2
        assert plan.buffers[conv.dst] == (6, 4, 6)                                    # (the convolution's buffer keeps its shape)
        assert plan.output_store == [(2, 4, 6)] and plan.output_shapes == [(2, 4, 6)]


def test_rank_one_input_reshape_and_output():
    x0 = L.Input(shape=(48,))
    t = L.Reshape((2, 4, 6))(x0)
    t = L.Conv2D(3, 3, padding='same', **CF)(t)
    t = L.Flatten()(t)
    m = Model(inputs=x0, outputs=t, device=CPU)
    assert m.output_shape == (None, 72) and m.plan._in_store == (48, 1, 1)
    assert [op.kind for op in m.infer_plan.ops] == ['copy', 'conv']
    with pytest.raises(NotImplementedError):
        Model(inputs=L.Input(shape=(4, 5)), outputs=L.Reshape((20,))(L.Input(shape=(4, 5))), device=CPU)


def test_dense_parameters_are_ordinary_flat_parameters():
    from dlwp_amd.training import flatten_parameters
    net = build(feed_forward_layers(24))
    flat, entries = flatten_parameters(net)
    assert [(lay.name, nm, shape) for lay, nm, off, numel, shape in entries] == [
        (net.layers[0].name, 'kernel', (24, 12)), (net.layers[0].name, 'bias', (12,)),
        (net.layers[2].name, 'kernel', (12, 24)), (net.layers[2].name, 'bias', (24,))]
    assert flat.numel() == net.count_params()


def test_model_config_round_trip_names_keras_classes():
    from dlwp_amd import serialization as S
    net = build(feed_forward_layers(24, seed=11))
    spec = [S._keras_layer_spec(lay) for lay in net.layers]
    assert [s['class_name'] for s in spec] == ['Dense', 'Dropout', 'Dense']
    assert spec[0]['config']['units'] == 12 and spec[0]['config']['activation'] == 'tanh' and spec[0]['config']['use_bias'] is True
    assert spec[0]['config']['kernel_regularizer']['config']['l2'] == pytest.approx(1e-4)
    assert spec[1]['config']['rate'] == 0.25 and spec[1]['config']['seed'] == 11 and spec[1]['config']['noise_shape'] is None
    kw = S._keras_layer_kwargs(L.Dense, spec[0]['config'])
    again = L.Dense(**kw)
    assert (again.units, again.activation, again.use_bias, again.kernel_regularizer.l2) == (12, 'tanh', True, pytest.approx(1e-4))
    assert L.Dropout(**S._keras_layer_kwargs(L.Dropout, spec[1]['config'])).mask_seed == 11
    f = S._keras_layer_spec(L.Flatten())
    assert f['class_name'] == 'Flatten' and L.Flatten(**S._keras_layer_kwargs(L.Flatten, f['config'])).data_format == 'channels_last'


def test_restatement_against_autograd():
    rng = np.random.RandomState(0)
    x, w, b, dy = rng.randn(5, 7), rng.randn(7, 3), rng.randn(3), rng.randn(5, 3)
    for act in ('linear', 'tanh', 'relu'):
        xt, wt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
        z = xt @ wt + bt
        yt = torch.tanh(z) if act == 'tanh' else (torch.relu(z) if act == 'relu' else z)
        yt.backward(torch.tensor(dy))
        y = np_dense_forward(x, w, b, act)
        dx, dw, db = np_dense_backward(x, w, y, dy, act)
        assert np.allclose(y, yt.detach().numpy(), rtol=0, atol=1e-12)
        for got, want in ((dx, xt.grad), (dw, wt.grad), (db, bt.grad)):
            assert np.allclose(got, want.numpy(), rtol=0, atol=1e-12)
