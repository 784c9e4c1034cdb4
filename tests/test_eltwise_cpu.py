"""Activation and merge layers without a GPU: the layers' Keras surface, the refusals, their lowering into the plan, the model
specification round trip, the import shim -- and the numpy restatements of every activation kind and every merge, forward and
backward, that tests/test_gpu_eltwise.py compares the kernels against (DESIGN.md section 5.25 holds the closed forms).  The
restatements compute in the dtype of their input, one numpy operation per rounding: in float64 they are the oracle (checked here
against torch autograd), in float32 they round in the order the kernels do."""
import json

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd.engine import Model, Sequential

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')

SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
KINDS = ('relu', 'elu', 'selu', 'sigmoid', 'hard_sigmoid', 'softplus', 'softsign', 'tanh')
TRANSCENDENTAL = KINDS[1:]
MERGES = ('add', 'subtract', 'multiply', 'average', 'maximum', 'minimum')
#: the relu family's layers of the exact tests: (layer class, arguments) -> (alpha, max_value, theta)
RELU_LAYERS = (('LeakyReLU', (0.3,)), ('ReLU', (10.0, 0.1, 0.0)), ('ReLU', (3.0, 0.1, 0.5)), ('ThresholdedReLU', (1.0,)))


# -- restatements --------------------------------------------------------------------------------------------------------------- #
def np_act_fwd(x, kind, alpha=0.0, max_value=None, theta=0.0):
    x = np.asarray(x)
    T = x.dtype.type
    with np.errstate(all='ignore'):
        if kind == 'relu':
            m = T(np.inf) if max_value is None else T(max_value)
            neg = np.where(np.isnan(x), x, T(0)) if float(alpha) == 0.0 else T(alpha) * (x - T(theta))
            return np.where(x > T(theta), np.minimum(x, m), neg).astype(x.dtype)
        if kind == 'elu':
            return np.where(x > 0, x, T(alpha) * (np.exp(x) - T(1))).astype(x.dtype)
        if kind == 'selu':
            return (T(SELU_SCALE) * np.where(x > 0, x, T(SELU_ALPHA) * (np.exp(x) - T(1)))).astype(x.dtype)
        if kind == 'sigmoid':
            return (T(1) / (T(1) + np.exp(-x))).astype(x.dtype)
        if kind == 'hard_sigmoid':
            return np.where(np.isnan(x), x, np.clip(T(0.2) * x + T(0.5), T(0), T(1))).astype(x.dtype)
        if kind == 'softplus':
            return (np.where(x > 0, x, T(0)) + np.log1p(np.exp(-np.abs(x)))).astype(x.dtype)
        if kind == 'softsign':
            return (x / (T(1) + np.abs(x))).astype(x.dtype)
        if kind == 'tanh':
            return np.tanh(x).astype(x.dtype)
    raise ValueError(kind)


def np_act_slope(x, kind, alpha=0.0, max_value=None, theta=0.0):
    """f'(x) from the INPUT x; NaN where x is NaN"""
    x = np.asarray(x)
    T = x.dtype.type
    with np.errstate(all='ignore'):
        if kind == 'relu':
            m = T(np.inf) if max_value is None else T(max_value)
            d = np.where(x > T(theta), np.where(x <= m, T(1), T(0)), T(alpha))
        elif kind == 'elu':
            d = np.where(x > 0, T(1), T(alpha) * np.exp(x))
        elif kind == 'selu':
            d = T(SELU_SCALE) * np.where(x > 0, T(1), T(SELU_ALPHA) * np.exp(x))
        elif kind == 'sigmoid':
            y = np_act_fwd(x, 'sigmoid')
            d = y * (T(1) - y)
        elif kind == 'hard_sigmoid':
            d = np.where((x > T(-2.5)) & (x < T(2.5)), T(0.2), T(0))
        elif kind == 'softplus':
            d = np_act_fwd(x, 'sigmoid')
        elif kind == 'softsign':
            t = T(1) + np.abs(x)
            d = T(1) / (t * t)
        elif kind == 'tanh':
            y = np.tanh(x)
            d = T(1) - y * y
        else:
            raise ValueError(kind)
        return np.where(np.isnan(x), x, d).astype(x.dtype)


def np_act_bwd(x, dy, kind, alpha=0.0, max_value=None, theta=0.0):
    with np.errstate(all='ignore'):
        return (np.asarray(dy) * np_act_slope(x, kind, alpha, max_value, theta)).astype(np.asarray(x).dtype)


def _np_merge2(a, b, kind):
    with np.errstate(all='ignore'):
        if kind in ('add', 'average'):
            return a + b
        if kind == 'subtract':
            return a - b
        if kind == 'multiply':
            return a * b
        if kind == 'maximum':                    # NaN propagates; of two equal operands the left one is kept
            return np.where((a >= b) | np.isnan(a), a, b)
        if kind == 'minimum':
            return np.where((a <= b) | np.isnan(a), a, b)
    raise ValueError(kind)


def np_merge_fwd(xs, kind):
    xs = [np.asarray(x) for x in xs]
    r = _np_merge2(xs[0], xs[1], kind)
    for x in xs[2:]:
        r = _np_merge2(r, x, kind)
    if kind == 'average':
        r = r / xs[0].dtype.type(len(xs))
    return r.astype(xs[0].dtype)


def np_merge_bwd(xs, dy, kind):
    xs = [np.asarray(x) for x in xs]
    dy = np.asarray(dy)
    T = xs[0].dtype.type
    with np.errstate(all='ignore'):
        if kind == 'add':
            return [dy.copy() for _ in xs]
        if kind == 'subtract':
            return [dy.copy(), -dy]
        if kind == 'average':
            return [dy / T(len(xs)) for _ in xs]
        if kind == 'multiply':
            out = []
            for i in range(len(xs)):
                others = [x for j, x in enumerate(xs) if j != i]
                p = others[0]
                for x in others[1:]:
                    p = p * x
                out.append(dy * p)
            return out
        y = np_merge_fwd(xs, kind)                # maximum / minimum: the first input that attains the result
        found = np.zeros(y.shape, dtype=bool)
        out = []
        for x in xs:
            hit = ~found & (x == y)
            out.append(np.where(hit, dy, T(0)))
            found |= hit
        return out


def relu_params(cls, args):
    """(alpha, max_value, theta) of the relu-family layer cls(*args)"""
    return getattr(L, cls)(*args).eltwise[1:]


def exact_values(rng, n):
    """odd multiples of 2^-7 with a standard deviation of 4: none equals a threshold or cap that is a multiple of 2^-6"""
    return ((2 * np.round(rng.standard_normal(n) * 256.0) + 1) * 2.0 ** -7).astype(np.float32)


def branch_shares(x, max_value, theta):
    """fractions of x on the negative side, on the linear part and above the cap"""
    x = np.asarray(x, np.float64)
    m = np.inf if max_value is None else max_value
    return float(np.mean(x <= theta)), float(np.mean((x > theta) & (x <= m))), float(np.mean(x > m))


# -- the restatements against autograd ---------------------------------------------------------------------------------------------- #
def _torch_act(x, kind, alpha, max_value, theta):
    F = torch.nn.functional
    if kind == 'relu':
        cap = x if max_value is None else torch.clamp(x, max=max_value)
        return torch.where(x > theta, cap, alpha * (x - theta))
    return {'elu': lambda: F.elu(x, alpha), 'selu': lambda: F.selu(x), 'sigmoid': lambda: torch.sigmoid(x),
            'hard_sigmoid': lambda: torch.clamp(0.2 * x + 0.5, 0.0, 1.0), 'softplus': lambda: F.softplus(x, threshold=1e9),
            'softsign': lambda: F.softsign(x), 'tanh': lambda: torch.tanh(x)}[kind]()


ACT_CASES = [('relu', 0.3, None, 0.0), ('relu', 0.1, 10.0, 0.0), ('relu', 0.1, 3.0, 0.5), ('relu', 0.0, None, 1.0),
             ('relu', 0.0, None, 0.0), ('elu', 1.0, None, 0.0), ('elu', 0.7, None, 0.0)] + [(k, 0.0, None, 0.0) for k in KINDS[2:]]


@pytest.mark.parametrize('case', ACT_CASES, ids=lambda c: '%s-%s-%s-%s' % c)
def test_activation_restatements_against_autograd(case):
    kind, alpha, max_value, theta = case
    rng = np.random.RandomState(3)
    x = 3.0 * rng.randn(4001)
    kinks = [0.0, theta, 2.5, -2.5] + ([max_value] if max_value is not None else [])
    x = x[np.all([np.abs(x - k) > 1e-3 for k in kinks], axis=0)]               # away from the kinks
    dy = rng.randn(x.size)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = _torch_act(xt, kind, alpha, max_value, theta)
    yt.backward(torch.tensor(dy))
    assert np.abs(np_act_fwd(x, kind, alpha, max_value, theta) - yt.detach().numpy()).max() <= 1e-12
    assert np.abs(np_act_bwd(x, dy, kind, alpha, max_value, theta) - xt.grad.numpy()).max() <= 1e-12


def test_softplus_and_sigmoid_stay_finite_and_correct_far_out():
    x = np.array([-100.0, -20.0, 20.0, 100.0])
    assert np.allclose(np_act_fwd(x, 'softplus'), [np.exp(-100.0), np.log1p(np.exp(-20.0)), 20.0 + np.log1p(np.exp(-20.0)), 100.0],
                       rtol=1e-15, atol=0)
    assert np.allclose(np_act_fwd(x, 'sigmoid'), [np.exp(-100.0), 1 / (1 + np.exp(20.0)), 1 / (1 + np.exp(-20.0)), 1.0], rtol=1e-15)
    for dt in (np.float32, np.float64):
        for kind in ('softplus', 'sigmoid'):
            assert np.isfinite(np_act_fwd(x.astype(dt), kind)).all() and np.isfinite(np_act_slope(x.astype(dt), kind)).all()


@pytest.mark.parametrize('kind', MERGES)
@pytest.mark.parametrize('n_src', [2, 3, 4])
def test_merge_restatements_against_autograd(kind, n_src):
    if kind == 'subtract' and n_src != 2:
        return
    rng = np.random.RandomState(5)
    xs = [rng.randn(997) for _ in range(n_src)]
    dy = rng.randn(997)
    ts = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in xs]
    two = {'add': torch.add, 'average': torch.add, 'subtract': torch.sub, 'multiply': torch.mul, 'maximum': torch.maximum,
           'minimum': torch.minimum}[kind]
    y = two(ts[0], ts[1])
    for t in ts[2:]:
        y = two(y, t)
    if kind == 'average':
        y = y / n_src
    y.backward(torch.tensor(dy))
    assert np.abs(np_merge_fwd(xs, kind) - y.detach().numpy()).max() <= 1e-12
    for got, t in zip(np_merge_bwd(xs, dy, kind), ts):
        assert np.abs(got - t.grad.numpy()).max() <= 1e-12


def test_ties_and_nan_follow_the_table():
    f = np.float32
    x = np.array([0.5, 3.0, np.nan, -0.0, 0.0, -np.inf, np.inf], dtype=f)
    y = np_act_fwd(x, 'relu', 0.1, 3.0, 0.5)
    assert y[0] == 0 and y[1] == 3 and np.isnan(y[2]) and y[5] == -np.inf and y[6] == 3       # x == theta: the negative side
    d = np_act_slope(x, 'relu', 0.1, 3.0, 0.5)
    assert d[0] == f(0.1) and d[1] == 1 and np.isnan(d[2]) and d[6] == 0                       # x == m: derivative 1
    z = np_act_fwd(x, 'relu', 0.0, None, 1.0)                                                  # ThresholdedReLU: 0 below, also at -inf
    assert z[5] == 0 and np.isnan(z[2]) and z[6] == np.inf
    for kind in KINDS:
        assert np.isnan(np_act_fwd(np.array([np.nan], f), kind, 1.0)).all()
        assert np.isnan(np_act_bwd(np.array([np.nan], f), np.array([1.0], f), kind, 1.0)).all()
    a, b = np.array([1.0, np.nan, 2.0, 0.0], f), np.array([np.nan, 1.0, 2.0, -0.0], f)
    for kind, ref in (('maximum', np.maximum), ('minimum', np.minimum)):
        got = np_merge_fwd([a, b], kind)
        assert np.array_equal(np.isnan(got), np.isnan(ref(a, b))) and np.array_equal(got[2:], ref(a, b)[2:])
        g = np_merge_bwd([a[2:], b[2:]], np.array([5.0, 7.0], f), kind)                       # ties: the first input takes dy
        assert np.array_equal(g[0], [5.0, 7.0]) and np.array_equal(g[1], [0.0, 0.0])


def test_exact_inputs_reach_every_branch():
    """the input family of the exact GPU tests: standard deviation 4, no value on a threshold or cap, and with theta 0.5 and
    max_value 3 every one of the three branches holds at least 10 % (about 55 / 22 / 23 %)"""
    x = exact_values(np.random.default_rng(1), 4099)
    assert 3.6 < x.std() < 4.4
    for cls, args in RELU_LAYERS:
        alpha, max_value, theta = relu_params(cls, args)
        assert not np.any(x == np.float32(theta)) and (max_value is None or not np.any(x == np.float32(max_value)))
    shares = branch_shares(x, 3.0, 0.5)
    assert min(shares) >= 0.10 and abs(shares[0] - 0.55) < 0.03 and abs(shares[1] - 0.22) < 0.03 and abs(shares[2] - 0.23) < 0.03
    for cls, args in RELU_LAYERS:          # every branch a layer HAS is reached (ReLU(10, ...) caps 0.6 % of these inputs)
        alpha, max_value, theta = relu_params(cls, args)
        lo, mid, hi = branch_shares(x, max_value, theta)
        assert lo >= 0.10 and mid >= 0.10 and (max_value is None or hi > 0)


# -- the layers' surface ------------------------------------------------------------------------------------------------------------ #
def test_defaults_and_config_keys():
    def keys(lay):
        return sorted(set(lay.get_config()) - {'name', 'trainable'})
    a = L.Activation('relu')
    assert a.activation == 'relu' and keys(a) == ['activation'] and a.eltwise == ('relu', 0.0, None, 0.0)
    assert L.Activation(None).activation == 'linear' and L.Activation('linear').eltwise is None
    assert L.Activation('elu').eltwise == ('elu', 1.0, None, 0.0) and L.Activation('tanh').eltwise[0] == 'tanh'
    lk = L.LeakyReLU()
    assert lk.alpha == pytest.approx(0.3) and keys(lk) == ['alpha'] and lk.eltwise == ('relu', lk.alpha, None, 0.0)
    r = L.ReLU()
    assert (r.max_value, r.negative_slope, r.threshold) == (None, 0.0, 0.0) and keys(r) == ['max_value', 'negative_slope', 'threshold']
    r = L.ReLU(max_value=10, negative_slope=0.1)
    assert r.get_config()['max_value'] == 10.0 and r.eltwise == ('relu', 0.1, 10.0, 0.0)
    e = L.ELU()
    assert e.alpha == 1.0 and keys(e) == ['alpha'] and e.eltwise == ('elu', 1.0, None, 0.0)
    t = L.ThresholdedReLU()
    assert t.theta == 1.0 and keys(t) == ['theta'] and t.eltwise == ('relu', 0.0, None, 1.0)
    for cls in (L.Add, L.Subtract, L.Multiply, L.Average, L.Maximum, L.Minimum):
        lay = cls()
        assert keys(lay) == [] and lay.kind == cls.__name__.lower() and lay.count_params() == 0
        assert lay.compute_output_shape([(3, 4, 5), (3, 4, 5)]) == (3, 4, 5)
    for lay in (a, lk, r, e, t):
        assert lay.compute_output_shape((3, 4, 5)) == (3, 4, 5) and lay.count_params() == 0
    x0 = L.Input(shape=(2, 4, 6))
    for fn, cls in ((L.add, L.Add), (L.subtract, L.Subtract), (L.multiply, L.Multiply), (L.average, L.Average),
                    (L.maximum, L.Maximum), (L.minimum, L.Minimum)):
        out = fn([x0, x0], name='m_' + cls.__name__)
        assert isinstance(out.layer, cls) and out.shape == (2, 4, 6) and out.layer.name == 'm_' + cls.__name__


def test_refusals():
    with pytest.raises(NotImplementedError):
        L.ReLU(threshold=-1.0)
    with pytest.raises(NotImplementedError):
        L.ThresholdedReLU(theta=-0.5)
    with pytest.raises(NotImplementedError):
        L.ReLU(max_value=1.0, threshold=1.0)
    with pytest.raises(NotImplementedError):
        L.ReLU(max_value=0.0)
    for name in ('softmax', 'exponential'):
        with pytest.raises(NotImplementedError):
            L.Activation(name)
    with pytest.raises(NotImplementedError):
        L.PReLU()
    with pytest.raises(NotImplementedError):
        L.Softmax()
    with pytest.raises(ValueError):
        L.Activation('no_such_function')
    x0 = L.Input(shape=(2, 4, 6))
    with pytest.raises(NotImplementedError):
        L.Add()([x0] * 5)
    with pytest.raises(ValueError):
        L.Add()([x0, L.Input(shape=(2, 4, 7))])
    with pytest.raises(ValueError):
        L.Subtract()([x0, x0, x0])
    with pytest.raises(ValueError):
        L.Add()([x0])
    # the activation= arguments of the weighted layers stay as they were
    with pytest.raises(NotImplementedError):
        L.Dense(4, activation='sigmoid')
    with pytest.raises(NotImplementedError):
        L.Conv2D(4, 3, activation='elu', **CF)
    net = Sequential(device=CPU)
    net.add(L.Conv2D(4, 3, padding='same', input_shape=(2, 4, 6), **CF))
    net.add(L.LeakyReLU(0.1, name='leaky'))
    with pytest.raises(NotImplementedError, match='leaky'):
        net.set_activation_dtype('bfloat16')


# -- lowering ------------------------------------------------------------------------------------------------------------------------ #
def test_sequential_conv_bn_activation_plan():
    net = Sequential(device=CPU)
    net.add(L.Conv2D(8, 3, padding='same', input_shape=(4, 8, 12), **CF))
    net.add(L.BatchNormalization(axis=1))
    net.add(L.LeakyReLU(0.1))
    net.add(L.Activation('linear'))
    net.add(L.Conv2D(4, 3, padding='same', **CF))
    for plan in (net.plan, net.infer_plan):
        assert [op.kind for op in plan.ops] == ['conv', 'bn', 'act', 'conv']          # Activation('linear') adds no op
        conv, bn, act, last = plan.ops
        assert act.src == bn.dst and last.src == act.dst and act.dst >= 0 and act.dst != act.src and act.xs == (8, 8, 12)
        assert act.layer is net.layers[2] and plan.eltwise_layers == [net.layers[2]]


def residual_block(cs=(4, 8, 12)):
    x0 = L.Input(shape=cs)
    skip = L.Conv2D(8, 3, padding='same', **CF)(x0)
    act = L.ReLU(max_value=10, negative_slope=0.1)
    t = act(L.Conv2D(8, 3, padding='same', **CF)(act(skip)))                           # one stateless layer, applied twice
    t = L.Add()([t, skip])
    return x0, L.Conv2D(cs[0], 3, padding='same', **CF)(t)


def test_functional_residual_block_plan():
    x0, out = residual_block()
    m = Model(inputs=x0, outputs=out, device=CPU)
    for plan in (m.plan, m.infer_plan):
        assert [op.kind for op in plan.ops] == ['conv', 'act', 'conv', 'act', 'merge', 'conv']
        c1, a1, c2, a2, add, c3 = plan.ops
        assert a1.layer is a2.layer and plan.eltwise_layers == [a1.layer, add.layer]
        assert (add.src,) + tuple(add.aux) == (a2.dst, c1.dst) and c3.src == add.dst and add.xs == (8, 8, 12)
        assert len({c1.dst, a1.dst, c2.dst, a2.dst, add.dst}) == 5                     # the training plan keeps every input
    # a merge as the model output writes the output slot; a view behind Flatten is merged flat
    x0 = L.Input(shape=(2, 4, 6))
    f = L.Flatten()(L.Conv2D(2, 3, padding='same', **CF)(x0))
    d = L.Dense(48)(f)
    m = Model(inputs=x0, outputs=L.maximum([d, f, L.ELU()(d)]), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['conv', 'dense', 'act', 'merge']
    conv, dense, elu, mx = m.plan.ops
    assert mx.dst == -2 and (mx.src,) + tuple(mx.aux) == (dense.dst, conv.dst, elu.dst) and m.plan.output_shapes == [(48,)]


# -- model specification and the import shim ----------------------------------------------------------------------------------------- #
def test_specification_round_trip_of_every_class():
    from dlwp_amd import serialization as S
    x0 = L.Input(shape=(2, 4, 6))
    t = L.Conv2D(2, 3, padding='same', **CF)(x0)
    acts = [L.Activation('softplus'), L.Activation('linear'), L.LeakyReLU(0.2), L.ReLU(6.0, 0.05, 0.25), L.ELU(0.5),
            L.ThresholdedReLU(0.75)]
    for a in acts:
        t = a(t)
    merges = [L.Add(), L.Subtract(), L.Multiply(), L.Average(), L.Maximum(), L.Minimum()]
    for mg in merges:
        t = mg([t, x0] if isinstance(mg, L.Subtract) else [t, x0, t])
    m = Model(inputs=x0, outputs=t, device=CPU)
    arch, _, _ = S.describe(m)
    arch = json.loads(json.dumps(arch))                                                # what travels to the ranks
    by_class = {l['class']: l['config'] for l in arch['layers']}
    assert by_class['ReLU'] == {'name': acts[3].name, 'max_value': 6.0, 'negative_slope': 0.05, 'threshold': 0.25}
    assert by_class['LeakyReLU']['alpha'] == pytest.approx(0.2) and by_class['ThresholdedReLU']['theta'] == 0.75
    assert by_class['Add'] == {'name': merges[0].name}
    for lay in acts + merges:
        spec = S._keras_layer_spec(lay)
        assert spec['class_name'] == type(lay).__name__
        again = type(lay)(**S._keras_layer_kwargs(type(lay), spec['config']))
        assert again.get_config() == lay.get_config()
        if isinstance(lay, L._Merge):
            assert sorted(spec['config']) == ['name', 'trainable']
    config, _ = S.keras_model_config(m)
    add = [sp for sp in config['config']['layers'] if sp['class_name'] == 'Add'][0]
    assert [len(node) for node in add['inbound_nodes']] == [3] and add['inbound_nodes'][0][1][0] == x0.layer.name


def test_model_files_round_trip_on_the_host(tmp_path):
    from dlwp_amd import serialization as S
    x0, out = residual_block()
    m = Model(inputs=x0, outputs=out, device=CPU, seed=2)
    for fmt in ('npz', 'keras'):
        path = str(tmp_path / ('m.' + fmt))
        S.save_model_file(m, path, format=fmt)
        m2 = S.load_model_file(path, device=CPU)
        assert [type(l).__name__ for l in m2.layers] == [type(l).__name__ for l in m.layers]
        assert [l.get_config() for l in m2.layers[1:]] == [l.get_config() for l in m.layers[1:]]
        assert [(op.kind, op.src, op.dst, op.aux if op.kind == 'merge' else None) for op in m2.plan.ops] == \
            [(op.kind, op.src, op.dst, op.aux if op.kind == 'merge' else None) for op in m.plan.ops]
        assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))


def test_import_shim():
    import dlwp_amd.compat  # noqa: F401
    from keras.layers import Activation, Add, LeakyReLU, add  # noqa: F401
    from keras.layers.advanced_activations import ELU, ReLU, ThresholdedReLU  # noqa: F401
    from keras.layers.merge import Maximum, average, concatenate  # noqa: F401
    assert LeakyReLU is L.LeakyReLU and Add is L.Add and add is L.add and ReLU is L.ReLU and average is L.average


def test_abi_descriptors_match_the_header():
    import ctypes
    from dlwp_amd import _lib
    assert ctypes.sizeof(_lib.Activation) == 16 and ctypes.sizeof(_lib.Merge) == 8
    from dlwp_amd import ops
    d = ops.activation_desc('relu', 0.1, None, 0.5)
    assert d.kind == _lib.ELT_RELU and d.max_value == float('inf') and d.theta == 0.5
    assert sorted(ops.MERGE_KINDS) == sorted(MERGES) and sorted(ops.ELT_KINDS) == sorted(KINDS)
