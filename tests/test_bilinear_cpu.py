"""UpSampling2D(2, interpolation='bilinear') on the host: the constructor, the lowering (always one 'bilinear' launch of its own, never a
lazy up-sampled source, a restated decoder layer or a convolution epilogue), bfloat16 buffer pairing, both model-file formats, the
Keras import shim, the C ABI, and the numpy float32 restatements of the kernels' arithmetic (which tests/test_gpu_bilinear.py holds
the kernels to, bit for bit) against the float64 interpolation matrices."""
import json

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd import plan as P
from dlwp_amd.engine import Model, Sequential

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')
HALF = np.float32(0.5)


# -- restatements -------------------------------------------------------------------------------------------------------------------- #
def np_mid(a, b):
    """a + (b - a) * 0.5f: a subtraction, a product and an addition, each rounded once (numpy float32 is IEEE)"""
    return a + (b - a) * HALF


def np_fwd(x):
    """the stated float32 expression: the row pass, then the column pass; even positions copy the bits"""
    x = np.asarray(x, np.float32)
    n, c, h, w = x.shape
    r = np.empty((n, c, h, 2 * w), np.float32)
    r[..., 0::2] = x
    r[..., 1::2] = np_mid(x, x[..., np.minimum(np.arange(w) + 1, w - 1)])
    y = np.empty((n, c, 2 * h, 2 * w), np.float32)
    y[:, :, 0::2] = r
    y[:, :, 1::2] = np_mid(r, r[:, :, np.minimum(np.arange(h) + 1, h - 1)])
    return y


def np_g(v):
    """the adjoint along the last axis, length 2W -> W: (v[2j] + h*v[2j-1]) + h*v[2j+1], the v[2j-1] term absent at j = 0 and the
    last term v[2W-1] with weight 1 at j = W-1"""
    v = np.asarray(v, np.float32)
    w = v.shape[-1] // 2
    s = v[..., 0::2].copy()
    if w > 1:
        s[..., 1:] = s[..., 1:] + HALF * v[..., 1:2 * w - 2:2]
    e = HALF * v[..., 1::2]
    e[..., w - 1] = v[..., 2 * w - 1]
    return s + e


def np_bwd(dy, shape):
    """g along the rows of dy, then g down the columns of the result"""
    n, c, h, w = shape
    t = np_g(np.asarray(dy, np.float32).reshape(n, c, 2 * h, 2 * w))
    return np.ascontiguousarray(np.swapaxes(np_g(np.swapaxes(t, -1, -2)), -1, -2))


def matrix(w):
    """the (2w, w) float64 interpolation matrix of one axis: every row sums to 1"""
    a = np.zeros((2 * w, w))
    for j in range(w):
        a[2 * j, j] = 1.0
        a[2 * j + 1, j] += 0.5
        a[2 * j + 1, min(j + 1, w - 1)] += 0.5
    return a


def fwd64(x):
    x = np.asarray(x, np.float64)
    return np.einsum('ri,ncij,sj->ncrs', matrix(x.shape[2]), x, matrix(x.shape[3]))


def bwd64(dy, shape):
    dy = np.asarray(dy, np.float64).reshape(shape[0], shape[1], 2 * shape[2], 2 * shape[3])
    return np.einsum('ri,ncrs,sj->ncij', matrix(shape[2]), dy, matrix(shape[3]))


#: an output passes through two levels of (subtract, halve, add) / (halve, add, add): the halving is exact in the normal range, so
#: four roundings of relative size 2^-24, each of a quantity no larger than the same interpolation (or adjoint) of the absolute
#: values; 2^-20 covers the second-order terms
ROUNDING = 4 * 2.0 ** -24 * (1 + 2.0 ** -20)

MAPS = [(1, 1), (1, 5), (4, 1), (5, 7), (4, 8), (3, 4), (7, 12)]


def reals(shape, seed):
    """normal float32 values over a few decades, both signs (|x| > 1e-30: halving is exact)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


@pytest.mark.parametrize('hw', MAPS, ids=['%dx%d' % m for m in MAPS])
def test_restatements_against_the_float64_matrices(hw):
    shape = (2, 3) + hw
    assert all(matrix(k).sum(axis=1).tolist() == [1.0] * (2 * k) for k in hw)
    x = reals(shape, 1)
    y = np_fwd(x)
    assert y.dtype == np.float32 and y.shape == (2, 3, 2 * hw[0], 2 * hw[1])
    assert np.array_equal(y[:, :, 0::2, 0::2].view(np.uint32), x.view(np.uint32))          # the bits are copied
    assert np.array_equal(y[:, :, -1, :].view(np.uint32), y[:, :, -2, :].view(np.uint32))  # the clamped last row: t + (t - t) * h = t
    assert np.array_equal(y[:, :, :, -1].view(np.uint32), y[:, :, :, -2].view(np.uint32))
    err, bound = np.abs(y.astype(np.float64) - fwd64(x)), ROUNDING * fwd64(np.abs(x))
    assert (err <= bound).all(), float((err / bound).max())
    dy = reals(y.shape, 2)
    dx = np_bwd(dy, shape)
    assert dx.dtype == np.float32 and dx.shape == shape
    err, bound = np.abs(dx.astype(np.float64) - bwd64(dy, shape)), ROUNDING * bwd64(np.abs(dy), shape)
    assert (err <= bound).all(), float((err / bound).max())
    # small integers are exact: halves and quarters of them are float32 numbers
    rng = np.random.default_rng(3)
    xi, di = rng.integers(-64, 65, shape).astype(np.float32), (4 * rng.integers(-32, 33, y.shape)).astype(np.float32)
    assert np.array_equal(np_fwd(xi).astype(np.float64), fwd64(xi))
    assert np.array_equal(np_bwd(di, shape).astype(np.float64), bwd64(di, shape))
    assert (np_fwd(xi).astype(np.float64) * di).sum() == (xi.astype(np.float64) * np_bwd(di, shape)).sum()      # the adjoint


def test_restatement_edges_one_column_and_infinities():
    assert np_g(np.array([3.0, 5.0], np.float32)).tolist() == [8.0]                                     # W = 1: v[0] + v[1]
    assert np_g(np.array([1.0, 2.0, 4.0, 8.0], np.float32)).tolist() == [2.0, 13.0]                     # 1 + 2/2;  (4 + 2/2) + 8
    with np.errstate(invalid='ignore'):
        y = np_fwd(np.array([[[[1.0, np.inf]]]], np.float32))
    assert y[0, 0, 0].tolist()[:3] == [1.0, np.inf, np.inf] and np.isnan(y[0, 0, 0, 3])                # inf + (inf - inf) * h


# -- constructor --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('size', [2, (2, 2)])
@pytest.mark.parametrize('interpolation', ['nearest', 'bilinear'])
def test_constructor_accepts_both_interpolations(size, interpolation):
    lay = L.UpSampling2D(size, interpolation=interpolation, **CF)
    assert (lay.size, lay.data_format, lay.interpolation) == ((2, 2), 'channels_first', interpolation)
    assert lay.compute_output_shape((3, 5, 7)) == (3, 10, 14)
    assert lay.weights == [] and lay.count_params() == 0
    cfg = lay.get_config()
    assert {k: cfg[k] for k in ('size', 'data_format', 'interpolation')} == {
        'size': (2, 2), 'data_format': 'channels_first', 'interpolation': interpolation}
    assert L.UpSampling2D(2, **CF).interpolation == 'nearest'


@pytest.mark.parametrize('args, kw, exc, text', [
    ((3,), dict(CF, interpolation='bilinear'), NotImplementedError, 'only size=2'),
    ((3,), dict(CF), NotImplementedError, 'only size=2'),
    (((2, 1),), dict(CF, interpolation='bilinear'), NotImplementedError, 'only size=2'),
    ((2,), dict(data_format='channels_last', interpolation='bilinear'), NotImplementedError, 'channels_first'),
    ((2,), dict(interpolation='bilinear'), NotImplementedError, 'channels_first'),      # Keras' default data format is channels_last
    ((2,), dict(CF, interpolation='bicubic'), ValueError, 'interpolation'),
    ((2,), dict(CF, interpolation='Bilinear'), ValueError, 'interpolation'),
    ((2,), dict(CF, interpolation=None), ValueError, 'interpolation'),
])
def test_constructor_refuses_the_rest(args, kw, exc, text):
    with pytest.raises(exc, match=text):
        L.UpSampling2D(*args, **kw)


# -- lowering ------------------------------------------------------------------------------------------------------------------------ #
def unet(interpolation, cs=(4, 8, 12)):
    from dlwp_amd.custom import PeriodicPadding2D

    def pads(t):
        return L.ZeroPadding2D(((1, 1), (0, 0)), **CF)(PeriodicPadding2D(((0, 0), (1, 1)), **CF)(t))
    x0 = L.Input(shape=cs)
    skip = L.Conv2D(8, 3, activation='tanh', **CF)(pads(x0))
    t = L.Conv2D(16, 3, activation='tanh', **CF)(pads(L.MaxPooling2D(2, **CF)(skip)))
    t = L.concatenate([L.UpSampling2D(2, interpolation=interpolation, **CF)(t), skip], axis=1)
    return x0, L.Conv2D(cs[0], 3, **CF)(pads(t))


def test_one_bilinear_op_per_layer_and_nothing_lazy():
    x0, out = unet('bilinear')
    m = Model(inputs=x0, outputs=out, device=CPU)
    for plan in (m.plan, m.infer_plan):
        ups = [op for op in plan.ops if op.kind == 'bilinear']
        assert len(ups) == 1 and 'upsample' not in {op.kind for op in plan.ops}
        up = ups[0]
        convs = [op for op in plan.ops if op.kind == 'conv']
        assert up.src == convs[1].dst and up.dst >= 0 and up.dst != up.src
        assert up.xs == (16, 4, 6) and up.out_shape == (16, 8, 12) and plan.buffers[up.dst] == (16, 8, 12)
        assert plan.buffers[up.src] == (16, 4, 6)                         # the decoder layer in front is not restated
        assert not any(op.src_mode == P.SRC_UPSAMPLE2 for op in plan.ops)
        assert up.src_mode == P.SRC_DIRECT and not up.out_pool
        readers = [op for op in plan.ops if op.src == up.dst]
        assert len(readers) == 1 and readers[0].kind == 'copy'            # the concatenation reads the stored image


def test_nearest_twin_keeps_its_plan():
    """the same net with the default interpolation lowers as before: no 'bilinear' op, the up-sampling a lazy source of what reads
    it or one 'upsample' launch"""
    x0, out = unet('nearest')
    m = Model(inputs=x0, outputs=out, device=CPU)
    x0, out = unet('bilinear')
    b = Model(inputs=x0, outputs=out, device=CPU)
    for plan, twin in ((m.plan, b.plan), (m.infer_plan, b.infer_plan)):
        kinds = [op.kind for op in plan.ops]
        assert 'bilinear' not in kinds and set(kinds) <= {'conv', 'maxpool', 'upsample', 'copy', 'pad', 'phasew'}
        up = [op for op in plan.ops if op.src_mode == P.SRC_UPSAMPLE2 or op.kind == 'upsample']
        assert len(up) == 1
        assert [k for k in kinds if k != 'upsample'] == [op.kind for op in twin.ops if op.kind != 'bilinear']
    net = Sequential(device=CPU)
    net.add(L.Conv2D(8, 3, padding='same', input_shape=(4, 7, 9), **CF))
    net.add(L.MaxPooling2D(2, **CF))
    net.add(L.UpSampling2D(2, **CF))
    net.add(L.Conv2D(4, 3, padding='same', **CF))
    assert [(op.kind, op.src_mode) for op in net.plan.ops] == [('conv', 0), ('maxpool', 0), ('conv', P.SRC_UPSAMPLE2)]
    assert [(op.kind, op.src_mode, op.out_pool) for op in net.infer_plan.ops] == [('conv', 0, True), ('conv', P.SRC_UPSAMPLE2, False)]


def test_two_layers_two_ops_and_a_lazy_source_in_front():
    net = Sequential(device=CPU)
    net.add(L.Conv2D(8, 3, padding='same', input_shape=(4, 7, 9), **CF))
    net.add(L.UpSampling2D(2, interpolation='bilinear', **CF))
    net.add(L.MaxPooling2D(2, **CF))
    net.add(L.UpSampling2D((2, 2), interpolation='bilinear', **CF))    # reads a lazy max-pooling: materialised first
    net.add(L.Conv2D(4, 3, padding='same', **CF))
    for plan in (net.plan, net.infer_plan):
        assert [op.kind for op in plan.ops] == ['conv', 'bilinear', 'maxpool', 'bilinear', 'conv']
        c1, u1, mp, u2, c2 = plan.ops
        assert u1.xs == (8, 7, 9) and u1.out_shape == (8, 14, 18) and u2.xs == (8, 7, 9) and u2.out_shape == (8, 14, 18)
        assert (u1.src, mp.src, u2.src, c2.src) == (c1.dst, u1.dst, mp.dst, u2.dst)
        assert all(op.src_mode == P.SRC_DIRECT and not op.out_pool for op in plan.ops)
        assert plan.output_shapes == [(4, 14, 18)]
    # a lazy nearest up-sampling and a lazy halo in front are stored first as well
    from dlwp_amd.custom import PeriodicPadding2D
    x0 = L.Input(shape=(4, 4, 6))
    t = PeriodicPadding2D(((0, 0), (1, 1)), **CF)(L.UpSampling2D(2, **CF)(x0))
    m = Model(inputs=x0, outputs=L.UpSampling2D(2, interpolation='bilinear', **CF)(t), device=CPU)
    for plan in (m.plan, m.infer_plan):
        assert [op.kind for op in plan.ops] == ['upsample', 'pad', 'bilinear']
        assert plan.ops[2].xs == (4, 8, 14) and plan.ops[2].dst == P.OUT(0) and plan.output_shapes == [(4, 16, 28)]


def test_channel_window_in_front_and_the_output_slot_as_target():
    from dlwp_amd.custom import slice_layer
    x0 = L.Input(shape=(4, 8, 12))
    m = Model(inputs=x0, outputs=L.UpSampling2D(2, interpolation='bilinear', **CF)(slice_layer(1, 3, axis=1)(x0)), device=CPU)
    for plan in (m.plan, m.infer_plan):
        assert [op.kind for op in plan.ops] == ['copy', 'bilinear']
        cp, up = plan.ops
        assert cp.src == P.STATE_IN and (cp.in_c_off, cp.in_c_total, cp.xs[0]) == (1, 4, 2)
        assert up.src == cp.dst and up.dst == P.OUT(0) and up.xs == (2, 8, 12)
        assert plan.output_store == [(2, 16, 24)] and plan.output_shapes == [(2, 16, 24)]


def test_reshaped_tensor_is_refused():
    x0 = L.Input(shape=(2, 2, 8, 12))
    with pytest.raises(NotImplementedError, match='on a reshaped tensor'):
        Model(inputs=x0, outputs=L.UpSampling2D(2, interpolation='bilinear', **CF)(x0), device=CPU).plan       # a (T, C, H, W) tensor


def test_bf16_buffers_pair_source_and_destination():
    def net(tail, interpolation='bilinear'):
        s = Sequential(device=CPU)
        s.add(L.Conv2D(8, 3, padding='same', input_shape=(4, 16, 24), **CF))
        s.add(L.UpSampling2D(2, interpolation=interpolation, **CF))
        for lay in tail:
            s.add(lay)
        return s
    # conv -> bilinear -> conv: the convolution's output and its interpolated image are bf16 together
    plan = net([L.Conv2D(4, 3, padding='same', **CF)]).infer_plan
    conv, up, _ = plan.ops
    assert up.kind == 'bilinear' and plan.bf16_buffers() == sorted([conv.dst, up.dst])
    # the interpolated tensor is the model output (float32): its source stays float32 as well
    plan = net([]).infer_plan
    conv, up = plan.ops
    assert up.dst == P.OUT(0) and plan.bf16_buffers() == []
    # a float32-only reader of the interpolated buffer (a padding kernel in front of a pooling) keeps both float32
    plan = net([L.ZeroPadding2D(((1, 1), (1, 1)), **CF), L.AveragePooling2D(2, **CF), L.Conv2D(4, 3, padding='same', **CF)]).infer_plan
    assert [op.kind for op in plan.ops] == ['conv', 'bilinear', 'pad', 'avgpool', 'conv']
    assert plan.bf16_buffers() == []      # the padded buffer is float32, so the pooled one is; the interpolated one is read by 'pad'
    # the model input as source
    x0 = L.Input(shape=(4, 16, 24))
    m = Model(inputs=x0, outputs=L.Conv2D(4, 3, padding='same', **CF)(L.UpSampling2D(2, interpolation='bilinear', **CF)(x0)), device=CPU)
    up, conv = m.infer_plan.ops
    assert up.src == P.STATE_IN and m.infer_plan.bf16_buffers() == []
    # the nearest twin: as before, nothing an up-sampling kernel touches
    plan = net([L.Conv2D(4, 3, padding='same', **CF)], 'nearest').infer_plan
    assert 'bilinear' not in [op.kind for op in plan.ops]


# -- model files, build_model, the import shim --------------------------------------------------------------------------------------- #
def test_native_config_and_keras_description_round_trip():
    from dlwp_amd import serialization as S
    near, lay = L.UpSampling2D(2, name='the_up', **CF), L.UpSampling2D(2, name='the_up', interpolation='bilinear', **CF)
    # nearest: byte for byte what it always was
    assert json.dumps(S._layer_config(near)) == '{"name": "the_up", "data_format": "channels_first"}'
    assert json.dumps(S._keras_layer_spec(near)) == json.dumps(
        {'class_name': 'UpSampling2D', 'config': {'name': 'the_up', 'trainable': True, 'size': [2, 2], 'data_format': 'channels_first',
                                                  'interpolation': 'nearest'}})
    assert S._layer_config(lay) == {'name': 'the_up', 'data_format': 'channels_first', 'interpolation': 'bilinear'}
    spec = json.loads(json.dumps(S._keras_layer_spec(lay)))
    assert spec['class_name'] == 'UpSampling2D'
    assert spec['config'] == {'name': 'the_up', 'trainable': True, 'size': [2, 2], 'data_format': 'channels_first',
                              'interpolation': 'bilinear'}
    again = L.UpSampling2D(**S._keras_layer_kwargs(L.UpSampling2D, spec['config']))
    assert again.get_config() == lay.get_config() and again.interpolation == 'bilinear'
    assert L.UpSampling2D(**S._layer_config(lay)).get_config() == lay.get_config()
    assert L.UpSampling2D(**S._layer_config(near)).interpolation == 'nearest'


def test_keras_layout_config_builds_the_layer_without_a_warning():
    import warnings
    from dlwp_amd import serialization as S
    cfg = {'name': 'up_sampling2d_1', 'trainable': True, 'size': [2, 2], 'data_format': 'channels_first', 'interpolation': 'bilinear'}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        lay = L.UpSampling2D(**S._keras_layer_kwargs(L.UpSampling2D, cfg))
        near = L.UpSampling2D(**S._keras_layer_kwargs(L.UpSampling2D, dict(cfg, interpolation='nearest')))
    assert lay.name == 'up_sampling2d_1' and lay.size == (2, 2) and lay.interpolation == 'bilinear' and near.interpolation == 'nearest'
    with pytest.raises(NotImplementedError):
        L.UpSampling2D(**S._keras_layer_kwargs(L.UpSampling2D, dict(cfg, size=[3, 3])))
    with pytest.raises(ValueError):
        L.UpSampling2D(**S._keras_layer_kwargs(L.UpSampling2D, dict(cfg, interpolation='bicubic')))


def test_model_files_round_trip_on_the_host(tmp_path):
    from dlwp_amd import serialization as S
    for interpolation in ('bilinear', 'nearest'):
        x0, out = unet(interpolation)
        m = Model(inputs=x0, outputs=out, device=CPU, seed=2)
        for fmt in ('npz', 'keras'):
            path = str(tmp_path / ('m_%s.%s' % (interpolation, fmt)))
            S.save_model_file(m, path, format=fmt)
            m2 = S.load_model_file(path, device=CPU)
            assert [type(l).__name__ for l in m2.layers] == [type(l).__name__ for l in m.layers]
            assert [l.interpolation for l in m2.layers if isinstance(l, L.UpSampling2D)] == [interpolation]
            assert [(op.kind, op.src, op.dst, op.xs) for op in m2.plan.ops] == [(op.kind, op.src, op.dst, op.xs) for op in m.plan.ops]
            assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))


def test_build_model_takes_the_argument_by_name():
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model((('Conv2D', (8, 3), dict(CF, padding='same', activation='tanh', input_shape=(4, 8, 12))),
                   ('MaxPooling2D', (2,), dict(CF)),
                   ('UpSampling2D', (2,), dict(CF, interpolation='bilinear')),
                   ('Conv2D', (4, 3), dict(CF, padding='same'))), loss='mse', optimizer='adam')
    assert [type(l).__name__ for l in d.model.layers if not isinstance(l, L.InputLayer)] == \
        ['Conv2D', 'MaxPooling2D', 'UpSampling2D', 'Conv2D']
    assert [op.kind for op in d.model.plan.ops].count('bilinear') == 1


def test_import_shim():
    import dlwp_amd.compat  # noqa: F401
    from keras.layers import UpSampling2D
    assert UpSampling2D is L.UpSampling2D
    assert UpSampling2D(2, interpolation='bilinear', **CF).interpolation == 'bilinear'


# -- C ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_entry_points_are_exported_declared_and_bound():
    import re
    from dlwp_amd import _lib
    names = _lib.declared_symbols()
    for n in ('dlwp_upsample2_bilinear_fwd', 'dlwp_upsample2_bilinear_bwd'):
        assert n in names and hasattr(_lib.lib, n)
        assert len(getattr(_lib.lib, n).argtypes) == 6
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r'#define\s+DLWP_OP_BILINEAR2\s+15\b', header) and _lib.OP_BILINEAR2 == 15
    assert _lib.OP_AVGPOOL2 == 14 and _lib.OP_UPSAMPLE2 == 3                # appended: no existing value moved
