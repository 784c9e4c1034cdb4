"""AveragePooling2D(2) on the host: the constructor, the lowering (always one 'avgpool' launch of its own, never a pooled source mode
or a convolution epilogue), bfloat16 buffer pairing, both model-file formats, the Keras import shim and the C ABI."""
import json

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd import plan as P
from dlwp_amd.engine import Model, Sequential

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')


# -- constructor --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('pool', [2, (2, 2)])
@pytest.mark.parametrize('strides', [None, 2, (2, 2)])
def test_constructor_accepts_what_max_pooling_accepts(pool, strides):
    lay = L.AveragePooling2D(pool, strides=strides, padding='valid', **CF)
    assert (lay.pool_size, lay.strides, lay.padding, lay.data_format) == ((2, 2), (2, 2), 'valid', 'channels_first')
    assert lay.compute_output_shape((3, 5, 7)) == (3, 2, 3)
    assert lay.weights == [] and lay.count_params() == 0
    cfg = lay.get_config()
    assert {k: cfg[k] for k in ('pool_size', 'strides', 'padding', 'data_format')} == {
        'pool_size': (2, 2), 'strides': (2, 2), 'padding': 'valid', 'data_format': 'channels_first'}


@pytest.mark.parametrize('args, kw, text', [
    ((3,), dict(CF), 'only pool_size=2'),
    ((2,), dict(CF, strides=1), 'only pool_size=2'),
    ((2,), dict(CF, padding='same'), 'only pool_size=2'),
    ((2,), dict(data_format='channels_last'), 'channels_first'),
    ((2,), dict(), 'channels_first'),                                     # Keras' default data format is channels_last
])
def test_constructor_refuses_the_rest_like_max_pooling(args, kw, text):
    with pytest.raises(NotImplementedError, match='AveragePooling2D.*' + text):
        L.AveragePooling2D(*args, **kw)
    with pytest.raises(NotImplementedError, match='MaxPooling2D.*' + text):
        L.MaxPooling2D(*args, **kw)


# -- lowering ------------------------------------------------------------------------------------------------------------------------ #
def unet(pool_cls, cs=(4, 8, 12)):
    from dlwp_amd.custom import PeriodicPadding2D

    def pads(t):
        return L.ZeroPadding2D(((1, 1), (0, 0)), **CF)(PeriodicPadding2D(((0, 0), (1, 1)), **CF)(t))
    x0 = L.Input(shape=cs)
    skip = L.Conv2D(8, 3, activation='tanh', **CF)(pads(x0))
    t = L.Conv2D(16, 3, activation='tanh', **CF)(pads(pool_cls(2, **CF)(skip)))
    t = L.concatenate([L.UpSampling2D(2, **CF)(t), skip], axis=1)
    return x0, L.Conv2D(cs[0], 3, **CF)(pads(t))


def test_one_avgpool_op_per_layer_and_nothing_fused():
    x0, out = unet(L.AveragePooling2D)
    m = Model(inputs=x0, outputs=out, device=CPU)
    for plan in (m.plan, m.infer_plan):
        pools = [op for op in plan.ops if op.kind == 'avgpool']
        assert len(pools) == 1 and 'maxpool' not in {op.kind for op in plan.ops}
        pool = pools[0]
        convs = [op for op in plan.ops if op.kind == 'conv']
        assert pool.src == convs[0].dst and pool.dst >= 0 and pool.dst != pool.src
        assert pool.xs == (8, 8, 12) and pool.out_shape == (8, 4, 6) and plan.buffers[pool.dst] == (8, 4, 6)
        assert convs[1].src == pool.dst and convs[1].xs == (8, 4, 6)
        assert not any(op.out_pool for op in plan.ops)
        assert not any(op.src_mode == P.SRC_MAXPOOL2 for op in plan.ops)
        assert plan.buffers[convs[0].dst] == (8, 8, 12)                   # the pre-pooling tensor is stored in both plans


def test_max_pooling_twin_keeps_its_plan():
    """the same net with MaxPooling2D lowers as before: the pooling in the producer's epilogue or the consumer's loader in the
    inference plan (no standalone launch there unless the library asks for one), a pooled source or a 'maxpool' op in training"""
    x0, out = unet(L.MaxPooling2D)
    m = Model(inputs=x0, outputs=out, device=CPU)
    for plan in (m.plan, m.infer_plan):
        assert 'avgpool' not in {op.kind for op in plan.ops}
        pooled = [op for op in plan.ops if op.out_pool or op.src_mode == P.SRC_MAXPOOL2 or op.kind == 'maxpool']
        assert len(pooled) == 1
    x0, out = unet(L.AveragePooling2D)
    a = Model(inputs=x0, outputs=out, device=CPU)
    assert len(a.plan.ops) >= len(m.plan.ops) and len(a.infer_plan.ops) >= len(m.infer_plan.ops)


def test_two_layers_two_ops_an_odd_edge_and_a_lazy_source_in_front():
    net = Sequential(device=CPU)
    net.add(L.Conv2D(8, 3, padding='same', input_shape=(4, 7, 9), **CF))
    net.add(L.AveragePooling2D(2, **CF))
    net.add(L.UpSampling2D(2, **CF))
    net.add(L.AveragePooling2D((2, 2), strides=(2, 2), **CF))          # reads a lazy up-sampling: materialised first
    net.add(L.Conv2D(4, 3, padding='same', **CF))
    for plan in (net.plan, net.infer_plan):
        assert [op.kind for op in plan.ops] == ['conv', 'avgpool', 'upsample', 'avgpool', 'conv']
        c1, p1, up, p2, c2 = plan.ops
        assert p1.xs == (8, 7, 9) and p1.out_shape == (8, 3, 4) and p2.xs == (8, 6, 8) and p2.out_shape == (8, 3, 4)
        assert (p1.src, up.src, p2.src, c2.src) == (c1.dst, p1.dst, up.dst, p2.dst)
        assert all(op.src_mode == P.SRC_DIRECT and not op.out_pool for op in plan.ops)
        assert plan.output_shapes == [(4, 3, 4)]


def test_channel_window_in_front_and_the_output_slot_as_target():
    from dlwp_amd.custom import slice_layer
    x0 = L.Input(shape=(4, 8, 12))
    m = Model(inputs=x0, outputs=L.AveragePooling2D(2, **CF)(slice_layer(1, 3, axis=1)(x0)), device=CPU)
    for plan in (m.plan, m.infer_plan):
        assert [op.kind for op in plan.ops] == ['copy', 'avgpool']
        cp, pool = plan.ops
        assert cp.src == P.STATE_IN and (cp.in_c_off, cp.in_c_total, cp.xs[0]) == (1, 4, 2)
        assert pool.src == cp.dst and pool.dst == P.OUT(0) and pool.xs == (2, 8, 12)
        assert plan.output_store == [(2, 4, 6)] and plan.output_shapes == [(2, 4, 6)]


def test_reshaped_tensor_is_refused_like_max_pooling():
    for cls in (L.AveragePooling2D, L.MaxPooling2D):
        x0 = L.Input(shape=(2, 2, 8, 12))
        with pytest.raises(NotImplementedError, match='on a reshaped tensor'):
            Model(inputs=x0, outputs=cls(2, **CF)(x0), device=CPU).plan       # a (T, C, H, W) tensor


def test_bf16_buffers_pair_source_and_destination():
    def net(tail):
        s = Sequential(device=CPU)
        s.add(L.Conv2D(8, 3, padding='same', input_shape=(4, 16, 24), **CF))
        s.add(L.AveragePooling2D(2, **CF))
        for lay in tail:
            s.add(lay)
        return s
    # conv -> avgpool -> conv: the convolution's output and its pooled image are bf16 together
    plan = net([L.Conv2D(4, 3, padding='same', **CF)]).infer_plan
    conv, pool, _ = plan.ops
    assert plan.bf16_buffers() == sorted([conv.dst, pool.dst])
    # the pooled tensor is the model output (float32): its source stays float32 as well
    plan = net([]).infer_plan
    conv, pool = plan.ops
    assert pool.dst == P.OUT(0) and plan.bf16_buffers() == []
    # a float32-only reader of the pooled buffer (up-sampling kernel) keeps both float32
    plan = net([L.UpSampling2D(2, **CF), L.AveragePooling2D(2, **CF), L.Conv2D(4, 3, padding='same', **CF)]).infer_plan
    assert [op.kind for op in plan.ops] == ['conv', 'avgpool', 'upsample', 'avgpool', 'conv']
    conv, p1, up, p2, _ = plan.ops
    assert plan.bf16_buffers() == []      # p1's image is float32, so its source is; p2 reads the float32 up-sampled buffer
    # the model input as source
    x0 = L.Input(shape=(4, 16, 24))
    m = Model(inputs=x0, outputs=L.Conv2D(4, 3, padding='same', **CF)(L.AveragePooling2D(2, **CF)(x0)), device=CPU)
    pool, conv = m.infer_plan.ops
    assert pool.src == P.STATE_IN and m.infer_plan.bf16_buffers() == []


# -- model files, build_model, the import shim --------------------------------------------------------------------------------------- #
def test_native_config_and_keras_description_round_trip():
    from dlwp_amd import serialization as S
    lay = L.AveragePooling2D(2, name='the_pool', **CF)
    assert S._layer_config(lay) == {'name': 'the_pool', 'data_format': 'channels_first'}
    spec = json.loads(json.dumps(S._keras_layer_spec(lay)))
    twin = S._keras_layer_spec(L.MaxPooling2D(2, name='the_pool', **CF))
    assert spec['class_name'] == 'AveragePooling2D' and spec['config'] == twin['config']
    assert spec['config'] == {'name': 'the_pool', 'trainable': True, 'pool_size': [2, 2], 'padding': 'valid', 'strides': [2, 2],
                              'data_format': 'channels_first'}
    again = L.AveragePooling2D(**S._keras_layer_kwargs(L.AveragePooling2D, spec['config']))
    assert again.get_config() == lay.get_config()


def test_keras_layout_config_builds_the_layer_without_a_warning():
    import warnings
    from dlwp_amd import serialization as S
    cfg = {'name': 'average_pooling2d_1', 'trainable': True, 'pool_size': [2, 2], 'padding': 'valid', 'strides': [2, 2],
           'data_format': 'channels_first'}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        lay = L.AveragePooling2D(**S._keras_layer_kwargs(L.AveragePooling2D, cfg))
    assert lay.name == 'average_pooling2d_1' and lay.pool_size == (2, 2) and lay.strides == (2, 2)
    with pytest.raises(NotImplementedError):
        L.AveragePooling2D(**S._keras_layer_kwargs(L.AveragePooling2D, dict(cfg, pool_size=[3, 3], strides=[3, 3])))


def test_model_files_round_trip_on_the_host(tmp_path):
    from dlwp_amd import serialization as S
    x0, out = unet(L.AveragePooling2D)
    m = Model(inputs=x0, outputs=out, device=CPU, seed=2)
    for fmt in ('npz', 'keras'):
        path = str(tmp_path / ('m.' + fmt))
        S.save_model_file(m, path, format=fmt)
        m2 = S.load_model_file(path, device=CPU)
        assert [type(l).__name__ for l in m2.layers] == [type(l).__name__ for l in m.layers]
        assert 'AveragePooling2D' in [type(l).__name__ for l in m2.layers]
        assert [(op.kind, op.src, op.dst, op.xs) for op in m2.plan.ops] == [(op.kind, op.src, op.dst, op.xs) for op in m.plan.ops]
        assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))


def test_build_model_takes_the_layer_by_name():
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model((('Conv2D', (8, 3), dict(CF, padding='same', activation='tanh', input_shape=(4, 8, 12))),
                   ('AveragePooling2D', (2,), dict(CF)),
                   ('UpSampling2D', (2,), dict(CF)),
                   ('Conv2D', (4, 3), dict(CF, padding='same'))), loss='mse', optimizer='adam')
    assert [type(l).__name__ for l in d.model.layers if not isinstance(l, L.InputLayer)] == \
        ['Conv2D', 'AveragePooling2D', 'UpSampling2D', 'Conv2D']
    assert [op.kind for op in d.model.plan.ops].count('avgpool') == 1


def test_import_shim():
    import dlwp_amd.compat  # noqa: F401
    from keras.layers import AveragePooling2D, MaxPooling2D
    assert AveragePooling2D is L.AveragePooling2D and MaxPooling2D is L.MaxPooling2D


# -- C ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_entry_points_are_exported_declared_and_bound():
    import re
    from dlwp_amd import _lib
    names = _lib.declared_symbols()
    for n in ('dlwp_avgpool2_fwd', 'dlwp_avgpool2_bwd'):
        assert n in names and hasattr(_lib.lib, n)
        assert len(getattr(_lib.lib, n).argtypes) == 6
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r'#define\s+DLWP_OP_AVGPOOL2\s+14\b', header) and _lib.OP_AVGPOOL2 == 14
    assert _lib.OP_MERGE == 13 and _lib.OP_MAXPOOL2 == 2                 # appended: no existing value moved
