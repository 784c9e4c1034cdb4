"""Conv2D(strides=2) on the host: the restatement the kernels of csrc/sconv.hip implement (weight map + padded space-to-depth + one
stride-1 cross-correlation, tests/sconv_cases.py) against float64 torch, the layer's arguments and shapes, the lowering, the model
files and the C ABI's refusals that need no device."""
import ctypes
import json
import re

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd.engine import Model
from tests import sconv_cases as S

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')


# -- the layer ------------------------------------------------------------------------------------------------------------------------ #
def test_constructor_accepts_stride_one_and_two_only():
    lay = L.Conv2D(8, 3, strides=2, padding='same', activation='tanh', name='down', **CF)
    assert lay.strides == (2, 2) and lay.kernel_size == (3, 3)
    for st in ((2, 2), [2, 2], np.int64(2), (np.int32(2), np.int64(2))):
        assert L.Conv2D(8, 3, strides=st, **CF).strides == (2, 2)
    for st in (1, (1, 1), np.int64(1)):
        assert L.Conv2D(8, 3, strides=st, **CF).strides == (1, 1)
    for st in ((2, 1), (1, 2), 3, 0, (3, 3)):
        with pytest.raises(NotImplementedError, match=r'Conv2D.*strides=1 and strides=2'):
            L.Conv2D(8, 3, strides=st, **CF)
    with pytest.raises(ValueError):
        L.Conv2D(8, 3, strides=(2, 2, 2), **CF)
    with pytest.raises(ValueError, match='dilation_rate'):
        L.Conv2D(8, 3, strides=2, dilation_rate=2, **CF)
    assert L.Conv2D(8, 3, strides=1, dilation_rate=2, **CF).dilation_rate == (2, 2)
    cfg = lay.get_config()
    assert cfg['strides'] == (2, 2) and cfg['name'] == 'down'
    assert L.Conv2D(**cfg).get_config() == cfg


def test_a_stride_one_layer_keeps_its_config_and_its_plan():
    lay = L.Conv2D(8, 3, padding='same', activation='tanh', name='c', **CF)
    cfg = lay.get_config()
    assert cfg.pop('strides') == (1, 1)
    assert cfg == {'name': 'c', 'trainable': True, 'filters': 8, 'kernel_size': (3, 3), 'padding': 'same',
                   'data_format': 'channels_first', 'dilation_rate': (1, 1), 'activation': 'tanh', 'use_bias': True}
    x0 = L.Input(shape=(4, 8, 12))
    m = Model(inputs=x0, outputs=lay(x0), device=CPU)
    assert [(op.kind, op.src, op.dst, op.xs, tuple(op.halo), op.wparam, op.ksize) for op in m.plan.ops] == \
        [('conv', -1, -2, (4, 8, 12), (1, 1, 1, 1, 0, 0), None, None)]
    assert m.plan.phase_params == [] and lay.same_halo() == (1, 1, 1, 1)


@pytest.mark.parametrize('padding', S.PADDINGS)
def test_output_shapes_equal_the_references(padding):
    from dlwp_amd import ops
    for k in range(1, 6):
        for n in range(1, 10):
            lay = L.Conv2D(2, (k, 1), strides=2, padding=padding, name='down', **CF)
            if padding == 'valid' and n < k:
                with pytest.raises(ValueError, match='down.*does not fit'):
                    lay.compute_output_shape((3, n, 4))
                with pytest.raises(ValueError):
                    ops.sconv_geometry(k, padding, n)
                with pytest.raises(ValueError):
                    S.geometry(k, padding, n)
                continue
            want = S.reference(np.zeros((1, 3, n, 4)), np.zeros((k, 1, 3, 2)), None, padding).shape
            assert lay.compute_output_shape((3, n, 4)) == want[1:] == (2, S.geometry(k, padding, n)[3], 2)
            assert L.Conv2D(2, (1, k), strides=2, padding=padding, **CF).compute_output_shape((3, 4, n)) == (2, 2, want[2])
            assert ops.sconv_geometry(k, padding, n) == S.geometry(k, padding, n) == lay.strided_geometry(n, 4)[0]


def test_the_references_example_geometry():
    """k = 5 'valid' on the 41 x 148 map of examples/train_generator.py: T = 3, 19 x 72 outputs, a 21 x 74 phase tensor"""
    lay = L.Conv2D(16, 5, strides=2, **CF)
    assert lay.compute_output_shape((6, 41, 148)) == (16, 19, 72)
    (th, _, _, ho), (tw, _, _, wo) = lay.strided_geometry(41, 148)
    assert (th, tw, ho + th - 1, wo + tw - 1) == (3, 3, 21, 74)


# -- the restatement ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('padding', S.PADDINGS)
def test_restatement_equals_float64_strided_convolution(padding):
    """every (kh, kw) in 1 ... 5, maps 5 x 5, 6 x 7, 7 x 6, 9 x 12, stored taps T, 3 x 3 and 5 x 5: 1e-12 of max|y|"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for kh, kw in S.KERNELS:
        for h, w in S.MAPS:
            x = rng.standard_normal((2, 3, h, w))
            K, b = rng.standard_normal((kh, kw, 3, 2)), rng.standard_normal(2)
            want = S.reference(x, K, b, padding, 'tanh')
            for taps in (None, (3, 3), (5, 5)):
                got = S.restated(x, K, b, padding, 'tanh', taps=taps)
                assert got.shape == want.shape and got.dtype == np.float64
                worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print('\nMEASURED restatement against conv2d(stride=2) (%s): max difference %.3g of max|y|' % (padding, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize('padding', S.PADDINGS)
def test_restatement_with_the_references_halo_in_front(padding):
    """PeriodicPadding2D((0, 2)) + ZeroPadding2D((2, 0)) in front, against the reference on the np.pad-ed input"""
    rng = np.random.default_rng(4)
    halo = ((2, 2, 2, 2), (S.ZERO, S.WRAP))
    worst = 0.0
    for kh, kw in S.KERNELS:
        for h, w in S.MAPS:
            x = rng.standard_normal((2, 3, h, w))
            K, b = rng.standard_normal((kh, kw, 3, 2)), rng.standard_normal(2)
            want = S.reference(S.pad_np(x, *halo), K, b, padding)
            for taps in (None, (3, 3), (5, 5)):
                got = S.restated(x, K, b, padding, taps=taps, halo=halo)
                assert got.shape == want.shape
                worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print('\nMEASURED restatement behind a wrap / zero halo of 2 (%s): max difference %.3g of max|y|' % (padding, worst))
    assert worst <= 1e-12


def test_float32_restatement_stays_at_round_off():
    rng = np.random.default_rng(5)
    x, K = rng.standard_normal((2, 3, 9, 12)).astype(np.float32), rng.standard_normal((5, 4, 3, 2)).astype(np.float32)
    got = S.restated(x, K, None, 'same', taps=(3, 3))
    want = S.reference(x, K, None, 'same')
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


# -- adjoints ------------------------------------------------------------------------------------------------------------------------- #
def test_space_to_depth_and_its_adjoint_are_adjoint_for_every_mode_pair():
    rng = np.random.default_rng(6)
    for mh in S.MODES:
        for mw in S.MODES:
            for pad, (hp, wp) in (((2, 1, 1, 3), (5, 6)), ((0, 0, 0, 0), (2, 2)), ((1, 0, 0, 3), (4, 5))):
                x = rng.standard_normal((2, 3, 5, 6))
                g = rng.standard_normal((2, 12, hp, wp))
                lhs = float((S.s2d_pad(x, pad, (mh, mw), hp, wp) * g).sum())
                dx, cnt, mag = S.s2d_pad_bwd(g, pad, (mh, mw), 5, 6, stats=True)
                assert abs(lhs - float((x * dx).sum())) <= 1e-10 * max(1.0, abs(lhs))
                assert np.array_equal(dx, S.s2d_pad_bwd(g, pad, (mh, mw), 5, 6))
                assert not dx[:, :, cnt == 0].any() and cnt.sum() == _terms(pad, (mh, mw), 5, 6, hp, wp)


def _terms(pad, modes, h, w, hp, wp):
    """padded positions inside the padded image and inside [0, 2hp) x [0, 2wp) that map to a source pixel"""
    n = 0
    for r in range(min(2 * hp, h + pad[0] + pad[1])):
        for s in range(min(2 * wp, w + pad[2] + pad[3])):
            n += S.map_coord(r - pad[0], h, modes[0]) >= 0 and S.map_coord(s - pad[2], w, modes[1]) >= 0
    return n


def test_weight_map_is_a_permutation_with_zero_fill_and_its_adjoint_a_gather():
    for kh, kw in S.KERNELS:
        K = np.arange(1, kh * kw * 3 * 2 + 1, dtype=np.float64).reshape(kh, kw, 3, 2)
        th, tw = (kh + 1) // 2, (kw + 1) // 2
        for taps in (None, (3, 3), (5, 5)):
            w2 = S.weight_map(K, taps)
            assert w2.shape == (taps or (th, tw)) + (12, 2)
            assert sorted(w2[w2 != 0].tolist()) == sorted(K.ravel().tolist())         # every element exactly once, zeros elsewhere
            assert not w2[th:].any() and not w2[:, tw:].any()                          # the block sits at the origin
            assert np.array_equal(S.weight_map_bwd(w2, K.shape), K)


# -- the lowering --------------------------------------------------------------------------------------------------------------------- #
def test_plan_of_a_valid_and_a_same_layer():
    x0 = L.Input(shape=(4, 9, 12))
    lay = L.Conv2D(8, 3, strides=2, activation='tanh', name='down', **CF)
    m = Model(inputs=x0, outputs=lay(x0), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['sphasew', 's2dp', 'conv'] == [op.kind for op in m.infer_plan.ops]
    w, s, c = m.plan.ops
    # 'valid', k = 3: T = 2 stored as 3 x 3, 4 x 5 outputs, a 6 x 7 phase tensor of 16 channels; nothing padded
    assert w.wparam == 0 and w.layer is lay and m.plan.phase_params[0]['w2_shape'] == (3, 3, 16, 8)
    assert m.plan.phase_params[0]['kind'] == 'sconv' and m.plan.phase_params[0]['bias'] is False
    assert (s.src, s.xs, tuple(s.halo), s.out_shape, s.in_c_off, s.in_c_total) == (-1, (4, 9, 12), (0, 0, 0, 0, 0, 0), (16, 6, 7), 0, 4)
    assert m.plan.buffers[s.dst] == (16, 6, 7)
    assert (c.src, c.dst, c.xs, tuple(c.halo), c.conv_geometry, c.wparam, c.act, c.out_shape) == \
        (s.dst, -2, (16, 6, 7), (0, 0, 0, 0, 0, 0), (8, (3, 3), (1, 1)), 0, 1, (8, 4, 5))
    assert m.plan.output_store == [(8, 4, 5)]
    assert m.plan.conv_flops_per_sample() == 2 * 4 * 5 * 8 * 4 * 3 * 3                # the layer's own multiplies
    assert 's2dp' in m.plan.describe()
    # 'same', k = 4 on 9 x 12: rows out 5, total (5-1) 2 + 4 - 9 = 3 -> (1, 2); columns out 6, total 2 -> (1, 1)
    m = Model(inputs=x0, outputs=L.Conv2D(8, 4, strides=2, padding='same', **CF)(x0), device=CPU)
    s, c = m.plan.ops[1:]
    assert tuple(s.halo) == (1, 2, 1, 1, 0, 0) and s.out_shape == (16, 7, 8) and c.out_shape == (8, 5, 6)
    # k = 5: T = 3 -> 3 x 3 taps; k = 7: T = 4 -> 5 x 5
    m = Model(inputs=x0, outputs=L.Conv2D(2, 7, strides=2, padding='same', **CF)(x0), device=CPU)
    assert m.plan.ops[2].conv_geometry[1] == (5, 5) and m.plan.ops[1].out_shape == (16, 5 + 4, 6 + 4)
    assert not set(m.plan.bf16_buffers()) & {m.plan.ops[1].dst}


def test_the_halo_in_front_rides_in_the_space_to_depth_op():
    from dlwp_amd.custom import PeriodicPadding2D
    x0 = L.Input(shape=(4, 9, 12))
    t = L.ZeroPadding2D((2, 0), **CF)(PeriodicPadding2D((0, 2), **CF)(x0))
    m = Model(inputs=x0, outputs=L.Conv2D(16, 5, strides=2, activation='tanh', **CF)(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['sphasew', 's2dp', 'conv']
    s = m.plan.ops[1]
    assert s.src == -1 and s.xs == (4, 9, 12) and tuple(s.halo) == (2, 2, 2, 2, S.ZERO, S.WRAP)
    assert s.out_shape == (16, 5 + 2, 6 + 2) and m.plan.output_store == [(16, 5, 6)]
    # 'same' zeros of the layer extend zero rows; on the periodic columns they do not compose: the halo is materialised first
    m = Model(inputs=x0, outputs=L.Conv2D(16, 5, strides=2, padding='same', **CF)(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['pad', 'sphasew', 's2dp', 'conv']
    assert m.plan.ops[2].xs == (4, 13, 16) and tuple(m.plan.ops[2].halo) == (2, 2, 1, 2, 0, 0)       # 13 -> 7: total 4; 16 -> 8: 3
    m = Model(inputs=x0, outputs=L.Conv2D(16, (5, 2), strides=2, padding='same', **CF)(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['sphasew', 's2dp', 'conv'] and tuple(m.plan.ops[1].halo) == (4, 4, 2, 2, S.ZERO, S.WRAP)


def test_channel_slice_lazy_pooling_and_second_application():
    from dlwp_amd.custom import slice_layer
    x0 = L.Input(shape=(5, 8, 12))
    m = Model(inputs=x0, outputs=L.Conv2D(4, 2, strides=2, **CF)(slice_layer(1, 4, axis=1)(x0)), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['sphasew', 's2dp', 'conv']
    s = m.plan.ops[1]
    assert (s.src, s.xs, s.in_c_off, s.in_c_total, s.out_shape) == (-1, (3, 8, 12), 1, 5, (12, 4 + 2, 6 + 2))
    assert m.plan.phase_params[0]['w2_shape'] == (3, 3, 12, 4)
    # a lazy pooling / up-sampling in front is materialised first
    t = L.MaxPooling2D(2, **CF)(L.Conv2D(4, 3, padding='same', **CF)(x0))
    m = Model(inputs=x0, outputs=L.Conv2D(4, 2, strides=2, **CF)(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['conv', 'maxpool', 'sphasew', 's2dp', 'conv']
    assert m.plan.ops[3].xs == (4, 4, 6) and m.plan.output_store == [(4, 2, 3)]
    down = L.Conv2D(5, 3, strides=2, padding='same', name='twice', **CF)
    x1 = L.Input(shape=(5, 8, 8))
    with pytest.raises(NotImplementedError, match='twice.*more than once'):
        Model(inputs=x1, outputs=down(L.UpSampling2D(2, **CF)(down(x1))), device=CPU).plan


# -- model files ---------------------------------------------------------------------------------------------------------------------- #
def encoder_decoder(device=CPU, seed=1, l2=None):
    """model (a) of tests/test_gpu_sconv.py on 4 x 8 x 12"""
    from dlwp_amd.regularizers import l2 as l2_reg
    reg = dict(kernel_regularizer=l2_reg(l2)) if l2 else {}
    x0 = L.Input(shape=(4, 8, 12))
    t = L.Conv2D(8, 3, strides=2, padding='same', activation='tanh', **dict(CF, **reg))(x0)
    t = L.Conv2D(8, 3, padding='same', **CF)(t)
    return Model(inputs=x0, outputs=L.Conv2DTranspose(4, 4, strides=2, padding='same', **dict(CF, **reg))(t), device=device, seed=seed)


def test_descriptions_carry_the_stride():
    from dlwp_amd import serialization as Z
    from dlwp_amd.regularizers import l2
    down = L.Conv2D(6, (4, 3), strides=2, padding='same', activation='relu', use_bias=False, kernel_regularizer=l2(1e-3), name='down',
                    **CF)
    spec = json.loads(json.dumps(Z._keras_layer_spec(down)))
    cfg = spec['config']
    assert spec['class_name'] == 'Conv2D' and cfg['strides'] == [2, 2] and cfg['dilation_rate'] == [1, 1]
    again = L.Conv2D(**Z._keras_layer_kwargs(L.Conv2D, cfg))
    assert again.get_config() == down.get_config() and again.strides == (2, 2)
    native = json.loads(json.dumps(Z._layer_config(down)))
    assert native['strides'] == [2, 2]
    assert Z._keras_layer_spec(L.Conv2D(6, 3, **CF))['config']['strides'] == [1, 1]
    assert json.loads(json.dumps(Z._layer_config(L.Conv2D(6, 3, **CF))))['strides'] == [1, 1]


@pytest.mark.parametrize('fmt', ['npz', 'keras'])
def test_model_files_round_trip_on_the_host(tmp_path, fmt):
    from dlwp_amd import serialization as Z
    m = encoder_decoder(seed=3, l2=1e-4)
    rng = np.random.default_rng(8)
    m.set_weights([rng.standard_normal(w.shape).astype(np.float32) for w in m.get_weights()])
    path = str(tmp_path / ('m.%s' % fmt))
    Z.save_model_file(m, path, format=fmt)
    m2 = Z.load_model_file(path, device=CPU)
    assert [l.get_config() for l in m2.layers] == [l.get_config() for l in m.layers]
    assert [l.strides for l in m2.layers if isinstance(l, L.Conv2D)] == [(2, 2), (1, 1)]
    assert [(op.kind, op.src, op.dst, op.xs, tuple(op.halo)) for op in m2.plan.ops] == \
        [(op.kind, op.src, op.dst, op.xs, tuple(op.halo)) for op in m.plan.ops]
    assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))


def test_keras_2_2_sequential_with_a_strided_convolution_instantiates(tmp_path):
    from dlwp_amd import hdf5_lite, serialization
    cfg = {'name': 'conv2d_1', 'trainable': True, 'batch_input_shape': [None, 4, 8, 12], 'dtype': 'float32', 'filters': 8,
           'kernel_size': [3, 3], 'strides': [2, 2], 'padding': 'same', 'data_format': 'channels_first', 'dilation_rate': [1, 1],
           'activation': 'tanh', 'use_bias': True,
           'kernel_initializer': {'class_name': 'VarianceScaling',
                                  'config': {'scale': 1.0, 'mode': 'fan_avg', 'distribution': 'uniform', 'seed': None}},
           'bias_initializer': {'class_name': 'Zeros', 'config': {}}, 'kernel_regularizer': None, 'bias_regularizer': None,
           'activity_regularizer': None, 'kernel_constraint': None, 'bias_constraint': None}
    config = {'class_name': 'Sequential', 'config': {'name': 'sequential_1', 'layers': [{'class_name': 'Conv2D', 'config': cfg}]}}
    rng = np.random.default_rng(2)
    k, b = rng.standard_normal((3, 3, 4, 8)).astype(np.float32), rng.standard_normal(8).astype(np.float32)
    root = hdf5_lite.GroupSpec()
    root.attrs['keras_version'] = b'2.2.4'
    root.attrs['backend'] = b'tensorflow'
    root.attrs['model_config'] = json.dumps(config).encode('utf-8')
    mw = root.create_group('model_weights')
    mw.attrs['layer_names'] = np.array([b'conv2d_1'])
    g = mw.create_group('conv2d_1')
    g.attrs['weight_names'] = np.array([b'conv2d_1/kernel:0', b'conv2d_1/bias:0'])
    g.create_dataset('conv2d_1/kernel:0', k)
    g.create_dataset('conv2d_1/bias:0', b)
    path = str(tmp_path / 'strided.h5')
    hdf5_lite.write_file(path, root)
    m = serialization.import_keras_hdf5(path, device=CPU)
    lay = [l for l in m.layers if isinstance(l, L.Conv2D)][0]
    assert lay.strides == (2, 2) and m.plan.output_store == [(8, 4, 6)]
    assert [op.kind for op in m.plan.ops] == ['sphasew', 's2dp', 'conv']
    assert np.array_equal(m.get_weights()[0], k) and np.array_equal(m.get_weights()[1], b)


def test_build_model_takes_the_layer_by_name():
    """the second stage of the network examples/train_generator.py of the reference carries, as build_model receives it"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model((('PeriodicPadding2D', ((0, 2),), dict(CF, input_shape=(4, 9, 12))),
                   ('ZeroPadding2D', ((2, 0),), dict(CF)),
                   ('Conv2D', (16, 5), dict(CF, strides=2, padding='valid', activation='tanh')),
                   ('Flatten', None, None),
                   ('Dense', (4 * 9 * 12,), {'activation': 'linear'}),
                   ('Reshape', ((4, 9, 12),), None)), loss='mse', optimizer='adam')
    kinds = [op.kind for op in d.model.plan.ops]
    assert kinds[:3] == ['sphasew', 's2dp', 'conv'] and 'pad' not in kinds and 'dense' in kinds


# -- C ABI ---------------------------------------------------------------------------------------------------------------------------- #
NEW = {'dlwp_sconv_geometry': 7, 'dlwp_sconv_weights': 11, 'dlwp_sconv_weights_bwd': 12, 'dlwp_space_to_depth2_pad': 14,
       'dlwp_space_to_depth2_pad_bwd': 14}


def test_entry_points_are_exported_declared_and_bound():
    from dlwp_amd import _lib
    names = _lib.declared_symbols()
    for n, nargs in NEW.items():
        assert n in names and hasattr(_lib.lib, n)
        assert len(getattr(_lib.lib, n).argtypes) == nargs
    header = open(_lib.HEADER_PATH).read()
    for name, num in (('SCONV_WEIGHTS', 19), ('SPACE2DEPTH_PAD', 20)):
        assert re.search(r'#define\s+DLWP_OP_%s\s+%d\b' % (name, num), header) and getattr(_lib, 'OP_' + name) == num
    assert _lib.OP_CROP2D == 18                                              # appended: no existing value moved
    assert ctypes.sizeof(_lib.Op) == 5 * 4 + 16 + ctypes.sizeof(_lib.Conv2d) + 24 + 4 * 4 + 3 * 4 + ctypes.sizeof(_lib.Conv2d)


def test_entry_point_refusals_without_a_device():
    from dlwp_amd import _lib, ops
    lib, F32 = _lib.lib, _lib.F32
    one = ctypes.c_void_p(16)           # (never dereferenced: every call below is refused before a launch)
    i = ctypes.c_int()

    def refused(rc, text):
        assert rc != 0 and text in lib.dlwp_last_error().decode(), lib.dlwp_last_error()
    for k, n in ((0, 4), (-1, 4), (3, 0)):
        refused(lib.dlwp_sconv_geometry(k, 1, n, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)),
                'dlwp_sconv_geometry: bad arguments')
    refused(lib.dlwp_sconv_geometry(3, 1, 4, None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)), 'dlwp_sconv_geometry')
    refused(lib.dlwp_sconv_geometry(5, 0, 4, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)), 'does not fit')
    refused(lib.dlwp_sconv_weights(None, one, one, 3, 3, 4, 2, 3, 3, F32, None), 'dlwp_sconv_weights: null handle')
    refused(lib.dlwp_sconv_weights(None, one, one, 0, 3, 4, 2, 3, 3, F32, None), 'dlwp_sconv_weights: bad arguments')
    refused(lib.dlwp_sconv_weights(None, one, one, 3, 3, 4, 2, 3, 3, _lib.BF16, None), 'dlwp_sconv_weights: bad arguments')
    refused(lib.dlwp_sconv_weights(None, one, one, 3, 5, 4, 2, 2, 2, F32, None), 'stored taps')              # 2 x 3 taps needed
    refused(lib.dlwp_sconv_weights_bwd(None, one, one, 3, 3, 4, 2, 2, 2, 0, F32, None), 'dlwp_sconv_weights_bwd: null handle')
    refused(lib.dlwp_sconv_weights_bwd(None, one, one, 3, 3, 0, 2, 2, 2, 0, F32, None), 'dlwp_sconv_weights_bwd: bad arguments')
    refused(lib.dlwp_sconv_weights_bwd(None, one, one, 7, 3, 4, 2, 3, 3, 0, F32, None), 'stored taps')
    none, wrap2 = ops.make_pad(0, 0, 0, 0, 0, 0), ops.make_pad(0, 0, 2, 2, S.ZERO, S.WRAP)
    for fn, name in ((lib.dlwp_space_to_depth2_pad, 'dlwp_space_to_depth2_pad'),
                     (lib.dlwp_space_to_depth2_pad_bwd, 'dlwp_space_to_depth2_pad_bwd')):
        refused(fn(None, one, one, 1, 3, 6, 8, none, 3, 4, 0, 3, F32, None), name + ': null handle')
        refused(fn(None, one, one, 1, 3, 6, 8, none, 3, 4, 1, 3, F32, None), name + ': the channel window')      # [1, 4) of 3
        refused(fn(None, one, one, 1, 3, 6, 8, none, 3, 4, -1, 5, F32, None), name + ': the channel window')
        refused(fn(None, one, one, 1, 3, 6, 8, none, 0, 4, 0, 3, F32, None), name + ': bad shape')               # hp < 1
        refused(fn(None, one, one, 1, 3, 6, 8, none, 3, 0, 0, 3, F32, None), name + ': bad shape')
        refused(fn(None, one, one, 1, 0, 6, 8, none, 3, 4, 0, 3, F32, None), name + ': bad shape')
        refused(fn(None, one, one, 1, 3, 0, 8, none, 3, 4, 0, 3, F32, None), name + ': bad shape')
        refused(fn(None, one, one, -1, 3, 6, 8, none, 3, 4, 0, 3, F32, None), name + ': bad shape')
        refused(fn(None, one, one, 1, 3, 6, 1, wrap2, 3, 4, 0, 3, F32, None), name + ': the column halo')         # wrap 2 on 1 column
        refused(fn(None, one, one, 1, 3, 2, 8, ops.make_pad(2, 0, 0, 0, S.REFLECT, S.ZERO), 3, 4, 0, 3, F32, None),
                name + ': the row halo')
        refused(fn(None, one, one, 1, 3, 6, 8, ops.make_pad(0, -1, 0, 0, 0, 0), 3, 4, 0, 3, F32, None), name + ': negative padding')
        refused(fn(None, one, one, 1, 3, 6, 8, ops.make_pad(0, 0, 0, 0, 5, 0), 3, 4, 0, 3, F32, None), name + ': unknown pad mode')
        refused(fn(None, one, one, 1, 3, 6, 8, none, 3, 4, 0, 3, _lib.BF16, None), name + ': dtype')
    # null pointers need no handle either (checked in front of it); an empty batch has none and gets as far as the handle
    for fn, name in ((lib.dlwp_space_to_depth2_pad, 'dlwp_space_to_depth2_pad'),
                     (lib.dlwp_space_to_depth2_pad_bwd, 'dlwp_space_to_depth2_pad_bwd')):
        for a, b in ((None, one), (one, None), (None, None)):
            refused(fn(None, a, b, 1, 3, 6, 8, none, 3, 4, 0, 3, F32, None), name + ': null pointer')
        refused(fn(None, None, None, 0, 3, 6, 8, none, 3, 4, 0, 3, F32, None), name + ': null handle')
    for a, b in ((None, one), (one, None), (None, None)):
        refused(lib.dlwp_sconv_weights(None, a, b, 3, 3, 4, 2, 3, 3, F32, None), 'dlwp_sconv_weights: null pointer')
        refused(lib.dlwp_sconv_weights_bwd(None, a, b, 3, 3, 4, 2, 2, 2, 0, F32, None), 'dlwp_sconv_weights_bwd: null pointer')
