"""Conv2DTranspose(strides=2) and Cropping2D on the host: the restatement the kernels of csrc/tconv.hip implement (weight map + full
cross-correlation + cropping interleave, tests/tconv_cases.py) against float64 torch, the layers' shapes and refusals, the lowering,
both model-file formats, the Keras import shim and the registry, and the C ABI's refusals that need no device."""
import ctypes
import json
import re

import numpy as np
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd.engine import Model
from tests import tconv_cases as T

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')


# -- the restatement ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('padding', T.PADDINGS)
def test_restatement_equals_float64_conv_transpose(padding):
    """every kh, kw in 1 ... 5 ((2, 3) and (5, 1) among them), maps 1 x 1, 2 x 3 and 5 x 4, cin = 3, F = 2, two samples: 1e-12"""
    assert (2, 3) in T.KERNELS and (5, 1) in T.KERNELS
    rng = np.random.default_rng(3)
    worst = 0.0
    for kh, kw in T.KERNELS:
        for h, w in T.MAPS:
            x = rng.standard_normal((2, 3, h, w))
            K, b = rng.standard_normal((kh, kw, 2, 3)), rng.standard_normal(2)
            got, want = T.restated(x, K, b, padding), T.reference(x, K, b, padding)
            assert got.shape == want.shape == (2, 2, T.geometry(kh, padding, h)[2], T.geometry(kw, padding, w)[2])
            worst = max(worst, float(np.abs(got - want).max()))
            # ... and stored with the 3 x 3 taps of the matrix-core kernels (zero taps, a wider zero halo): the same tensor
            wide = T.restated(x, K, b, padding, taps=T.stored_taps((kh + 1) // 2, (kw + 1) // 2))
            worst = max(worst, float(np.abs(wide - want).max()))
    print('\nMEASURED restatement against conv_transpose2d (%s): max difference %.3g' % (padding, worst))
    assert worst <= 1e-12


def test_same_padding_is_the_slice_of_the_full_result():
    rng = np.random.default_rng(4)
    for kh, kw in T.KERNELS:
        x, K = rng.standard_normal((1, 2, 5, 4)), rng.standard_normal((kh, kw, 3, 2))
        full, same = T.reference(x, K, None, 'valid'), T.reference(x, K, None, 'same')
        pt, pl = max(kh - 2, 0) // 2, max(kw - 2, 0) // 2
        assert np.abs(full[:, :, pt:pt + 10, pl:pl + 8] - same).max() <= 1e-12


def test_extra_row_and_column_of_odd_kernels_are_exactly_zero():
    rng = np.random.default_rng(5)
    for kh, kw in T.KERNELS:
        for h, w in T.MAPS:
            x, K = rng.standard_normal((1, 3, h, w)), rng.standard_normal((kh, kw, 2, 3))
            full = T.restated(x, K, full=True)
            hf, wf = T.geometry(kh, 'valid', h)[2], T.geometry(kw, 'valid', w)[2]
            assert full.shape[2] - hf == kh % 2 * (kh > 1) and full.shape[3] - wf == kw % 2 * (kw > 1)
            assert not full[:, :, hf:].any() and not full[:, :, :, wf:].any()
            if kh == 1:                                # Keras' deconv_length keeps an all-zero last row for k = 1
                assert not full[:, :, hf - 1].any()


def test_weight_map_is_a_permutation_with_zero_fill_and_its_adjoint_a_gather():
    rng = np.random.default_rng(6)
    for kh, kw in T.KERNELS:
        K = rng.standard_normal((kh, kw, 2, 3)).astype(np.float32)
        w2, b2 = T.weight_map(K, np.arange(2, dtype=np.float32))
        assert w2.shape == ((kh + 1) // 2, (kw + 1) // 2, 3, 8) and b2.tolist() == [0, 1] * 4
        assert sorted(np.abs(w2[w2 != 0]).tolist()) == sorted(np.abs(K).reshape(-1).tolist())
        assert np.array_equal(T.weight_map_bwd(w2, K.shape), K)                      # adjoint o map = identity on K
        for taps in ((3, 3), (5, 5), (3, 4)):
            w3, _ = T.weight_map(K, None, taps)
            oh, ow = (taps[0] - w2.shape[0]) // 2, (taps[1] - w2.shape[1]) // 2
            assert np.array_equal(w3[oh:oh + w2.shape[0], ow:ow + w2.shape[1]], w2) and np.count_nonzero(w3) == np.count_nonzero(w2)
            assert np.array_equal(T.weight_map_bwd(w3, K.shape), K)
        g2 = rng.standard_normal(w2.shape)
        assert np.isclose((T.weight_map_bwd(g2, K.shape) * K).sum(), (g2 * w2).sum())     # <A* g, K> = <g, A K>


def test_interleave_and_its_adjoint_are_adjoint():
    rng = np.random.default_rng(7)
    for hp, wp, top, left, hh, ww in [(3, 4, 0, 0, 6, 8), (3, 4, 1, 1, 4, 6), (5, 7, 1, 3, 8, 9), (1, 1, 1, 0, 1, 2)]:
        ph, dy = rng.standard_normal((2, 8, hp, wp)), rng.standard_normal((2, 2, hh, ww))
        y, dph = T.d2s_crop(ph, 2, top, left, hh, ww), T.s2d_fill(dy, hp, wp, top, left)
        assert np.isclose((y * dy).sum(), (ph * dph).sum())
        assert np.array_equal(T.d2s_crop(dph, 2, top, left, hh, ww), dy)


# -- the layers ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('padding', T.PADDINGS)
def test_output_shapes_are_keras_deconv_length(padding):
    for kh, kw in T.KERNELS:
        for h, w in T.MAPS:
            lay = L.Conv2DTranspose(5, (kh, kw), padding=padding, **CF)
            want = (5, 2 * h + (max(kh - 2, 0) if padding == 'valid' else 0), 2 * w + (max(kw - 2, 0) if padding == 'valid' else 0))
            assert lay.compute_output_shape((3, h, w)) == want
            assert lay(L.Input(shape=(3, h, w))).shape == want


def test_conv2d_transpose_weights_config_and_parameter_count():
    lay = L.Conv2DTranspose(6, (2, 3), strides=2, padding='same', activation='tanh', name='up', **CF)
    x0 = L.Input(shape=(4, 5, 7))
    m = Model(inputs=x0, outputs=lay(x0), device=CPU, seed=1)
    assert [nm for nm, _ in lay._weights] == ['kernel', 'bias']
    assert tuple(lay.kernel.shape) == (2, 3, 6, 4) and tuple(lay.bias.shape) == (6,)           # filters before input channels
    limit = np.sqrt(6.0 / (6 * 6 + 4 * 6))                                                     # fan_in = F kh kw, fan_out = cin kh kw
    k = lay.get_weights()[0]
    assert np.abs(k).max() <= limit and np.abs(k).max() > 0.8 * limit and not lay.get_weights()[1].any()
    assert lay.count_params() == 2 * 3 * 6 * 4 + 6 and m.count_params() == lay.count_params()
    assert lay.get_config() == {'name': 'up', 'trainable': True, 'filters': 6, 'kernel_size': (2, 3), 'strides': (2, 2),
                                'padding': 'same', 'output_padding': None, 'data_format': 'channels_first', 'dilation_rate': (1, 1),
                                'activation': 'tanh', 'use_bias': True}
    nb = L.Conv2DTranspose(6, 2, use_bias=False, kernel_initializer='zeros', **CF)
    Model(inputs=x0, outputs=nb(x0), device=CPU)
    assert [nm for nm, _ in nb._weights] == ['kernel'] and not nb.get_weights()[0].any()
    m.summary()


@pytest.mark.parametrize('kwargs, what', [
    (dict(strides=1), 'strides'), (dict(strides=(2, 1)), 'strides'), (dict(strides=3), 'strides'),
    (dict(dilation_rate=2), 'dilation_rate'), (dict(output_padding=1), 'output_padding'), (dict(output_padding=(0, 0)), 'output_padding'),
    (dict(data_format=None), 'channels_first'), (dict(data_format='channels_last'), 'channels_first'),
    (dict(activation='sigmoid'), 'activation'), (dict(kernel_initializer='he_normal'), 'initialisers'),
    (dict(bias_initializer='ones'), 'initialisers')])
def test_conv2d_transpose_refusals_name_the_layer(kwargs, what):
    kw = dict(CF)
    kw.update(kwargs)
    with pytest.raises(NotImplementedError, match='Conv2DTranspose.*%s' % what):
        L.Conv2DTranspose(4, 3, **kw)


def test_conv2d_transpose_refuses_reshaped_tensors_and_a_second_application():
    x0 = L.Input(shape=(2, 3, 4, 5))
    with pytest.raises(NotImplementedError, match='the_up.*Conv2DTranspose'):
        L.Conv2DTranspose(4, 2, name='the_up', **CF)(x0)
    with pytest.raises(NotImplementedError, match='the_up.*Conv2DTranspose'):
        L.Conv2DTranspose(4, 2, name='the_up', **CF)(L.Reshape((2, 4, 3, 6))(L.Input(shape=(8, 3, 6))))
    x0 = L.Input(shape=(8, 3, 6))                                # (a Reshape back to three axes is a plain 3-D tensor again)
    m = Model(inputs=x0, outputs=L.Conv2DTranspose(4, 2, **CF)(L.Reshape((4, 6, 6))(x0)), device=CPU)
    assert m.plan.output_store == [(4, 12, 12)]
    up =L.Conv2DTranspose(4, 2, padding='same', name='twice', **CF)
    x0 = L.Input(shape=(4, 4, 6))
    with pytest.raises(NotImplementedError, match='twice.*Conv2DTranspose.*more than once'):
        Model(inputs=x0, outputs=L.concatenate([up(x0), up(L.Conv2D(4, 3, padding='same', **CF)(x0))], axis=1), device=CPU).plan
    with pytest.raises(ValueError):
        L.Conv2DTranspose(4, 2, padding='full', **CF)


def test_cropping2d_argument_forms_shapes_and_errors():
    assert L.Cropping2D(2, **CF).cropping == ((2, 2), (2, 2))
    assert L.Cropping2D((1, 3), **CF).cropping == ((1, 1), (3, 3))
    assert L.Cropping2D(((1, 0), (0, 2)), **CF).cropping == ((1, 0), (0, 2))
    assert L.Cropping2D([[1, 0], [0, 2]], **CF).cropping == ((1, 0), (0, 2))
    assert L.Cropping2D(**CF).cropping == ((0, 0), (0, 0))
    lay = L.Cropping2D(((1, 0), (0, 2)), name='trim', **CF)
    assert lay.compute_output_shape((3, 73, 144)) == (3, 72, 142) and lay.count_params() == 0
    assert lay.get_config() == {'name': 'trim', 'trainable': True, 'cropping': ((1, 0), (0, 2)), 'data_format': 'channels_first'}
    for bad in ((1, 2, 3), ((1, 2, 3), (0, 0)), 'ab' * 3):
        with pytest.raises(ValueError):
            L.Cropping2D(bad, **CF)
    with pytest.raises(ValueError, match='negative'):
        L.Cropping2D(((0, -1), (0, 0)), **CF)
    for crop, shape in ((((2, 2), (0, 0)), (3, 4, 9)), (((0, 0), (4, 5)), (3, 4, 9)), (5, (1, 10, 12))):
        with pytest.raises(ValueError, match='Cropping2D.*nothing'):
            L.Cropping2D(crop, **CF)(L.Input(shape=shape))
    for df in (None, 'channels_last'):
        with pytest.raises(NotImplementedError, match='Cropping2D.*channels_first'):
            L.Cropping2D(1, data_format=df)
    with pytest.raises(NotImplementedError, match='trim.*Cropping2D'):
        lay(L.Input(shape=(2, 3, 8, 8)))


# -- the lowering --------------------------------------------------------------------------------------------------------------------- #
def small_model(device=CPU, seed=1, l2=None):
    """the encoder / decoder of tests/test_gpu_tconv.py on 4 x 8 x 12: conv -> max-pool -> Conv2DTranspose(8, 2) ->
    PeriodicPadding2D((0, 1)) + Conv2DTranspose(4, 4, 'same') + Cropping2D((0, 2)) -> conv"""
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.regularizers import l2 as l2_reg
    reg = dict(kernel_regularizer=l2_reg(l2)) if l2 else {}
    x0 = L.Input(shape=(4, 8, 12))
    t = L.MaxPooling2D(2, **CF)(L.Conv2D(8, 3, padding='same', activation='tanh', **CF)(x0))
    t = L.Conv2DTranspose(8, 2, activation='tanh', **dict(CF, **reg))(t)
    t = L.Conv2DTranspose(4, 4, padding='same', activation='relu', **dict(CF, **reg))(PeriodicPadding2D((0, 1), **CF)(t))
    t = L.Cropping2D((0, 2), **CF)(t)
    return Model(inputs=x0, outputs=L.Conv2D(4, 3, padding='same', **CF)(t), device=device, seed=seed)


def test_plan_of_the_small_model():
    m = small_model()
    assert [op.kind for op in m.plan.ops] == ['conv', 'maxpool', 'tphasew', 'conv', 'd2sc', 'pad', 'tphasew', 'conv', 'd2sc', 'conv']
    ops_ = m.plan.ops
    # Conv2DTranspose(8, 2): one tap (T = 1), stored as the centre of 3 x 3 taps with a zero halo of 1: a convolution with 32 phase
    # channels on the pooled 4 x 6 map, nothing cropped
    assert ops_[3].conv_geometry == (32, (3, 3), (1, 1)) and ops_[3].xs == (8, 4, 6) and tuple(ops_[3].halo[:4]) == (1, 1, 1, 1)
    assert ops_[3].wparam == 0 and ops_[3].act == 1 and ops_[4].crop == (0, 0) and ops_[4].xs == (8, 4, 6)
    assert ops_[4].out_shape == (8, 8, 12)
    # Conv2DTranspose(4, 4, 'same') on the periodic 8 x 14 map: 2 x 2 taps in the upper left of 3 x 3, zero halo 1 above / left and
    # 2 below / right, a 9 x 15 phase map; 'same' crops (1, 1), the Cropping2D((0, 2)) behind it is folded into the interleave:
    # columns from 3 on, 24 of them
    assert ops_[7].conv_geometry == (16, (3, 3), (1, 1)) and ops_[7].xs == (8, 8, 14) and tuple(ops_[7].halo) == (1, 2, 1, 2, 0, 0)
    assert ops_[8].xs == (4, 9, 15) and ops_[8].crop == (1, 3) and ops_[8].out_shape == (4, 16, 24)
    assert m.plan.buffers[ops_[8].dst] == (4, 16, 24)
    assert [p['w2_shape'] for p in m.plan.phase_params] == [(3, 3, 8, 32), (3, 3, 8, 16)]
    assert m.plan.output_store == [(4, 8 * 2, 12 * 2)]
    # the inference plan pools in the first convolution's epilogue; the transposed layers lower alike
    assert [op.kind for op in m.infer_plan.ops] == ['conv', 'tphasew', 'conv', 'd2sc', 'pad', 'tphasew', 'conv', 'd2sc', 'conv'] or \
        [op.kind for op in m.infer_plan.ops] == ['conv', 'tphasew', 'conv', 'pad', 'tphasew', 'conv', 'd2sc', 'conv']
    assert 'crop(1, 3)' in m.plan.describe()
    # nothing of these layers is stored as bfloat16: the phase tensors and what the interleave writes stay float32
    bf = set(m.plan.bf16_buffers())
    assert not bf & {ops_[3].dst, ops_[4].dst, ops_[7].dst, ops_[8].dst}


def test_crop_on_its_own_and_behind_a_transposed_convolution():
    x0 = L.Input(shape=(3, 9, 10))
    m = Model(inputs=x0, outputs=L.Cropping2D(((1, 0), (2, 3)), **CF)(x0), device=CPU)
    assert [(op.kind, op.src, op.dst, op.xs, tuple(op.halo[:4]), op.out_shape) for op in m.plan.ops] == \
        [('crop', -1, -2, (3, 9, 10), (1, 0, 2, 3), (3, 8, 5))]
    # a channel window in front is extracted first; the crop of a tensor something else reads too stays a launch of its own
    from dlwp_amd.custom import slice_layer
    m = Model(inputs=x0, outputs=L.Cropping2D(1, **CF)(slice_layer(1, 3, axis=1)(x0)), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['copy', 'crop'] and m.plan.output_store == [(2, 7, 8)]
    up = L.Conv2DTranspose(2, 3, **CF)(x0)                                   # (2, 19, 21)
    m = Model(inputs=x0, outputs=[L.Cropping2D(((0, 1), (1, 0)), **CF)(up), up], device=CPU)
    assert [op.kind for op in m.plan.ops] == ['tphasew', 'conv', 'd2sc', 'crop'] and m.plan.ops[2].crop == (0, 0)
    assert m.plan.output_store == [(2, 18, 20), (2, 19, 21)]
    # alone behind the layer, as the model's output: the interleave writes the cropped window into the output slot
    m = Model(inputs=x0, outputs=L.Cropping2D(((0, 1), (1, 0)), **CF)(L.Conv2DTranspose(2, 3, **CF)(x0)), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['tphasew', 'conv', 'd2sc']
    assert m.plan.ops[2].crop == (0, 1) and m.plan.ops[2].dst == -2 and m.plan.ops[2].out_shape == (2, 18, 20)
    assert m.plan.ops[2].xs == (2, 10, 11) and m.plan.output_store == [(2, 18, 20)]


def test_stored_taps_follow_the_kernel_size(monkeypatch):
    from dlwp_amd import plan as P
    for k, want in ((1, (3, 3)), (2, (3, 3)), (4, (3, 3)), (6, (3, 3)), (7, (5, 5)), (10, (5, 5)), (11, (6, 6)), ((2, 9), (5, 5))):
        ks = (k, k) if isinstance(k, int) else k
        th, tw = (ks[0] + 1) // 2, (ks[1] + 1) // 2
        assert P.tconv_taps(th, tw) == want == T.stored_taps(th, tw)
        x0 = L.Input(shape=(3, 5, 6))
        m = Model(inputs=x0, outputs=L.Conv2DTranspose(2, k, padding='same', **CF)(x0), device=CPU)
        conv = m.plan.ops[1]
        oh, ow = (want[0] - th) // 2, (want[1] - tw) // 2
        assert conv.conv_geometry[1] == want and m.plan.output_store == [(2, 10, 12)]
        assert tuple(conv.halo[:4]) == (th - 1 + oh, th - 1 + want[0] - th - oh, tw - 1 + ow, tw - 1 + want[1] - tw - ow)
    monkeypatch.setenv('DLWP_TCONV_TAPS', 'exact')
    assert P.tconv_taps(1, 2) == (1, 2)


def test_73_row_model_returns_a_73_row_state():
    x0 = L.Input(shape=(2, 73, 144))
    t = L.Cropping2D(((1, 0), (0, 0)), **CF)(x0)
    t = L.MaxPooling2D(2, **CF)(L.Conv2D(4, 3, padding='same', activation='tanh', **CF)(t))
    t = L.Conv2DTranspose(2, 2, **CF)(t)
    m = Model(inputs=x0, outputs=L.ZeroPadding2D(((1, 0), (0, 0)), **CF)(t), device=CPU)
    assert m.plan.output_store == [(2, 73, 144)] and m.plan.ops[0].kind == 'crop'


# -- model files, the shim, the registry ---------------------------------------------------------------------------------------------- #
def test_native_config_and_keras_description_round_trip():
    from dlwp_amd import serialization as S
    from dlwp_amd.regularizers import l2
    up = L.Conv2DTranspose(6, (4, 3), padding='same', activation='relu', use_bias=False, kernel_regularizer=l2(1e-3), name='up', **CF)
    crop = L.Cropping2D(((1, 0), (0, 2)), name='trim', **CF)
    spec = json.loads(json.dumps(S._keras_layer_spec(up)))
    assert spec['class_name'] == 'Conv2DTranspose'
    cfg = spec['config']
    assert (cfg['filters'], cfg['kernel_size'], cfg['strides'], cfg['padding'], cfg['output_padding'], cfg['data_format'],
            cfg['dilation_rate'], cfg['activation'], cfg['use_bias']) == (6, [4, 3], [2, 2], 'same', None, 'channels_first', [1, 1],
                                                                          'relu', False)
    assert cfg['kernel_regularizer'] == {'class_name': 'L1L2', 'config': {'l1': 0.0, 'l2': pytest.approx(1e-3)}}
    again = L.Conv2DTranspose(**S._keras_layer_kwargs(L.Conv2DTranspose, cfg))
    assert again.get_config() == up.get_config() and again.kernel_regularizer.l2 == pytest.approx(1e-3)
    spec = json.loads(json.dumps(S._keras_layer_spec(crop)))
    assert spec == {'class_name': 'Cropping2D', 'config': {'name': 'trim', 'trainable': True, 'cropping': [[1, 0], [0, 2]],
                                                           'data_format': 'channels_first'}}
    assert L.Cropping2D(**S._keras_layer_kwargs(L.Cropping2D, spec['config'])).get_config() == crop.get_config()
    assert L.Cropping2D(**json.loads(json.dumps(S._layer_config(crop)))).get_config() == crop.get_config()


@pytest.mark.parametrize('fmt', ['npz', 'keras'])
def test_model_files_round_trip_on_the_host(tmp_path, fmt):
    from dlwp_amd import hdf5_lite
    from dlwp_amd import serialization as S
    m = small_model(seed=3, l2=1e-4)
    rng = np.random.default_rng(8)
    m.set_weights([rng.standard_normal(w.shape).astype(np.float32) for w in m.get_weights()])
    path = str(tmp_path / ('m.%s' % fmt))
    S.save_model_file(m, path, format=fmt)
    m2 = S.load_model_file(path, device=CPU)
    assert [type(l).__name__ for l in m2.layers] == [type(l).__name__ for l in m.layers]
    assert [l.get_config() for l in m2.layers] == [l.get_config() for l in m.layers]
    assert [getattr(l.kernel_regularizer, 'l2', None) for l in m2.layers if isinstance(l, L.Conv2DTranspose)] == \
        [pytest.approx(1e-4)] * 2
    assert [(op.kind, op.src, op.dst, op.xs, op.crop) for op in m2.plan.ops] == [(op.kind, op.src, op.dst, op.xs, op.crop) for op in m.plan.ops]
    assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))
    if fmt == 'keras':                                   # Keras' names: <layer>/kernel:0, <layer>/bias:0, the kernel (kh, kw, F, cin)
        f = hdf5_lite.File(path)
        up = [l for l in m.layers if isinstance(l, L.Conv2DTranspose)][1]
        g = f['model_weights'][up.name]
        assert tuple(np.asarray(g['%s/kernel:0' % up.name][...]).shape) == (4, 4, 4, 8)
        assert tuple(np.asarray(g['%s/bias:0' % up.name][...]).shape) == (4,)
        names = [c['class_name'] for c in json.loads(bytes(f.attrs['model_config']).decode())['config']['layers']]
        assert 'Conv2DTranspose' in names and 'Cropping2D' in names


def test_import_shim_and_registry_resolve_both_names():
    import dlwp_amd.compat  # noqa: F401
    from dlwp_amd import util
    from keras.layers import Conv2DTranspose, Cropping2D
    from keras.layers.convolutional import Conv2DTranspose as C2, Cropping2D as C3
    assert Conv2DTranspose is L.Conv2DTranspose is C2 and Cropping2D is L.Cropping2D is C3
    assert util.get_from_class('keras.layers', 'Conv2DTranspose') is L.Conv2DTranspose
    assert util.get_from_class('keras.layers', 'Cropping2D') is L.Cropping2D


def test_build_model_takes_both_layers_by_name():
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model((('Conv2D', (8, 3), dict(CF, padding='same', activation='tanh', input_shape=(4, 8, 12))),
                   ('MaxPooling2D', (2,), dict(CF)),
                   ('Conv2DTranspose', (4, 3), dict(CF, strides=2, activation='tanh')),
                   ('Cropping2D', (((0, 1), (1, 0)),), dict(CF))), loss='mse', optimizer='adam')
    assert [type(l).__name__ for l in d.model.layers if not isinstance(l, L.InputLayer)] == \
        ['Conv2D', 'MaxPooling2D', 'Conv2DTranspose', 'Cropping2D']
    assert d.model.plan.output_store == [(4, 8, 12)]


# -- C ABI ---------------------------------------------------------------------------------------------------------------------------- #
NEW = {'dlwp_tconv_geometry': 6, 'dlwp_tconv_weights': 13, 'dlwp_tconv_weights_bwd': 12, 'dlwp_depth_to_space2_crop': 15,
       'dlwp_space_to_depth2_fill': 15}


def test_entry_points_are_exported_declared_and_bound():
    from dlwp_amd import _lib
    names = _lib.declared_symbols()
    for n, nargs in NEW.items():
        assert n in names and hasattr(_lib.lib, n)
        assert len(getattr(_lib.lib, n).argtypes) == nargs
    header = open(_lib.HEADER_PATH).read()
    for name, num in (('TCONV_WEIGHTS', 16), ('DEPTH2SPACE_CROP', 17), ('CROP2D', 18)):
        assert re.search(r'#define\s+DLWP_OP_%s\s+%d\b' % (name, num), header) and getattr(_lib, 'OP_' + name) == num
    assert _lib.OP_BILINEAR2 == 15 and _lib.OP_PHASE_WEIGHTS == 6           # appended: no existing value moved
    assert ctypes.sizeof(_lib.Op) == 5 * 4 + 16 + ctypes.sizeof(_lib.Conv2d) + 24 + 4 * 4 + 3 * 4 + ctypes.sizeof(_lib.Conv2d)


def test_geometry_helper():
    from dlwp_amd import _lib, ops
    for k in range(1, 8):
        for padding in T.PADDINGS:
            for n in (1, 5, 22):
                assert ops.tconv_geometry(k, padding, n) == T.geometry(k, padding, n)
                t, crop, out = ops.tconv_geometry(k, padding, n)
                assert crop + out <= 2 * (n + t - 1)                       # the output is a window of the interleaved phase tensor
    i = ctypes.c_int()
    for k, n in ((0, 4), (-1, 4), (3, 0)):
        assert _lib.lib.dlwp_tconv_geometry(k, 0, n, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) != 0
        assert b'dlwp_tconv_geometry' in _lib.lib.dlwp_last_error()
    assert _lib.lib.dlwp_tconv_geometry(3, 0, 4, None, ctypes.byref(i), ctypes.byref(i)) != 0


def test_entry_point_refusals_without_a_device():
    from dlwp_amd import _lib
    lib, F32 = _lib.lib, _lib.F32
    one = ctypes.c_void_p(16)           # (never dereferenced: every call below is refused before a launch)

    def refused(rc, text):
        assert rc != 0 and text in lib.dlwp_last_error().decode(), lib.dlwp_last_error()
    refused(lib.dlwp_tconv_weights(None, one, None, one, None, 3, 3, 4, 2, 3, 3, F32, None), 'dlwp_tconv_weights: null handle')
    refused(lib.dlwp_tconv_weights(None, one, None, one, None, 0, 3, 4, 2, 3, 3, F32, None), 'dlwp_tconv_weights: bad arguments')
    refused(lib.dlwp_tconv_weights(None, one, None, one, None, 3, -1, 4, 2, 3, 3, F32, None), 'dlwp_tconv_weights: bad arguments')
    refused(lib.dlwp_tconv_weights(None, one, None, one, None, 3, 3, 4, 2, 3, 3, _lib.BF16, None), 'dlwp_tconv_weights: bad arguments')
    refused(lib.dlwp_tconv_weights(None, one, None, one, None, 3, 5, 4, 2, 2, 2, F32, None), 'stored taps')     # 2 x 3 taps needed
    refused(lib.dlwp_tconv_weights_bwd(None, one, one, 3, 3, 4, 2, 2, 2, 0, F32, None), 'dlwp_tconv_weights_bwd: null handle')
    refused(lib.dlwp_tconv_weights_bwd(None, one, one, 3, 0, 4, 2, 2, 2, 0, F32, None), 'dlwp_tconv_weights_bwd: bad arguments')
    refused(lib.dlwp_tconv_weights_bwd(None, one, one, 7, 3, 4, 2, 3, 3, 0, F32, None), 'stored taps')
    for fn, name in ((lib.dlwp_depth_to_space2_crop, 'dlwp_depth_to_space2_crop'), (lib.dlwp_space_to_depth2_fill, 'dlwp_space_to_depth2_fill')):
        refused(fn(None, one, one, 1, 2, 3, 4, 0, 0, 6, 8, 0, 2, F32, None), name + ': null handle')
        refused(fn(None, one, one, 1, 2, 3, 4, 1, 0, 6, 8, 0, 2, F32, None), name + ': the crop')        # rows 1 ... 6 of 6
        refused(fn(None, one, one, 1, 2, 3, 4, 0, 1, 6, 8, 0, 2, F32, None), name + ': the crop')        # columns 1 ... 8 of 8
        refused(fn(None, one, one, 1, 2, 3, 4, 0, 0, 7, 8, 0, 2, F32, None), name + ': the crop')
        refused(fn(None, one, one, 1, 2, 3, 4, -1, 0, 6, 8, 0, 2, F32, None), name + ': the crop')
        refused(fn(None, one, one, 1, 2, 3, 4, 0, 0, 0, 8, 0, 2, F32, None), name + ': bad arguments')
        refused(fn(None, one, one, 1, 2, 3, 4, 0, 0, 6, 8, 1, 2, F32, None), name + ': bad arguments')   # channel window past the tensor
        refused(fn(None, one, one, 1, 0, 3, 4, 0, 0, 6, 8, 0, 2, F32, None), name + ': bad arguments')
