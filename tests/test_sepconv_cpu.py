"""DepthwiseConv2D / SeparableConv2D on the host: the numpy restatements of tests/sepconv_cases.py against float64 torch
conv2d(groups=cin) and autograd, the layers' arguments, shapes, halos and fans, the Keras 2.2.4 config layout, the lowering, the model
files and the C ABI's refusals that need no device."""
import ctypes
import json
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from dlwp_amd.engine import Model
from tests import sepconv_cases as S

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')
NP_MODE = {S.ZERO: 'constant', S.WRAP: 'wrap', S.EDGE: 'edge', S.REFLECT: 'reflect', S.SYMMETRIC: 'symmetric'}


def _torch_weight(K):
    """(kh, kw, cin, dm) -> (cin dm, 1, kh, kw): output channel c dm + m of group c"""
    kh, kw, cin, dm = K.shape
    return K.permute(2, 3, 0, 1).reshape(cin * dm, 1, kh, kw)


# -- the restatements ----------------------------------------------------------------------------------------------------------------- #
def test_halo_map_equals_numpy_pad_for_every_mode_pair():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 3, 5, 7))
    for mh, mw in S.MODE_PAIRS:
        for pad in S.DW_HALOS:
            want = np.pad(np.pad(x, ((0, 0), (0, 0), (pad[0], pad[1]), (0, 0)), mode=NP_MODE[mh]),
                          ((0, 0), (0, 0), (0, 0), (pad[2], pad[3])), mode=NP_MODE[mw])
            got = S.pad_np(x, pad, (mh, mw))
            assert np.array_equal(got, want), (mh, mw, pad)
            g = rng.standard_normal(got.shape)
            lhs, rhs = float((got * g).sum()), float((x * S.pad_bwd(g, pad, (mh, mw), 5, 7)).sum())
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


@pytest.mark.parametrize('ks', S.DW_KERNELS, ids=lambda k: '%dx%d' % k)
def test_depthwise_restatement_and_adjoints_equal_float64_torch(ks):
    rng = np.random.default_rng(ks[0] * 7 + ks[1])
    worst = 0.0
    for dil in S.DW_DILATIONS:
        for dm in S.DW_MULTIPLIERS:
            for pad, modes in (((0, 0, 0, 0), (S.ZERO, S.ZERO)), ((2, 2, 2, 2), (S.ZERO, S.WRAP)), ((1, 0, 0, 3), (S.REFLECT, S.EDGE))):
                x, K, b = rng.standard_normal((2, 3, 9, 11)), rng.standard_normal(ks + (3, dm)), rng.standard_normal(3 * dm)
                xt, Kt, bt = [torch.tensor(a, requires_grad=True) for a in (x, K, b)]
                xp = torch.tensor(S.pad_np(np.eye(9 * 11).reshape(9 * 11, 1, 9, 11), pad, modes))      # the halo as a matrix
                xpad = torch.einsum('ncp,pij->ncij', xt.reshape(2, 3, -1), xp[:, 0])
                y = F.conv2d(xpad, _torch_weight(Kt), bt, dilation=dil, groups=3)
                got = S.depthwise(x, K, b, pad, modes, (dil, dil))
                assert got.shape == tuple(y.shape)
                worst = max(worst, float(np.abs(got - y.detach().numpy()).max()))
                g = rng.standard_normal(got.shape)
                y.backward(torch.tensor(g))
                worst = max(worst, float(np.abs(S.depthwise_bwd_data(g, K, pad, modes, (dil, dil), 9, 11) - xt.grad.numpy()).max()))
                worst = max(worst, float(np.abs(S.depthwise_bwd_weight(x, g, pad, modes, (dil, dil), ks) - Kt.grad.numpy()).max()))
                assert np.abs(S.depthwise(x, K, b, pad, modes, (dil, dil), 'tanh') - np.tanh(got)).max() == 0
    print('\nMEASURED depthwise restatement %r against torch float64: %.3g' % (ks, worst))
    assert worst <= 1e-11


def test_pointwise_restatement_and_adjoints_equal_float64_torch():
    rng = np.random.default_rng(2)
    for q in S.PW_Q:
        for o in S.PW_O:
            x, P, b = rng.standard_normal((3, q, 35)), rng.standard_normal((q, o)), rng.standard_normal(o)
            xt, Pt, bt = [torch.tensor(a, requires_grad=True) for a in (x, P, b)]
            y = F.conv2d(xt.reshape(3, q, 5, 7), Pt.t().reshape(o, q, 1, 1), bt).reshape(3, o, 35)
            got = S.pointwise(x, P, b)
            assert np.abs(got - y.detach().numpy()).max() <= 1e-12
            g = rng.standard_normal(got.shape)
            y.backward(torch.tensor(g))
            assert np.abs(S.pointwise_bwd_data(g, P) - xt.grad.numpy()).max() <= 1e-12
            assert np.abs(S.pointwise_bwd_weight(x, g) - Pt.grad.numpy()).max() <= 1e-11
            assert np.array_equal(S.pointwise(x, P, b, 'relu'), np.maximum(got, 0))


def test_separable_restatement_equals_the_two_torch_convolutions():
    rng = np.random.default_rng(3)
    x, K, P, b = rng.standard_normal((2, 4, 8, 9)), rng.standard_normal((3, 3, 4, 2)), rng.standard_normal((1, 1, 8, 5)), rng.standard_normal(5)
    t = F.conv2d(torch.tensor(x), _torch_weight(torch.tensor(K)), None, dilation=2, groups=4, padding=2)
    want = torch.tanh(F.conv2d(t, torch.tensor(P[0, 0].T.copy()).reshape(5, 8, 1, 1), torch.tensor(b))).numpy()
    got = S.separable(x, K, P, b, S.same_halo((3, 3), (2, 2)), dil=(2, 2), act='tanh')
    assert got.shape == want.shape == (2, 5, 8, 9) and np.abs(got - want).max() <= 1e-12


def test_case_tables_cover_what_the_kernels_branch_on():
    th, tw = S.DW_TILE
    assert any(h > th and h % th and w > tw and w % tw for _, _, h, w in S.DW_MAPS)       # several ragged tiles on both axes
    assert S.dw_partials(2, 37, 70) > 1 and S.pw_partials(3, 990) > 1
    assert {q % 2 for q in S.PW_Q} == {0, 1} and max(S.PW_O) > 32 and any(hw % 32 for hw in S.PW_HW)
    assert 16 * 3 * 990 < 2 ** 24 and 16 * 2 * 37 * 70 < 2 ** 24                          # the integer cases stay exact in float32


# -- the layers ----------------------------------------------------------------------------------------------------------------------- #
def test_shapes_halos_and_fans():
    lay = L.SeparableConv2D(6, (3, 5), dilation_rate=2, depth_multiplier=2, padding='same', **CF)
    assert lay.compute_output_shape((4, 9, 12)) == (6, 9, 12) and lay.same_halo() == S.same_halo((3, 5), (2, 2)) == (2, 2, 4, 4)
    assert L.SeparableConv2D(6, (3, 5), dilation_rate=2, **CF).compute_output_shape((4, 9, 12)) == (6, 5, 4)
    dw = L.DepthwiseConv2D((2, 3), depth_multiplier=3, **CF)
    assert dw.compute_output_shape((4, 9, 12)) == (12, 8, 10) and dw.same_halo() == (0, 1, 1, 1)
    with pytest.raises(ValueError, match='does not fit'):
        L.DepthwiseConv2D(7, dilation_rate=2, **CF).compute_output_shape((4, 9, 12))
    assert S.fans((3, 5, 4, 2)) == (60, 30) and S.fans((1, 1, 8, 6)) == (8, 6)
    x0 = L.Input(shape=(4, 9, 12))
    m = Model(inputs=x0, outputs=lay(x0), device=CPU, seed=1)
    names = [nm for nm, _ in lay._weights]
    assert names == ['depthwise_kernel', 'pointwise_kernel', 'bias']                      # Keras order
    dk, pk, b = lay.get_weights()
    assert dk.shape == (3, 5, 4, 2) and pk.shape == (1, 1, 8, 6) and b.shape == (6,) and not b.any()
    for k, (fi, fo) in ((dk, (60, 30)), (pk, (8, 6))):                                    # glorot_uniform on Keras' fans
        lim = np.sqrt(6.0 / (fi + fo))
        assert np.abs(k).max() <= lim and np.abs(k).max() > 0.8 * lim
    assert lay.depthwise_part.kernel is lay.depthwise_kernel and lay.depthwise_part.bias is None
    assert lay.pointwise_part.kernel is lay.pointwise_kernel and lay.pointwise_part.bias is lay.bias
    assert lay.depthwise_part.activation == 'linear' and lay.pointwise_part.name.endswith('/pointwise')
    m = Model(inputs=x0, outputs=dw(x0), device=CPU, seed=1)
    assert [nm for nm, _ in dw._weights] == ['depthwise_kernel', 'bias'] and dw.get_weights()[1].shape == (12,)
    assert dw.depthwise_part.bias is dw.bias
    z = L.SeparableConv2D(2, 3, depthwise_initializer='zeros', pointwise_initializer='zeros', use_bias=False, **CF)
    Model(inputs=x0, outputs=z(x0), device=CPU)
    assert len(z.get_weights()) == 2 and not any(w.any() for w in z.get_weights())


def test_refusals_name_the_argument():
    for cls, args in ((L.SeparableConv2D, (4, 3)), (L.DepthwiseConv2D, (3,))):
        for kw, text in ((dict(strides=2), 'strides'), (dict(strides=(1, 2)), 'strides'), (dict(activation='elu'), 'activation'),
                         (dict(depthwise_initializer='he_normal'), 'depthwise_initializer'),
                         (dict(bias_initializer='ones'), 'bias_initializer'), (dict(depthwise_constraint='max_norm'), 'depthwise_constraint'),
                         (dict(bias_constraint='max_norm'), 'bias_constraint'), (dict(activity_regularizer='l2'), 'activity_regularizer')):
            with pytest.raises(NotImplementedError, match=text):
                cls(*args, **dict(CF, **kw))
        with pytest.raises(NotImplementedError, match='channels_first'):
            cls(*args, data_format='channels_last')
        with pytest.raises(NotImplementedError, match='channels_first'):
            cls(*args)
        for kw in (dict(dilation_rate=5), dict(depth_multiplier=9), dict(depth_multiplier=0), dict(padding='full')):
            with pytest.raises(ValueError):
                cls(*args, **dict(CF, **kw))
        with pytest.raises(ValueError):
            cls(*(args[:-1] + (8,)), **CF)
    for kw, text in ((dict(pointwise_initializer='ones'), 'pointwise_initializer'), (dict(pointwise_constraint='x'), 'pointwise_constraint')):
        with pytest.raises(NotImplementedError, match=text):
            L.SeparableConv2D(4, 3, **dict(CF, **kw))
    assert L.SeparableConv2D(4, (7, 1), dilation_rate=4, depth_multiplier=8, activation='relu', **CF).kernel_size == (7, 1)


#: keras.layers.SeparableConv2D(6, (3, 2), padding='same', data_format='channels_first', dilation_rate=2, depth_multiplier=2,
#: activation='tanh', depthwise_regularizer=l2(1e-3)).get_config() as Keras 2.2.4 writes it (keras/layers/convolutional.py:
#: _SeparableConv.get_config = Conv's keys without rank / kernel_*, + depth_multiplier and the depthwise_* / pointwise_* keys)
KERAS_SEPARABLE = json.loads("""{"name": "separable_conv2d_1", "trainable": true, "filters": 6, "kernel_size": [3, 2], "strides": [1, 1],
 "padding": "same", "data_format": "channels_first", "dilation_rate": [2, 2], "activation": "tanh", "use_bias": true,
 "bias_initializer": {"class_name": "Zeros", "config": {}}, "bias_regularizer": null, "activity_regularizer": null,
 "bias_constraint": null, "depth_multiplier": 2,
 "depthwise_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
 "pointwise_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
 "depthwise_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.001}}, "pointwise_regularizer": null,
 "depthwise_constraint": null, "pointwise_constraint": null}""")
#: keras.layers.DepthwiseConv2D(3, depth_multiplier=2, data_format='channels_first', activation='tanh').get_config(): Conv2D's keys
#: without filters / kernel_*, + depth_multiplier and the depthwise_* keys
KERAS_DEPTHWISE = json.loads("""{"name": "depthwise_conv2d_1", "trainable": true, "kernel_size": [3, 3], "strides": [1, 1],
 "padding": "valid", "data_format": "channels_first", "dilation_rate": [1, 1], "activation": "tanh", "use_bias": true,
 "bias_initializer": {"class_name": "Zeros", "config": {}}, "bias_regularizer": null, "activity_regularizer": null,
 "bias_constraint": null, "depth_multiplier": 2,
 "depthwise_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
 "depthwise_regularizer": null, "depthwise_constraint": null}""")


def test_keras_config_layout():
    from dlwp_amd import serialization as Z
    from dlwp_amd.regularizers import l2
    sep = L.SeparableConv2D(6, (3, 2), padding='same', dilation_rate=2, depth_multiplier=2, activation='tanh',
                            depthwise_regularizer=l2(1e-3), name='separable_conv2d_1', **CF)
    spec = json.loads(json.dumps(Z._keras_layer_spec(sep)))
    assert spec['class_name'] == 'SeparableConv2D' and spec['config'] == KERAS_SEPARABLE
    dw = L.DepthwiseConv2D(3, depth_multiplier=2, activation='tanh', name='depthwise_conv2d_1', **CF)
    spec = json.loads(json.dumps(Z._keras_layer_spec(dw)))
    assert spec['class_name'] == 'DepthwiseConv2D' and spec['config'] == KERAS_DEPTHWISE
    assert 'filters' not in spec['config'] and not [k for k in spec['config'] if k.startswith('kernel_') and k != 'kernel_size']
    # ... and back: the hand-written Keras config builds the same layer
    again = L.SeparableConv2D(**Z._keras_layer_kwargs(L.SeparableConv2D, KERAS_SEPARABLE))
    assert again.get_config() == sep.get_config() and again.depthwise_regularizer.l2 == pytest.approx(1e-3)
    assert again.pointwise_regularizer is None
    again = L.DepthwiseConv2D(**Z._keras_layer_kwargs(L.DepthwiseConv2D, KERAS_DEPTHWISE))
    assert again.get_config() == dw.get_config()
    cfg = sep.get_config()
    assert cfg['depth_multiplier'] == 2 and cfg['filters'] == 6 and cfg['dilation_rate'] == (2, 2)
    assert 'filters' not in dw.get_config()
    assert L.SeparableConv2D(**cfg).get_config() == cfg and L.DepthwiseConv2D(**dw.get_config()).get_config() == dw.get_config()


def test_the_keras_shim_exports_both_layers():
    import sys
    from dlwp_amd import compat
    before = {k: sys.modules.get(k) for k in list(sys.modules) if k == 'keras' or k.startswith('keras.') or k == 'DLWP' or
              k.startswith('DLWP.')}
    try:
        compat.install(force=True)
        import keras
        assert keras.layers.SeparableConv2D is L.SeparableConv2D and keras.layers.DepthwiseConv2D is L.DepthwiseConv2D
        assert keras.layers.convolutional.SeparableConv2D is L.SeparableConv2D
        assert keras.layers.convolutional.DepthwiseConv2D is L.DepthwiseConv2D
    finally:
        for k in [k for k in sys.modules if k == 'keras' or k.startswith('keras.') or k == 'DLWP' or k.startswith('DLWP.')]:
            if k in before and before[k] is not None:
                sys.modules[k] = before[k]
            else:
                del sys.modules[k]


# -- the lowering --------------------------------------------------------------------------------------------------------------------- #
def test_plan_structure():
    from dlwp_amd.custom import PeriodicPadding2D
    x0 = L.Input(shape=(4, 9, 12))
    t = L.ZeroPadding2D((1, 0), **CF)(PeriodicPadding2D((0, 1), **CF)(x0))
    sep = L.SeparableConv2D(8, 3, depth_multiplier=2, activation='tanh', name='s', **CF)
    m = Model(inputs=x0, outputs=sep(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['dwconv', 'pwconv'] == [op.kind for op in m.infer_plan.ops]
    d, p = m.plan.ops
    # the lazy halo is consumed by the stencil, which has neither bias nor activation; the intermediate tensor is a plan buffer
    assert (d.src, d.xs, tuple(d.halo), d.act, d.out_shape, d.layer) == (-1, (4, 9, 12), (1, 1, 1, 1, S.ZERO, S.WRAP), 0, (8, 9, 12), sep)
    assert d.dst >= 0 and m.plan.buffers[d.dst] == (8, 9, 12)
    assert (p.src, p.dst, p.xs, p.act, p.out_shape, tuple(p.halo)) == (d.dst, -2, (8, 9, 12), 1, (8, 9, 12), (0, 0, 0, 0, 0, 0))
    assert m.plan.sep_layers == [sep] and m.plan.output_store == [(8, 9, 12)] and 'dwconv' in m.plan.describe()
    # 'same' zeros compose with a zero halo and not with the periodic columns: the halo is materialised first
    m = Model(inputs=x0, outputs=L.DepthwiseConv2D(3, padding='same', activation='relu', **CF)(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['pad', 'dwconv']
    assert tuple(m.plan.ops[1].halo) == (1, 1, 1, 1, 0, 0) and m.plan.ops[1].act == 2 and m.plan.ops[1].dst == -2
    m = Model(inputs=x0, outputs=L.DepthwiseConv2D((3, 1), padding='same', **CF)(t), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['dwconv'] and tuple(m.plan.ops[0].halo) == (2, 2, 1, 1, S.ZERO, S.WRAP)


def test_channel_slice_lazy_views_and_second_application():
    from dlwp_amd.custom import slice_layer
    x0 = L.Input(shape=(5, 8, 12))
    m = Model(inputs=x0, outputs=L.SeparableConv2D(4, 3, **CF)(slice_layer(1, 4, axis=1)(x0)), device=CPU)
    d = m.plan.ops[0]
    assert [op.kind for op in m.plan.ops] == ['dwconv', 'pwconv'] and (d.src, d.xs, d.in_c_off, d.in_c_total) == (-1, (3, 8, 12), 1, 5)
    # a lazy pooling / up-sampling view in front is materialised first
    c = L.Conv2D(4, 3, padding='same', **CF)(x0)
    m = Model(inputs=x0, outputs=L.DepthwiseConv2D(3, **CF)(L.MaxPooling2D(2, **CF)(c)), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['conv', 'maxpool', 'dwconv'] and m.plan.ops[2].xs == (4, 4, 6)
    m = Model(inputs=x0, outputs=L.SeparableConv2D(2, 3, **CF)(L.UpSampling2D(2, **CF)(c)), device=CPU)
    assert [op.kind for op in m.plan.ops] == ['conv', 'upsample', 'dwconv', 'pwconv'] and m.plan.output_store == [(2, 14, 22)]
    for twice in (L.SeparableConv2D(5, 3, padding='same', name='twice', **CF), L.DepthwiseConv2D(3, padding='same', name='twice', **CF)):
        x1 = L.Input(shape=(5, 8, 8))
        with pytest.raises(NotImplementedError, match='twice.*more than once'):
            Model(inputs=x1, outputs=twice(twice(x1)), device=CPU).plan


def test_build_model_takes_the_layers_by_name():
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model((('PeriodicPadding2D', ((0, 1),), dict(CF, input_shape=(4, 9, 12))),
                   ('ZeroPadding2D', ((1, 0),), dict(CF)),
                   ('SeparableConv2D', (64, 3), dict(CF, activation='tanh')),
                   ('DepthwiseConv2D', (3,), dict(CF, padding='same')),
                   ('SeparableConv2D', (4, 1), dict(CF))), loss='mse', optimizer='adam')
    assert [op.kind for op in d.model.plan.ops] == ['dwconv', 'pwconv', 'dwconv', 'dwconv', 'pwconv']
    tr = d.model._trainer
    assert [(lay.name.split('_')[0], nm) for lay, nm, _, _, _ in tr.entries] == \
        [('separable', 'depthwise_kernel'), ('separable', 'pointwise_kernel'), ('separable', 'bias'), ('depthwise', 'depthwise_kernel'),
         ('depthwise', 'bias'), ('separable', 'depthwise_kernel'), ('separable', 'pointwise_kernel'), ('separable', 'bias')]


def test_l2_on_both_kernels_is_the_trainers():
    from dlwp_amd.regularizers import l2
    from dlwp_amd.training import Adam
    x0 = L.Input(shape=(3, 6, 7))
    lay = L.SeparableConv2D(4, 3, depthwise_regularizer=l2(0.5), pointwise_regularizer=l2(0.25), **CF)
    m = Model(inputs=x0, outputs=lay(x0), device=CPU, seed=2)
    m.compile(optimizer=Adam(lr=1e-3), loss='mse')
    tr = m._trainer
    regs = sorted((l2v, numel) for l2v, _, numel in tr._regularized())
    assert regs == [(0.25, 12), (0.5, 27)]
    dk, pk, _ = [w.astype(np.float64) for w in lay.get_weights()]
    assert tr._regularizer_loss() == pytest.approx(0.5 * (dk ** 2).sum() + 0.25 * (pk ** 2).sum(), rel=1e-5)


# -- model files ---------------------------------------------------------------------------------------------------------------------- #
def small_net(device=CPU, seed=1, l2=None):
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.regularizers import l2 as l2_reg
    reg = dict(depthwise_regularizer=l2_reg(l2), pointwise_regularizer=l2_reg(2 * l2)) if l2 else {}
    x0 = L.Input(shape=(4, 8, 12))
    t = L.ZeroPadding2D((2, 0), **CF)(PeriodicPadding2D((0, 2), **CF)(x0))
    t = L.SeparableConv2D(8, 3, dilation_rate=2, depth_multiplier=2, activation='tanh', **dict(CF, **reg))(t)
    t = L.DepthwiseConv2D((3, 2), depth_multiplier=2, padding='same', activation='relu', use_bias=False, **CF)(t)
    return Model(inputs=x0, outputs=L.SeparableConv2D(4, 1, **CF)(t), device=device, seed=seed)


@pytest.mark.parametrize('fmt', ['npz', 'keras'])
def test_model_files_round_trip_on_the_host(tmp_path, fmt):
    from dlwp_amd import serialization as Z
    m = small_net(seed=3, l2=1e-4)
    rng = np.random.default_rng(8)
    m.set_weights([rng.standard_normal(w.shape).astype(np.float32) for w in m.get_weights()])
    path = str(tmp_path / ('m.%s' % fmt))
    Z.save_model_file(m, path, format=fmt)
    m2 = Z.load_model_file(path, device=CPU)
    assert [type(l).__name__ for l in m2.layers] == [type(l).__name__ for l in m.layers]
    assert [l.get_config() for l in m2.layers] == [l.get_config() for l in m.layers]
    seps = [l for l in m2.layers if isinstance(l, L.SeparableConv2D)]
    assert [(getattr(l.depthwise_regularizer, 'l2', None), getattr(l.pointwise_regularizer, 'l2', None)) for l in seps] == \
        [(pytest.approx(1e-4), pytest.approx(2e-4)), (None, None)]
    assert [(op.kind, op.src, op.dst, op.xs, tuple(op.halo)) for op in m2.plan.ops] == \
        [(op.kind, op.src, op.dst, op.xs, tuple(op.halo)) for op in m.plan.ops]
    assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))
    if fmt == 'keras':          # class names, weight names and their order as Keras writes them
        text = open(path, 'rb').read()
        for name in (b'SeparableConv2D', b'DepthwiseConv2D', b'depthwise_kernel:0', b'pointwise_kernel:0', b'bias:0'):
            assert name in text, name


def test_keras_2_2_sequential_with_both_layers_instantiates(tmp_path):
    """a checkpoint as Keras 2.2.4 lays it out (hand-written: no Keras here): config keys, weight names and their order"""
    from dlwp_amd import hdf5_lite, serialization
    c1 = dict(KERAS_SEPARABLE, batch_input_shape=[None, 4, 8, 12], dtype='float32')
    c2 = dict(KERAS_DEPTHWISE)
    config = {'class_name': 'Sequential', 'config': {'name': 'sequential_1', 'layers': [
        {'class_name': 'SeparableConv2D', 'config': c1}, {'class_name': 'DepthwiseConv2D', 'config': c2}]}}
    rng = np.random.default_rng(2)
    arrays = {'separable_conv2d_1': [('depthwise_kernel:0', (3, 2, 4, 2)), ('pointwise_kernel:0', (1, 1, 8, 6)), ('bias:0', (6,))],
              'depthwise_conv2d_1': [('depthwise_kernel:0', (3, 3, 6, 2)), ('bias:0', (12,))]}
    root = hdf5_lite.GroupSpec()
    root.attrs['keras_version'] = b'2.2.4'
    root.attrs['backend'] = b'tensorflow'
    root.attrs['model_config'] = json.dumps(config).encode('utf-8')
    mw = root.create_group('model_weights')
    mw.attrs['layer_names'] = np.array([k.encode() for k in arrays])
    vals = {}
    for lname, ws in arrays.items():
        g = mw.create_group(lname)
        g.attrs['weight_names'] = np.array([('%s/%s' % (lname, nm)).encode() for nm, _ in ws])
        for nm, shape in ws:
            vals[(lname, nm)] = rng.standard_normal(shape).astype(np.float32)
            g.create_dataset('%s/%s' % (lname, nm), vals[(lname, nm)])
    path = str(tmp_path / 'sep.h5')
    hdf5_lite.write_file(path, root)
    m = serialization.import_keras_hdf5(path, device=CPU)
    sep = [l for l in m.layers if isinstance(l, L.SeparableConv2D)][0]
    dw = [l for l in m.layers if type(l) is L.DepthwiseConv2D][0]
    assert sep.dilation_rate == (2, 2) and sep.depth_multiplier == 2 and sep.depthwise_regularizer.l2 == pytest.approx(1e-3)
    assert m.plan.output_store == [(12, 6, 10)] and [op.kind for op in m.plan.ops] == ['dwconv', 'pwconv', 'dwconv']
    for lay, lname in ((sep, 'separable_conv2d_1'), (dw, 'depthwise_conv2d_1')):
        for (nm, _), a in zip(lay._weights, lay.get_weights()):
            assert np.array_equal(a, vals[(lname, nm + ':0')])


# -- C ABI ---------------------------------------------------------------------------------------------------------------------------- #
NEW = {'dlwp_depthwise2d_out_shape': 3, 'dlwp_depthwise2d_fwd': 9, 'dlwp_depthwise2d_bwd_data': 8, 'dlwp_depthwise2d_bwd_workspace': 2,
       'dlwp_depthwise2d_bwd_weight': 10, 'dlwp_pointwise2d_fwd': 10, 'dlwp_pointwise2d_bwd_data': 9,
       'dlwp_pointwise2d_bwd_workspace': 3, 'dlwp_pointwise2d_bwd_weight': 11}


def test_entry_points_are_exported_declared_and_bound():
    from dlwp_amd import _lib
    names = _lib.declared_symbols()
    for n, nargs in NEW.items():
        assert n in names and hasattr(_lib.lib, n)
        assert len(getattr(_lib.lib, n).argtypes) == nargs
    header = open(_lib.HEADER_PATH).read()
    for name, num in (('DEPTHWISE2D', 21), ('POINTWISE2D', 22)):
        assert re.search(r'#define\s+DLWP_OP_%s\s+%d\b' % (name, num), header) and getattr(_lib, 'OP_' + name) == num
    assert _lib.OP_SPACE2DEPTH_PAD == 20                                     # appended: no existing value moved
    assert ctypes.sizeof(_lib.Depthwise2d) == 5 * 4 + 24 + 5 * 4 and ctypes.sizeof(_lib.Pointwise2d) == 7 * 4
    assert ctypes.sizeof(_lib.Op) == 5 * 4 + 16 + ctypes.sizeof(_lib.Conv2d) + 24 + 4 * 4 + 3 * 4 + ctypes.sizeof(_lib.Conv2d)
    src = open(_lib.HEADER_PATH.replace('include/dlwp_hip.h', 'dlwp_amd/csrc/sepconv.hip')).read()
    assert 'atomic' not in src.split('#include')[1] and src.count('DLWP_TAPE(') == 6


def test_out_shape_and_workspace_queries():
    from dlwp_amd import _lib, ops
    d = ops.make_depthwise(3, 5, (2, 1), 3, ops.make_pad(2, 2, 1, 0, S.ZERO, S.WRAP), in_c_off=1, in_c_total=6)
    ys = ops.depthwise_out_shape(_lib.Shape4(2, 4, 9, 12), d)
    assert (ys.n, ys.c, ys.h, ys.w) == (2, 12, 9, 9) == (2, 12) + S.out_hw(9, 12, (2, 2, 1, 0), (3, 5), (2, 1))
    assert _lib.lib.dlwp_depthwise2d_bwd_workspace(_lib.Shape4(2, 4, 9, 12), d) == S.dw_partials(2, 9, 9) * 3 * 5 * 4 * 3 * 4
    assert _lib.lib.dlwp_depthwise2d_bwd_workspace(_lib.Shape4(2, 3, 37, 70), ops.make_depthwise(1, 1)) == 2 * 3 * 4
    p = ops.make_pointwise(33, 35)
    assert _lib.lib.dlwp_pointwise2d_bwd_workspace(3, 990, p) == S.pw_partials(3, 990) * 33 * 35 * 4 == 6 * 33 * 35 * 4
    assert _lib.lib.dlwp_pointwise2d_bwd_workspace(1, 35, p) == 33 * 35 * 4


def test_entry_point_refusals_without_a_device():
    """bad sizes, halos that do not fit the map, bad channel windows, null pointers, a null handle: refused in that order"""
    from dlwp_amd import _lib, ops
    lib, F32 = _lib.lib, _lib.F32
    one = ctypes.c_void_p(16)           # (never dereferenced: every call below is refused before a launch)
    xs = _lib.Shape4(1, 3, 6, 8)

    def refused(rc, text):
        name, _, rest = text.rpartition(': ')
        msg = lib.dlwp_last_error().decode()
        assert rc != 0 and msg.startswith(name) and rest in msg, msg
    ok = ops.make_depthwise(3, 3)
    calls = (('dlwp_depthwise2d_fwd', lambda a, b, s, d: lib.dlwp_depthwise2d_fwd(None, a, b, None, one if a and b else None, s, d, F32, None)),
             ('dlwp_depthwise2d_bwd_data', lambda a, b, s, d: lib.dlwp_depthwise2d_bwd_data(None, a, b, one if a and b else None, s, d, F32, None)),
             ('dlwp_depthwise2d_bwd_weight', lambda a, b, s, d: lib.dlwp_depthwise2d_bwd_weight(None, a, b, one if a and b else None, s, d,
                                                                                                 one, 0, F32, None)))
    for name, fn in calls:
        refused(fn(one, one, xs, ok), name + ': null handle')
        for bad, text in ((ops.make_depthwise(0, 3), 'kernel size'), (ops.make_depthwise(3, 8), 'kernel size'),
                          (ops.make_depthwise(3, 3, 5), 'dilation'), (ops.make_depthwise(3, 3, 1, 9), 'depth_multiplier'),
                          (ops.make_depthwise(3, 3, 1, 0), 'depth_multiplier'), (ops.make_depthwise(3, 3, act=3), 'unknown activation'),
                          (ops.make_depthwise(3, 3, halo=ops.make_pad(0, -1, 0, 0)), 'negative padding'),
                          (ops.make_depthwise(3, 3, halo=ops.make_pad(0, 0, 0, 0, 5, 0)), 'unknown pad mode'),
                          (ops.make_depthwise(3, 3, halo=ops.make_pad(0, 0, 9, 9, S.ZERO, S.WRAP)), 'the column halo'),
                          (ops.make_depthwise(3, 3, halo=ops.make_pad(6, 0, 0, 0, S.REFLECT, S.ZERO)), 'the row halo'),
                          (ops.make_depthwise(7, 3), 'larger than the padded input'),
                          (ops.make_depthwise(3, 3, in_c_off=1, in_c_total=3), 'the input channel window'),
                          (ops.make_depthwise(3, 3, 1, 2, out_c_off=1, out_c_total=6), 'the output channel window')):
            refused(fn(one, one, xs, bad), '%s: %s' % (name, text))
        for s in (_lib.Shape4(-1, 3, 6, 8), _lib.Shape4(1, 0, 6, 8), _lib.Shape4(1, 3, 0, 8), _lib.Shape4(1, 3, 6, 0)):
            refused(fn(one, one, s, ok), name + ': bad input shape')
        # a halo that does not fit is reported in front of a bad window, a bad window in front of a null pointer, that in front of the handle
        both = ops.make_depthwise(3, 3, halo=ops.make_pad(0, 0, 9, 9, S.ZERO, S.WRAP), in_c_off=1, in_c_total=3)
        refused(fn(None, None, xs, both), name + ': the column halo')
        refused(fn(None, None, xs, ops.make_depthwise(3, 3, in_c_off=1, in_c_total=3)), name + ': the input channel window')
        for a, b in ((None, one), (one, None), (None, None)):
            refused(fn(a, b, xs, ok), name + ': null pointer')
    refused(lib.dlwp_depthwise2d_fwd(None, one, one, None, one, xs, ok, _lib.BF16, None), 'dlwp_depthwise2d_fwd: dtype')
    refused(lib.dlwp_depthwise2d_out_shape(xs, ok, None), 'dlwp_depthwise2d_out_shape: null pointer')
    okp = ops.make_pointwise(3, 4)
    pcalls = (('dlwp_pointwise2d_fwd', lambda a, b, n, hw, d: lib.dlwp_pointwise2d_fwd(None, a, b, None, one if a and b else None, n, hw, d,
                                                                                         F32, None)),
              ('dlwp_pointwise2d_bwd_data', lambda a, b, n, hw, d: lib.dlwp_pointwise2d_bwd_data(None, a, b, one if a and b else None, n, hw,
                                                                                                   d, F32, None)),
              ('dlwp_pointwise2d_bwd_weight', lambda a, b, n, hw, d: lib.dlwp_pointwise2d_bwd_weight(None, a, b, one if a and b else None, n,
                                                                                                       hw, d, one, 0, F32, None)))
    for name, fn in pcalls:
        refused(fn(one, one, 2, 35, okp), name + ': null handle')
        for n, hw, d in ((-1, 35, okp), (2, 0, okp), (2, 35, ops.make_pointwise(0, 4)), (2, 35, ops.make_pointwise(3, 0))):
            refused(fn(one, one, n, hw, d), name + ': bad sizes')
        refused(fn(one, one, 2, 35, ops.make_pointwise(3, 4, act=7)), name + ': unknown activation')
        refused(fn(one, one, 2, 35, ops.make_pointwise(3, 4, in_c_off=2, in_c_total=4)), name + ': the input channel window')
        refused(fn(one, one, 2, 35, ops.make_pointwise(3, 4, out_c_off=-1, out_c_total=9)), name + ': the output channel window')
        refused(fn(None, None, 2, 35, ops.make_pointwise(3, 4, in_c_off=2, in_c_total=4)), name + ': the input channel window')
        for a, b in ((None, one), (one, None), (None, None)):
            refused(fn(a, b, 2, 35, okp), name + ': null pointer')
    refused(lib.dlwp_pointwise2d_fwd(None, one, one, None, one, 2, 35, okp, _lib.BF16, None), 'dlwp_pointwise2d_fwd: dtype')
    # an empty batch has no pointers and gets as far as the handle
    refused(lib.dlwp_depthwise2d_fwd(None, None, None, None, None, _lib.Shape4(0, 3, 6, 8), ok, F32, None), 'null handle')
    refused(lib.dlwp_pointwise2d_fwd(None, None, None, None, None, 0, 35, okp, F32, None), 'null handle')
