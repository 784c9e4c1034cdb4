"""BatchNormalization(axis=1) without a GPU: the layer's Keras surface, its lowering into the fused plan, and the fp64 oracle the
GPU tests compare against (tests/test_gpu_batchnorm.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from dlwp_amd.engine import Model, Sequential
from dlwp_amd.presets import unet_layers

CF = {'data_format': 'channels_first'}


def bn_layers(cs, **bn_kwargs):
    """the reference U-Net stack (examples/train.py:159-219) with its five commented-out BatchNormalization lines switched on:
    one after every tanh Conv2D"""
    out = []
    for spec in unet_layers(cs):
        out.append(spec)
        if spec[0] == 'Conv2D' and spec[2].get('activation') == 'tanh':
            out.append(('BatchNormalization', None, dict({'axis': 1}, **bn_kwargs)))
    return tuple(out)


def build(specs):
    from dlwp_amd import custom
    net = Sequential(device=torch.device('cpu'))
    for name, args, kwargs in specs:
        cls = getattr(L, name, None) or getattr(custom, name)
        net.add(cls(*(args or ()), **(kwargs or {})))
    return net


# -- numpy fp64 restatement ----------------------------------------------------------------------------------------------- #
def np_bn_forward(x, gamma, beta, mm, mv, momentum, eps):
    m = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(axis=(0, 2, 3))
    var = ((x - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean[None, :, None, None]) * invstd[None, :, None, None]
    y = gamma[None, :, None, None] * xhat + beta[None, :, None, None]
    return y, mean, invstd, momentum * mm + (1 - momentum) * mean, momentum * mv + (1 - momentum) * var * m / (m - 1.0)


def np_bn_backward(x, dy, gamma, mean, invstd):
    m = x.shape[0] * x.shape[2] * x.shape[3]
    xhat = (x - mean[None, :, None, None]) * invstd[None, :, None, None]
    sdy = dy.sum(axis=(0, 2, 3))
    sdyx = (dy * xhat).sum(axis=(0, 2, 3))
    dx = (gamma * invstd)[None, :, None, None] * (dy - (sdy[None, :, None, None] + xhat * sdyx[None, :, None, None]) / m)
    return dx, sdyx, sdy


def test_defaults_weights_and_split():
    lay = L.BatchNormalization()
    assert (lay.axis, lay.momentum, lay.epsilon, lay.center, lay.scale) == (-1, 0.99, 1e-3, True, True)
    for center, scale, names in ((True, True, ['gamma', 'beta', 'moving_mean', 'moving_variance']),
                                 (False, True, ['gamma', 'moving_mean', 'moving_variance']),
                                 (True, False, ['beta', 'moving_mean', 'moving_variance']),
                                 (False, False, ['moving_mean', 'moving_variance'])):
        x0 = L.Input(shape=(5, 6, 7))
        bn = L.BatchNormalization(axis=1, center=center, scale=scale)
        m = Model(inputs=x0, outputs=bn(x0), device=torch.device('cpu'))
        assert [nm for nm, _ in bn._weights] == names
        ws = dict(zip(names, bn.get_weights()))
        assert all(w.shape == (5,) and w.dtype == np.float32 for w in ws.values())
        for nm in names:
            assert np.all(ws[nm] == (1.0 if nm in ('gamma', 'moving_variance') else 0.0))
        assert bn.count_params() == 5 * len(names) == m.count_params()
        trainable = [nm for nm, _ in bn._weights if nm not in bn.non_trainable_names]
        assert trainable == [nm for nm in names if nm in ('gamma', 'beta')]
        cfg = bn.get_config()
        again = L.BatchNormalization(**{k: v for k, v in cfg.items() if k != 'name'})
        assert {k: v for k, v in again.get_config().items() if k != 'name'} == {k: v for k, v in cfg.items() if k != 'name'}
        assert cfg['axis'] == 1 and cfg['center'] == center and cfg['scale'] == scale


def test_flat_parameters_leave_the_moving_statistics_out():
    from dlwp_amd.training import flatten_parameters
    net = build(bn_layers((4, 16, 24)))
    bns = [lay for lay in net.layers if isinstance(lay, L.BatchNormalization)]
    before = [lay.moving_mean for lay in bns]
    flat, entries = flatten_parameters(net)
    names = {(lay.name, nm) for lay, nm, _, _, _ in entries}
    for lay, mm in zip(bns, before):
        assert (lay.name, 'gamma') in names and (lay.name, 'beta') in names
        assert (lay.name, 'moving_mean') not in names and (lay.name, 'moving_variance') not in names
        assert lay.moving_mean is mm                                       # never re-homed: captured graphs keep reading it
    assert flat.numel() == sum(e[3] for e in entries)
    assert net.count_params() == flat.numel() + sum(2 * lay.moving_mean.numel() for lay in bns)


@pytest.mark.parametrize('kwargs, word', [
    ({'axis': 2}, 'axis'), ({'axis': 0}, 'axis'), ({'beta_regularizer': 'l2'}, 'beta_regularizer'),
    ({'gamma_regularizer': 'l2'}, 'gamma_regularizer'), ({'beta_constraint': 'max_norm'}, 'beta_constraint'),
    ({'gamma_constraint': 'max_norm'}, 'gamma_constraint'), ({'renorm': True}, 'renorm'),
    ({'virtual_batch_size': 4}, 'virtual_batch_size'), ({'adjustment': lambda s: s}, 'adjustment'),
    ({'trainable': False}, 'trainable'), ({'gamma_initializer': 'glorot_uniform'}, 'gamma_initializer')])
def test_unsupported_arguments_raise(kwargs, word):
    with pytest.raises(NotImplementedError, match=word):
        L.BatchNormalization(**kwargs)


def test_unsupported_inputs_raise():
    x0 = L.Input(shape=(5, 6, 7))
    with pytest.raises(NotImplementedError, match='axis'):
        L.BatchNormalization()(x0)                                # Keras' default axis=-1 is W on a channels_first tensor
    x5 = L.Input(shape=(2, 5, 6, 7))                              # what ConvLSTM2D(return_sequences=True) produces
    with pytest.raises(NotImplementedError, match='4-D'):
        L.BatchNormalization(axis=1)(x5)
    assert L.BatchNormalization(axis=-3)(x0).shape == (5, 6, 7)


def test_plan_of_the_reference_stack():
    net = build(bn_layers((4, 32, 48)))
    bns = [lay for lay in net.layers if isinstance(lay, L.BatchNormalization)]
    assert len(bns) == 5
    for plan in (net.plan, net.infer_plan):
        ops = plan.ops
        bn_ops = [op for op in ops if op.kind == 'bn']
        assert [op.layer for op in bn_ops] == bns == plan.bn_layers
        bn_src = {op.src for op in bn_ops}
        bn_dst = {op.dst for op in bn_ops}
        for op in bn_ops:
            writer = [o for o in ops if o.dst == op.src]
            assert len(writer) == 1
            if writer[0].kind == 'upsample':      # a decoder layer restated on the low-resolution tensor: its output, up-sampled
                writer = [o for o in ops if o.dst == writer[0].src]
                assert len(writer) == 1 and writer[0].dil == (1, 1)
            assert writer[0].kind == 'conv' and writer[0].act == 1                       # the tanh convolution's own output
            assert not writer[0].out_pool and not writer[0].out_d2s
            assert plan.buffers[op.src] == plan.buffers[op.dst] == op.xs
        for op in ops:
            if op.kind == 'conv':
                assert not op.out_pool or op.dst not in bn_src                  # no pooled store of a pre-normalisation tensor
            if op.kind in ('maxpool', 'upsample', 'pad', 'copy'):
                assert op.src not in bn_src                                     # lazy views read the normalised buffer
            if op.kind == 'conv' and op.src >= 0 and op.src in bn_src:
                raise AssertionError('a convolution reads a pre-normalisation tensor: %r' % op)
        # every convolution behind a normalised tensor reads the BN output (directly, pooled or up-sampled by its loader)
        views = {op.dst: op.src for op in ops if op.kind in ('maxpool', 'upsample', 'pad', 'copy')}
        convs = [op for op in ops if op.kind == 'conv']
        assert convs[0].src == -1 and len(convs) == 6
        for op in convs[1:]:
            assert op.src in bn_dst or views.get(op.src) in bn_dst, op
        assert plan.bf16_buffers() == [] or not (set(plan.bf16_buffers()) & (bn_src | bn_dst))
    # the training forward's conv + pooling pair (dlwp_conv2d_fwd_pool2) and the pooled weight gradient find no convolution
    # whose only reader is MaxPooling2D
    from dlwp_amd.engine import Executor
    ex = Executor(net.plan, torch.device('cpu'))
    assert ex._pooled_too() == {}
    for k, op in enumerate(net.plan.ops):
        if op.kind == 'conv':
            assert not any(r.kind == 'maxpool' and r.src == op.dst for r in net.plan.ops)
    # without BatchNormalization the same stack keeps its fusions (nothing changes for models without it)
    plain = build(unet_layers((4, 32, 48)))
    assert not any(op.kind == 'bn' for op in plain.plan.ops)
    assert Executor(plain.plan, torch.device('cpu'))._pooled_too() != {}


def test_keras_name_resolution():
    from dlwp_amd import util
    import dlwp_amd.compat  # noqa: F401
    import keras.layers
    assert util.get_from_class('dlwp_amd.layers', 'BatchNormalization') is L.BatchNormalization
    assert keras.layers.BatchNormalization is L.BatchNormalization


def test_oracle_matches_torch_batch_norm_fp64():
    rng = np.random.default_rng(3)
    for n, c, h, w in ((2, 3, 5, 7), (8, 4, 22, 45), (1, 1, 3, 3)):
        x = rng.standard_normal((n, c, h, w)) * 3.0 + 10.0
        dy = rng.standard_normal((n, c, h, w))
        gamma, beta = rng.uniform(0.5, 2.0, c), rng.standard_normal(c)
        mm, mv = rng.standard_normal(c), rng.uniform(0.5, 2.0, c)
        y, mean, invstd, mm2, mv2 = np_bn_forward(x, gamma, beta, mm, mv, 0.99, 1e-3)
        xt = torch.tensor(x, requires_grad=True)
        gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
        rm, rv = torch.tensor(mm), torch.tensor(mv)
        yt = F.batch_norm(xt, rm, rv, gt, bt, training=True, momentum=1 - 0.99, eps=1e-3)
        yt.backward(torch.tensor(dy))
        np.testing.assert_allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(mm2, rm.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(mv2, rv.numpy(), rtol=1e-12, atol=1e-12)
        dx, dg, db = np_bn_backward(x, dy, gamma, mean, invstd)
        np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(dg, gt.grad.numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-10, atol=1e-12)
        # inference: the moving statistics
        yi = F.batch_norm(torch.tensor(x), torch.tensor(mm), torch.tensor(mv), torch.tensor(gamma), torch.tensor(beta),
                          training=False, eps=1e-3)
        np.testing.assert_allclose(yi.numpy(), gamma[None, :, None, None] * (x - mm[None, :, None, None]) /
                                   np.sqrt(mv[None, :, None, None] + 1e-3) + beta[None, :, None, None], rtol=1e-12)


def test_model_file_round_trip_cpu(tmp_path):
    from dlwp_amd.serialization import load_model_file
    net = build(bn_layers((4, 16, 24)))
    rng = np.random.default_rng(0)
    net.set_weights([rng.standard_normal(w.shape).astype(np.float32) for w in net.get_weights()])
    for fmt in ('keras', 'npz'):
        path = str(tmp_path / ('bn.' + fmt))
        net.save(path, format=fmt)
        m2 = load_model_file(path, device=torch.device('cpu')) if 'device' in load_model_file.__code__.co_varnames \
            else load_model_file(path)
        assert [type(lay).__name__ for lay in m2.layers if isinstance(lay, L.BatchNormalization)] == ['BatchNormalization'] * 5
        assert all(np.array_equal(a, b) for a, b in zip(net.get_weights(), m2.get_weights()))
        b2 = [lay for lay in m2.layers if isinstance(lay, L.BatchNormalization)][0]
        assert (b2.axis, b2.momentum, b2.epsilon) == (1, 0.99, 1e-3)
    from dlwp_amd.serialization import keras_model_config
    cfg, _ = keras_model_config(net)
    spec = [s for s in cfg['config']['layers'] if s['class_name'] == 'BatchNormalization'][0]['config']
    assert spec['axis'] == 1 and spec['gamma_initializer']['class_name'] == 'Ones'


def test_out_of_scope_errors_without_gpu():
    from dlwp_amd.model import DLWPNeuralNet
    d = DLWPNeuralNet(is_convolutional=True, scaler_type=None, scale_targets=False)
    with pytest.raises(NotImplementedError, match='gpus > 1'):
        d.build_model(bn_layers((4, 16, 24)), gpus=2, loss='mse', optimizer='adam')
