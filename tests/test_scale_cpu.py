"""The wrapper's scaler and imputer on the device, the parts that need no GPU: the numpy restatement of the pinned arithmetic
(include/dlwp_hip.h: dlwp_scale_fwd / dlwp_scale_inv) against scikit-learn bit for bit, the eligibility rules of
DLWPNeuralNet.device_transform_stages, the 'scale' ops of plan.build_plan(transform=...), and the header against the bindings.
tests/test_gpu_scale.py compares the kernels against the same restatement."""
import os
import re

import numpy as np
import pytest
import torch

from dlwp_amd import plan as P
from dlwp_amd.model import DLWPNeuralNet
from tests.test_dense_cpu import feed_forward_layers

sklearn = pytest.importorskip('sklearn')
from sklearn.impute import SimpleImputer  # noqa: E402
from sklearn.preprocessing import MinMaxScaler, StandardScaler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------------- #
# the restatement: what numpy does when sklearn updates a float32 array in place with float64 parameters -- every stage in
# double, rounded to float32 before the next one
# ----------------------------------------------------------------------------------------------------------------------- #
def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def np_sub_div(x, sub, div):
    x = np.array(x, dtype=np.float32)
    if sub is not None:
        x = (x.astype(np.float64) - _f64(sub)).astype(np.float32)
    if div is not None:
        x = (x.astype(np.float64) / _f64(div)).astype(np.float32)
    return x


def np_mul_add(x, mul, add):
    x = np.array(x, dtype=np.float32)
    if mul is not None:
        x = (x.astype(np.float64) * _f64(mul)).astype(np.float32)
    if add is not None:
        x = (x.astype(np.float64) + _f64(add)).astype(np.float32)
    return x


def np_impute(x, stat):
    x = np.array(x, dtype=np.float32)
    if stat is None:
        return x
    return np.where(np.isnan(x), np.broadcast_to(_f64(stat).astype(np.float32), x.shape), x)


def np_scale_fwd(x, kind, fill=None, shift=None, scale=None):
    """impute, then StandardScaler.transform ('standard': shift = mean_) or MinMaxScaler.transform ('minmax': shift = min_)"""
    x = np_impute(x, fill)
    return np_sub_div(x, shift, scale) if kind == 'standard' else np_mul_add(x, scale, shift)


def np_scale_inv(x, kind, shift=None, scale=None):
    """StandardScaler.inverse_transform / MinMaxScaler.inverse_transform"""
    return np_mul_add(x, scale, shift) if kind == 'standard' else np_sub_div(x, shift, scale)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _data(n=64, f=37, seed=0):
    """features of very different magnitude, one constant column (sklearn sets its scale_ to 1)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, f)) * 10.0 ** rng.integers(-3, 4, size=f) + rng.standard_normal(f) * 50).astype(np.float32)
    x[:, 5] = np.float32(3.25)
    return x


@pytest.mark.parametrize('with_mean', [True, False])
@pytest.mark.parametrize('with_std', [True, False])
def test_restatement_equals_standard_scaler_bit_for_bit(with_mean, with_std):
    x = _data()
    sc = StandardScaler(with_mean=with_mean, with_std=with_std).fit(x)
    if with_std:
        assert sc.scale_[5] == 1.0 and sc.scale_.dtype == np.float64
    y = _data(19, seed=1)
    shift, scale = (sc.mean_ if with_mean else None), (sc.scale_ if with_std else None)
    t = sc.transform(y)
    assert t.dtype == np.float32
    assert np.array_equal(_bits(t), _bits(np_scale_fwd(y, 'standard', shift=shift, scale=scale)))
    assert np.array_equal(_bits(sc.inverse_transform(t)), _bits(np_scale_inv(t, 'standard', shift=shift, scale=scale)))


@pytest.mark.parametrize('feature_range', [(0, 1), (-1, 2)])
def test_restatement_equals_minmax_scaler_bit_for_bit(feature_range):
    x = _data()
    sc = MinMaxScaler(feature_range=feature_range).fit(x)
    assert sc.scale_[5] == feature_range[1] - feature_range[0]            # the constant column: data range 0 counts as 1
    y = _data(19, seed=1)
    t = sc.transform(y)
    assert t.dtype == np.float32
    assert np.array_equal(_bits(t), _bits(np_scale_fwd(y, 'minmax', shift=sc.min_, scale=sc.scale_)))
    assert np.array_equal(_bits(sc.inverse_transform(t)), _bits(np_scale_inv(t, 'minmax', shift=sc.min_, scale=sc.scale_)))


def test_restatement_equals_simple_imputer_bit_for_bit():
    rng = np.random.default_rng(2)
    x = _data()
    x[rng.random(x.shape) < 0.1] = np.nan
    im = SimpleImputer(missing_values=np.nan, strategy='mean', copy=False).fit(x)
    y = _data(19, seed=1)
    y[rng.random(y.shape) < 0.1] = np.nan
    y[3] = np.nan
    want = im.transform(y.copy())
    assert want.dtype == np.float32 and not np.isnan(want).any()
    assert np.array_equal(_bits(want), _bits(np_impute(y, im.statistics_)))
    # ... and in front of a scaler, as DLWPNeuralNet._prepare chains them
    sc = StandardScaler().fit(im.transform(x.copy()))
    assert np.array_equal(_bits(sc.transform(want)), _bits(np_scale_fwd(y, 'standard', im.statistics_, sc.mean_, sc.scale_)))


# ----------------------------------------------------------------------------------------------------------------------- #
# eligibility
# ----------------------------------------------------------------------------------------------------------------------- #
F = 24


def _wrapper(monkeypatch=None, on_cuda=True, layers=None, **kw):
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=False, is_recurrent=False, time_dim=2, **kw)
    d.build_model(layers or feed_forward_layers(F, reg=0.0), loss='mse', optimizer='adam')
    if on_cuda:          # (the rules read the device's type only; nothing is uploaded by device_transform_stages)
        d.model.device = torch.device('cuda', 0)
    return d


def _fit(d, x=None, **kw):
    x = _data(16, F, seed=3) if x is None else x
    d.init_fit(x, (x * 0.5 + 1).astype(np.float32), **kw)
    return d


HEAD_STD = {'kind': 'standard', 'fill': False, 'shift': True, 'scale': True}
TAIL_STD = {'kind': 'standard', 'shift': True, 'scale': True}


def test_default_wrapper_is_eligible_with_both_transforms():
    d = _fit(_wrapper())
    assert d.device_transform_stages() == {'head': HEAD_STD, 'tail': TAIL_STD}


def test_stage_flags_follow_the_scaler_and_the_wrapper_switches():
    d = _fit(_wrapper(), scaler_kwargs={'with_mean': False})
    assert d.device_transform_stages() == {'head': dict(HEAD_STD, shift=False), 'tail': dict(TAIL_STD, shift=False)}
    d = _fit(_wrapper(), scaler_kwargs={'with_std': False})
    assert d.device_transform_stages() == {'head': dict(HEAD_STD, scale=False), 'tail': dict(TAIL_STD, scale=False)}
    d = _fit(_wrapper(), scaler_kwargs={'with_mean': False, 'with_std': False})          # nothing left to launch
    assert d.device_transform_stages() == {'head': None, 'tail': None}
    d = _fit(_wrapper(scaler_type='MinMaxScaler'), scaler_kwargs={'feature_range': (-1, 2)})
    assert d.device_transform_stages() == {'head': dict(HEAD_STD, kind='minmax'), 'tail': dict(TAIL_STD, kind='minmax')}
    d = _fit(_wrapper(scale_targets=False))
    assert d.device_transform_stages() == {'head': HEAD_STD, 'tail': None}
    d = _fit(_wrapper(apply_same_y_scaling=False))
    assert d.scaler_y is not d.scaler and d.device_transform_stages() == {'head': HEAD_STD, 'tail': TAIL_STD}
    x = _data(16, F, seed=3)
    x[2, 3] = np.nan
    d = _fit(_wrapper(impute_missing=True), x)
    assert d.device_transform_stages() == {'head': dict(HEAD_STD, fill=True), 'tail': TAIL_STD}
    d = _fit(_wrapper(scaler_type=None, impute_missing=True), x)                          # an imputer alone
    assert d.device_transform_stages() == {'head': {'kind': None, 'fill': True, 'shift': False, 'scale': False}, 'tail': None}


def test_ineligible_wrappers_stay_on_the_host():
    assert _fit(_wrapper(on_cuda=False)).device_transform_stages() is False               # no CUDA device
    assert _wrapper().device_transform_stages() is False                                   # not fitted yet
    d = _fit(_wrapper())
    d.model.activation_dtype = 'bfloat16'
    assert d.device_transform_stages() is False
    d = _fit(_wrapper())
    d.gpus = 2
    assert d.device_transform_stages() is False
    d = _fit(_wrapper())
    d.model.__dict__['_driver'] = object()
    assert d.device_transform_stages() is False
    d = _fit(_wrapper())
    d.model.outputs = d.model.outputs * 2                                                  # two outputs
    assert d.device_transform_stages() is False
    assert _fit(_wrapper(scaler_type='MinMaxScaler'), scaler_kwargs={'clip': True}).device_transform_stages() is False
    assert _fit(_wrapper(scaler_type='RobustScaler')).device_transform_stages() is False

    class Mine(StandardScaler):                                                            # a subclass may override transform
        pass
    d = _fit(_wrapper())
    d.scaler = d.scaler_y = Mine().fit(_data(16, F))
    assert d.device_transform_stages() is False
    d = _fit(_wrapper())
    d.scaler_y = MinMaxScaler(clip=True).fit(_data(16, F))                                 # the output side alone
    assert d.device_transform_stages() is False
    # parameter lengths: the input side, the output side
    d = _fit(_wrapper())
    d.scaler = StandardScaler().fit(_data(16, F + 1))
    assert d.device_transform_stages() is False
    d = _fit(_wrapper())
    d.scaler_y = StandardScaler().fit(_data(16, F // 2))
    assert d.device_transform_stages() is False
    # imputers: another strategy; a column without any value (sklearn drops it: the shape changes)
    x = _data(16, F, seed=3)
    x[2, 3] = np.nan
    d = _fit(_wrapper(impute_missing=True), x)
    d.imputer = SimpleImputer(strategy='median').fit(x)
    assert d.device_transform_stages() is False
    d = _fit(_wrapper(impute_missing=True), x)
    d.imputer.statistics_ = d.imputer.statistics_.copy()
    d.imputer.statistics_[4] = np.nan
    assert d.device_transform_stages() is False


def test_the_inverse_transform_needs_a_vector_per_sample():
    """sklearn's inverse_transform refuses arrays of more than two axes, so predict() of a convolutional wrapper with scaled targets
    raises on the host; that call stays there.  Without scaled targets the same model is eligible."""
    cf = {'data_format': 'channels_first'}
    conv = (('Conv2D', (4, 3), dict(cf, padding='same', activation='tanh', input_shape=(4, 3, 2))),)
    x = _data(16, F, seed=3).reshape(16, 4, 3, 2)
    d = _wrapper(layers=conv, scaler_type='MinMaxScaler')
    d.is_convolutional = True
    d.init_fit(x, x)
    assert d.device_transform_stages() is False
    d = _wrapper(layers=conv, scaler_type='MinMaxScaler', scale_targets=False)
    d.init_fit(x, x)
    assert d.device_transform_stages() == {'head': dict(HEAD_STD, kind='minmax'), 'tail': None}


def test_host_switch_and_float64_data_keep_a_call_on_the_host(monkeypatch):
    d = _fit(_wrapper())
    made = []
    monkeypatch.setattr(d, '_sync_device_transform', lambda: made.append(1) or {'head': HEAD_STD, 'tail': TAIL_STD})
    x = _data(4, F)
    assert d._device_io(x) and made == [1]
    assert d._device_io(x.astype(np.float64)) is False and made == [1]     # sklearn would transform it in float64
    monkeypatch.setenv('DLWP_SCALER_HOST', '1')
    assert d._device_io(x) is False and made == [1]
    monkeypatch.delenv('DLWP_SCALER_HOST')
    plain = _wrapper(scaler_type=None, scale_targets=False)
    monkeypatch.setattr(plain, '_sync_device_transform', lambda: made.append(2))
    assert plain._device_io(x) is False and made == [1]                    # an identity wrapper has nothing to move


# ----------------------------------------------------------------------------------------------------------------------- #
# the plan
# ----------------------------------------------------------------------------------------------------------------------- #
def _kinds(plan):
    return [op.kind for op in plan.ops]


def _models():
    from tests.nets import unet_layers
    dense = _wrapper(on_cuda=False).model
    np.random.seed(1)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(unet_layers((4, 16, 24), widths=(8, 16, 16, 16, 8)), loss='mse', optimizer='adam')
    return [dense, d.model]


@pytest.mark.parametrize('which', [0, 1])
def test_build_plan_puts_one_scale_op_first_and_one_last(which):
    net = _models()[which]
    base = P.build_plan(net.inputs, net.outputs, inference=True)
    both = P.build_plan(net.inputs, net.outputs, inference=True, transform=(True, True))
    assert _kinds(both) == ['scale'] + _kinds(base) + ['scale']
    first, last = both.ops[0], both.ops[-1]
    assert (first.role, first.src) == ('head', P.STATE_IN) and first.dst >= 0
    assert both.buffers[first.dst] == both._in_store == tuple(first.xs)
    assert (last.role, last.src, last.dst) == ('tail', P.OUT(0), P.OUT(0)) and tuple(last.xs) == both.output_store[0]
    # every consumer of the model input reads the scaled buffer; nothing but the head op reads the input state
    assert [op for op in both.ops[1:] if op.kind != 'phasew' and op.src == P.STATE_IN] == []
    assert any(op.src == first.dst for op in both.ops[1:])
    assert any(op.src == P.STATE_IN for op in base.ops)
    head_only = P.build_plan(net.inputs, net.outputs, inference=True, transform=(True, False))
    assert _kinds(head_only) == ['scale'] + _kinds(base)
    tail_only = P.build_plan(net.inputs, net.outputs, inference=True, transform=(False, True))
    assert _kinds(tail_only) == _kinds(base) + ['scale']
    assert both.output_store == base.output_store and both.output_shapes == base.output_shapes


@pytest.mark.parametrize('which', [0, 1])
def test_training_and_default_inference_plans_are_unchanged(which):
    net = _models()[which]
    assert 'scale' not in _kinds(net.plan) and 'scale' not in _kinds(net.infer_plan)
    for inference in (False, True):
        a = P.build_plan(net.inputs, net.outputs, inference=inference)
        b = P.build_plan(net.inputs, net.outputs, inference=inference, transform=None)
        c = P.build_plan(net.inputs, net.outputs, inference=inference, transform=(False, False))
        assert _kinds(a) == _kinds(b) == _kinds(c) == _kinds(net.infer_plan if inference else net.plan)
        assert a.buffers == b.buffers == c.buffers
        assert [(op.src, op.dst) for op in a.ops] == [(op.src, op.dst) for op in c.ops]
    with pytest.raises(ValueError, match='inference'):
        P.build_plan(net.inputs, net.outputs, transform=(True, True))


def test_an_output_transform_needs_a_single_output():
    from dlwp_amd import layers as L
    from dlwp_amd.engine import Model
    cf = {'data_format': 'channels_first'}
    x = L.Input((2, 6, 8))
    a = L.Conv2D(2, 3, padding='same', **cf)(x)
    b = L.Conv2D(2, 3, padding='same', **cf)(a)
    m = Model(x, [a, b], device=torch.device('cpu'))
    with pytest.raises(ValueError, match='exactly one output'):
        P.build_plan(m.inputs, m.outputs, inference=True, transform=(True, True))
    assert _kinds(P.build_plan(m.inputs, m.outputs, inference=True, transform=(True, False)))[0] == 'scale'


def test_the_scaled_call_needs_a_transform():
    net = _models()[0]
    with pytest.raises(RuntimeError, match='set_io_transform'):
        net.predict(np.zeros((2, F), dtype=np.float32), scaled=True)


# ----------------------------------------------------------------------------------------------------------------------- #
# the ABI
# ----------------------------------------------------------------------------------------------------------------------- #
def test_header_declares_every_symbol_the_wrappers_bind():
    from dlwp_amd import _lib
    declared = set(_lib.declared_symbols())
    src = open(os.path.join(ROOT, 'dlwp_amd', 'ops.py')).read()
    start = src.index('# the wrapper\'s scaler and imputer (csrc/scale.hip)')
    section = src[start:src.index('# Dense and Dropout (csrc/dense.hip)')]
    bound = set(re.findall(r'_lib\.lib\.(dlwp_\w+)', section))
    assert bound == {'dlwp_scale_fwd', 'dlwp_scale_inv'}
    assert bound <= declared
    for name in bound:
        assert getattr(_lib.lib, name).argtypes is not None
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r'#define\s+DLWP_OP_SCALE\s+11\b', header) and _lib.OP_SCALE == 11
    assert re.search(r'#define\s+DLWP_SCALE_STANDARD\s+0\b', header) and re.search(r'#define\s+DLWP_SCALE_MINMAX\s+1\b', header)
    assert (_lib.SCALE_STANDARD, _lib.SCALE_MINMAX) == (0, 1)
    import ctypes
    assert ctypes.sizeof(_lib.Scale) == 12                                  # dlwp_scale: three ints
