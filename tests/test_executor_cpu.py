"""The Executor's two forward walks on the host (dlwp_amd/forward.py): the op table a rollout graph is captured from
(Executor.encode_ops) byte for byte, and the launches of Executor.run with the ops wrappers replaced by recorders -- wrapper,
scalars, descriptor bytes and WHICH tensor each argument is.  One small model per op kind; a kind without a fixture fails
test_every_op_kind_has_a_fixture.

The goldens (tests/golden/executor_ops.npz, executor_launches.json) were recorded from the commit in front of forward.py, whose
Executor spelled both walks as if / elif chains.  After a DELIBERATE change of the planner or the encoding, look at what this
test reports, then record again:

    import tests.test_executor_cpu as t
    t.record()

Run with no DLWP_* variable set (they change plans and layouts)."""
import ctypes
import functools
import json
import numbers
import os

import numpy as np
import pytest
import torch

from dlwp_amd import _lib, custom as C, forward as F, layers as L, ops, presets
from dlwp_amd.engine import Model, ScaleStage

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')
N = 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OPS_NPZ, LAUNCHES_JSON = os.path.join(GOLDEN, 'executor_ops.npz'), os.path.join(GOLDEN, 'executor_launches.json')

#: every ops wrapper Executor.run launches through
WRAPPERS = ('conv2d', 'convlstm_step', 'convlstm_conv', 'rowconv2d', 'phase_weights', 'depth_to_space2', 'tconv_weights',
            'depth_to_space2_crop', 'crop2d', 'sconv_weights', 'depthwise2d', 'pointwise2d', 'space_to_depth2_pad', 'pad2d',
            'maxpool2', 'avgpool2', 'upsample2', 'upsample2_bilinear', 'copy_channels', 'dense_fwd', 'dropout_fwd',
            'batchnorm_fwd_train', 'batchnorm_fwd_infer', 'activation_fwd', 'merge_fwd', 'scale_fwd', 'scale_inv', 'convlstm_gates')


# -- the models ------------------------------------------------------------------------------------------------------------ #
def X(*shape):
    return L.Input(shape=shape or (4, 16, 24))


def conv(t, f=8, k=3, **kw):
    return L.Conv2D(f, k, **dict(CF, **dict({'padding': 'same'}, **kw)))(t)


def _stack(specs):
    t = x = None
    for name, a, kw in specs:
        kw = dict(kw or {})
        if x is None:
            t = x = L.Input(shape=kw.pop('input_shape'))
        t = (getattr(L, name, None) or getattr(C, name))(*(a or ()), **kw)(t)
    return x, t


def _unet():
    return _stack(presets.unet_layers((4, 16, 24)))


def _unet_rows():
    return _stack(presets.unet_layers((4, 16, 24), latitude_dependent=True))


def _lstm_unet():
    return _stack(presets.lstm_unet_layers((2, 3, 16, 24)))


def _lstm_unet_bf16():          # 16 gate filters: the octet layout and the fused cell forms apply
    return _stack(presets.lstm_unet_layers((2, 4, 16, 24)))


def _bilinear():
    x = X()
    return x, conv(L.UpSampling2D(2, interpolation='bilinear', **CF)(x))


def _separable():
    x = X()
    return x, conv(L.SeparableConv2D(8, 3, activation='tanh', **CF)(x))


def _depthwise():
    x = X()
    return x, L.DepthwiseConv2D(3, depth_multiplier=2, padding='same', activation='relu', **CF)(x)


def _strided():
    x = X()
    return x, conv(x, strides=2)


def _transposed_cropped():
    x = X()
    return x, conv(L.Cropping2D(1, **CF)(L.Conv2DTranspose(6, 4, strides=2, **CF)(x)))


def _crop():
    x = X()
    return x, L.Cropping2D(((1, 2), (0, 3)), **CF)(L.ChannelSlice(1, 3)(x))


def _direct_outputs():          # a padding layer, both poolings and a nearest up-sampling, each feeding an output itself
    x = X()
    return x, [L.ZeroPadding2D(1, **CF)(x), L.MaxPooling2D(2, **CF)(x), L.AveragePooling2D(2, **CF)(x), L.UpSampling2D(2, **CF)(x)]


def _pad_channels_last():
    x = X(16, 24, 4)
    return x, L.ZeroPadding2D((1, 2), data_format='channels_last')(x)


def _same_tensor_twice():
    x = X()
    c = conv(x)
    return x, [c, c]


def _batchnorm():
    x = X()
    return x, L.BatchNormalization(axis=1)(conv(x))


def _activation():
    x = X()
    return x, L.LeakyReLU(0.1)(L.Activation('relu')(L.UpSampling2D(2, **CF)(conv(x))))


def _add():
    x = X()
    return x, L.Add()([conv(x), conv(x)])


def _dense():
    x = X()
    t = L.Dropout(0.25, seed=7)(L.Dense(32, activation='tanh')(L.Flatten()(L.MaxPooling2D(2, **CF)(conv(x)))))
    return x, L.Reshape((4, 16, 24))(L.Dense(4 * 16 * 24)(t))


def _scaled():
    x = X()
    return x, conv(conv(x), f=4)


MODELS = {'unet': _unet, 'unet_rows': _unet_rows, 'lstm_unet': _lstm_unet, 'lstm_unet_bf16': _lstm_unet_bf16,
          'bilinear': _bilinear, 'separable': _separable, 'depthwise': _depthwise, 'strided': _strided,
          'transposed_cropped': _transposed_cropped, 'crop': _crop, 'direct_outputs': _direct_outputs,
          'pad_channels_last': _pad_channels_last, 'same_tensor_twice': _same_tensor_twice, 'batchnorm': _batchnorm,
          'activation': _activation, 'add': _add, 'dense': _dense, 'scaled': _scaled}


@functools.lru_cache(maxsize=None)
def model(name):
    x, outs = MODELS[name]()
    m = Model(inputs=x, outputs=outs, device=CPU, seed=0)
    if name == 'lstm_unet_bf16':
        m.set_activation_dtype('bfloat16')
    if name == 'scaled':
        f = 4 * 16 * 24
        v = np.arange(1, f + 1, dtype=np.float64)
        m.set_io_transform(ScaleStage('standard', fill=v, shift=v / 2, scale=v / 3, device=CPU),
                           ScaleStage('minmax', shift=v / 5, scale=v / 7, device=CPU))
    return m


def executors(name):
    """{'infer' | 'train' | 'scaled': Executor} of a model; 'train' only where training runs another plan"""
    m = model(name)
    found = {'infer': m.executor}
    if m.train_executor is not m.executor:
        found['train'] = m.train_executor
    if m._scaled is not None:
        found['scaled'] = m._scaled
    return found


def executor(key):
    name, which = key.split('/')
    return executors(name)[which]


TRAIN_PLANS = ('unet', 'unet_rows', 'lstm_unet', 'lstm_unet_bf16', 'dense')      # training runs a plan of its own
EXECUTOR_KEYS = ['%s/infer' % name for name in MODELS] + ['%s/train' % name for name in TRAIN_PLANS] + ['scaled/scaled']
TABLE_KEYS = [key for key in EXECUTOR_KEYS if key != 'dense/train']            # (a plan with a 'dropout' op has no table)


# -- what a tensor is ------------------------------------------------------------------------------------------------------ #
def names_of(name, ex, x=None, outs=None, bufs=None):
    """{data_ptr: what the tensor is}: model input, output slot, scratch buffer, a layer's parameter (layers by their position in
    the model: automatic names depend on what the process built before), derived kernel, scaler parameter, BN state"""
    m, found = model(name), {}

    def put(t, what):
        if t is not None and t.numel():
            found.setdefault(t.data_ptr(), what)
    put(x, 'input')
    for i, t in enumerate(outs or ()):
        put(t, 'out[%d]' % i)
    for i, t in enumerate(bufs if bufs is not None else ex.scratch(N)):
        put(t, 'scratch[%d]' % i)
    for i, lay in enumerate(m.layers):
        for nm, w in lay._weights:
            put(w, '%d:%s.%s' % (i, type(lay).__name__, nm))
    for i, (w2, b2) in enumerate(ex.phase_buffers()):
        put(w2, 'derived[%d].kernel' % i)
        put(b2, 'derived[%d].bias' % i)
    for role, st in ex.transform.items():
        for nm in ('fill', 'shift', 'scale'):
            put(getattr(st, nm, None), '%s.%s' % (role, nm))
    for (k, n), st in ex._bn.items():
        for nm, t in st.items():
            put(t, 'bn_state[%d].%s' % (k, nm))
    return found


# -- op tables ------------------------------------------------------------------------------------------------------------- #
def table_of(key):
    """(op table bytes, [what each tensor of the parameter table is])"""
    ex = executor(key)
    arr, params = ex.encode_ops(N)
    names = names_of(key.split('/')[0], ex)
    return bytes(arr), [names.get(t.data_ptr(), 'unknown %r' % (tuple(t.shape),)) for t in params]


def _fields(s, prefix=''):
    for nm, _ in s._fields_:
        v = getattr(s, nm)
        if isinstance(v, ctypes.Structure):
            for item in _fields(v, prefix + nm + '.'):
                yield item
        elif isinstance(v, ctypes.Array):
            for j, e in enumerate(v):
                yield '%s%s[%d]' % (prefix, nm, j), e
        else:
            yield prefix + nm, v


def first_difference(got, want):
    """'op k: field: got != want' of two op tables"""
    size = ctypes.sizeof(_lib.Op)
    if len(got) != len(want):
        return '%d ops, golden %d' % (len(got) // size, len(want) // size)
    for k in range(len(got) // size):
        a, b = (_lib.Op.from_buffer_copy(t[k * size:(k + 1) * size]) for t in (got, want))
        for (nm, va), (_, vb) in zip(_fields(a), _fields(b)):
            if va != vb:
                return 'op %d: %s: %r, golden %r' % (k, nm, va, vb)
    return None


# -- launch traces --------------------------------------------------------------------------------------------------------- #
class Recorder(object):
    """Stands in for the ops wrappers: keeps (wrapper, args, kwargs) and answers as a wrapper does, with `out`.
    refuse_pool2: conv2d(out_pool2=...) answers None, as where no kernel stores the pooled image too."""

    def __init__(self, monkeypatch, refuse_pool2=False):
        self.calls, self.refuse_pool2 = [], refuse_pool2
        for nm in WRAPPERS:
            monkeypatch.setattr(ops, nm, functools.partial(self.call, nm))

    def call(self, nm, *args, **kwargs):
        self.calls.append((nm, args, kwargs))
        if kwargs.get('out_pool2') is not None and self.refuse_pool2:
            return None
        return kwargs.get('out')


def _plain(a, names):
    if isinstance(a, torch.Tensor):
        return '%s %r' % (names.get(a.data_ptr(), 'unknown'), tuple(a.shape))
    if isinstance(a, ctypes.Structure):       # a descriptor: its bytes (every field is an int), and the mark Executor.few_wino leaves
        return {type(a).__name__ + ('+few_wino' if getattr(a, 'few_wino', False) else ''): np.frombuffer(bytes(a), dtype='<i4').tolist()}
    if isinstance(a, (list, tuple)):
        return [_plain(v, names) for v in a]
    if a is None or isinstance(a, (bool, str)):
        return a
    if isinstance(a, numbers.Integral):
        return int(a)
    if isinstance(a, numbers.Real):
        return float(a)
    raise TypeError('launch argument %r' % (a,))


#: the call forms: name -> (executor, keywords of run | a function of the executor that gives them, recorder keywords)
def _skip_d2s(ex):
    (k,) = [k for k, op in enumerate(ex.plan.ops) if op.kind == 'd2s']
    return dict(prepared={}, skip_phasew=True, skip_ops=(k,), training=True)


STEP = dict(prepared={}, skip_phasew=True, training=True)
FORMS = {'run': {}, 'step': STEP, 'step_pool_refused': STEP, 'step_skip_d2s': _skip_d2s}
LAUNCH_KEYS = ['%s/run' % key for key in EXECUTOR_KEYS] + \
    ['%s/train/step' % name for name in MODELS if name != 'scaled'] + ['unet/train/step_pool_refused', 'unet/train/step_skip_d2s']


def launches_of(key, monkeypatch):
    name, which, form = key.split('/')
    m = model(name)
    ex = m.train_executor if which == 'train' else executors(name)[which]
    kw = FORMS[form](ex) if callable(FORMS[form]) else FORMS[form]
    rec = Recorder(monkeypatch, refuse_pool2=(form == 'step_pool_refused'))
    x = torch.zeros((N,) + tuple(m.inputs[0].shape))
    outs = ex.alloc_outputs(N)
    assert ex.run(x, outs, **kw) is outs
    names = names_of(name, ex, x, outs)
    return [[nm, _plain(args, names), {k: _plain(v, names) for k, v in sorted(kwargs.items())}] for nm, args, kwargs in rec.calls]


# -- recording ------------------------------------------------------------------------------------------------------------- #
def _host_rules(monkeypatch):
    """plans and layouts as a host without a device gives them: no option set, the library's hints asked without a handle"""
    for k in [k for k in os.environ if k.startswith('DLWP_')]:
        monkeypatch.delenv(k)
    monkeypatch.setattr(_lib, 'handle_or_none', lambda device_index=None: None)


def record(tables=table_of):
    """Write both goldens from the code as it stands."""
    mp = pytest.MonkeyPatch()
    try:
        _host_rules(mp)
        got = {key: tables(key) for key in TABLE_KEYS}
        launches = {key: launches_of(key, mp) for key in LAUNCH_KEYS}
    finally:
        mp.undo()
    np.savez_compressed(OPS_NPZ, **{key: np.frombuffer(b, dtype=np.uint8) for key, (b, _) in got.items()})
    text = json.dumps({'params': {key: names for key, (_, names) in got.items()}, 'launches': launches}, sort_keys=True,
                      separators=(',', ':'))
    with open(LAUNCHES_JSON, 'w') as fh:          # one launch, one table per line
        fh.write(text.replace('}],["', '}],\n["').replace(']],"', ']],\n"').replace('],"', '],\n"') + '\n')


@functools.lru_cache(maxsize=None)
def goldens():
    with open(LAUNCHES_JSON) as fh:
        doc = json.load(fh)
    with np.load(OPS_NPZ) as z:
        doc['ops'] = {key: z[key].tobytes() for key in z.files}
    return doc


# -- the tests ------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(autouse=True)
def host_rules(monkeypatch):
    _host_rules(monkeypatch)


def test_every_op_kind_has_a_fixture():
    assert sorted('%s/%s' % (name, which) for name in MODELS for which in executors(name)) == sorted(EXECUTOR_KEYS)
    kinds = {op.kind for key in EXECUTOR_KEYS for op in executor(key).plan.ops}
    assert kinds == set(F.LAUNCHES)
    assert set(F.LAUNCHES) - set(F.ROLLOUT_OPS) == {'dropout'} and set(F.ROLLOUT_OPS) <= set(F.LAUNCHES)
    assert sorted(goldens()['ops']) == sorted(goldens()['params']) == sorted(TABLE_KEYS)
    assert sorted(goldens()['launches']) == sorted(LAUNCH_KEYS)
    for key, trace in goldens()['launches'].items():          # the recorders stand in for every wrapper run() can reach
        assert {call[0] for call in trace} <= set(WRAPPERS), key


@pytest.mark.parametrize('key', TABLE_KEYS)
def test_op_table_matches_the_golden(key):
    got, params = table_of(key)
    assert len(got) == ctypes.sizeof(_lib.Op) * len(executor(key).plan.ops) and ctypes.sizeof(_lib.Op) == 256
    assert first_difference(got, goldens()['ops'][key]) is None
    assert got == goldens()['ops'][key]
    assert params == goldens()['params'][key]            # its length, its order, and which optional tensors are missing


def test_a_chain_encodes_against_its_own_buffers():
    ex = executor('unet/infer')
    bufs = [torch.empty_like(b) for b in ex.scratch(N)]
    arr, params = ex.encode_ops(N, bufs)
    assert bytes(arr) == goldens()['ops']['unet/infer']
    assert all(a is b for a, b in zip(params, bufs)) and params[len(bufs):] == ex.encode_ops(N)[1][len(bufs):]


def test_dropout_has_no_rollout_form():
    with pytest.raises(RuntimeError, match='dropout'):
        model('dense').train_executor.encode_ops(N)


def test_an_unknown_kind_is_an_error(monkeypatch):
    m = model('bilinear')
    from dlwp_amd.engine import Executor
    ex = Executor(m.infer_plan, CPU)
    monkeypatch.setattr(ex.plan.ops[0], 'kind', 'nonesuch')
    with pytest.raises(RuntimeError, match='^nonesuch$'):
        ex.run(torch.zeros(N, 4, 16, 24))
    with pytest.raises(RuntimeError, match='nonesuch'):
        ex.encode_ops(N)


@pytest.mark.parametrize('key', LAUNCH_KEYS)
def test_launches_match_the_golden(key, monkeypatch):
    got, want = launches_of(key, monkeypatch), goldens()['launches'][key]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, 'launch %d of %s' % (k, key)
    assert len(got) == len(want)


def test_a_pooled_output_skips_the_pooling_op_unless_the_convolution_refuses(monkeypatch):
    ex = model('unet').train_executor
    pooled = ex._pooled_too()
    assert pooled and all(ex.plan.ops[k].kind == 'conv' and ex.plan.ops[j].kind == 'maxpool' for k, j in pooled.items())
    taken = [c[0] for c in launches_of('unet/train/step', monkeypatch)]
    refused = [c[0] for c in launches_of('unet/train/step_pool_refused', monkeypatch)]
    assert taken.count('maxpool2') == 0 and refused.count('maxpool2') == len(pooled)
    assert refused.count('conv2d') == taken.count('conv2d') + len(pooled)      # the attempt, then the plain convolution
    assert 'maxpool2' in [c[0] for c in launches_of('unet/train/run', monkeypatch)]       # a plain run() never asks


def test_skipped_ops_and_up_to_date_derived_kernels_are_not_launched(monkeypatch):
    run = [c[0] for c in launches_of('unet/train/run', monkeypatch)]
    step = [c[0] for c in launches_of('unet/train/step_skip_d2s', monkeypatch)]
    assert run.count('phase_weights') > 0 and step.count('phase_weights') == 0
    assert run.count('depth_to_space2') == 1 and step.count('depth_to_space2') == 0
