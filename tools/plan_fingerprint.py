#!/usr/bin/env python
"""Print a full fingerprint of plan.build_plan over a fixed corpus of small models (host data only: no GPU work, no compile()).

  python tools/plan_fingerprint.py > new.txt
  git show HEAD~1:dlwp_amd/plan.py > old_plan.py && python tools/plan_fingerprint.py --plan-module old_plan.py > old.txt
  cmp old.txt new.txt

A refactor of the planner leaves the two outputs byte-identical.  The planner asks the library which epilogues a kernel can
fold, so compare in each environment of interest: --no-library (every answer is no), with the built library on a host without
a device (host rules) and on the GPU.  The corpus reaches every row of plan._LOWERINGS, every op kind of PlanOp's docstring and
every `raise` of the planner (the refusals: exception type and message)."""
import argparse
import importlib.util
import itertools
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENVS = ({}, {'DLWP_TCONV_TAPS': 'exact'}, {'DLWP_LSTM_STEP': '0'})
FLAGS = ('inference', 'fuse_d2s', 'fuse_lstm', 'fuse_lstm_step')
LISTS = ('conv_layers', 'bn_layers', 'dense_layers', 'dropout_layers', 'eltwise_layers', 'sep_layers')


def load_plan_module(path):
    """another copy of plan.py as a submodule of dlwp_amd, so that its relative imports work"""
    spec = importlib.util.spec_from_file_location('dlwp_amd._plan_under_test', path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def labels_of(P, outputs):
    """layer -> 'Type#index of its first tensor in the toposort' (auto-generated names depend on the process's history)"""
    index = {}
    for k, t in enumerate(P.toposort(outputs)):
        index.setdefault(id(t.layer), '%s#%d' % (type(t.layer).__name__, k))

    def label(lay):
        if hasattr(lay, 'parent'):                  # the two convolutions of a ConvLSTM2D / a SeparableConv2D
            return '%s/%s' % (label(lay.parent), lay.which)
        return index[id(lay)]
    return label


def norm(x, label):
    if isinstance(x, dict):
        return tuple((k, norm(v, label)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(norm(v, label) for v in x)
    return label(x) if hasattr(x, 'name') and hasattr(x, 'trainable') or hasattr(x, 'parent') else x


def fingerprint(P, plan, outputs, out):
    label = labels_of(P, outputs)
    for k, op in enumerate(plan.ops):
        attrs = dict(vars(op), conv_out_shape=getattr(op, 'conv_out_shape', None))
        out('  op %d %s' % (k, ' '.join('%s=%r' % (a, norm(v, label)) for a, v in sorted(attrs.items()))))
    for name in ('buffers', '_in_store', 'input_shape', 'output_shapes', 'output_store') + LISTS + ('phase_params',):
        out('  %s %r' % (name, norm(getattr(plan, name), label)))
    out('  bf16 %r flops %r launches %r' % (plan.bf16_buffers(), plan.conv_flops_per_sample(), plan.n_launches))


def build_layers(P, L, outputs, lenient=False):
    """what Model._init_graph does in front of build_plan: weights on the host (RowConnected2D and Dense are planned by them)"""
    import numpy as np
    import torch
    rng = np.random.RandomState(0)
    for t in P.toposort(outputs):
        if not isinstance(t.layer, L.InputLayer) and not t.layer.built:
            try:
                t.layer.build(t.inputs[0].shape, torch.device('cpu'), rng)
            except Exception:
                if not lenient:                     # (a refusal model may hand a layer a shape it cannot be built for)
                    raise


CF = {'data_format': 'channels_first'}


def models(L):
    """(name, (input, [outputs])): 4 channels on 16 x 24 unless a case needs otherwise"""
    from dlwp_amd import custom as C, presets

    def X(*shape):
        return L.Input(shape=shape or (4, 16, 24))

    def conv(t, f=8, k=3, **kw):
        return L.Conv2D(f, k, **dict(CF, **dict({'padding': 'same'}, **kw)))(t)

    def up(t, **kw):
        return L.UpSampling2D(2, **dict(CF, **kw))(t)

    def pool(t):
        return L.MaxPooling2D(2, **CF)(t)

    def wrap_zero(t, k):
        return L.ZeroPadding2D((k, 0), **CF)(C.PeriodicPadding2D((0, k), **CF)(t))

    def stack(specs):
        t = x = None
        for name, a, kw in specs:
            kw = dict(kw or {})
            if x is None:
                t = x = L.Input(shape=kw.pop('input_shape'))
            t = (getattr(L, name, None) or getattr(C, name))(*(a or ()), **kw)(t)
        return x, [t]
    w = (8, 16, 16, 16, 8)
    yield 'unet', stack(presets.unet_layers((4, 16, 24), widths=w))
    yield 'unet_rows', stack(presets.unet_layers((4, 16, 24), widths=w, latitude_dependent=True))
    yield 'cnn2', stack(presets.cnn2_layers((4, 16, 24), hidden=8))
    yield 'lstm_unet', stack(presets.lstm_unet_layers((2, 4, 16, 24), lstm_mult=2, widths=w))
    x = X(16, 24, 4)
    yield 'pad_nhwc', (x, [L.ZeroPadding2D((1, 2), data_format='channels_last')(x)])
    for name, zero in (('pad3d_composes', (0, 1, 0)), ('pad3d_materialises', (0, 1, 1))):
        x = X(2, 4, 16, 24)
        t = L.ZeroPadding3D(zero, **CF)(C.PeriodicPadding3D((0, 0, 2), **CF)(x))
        yield name, (x, [L.ConvLSTM2D(4, 3, **CF)(t)])
    x = X()
    yield 'wrap_then_same', (x, [conv(C.PeriodicPadding2D((0, 2), **CF)(x))])
    x = X()
    yield 'bilinear', (x, [conv(up(L.ChannelSlice(1, 7)(conv(x)), interpolation='bilinear'))])
    x = X()
    yield 'bilinear_out', (x, [up(wrap_zero(x, 1), interpolation='bilinear')])
    x = X()
    yield 'nearest_out', (x, [up(conv(x))])
    x = X()
    yield 'pool_folds', (x, [conv(pool(conv(x)))])
    x = X()
    c = conv(x)
    yield 'pool_two_consumers', (x, [L.Add()([conv(pool(c)), pool(conv(c))])])
    x = X()
    c = conv(x)
    yield 'pool_of_an_output', (x, [c, conv(pool(c))])
    x = X(1, 4, 16, 24)
    yield 'pool_of_a_cell', (x, [conv(pool(L.ConvLSTM2D(8, 3, padding='same', **CF)(x)))])
    x = X()
    yield 'avgpool', (x, [L.AveragePooling2D(2, **CF)(L.AveragePooling2D(2, **CF)(L.ChannelSlice(1, 3)(up(x))))])
    x = X()
    yield 'slice_concat_out', (x, [L.Concatenate(axis=1)([L.ChannelSlice(0, 2)(x), conv(x), pool(up(x))])])
    x = X()
    yield 'slice_concat_scratch', (x, [conv(L.Concatenate(axis=1)([L.ChannelSlice(1, 3)(conv(x)), wrap_zero(x, 0)]))])
    x = X()
    yield 'reshape_scratch', (x, [conv(L.Reshape((8, 16, 24))(L.Reshape((2, 4, 16, 24))(conv(x))))])
    x = X()
    yield 'reshape_input', (x, [conv(L.Reshape((4, 16, 24))(L.Reshape((2, 2, 16, 24))(x)))])
    x = X()
    yield 'up_dil2_even', (x, [conv(conv(up(x), dilation_rate=2))])
    x = X()
    yield 'up_dil2_odd', (x, [conv(L.ZeroPadding2D(1, **CF)(up(x)), dilation_rate=2, padding='valid')])
    for k in (3, 5):
        x = X()
        yield 'up_k%d_out' % k, (x, [conv(up(conv(x)), k=k, activation='tanh')])
        x = X()
        yield 'up_k%d_inner' % k, (x, [conv(conv(up(L.ChannelSlice(1, 4)(x)), k=k, use_bias=False))])
    for inner in (False, True):             # (3 taps restate behind a top / left halo of 2 only: 2 source pixels per axis)
        x = X()
        t = conv(L.ZeroPadding2D(((2, 0), (2, 0)), **CF)(up(conv(x))), padding='valid', activation='tanh')
        yield 'up_k3_halo2_%s' % ('inner' if inner else 'out'), (x, [conv(t) if inner else t])
    x = X()
    yield 'up_reflect', (x, [conv(C.TFPadding2D(1, mode='REFLECT', **CF)(up(x)), padding='valid')])
    for pad in ('same', 'valid'):
        x = X()
        yield 'sconv_%s_input' % pad, (x, [conv(x, strides=2, padding=pad)])
        x = X()
        yield 'sconv_%s_padded' % pad, (x, [conv(conv(wrap_zero(x, 2), k=5, strides=2, padding=pad, activation='tanh'))])
        x = X()
        yield 'sconv_%s_pooled' % pad, (x, [pool(conv(pool(conv(x)), k=4, strides=2, padding=pad))])
    x = X()
    yield 'depthwise', (x, [L.DepthwiseConv2D(3, depth_multiplier=2, padding='same', activation='relu', **CF)(wrap_zero(pool(x), 1))])
    x = X()
    yield 'separable', (x, [conv(L.SeparableConv2D(8, 3, activation='tanh', **CF)(x))])
    x = X()
    yield 'separable_out', (x, [L.SeparableConv2D(8, 3, padding='same', **CF)(wrap_zero(x, 1))])
    for k, pad, inner in itertools.product((2, 3, 4, 5), ('same', 'valid'), (False, True)):
        x = X()
        t = L.Conv2DTranspose(6, k, strides=2, padding=pad, activation='tanh', **CF)(wrap_zero(x, 1) if k == 3 else x)
        yield 'tconv_k%d_%s_%s' % (k, pad, 'inner' if inner else 'out'), (x, [conv(t) if inner else t])
    x = X()
    yield 'crop_of_tconv_out', (x, [L.Cropping2D(((1, 0), (2, 1)), **CF)(L.Conv2DTranspose(6, 3, strides=2, **CF)(pool(x)))])
    x = X()
    yield 'crop_of_tconv_inner', (x, [conv(L.Cropping2D(1, **CF)(L.Conv2DTranspose(6, 4, strides=2, **CF)(x)))])
    x = X()
    t = L.Conv2DTranspose(6, 3, strides=2, **CF)(x)
    yield 'crop_two_readers', (x, [L.Cropping2D(1, **CF)(t), conv(L.Cropping2D(((0, 2), (0, 2)), **CF)(t))])
    x = X()
    yield 'crop_plain', (x, [L.Cropping2D(((1, 2), (0, 3)), **CF)(L.ChannelSlice(1, 3)(x))])
    x = X()
    yield 'rowconv_up', (x, [L.RowConnected2D(4, 3, **CF)(wrap_zero(up(pool(pool(x))), 1))])
    x = X()
    yield 'batchnorm', (x, [L.BatchNormalization(axis=1)(L.BatchNormalization(axis=1)(pool(conv(x))))])
    x = X()
    t = L.Dropout(0.25)(L.Dense(32, activation='tanh')(L.Flatten()(pool(conv(x)))))
    yield 'dense', (x, [L.Reshape((4, 16, 24))(L.Dense(4 * 16 * 24)(t))])
    x = X()
    yield 'dropout_out', (x, [L.Dropout(0.5)(L.ChannelSlice(0, 2)(conv(x)))])
    x = X()
    yield 'activations', (x, [L.LeakyReLU(0.1)(L.Activation('linear')(L.Activation('relu')(up(conv(x)))))])
    x = X()
    c = conv(x)
    yield 'merges', (x, [conv(L.Average()([c, conv(c), L.ChannelSlice(0, 8)(conv(c, f=12)), pool(up(c))])), L.Subtract()([c, conv(x)])])
    x = X()
    c = conv(x)
    yield 'same_tensor_twice', (x, [c, c])
    x = X()
    yield 'redirect_alone', (x, [L.Reshape((2, 4, 16, 24))(conv(x))])
    x = X()
    c = conv(x)
    yield 'redirect_with_a_reader', (x, [L.Reshape((2, 4, 16, 24))(c), conv(c)])
    x = X()
    yield 'redirect_of_d2s', (x, [L.Reshape((2, 4, 32, 48))(conv(up(x)))])
    for seq in (True, False):
        x = X(2, 4, 16, 24)
        t = L.ConvLSTM2D(8, 3, padding='same', return_sequences=seq, recurrent_activation='sigmoid', **CF)(x)
        yield 'convlstm_seq%d' % seq, (x, [conv(L.Reshape((16, 16, 24))(t)) if seq else conv(t)])


def refusals(L):
    """(name, builder -> ([inputs], [outputs], build_plan keywords)): one model per `raise` of the planner.  node() applies a layer
    to a tensor WITHOUT the layer's own shape check, where that check would refuse the model first."""
    from dlwp_amd import custom as C

    def X(*shape):
        return L.Input(shape=shape or (4, 16, 24))

    def node(lay, t, shape=None):
        ins = t if isinstance(t, list) else [t]
        return L.KTensor(shape or ins[0].shape, lay, ins)

    def one(make, shape=(), **kw):
        def build():
            x = X(*shape)
            outs = make(x)
            return [x], outs if isinstance(outs, list) else [outs], kw
        return build

    def four_d(x):
        return L.Reshape((2, 2, 16, 24))(x)

    def twice(lay):
        return lambda x: lay(L.Conv2D(4, 3, padding='same', **CF)(lay(x)))

    class Odd(L.Layer):
        pass
    yield 'two_inputs', lambda: ([X(), X()], [X()], {})
    yield 'transform_in_training', one(lambda x: x, transform=(True, False))
    yield 'tail_two_outputs', one(lambda x: [L.Flatten()(x), L.Flatten()(x)], inference=True, transform=(False, True))
    yield 'rank2_input', one(lambda x: L.Flatten()(x), shape=(4, 16))
    yield 'rank2_reshape', one(lambda x: L.Reshape((64, 24))(x))
    yield 'foreign_input', one(lambda x: L.Add(name='r')([x, X()]))
    yield 'output_is_input', one(lambda x: x)
    yield 'pad2d_reshaped', one(lambda x: node(L.ZeroPadding2D(1, name='r', **CF), four_d(x)))
    yield 'pad2d_wrap_rows', one(lambda x: node(C.PeriodicPadding2D((17, 0), name='r', **CF), x, (4, 50, 24)))
    yield 'pad2d_wrap_cols', one(lambda x: node(C.PeriodicPadding2D((0, 25), name='r', **CF), x, (4, 16, 74)))
    yield 'pad3d_channels_last', one(lambda x: node(L.ZeroPadding3D(1, name='r', data_format='channels_last'), x), shape=(2, 4, 16, 24))
    yield 'pad3d_first_axis', one(lambda x: L.ZeroPadding3D((1, 0, 0), name='r', **CF)(x), shape=(2, 4, 16, 24))
    yield 'pad3d_wrap_rows', one(lambda x: node(C.PeriodicPadding3D((0, 17, 0), name='r', **CF), x), shape=(2, 4, 16, 24))
    yield 'pad3d_wrap_cols', one(lambda x: node(C.PeriodicPadding3D((0, 0, 25), name='r', **CF), x), shape=(2, 4, 16, 24))
    yield 'convlstm_channels', one(lambda x: node(L.ConvLSTM2D(4, 3, name='r', **CF), L.ChannelSlice(0, 4)(x), (2, 4, 16, 24)),
                                   shape=(8, 16, 24))
    for name, lay in (('bilinear', L.UpSampling2D(2, interpolation='bilinear', name='r', **CF)),
                      ('maxpool', L.MaxPooling2D(2, name='r', **CF)),
                      ('avgpool', L.AveragePooling2D(2, name='r', **CF)), ('slice', L.ChannelSlice(0, 1)),
                      ('sconv', L.Conv2D(4, 3, strides=2, name='r', **CF)), ('depthwise', L.DepthwiseConv2D(3, name='r', **CF)),
                      ('conv', L.Conv2D(4, 3, name='r', **CF)), ('tconv', L.Conv2DTranspose(4, 3, name='r', **CF)),
                      ('crop', L.Cropping2D(1, name='r', **CF)), ('rowconv', L.RowConnected2D(4, 3, name='r', **CF)),
                      ('batchnorm', L.BatchNormalization(axis=1, name='r'))):
        yield name + '_reshaped', one(lambda x, lay=lay: node(lay, four_d(x)))
    yield 'reshape_size', one(lambda x: node(L.Reshape((4, 16, 25)), x, (4, 16, 25)))
    yield 'sconv_twice', one(twice(L.Conv2D(4, 3, strides=2, padding='same', name='r', **CF)))
    yield 'separable_twice', one(twice(L.SeparableConv2D(4, 3, padding='same', name='r', **CF)))
    yield 'depthwise_does_not_fit', one(lambda x: node(L.DepthwiseConv2D(3, dilation_rate=4, name='r', **CF), x), shape=(4, 8, 24))
    yield 'tconv_twice', one(twice(L.Conv2DTranspose(4, 3, padding='same', name='r', **CF)))
    yield 'crop_leaves_nothing', one(lambda x: node(L.Cropping2D(8, name='r', **CF), x))
    row = L.RowConnected2D(4, 3, name='r', **CF)
    yield 'rowconv_kernel', one(lambda x: row(row(x)))
    yield 'batchnorm_twice', one(twice(L.BatchNormalization(axis=1, name='r')))
    dense = L.Dense(8, name='r')
    yield 'dense_twice', one(lambda x: dense(dense(L.Flatten()(L.ChannelSlice(0, 1)(L.Cropping2D(((0, 14), (0, 20)), **CF)(x))))))
    yield 'dense_kernel', one(lambda x: L.Dense(8, name='r')(node(L.Flatten(), x, (10,))))
    drop = L.Dropout(0.5, name='r')
    yield 'dropout_twice', one(lambda x: drop(drop(x)))
    yield 'merge_sizes', one(lambda x: node(L.Add(name='r'), [x, L.ChannelSlice(0, 2)(x)]))
    yield 'no_lowering', one(lambda x: Odd(name='r')(x))


def main():
    ap =argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--plan-module', help='take build_plan from this copy of plan.py')
    ap.add_argument('--no-library', action='store_true', help='plan as a host without the built library does')
    args = ap.parse_args()
    if args.no_library:
        sys.modules['dlwp_amd.ops'] = None          # `from . import ops` in the planner raises ImportError: every fold is refused
    from dlwp_amd import layers as L
    P = load_plan_module(args.plan_module) if args.plan_module else importlib.import_module('dlwp_amd.plan')
    rows = set()
    if hasattr(P, '_LOWERINGS'):                    # count the rows taken
        def counted(k, fn):
            return lambda *a: (rows.add(k), fn(*a))[1]
        P._LOWERINGS = tuple((m, counted(k, fn)) for k, (m, fn) in enumerate(P._LOWERINGS))
    out = sys.stdout.write
    kinds, n_plans = set(), 0
    corpus = [(name, x, outs) for name, (x, outs) in models(L)]
    for _, _, outs in corpus:
        build_layers(P, L, outs)
    refused = list(refusals(L))
    for env in ENVS:
        for k in ('DLWP_TCONV_TAPS', 'DLWP_LSTM_STEP'):
            os.environ.pop(k, None)
        os.environ.update(env)
        for name, x, outs in corpus:
            for flags in itertools.product((False, True), repeat=4):
                kw = dict(zip(FLAGS, flags))
                transforms = [None] + ([(True, False), (False, True), (True, True)] if kw['inference'] and len(outs) == 1 else [])
                for tr in transforms:
                    out('== %s env=%r %s transform=%r\n' % (name, sorted(env.items()), ' '.join('%s=%d' % i for i in kw.items()), tr))
                    plan = P.build_plan([x], outs, transform=tr, **kw)
                    fingerprint(P, plan, outs, lambda s: out(s + '\n'))
                    kinds.update(op.kind for op in plan.ops)
                    n_plans += 1
        for name, fn in refused:
            ins, outs, kw = fn()
            build_layers(P, L, outs, lenient=True)
            try:
                P.build_plan(ins, outs, **kw)
                raise SystemExit('refusal model %s was planned' % name)
            except (NotImplementedError, ValueError, RuntimeError) as e:
                out('== refusal %s env=%r: %s: %s\n' % (name, sorted(env.items()), type(e).__name__, e))
    want = set(re.findall(r"'(\w+)'", P.PlanOp.__doc__))
    assert len(want) == 24 and kinds == want, 'op kinds: missing %r, unknown %r' % (sorted(want - kinds), sorted(kinds - want))
    if hasattr(P, '_LOWERINGS'):
        assert rows == set(range(len(P._LOWERINGS))), 'rows of _LOWERINGS never taken: %r' % sorted(set(range(len(P._LOWERINGS))) - rows)
    sys.stderr.write('%d plans, %d refusals x %d environments, %d op kinds\n' % (n_plans, len(refused), len(ENVS), len(kinds)))


if __name__ == '__main__':
    main()
