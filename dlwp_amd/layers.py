"""
Layer objects with the Keras names and constructor signatures the reference resolves through its registry
(`util.get_from_class('keras.layers', name)`, DLWP/model/models.py:97-103).  They are *descriptions*: a layer records
its hyper-parameters and output shape and owns its weights (device tensors in Keras layout); it never computes.  The
graph of layers is lowered by dlwp_amd.plan into fused libdlwp_hip.so launches.

Shapes are per-sample tuples without the batch axis, as in Keras `input_shape=`.
"""
import itertools
import math

import numpy as np

_uid = itertools.count(1)
_name_counts = {}


def _auto_name(cls_name):
    # keras-style snake_case + running index: Conv2D -> conv2d_1, PeriodicPadding2D -> periodic_padding2d_1
    out = []
    for i, ch in enumerate(cls_name):
        if ch.isupper() and i and (cls_name[i - 1].islower() or (i + 1 < len(cls_name) and cls_name[i + 1].islower())):
            out.append('_')
        out.append(ch.lower())
    base = ''.join(out).replace('2_d', '2d').replace('3_d', '3d')
    _name_counts[base] = _name_counts.get(base, 0) + 1
    return '%s_%d' % (base, _name_counts[base])


def normalize_data_format(value):
    """Keras: None -> the image_data_format default, which is 'channels_last'."""
    if value is None:
        return 'channels_last'
    if value not in ('channels_first', 'channels_last'):
        raise ValueError("data_format must be 'channels_first' or 'channels_last', got %r" % (value,))
    return value


def normalize_padding(padding, rank):
    """int | tuple of ints | tuple of pairs  ->  ((lo, hi),) * rank   (keras ZeroPadding2D/3D argument forms)."""
    if isinstance(padding, (int, np.integer)):
        return tuple((int(padding), int(padding)) for _ in range(rank))
    if not hasattr(padding, '__len__') or len(padding) != rank:
        raise ValueError('`padding` should have %d elements. Found: %r' % (rank, padding))
    out = []
    for p in padding:
        if isinstance(p, (int, np.integer)):
            out.append((int(p), int(p)))
        else:
            p = tuple(int(v) for v in p)
            if len(p) != 2:
                raise ValueError('each `padding` entry must be an int or a tuple of 2 ints. Found: %r' % (p,))
            out.append(p)
    for lo, hi in out:
        if lo < 0 or hi < 0:
            raise ValueError('negative padding is not supported: %r' % (padding,))
    return tuple(out)


class KTensor(object):
    """Symbolic tensor: per-sample shape + the node (layer application) that produced it."""

    def __init__(self, shape, layer=None, inputs=(), index=0):
        self.shape = tuple(int(s) for s in shape)
        self.layer = layer
        self.inputs = tuple(inputs)
        self.index = index
        self.uid = next(_uid)

    @property
    def _keras_shape(self):
        return (None,) + self.shape

    def __repr__(self):
        return '<KTensor %s from %s>' % ((None,) + self.shape, self.layer.name if self.layer else 'input')


class Layer(object):
    """Base class; also the extension point DLWP.custom-style layers subclass."""

    def __init__(self, input_shape=None, name=None, trainable=True, **kwargs):
        kwargs.pop('batch_input_shape', None)
        kwargs.pop('dtype', None)
        if kwargs:
            raise TypeError('unexpected keyword arguments for %s: %r' % (type(self).__name__, sorted(kwargs)))
        self.name = name or _auto_name(type(self).__name__)
        self.trainable = trainable
        self.batch_input_shape = (None,) + tuple(input_shape) if input_shape is not None else None
        self.input_shape = None
        self.output_shape = None
        self.built = False
        self._weights = []          # list of (name, device tensor) -- filled by build()
        self._calls = 0

    # -- protocol ------------------------------------------------------------------------------------------------ #
    def compute_output_shape(self, input_shape):
        """per-sample input shape(s) -> per-sample output shape"""
        return tuple(input_shape)

    def build(self, input_shape, device, rng):
        self.built = True

    def __call__(self, inputs):
        multi = isinstance(inputs, (list, tuple))
        ins = list(inputs) if multi else [inputs]
        for t in ins:
            if not isinstance(t, KTensor):
                raise TypeError('%s must be called on symbolic tensors (Input(...) or the output of another layer); '
                                'got %r' % (self.name, type(t)))
        in_shape = [t.shape for t in ins] if multi else ins[0].shape
        out_shape = self.compute_output_shape(in_shape)
        if self._calls == 0:
            self.input_shape = [(None,) + tuple(s) for s in in_shape] if multi else (None,) + tuple(in_shape)
            self.output_shape = (None,) + tuple(out_shape)
        self._calls += 1
        return KTensor(out_shape, self, ins, self._calls - 1)

    # -- weights --------------------------------------------------------------------------------------------------- #
    @property
    def weights(self):
        return [w for _, w in self._weights]

    def get_weights(self):
        return [w.detach().cpu().numpy() for _, w in self._weights]

    def set_weights(self, arrays):
        import torch
        if len(arrays) != len(self._weights):
            raise ValueError('layer %s expects %d weight arrays, got %d' % (self.name, len(self._weights), len(arrays)))
        for (nm, w), a in zip(self._weights, arrays):
            a = np.asarray(a, dtype=np.float32)
            if tuple(a.shape) != tuple(w.shape):
                raise ValueError('layer %s weight %s: shape %s != %s' % (self.name, nm, a.shape, tuple(w.shape)))
            w.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def count_params(self):
        return int(sum(int(np.prod(w.shape)) for _, w in self._weights))

    def get_config(self):
        return {'name': self.name, 'trainable': self.trainable}


class InputLayer(Layer):
    def __init__(self, input_shape=None, name=None, **kwargs):
        super(InputLayer, self).__init__(input_shape=input_shape, name=name, **kwargs)
        self.output_shape = self.batch_input_shape
        self.input_shape = self.batch_input_shape


def Input(shape=None, name=None, **kwargs):
    """keras.layers.Input: a symbolic placeholder with per-sample `shape` (examples/train_functional.py:154)."""
    if shape is None:
        raise ValueError('Input() needs shape=')
    layer = InputLayer(input_shape=tuple(shape), name=name or _auto_name('Input'))
    return KTensor(tuple(shape), layer, ())


class _Pad2DBase(Layer):
    """Shared argument handling of ZeroPadding2D / PeriodicPadding2D / FillPadding2D (they differ only in mode)."""
    mode = 0  # _lib.PAD_ZERO

    def __init__(self, padding=(1, 1), data_format=None, **kwargs):
        super(_Pad2DBase, self).__init__(**kwargs)
        self.padding = normalize_padding(padding, 2)
        self.data_format = normalize_data_format(data_format)

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise ValueError('%s expects 4D input (batch + 3), got per-sample shape %r' % (self.name, s))
        (t, b), (l, r) = self.padding
        if self.data_format == 'channels_first':
            return (s[0], s[1] + t + b, s[2] + l + r)
        return (s[0] + t + b, s[1] + l + r, s[2])

    def get_config(self):
        cfg = super(_Pad2DBase, self).get_config()
        cfg.update({'padding': self.padding, 'data_format': self.data_format})
        return cfg


class ZeroPadding2D(_Pad2DBase):
    """keras.layers.ZeroPadding2D -- the pole-row halo of every reference stack (examples/train.py:163 ...)."""
    mode = 0


class Conv2D(Layer):
    """keras.layers.Conv2D: strides 1 or 2, 'valid' | 'same', dilation (stride 1 only), bias, activation in
    {None,'linear','tanh','relu'}, data_format='channels_first' (what every reference call site passes: examples/train.py:164-219).
    Weights: kernel (kh, kw, cin, cout) glorot_uniform, bias (cout,) zeros -- Keras layout and initialisers.
    strides=2 (the learned down-sampling of an encoder; examples/train_generator.py:113-141 of the reference carries one) runs as a
    padded space-to-depth pass + one stride-1 convolution on 4 x cin phase channels (csrc/sconv.hip)."""

    def __init__(self, filters, kernel_size, strides=(1, 1), padding='valid', data_format=None, dilation_rate=(1, 1),
                 activation=None, use_bias=True, kernel_initializer='glorot_uniform', bias_initializer='zeros',
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, **kwargs):
        super(Conv2D, self).__init__(**kwargs)
        self.filters = int(filters)
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, (int, np.integer)) else tuple(kernel_size)
        st = (strides, strides) if isinstance(strides, (int, np.integer)) else tuple(strides)
        dl = (dilation_rate, dilation_rate) if isinstance(dilation_rate, (int, np.integer)) else tuple(dilation_rate)
        if len(ks) != 2 or len(st) != 2 or len(dl) != 2:
            raise ValueError('kernel_size / strides / dilation_rate must be an int or a pair')
        try:
            st = tuple(int(v) if int(v) == v else v for v in st)
        except (TypeError, ValueError):
            raise ValueError('Conv2D: strides %r' % (strides,))
        if st not in ((1, 1), (2, 2)):
            raise NotImplementedError('Conv2D: strides=1 and strides=2 are implemented (equal on both axes), got %r' % (st,))
        if st == (2, 2) and any(int(d) != 1 for d in dl):
            raise ValueError('Conv2D: strides > 1 is not supported together with dilation_rate > 1 (got strides %r, '
                             'dilation_rate %r)' % (st, tuple(dl)))
        if padding not in ('valid', 'same'):
            raise ValueError("Conv2D padding must be 'valid' or 'same'")
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation not in (None, 'linear', 'tanh', 'relu'):
            raise NotImplementedError('Conv2D activation %r is not implemented (linear, tanh, relu are)' % (activation,))
        if kernel_initializer not in ('glorot_uniform', 'zeros') or bias_initializer not in ('zeros',):
            raise NotImplementedError('initialisers: kernel glorot_uniform|zeros, bias zeros')
        self.kernel_size = tuple(int(k) for k in ks)
        self.strides = st
        self.padding = padding
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("Conv2D: data_format='channels_first' is required (pass it explicitly, as the "
                                      "reference scripts do; Keras' default is channels_last)")
        self.dilation_rate = tuple(int(d) for d in dl)
        self.activation = activation or 'linear'
        self.use_bias = bool(use_bias)
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer   # l2 handled by the trainer when it is a dlwp_amd.regularizers.L2
        self.kernel = None
        self.bias = None

    def same_halo(self):
        """Keras 'same' for stride 1: total pad = dil*(k-1), smaller half first."""
        tot_h = self.dilation_rate[0] * (self.kernel_size[0] - 1)
        tot_w = self.dilation_rate[1] * (self.kernel_size[1] - 1)
        return (tot_h // 2, tot_h - tot_h // 2, tot_w // 2, tot_w - tot_w // 2)

    def strided_geometry(self, h, w):
        """strides=2, per axis (T, pad_lo, pad_hi, out): T = ceil(k / 2) taps on the space-to-depth image, TensorFlow's padding
        ('same': out = ceil(len / 2), total max((out - 1) 2 + k - len, 0), smaller half first; 'valid': none,
        out = (len - k) // 2 + 1) -- the rule of dlwp_sconv_geometry (include/dlwp_hip.h), restated on the host."""
        geo = []
        for k, n in zip(self.kernel_size, (int(h), int(w))):
            if self.padding == 'same':
                out = (n + 1) // 2
                tot = max((out - 1) * 2 + k - n, 0)
                lo, hi = tot // 2, tot - tot // 2
            else:
                if n < k:
                    raise ValueError('%s: kernel %r does not fit the input %r' % (self.name, self.kernel_size, (h, w)))
                out, lo, hi = (n - k) // 2 + 1, 0, 0
            geo.append(((k + 1) // 2, lo, hi, out))
        return tuple(geo)

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise ValueError('%s expects 4D input, got per-sample shape %r' % (self.name, s))
        c, h, w = s
        if self.strides == (2, 2):
            (_, _, _, ho), (_, _, _, wo) = self.strided_geometry(h, w)
            return (self.filters, ho, wo)
        if self.padding == 'same':
            return (self.filters, h, w)
        ho = h - self.dilation_rate[0] * (self.kernel_size[0] - 1)
        wo = w - self.dilation_rate[1] * (self.kernel_size[1] - 1)
        if ho <= 0 or wo <= 0:
            raise ValueError('%s: kernel %r with dilation %r does not fit the input %r' %
                             (self.name, self.kernel_size, self.dilation_rate, s))
        return (self.filters, ho, wo)

    def build(self, input_shape, device, rng):
        import torch
        if self.built:
            if self.kernel.shape[2] != input_shape[0]:
                raise ValueError('%s was built for %d input channels, now called with %d' %
                                 (self.name, self.kernel.shape[2], input_shape[0]))
            return
        kh, kw = self.kernel_size
        cin = int(input_shape[0])
        if self.kernel_initializer == 'glorot_uniform':
            limit = math.sqrt(6.0 / (kh * kw * cin + kh * kw * self.filters))
            k = rng.uniform(-limit, limit, size=(kh, kw, cin, self.filters)).astype(np.float32)
        else:
            k = np.zeros((kh, kw, cin, self.filters), dtype=np.float32)
        self.kernel = torch.from_numpy(k).to(device)
        self._weights = [('kernel', self.kernel)]
        if self.use_bias:
            self.bias = torch.zeros(self.filters, dtype=torch.float32, device=device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(Conv2D, self).get_config()
        cfg.update({'filters': self.filters, 'kernel_size': self.kernel_size, 'strides': self.strides, 'padding': self.padding,
                    'data_format': self.data_format, 'dilation_rate': self.dilation_rate,
                    'activation': self.activation, 'use_bias': self.use_bias})
        return cfg


class _SepPart(object):
    """One of the two stages of a SeparableConv2D (or the one stage of a DepthwiseConv2D), presented like a layer of its own: it
    reads the parent's weights through properties, so re-homed (flattened) parameters stay visible (as _ConvPart does)."""

    def __init__(self, parent, which, last):
        self.parent, self.which = parent, which            # which: 'depthwise_kernel' | 'pointwise_kernel'
        self.name = '%s/%s' % (parent.name, which[:-len('_kernel')])
        self.activation = parent.activation if last else 'linear'
        self._last = last

    @property
    def kernel(self):
        return getattr(self.parent, self.which)

    @property
    def bias(self):
        return self.parent.bias if self._last else None


def _pair(v, what):
    p = (v, v) if isinstance(v, (int, np.integer)) else tuple(v)
    if len(p) != 2:
        raise ValueError('%s must be an int or a pair, got %r' % (what, v))
    return tuple(int(a) for a in p)


class DepthwiseConv2D(Layer):
    """keras.layers.DepthwiseConv2D (Keras 2.2.4): strides 1, 'valid' | 'same', dilation 1..4, depth_multiplier 1..8, kernel sizes
    1..7 per axis, bias, activation in {None,'linear','tanh','relu'}, data_format='channels_first'.
    Weights, in Keras order: depthwise_kernel (kh, kw, cin, dm) glorot_uniform (Keras' _compute_fans on this shape: fan_in =
    kh kw cin, fan_out = kh kw dm), bias (cin dm,) zeros.  Output channel c dm + m reads input channel c (csrc/sepconv.hip)."""

    _has_pointwise = False

    def __init__(self, kernel_size, strides=(1, 1), padding='valid', depth_multiplier=1, data_format=None, dilation_rate=(1, 1),
                 activation=None, use_bias=True, depthwise_initializer='glorot_uniform', bias_initializer='zeros',
                 depthwise_regularizer=None, bias_regularizer=None, activity_regularizer=None, depthwise_constraint=None,
                 bias_constraint=None, **kwargs):
        super(DepthwiseConv2D, self).__init__(**kwargs)
        self._init_common(kernel_size, strides, padding, depth_multiplier, data_format, dilation_rate, activation, use_bias,
                          bias_initializer, bias_regularizer, activity_regularizer, bias_constraint)
        if depthwise_initializer not in ('glorot_uniform', 'zeros'):
            raise NotImplementedError('%s: depthwise_initializer %r is not implemented (glorot_uniform, zeros are)'
                                      % (type(self).__name__, depthwise_initializer))
        if depthwise_constraint is not None:
            raise NotImplementedError('%s: depthwise_constraint is not implemented' % type(self).__name__)
        self.depthwise_initializer = depthwise_initializer
        self.depthwise_regularizer = depthwise_regularizer     # l2 handled by the trainer, as Conv2D's kernel_regularizer
        self.depthwise_kernel = None
        self.depthwise_part = _SepPart(self, 'depthwise_kernel', last=not self._has_pointwise)

    def _init_common(self, kernel_size, strides, padding, depth_multiplier, data_format, dilation_rate, activation, use_bias,
                     bias_initializer, bias_regularizer, activity_regularizer, bias_constraint):
        who = type(self).__name__
        ks, st, dl = _pair(kernel_size, 'kernel_size'), _pair(strides, 'strides'), _pair(dilation_rate, 'dilation_rate')
        if st != (1, 1):
            raise NotImplementedError('%s: only strides=1 is implemented, got strides %r' % (who, strides))
        if padding not in ('valid', 'same'):
            raise ValueError("%s padding must be 'valid' or 'same'" % who)
        if any(k < 1 or k > 7 for k in ks):
            raise ValueError('%s: kernel_size %r (1 .. 7 per axis)' % (who, ks))
        if any(d < 1 or d > 4 for d in dl):
            raise ValueError('%s: dilation_rate %r (1 .. 4 per axis)' % (who, dl))
        if int(depth_multiplier) != depth_multiplier or not 1 <= int(depth_multiplier) <= 8:
            raise ValueError('%s: depth_multiplier %r (1 .. 8)' % (who, depth_multiplier))
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation not in (None, 'linear', 'tanh', 'relu'):
            raise NotImplementedError('%s activation %r is not implemented (linear, tanh, relu are)' % (who, activation))
        if bias_initializer not in ('zeros',):
            raise NotImplementedError('%s: bias_initializer %r is not implemented (zeros is)' % (who, bias_initializer))
        if activity_regularizer is not None:
            raise NotImplementedError('%s: activity_regularizer is not implemented' % who)
        if bias_regularizer is not None:
            raise NotImplementedError('%s: bias_regularizer is not implemented' % who)
        if bias_constraint is not None:
            raise NotImplementedError('%s: bias_constraint is not implemented' % who)
        self.kernel_size, self.strides, self.padding, self.dilation_rate = ks, (1, 1), padding, dl
        self.depth_multiplier = int(depth_multiplier)
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("%s: data_format='channels_first' is required (pass it explicitly; Keras' default is "
                                      "channels_last)" % who)
        self.activation = activation or 'linear'
        self.use_bias = bool(use_bias)
        self.bias = None

    same_halo = Conv2D.same_halo

    def _out_channels(self, cin):
        return cin * self.depth_multiplier

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise ValueError('%s expects 4D input, got per-sample shape %r' % (self.name, s))
        c, h, w = s
        if self.padding == 'same':
            return (self._out_channels(c), h, w)
        ho = h - self.dilation_rate[0] * (self.kernel_size[0] - 1)
        wo = w - self.dilation_rate[1] * (self.kernel_size[1] - 1)
        if ho <= 0 or wo <= 0:
            raise ValueError('%s: kernel %r with dilation %r does not fit the input %r' %
                             (self.name, self.kernel_size, self.dilation_rate, s))
        return (self._out_channels(c), ho, wo)

    @staticmethod
    def _glorot(rng, shape, fan_in, fan_out):
        limit = math.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-limit, limit, size=shape).astype(np.float32)

    def _new_depthwise(self, cin, rng):
        kh, kw = self.kernel_size
        shape = (kh, kw, cin, self.depth_multiplier)
        if self.depthwise_initializer == 'glorot_uniform':        # (_compute_fans: receptive field x shape[-2] / shape[-1])
            return self._glorot(rng, shape, kh * kw * cin, kh * kw * self.depth_multiplier)
        return np.zeros(shape, dtype=np.float32)

    def build(self, input_shape, device, rng):
        import torch
        if self.built:
            if self.depthwise_kernel.shape[2] != input_shape[0]:
                raise ValueError('%s was built for %d input channels, now called with %d' %
                                 (self.name, self.depthwise_kernel.shape[2], input_shape[0]))
            return
        cin = int(input_shape[0])
        self.depthwise_kernel = torch.from_numpy(self._new_depthwise(cin, rng)).to(device)
        self._weights = [('depthwise_kernel', self.depthwise_kernel)]
        if self.use_bias:
            self.bias = torch.zeros(cin * self.depth_multiplier, dtype=torch.float32, device=device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(DepthwiseConv2D, self).get_config()
        cfg.update({'kernel_size': self.kernel_size, 'strides': self.strides, 'padding': self.padding,
                    'data_format': self.data_format, 'dilation_rate': self.dilation_rate, 'activation': self.activation,
                    'use_bias': self.use_bias, 'depth_multiplier': self.depth_multiplier})
        return cfg


class SeparableConv2D(DepthwiseConv2D):
    """keras.layers.SeparableConv2D (Keras 2.2.4): a depthwise stencil (no bias, no activation) followed by a 1 x 1 product that
    applies both.  Weights, in Keras order: depthwise_kernel (kh, kw, cin, dm), pointwise_kernel (1, 1, cin dm, filters)
    (glorot_uniform: fan_in = cin dm, fan_out = filters), bias (filters,).  The two stages are `depthwise_part` / `pointwise_part`
    (as ConvLSTM2D's input_part / recurrent_part); the pointwise product runs on the matrix cores (csrc/sepconv.hip)."""

    _has_pointwise = True

    def __init__(self, filters, kernel_size, strides=(1, 1), padding='valid', data_format=None, dilation_rate=(1, 1),
                 depth_multiplier=1, activation=None, use_bias=True, depthwise_initializer='glorot_uniform',
                 pointwise_initializer='glorot_uniform', bias_initializer='zeros', depthwise_regularizer=None,
                 pointwise_regularizer=None, bias_regularizer=None, activity_regularizer=None, depthwise_constraint=None,
                 pointwise_constraint=None, bias_constraint=None, **kwargs):
        super(SeparableConv2D, self).__init__(kernel_size, strides=strides, padding=padding, depth_multiplier=depth_multiplier,
                                              data_format=data_format, dilation_rate=dilation_rate, activation=activation,
                                              use_bias=use_bias, depthwise_initializer=depthwise_initializer,
                                              bias_initializer=bias_initializer, depthwise_regularizer=depthwise_regularizer,
                                              bias_regularizer=bias_regularizer, activity_regularizer=activity_regularizer,
                                              depthwise_constraint=depthwise_constraint, bias_constraint=bias_constraint, **kwargs)
        if pointwise_initializer not in ('glorot_uniform', 'zeros'):
            raise NotImplementedError('SeparableConv2D: pointwise_initializer %r is not implemented (glorot_uniform, zeros are)'
                                      % (pointwise_initializer,))
        if pointwise_constraint is not None:
            raise NotImplementedError('SeparableConv2D: pointwise_constraint is not implemented')
        self.filters = int(filters)
        if self.filters < 1:
            raise ValueError('SeparableConv2D: filters %r' % (filters,))
        self.pointwise_initializer = pointwise_initializer
        self.pointwise_regularizer = pointwise_regularizer
        self.pointwise_kernel = None
        self.pointwise_part = _SepPart(self, 'pointwise_kernel', last=True)

    def _out_channels(self, cin):
        return self.filters

    def build(self, input_shape, device, rng):
        import torch
        if self.built:
            if self.depthwise_kernel.shape[2] != input_shape[0]:
                raise ValueError('%s was built for %d input channels, now called with %d' %
                                 (self.name, self.depthwise_kernel.shape[2], input_shape[0]))
            return
        cin = int(input_shape[0])
        q = cin * self.depth_multiplier
        self.depthwise_kernel = torch.from_numpy(self._new_depthwise(cin, rng)).to(device)
        if self.pointwise_initializer == 'glorot_uniform':
            pk = self._glorot(rng, (1, 1, q, self.filters), q, self.filters)
        else:
            pk = np.zeros((1, 1, q, self.filters), dtype=np.float32)
        self.pointwise_kernel = torch.from_numpy(pk).to(device)
        self._weights = [('depthwise_kernel', self.depthwise_kernel), ('pointwise_kernel', self.pointwise_kernel)]
        if self.use_bias:
            self.bias = torch.zeros(self.filters, dtype=torch.float32, device=device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(SeparableConv2D, self).get_config()
        cfg['filters'] = self.filters
        return cfg


class RowConnected2D(Layer):
    """DLWP.custom.RowConnected2D (reference DLWP/custom.py:695-837; a keras LocallyConnected2D subclass): a convolution whose
    filters are shared along a row only.  kernel (output_rows, kh, kw, cin, filters), bias (output_rows, 1, filters)
    (custom.py:800-816), glorot_uniform / zeros as Keras initialises them for those shapes (every axis in front of the last
    two counts as receptive field).  As in the reference only padding='valid' exists; on the HIP path the layer needs
    strides 1 and data_format='channels_first' (the call sites: examples/train_functional.py:191-196)."""

    def __init__(self, filters, kernel_size, strides=(1, 1), padding='valid', data_format=None, activation=None,
                 use_bias=True, kernel_initializer='glorot_uniform', bias_initializer='zeros', kernel_regularizer=None,
                 bias_regularizer=None, activity_regularizer=None, kernel_constraint=None, bias_constraint=None, **kwargs):
        super(RowConnected2D, self).__init__(**kwargs)
        self.filters = int(filters)
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, (int, np.integer)) else tuple(kernel_size)
        st = (strides, strides) if isinstance(strides, (int, np.integer)) else tuple(strides)
        if len(ks) != 2 or len(st) != 2:
            raise ValueError('kernel_size / strides must be an int or a pair')
        if str(padding).lower() != 'valid':        # keras LocallyConnected2D.__init__
            raise ValueError('Invalid border mode for LocallyConnected2D (only "valid" is supported): ' + str(padding))
        if tuple(st) != (1, 1):
            raise NotImplementedError('RowConnected2D: only strides=1 is implemented (the reference never strides it)')
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation not in (None, 'linear', 'tanh', 'relu'):
            raise NotImplementedError('RowConnected2D activation %r is not implemented (linear, tanh, relu are)' % (activation,))
        if kernel_initializer not in ('glorot_uniform', 'zeros') or bias_initializer not in ('zeros',):
            raise NotImplementedError('initialisers: kernel glorot_uniform|zeros, bias zeros')
        self.kernel_size = tuple(int(k) for k in ks)
        self.strides = (1, 1)
        self.padding = 'valid'
        self.dilation_rate = (1, 1)
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("RowConnected2D: data_format='channels_first' is required (pass it explicitly, as the "
                                      "reference scripts do; Keras' default is channels_last)")
        self.activation = activation or 'linear'
        self.use_bias = bool(use_bias)
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer
        self.kernel = None
        self.bias = None
        self.output_row = self.output_col = None
        self.kernel_shape = None

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise ValueError('%s expects 4D input, got per-sample shape %r' % (self.name, s))
        c, h, w = s
        ho, wo = h - self.kernel_size[0] + 1, w - self.kernel_size[1] + 1
        if ho <= 0 or wo <= 0:
            raise ValueError('%s: kernel %r does not fit the input %r' % (self.name, self.kernel_size, s))
        return (self.filters, ho, wo)

    def build(self, input_shape, device, rng):
        """input_shape: per-sample (cin, h, w) AFTER the halo in front -- the row count of the weights is the output height
        (custom.py:794-805)."""
        import torch
        cin, h, w = (int(v) for v in input_shape)
        kh, kw = self.kernel_size
        rows, cols = h - kh + 1, w - kw + 1
        if self.built:
            if tuple(self.kernel.shape) != (rows, kh, kw, cin, self.filters):
                raise ValueError('%s was built for a kernel of shape %r, now called on an input that needs %r' %
                                 (self.name, tuple(self.kernel.shape), (rows, kh, kw, cin, self.filters)))
            return
        self.output_row, self.output_col = rows, cols
        self.kernel_shape = (rows, kh, kw, cin, self.filters)
        if self.kernel_initializer == 'glorot_uniform':
            rf = rows * kh * kw                       # keras.initializers._compute_fans on a rank-5 shape
            limit = math.sqrt(6.0 / (rf * cin + rf * self.filters))
            k = rng.uniform(-limit, limit, size=self.kernel_shape).astype(np.float32)
        else:
            k = np.zeros(self.kernel_shape, dtype=np.float32)
        self.kernel = torch.from_numpy(k).to(device)
        self._weights = [('kernel', self.kernel)]
        if self.use_bias:
            self.bias = torch.zeros((rows, 1, self.filters), dtype=torch.float32, device=device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(RowConnected2D, self).get_config()
        cfg.update({'filters': self.filters, 'kernel_size': self.kernel_size, 'strides': self.strides,
                    'padding': self.padding, 'data_format': self.data_format, 'activation': self.activation,
                    'use_bias': self.use_bias})
        return cfg


class BatchNormalization(Layer):
    """keras.layers.BatchNormalization -- the `('BatchNormalization', None, {'axis': 1})` entry behind each Conv2D of the reference's
    training scripts (examples/train.py:170-210, commented out there).  Keras 2 defaults.  On the HIP path: 4-D channels_first
    inputs (axis 1 or -3), statistics over (N, H, W) per channel.  Weights in Keras order [gamma, beta, moving_mean,
    moving_variance] (gamma without scale=False, beta without center=False); the moving statistics are NON-TRAINABLE: the
    optimizer and the gradient exchange never see them, training updates them in place."""
    non_trainable_names = ('moving_mean', 'moving_variance')

    def __init__(self, axis=-1, momentum=0.99, epsilon=1e-3, center=True, scale=True, beta_initializer='zeros',
                 gamma_initializer='ones', moving_mean_initializer='zeros', moving_variance_initializer='ones',
                 beta_regularizer=None, gamma_regularizer=None, beta_constraint=None, gamma_constraint=None, renorm=False,
                 renorm_clipping=None, renorm_momentum=0.99, fused=None, virtual_batch_size=None, adjustment=None, **kwargs):
        if kwargs.get('trainable', True) is False:
            raise NotImplementedError('BatchNormalization: trainable=False (frozen statistics) is not implemented')
        super(BatchNormalization, self).__init__(**kwargs)
        for nm, v in (('beta_regularizer', beta_regularizer), ('gamma_regularizer', gamma_regularizer),
                      ('beta_constraint', beta_constraint), ('gamma_constraint', gamma_constraint)):
            if v is not None:
                raise NotImplementedError('BatchNormalization: %s is not implemented' % nm)
        if renorm:
            raise NotImplementedError('BatchNormalization: renorm is not implemented')
        if virtual_batch_size is not None:
            raise NotImplementedError('BatchNormalization: virtual_batch_size is not implemented')
        if adjustment is not None:
            raise NotImplementedError('BatchNormalization: adjustment is not implemented')
        inits = {'beta_initializer': beta_initializer, 'gamma_initializer': gamma_initializer,
                 'moving_mean_initializer': moving_mean_initializer,
                 'moving_variance_initializer': moving_variance_initializer}
        for nm, v in inits.items():
            if v not in ('zeros', 'ones'):
                raise NotImplementedError('BatchNormalization: %s=%r is not implemented (zeros, ones are)' % (nm, v))
        self.axis = int(axis)
        if self.axis not in (1, -3, -1):
            raise NotImplementedError('BatchNormalization: axis=%r is not implemented (axis=1 on channels_first 4-D inputs)'
                                      % (axis,))
        self.momentum = float(momentum)
        self.epsilon = float(epsilon)
        self.center = bool(center)
        self.scale = bool(scale)
        self.initializers = inits
        self.gamma = self.beta = self.moving_mean = self.moving_variance = None

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError('BatchNormalization: only 4-D (N, C, H, W) inputs are implemented, got per-sample shape %r'
                                      % (s,))
        if self.axis == -1:
            raise NotImplementedError("BatchNormalization: axis=-1 (Keras' default, channels_last) is not implemented; "
                                      "pass axis=1 as the reference scripts do")
        return tuple(s)

    def build(self, input_shape, device, rng):
        import torch
        c = int(input_shape[0])
        if self.built:
            if self.moving_mean.shape[0] != c:
                raise ValueError('%s was built for %d channels, now called with %d' % (self.name, self.moving_mean.shape[0], c))
            return

        def init(nm):
            v = 1.0 if self.initializers[nm + '_initializer'] == 'ones' else 0.0
            return torch.full((c,), v, dtype=torch.float32, device=device)
        self._weights = []
        if self.scale:
            self.gamma = init('gamma')
            self._weights.append(('gamma', self.gamma))
        if self.center:
            self.beta = init('beta')
            self._weights.append(('beta', self.beta))
        self.moving_mean = init('moving_mean')
        self.moving_variance = init('moving_variance')
        self._weights += [('moving_mean', self.moving_mean), ('moving_variance', self.moving_variance)]
        self.built = True

    def get_config(self):
        cfg = super(BatchNormalization, self).get_config()
        cfg.update({'axis': self.axis, 'momentum': self.momentum, 'epsilon': self.epsilon, 'center': self.center,
                    'scale': self.scale})
        cfg.update(self.initializers)
        return cfg


class Dense(Layer):
    """keras.layers.Dense on per-sample rank-1 inputs -- the feed-forward model of the reference (examples/train_generator.py:224-233:
    Dense(n_features // 2, tanh, l2) -> Dropout(0.25) -> Dense(n_features)) and the dense head behind Flatten (:138-140).
    Weights in Keras layout: kernel (in, units) glorot_uniform (limit sqrt(6 / (in + units))), bias (units,) zeros.  Activations
    None | 'linear' | 'tanh' | 'relu'.  Keras applies Dense to the last axis of a higher-rank input; no reference call site does,
    and that raises NotImplementedError here."""

    def __init__(self, units, activation=None, use_bias=True, kernel_initializer='glorot_uniform', bias_initializer='zeros',
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, **kwargs):
        if 'input_dim' in kwargs and 'input_shape' not in kwargs:
            kwargs['input_shape'] = (int(kwargs.pop('input_dim')),)
        super(Dense, self).__init__(**kwargs)
        self.units = int(units)
        if self.units <= 0:
            raise ValueError('Dense: units must be positive, got %r' % (units,))
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation not in (None, 'linear', 'tanh', 'relu'):
            raise NotImplementedError('Dense activation %r is not implemented (linear, tanh, relu are)' % (activation,))
        if kernel_initializer not in ('glorot_uniform', 'zeros') or bias_initializer not in ('zeros',):
            raise NotImplementedError('initialisers: kernel glorot_uniform|zeros, bias zeros')
        for nm, v in (('bias_regularizer', bias_regularizer), ('activity_regularizer', activity_regularizer),
                      ('kernel_constraint', kernel_constraint), ('bias_constraint', bias_constraint)):
            if v is not None:
                raise NotImplementedError('Dense: %s is not implemented' % nm)
        self.activation = activation or 'linear'
        self.use_bias = bool(use_bias)
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer   # l2 handled by the trainer when it is a dlwp_amd.regularizers.L2
        self.kernel = None
        self.bias = None

    def compute_output_shape(self, s):
        if len(s) != 1:
            raise NotImplementedError('%s: Dense on a per-sample shape %r is not implemented (Keras would apply it to the last '
                                      'axis; put a Flatten in front)' % (self.name, tuple(s)))
        return (self.units,)

    def build(self, input_shape, device, rng):
        import torch
        fin = int(input_shape[0])
        if self.built:
            if self.kernel.shape[0] != fin:
                raise ValueError('%s was built for %d input features, now called with %d' % (self.name, self.kernel.shape[0], fin))
            return
        if self.kernel_initializer == 'glorot_uniform':
            limit = math.sqrt(6.0 / (fin + self.units))
            k = rng.uniform(-limit, limit, size=(fin, self.units)).astype(np.float32)
        else:
            k = np.zeros((fin, self.units), dtype=np.float32)
        self.kernel = torch.from_numpy(k).to(device)
        self._weights = [('kernel', self.kernel)]
        if self.use_bias:
            self.bias = torch.zeros(self.units, dtype=torch.float32, device=device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(Dense, self).get_config()
        cfg.update({'units': self.units, 'activation': self.activation, 'use_bias': self.use_bias})
        return cfg


class Flatten(Layer):
    """keras.layers.Flatten.  data_format None / 'channels_last' (Keras' default configuration, what `('Flatten', None, None)`
    builds): a relabelling of the contiguous per-sample block, like Reshape -- no launch.  Keras' data_format='channels_first'
    permutes the tensor to channels-last order first; that permutation is not implemented and raises."""

    def __init__(self, data_format=None, **kwargs):
        super(Flatten, self).__init__(**kwargs)
        self.data_format = normalize_data_format(data_format)
        if self.data_format == 'channels_first':
            raise NotImplementedError("Flatten(data_format='channels_first') permutes the tensor to channels-last order before "
                                      "flattening in Keras; that permutation is not implemented (data_format=None keeps the "
                                      "stored order, as Keras' default configuration does)")

    def compute_output_shape(self, s):
        return (int(np.prod(s)),)

    def get_config(self):
        cfg = super(Flatten, self).get_config()
        cfg.update({'data_format': self.data_format})
        return cfg


class Dropout(Layer):
    """keras.layers.Dropout(rate): the identity in predict / evaluate / rollouts (no launch there); in a training step the input times
    mask / (1 - rate).  The mask comes from Philox-4x32-10 keyed by (seed, layer index among the model's Dropout layers, training
    step, element index): no state, the same in the forward and the backward of a step, another one at the next step, reproducible
    from the seed (seed=None draws one from the model's generator when the model is built)."""

    def __init__(self, rate, noise_shape=None, seed=None, **kwargs):
        super(Dropout, self).__init__(**kwargs)
        self.rate = float(rate)
        if not 0.0 <= self.rate < 1.0:
            raise ValueError('Dropout: rate must be in [0, 1), got %r' % (rate,))
        if noise_shape is not None:
            raise NotImplementedError('Dropout: noise_shape is not implemented (one mask element per tensor element)')
        self.noise_shape = None
        self.seed = None if seed is None else int(seed)
        self.mask_seed = self.seed       # what the kernels are keyed with (build() fills it when seed is None)

    def build(self, input_shape, device, rng):
        if self.mask_seed is None:
            self.mask_seed = int(rng.randint(0, 2 ** 31 - 1))
        self.built = True

    def get_config(self):
        cfg = super(Dropout, self).get_config()
        cfg.update({'rate': self.rate, 'noise_shape': None, 'seed': self.seed})
        return cfg


class _Pad3DBase(Layer):
    """ZeroPadding3D / PeriodicPadding3D argument handling (keras ZeroPadding3D forms).  On the HIP path these layers
    pad the recurrent (T, C, H, W) tensor in front of ConvLSTM2D (examples/train.py:144-147): channels_first makes T the
    'channel' axis, so `padding` addresses (C, H, W)."""
    mode = 0

    def __init__(self, padding=(1, 1, 1), data_format=None, **kwargs):
        super(_Pad3DBase, self).__init__(**kwargs)
        self.padding = normalize_padding(padding, 3)
        self.data_format = normalize_data_format(data_format)

    def compute_output_shape(self, s):
        if len(s) != 4:
            raise ValueError('%s expects 5D input (batch + 4), got per-sample shape %r' % (self.name, s))
        p = self.padding
        if self.data_format == 'channels_first':
            return (s[0],) + tuple(s[1 + k] + p[k][0] + p[k][1] for k in range(3))
        return tuple(s[k] + p[k][0] + p[k][1] for k in range(3)) + (s[3],)

    def get_config(self):
        cfg = super(_Pad3DBase, self).get_config()
        cfg.update({'padding': self.padding, 'data_format': self.data_format})
        return cfg


class ZeroPadding3D(_Pad3DBase):
    """keras.layers.ZeroPadding3D -- the pole-row halo in front of ConvLSTM2D (examples/train.py:147)."""
    mode = 0


class _ConvPart(object):
    """One of the two convolutions of a ConvLSTM2D step, presented to the planner / executor like a Conv2D layer: it
    reads the parent's weights through properties, so re-homed (flattened) parameters stay visible."""

    def __init__(self, parent, which):
        self.parent, self.which = parent, which
        self.name = '%s/%s' % (parent.name, 'input_conv' if which == 'kernel' else 'recurrent_conv')
        self.kernel_size = parent.kernel_size
        self.dilation_rate = parent.dilation_rate if which == 'kernel' else (1, 1)
        self.filters = 4 * parent.filters
        self.activation = 'linear'

    @property
    def kernel(self):
        return getattr(self.parent, self.which)

    @property
    def bias(self):
        return self.parent.bias if self.which == 'kernel' else None


class ConvLSTM2D(Layer):
    """keras.layers.ConvLSTM2D as the reference uses it (examples/train.py:148-155, train_functional.py:207-219):
    data_format='channels_first' input (T, C, H, W), stride 1, input convolution 'valid' | 'same' with dilation,
    recurrent convolution 'same' / zero halo / no dilation, gates i, f, c, o, activation tanh,
    recurrent_activation hard_sigmoid | sigmoid, unit_forget_bias, return_sequences.  Weights in Keras order and layout:
    kernel (kh, kw, C, 4F) glorot_uniform, recurrent_kernel (kh, kw, F, 4F) orthogonal, bias (4F,) zeros with the
    forget block at 1.  States start at zero on every call (stateful=False, as everywhere in the reference)."""

    def __init__(self, filters, kernel_size, strides=(1, 1), padding='valid', data_format=None, dilation_rate=(1, 1),
                 activation='tanh', recurrent_activation='hard_sigmoid', use_bias=True,
                 kernel_initializer='glorot_uniform', recurrent_initializer='orthogonal', bias_initializer='zeros',
                 unit_forget_bias=True, kernel_regularizer=None, recurrent_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, kernel_constraint=None, recurrent_constraint=None, bias_constraint=None,
                 return_sequences=False, go_backwards=False, stateful=False, dropout=0., recurrent_dropout=0., **kwargs):
        super(ConvLSTM2D, self).__init__(**kwargs)
        self.filters = int(filters)
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, (int, np.integer)) else tuple(kernel_size)
        st = (strides, strides) if isinstance(strides, (int, np.integer)) else tuple(strides)
        dl = (dilation_rate, dilation_rate) if isinstance(dilation_rate, (int, np.integer)) else tuple(dilation_rate)
        if tuple(st) != (1, 1):
            raise NotImplementedError('ConvLSTM2D: only strides=1 is implemented')
        if padding not in ('valid', 'same'):
            raise ValueError("ConvLSTM2D padding must be 'valid' or 'same'")
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation not in (None, 'linear', 'tanh', 'relu'):
            raise NotImplementedError('ConvLSTM2D activation %r is not implemented' % (activation,))
        if recurrent_activation not in ('hard_sigmoid', 'sigmoid'):
            raise NotImplementedError('ConvLSTM2D recurrent_activation %r is not implemented' % (recurrent_activation,))
        if go_backwards or stateful or dropout or recurrent_dropout:
            raise NotImplementedError('ConvLSTM2D: go_backwards / stateful / dropout are not implemented')
        if any(k % 2 == 0 for k in ks):
            raise NotImplementedError("ConvLSTM2D: even kernel sizes (asymmetric 'same' recurrent halo) are not implemented")
        self.kernel_size = tuple(int(k) for k in ks)
        self.strides = (1, 1)
        self.padding = padding
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("ConvLSTM2D: data_format='channels_first' is required")
        self.dilation_rate = tuple(int(d) for d in dl)
        self.activation = activation or 'linear'
        self.recurrent_activation = recurrent_activation
        self.use_bias = bool(use_bias)
        self.unit_forget_bias = bool(unit_forget_bias)
        self.kernel_regularizer = kernel_regularizer
        self.return_sequences = bool(return_sequences)
        self.kernel = self.recurrent_kernel = self.bias = None
        self.input_part = _ConvPart(self, 'kernel')
        self.recurrent_part = _ConvPart(self, 'recurrent_kernel')

    def same_halo(self):
        tot_h = self.dilation_rate[0] * (self.kernel_size[0] - 1)
        tot_w = self.dilation_rate[1] * (self.kernel_size[1] - 1)
        return (tot_h // 2, tot_h - tot_h // 2, tot_w // 2, tot_w - tot_w // 2)

    def compute_output_shape(self, s):
        if len(s) != 4:
            raise ValueError('%s expects 5D input (batch, time, channels, rows, cols), got per-sample shape %r' %
                             (self.name, s))
        t, c, h, w = s
        if self.padding == 'same':
            ho, wo = h, w
        else:
            ho = h - self.dilation_rate[0] * (self.kernel_size[0] - 1)
            wo = w - self.dilation_rate[1] * (self.kernel_size[1] - 1)
        if ho <= 0 or wo <= 0:
            raise ValueError('%s: kernel %r with dilation %r does not fit the input %r' %
                             (self.name, self.kernel_size, self.dilation_rate, s))
        return (t, self.filters, ho, wo) if self.return_sequences else (self.filters, ho, wo)

    def build(self, input_shape, device, rng):
        import torch
        cin = int(input_shape[1])
        if self.built:
            if self.kernel.shape[2] != cin:
                raise ValueError('%s was built for %d input channels, now called with %d' %
                                 (self.name, self.kernel.shape[2], cin))
            return
        kh, kw = self.kernel_size
        f = self.filters
        limit = math.sqrt(6.0 / (kh * kw * cin + kh * kw * 4 * f))
        k = rng.uniform(-limit, limit, size=(kh, kw, cin, 4 * f)).astype(np.float32)
        # keras.initializers.Orthogonal: SVD of a normal matrix flattened to (prod(shape[:-1]), shape[-1])
        a = rng.normal(0.0, 1.0, (kh * kw * f, 4 * f))
        u, _, vt = np.linalg.svd(a, full_matrices=False)
        q = u if u.shape == a.shape else vt
        r = q.reshape(kh, kw, f, 4 * f).astype(np.float32)
        self.kernel = torch.from_numpy(k).to(device)
        self.recurrent_kernel = torch.from_numpy(np.ascontiguousarray(r)).to(device)
        self._weights = [('kernel', self.kernel), ('recurrent_kernel', self.recurrent_kernel)]
        if self.use_bias:
            b = np.zeros(4 * f, dtype=np.float32)
            if self.unit_forget_bias:
                b[f:2 * f] = 1.0
            self.bias = torch.from_numpy(b).to(device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(ConvLSTM2D, self).get_config()
        cfg.update({'filters': self.filters, 'kernel_size': self.kernel_size, 'padding': self.padding,
                    'data_format': self.data_format, 'dilation_rate': self.dilation_rate,
                    'activation': self.activation, 'recurrent_activation': self.recurrent_activation,
                    'use_bias': self.use_bias, 'unit_forget_bias': self.unit_forget_bias,
                    'return_sequences': self.return_sequences})
        return cfg


class MaxPooling2D(Layer):
    """keras.layers.MaxPooling2D(2): 2x2 / stride 2 / 'valid' (examples/train.py:171,181)."""

    def __init__(self, pool_size=(2, 2), strides=None, padding='valid', data_format=None, **kwargs):
        super(MaxPooling2D, self).__init__(**kwargs)
        ps = (pool_size, pool_size) if isinstance(pool_size, (int, np.integer)) else tuple(pool_size)
        st = ps if strides is None else ((strides, strides) if isinstance(strides, (int, np.integer)) else tuple(strides))
        if tuple(ps) != (2, 2) or tuple(st) != (2, 2) or padding != 'valid':
            raise NotImplementedError("MaxPooling2D: only pool_size=2, strides=2, padding='valid' is implemented")
        self.pool_size, self.strides, self.padding = (2, 2), (2, 2), 'valid'
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("MaxPooling2D: data_format='channels_first' is required")

    def compute_output_shape(self, s):
        return (s[0], s[1] // 2, s[2] // 2)


class AveragePooling2D(Layer):
    """keras.layers.AveragePooling2D(2): 2x2 / stride 2 / 'valid' (the reference's average-pooling U-Net, examples/validate.py:35-44).
    An odd last row / column belongs to no window.  No weights, no state."""

    def __init__(self, pool_size=(2, 2), strides=None, padding='valid', data_format=None, **kwargs):
        super(AveragePooling2D, self).__init__(**kwargs)
        ps = (pool_size, pool_size) if isinstance(pool_size, (int, np.integer)) else tuple(pool_size)
        st = ps if strides is None else ((strides, strides) if isinstance(strides, (int, np.integer)) else tuple(strides))
        if tuple(ps) != (2, 2) or tuple(st) != (2, 2) or padding != 'valid':
            raise NotImplementedError("AveragePooling2D: only pool_size=2, strides=2, padding='valid' is implemented")
        self.pool_size, self.strides, self.padding = (2, 2), (2, 2), 'valid'
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("AveragePooling2D: data_format='channels_first' is required")

    def compute_output_shape(self, s):
        return (s[0], s[1] // 2, s[2] // 2)

    def get_config(self):
        cfg = super(AveragePooling2D, self).get_config()
        cfg.update({'pool_size': self.pool_size, 'strides': self.strides, 'padding': self.padding,
                    'data_format': self.data_format})
        return cfg


class UpSampling2D(Layer):
    """keras.layers.UpSampling2D(2): 'nearest' (examples/train.py:191,201) or 'bilinear' (Keras 2.2.4's
    tf.image.resize_bilinear with align_corners=False and no half-pixel centres: even outputs copy the source, odd outputs are the
    mean of two neighbours, the last one clamped).  No weights, no state."""

    def __init__(self, size=(2, 2), data_format=None, interpolation='nearest', **kwargs):
        super(UpSampling2D, self).__init__(**kwargs)
        sz = (size, size) if isinstance(size, (int, np.integer)) else tuple(size)
        if interpolation not in ('nearest', 'bilinear'):
            raise ValueError('`interpolation` argument should be one of `"nearest"` or `"bilinear"`.')
        if tuple(sz) != (2, 2):
            raise NotImplementedError('UpSampling2D: only size=2 is implemented')
        self.size = (2, 2)
        self.interpolation = interpolation
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("UpSampling2D: data_format='channels_first' is required")

    def compute_output_shape(self, s):
        return (s[0], s[1] * 2, s[2] * 2)

    def get_config(self):
        cfg = super(UpSampling2D, self).get_config()
        cfg.update({'size': self.size, 'data_format': self.data_format, 'interpolation': self.interpolation})
        return cfg


def _deconv_length(length, k, padding):
    """Keras' deconv_length for stride 2 and no output_padding: 'valid' 2 n + max(k - 2, 0), 'same' 2 n."""
    return 2 * int(length) + (max(int(k) - 2, 0) if padding == 'valid' else 0)


class Conv2DTranspose(Layer):
    """keras.layers.Conv2DTranspose with strides=2: the learned up-sampling of a decoder.  'valid' | 'same', bias, activation in
    {None,'linear','tanh','relu'}, data_format='channels_first'.  y_full[o, 2i+u, 2j+v] += x[c, i, j] K[u, v, o, c] (no flip) on
    2h + max(kh-2, 0) rows; 'same' keeps rows [pt, pt + 2h), pt = max(kh-2, 0) // 2 -- the gradient of a SAME-padded stride-2
    convolution.  Weights: kernel (kh, kw, filters, cin) glorot_uniform (Keras' order: filters before input channels), bias
    (filters,) zeros.  Runs as one stride-1 convolution with 4 x filters phase channels + a cropping interleave (csrc/tconv.hip)."""

    def __init__(self, filters, kernel_size, strides=(2, 2), padding='valid', output_padding=None, data_format=None,
                 dilation_rate=(1, 1), activation=None, use_bias=True, kernel_initializer='glorot_uniform',
                 bias_initializer='zeros', kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None, **kwargs):
        super(Conv2DTranspose, self).__init__(**kwargs)
        self.filters = int(filters)
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, (int, np.integer)) else tuple(kernel_size)
        st = (strides, strides) if isinstance(strides, (int, np.integer)) else tuple(strides)
        dl = (dilation_rate, dilation_rate) if isinstance(dilation_rate, (int, np.integer)) else tuple(dilation_rate)
        if len(ks) != 2 or len(st) != 2 or len(dl) != 2:
            raise ValueError('kernel_size / strides / dilation_rate must be an int or a pair')
        if any(int(k) <= 0 for k in ks):
            raise ValueError('Conv2DTranspose: kernel_size %r' % (ks,))
        if tuple(st) != (2, 2):
            raise NotImplementedError('Conv2DTranspose: only strides=2 is implemented, got %r' % (tuple(st),))
        if tuple(dl) != (1, 1):
            raise NotImplementedError('Conv2DTranspose: dilation_rate %r is not implemented (1 is)' % (tuple(dl),))
        if output_padding is not None:
            raise NotImplementedError('Conv2DTranspose: output_padding=%r is not implemented (None is)' % (output_padding,))
        if padding not in ('valid', 'same'):
            raise ValueError("Conv2DTranspose padding must be 'valid' or 'same'")
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation not in (None, 'linear', 'tanh', 'relu'):
            raise NotImplementedError('Conv2DTranspose activation %r is not implemented (linear, tanh, relu are)' % (activation,))
        if kernel_initializer not in ('glorot_uniform', 'zeros') or bias_initializer not in ('zeros',):
            raise NotImplementedError('Conv2DTranspose initialisers: kernel glorot_uniform|zeros, bias zeros')
        self.kernel_size = tuple(int(k) for k in ks)
        self.strides = (2, 2)
        self.padding = padding
        self.output_padding = None
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("Conv2DTranspose: data_format='channels_first' is required (pass it explicitly; Keras' "
                                      "default is channels_last)")
        self.dilation_rate = (1, 1)
        self.activation = activation or 'linear'
        self.use_bias = bool(use_bias)
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer   # l2 handled by the trainer when it is a dlwp_amd.regularizers.L2
        self.kernel = None
        self.bias = None

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError('%s (Conv2DTranspose) expects a 4D input, got the per-sample shape %r' % (self.name, s))
        c, h, w = s
        return (self.filters, _deconv_length(h, self.kernel_size[0], self.padding),
                _deconv_length(w, self.kernel_size[1], self.padding))

    def build(self, input_shape, device, rng):
        import torch
        if self.built:
            if self.kernel.shape[3] != input_shape[0]:
                raise ValueError('%s was built for %d input channels, now called with %d' %
                                 (self.name, self.kernel.shape[3], input_shape[0]))
            return
        kh, kw = self.kernel_size
        cin = int(input_shape[0])
        if self.kernel_initializer == 'glorot_uniform':      # Keras' fans of (kh, kw, filters, cin): the limit is symmetric in them
            limit = math.sqrt(6.0 / (kh * kw * self.filters + kh * kw * cin))
            k = rng.uniform(-limit, limit, size=(kh, kw, self.filters, cin)).astype(np.float32)
        else:
            k = np.zeros((kh, kw, self.filters, cin), dtype=np.float32)
        self.kernel = torch.from_numpy(k).to(device)
        self._weights = [('kernel', self.kernel)]
        if self.use_bias:
            self.bias = torch.zeros(self.filters, dtype=torch.float32, device=device)
            self._weights.append(('bias', self.bias))
        self.built = True

    def get_config(self):
        cfg = super(Conv2DTranspose, self).get_config()
        cfg.update({'filters': self.filters, 'kernel_size': self.kernel_size, 'strides': self.strides, 'padding': self.padding,
                    'output_padding': None, 'data_format': self.data_format, 'dilation_rate': self.dilation_rate,
                    'activation': self.activation, 'use_bias': self.use_bias})
        return cfg


def _normalize_cropping(cropping):
    """Keras Cropping2D: int | (ch, cw) | ((top, bottom), (left, right))  ->  ((top, bottom), (left, right))."""
    if isinstance(cropping, (int, np.integer)):
        out = ((int(cropping),) * 2,) * 2
    else:
        if not hasattr(cropping, '__len__') or len(cropping) != 2:
            raise ValueError('`cropping` should have two elements. Found: %r' % (cropping,))
        out = []
        for c in cropping:
            if isinstance(c, (int, np.integer)):
                out.append((int(c), int(c)))
            else:
                c = tuple(int(v) for v in c)
                if len(c) != 2:
                    raise ValueError('`cropping` should be either an int, a tuple of 2 ints or a tuple of 2 tuples of 2 ints. '
                                     'Found: %r' % (cropping,))
                out.append(c)
        out = tuple(out)
    if any(v < 0 for c in out for v in c):
        raise ValueError('negative cropping is not supported: %r' % (cropping,))
    return out


class Cropping2D(Layer):
    """keras.layers.Cropping2D: drops rows / columns at the borders -- trims a decoder's output, or takes the pole row / the
    periodic halo off again so that an odd grid (73 x 144) runs through a pool / up-sample stack.  data_format='channels_first'.
    Its forward is the adjoint of zero padding (dlwp_pad2d_bwd, 'zero drops'), its gradient zero padding.  No weights."""

    def __init__(self, cropping=((0, 0), (0, 0)), data_format=None, **kwargs):
        super(Cropping2D, self).__init__(**kwargs)
        self.cropping = _normalize_cropping(cropping)
        self.data_format = normalize_data_format(data_format)
        if self.data_format != 'channels_first':
            raise NotImplementedError("Cropping2D: data_format='channels_first' is required (pass it explicitly; Keras' default "
                                      "is channels_last)")

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError('%s (Cropping2D) expects a 4D input, got the per-sample shape %r' % (self.name, s))
        (t, b), (l, r) = self.cropping
        h, w = s[1] - t - b, s[2] - l - r
        if h <= 0 or w <= 0:
            raise ValueError('%s (Cropping2D): cropping %r leaves nothing of the input %r' % (self.name, self.cropping, tuple(s)))
        return (s[0], h, w)

    def get_config(self):
        cfg = super(Cropping2D, self).get_config()
        cfg.update({'cropping': self.cropping, 'data_format': self.data_format})
        return cfg


class Reshape(Layer):
    """keras.layers.Reshape(target_shape): a relabelling of the contiguous per-sample block (examples/train.py:220)."""

    def __init__(self, target_shape, **kwargs):
        super(Reshape, self).__init__(**kwargs)
        self.target_shape = tuple(int(v) for v in target_shape)

    def compute_output_shape(self, s):
        n_in = int(np.prod(s))
        tgt = list(self.target_shape)
        if tgt.count(-1) > 1:
            raise ValueError('Reshape: at most one -1')
        if -1 in tgt:
            known = int(np.prod([v for v in tgt if v != -1]))
            tgt[tgt.index(-1)] = n_in // max(known, 1)
        if int(np.prod(tgt)) != n_in:
            raise ValueError('total size of new array must be unchanged: %r -> %r' % (s, self.target_shape))
        return tuple(tgt)


class ChannelSlice(Layer):
    """What `slice_layer(start, end, axis=1)` builds (DLWP/custom.py:675-692): a window of the channel axis."""

    def __init__(self, start, end, step=None, axis=1, **kwargs):
        super(ChannelSlice, self).__init__(**kwargs)
        if step not in (None, 1):
            raise NotImplementedError('slice_layer: only step=None/1 is implemented')
        if axis != 1:
            raise NotImplementedError('slice_layer: only axis=1 (channels_first channel axis) is implemented')
        self.start, self.end, self.axis = start, end, axis

    def window(self, c):
        lo, hi, _ = slice(self.start, self.end).indices(c)
        if hi <= lo:
            raise ValueError('slice_layer(%r, %r) selects no channels out of %d' % (self.start, self.end, c))
        return lo, hi

    def compute_output_shape(self, s):
        lo, hi = self.window(s[0])
        return (hi - lo,) + tuple(s[1:])


class Concatenate(Layer):
    """keras.layers.Concatenate(axis=1) for channels_first maps (examples/train_functional.py:255,259,266,270)."""

    def __init__(self, axis=-1, **kwargs):
        super(Concatenate, self).__init__(**kwargs)
        self.axis = axis

    def compute_output_shape(self, shapes):
        if not isinstance(shapes, list) or len(shapes) < 2:
            raise ValueError('Concatenate needs a list of at least 2 inputs')
        rank = len(shapes[0]) + 1
        ax = self.axis if self.axis >= 0 else rank + self.axis
        if ax != 1:
            raise NotImplementedError('Concatenate: only the channel axis (axis=1, channels_first) is implemented')
        for s in shapes[1:]:
            if tuple(s[1:]) != tuple(shapes[0][1:]):
                raise ValueError('Concatenate: inputs must match except on the channel axis: %r' % (shapes,))
        return (sum(s[0] for s in shapes),) + tuple(shapes[0][1:])


def concatenate(inputs, axis=-1, **kwargs):
    return Concatenate(axis=axis, **kwargs)(list(inputs))


# ------------------------------------------------------------------------------------------------------------------ #
# Activation layers (keras.layers.Activation, keras.layers.advanced_activations) and merge layers (keras.layers.merge):
# element-wise, no weights, no state -- a layer object may be applied any number of times.  The closed forms are the
# project's statement of Keras 2.2.x; the kernels are csrc/eltwise.hip.
# ------------------------------------------------------------------------------------------------------------------ #

#: what Activation(name) lowers to: 'relu' is the relu family at its defaults, 'linear' is a view
ELTWISE_ACTIVATIONS = ('relu', 'elu', 'selu', 'sigmoid', 'hard_sigmoid', 'softplus', 'softsign', 'tanh')


def _relu_family(who, alpha, max_value, theta):
    """(alpha, max_value | None, theta) of y = x > theta ? min(x, max_value) : alpha (x - theta), validated"""
    alpha, theta = float(alpha), float(theta)
    max_value = None if max_value is None else float(max_value)
    if not alpha >= 0.0 or math.isinf(alpha):
        raise ValueError('%s: the negative slope must be a finite number >= 0, got %r' % (who, alpha))
    if not theta >= 0.0 or math.isinf(theta):
        if theta < 0.0:
            raise NotImplementedError('%s: a negative threshold (%r) is not implemented' % (who, theta))
        raise ValueError('%s: the threshold must be a finite number, got %r' % (who, theta))
    if max_value is not None and not max_value > theta:
        raise NotImplementedError('%s: max_value=%r at or below the threshold %r is not implemented' % (who, max_value, theta))
    return alpha, max_value, theta


class _ActivationLayer(Layer):
    """An element-wise function of one tensor.  eltwise: None (the identity: a view, no launch) or (kind, alpha,
    max_value | None, theta) with kind in ELTWISE_ACTIVATIONS -- what plan / engine / backward launch."""
    eltwise = None

    def compute_output_shape(self, input_shape):
        if isinstance(input_shape, list):
            raise ValueError('%s takes one input tensor, got a list of %d' % (self.name, len(input_shape)))
        return tuple(input_shape)


class Activation(_ActivationLayer):
    """keras.layers.Activation(activation): 'linear' | 'relu' | 'elu' | 'selu' | 'sigmoid' | 'hard_sigmoid' | 'softplus' |
    'softsign' | 'tanh', or a Keras activation function of one of those names.  'softmax' and 'exponential' are not implemented."""

    def __init__(self, activation, **kwargs):
        super(Activation, self).__init__(**kwargs)
        if callable(activation):
            activation = getattr(activation, '__name__', None)
        if activation is None:
            activation = 'linear'
        if activation in ('softmax', 'exponential'):
            raise NotImplementedError('Activation(%r) is not implemented' % (activation,))
        if activation != 'linear' and activation not in ELTWISE_ACTIVATIONS:
            raise ValueError('Activation: unknown activation function %r' % (activation,))
        self.activation = activation
        if activation == 'relu':
            self.eltwise = ('relu', 0.0, None, 0.0)
        elif activation == 'elu':
            self.eltwise = ('elu', 1.0, None, 0.0)
        elif activation != 'linear':
            self.eltwise = (activation, 0.0, None, 0.0)

    def get_config(self):
        cfg = super(Activation, self).get_config()
        cfg.update({'activation': self.activation})
        return cfg


class LeakyReLU(_ActivationLayer):
    """keras.layers.LeakyReLU(alpha=0.3): x > 0 ? x : alpha x"""

    def __init__(self, alpha=0.3, **kwargs):
        super(LeakyReLU, self).__init__(**kwargs)
        self.alpha = _relu_family('LeakyReLU', alpha, None, 0.0)[0]
        self.eltwise = ('relu', self.alpha, None, 0.0)

    def get_config(self):
        cfg = super(LeakyReLU, self).get_config()
        cfg.update({'alpha': self.alpha})
        return cfg


class ReLU(_ActivationLayer):
    """keras.layers.ReLU(max_value=None, negative_slope=0., threshold=0.): x > threshold ? min(x, max_value) :
    negative_slope (x - threshold).  ReLU(max_value=m, negative_slope=a) is the capped leaky ReLU."""

    def __init__(self, max_value=None, negative_slope=0., threshold=0., **kwargs):
        super(ReLU, self).__init__(**kwargs)
        self.negative_slope, self.max_value, self.threshold = _relu_family('ReLU', negative_slope, max_value, threshold)
        self.eltwise = ('relu', self.negative_slope, self.max_value, self.threshold)

    def get_config(self):
        cfg = super(ReLU, self).get_config()
        cfg.update({'max_value': self.max_value, 'negative_slope': self.negative_slope, 'threshold': self.threshold})
        return cfg


class ELU(_ActivationLayer):
    """keras.layers.ELU(alpha=1.0): x > 0 ? x : alpha (exp(x) - 1)"""

    def __init__(self, alpha=1.0, **kwargs):
        super(ELU, self).__init__(**kwargs)
        self.alpha = float(alpha)
        if math.isnan(self.alpha) or math.isinf(self.alpha):
            raise ValueError('ELU: alpha must be a finite number, got %r' % (alpha,))
        self.eltwise = ('elu', self.alpha, None, 0.0)

    def get_config(self):
        cfg = super(ELU, self).get_config()
        cfg.update({'alpha': self.alpha})
        return cfg


class ThresholdedReLU(_ActivationLayer):
    """keras.layers.ThresholdedReLU(theta=1.0): x > theta ? x : 0"""

    def __init__(self, theta=1.0, **kwargs):
        super(ThresholdedReLU, self).__init__(**kwargs)
        self.theta = _relu_family('ThresholdedReLU', 0.0, None, theta)[2]
        self.eltwise = ('relu', 0.0, None, self.theta)

    def get_config(self):
        cfg = super(ThresholdedReLU, self).get_config()
        cfg.update({'theta': self.theta})
        return cfg


class PReLU(Layer):
    """keras.layers.PReLU has a learned slope per element: not implemented."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('PReLU (a learned negative slope) is not implemented; LeakyReLU(alpha) has a fixed one')


class Softmax(Layer):
    """keras.layers.Softmax normalises along an axis, it is not element-wise: not implemented."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('Softmax is not implemented (the element-wise activations of keras.layers.Activation are)')


MERGE_MAX_INPUTS = 4


class _Merge(Layer):
    """keras.layers.merge._Merge on inputs of identical shape: ((a o b) o c) o d, left to right in float32, 2 to 4 inputs."""
    kind = None

    def compute_output_shape(self, shapes):
        if not isinstance(shapes, list) or len(shapes) < 2:
            raise ValueError('A merge layer should be called on a list of at least 2 inputs (%s)' % self.name)
        if len(shapes) > MERGE_MAX_INPUTS:
            raise NotImplementedError('%s: %d inputs; merging more than %d is not implemented (nest two layers)'
                                      % (self.name, len(shapes), MERGE_MAX_INPUTS))
        for s in shapes[1:]:
            if tuple(s) != tuple(shapes[0]):
                raise ValueError('%s: inputs must have the same shape (no broadcasting), got %r' % (self.name, shapes))
        return tuple(shapes[0])


class Add(_Merge):
    """keras.layers.Add"""
    kind = 'add'


class Subtract(_Merge):
    """keras.layers.Subtract: exactly two inputs, a - b"""
    kind = 'subtract'

    def compute_output_shape(self, shapes):
        if not isinstance(shapes, list) or len(shapes) != 2:
            raise ValueError('A `Subtract` layer should be called on exactly 2 inputs')
        return super(Subtract, self).compute_output_shape(shapes)


class Multiply(_Merge):
    """keras.layers.Multiply"""
    kind = 'multiply'


class Average(_Merge):
    """keras.layers.Average: the left-to-right sum divided by float32(number of inputs)"""
    kind = 'average'


class Maximum(_Merge):
    """keras.layers.Maximum (NaN propagates, as in np.maximum)"""
    kind = 'maximum'


class Minimum(_Merge):
    """keras.layers.Minimum (NaN propagates, as in np.minimum)"""
    kind = 'minimum'


def add(inputs, **kwargs):
    return Add(**kwargs)(list(inputs))


def subtract(inputs, **kwargs):
    return Subtract(**kwargs)(list(inputs))


def multiply(inputs, **kwargs):
    return Multiply(**kwargs)(list(inputs))


def average(inputs, **kwargs):
    return Average(**kwargs)(list(inputs))


def maximum(inputs, **kwargs):
    return Maximum(**kwargs)(list(inputs))


def minimum(inputs, **kwargs):
    return Minimum(**kwargs)(list(inputs))
