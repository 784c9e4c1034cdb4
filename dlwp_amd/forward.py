"""
The forward side of a plan op, one function per op kind, in the two forms the Executor (engine.py) walks a plan in:

  LAUNCHES   kind -> launch(ex, k, op, d, src, dst, res, prepared, training): the eager launch of Executor.run;
  ROLLOUT_OPS   kind -> (OP_* code, encoder): the op's _lib.Op record in the table a rollout graph is captured from
  (OpTable, Executor.encode_ops).

The backward side is BackwardPass.adjoints (backward.py), the planner's plan._LOWERINGS.  A new op kind needs one entry in
each; tests/test_executor_cpu.py pins both walks here byte for byte and fails for a kind without a fixture.
"""
import struct

from . import _lib, ops

WEIGHT_KINDS = ('phasew', 'tphasew', 'sphasew')      # kernel -> derived kernel (plan.phase_params)


def _f32_bits(v):
    """a float32 as the int that carries its bits in an Op's aux slot"""
    return struct.unpack('<i', struct.pack('<f', v))[0]


# A convolution multiplies with its layer's kernel and bias, or with the derived ones of a restated layer -- except that a strided
# Conv2D ('sconv') restates its kernel only and keeps its own bias.  On tensors for a launch, on table indices for an Op record:
def conv_weights(ex, op):
    if op.wparam is None:
        return op.layer.kernel, op.layer.bias
    w2, b2 = ex.phase_buffers()[op.wparam]
    return w2, (op.layer.bias if ex.plan.phase_params[op.wparam].get('kind') == 'sconv' else b2)


def conv_indices(table, op):
    if op.wparam is None:
        return table.conv[id(op.layer)]
    w2, b2 = table.phase[op.wparam]
    return w2, (table.conv[id(op.layer)][1] if table.ex.plan.phase_params[op.wparam].get('kind') == 'sconv' else b2)


# -- eager launches -------------------------------------------------------------------------------------------------------- #
# res(i): the tensor of buffer index i (scratch, model input, output slot); prepared / training: as Executor.run takes them.
def _conv(ex, k, op, d, src, dst, res, prepared, training):
    kern, bias = conv_weights(ex, op)
    if op.src2 is not None:          # a whole ConvLSTM2D step (dlwp_convlstm_step_fwd)
        if op.dst not in ex._oct:
            raise RuntimeError('whole-step ConvLSTM2D launches need the h sequence in octets (Model.set_activation_dtype '
                               're-plans without them otherwise)')
        za, cp, co = op.aux
        ops.convlstm_step(dst, res(op.src2['buf']), kern, op.src2['layer'].kernel, op.src2['layer'].bias, d,
                          ex._descriptor2(op), res(cp), res(co), op.src2['xs'][0])
    elif op.lstm_f:
        za, cp, co = op.aux
        ops.convlstm_conv(src, kern, bias, d, dst, res(co), z_add=res(za) if za is not None else None,
                          c_prev=res(cp) if cp is not None else None, x_channels=op.xs[0],
                          compute_bf16=(op.dst in ex._bf16 and op.src not in ex._bf16),
                          in_o8=op.src in ex._oct, out_o8=op.dst in ex._oct)
    else:
        ops.conv2d(src, kern, bias, d, out=dst, x_channels=op.xs[0],
                   compute_bf16=(op.dst in ex._bf16 and op.src not in ex._bf16),
                   prepared=prepared.get(k) if prepared else None,
                   in_o8=op.src in ex._oct, out_o8=op.dst in ex._oct)


def _rowconv(ex, k, op, d, src, dst, res, prepared, training):
    ops.rowconv2d(src, op.layer.kernel, op.layer.bias, d, out=dst, x_channels=op.xs[0])


def _derive_weights(ex, k, op, d, src, dst, res, prepared, training):
    w2, b2 = ex.phase_buffers()[op.wparam]
    if op.kind == 'phasew':
        ops.phase_weights(op.layer.kernel, op.layer.bias, op.halo.top, op.halo.left, w2=w2, b2=b2)
    elif op.kind == 'tphasew':       # Conv2DTranspose: kernel -> the kernel of its 4 F phase channels
        ops.tconv_weights(op.layer.kernel, op.layer.bias, w2=w2, b2=b2)
    else:                            # Conv2D(strides=2): kernel -> the kernel on its 4 cin phase channels
        ops.sconv_weights(op.layer.kernel, w2=w2)


def _d2s(ex, k, op, d, src, dst, res, prepared, training):
    ops.depth_to_space2(src, op.xs[0], out=dst, c_off=op.out_c_off)


def _d2sc(ex, k, op, d, src, dst, res, prepared, training):
    ops.depth_to_space2_crop(src, op.xs[0], op.crop[0], op.crop[1], op.out_shape[1], op.out_shape[2], out=dst,
                             c_off=op.out_c_off)


def _crop(ex, k, op, d, src, dst, res, prepared, training):
    ops.crop2d(src, d, out=dst)


def _dwconv(ex, k, op, d, src, dst, res, prepared, training):
    """DepthwiseConv2D / the stencil of a SeparableConv2D (which has no bias of its own)"""
    ops.depthwise2d(src, op.layer.depthwise_kernel, op.layer.depthwise_part.bias, d, out=dst)


def _pwconv(ex, k, op, d, src, dst, res, prepared, training):
    """the 1 x 1 product of a SeparableConv2D"""
    ops.pointwise2d(src, op.layer.pointwise_kernel, op.layer.bias, d, out=dst)


def _s2dp(ex, k, op, d, src, dst, res, prepared, training):
    """halo + 'same' zeros + de-interleave, one pass"""
    ops.space_to_depth2_pad(src, op.xs[0], d, op.out_shape[1], op.out_shape[2], c_off=op.in_c_off, out=dst)


def _pad(ex, k, op, d, src, dst, res, prepared, training):
    if op.inner > 1:
        hh, ww = op.xs[1], op.xs[2]
        ops.pad2d(src.reshape(src.shape[0], hh, ww, op.inner), d, channels_last=True, out=dst)
    else:
        ops.pad2d(src, d, out=dst)


def _maxpool(ex, k, op, d, src, dst, res, prepared, training):
    ops.maxpool2(src, out=dst)


def _avgpool(ex, k, op, d, src, dst, res, prepared, training):
    ops.avgpool2(src, out=dst)


def _upsample(ex, k, op, d, src, dst, res, prepared, training):
    ops.upsample2(src, out=dst)


def _bilinear(ex, k, op, d, src, dst, res, prepared, training):
    ops.upsample2_bilinear(src, out=dst)


def _copy(ex, k, op, d, src, dst, res, prepared, training):
    if tuple(dst.shape[2:]) != tuple(src.shape[2:]) and dst.numel() == src.numel():
        dst = dst.view(src.shape)          # a Reshape relabelled the target: the same contiguous block
    ops.copy_channels(src, dst, op.xs[0], op.in_c_off, op.out_c_off)


def _dense(ex, k, op, d, src, dst, res, prepared, training):
    ops.dense_fwd(src, op.layer.kernel, op.layer.bias, op.act, out=dst)


def _dropout(ex, k, op, d, src, dst, res, prepared, training):
    """(training plans only; outside a training step: rate 0 = a copy)"""
    lay = op.layer
    ops.dropout_fwd(src, lay.rate if training else 0.0, lay.mask_seed, ex.plan.dropout_layers.index(lay), ex.dropout_step,
                    out=dst)


def _bn(ex, k, op, d, src, dst, res, prepared, training):
    lay = op.layer
    if training:
        st = ex.bn_state(k, src.shape[0])
        ops.batchnorm_fwd_train(src, lay.gamma, lay.beta, lay.moving_mean, lay.moving_variance, st['mean'],
                                st['invstd'], st['ws'], lay.momentum, lay.epsilon, out=dst)
    else:
        ops.batchnorm_fwd_infer(src, lay.gamma, lay.beta, lay.moving_mean, lay.moving_variance, lay.epsilon,
                                out=dst)


def _act(ex, k, op, d, src, dst, res, prepared, training):
    """keras activation layers: whole flat buffers (csrc/eltwise.hip)"""
    ops.activation_fwd(src, *op.layer.eltwise, out=dst)


def _merge(ex, k, op, d, src, dst, res, prepared, training):
    """keras merge layers: 2 to 4 whole flat buffers of one size"""
    ops.merge_fwd(op.layer.kind, [src] + [res(b) for b in op.aux], out=dst)


def _scale(ex, k, op, d, src, dst, res, prepared, training):
    """the wrapper's imputer + scaler in front, its inverse scaler behind (in place)"""
    st = ex.transform[op.role]
    if op.role == 'head':
        ops.scale_fwd(src, st.kind, st.fill, st.shift, st.scale, out=dst)
    else:
        ops.scale_inv(src, st.kind, st.shift, st.scale, out=dst)


def _lstm(ex, k, op, d, src, dst, res, prepared, training):
    zh, cp, co = op.aux
    ops.convlstm_gates(src, res(zh) if zh is not None else None, res(cp) if cp is not None else None,
                       res(co), dst, op.xs[0], h_c_off=op.out_c_off, act=op.act, rec_act=op.rec_act)


LAUNCHES = {'conv': _conv, 'rowconv': _rowconv, 'phasew': _derive_weights, 'tphasew': _derive_weights,
            'sphasew': _derive_weights, 'd2s': _d2s, 'd2sc': _d2sc, 'crop': _crop, 'dwconv': _dwconv, 'pwconv': _pwconv,
            's2dp': _s2dp, 'pad': _pad, 'maxpool': _maxpool, 'avgpool': _avgpool, 'upsample': _upsample,
            'bilinear': _bilinear, 'copy': _copy, 'dense': _dense, 'dropout': _dropout, 'bn': _bn, 'act': _act,
            'merge': _merge, 'scale': _scale, 'lstm': _lstm}


def launches_of(plan):
    """the launch of every op of a plan, resolved once (Executor._launches)"""
    for op in plan.ops:
        if op.kind not in LAUNCHES:
            raise RuntimeError(op.kind)
    return [LAUNCHES[op.kind] for op in plan.ops]


# -- rollout op records ---------------------------------------------------------------------------------------------------- #
class ParamTable(object):
    """The tensors a rollout graph addresses by index: add() appends the tensors that exist and returns each one's index, -1 for
    None."""

    def __init__(self, tensors=()):
        self.tensors = list(tensors)

    def add(self, *tensors):
        idx = []
        for t in tensors:
            idx.append(-1 if t is None else len(self.tensors))
            if t is not None:
                self.tensors.append(t)
        return tuple(idx)


def _or_none(buf):
    return buf if buf is not None else _lib.BUF_NONE


def _windows(o, d):
    o.conv.in_c_off, o.conv.in_c_total, o.conv.out_c_off, o.conv.out_c_total = d.in_c_off, d.in_c_total, d.out_c_off, d.out_c_total


class OpTable(object):
    """The _lib.Op records of an executor's plan at n samples per launch, and the tensors they index (`params`).  The order of the
    table is part of the encoding: the scratch buffers `bufs` (their index = the plan's buffer number), then per layer list
    kernel and bias of conv_layers, of dense_layers, gamma / beta / moving mean / moving variance of bn_layers, shift / scale /
    fill of the transform's roles, depthwise kernel / pointwise kernel / bias of sep_layers, the derived kernels and biases."""

    def __init__(self, ex, n, bufs):
        self.ex, self.n = ex, n
        plan, t = ex.plan, ParamTable(bufs)
        self.params = t.tensors
        self.conv = {id(lay): t.add(lay.kernel, lay.bias) for lay in plan.conv_layers}
        self.dense = {id(lay): t.add(lay.kernel, lay.bias) for lay in plan.dense_layers}
        self.bn = {id(lay): t.add(lay.gamma, lay.beta, lay.moving_mean, lay.moving_variance) for lay in plan.bn_layers}
        self.scale = {role: t.add(*st.tensors) for role, st in ex.transform.items() if st is not None}     # float64
        self.sep = {id(lay): t.add(lay.depthwise_kernel, getattr(lay, 'pointwise_kernel', None), lay.bias)
                    for lay in plan.sep_layers}
        self.phase = [t.add(w2, b2) for w2, b2 in ex.phase_buffers()]

    def encode(self):
        plan_ops = self.ex.plan.ops
        arr = (_lib.Op * len(plan_ops))()
        for k, (op, d) in enumerate(zip(plan_ops, self.ex._descriptors())):
            if op.kind not in ROLLOUT_OPS:
                raise RuntimeError('a %r op has no rollout form' % op.kind)
            code, fill = ROLLOUT_OPS[op.kind]
            o = arr[k]
            o.kind, o.src, o.dst, o.w, o.b = code, op.src, op.dst, -1, -1
            o.src2, o.w2 = _lib.BUF_NONE, -1
            o.xs = _lib.Shape4(self.n, *op.xs)
            fill(self, o, op, d)
        return arr

    def _conv(self, o, op, d):
        o.w, o.b = conv_indices(self, op)
        o.conv = d
        o.aux[0] = self.ex._conv_dtype(op)
        if op.lstm_f:                          # cell update in the epilogue: z_add | NONE, c_prev | NONE, c_out
            za, cp, co = op.aux
            o.aux[1], o.aux[2], o.aux[3] = _or_none(za), _or_none(cp), co
        if op.src2 is not None:                # a whole step: the input convolution rides along
            w_in, b_in = self.conv[id(op.src2['layer'])]
            o.src2, o.w2, o.xs2_c = op.src2['buf'], w_in, op.src2['xs'][0]
            o.conv2 = self.ex._descriptor2(op)
            o.b = b_in                         # the layer's bias belongs to its input convolution

    def _rowconv(self, o, op, d):
        """RowConnected2D: float32 buffers, per-row weights as stored"""
        o.w, o.b = self.conv[id(op.layer)]
        o.conv = d
        o.aux[0] = _lib.F32

    def _derive_weights(self, o, op, d):
        """kernel -> derived kernel, once at the head of the graph: src / b = the layer's kernel / bias, dst / aux[0] = the derived
        ones; a Conv2D(strides=2) restates no bias"""
        (w, b), (w2, b2) = self.conv[id(op.layer)], self.phase[op.wparam]
        if op.kind == 'sphasew':
            b = b2 = -1
        o.src, o.b, o.dst = w, b, w2
        o.aux[0] = b2 if b2 >= 0 else _lib.BUF_NONE
        o.conv.cout, (o.conv.kh, o.conv.kw) = op.layer.filters, op.layer.kernel_size
        if op.kind == 'phasew':
            o.conv.halo.top, o.conv.halo.left = op.halo.top, op.halo.left
        else:
            o.aux[1], o.aux[2] = self.ex.plan.phase_params[op.wparam]['w2_shape'][:2]      # the stored taps
        o.xs = _lib.Shape4(self.n, op.xs[0], 1, 1)

    def _d2s(self, o, op, d):
        o.conv.out_c_off, o.conv.out_c_total = op.out_c_off, op.out_c_total

    def _d2sc(self, o, op, d):
        """the cropping interleave: aux = top, left, out_h, out_w"""
        o.conv.out_c_off, o.conv.out_c_total = op.out_c_off, op.out_c_total
        o.aux[0], o.aux[1], o.aux[2], o.aux[3] = op.crop[0], op.crop[1], op.out_shape[1], op.out_shape[2]

    def _crop(self, o, op, d):
        o.pad = d

    def _dwconv(self, o, op, d):
        """the depthwise stencil: conv = taps, dilation, halo, act, windows; aux[0] = dm"""
        dk, pk, bi = self.sep[id(op.layer)]
        o.w, o.b = dk, (bi if pk < 0 else -1)      # (the bias of a SeparableConv2D belongs to its pointwise stage)
        o.conv.kh, o.conv.kw, o.conv.dil_h, o.conv.dil_w = d.kh, d.kw, d.dil_h, d.dil_w
        o.conv.halo, o.conv.act = d.halo, d.act
        _windows(o, d)
        o.aux[0] = d.depth_multiplier

    def _pwconv(self, o, op, d):
        """the 1 x 1 product: conv = cout, act, windows"""
        dk, o.w, o.b = self.sep[id(op.layer)]
        o.conv.cout, o.conv.act = d.o, d.act
        _windows(o, d)

    def _s2dp(self, o, op, d):
        """the padded space-to-depth: pad = the halo, aux = hp, wp"""
        o.pad = d
        o.conv.in_c_off, o.conv.in_c_total = op.in_c_off, op.in_c_total
        o.aux[0], o.aux[1] = op.out_shape[1], op.out_shape[2]

    def _dense(self, o, op, d):
        o.w, o.b = self.dense[id(op.layer)]
        o.conv.cout, o.conv.act = op.layer.units, op.act

    def _bn(self, o, op, d):
        """inference form: the moving statistics, read at every launch"""
        o.w, o.b, o.aux[0], o.aux[1] = self.bn[id(op.layer)]
        o.aux[2] = _f32_bits(op.layer.epsilon)

    def _act(self, o, op, d):
        """the kind, and alpha / max_value / theta as float bits"""
        a = ops.activation_desc(*op.layer.eltwise)
        o.conv.act = a.kind
        o.aux[0], o.aux[1], o.aux[2] = _f32_bits(a.alpha), _f32_bits(a.max_value), _f32_bits(a.theta)

    def _merge(self, o, op, d):
        """the other sources ride in aux"""
        o.conv.act = ops.MERGE_KINDS[op.layer.kind]
        for j in range(3):
            o.aux[j] = op.aux[j] if j < len(op.aux) else _lib.BUF_NONE

    def _scale(self, o, op, d):
        """float64 parameters, read at every launch; the fill on the input side only"""
        o.w, o.b, fill = self.scale[op.role]
        o.aux[0] = fill if (fill >= 0 and op.role == 'head') else _lib.BUF_NONE
        o.aux[1] = ops.SCALE_KINDS[self.ex.transform[op.role].kind]
        o.aux[2] = 0 if op.role == 'head' else 1

    def _resample(self, o, op, d):
        o.aux[0] = _lib.BF16 if op.src in self.ex._bf16 else _lib.F32

    def _upsample(self, o, op, d):
        pass

    def _pad(self, o, op, d):
        o.pad = d
        if op.inner > 1:
            o.xs = _lib.Shape4(self.n, 1, op.xs[1], op.xs[2])
            o.conv.in_c_total = op.inner

    def _copy(self, o, op, d):
        _windows(o, op)

    def _lstm(self, o, op, d):
        zh, cp, co = op.aux
        bf16 = self.ex._bf16
        o.aux[0], o.aux[1], o.aux[2] = _or_none(zh), _or_none(cp), co
        o.aux[3] = op.rec_act + (256 if op.dst in bf16 else 0) + (512 if op.src in bf16 else 0)
        o.conv.act = op.act
        o.conv.out_c_off, o.conv.out_c_total = op.out_c_off, op.out_c_total


#: kind -> (OP_* code of include/dlwp_hip.h, encoder); 'dropout' has no rollout form (inference plans drop the layer)
ROLLOUT_OPS = {'conv': (_lib.OP_CONV2D, OpTable._conv), 'pad': (_lib.OP_PAD2D, OpTable._pad),
               'maxpool': (_lib.OP_MAXPOOL2, OpTable._resample), 'upsample': (_lib.OP_UPSAMPLE2, OpTable._upsample),
               'copy': (_lib.OP_COPYCH, OpTable._copy), 'lstm': (_lib.OP_LSTM_GATES, OpTable._lstm),
               'phasew': (_lib.OP_PHASE_WEIGHTS, OpTable._derive_weights), 'd2s': (_lib.OP_DEPTH2SPACE, OpTable._d2s),
               'rowconv': (_lib.OP_ROWCONV2D, OpTable._rowconv), 'bn': (_lib.OP_BATCHNORM, OpTable._bn),
               'dense': (_lib.OP_DENSE, OpTable._dense), 'scale': (_lib.OP_SCALE, OpTable._scale),
               'act': (_lib.OP_ACTIVATION, OpTable._act), 'merge': (_lib.OP_MERGE, OpTable._merge),
               'avgpool': (_lib.OP_AVGPOOL2, OpTable._resample), 'bilinear': (_lib.OP_BILINEAR2, OpTable._resample),
               'tphasew': (_lib.OP_TCONV_WEIGHTS, OpTable._derive_weights), 'd2sc': (_lib.OP_DEPTH2SPACE_CROP, OpTable._d2sc),
               'crop': (_lib.OP_CROP2D, OpTable._crop), 'sphasew': (_lib.OP_SCONV_WEIGHTS, OpTable._derive_weights),
               's2dp': (_lib.OP_SPACE2DEPTH_PAD, OpTable._s2dp), 'dwconv': (_lib.OP_DEPTHWISE2D, OpTable._dwconv),
               'pwconv': (_lib.OP_POINTWISE2D, OpTable._pwconv)}
