"""
Lowering of a layer graph to fused libdlwp_hip.so launches.

The reference executes every layer as its own TF op and materialises 3 padded copies in front of each convolution
(SURVEY.md 3.4).  Here padding, pooling, up-sampling and channel slicing are *lazy*: they only edit a `View` (which
stored buffer, which channel window, which loader transform, which halo).  A Conv2D consumes the view in one fused kernel
(dlwp_conv2d_fwd).  Only when a view reaches a consumer that cannot fuse it (a model output, a concatenate, a second
pad on the same axis with another mode, ...) is it materialised with the standalone kernels.

A plan is pure host data (no device access): it can be built and inspected on a machine without a GPU.
"""
import collections
import os

import numpy as np

from . import layers as L

PAD_ZERO, PAD_WRAP, PAD_EDGE, PAD_REFLECT, PAD_SYMMETRIC = 0, 1, 2, 3, 4
SRC_DIRECT, SRC_UPSAMPLE2, SRC_MAXPOOL2 = 0, 1, 2
ACT = {'linear': 0, None: 0, 'tanh': 1, 'relu': 2}
STATE_IN = -1


def OUT(o):
    return -2 - o


Halo = collections.namedtuple('Halo', 'top bottom left right mode_h mode_w')
NO_HALO = Halo(0, 0, 0, 0, PAD_ZERO, PAD_ZERO)


class View(object):
    """Lazy value of a symbolic NCHW tensor: pad(src_transform(buffer[:, c_off:c_off+c]))."""
    __slots__ = ('buf', 'c_off', 'c', 'c_total', 'h', 'w', 'src_mode', 'halo', 'shape')

    def __init__(self, buf, c_off, c, c_total, h, w, src_mode=SRC_DIRECT, halo=NO_HALO, shape=None):
        self.buf, self.c_off, self.c, self.c_total, self.h, self.w = buf, c_off, c, c_total, h, w
        self.src_mode, self.halo = src_mode, halo
        self.shape = shape      # logical per-sample shape when it is not (c, H, W) (after a Reshape)

    def copy(self, **kw):
        v = View(self.buf, self.c_off, self.c, self.c_total, self.h, self.w, self.src_mode, self.halo, self.shape)
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    @property
    def src_hw(self):
        f = {SRC_DIRECT: lambda d: d, SRC_UPSAMPLE2: lambda d: 2 * d, SRC_MAXPOOL2: lambda d: d // 2}[self.src_mode]
        return f(self.h), f(self.w)

    @property
    def logical(self):
        h, w = self.src_hw
        return (self.c, h + self.halo.top + self.halo.bottom, w + self.halo.left + self.halo.right)

    @property
    def plain(self):
        return self.src_mode == SRC_DIRECT and self.halo == NO_HALO

    @property
    def full(self):
        return self.plain and self.c_off == 0 and self.c == self.c_total


class PlanOp(object):
    """One launch.  kind in {'conv','rowconv','pad','maxpool','avgpool','upsample','bilinear','copy','lstm','phasew','d2s','bn',
    'dense','dropout','scale','act','merge','tphasew','d2sc','crop','sphasew','s2dp','dwconv','pwconv'}."""

    def __init__(self, kind, src, dst, xs, **kw):
        self.kind, self.src, self.dst = kind, src, dst
        self.xs = tuple(xs)                 # per-sample (c, h, w) of the stored input this op reads
        self.layer = kw.pop('layer', None)  # Conv2D layer owning the weights
        self.halo = kw.pop('halo', NO_HALO)
        self.src_mode = kw.pop('src_mode', SRC_DIRECT)
        self.act = kw.pop('act', 0)
        self.in_c_off = kw.pop('in_c_off', 0)
        self.in_c_total = kw.pop('in_c_total', 0)
        self.out_c_off = kw.pop('out_c_off', 0)
        self.out_c_total = kw.pop('out_c_total', 0)
        self.inner = kw.pop('inner', 1)     # pad only: 1 = NCHW rows, C = NHWC
        self.out_shape = kw.pop('out_shape', None)   # per-sample (c, h, w) this op produces (window it writes)
        # lstm only: src = zx buffer, dst = h buffer; aux = (zh buffer | None, c_prev buffer | None, c_out buffer)
        # merge only: src = the first source, aux = the buffers of the other sources (1 to 3), all read as whole flat tensors
        self.aux = kw.pop('aux', None)
        self.out_pool = kw.pop('out_pool', False)   # conv only: MaxPooling2D(2) applied in the epilogue (inference plans)
        self.out_d2s = kw.pop('out_d2s', False)     # conv only: the 4 F phase channels stored interleaved (inference plans)
        self.rec_act = kw.pop('rec_act', 0)
        # conv with the ConvLSTM2D cell update in its epilogue (bfloat16 inference plans): lstm_f = F hidden channels, dst = the h
        # buffer, aux = (z_add buffer | None, c_prev buffer | None, c_out buffer), act / rec_act = the cell's activations
        self.lstm_f = kw.pop('lstm_f', 0)
        # ... and a WHOLE step in one launch (dlwp_convlstm_step_fwd; octet layout): this op is the recurrent convolution, src2
        # describes the input convolution of the same step: {'buf', 'xs' (c, h, w), 'layer', 'halo', 'in_c_off', 'in_c_total'}
        self.src2 = kw.pop('src2', None)
        # conv restated on a low-resolution source (inference plans; build_plan): geometry that overrides the layer's
        self.dil = kw.pop('dil', None)            # dilation (dh, dw)
        self.ksize = kw.pop('ksize', None)        # kernel size (kh, kw)
        self.filters = kw.pop('filters', None)    # output channels
        self.wparam = kw.pop('wparam', None)      # index into plan.phase_params: derived kernel / bias instead of the layer's
        self.alg_flops = kw.pop('alg_flops', None)   # algorithmic FLOPs per sample of the ORIGINAL layer
        # scale only (inference plans with an input / output transform): 'head' = imputer + scaler transform of the model input,
        # 'tail' = the scaler's inverse transform of the model output; the executor holds the parameters
        self.role = kw.pop('role', None)
        # d2sc only (the cropping interleave of a Conv2DTranspose): (top, left) of the window [top, +ho) x [left, +wo) it takes of
        # the depth-to-space image of its source; layer / act = the layer's, for the backward (bias gradient at full resolution)
        self.crop = kw.pop('crop', None)
        # conv of a Conv2D(strides=2) only: its source is the space-to-depth image of the MODEL INPUT (the 's2dp' op in front reads
        # STATE_IN), so nobody needs the gradient of that source: the backward pass launches no data gradient
        self.input_image = kw.pop('input_image', False)
        # conv only: per-sample (c, h, w) the convolution COMPUTES where that is not what it stores (out_pool: the pre-pooling tensor,
        # out_d2s: the 4 F phase channels); None = out_shape.  FLOP accounting reads it (conv_flops_per_sample, bench.py)
        self.conv_out_shape = kw.pop('conv_out_shape', None)
        assert not kw, kw

    @property
    def conv_geometry(self):
        """(filters, (kh, kw), (dh, dw)) this conv launch runs with."""
        lay = self.layer
        return (self.filters or lay.filters, tuple(self.ksize or lay.kernel_size), tuple(self.dil or lay.dilation_rate))

    def __repr__(self):
        extra = ''
        if self.kind == 'lstm':
            extra = ' aux%r h[%d:+%d/%d] act%d rec%d' % (self.aux, self.out_c_off, self.xs[0], self.out_c_total, self.act,
                                                        self.rec_act)
        if self.kind in ('conv', 'rowconv'):
            f, ks, dil = self.conv_geometry
            extra = ' %s k%s d%s src%d halo%s act%d cin[%d:+%d/%d] cout[%d:+%d/%d]%s%s' % (
                self.layer.name, ks, dil, self.src_mode, tuple(self.halo),
                self.act, self.in_c_off, self.xs[0], self.in_c_total, self.out_c_off, f,
                self.out_c_total, ' +pool' if self.out_pool else '', ' phase-kernels' if self.wparam is not None else '')
            if self.lstm_f:
                extra += ' +cell-update F=%d aux%r rec%d' % (self.lstm_f, self.aux, self.rec_act)
        if self.kind == 'act':
            extra = ' %s %r' % (self.layer.name, self.layer.eltwise)
        if self.kind == 'merge':
            extra = ' %s %s%r' % (self.layer.name, self.layer.kind, (self.src,) + tuple(self.aux))
        if self.kind == 'd2sc':
            extra = ' %s crop%r -> %r' % (self.layer.name, tuple(self.crop), tuple(self.out_shape))
        if self.kind == 'crop':
            extra = ' crop%r' % (tuple(self.halo[:4]),)
        if self.kind == 's2dp':
            extra = ' halo%s cin[%d:+%d/%d] -> %r' % (tuple(self.halo), self.in_c_off, self.xs[0], self.in_c_total,
                                                     tuple(self.out_shape))
        if self.kind in ('dwconv', 'pwconv'):
            extra = ' %s halo%s act%d cin[%d:+%d/%d] -> %r' % (self.layer.name, tuple(self.halo), self.act, self.in_c_off, self.xs[0],
                                                              self.in_c_total, tuple(self.out_shape))
        return '<%s %s -> %s xs=%s%s>' % (self.kind, self.src, self.dst, self.xs, extra)


class Plan(object):
    def __init__(self):
        self.ops = []
        self.buffers = []        # per-sample (c_total, h, w) of each scratch buffer; index = buffer id
        self.input_shape = None  # per-sample
        self.output_shapes = []  # per-sample logical shapes of the model outputs
        self.output_store = []   # per-sample stored (c, h, w) of each output slot
        self.conv_layers = []    # unique Conv2D layers in first-use order
        # derived kernels ('phasew' / 'tphasew' / 'sphasew' ops; _PlanBuilder.derived_kernel): dicts layer, w2_shape, bias (bool: a
        # derived bias too) + either pad_top, pad_left (an up-sampled Conv2D) or kind in {'tconv', 'sconv'}
        self.phase_params = []
        self.bn_layers = []      # BatchNormalization layers in plan order (one 'bn' op each)
        self.dense_layers = []   # Dense layers in plan order (one 'dense' op each)
        self.dropout_layers = [] # Dropout layers in graph order (training plans: one 'dropout' op each; its index keys the mask)
        self.eltwise_layers = [] # activation / merge layers with a launch, in first-use order (stateless: any number of ops each)
        self.sep_layers = []     # DepthwiseConv2D / SeparableConv2D layers in plan order (one 'dwconv' (+ one 'pwconv') op each)

    def new_buffer(self, c, h, w):
        self.buffers.append((int(c), int(h), int(w)))
        return len(self.buffers) - 1

    def buffer_shape(self, buf):
        if buf == STATE_IN:
            return self._in_store
        if buf <= -2:
            return self.output_store[-2 - buf]
        return self.buffers[buf]

    @property
    def n_launches(self):
        return len(self.ops)

    def conv_flops_per_sample(self):
        """sum over conv ops of 2*Ho*Wo*Cout*Cin*kh*kw."""
        tot = 0
        for op in self.ops:
            if op.kind in ('conv', 'rowconv'):
                if op.alg_flops is not None:
                    tot += op.alg_flops
                    continue
                kh, kw = op.layer.kernel_size
                co, ho, wo = op.conv_out_shape or op.out_shape
                tot += 2 * ho * wo * co * op.xs[0] * kh * kw
                if op.src2 is not None:          # a whole ConvLSTM2D step: the input convolution's share
                    k2 = op.src2['layer'].kernel_size
                    tot += 2 * ho * wo * 4 * op.lstm_f * op.src2['xs'][0] * k2[0] * k2[1]
        return tot

    def algorithmic_bytes_per_sample(self, itemsize=4):
        """fused-forward algorithmic bytes: sum over launches of (input window + output window) + weights once."""
        tot = 0
        for op in self.ops:
            c, h, w = op.xs
            tot += c * h * w * itemsize * (1 + len(op.aux) if op.kind == 'merge' else 1)
            co, ho, wo = op.out_shape
            tot += co * ho * wo * itemsize
        for lay in self.conv_layers:
            if lay.kernel is not None:
                tot += (int(np.prod(lay.kernel.shape)) + (int(np.prod(lay.bias.shape)) if lay.bias is not None else 0)) * itemsize
        return tot

    def bf16_buffers(self):
        """Scratch buffers that may be stored as bfloat16 (config 4: bf16 activations between the layers): written by a
        convolution (Conv2D output, ConvLSTM2D gate pre-activations), by the ConvLSTM2D cell update (the h sequence) or
        by a max- or average-pooling or a bilinear up-sampling of such a buffer, and read only by convolutions / pooling /
        bilinear up-sampling / the cell update.  Model inputs and outputs, the ConvLSTM2D cell state, and anything a copy / pad /
        nearest up-sampling kernel touches stay float32."""
        ok = {}
        for op in self.ops:
            for b, role in ((op.src, 'r'), (op.dst, 'w')):
                if b >= 0:
                    ok[b] = ok.get(b, True) and op.kind in ('conv', 'maxpool', 'avgpool', 'bilinear', 'lstm') and not (role == 'w' and op.out_d2s)
            if op.kind == 'merge':                                                # (float32 kernels)
                for b in op.aux:
                    if b >= 0:
                        ok[b] = False
            if op.kind == 'lstm' or (op.kind == 'conv' and op.lstm_f):
                zh, cp, co = op.aux
                for b in (cp, co):                                                # the cell state stays float32
                    if b is not None and b >= 0:
                        ok[b] = False
                if op.kind == 'conv' and zh is not None and zh >= 0:             # (read by this convolution's epilogue)
                    ok[zh] = ok.get(zh, True)
        for op in self.ops:                                                       # zx and zh of a step: the same type
            if op.kind == 'lstm' and op.aux[0] is not None and op.src >= 0 and op.aux[0] >= 0:
                both = ok.get(op.src, False) and ok.get(op.aux[0], False)
                ok[op.src] = ok[op.aux[0]] = both
        changed = True
        while changed:                  # a pooled / interpolated copy is bf16 only if its source is (and vice versa)
            changed = False
            for op in self.ops:
                if op.kind in ('maxpool', 'avgpool', 'bilinear') and op.src >= 0 and op.dst >= 0 and ok.get(op.src, False) != ok.get(op.dst, False):
                    ok[op.src] = ok[op.dst] = False
                    changed = True
                if op.kind in ('maxpool', 'avgpool', 'bilinear') and (op.src < 0 or op.dst < 0):
                    for b in (op.src, op.dst):
                        if b >= 0 and ok.get(b, False):
                            ok[b] = False
                            changed = True
        return sorted(b for b, v in ok.items() if v)

    def describe(self):
        return '\n'.join(repr(op) for op in self.ops)


def _compose_halo(first, layer_pad, mode):
    """Halo after applying a padding layer (pads ((t,b),(l,r)), `mode`) on top of an existing lazy halo.
    Returns None when the two do not compose into one per-axis mode (caller materialises first)."""
    (t, b), (l, r) = layer_pad

    def axis(lo0, hi0, m0, lo1, hi1):
        if lo1 == 0 and hi1 == 0:
            return lo0, hi0, m0
        if lo0 == 0 and hi0 == 0:
            return lo1, hi1, mode
        if m0 == mode and mode in (PAD_ZERO, PAD_EDGE):
            return lo0 + lo1, hi0 + hi1, mode       # zero-of-zero / edge-of-edge extend; wrap-of-wrap does not
        return None
    ah = axis(first.top, first.bottom, first.mode_h, t, b)
    aw = axis(first.left, first.right, first.mode_w, l, r)
    if ah is None or aw is None:
        return None
    return Halo(ah[0], ah[1], aw[0], aw[1], ah[2], aw[2])


def _prefers_unfused_pool(cin, lay):
    """Ask the library (host logic only, works without a GPU) whether a pooled source should be materialised for this
    convolution; False when the library is not built."""
    try:
        from . import ops
        return ops.prefers_unfused_pool(cin, lay.filters, lay.kernel_size[0], lay.kernel_size[1],
                                        lay.dilation_rate[0], lay.dilation_rate[1])
    except (ImportError, OSError, AttributeError):
        return False


# Inference plans restate a Conv2D that reads a 2x up-sampled tensor on the low-resolution tensor (see build_plan).
# DLWP_RESTATE_UPSAMPLED=0 keeps the reference's own formulation (the fused up-sampling loader) for A/B comparisons.
RESTATE_UPSAMPLED = os.environ.get('DLWP_RESTATE_UPSAMPLED', '1') != '0'


def _phase_geometry(k, pad):
    """(k2, lo, hi): the distinct source offsets [lo, hi] the k taps of an axis reach on a 2x up-sampled tensor with a
    top / left halo of `pad` (csrc/phase.hip: dlwp_phase_geometry; ops.phase_geometry is this function)."""
    offs = [(a + u - pad) // 2 for a in (0, 1) for u in range(k)]
    return max(offs) - min(offs) + 1, min(offs), max(offs)


def tconv_taps(th, tw):
    """(sh, sw): the taps the derived kernel of a Conv2DTranspose is STORED with -- 3 x 3 where T <= 3 (k <= 6), 5 x 5 where
    T <= 5 (k <= 10): the sizes the matrix-core forward and weight-gradient kernels exist for (csrc/tconv.hip); T itself beyond that
    (the forward then runs on the direct kernel and there is no weight gradient).  DLWP_TCONV_TAPS=exact keeps T x T (A/B runs of
    the forward)."""
    t = max(int(th), int(tw))
    if os.environ.get('DLWP_TCONV_TAPS') == 'exact' or t > 5:
        return int(th), int(tw)
    return (3, 3) if t <= 3 else (5, 5)


def toposort(outputs):
    order, seen = [], set()

    def visit(t):
        if t.uid in seen:
            return
        seen.add(t.uid)
        for i in t.inputs:
            visit(i)
        order.append(t)
    for o in outputs:
        visit(o)
    return order


def _supports_out_pool(op):
    try:
        from . import ops
        f, ks, dil = op.conv_geometry
        cd = ops.make_conv(f, ks[0], ks[1], dil, ops.make_pad(*op.halo),
                           op.act, op.in_c_off, op.in_c_total, op.out_c_off, op.out_c_total, op.src_mode)
        return ops.supports_out_pool(op.xs, cd)
    except (ImportError, OSError, AttributeError):
        return False


def _supports_out_d2s(xs, f4, ks, halo, act, in_c_off, in_c_total):
    """can the restated layer's convolution store its 4 F phase channels interleaved (dlwp_conv2d.out_d2s)?"""
    try:
        from . import ops
        cd = ops.make_conv(f4, ks[0], ks[1], 1, ops.make_pad(*halo), act, in_c_off, in_c_total, 0, 0, SRC_DIRECT)
        return ops.supports_out_d2s(xs, cd)
    except (ImportError, OSError, AttributeError):
        return False


def _supports_lstm_conv(xs, part, halo, src_mode, act, rec_act, f, in_c_off, in_c_total, out_c_off, out_c_total, in_bf16):
    """can this convolution of a ConvLSTM2D step carry the cell update in its epilogue (dlwp_convlstm_conv_fwd)?"""
    try:
        from . import ops
        cd = ops.make_conv(4 * f, part.kernel_size[0], part.kernel_size[1], tuple(part.dilation_rate), ops.make_pad(*halo), act,
                           in_c_off, in_c_total, out_c_off, out_c_total, src_mode, lstm_f=f, lstm_rec_act=rec_act)
        return ops.convlstm_conv_supported(xs, cd, in_bf16, compute_bf16=not in_bf16)
    except (ImportError, OSError, AttributeError):
        return False


def _supports_lstm_step(lay, f, ho, wo, t_len, cin, v, halo, act, rec_act):
    """can ONE launch run a step t >= 1 of this ConvLSTM2D (dlwp_convlstm_step_fwd)?"""
    try:
        from . import ops
        ip, rp = lay.input_part, lay.recurrent_part
        rk = ((rp.kernel_size[0] - 1) // 2, (rp.kernel_size[1] - 1) // 2)
        cd_h = ops.make_conv(4 * f, rp.kernel_size[0], rp.kernel_size[1], 1, ops.make_pad(rk[0], rk[0], rk[1], rk[1], 0, 0), act,
                             0, t_len * f, f, t_len * f, SRC_DIRECT, lstm_f=f, lstm_rec_act=rec_act)
        cd_x = ops.make_conv(4 * f, ip.kernel_size[0], ip.kernel_size[1], tuple(ip.dilation_rate), ops.make_pad(*halo), 0,
                             v.c_off + cin, v.c_total, 0, 4 * f, v.src_mode)
        return v.h == ho and v.w == wo and ops.convlstm_step_supported((f, ho, wo), cd_h, (cin, v.h, v.w), cd_x)
    except (ImportError, OSError, AttributeError):
        return False


def _store_of(shape):
    """stored 3-D (c, h, w) block of a logical per-sample shape: everything in front of the last two axes is
    channels (the recurrent (T, C, H, W) layout is (T*C, H, W) in memory).  A rank-1 tensor of F features (Dense models) is
    stored as (F, 1, 1)."""
    if len(shape) == 1:
        return (int(shape[0]), 1, 1)
    if len(shape) < 3:
        raise NotImplementedError('dense (non-convolutional) tensors of per-sample shape %r are not on the HIP path'
                                  % (shape,))
    c = 1
    for d in shape[:-2]:
        c *= d
    return (c, shape[-2], shape[-1])


# what the per-step emitters of a ConvLSTM2D share (_PlanBuilder.lower_convlstm)
_LstmSteps = collections.namedtuple('_LstmSteps', 'lay v halo rhalo cin f ho wo t_len hbuf cbufs zxs zhs act rec')


class _PlanBuilder(object):
    """The state of one build_plan call and one lowering method per layer kind (_LOWERINGS below says which).  A lowering method
    (t, lay, ins, outs) -- the tensor, its layer, the views of its inputs, the output slots it fills -- sets views[t.uid].
    Buffer numbers are part of the contract (the backward pass, bf16_buffers() and the rollout op table index buffers by
    number): the order of the new_buffer calls inside a method must not change."""

    def __init__(self, inputs, outputs, inference, fuse_d2s, fuse_lstm, fuse_lstm_step, head):
        self.inference, self.fuse_d2s, self.fuse_lstm, self.fuse_lstm_step = inference, fuse_d2s, fuse_lstm, fuse_lstm_step
        self.plan = plan = Plan()
        self.x_in = inputs[0]
        plan.input_shape = tuple(self.x_in.shape)
        self.order = toposort(outputs)
        self.consumers = collections.Counter()
        for t in self.order:
            for i in t.inputs:
                self.consumers[i.uid] += 1
        self.out_index = {}
        for o, t in enumerate(outputs):
            self.out_index.setdefault(t.uid, []).append(o)
        plan.output_shapes = [tuple(t.shape) for t in outputs]
        plan.output_store = [None] * len(outputs)
        plan._in_store = _store_of(self.x_in.shape)
        self.views = {}
        self.in_buf = STATE_IN             # what the consumers of the model input read
        if head:
            self.in_buf = plan.new_buffer(*plan._in_store)
            plan.ops.append(PlanOp('scale', STATE_IN, self.in_buf, plan._in_store, role='head', out_shape=plan._in_store))
        self.producer = {}                 # scratch buffer -> the conv op that wrote all of it

    def run(self):
        for t in self.order:
            lay = t.layer
            if isinstance(lay, L.InputLayer):
                if t.uid != self.x_in.uid:
                    raise ValueError('graph reaches an Input that is not the model input')
                c, h, w = self.plan._in_store
                self.views[t.uid] = View(self.in_buf, 0, c, c, h, w, shape=tuple(t.shape) if len(t.shape) != 3 else None)
                continue
            ins = [self.views[i.uid] for i in t.inputs]
            outs = self.out_index.get(t.uid, [])
            for match, lower in _LOWERINGS:
                if isinstance(lay, match) if isinstance(match, type) else match(lay):
                    break
            else:
                raise NotImplementedError('layer %s (%s) has no HIP lowering' % (lay.name, type(lay).__name__))
            lower(self, t, lay, ins, outs)
            self.finish_outputs(t, outs)
        return self.plan

    # -- launches and buffers ---------------------------------------------------------------------------------------------------- #
    def emit(self, op):
        plan, producer = self.plan, self.producer
        plan.ops.append(op)
        if op.kind == 'conv' and op.dst >= 0 and op.out_c_off == 0 and op.out_c_total == op.layer.filters:
            producer[op.dst] = op
        elif op.dst in producer:
            del producer[op.dst]
        if op.kind in ('conv', 'rowconv') and op.layer not in plan.conv_layers:
            plan.conv_layers.append(op.layer)
        return op

    def materialize(self, v, dst=None, dst_c_off=0, dst_c_total=None):
        """Turn a lazy view into real data.  With dst=None a new buffer is created (or the view is returned untouched if
        it is already a whole buffer).  With dst given, the data lands in channels [dst_c_off, +c) of that buffer."""
        plan, emit = self.plan, self.emit
        cur = v
        steps = []
        if not (cur.c_off == 0 and cur.c == cur.c_total) and not cur.plain:
            steps.append('window')      # pool/pad kernels want a dense (n*c) plane run: extract the window first
        if cur.src_mode != SRC_DIRECT:
            steps.append('src')
        if cur.halo != NO_HALO:
            steps.append('halo')
        into_window = dst is not None and not (dst_c_off == 0 and (dst_c_total is None or dst_c_total == v.logical[0]))
        if dst is not None and (not steps or into_window or steps[-1] == 'window'):
            steps.append('final_copy')
        if not steps:
            return cur
        for k, step in enumerate(steps):
            last = k == len(steps) - 1
            tgt_direct = last and dst is not None and step != 'final_copy'
            if step == 'window':
                nb = plan.new_buffer(cur.c, cur.h, cur.w)
                emit(PlanOp('copy', cur.buf, nb, (cur.c, cur.h, cur.w), in_c_off=cur.c_off, in_c_total=cur.c_total,
                            out_c_off=0, out_c_total=cur.c, out_shape=(cur.c, cur.h, cur.w)))
                cur = cur.copy(buf=nb, c_off=0, c_total=cur.c)
            elif step == 'src':
                h2, w2 = cur.src_hw
                nb = dst if tgt_direct else plan.new_buffer(cur.c, h2, w2)
                emit(PlanOp('maxpool' if cur.src_mode == SRC_MAXPOOL2 else 'upsample', cur.buf, nb,
                            (cur.c, cur.h, cur.w), out_shape=(cur.c, h2, w2)))
                cur = cur.copy(buf=nb, h=h2, w=w2, src_mode=SRC_DIRECT)
            elif step == 'halo':
                c, hp, wp = cur.logical
                nb = dst if tgt_direct else plan.new_buffer(c, hp, wp)
                emit(PlanOp('pad', cur.buf, nb, (cur.c, cur.h, cur.w), halo=cur.halo, out_shape=(c, hp, wp)))
                cur = cur.copy(buf=nb, h=hp, w=wp, halo=NO_HALO)
            else:  # final_copy
                tot = dst_c_total if dst_c_total is not None else cur.c
                emit(PlanOp('copy', cur.buf, dst, (cur.c, cur.h, cur.w), in_c_off=cur.c_off, in_c_total=cur.c_total,
                            out_c_off=dst_c_off, out_c_total=tot, out_shape=(cur.c, cur.h, cur.w)))
                cur = View(dst, dst_c_off, cur.c, tot, cur.h, cur.w)
        return cur

    # -- the idioms the lowerings share ------------------------------------------------------------------------------------------ #
    def out_or_new(self, outs, shape):
        """where a layer's launch writes: the model's output slot when the tensor is a model output (the slot's stored shape is
        recorded), a new scratch buffer otherwise"""
        if outs:
            self.plan.output_store[outs[0]] = shape
            return OUT(outs[0])
        return self.plan.new_buffer(*shape)

    def whole(self, v):
        """the view as a whole stored buffer: anything lazy in front is materialised, a channel window is extracted"""
        v = self.materialize(v)
        if not v.full:
            v = self.materialize(v, dst=self.plan.new_buffer(*v.logical))
        return v

    def with_zero_halo(self, v, pads):
        """(v, halo): a layer's own zero halo ((t, b), (l, r)) composed with the lazy halo of its input; where the two do not
        compose, the input is materialised and the halo starts afresh"""
        halo = _compose_halo(v.halo, pads, PAD_ZERO)
        if halo is None:
            v = self.materialize(v)
            halo = Halo(pads[0][0], pads[0][1], pads[1][0], pads[1][1], PAD_ZERO, PAD_ZERO)
        return v, halo

    @staticmethod
    def check_wrap(lay, halo, hh, ww):
        if halo.mode_h == PAD_WRAP and max(halo.top, halo.bottom) > hh:
            raise ValueError('%s: periodic row padding exceeds the input height %d' % (lay.name, hh))
        if halo.mode_w == PAD_WRAP and max(halo.left, halo.right) > ww:
            raise ValueError('%s: periodic column padding exceeds the input width %d' % (lay.name, ww))

    def derived_kernel(self, op_kind, lay, cin, w2_shape, bias, halo=NO_HALO, **entry):
        """A convolution restated on a derived kernel: the plan.phase_params entry and the op that fills it ('phasew' / 'tphasew' /
        'sphasew'); returns the entry's index, the wparam of the convolution"""
        pidx = len(self.plan.phase_params)
        self.plan.phase_params.append(dict({'layer': lay, 'w2_shape': w2_shape, 'bias': bias}, **entry))
        self.emit(PlanOp(op_kind, STATE_IN, STATE_IN, (cin, 0, 0), layer=lay, wparam=pidx, halo=halo, out_shape=(0, 0, 0)))
        return pidx

    def phase_conv(self, lay, v, outs, halo, taps, pidx, alg, phase_hw, out_hw, crop=None):
        """The tail of a layer restated as ONE convolution with 4 x filters phase channels on derived kernels: the convolution
        stores the phases interleaved itself (out_d2s: inference plans, where a kernel can and nothing is cropped) or writes a
        temporary that 'd2s' (crop=None: an up-sampled Conv2D) / 'd2sc' (crop=(top, left): a Conv2DTranspose) interleaves.
        Returns the destination.  The destination is allocated in front of the temporary (buffer numbers: see the class)."""
        f, (hp, wp), (ho, wo), act = lay.filters, phase_hw, out_hw, ACT[lay.activation]
        dst = self.out_or_new(outs, (f, ho, wo))
        no_crop = crop is None or (crop[0] == 0 and crop[1] == 0 and ho == 2 * hp and wo == 2 * wp)
        fold = (self.inference and self.fuse_d2s and no_crop and
                _supports_out_d2s((v.c, v.h, v.w), 4 * f, taps, halo, act, v.c_off, v.c_total))
        conv = dict(layer=lay, halo=halo, src_mode=SRC_DIRECT, act=act, in_c_off=v.c_off, in_c_total=v.c_total, out_c_off=0,
                    dil=(1, 1), ksize=taps, filters=4 * f, wparam=pidx, alg_flops=alg)
        if fold:                 # the convolution's epilogue stores the phases interleaved: no interleave pass
            self.emit(PlanOp('conv', v.buf, dst, (v.c, v.h, v.w), out_c_total=f, out_shape=(f, ho, wo), out_d2s=True,
                             conv_out_shape=(4 * f, hp, wp), **conv))
            return dst
        tmp = self.plan.new_buffer(4 * f, hp, wp)
        self.emit(PlanOp('conv', v.buf, tmp, (v.c, v.h, v.w), out_c_total=4 * f, out_shape=(4 * f, hp, wp), **conv))
        if crop is None:
            self.emit(PlanOp('d2s', tmp, dst, (f, hp, wp), out_c_off=0, out_c_total=f, out_shape=(f, ho, wo)))
        else:
            self.emit(PlanOp('d2sc', tmp, dst, (f, hp, wp), layer=lay, act=act, crop=crop, out_c_off=0, out_c_total=f,
                             out_shape=(f, ho, wo)))
        return dst

    # -- one method per row of _LOWERINGS ---------------------------------------------------------------------------------------- #
    def lower_pad2d(self, t, lay, ins, outs):
        plan = self.plan
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('%s on a reshaped (non-3D) tensor' % lay.name)
        if lay.data_format == 'channels_last':
            # standalone only: buffer holds (H, W, C) per sample, rows of W*C floats
            v = self.materialize(v)
            hh, ww, cc = t.inputs[0].shape
            (tp, bt), (lf, rt) = lay.padding
            nb = plan.new_buffer(hh + tp + bt, ww + lf + rt, cc)
            self.emit(PlanOp('pad', v.buf, nb, (1, hh, ww), halo=Halo(tp, bt, lf, rt, lay.mode, lay.mode), inner=cc,
                             out_shape=(hh + tp + bt, ww + lf + rt, cc)))
            self.views[t.uid] = View(nb, 0, hh + tp + bt, hh + tp + bt, ww + lf + rt, cc)
            self.views[t.uid].shape = tuple(t.shape)
        else:
            halo = _compose_halo(v.halo, lay.padding, lay.mode)
            if halo is None:
                v = self.materialize(v)
                halo = _compose_halo(NO_HALO, lay.padding, lay.mode)
            self.check_wrap(lay, halo, *v.src_hw)
            self.views[t.uid] = v.copy(halo=halo)

    def lower_pad3d(self, t, lay, ins, outs):
        # (T, C, H, W) stored as (T*C, H, W): a 3-D pad that leaves the first (channel) axis alone is the 2-D halo
        v = ins[0]
        if lay.data_format != 'channels_first':
            raise NotImplementedError("%s: data_format='channels_first' is required" % lay.name)
        if lay.padding[0] != (0, 0):
            raise NotImplementedError('%s: padding of the first (channel) axis %r is not lowered to the HIP path'
                                      % (lay.name, lay.padding[0]))
        pad2 = (lay.padding[1], lay.padding[2])
        halo = _compose_halo(v.halo, pad2, lay.mode)
        if halo is None:
            shp = v.shape
            v = self.materialize(v)
            v.shape = shp
            halo = _compose_halo(NO_HALO, pad2, lay.mode)
        self.check_wrap(lay, halo, *v.src_hw)
        self.views[t.uid] = v.copy(halo=halo, shape=tuple(t.shape))

    def lower_convlstm(self, t, lay, ins, outs):
        """geometry, buffers and which launches run a step; the steps themselves: lstm_step_plain / _fused / _whole"""
        plan = self.plan
        v = ins[0]
        t_len, cin = t.inputs[0].shape[0], t.inputs[0].shape[1]
        if v.c != t_len * cin:
            raise ValueError('%s: input view has %d channels, expected T*C = %d' % (lay.name, v.c, t_len * cin))
        halo = v.halo
        if lay.padding == 'same':
            st, sb, sl, sr = lay.same_halo()
            v, halo = self.with_zero_halo(v, ((st, sb), (sl, sr)))
        _, hl, wl = v.copy(halo=halo).logical
        ho = hl - lay.dilation_rate[0] * (lay.kernel_size[0] - 1)
        wo = wl - lay.dilation_rate[1] * (lay.kernel_size[1] - 1)
        f = lay.filters
        hbuf = plan.new_buffer(t_len * f, ho, wo)           # h_0 .. h_{T-1}, the return_sequences output
        # every step keeps its own pre-activations and cell state: they are the saved activations of the backward
        # pass (dlwp_convlstm_gates_bwd) -- T is the reference's time_dim (2), so this costs little
        cbufs = [plan.new_buffer(f, ho, wo) for _ in range(t_len)]
        rk = ((lay.kernel_size[0] - 1) // 2, (lay.kernel_size[1] - 1) // 2)
        act, rec_code = ACT[lay.activation], {'hard_sigmoid': 0, 'sigmoid': 1}[lay.recurrent_activation]
        rhalo = Halo(rk[0], rk[0], rk[1], rk[1], PAD_ZERO, PAD_ZERO)
        # bfloat16 inference: the convolution that completes a step's pre-activations applies the cell update in its
        # epilogue (the input convolution on the first step, the recurrent one afterwards): z_h (z_x on the first step)
        # is never stored and the gate kernel disappears.  The model input feeds the input convolution as float32.
        fused = (self.inference and self.fuse_lstm and v.buf == STATE_IN and
                 _supports_lstm_conv((cin, v.h, v.w), lay.input_part, halo, v.src_mode, act, rec_code, f,
                                     v.c_off, v.c_total, 0, t_len * f, False) and
                 (t_len == 1 or _supports_lstm_conv((f, ho, wo), lay.recurrent_part, rhalo, SRC_DIRECT, act,
                                                    rec_code, f, 0, t_len * f, f, t_len * f, True)))
        # ... and every later step as ONE launch where the library has the dual-source instance (octet layout; the executor
        # falls back to the two launches when it cannot keep the h sequence in octets)
        whole = (fused and self.fuse_lstm_step and t_len > 1 and os.environ.get('DLWP_LSTM_STEP', '1') != '0' and
                 _supports_lstm_step(lay, f, ho, wo, t_len, cin, v, halo, act, rec_code))
        zxs = [None if (fused and (step == 0 or whole)) else plan.new_buffer(4 * f, ho, wo) for step in range(t_len)]
        zhs = [None] + [None if fused else plan.new_buffer(4 * f, ho, wo) for _ in range(t_len - 1)]
        g = _LstmSteps(lay, v, halo, rhalo, cin, f, ho, wo, t_len, hbuf, cbufs, zxs, zhs, act, rec_code)
        for step in range(t_len):
            if not fused:
                self.lstm_step_plain(g, step)
            elif whole and step > 0:
                self.lstm_step_whole(g, step)
            else:
                self.lstm_step_fused(g, step)
        if lay.return_sequences:
            self.views[t.uid] = View(hbuf, 0, t_len * f, t_len * f, ho, wo, shape=(t_len, f, ho, wo))
        else:
            self.views[t.uid] = View(hbuf, (t_len - 1) * f, f, t_len * f, ho, wo)

    def lstm_input_conv(self, g, step):
        """z_x of a step: the input convolution into the step's own pre-activation buffer"""
        v, f = g.v, g.f
        self.emit(PlanOp('conv', v.buf, g.zxs[step], (g.cin, v.h, v.w), layer=g.lay.input_part, halo=g.halo,
                         src_mode=v.src_mode, act=0, in_c_off=v.c_off + step * g.cin, in_c_total=v.c_total, out_c_off=0,
                         out_c_total=4 * f, out_shape=(4 * f, g.ho, g.wo)))

    def lstm_step_plain(self, g, step):
        """z_x, z_h (from the second step on) and the gate kernel"""
        f, ho, wo, t_len = g.f, g.ho, g.wo, g.t_len
        self.lstm_input_conv(g, step)
        if step > 0:
            self.emit(PlanOp('conv', g.hbuf, g.zhs[step], (f, ho, wo), layer=g.lay.recurrent_part, halo=g.rhalo,
                             src_mode=SRC_DIRECT, act=0, in_c_off=(step - 1) * f, in_c_total=t_len * f, out_c_off=0,
                             out_c_total=4 * f, out_shape=(4 * f, ho, wo)))
        self.emit(PlanOp('lstm', g.zxs[step], g.hbuf, (f, ho, wo), act=g.act, rec_act=g.rec,
                         aux=(g.zhs[step], g.cbufs[step - 1] if step > 0 else None, g.cbufs[step]),
                         out_c_off=step * f, out_c_total=t_len * f, out_shape=(f, ho, wo)))

    def lstm_step_fused(self, g, step):
        """the cell update in the epilogue of the convolution that completes the pre-activations: the input convolution on the
        first step, the recurrent one (behind a stored z_x) afterwards"""
        v, f, ho, wo, t_len = g.v, g.f, g.ho, g.wo, g.t_len
        if step == 0:
            self.emit(PlanOp('conv', v.buf, g.hbuf, (g.cin, v.h, v.w), layer=g.lay.input_part, halo=g.halo, src_mode=v.src_mode,
                             act=g.act, rec_act=g.rec, lstm_f=f, aux=(None, None, g.cbufs[0]),
                             in_c_off=v.c_off, in_c_total=v.c_total, out_c_off=0, out_c_total=t_len * f,
                             out_shape=(f, ho, wo)))
            return
        self.lstm_input_conv(g, step)
        self.emit(PlanOp('conv', g.hbuf, g.hbuf, (f, ho, wo), layer=g.lay.recurrent_part, halo=g.rhalo, src_mode=SRC_DIRECT,
                         act=g.act, rec_act=g.rec, lstm_f=f, aux=(g.zxs[step], g.cbufs[step - 1], g.cbufs[step]),
                         in_c_off=(step - 1) * f, in_c_total=t_len * f, out_c_off=step * f, out_c_total=t_len * f,
                         out_shape=(f, ho, wo)))

    def lstm_step_whole(self, g, step):
        """a step t >= 1 as ONE launch: the recurrent convolution with the cell update; src2 = the step's input convolution"""
        v, f, ho, wo, t_len = g.v, g.f, g.ho, g.wo, g.t_len
        self.emit(PlanOp('conv', g.hbuf, g.hbuf, (f, ho, wo), layer=g.lay.recurrent_part, halo=g.rhalo, src_mode=SRC_DIRECT,
                         act=g.act, rec_act=g.rec, lstm_f=f, aux=(None, g.cbufs[step - 1], g.cbufs[step]),
                         in_c_off=(step - 1) * f, in_c_total=t_len * f, out_c_off=step * f, out_c_total=t_len * f,
                         out_shape=(f, ho, wo),
                         src2={'buf': v.buf, 'xs': (g.cin, v.h, v.w), 'layer': g.lay.input_part, 'halo': g.halo,
                               'in_c_off': v.c_off + step * g.cin, 'in_c_total': v.c_total}))

    def lower_bilinear(self, t, lay, ins, outs):
        # keras UpSampling2D(2, interpolation='bilinear') (csrc/halo.hip): always one launch of its own on a whole stored
        # buffer -- anything lazy in front is materialised, a channel window is extracted first -- into a new buffer or the
        # model's output slot.  Never SRC_UPSAMPLE2, never a restated decoder layer and never a convolution's epilogue: the
        # convolution kernels know nearest up-sampling only.
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('%s on a reshaped tensor' % lay.name)
        v = self.whole(v)
        h2, w2 = 2 * v.h, 2 * v.w
        dst = self.out_or_new(outs, (v.c, h2, w2))
        self.emit(PlanOp('bilinear', v.buf, dst, (v.c, v.h, v.w), out_c_total=v.c, out_shape=(v.c, h2, w2)))
        self.views[t.uid] = View(dst, 0, v.c, v.c, h2, w2)

    def lower_pool_or_upsample(self, t, lay, ins, outs):
        """MaxPooling2D(2) / nearest UpSampling2D(2): a lazy source mode of the view -- or, in an inference plan, the epilogue of the
        convolution whose only consumer the pooling is"""
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('%s on a reshaped tensor' % lay.name)
        if not v.plain:
            v = self.materialize(v)
        prod = self.producer.get(v.buf) if (self.inference and isinstance(lay, L.MaxPooling2D) and v.full and not outs) else None
        if (prod is not None and self.consumers[t.inputs[0].uid] == 1 and not isinstance(prod.layer, L._ConvPart)
                and not prod.out_pool and _supports_out_pool(prod)):
            # the pooling runs in the producing convolution's epilogue: its buffer now holds the pooled tensor
            prod.out_pool = True
            c, h2, w2 = v.c, v.h // 2, v.w // 2
            prod.conv_out_shape = prod.out_shape        # what the convolution computes (FLOP accounting)
            prod.out_shape = (c, h2, w2)                # what it stores
            self.plan.buffers[v.buf] = (c, h2, w2)
            self.views[t.uid] = View(v.buf, 0, c, c, h2, w2)
        else:
            self.views[t.uid] = v.copy(src_mode=SRC_MAXPOOL2 if isinstance(lay, L.MaxPooling2D) else SRC_UPSAMPLE2)

    def lower_avgpool(self, t, lay, ins, outs):
        # keras AveragePooling2D(2) (csrc/halo.hip): always one launch of its own on a whole stored buffer -- anything lazy in
        # front is materialised, a channel window is extracted first -- into a new buffer or the model's output slot.  Never a
        # lazy source mode and never a convolution's epilogue: the convolution kernels know max-pooling only.
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('%s on a reshaped tensor' % lay.name)
        v = self.whole(v)
        h2, w2 = v.h // 2, v.w // 2
        dst = self.out_or_new(outs, (v.c, h2, w2))
        self.emit(PlanOp('avgpool', v.buf, dst, (v.c, v.h, v.w), out_c_total=v.c, out_shape=(v.c, h2, w2)))
        self.views[t.uid] = View(dst, 0, v.c, v.c, h2, w2)

    def lower_slice(self, t, lay, ins, outs):
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('slice_layer on a reshaped tensor')
        lo, hi = lay.window(v.c)
        self.views[t.uid] = v.copy(c_off=v.c_off + lo, c=hi - lo)

    def lower_reshape(self, t, lay, ins, outs):
        plan = self.plan
        v = self.whole(ins[0])
        c, h, w = _store_of(t.shape)
        if (c * h * w) != v.c * v.h * v.w:
            raise ValueError('Reshape size mismatch')
        # relabel the same contiguous block
        if v.buf >= 0:
            plan.buffers[v.buf] = (c, h, w)
            self.views[t.uid] = View(v.buf, 0, c, c, h, w, shape=tuple(t.shape) if len(t.shape) != 3 else None)
        else:
            nb = plan.new_buffer(v.c, v.h, v.w)
            self.emit(PlanOp('copy', v.buf, nb, (v.c, v.h, v.w), in_c_total=v.c, out_c_total=v.c,
                             out_shape=(v.c, v.h, v.w)))
            plan.buffers[nb] = (c, h, w)
            self.views[t.uid] = View(nb, 0, c, c, h, w, shape=tuple(t.shape) if len(t.shape) != 3 else None)

    def lower_concatenate(self, t, lay, ins, outs):
        c_tot = sum(v.logical[0] for v in ins)
        _, hh, ww = ins[0].logical
        dst = self.out_or_new(outs, (c_tot, hh, ww))
        off = 0
        for v in ins:
            self.materialize(v, dst=dst, dst_c_off=off, dst_c_total=c_tot)
            off += v.logical[0]
        self.views[t.uid] = View(dst, 0, c_tot, c_tot, hh, ww)

    def lower_strided_conv(self, t, lay, ins, outs):
        # keras Conv2D(strides=2) (csrc/sconv.hip): a stride-1 'valid' convolution of the space-to-depth image P of the padded
        # input (4 cin phase-major channels) with a kernel that is a permutation of the layer's own, stored with the 3 x 3 /
        # 5 x 5 taps the matrix-core kernels exist for (tconv_taps; the T x T block at the origin, zero taps below / right, P
        # that much longer).  Three ops: 'sphasew' (kernel -> derived kernel; plan.phase_params), 's2dp' (the lazy halo of the
        # input + the layer's own 'same' zeros + the de-interleave in one pass) and ONE 'conv' on P with the layer's bias and
        # activation in its epilogue.
        plan = self.plan
        if any(p['layer'] is lay for p in plan.phase_params):
            raise NotImplementedError('%s: a Conv2D layer with strides=2 applied more than once is not implemented' % lay.name)
        v = ins[0]
        if v.shape is not None and len(v.shape) != 3:
            raise NotImplementedError('%s on a non-3D tensor %r' % (lay.name, v.shape))
        if v.src_mode != SRC_DIRECT:         # (the pass reads a stored tensor; a halo in front may stay lazy)
            v = self.materialize(v.copy(halo=NO_HALO)).copy(halo=v.halo)
        _, hl, wl = v.logical                                   # what the layer sees as its input
        (th, pt, pb, ho), (tw, pl, pr, wo) = lay.strided_geometry(hl, wl)
        v, halo = self.with_zero_halo(v, ((pt, pb), (pl, pr)))
        kh, kw = lay.kernel_size
        sh, sw = tconv_taps(th, tw)
        hp, wp = ho + sh - 1, wo + sw - 1                       # the phase tensor the stored taps read
        f = lay.filters
        alg = 2 * ho * wo * f * v.c * kh * kw
        pidx = self.derived_kernel('sphasew', lay, v.c, (sh, sw, 4 * v.c, f), False, kind='sconv')
        # the phase tensor in front of the destination (buffer numbers), and one convolution with `filters` channels that reads
        # it: no phase channels and no interleave, so not phase_conv
        tmp = plan.new_buffer(4 * v.c, hp, wp)
        self.emit(PlanOp('s2dp', v.buf, tmp, (v.c, v.h, v.w), halo=halo, in_c_off=v.c_off, in_c_total=v.c_total,
                         out_c_total=4 * v.c, out_shape=(4 * v.c, hp, wp)))
        dst = self.out_or_new(outs, (f, ho, wo))
        self.emit(PlanOp('conv', tmp, dst, (4 * v.c, hp, wp), layer=lay, halo=NO_HALO, src_mode=SRC_DIRECT, act=ACT[lay.activation],
                         in_c_off=0, in_c_total=4 * v.c, out_c_off=0, out_c_total=f, out_shape=(f, ho, wo), dil=(1, 1),
                         ksize=(sh, sw), filters=f, wparam=pidx, alg_flops=alg, input_image=v.buf == STATE_IN))
        self.producer.pop(dst, None)         # (a MaxPooling2D behind it stays a launch / a lazy source of its own)
        self.views[t.uid] = View(dst, 0, f, f, ho, wo)

    def lower_depthwise(self, t, lay, ins, outs):
        # keras DepthwiseConv2D / SeparableConv2D (csrc/sepconv.hip): 'dwconv' = the stencil, which takes the lazy halo of its
        # input and the layer's own 'same' zeros composed (a lazy pooling / up-sampling view is materialised first: the stencil
        # reads a stored tensor); for a SeparableConv2D it has neither bias nor activation and writes a plan buffer that the
        # training step keeps (the pointwise weight gradient reads it), and 'pwconv' = the 1 x 1 product on the matrix cores
        # with the layer's bias and activation, which writes the model's output slot or a buffer of its own.
        plan = self.plan
        if lay in plan.sep_layers:
            raise NotImplementedError('%s: a %s layer applied more than once is not implemented' % (lay.name, type(lay).__name__))
        plan.sep_layers.append(lay)
        v = ins[0]
        if v.shape is not None and len(v.shape) != 3:
            raise NotImplementedError('%s on a non-3D tensor %r' % (lay.name, v.shape))
        if v.src_mode != SRC_DIRECT:
            v = self.materialize(v.copy(halo=NO_HALO)).copy(halo=v.halo)
        halo = v.halo
        if lay.padding == 'same':
            st, sb, sl, sr = lay.same_halo()
            v, halo = self.with_zero_halo(v, ((st, sb), (sl, sr)))
        _, hl, wl = v.copy(halo=halo).logical
        ho = hl - lay.dilation_rate[0] * (lay.kernel_size[0] - 1)
        wo = wl - lay.dilation_rate[1] * (lay.kernel_size[1] - 1)
        if ho < 1 or wo < 1:
            raise ValueError('%s: kernel %r with dilation %r does not fit the input' % (lay.name, lay.kernel_size, lay.dilation_rate))
        q = v.c * lay.depth_multiplier
        sep = isinstance(lay, L.SeparableConv2D)
        f = lay.filters if sep else q
        dst = self.out_or_new(outs, (f, ho, wo))
        mid = plan.new_buffer(q, ho, wo) if sep else dst
        self.emit(PlanOp('dwconv', v.buf, mid, (v.c, v.h, v.w), layer=lay, halo=halo, act=0 if sep else ACT[lay.activation],
                         in_c_off=v.c_off, in_c_total=v.c_total, out_c_off=0, out_c_total=q, out_shape=(q, ho, wo)))
        if sep:
            self.emit(PlanOp('pwconv', mid, dst, (q, ho, wo), layer=lay, act=ACT[lay.activation], in_c_off=0, in_c_total=q,
                             out_c_off=0, out_c_total=f, out_shape=(f, ho, wo)))
        self.views[t.uid] = View(dst, 0, f, f, ho, wo)

    def lower_conv2d(self, t, lay, ins, outs):
        """the layer's geometry, then one of three forms: conv_upsampled_dilated (a), conv_upsampled_phases (b), conv_plain"""
        v = ins[0]
        if v.shape is not None and len(v.shape) != 3:
            raise NotImplementedError('%s on a non-3D tensor %r' % (lay.name, v.shape))
        if v.src_mode == SRC_MAXPOOL2 and _prefers_unfused_pool(v.c, lay):
            # the Winograd kernels read plain tensors: pool once with the standalone kernel, keep the halo lazy
            v = self.materialize(v.copy(halo=NO_HALO)).copy(halo=v.halo)
        halo = v.halo
        if lay.padding == 'same':
            st, sb, sl, sr = lay.same_halo()
            v, halo = self.with_zero_halo(v, ((st, sb), (sl, sr)))
        _, hl, wl = v.copy(halo=halo).logical
        ho = hl - lay.dilation_rate[0] * (lay.kernel_size[0] - 1)
        wo = wl - lay.dilation_rate[1] * (lay.kernel_size[1] - 1)
        kh, kw = lay.kernel_size
        alg = 2 * ho * wo * lay.filters * v.c * kh * kw
        # ---- inference: a convolution on a 2x nearest-neighbour up-sampled tensor, restated on the tensor itself: (a) and (b).
        # both serve the training plan as well: (a) is a plain graph identity (forward, data and weight gradient of
        # the layer then run on the low-resolution tensors); (b) trains through the adjoints of its two linear maps
        # (dlwp_phase_weights_bwd, dlwp_space_to_depth2; training.py)
        # (a mirror halo WITHOUT the border element -- TFPadding2D 'REFLECT' -- does not commute with the up-sampling:
        #  up-sampled coordinate 2n reflects to source n - 1, low-resolution coordinate n to n - 2; the layer then keeps
        #  the reference's formulation.  'SYMMETRIC', periodic, zero and edge halos commute.)
        restate = (RESTATE_UPSAMPLED and v.src_mode == SRC_UPSAMPLE2 and
                   halo.mode_h != PAD_REFLECT and halo.mode_w != PAD_REFLECT)
        if (restate and tuple(lay.dilation_rate) == (2, 2) and
                all(p % 2 == 0 for p in halo[:4]) and ho % 2 == 0 and wo % 2 == 0):
            self.conv_upsampled_dilated(t, lay, v, halo, ho, wo, alg)
        elif (restate and tuple(lay.dilation_rate) == (1, 1) and
              ho == 2 * v.h and wo == 2 * v.w and
              _phase_geometry(kh, halo.top)[0] * _phase_geometry(kw, halo.left)[0] < kh * kw):
            self.conv_upsampled_phases(t, lay, v, outs, halo, ho, wo, alg)
        else:
            self.conv_plain(t, lay, v, outs, halo, ho, wo)

    def conv_upsampled_dilated(self, t, lay, v, halo, ho, wo, alg):
        # (a) dilation 2, even halo: tap u of output row 2i + a reads source row i + u - top/2 whatever a is, so the
        #     result is UpSampling2D(conv with dilation 1 and half the halo on the low-resolution tensor): a quarter
        #     of the multiplies, and the up-sampling stays lazy for the consumer.
        h2 = Halo(halo.top // 2, halo.bottom // 2, halo.left // 2, halo.right // 2, halo.mode_h, halo.mode_w)
        # (always a new buffer: the view is lazily up-sampled, so a model output is materialised from it by finish_outputs)
        dst = self.plan.new_buffer(lay.filters, ho // 2, wo // 2)
        self.emit(PlanOp('conv', v.buf, dst, (v.c, v.h, v.w), layer=lay, halo=h2, src_mode=SRC_DIRECT,
                         act=ACT[lay.activation], in_c_off=v.c_off, in_c_total=v.c_total, out_c_off=0,
                         out_c_total=lay.filters, out_shape=(lay.filters, ho // 2, wo // 2), dil=(1, 1), alg_flops=alg))
        self.views[t.uid] = View(dst, 0, lay.filters, lay.filters, ho // 2, wo // 2, src_mode=SRC_UPSAMPLE2)

    def conv_upsampled_phases(self, t, lay, v, outs, halo, ho, wo, alg):
        # (b) dilation 1: the k taps of an axis fall on k2 < k distinct source pixels; each of the 4 output phases is
        #     a k2 x k2 kernel of summed weights over the SAME window, so the layer runs as one convolution with
        #     4 x filters channels on the low-resolution tensor + a depth-to-space interleave (csrc/phase.hip).
        kh, kw = lay.kernel_size
        (kh2, lo_h, hi_h), (kw2, lo_w, hi_w) = _phase_geometry(kh, halo.top), _phase_geometry(kw, halo.left)
        h2 = Halo(-lo_h, hi_h, -lo_w, hi_w, halo.mode_h, halo.mode_w)
        pidx = self.derived_kernel('phasew', lay, v.c, (kh2, kw2, v.c, 4 * lay.filters), lay.use_bias, halo=halo,
                                   pad_top=halo.top, pad_left=halo.left)
        dst = self.phase_conv(lay, v, outs, h2, (kh2, kw2), pidx, alg, (v.h, v.w), (ho, wo))
        self.views[t.uid] = View(dst, 0, lay.filters, lay.filters, ho, wo)

    def conv_plain(self, t, lay, v, outs, halo, ho, wo):
        dst = self.out_or_new(outs, (lay.filters, ho, wo))
        self.emit(PlanOp('conv', v.buf, dst, (v.c, v.h, v.w), layer=lay, halo=halo, src_mode=v.src_mode,
                         act=ACT[lay.activation], in_c_off=v.c_off, in_c_total=v.c_total, out_c_off=0,
                         out_c_total=lay.filters, out_shape=(lay.filters, ho, wo)))
        self.views[t.uid] = View(dst, 0, lay.filters, lay.filters, ho, wo)

    def lower_tconv(self, t, lay, ins, outs):
        # keras Conv2DTranspose(strides=2) (csrc/tconv.hip): the 4 output phases are stride-1 cross-correlations of the layer's
        # input (zero halo T - 1, T = ceil(k / 2)) with kernels that are a permutation of the layer's own (stored with the
        # 3 x 3 / 5 x 5 taps the matrix-core kernels exist for, zero taps and a wider zero halo around: tconv_taps), so it runs as
        # 'tphasew' (kernel -> derived kernel; plan.phase_params) + ONE convolution with 4 x filters channels (bias and
        # activation in its epilogue) + 'd2sc', an interleave that also crops ('same' padding, the extra row / column of an odd
        # kernel).  An inference plan lets the convolution store the phases interleaved where a kernel can and nothing is cropped.
        if any(p['layer'] is lay for p in self.plan.phase_params):
            raise NotImplementedError('%s: a Conv2DTranspose layer applied more than once is not implemented' % lay.name)
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('%s (Conv2DTranspose) on a reshaped (non-3D) tensor %r' % (lay.name, v.shape))
        if v.src_mode != SRC_DIRECT:         # (its convolution reads a stored tensor; a halo in front may stay lazy)
            v = self.materialize(v.copy(halo=NO_HALO)).copy(halo=v.halo)
        kh, kw = lay.kernel_size
        th, tw = (kh + 1) // 2, (kw + 1) // 2
        sh, sw = tconv_taps(th, tw)
        oh, ow = (sh - th) // 2, (sw - tw) // 2             # where the Th x Tw block sits in the stored taps
        own = ((th - 1 + oh, th - 1 + sh - th - oh), (tw - 1 + ow, tw - 1 + sw - tw - ow))
        v, halo = self.with_zero_halo(v, own)
        _, hl, wl = v.copy(halo=halo).logical
        hp, wp = hl - sh + 1, wl - sw + 1                   # the phase tensor: (4F, h + Th - 1, w + Tw - 1)
        hin, win = hp - th + 1, wp - tw + 1                 # what the layer sees as its input
        same = lay.padding == 'same'
        top, left = (max(kh - 2, 0) // 2, max(kw - 2, 0) // 2) if same else (0, 0)
        ho = 2 * hin + (0 if same else max(kh - 2, 0))
        wo = 2 * win + (0 if same else max(kw - 2, 0))
        f = lay.filters
        alg = 2 * hin * win * f * v.c * kh * kw
        pidx = self.derived_kernel('tphasew', lay, v.c, (sh, sw, v.c, 4 * f), lay.use_bias, kind='tconv')
        dst = self.phase_conv(lay, v, outs, halo, (sh, sw), pidx, alg, (hp, wp), (ho, wo), crop=(top, left))
        self.views[t.uid] = View(dst, 0, f, f, ho, wo)

    def lower_crop(self, t, lay, ins, outs):
        # keras Cropping2D: one launch of its own on a whole stored buffer (the adjoint of zero padding) -- or, directly behind
        # a Conv2DTranspose whose interleave nothing else reads, a smaller window of that interleave (moves only: same bits)
        plan = self.plan
        v = ins[0]
        if v.shape is not None:
            raise NotImplementedError('%s (Cropping2D) on a reshaped (non-3D) tensor %r' % (lay.name, v.shape))
        (ct, cb), (cl, cr) = lay.cropping
        v = self.whole(v)
        ho, wo = v.h - ct - cb, v.w - cl - cr
        if ho <= 0 or wo <= 0:
            raise ValueError('%s (Cropping2D): cropping %r leaves nothing of %d x %d' % (lay.name, lay.cropping, v.h, v.w))
        writers = [op for op in plan.ops if op.dst == v.buf]
        w0 = writers[0] if len(writers) == 1 else None
        if (w0 is not None and w0.kind == 'd2sc' and v.buf >= 0 and self.consumers[t.inputs[0].uid] == 1 and
                not self.out_index.get(t.inputs[0].uid) and not any(op.src == v.buf for op in plan.ops)):
            w0.crop = (w0.crop[0] + ct, w0.crop[1] + cl)
            w0.out_shape = (v.c, ho, wo)
            if outs:                             # the interleave writes the model's output slot itself
                w0.dst = OUT(outs[0])
                plan.output_store[outs[0]] = (v.c, ho, wo)
            else:
                plan.buffers[v.buf] = (v.c, ho, wo)
            self.views[t.uid] = View(w0.dst, 0, v.c, v.c, ho, wo)
        else:
            dst = self.out_or_new(outs, (v.c, ho, wo))
            self.emit(PlanOp('crop', v.buf, dst, (v.c, v.h, v.w), halo=Halo(ct, cb, cl, cr, PAD_ZERO, PAD_ZERO), out_c_total=v.c,
                             out_shape=(v.c, ho, wo)))
            self.views[t.uid] = View(dst, 0, v.c, v.c, ho, wo)

    def lower_rowconv(self, t, lay, ins, outs):
        # DLWP.custom.RowConnected2D (reference custom.py:695-837): per-row filters, dlwp_rowconv2d_fwd.  Its kernels read a
        # stored float32 tensor, directly or 2x up-sampled (a lazy pooling in front is materialised); the halo stays in the
        # loader.
        v = ins[0]
        if v.shape is not None and len(v.shape) != 3:
            raise NotImplementedError('%s on a non-3D tensor %r' % (lay.name, v.shape))
        if v.src_mode == SRC_MAXPOOL2:           # (a 2x up-sampling in front is resolved by the row kernels' loaders)
            v = self.materialize(v.copy(halo=NO_HALO)).copy(halo=v.halo)
        _, hl, wl = v.logical
        kh, kw = lay.kernel_size
        ho, wo = hl - kh + 1, wl - kw + 1
        if tuple(lay.kernel.shape) != (ho, kh, kw, v.c, lay.filters):
            raise ValueError('%s: kernel %r does not fit the input (%d rows of output, %d channels)' %
                             (lay.name, tuple(lay.kernel.shape), ho, v.c))
        dst = self.out_or_new(outs, (lay.filters, ho, wo))
        self.emit(PlanOp('rowconv', v.buf, dst, (v.c, v.h, v.w), layer=lay, halo=v.halo, src_mode=v.src_mode,
                         act=ACT[lay.activation], in_c_off=v.c_off, in_c_total=v.c_total, out_c_off=0,
                         out_c_total=lay.filters, out_shape=(lay.filters, ho, wo)))
        self.views[t.uid] = View(dst, 0, lay.filters, lay.filters, ho, wo)

    def lower_batchnorm(self, t, lay, ins, outs):
        # keras BatchNormalization(axis=1) (csrc/batchnorm.hip): its input is materialised as a whole buffer (the statistics
        # pass reads it, and the training plan keeps it for the backward); its output is a new buffer, so nothing lazy and no
        # epilogue of the convolution in front (pooled store, pooled weight gradient) carries a value across it
        if lay in self.plan.bn_layers:
            raise NotImplementedError('%s: a BatchNormalization layer applied more than once is not implemented' % lay.name)
        v = ins[0]
        if v.shape is not None and len(v.shape) != 3:
            raise NotImplementedError('%s on a non-3D tensor %r' % (lay.name, v.shape))
        v = self.whole(v)
        dst = self.out_or_new(outs, (v.c, v.h, v.w))
        self.plan.bn_layers.append(lay)
        self.emit(PlanOp('bn', v.buf, dst, (v.c, v.h, v.w), layer=lay, out_c_total=v.c, out_shape=(v.c, v.h, v.w)))
        self.views[t.uid] = View(dst, 0, v.c, v.c, v.h, v.w)

    def lower_flatten(self, t, lay, ins, outs):
        # keras Flatten (default data_format): the contiguous per-sample block read as one row -- a view, no launch.  The
        # buffer keeps its stored shape (what its producer and that producer's backward know); only the logical shape changes.
        self.views[t.uid] = self.whole(ins[0]).copy(shape=tuple(t.shape))

    def lower_dense(self, t, lay, ins, outs):
        # keras Dense (csrc/dense.hip): reads a whole stored buffer as (n, k) rows, writes (n, units)
        if lay in self.plan.dense_layers:
            raise NotImplementedError('%s: a Dense layer applied more than once is not implemented' % lay.name)
        v = self.whole(ins[0])
        if lay.kernel is not None and v.c * v.h * v.w != int(lay.kernel.shape[0]):
            raise ValueError('%s: kernel for %d features on an input of %d' % (lay.name, lay.kernel.shape[0], v.c * v.h * v.w))
        dst = self.out_or_new(outs, (lay.units, 1, 1))
        self.plan.dense_layers.append(lay)
        self.emit(PlanOp('dense', v.buf, dst, (v.c, v.h, v.w), layer=lay, act=ACT[lay.activation], out_c_total=lay.units,
                         out_shape=(lay.units, 1, 1)))
        self.views[t.uid] = View(dst, 0, lay.units, lay.units, 1, 1, shape=tuple(t.shape))

    def lower_dropout(self, t, lay, ins, outs):
        # keras Dropout: the identity outside training -- an inference plan passes the view on.  The training plan gives it a
        # launch and a buffer of its own (the executor runs it as a copy when the forward is not a training step's).
        if lay in self.plan.dropout_layers:
            raise NotImplementedError('%s: a Dropout layer applied more than once is not implemented' % lay.name)
        self.plan.dropout_layers.append(lay)
        if self.inference:
            self.views[t.uid] = ins[0]
        else:
            shp = ins[0].shape
            v = self.whole(ins[0])
            dst = self.out_or_new(outs, (v.c, v.h, v.w))
            self.emit(PlanOp('dropout', v.buf, dst, (v.c, v.h, v.w), layer=lay, out_c_total=v.c, out_shape=(v.c, v.h, v.w)))
            self.views[t.uid] = View(dst, 0, v.c, v.c, v.h, v.w, shape=shp)

    def lower_activation(self, t, lay, ins, outs):
        # keras activation layers (csrc/eltwise.hip): 'linear' passes the view on; every other kind reads its input as a whole
        # flat buffer (materialised like BatchNormalization's: the training plan keeps it, the backward takes f' from it) and
        # writes a new buffer or the model's output slot.  Nothing lazy crosses the layer, and no state: the same layer object
        # may appear in any number of ops.
        if lay.eltwise is None:
            self.views[t.uid] = ins[0].copy()
        else:
            shp = ins[0].shape
            v = self.whole(ins[0])
            dst = self.out_or_new(outs, (v.c, v.h, v.w))
            if lay not in self.plan.eltwise_layers:
                self.plan.eltwise_layers.append(lay)
            self.emit(PlanOp('act', v.buf, dst, (v.c, v.h, v.w), layer=lay, out_c_total=v.c, out_shape=(v.c, v.h, v.w)))
            self.views[t.uid] = View(dst, 0, v.c, v.c, v.h, v.w, shape=shp)

    def lower_merge(self, t, lay, ins, outs):
        # keras merge layers (csrc/eltwise.hip): 2 to 4 whole flat buffers of one size -> a new buffer or the output slot
        shp = ins[0].shape
        vs = [self.whole(v) for v in ins]
        v0 = vs[0]
        if any(v.c * v.h * v.w != v0.c * v0.h * v0.w for v in vs):
            raise ValueError('%s: inputs of different sizes' % lay.name)
        dst = self.out_or_new(outs, (v0.c, v0.h, v0.w))
        if lay not in self.plan.eltwise_layers:
            self.plan.eltwise_layers.append(lay)
        self.emit(PlanOp('merge', v0.buf, dst, (v0.c, v0.h, v0.w), layer=lay, aux=tuple(v.buf for v in vs[1:]), out_c_total=v0.c,
                         out_shape=(v0.c, v0.h, v0.w)))
        self.views[t.uid] = View(dst, 0, v0.c, v0.c, v0.h, v0.w, shape=shp)

    def finish_outputs(self, t, outs):
        """a model output that was not produced in place by a conv / concatenate: materialise it into its slot"""
        plan, views = self.plan, self.views
        for k, o in enumerate(outs):
            v = views[t.uid]
            if v.buf == OUT(o) and v.full:
                continue
            lc = v.logical
            plan.output_store[o] = lc
            # The value is the whole of a scratch buffer that exactly one launch writes and nothing reads (a convolution -- or its
            # depth-to-space pass -- behind a Reshape, which is a view: examples/train.py's recurrent stack ends that way): let
            # that launch write the output slot itself instead of copying the buffer (9 us per forward of config 4 at 8 members).
            if k == 0 and v.full and v.buf >= 0:
                def reads(op):
                    extra = [b for b in (op.aux or ()) if isinstance(b, int)] if op.kind in ('conv', 'lstm', 'merge') else []
                    return op.src == v.buf or v.buf in extra
                writers = [op for op in plan.ops if op.dst == v.buf]
                w0 = writers[0] if len(writers) == 1 else None
                if (w0 is not None and w0.kind in ('conv', 'd2s', 'rowconv', 'dense') and not w0.lstm_f and not w0.out_pool and
                        (w0.kind == 'dense' or (w0.out_c_off == 0 and w0.out_c_total in (0, lc[0]))) and
                        not any(reads(op) for op in plan.ops)):
                    # every view of the abandoned scratch buffer follows the launch into the output slot (the convolution's own
                    # tensor in front of the Reshape, slices of it): a consumer lowered LATER -- another branch of a
                    # multi-output model -- must not read a buffer nothing writes any more
                    old = v.buf
                    w0.dst = OUT(o)
                    for uid in [u for u, vv in views.items() if vv.buf == old]:
                        views[uid] = views[uid].copy(buf=OUT(o))
                    views[t.uid] = View(OUT(o), 0, lc[0], lc[0], lc[1], lc[2], shape=v.shape)
                    continue
            self.materialize(v, dst=OUT(o), dst_c_off=0, dst_c_total=lc[0])
            if k == 0:
                views[t.uid] = View(OUT(o), 0, lc[0], lc[0], lc[1], lc[2], shape=v.shape)


# (class or predicate of the layer, lowering): the FIRST row that matches lowers the layer.  A new layer kind is one method of
# _PlanBuilder and one row here.  Rows whose position matters say which later row they must stay in front of; every other row
# matches a class that no other row's class is a base or a subclass of.
_LOWERINGS = (
    (L._Pad2DBase, _PlanBuilder.lower_pad2d),
    (L._Pad3DBase, _PlanBuilder.lower_pad3d),
    (L.ConvLSTM2D, _PlanBuilder.lower_convlstm),
    # in front of UpSampling2D below: a bilinear UpSampling2D is never the lazy (nearest) source mode
    (lambda lay: isinstance(lay, L.UpSampling2D) and lay.interpolation == 'bilinear', _PlanBuilder.lower_bilinear),
    (L.MaxPooling2D, _PlanBuilder.lower_pool_or_upsample),
    (L.UpSampling2D, _PlanBuilder.lower_pool_or_upsample),
    (L.AveragePooling2D, _PlanBuilder.lower_avgpool),
    (L.ChannelSlice, _PlanBuilder.lower_slice),
    (L.Reshape, _PlanBuilder.lower_reshape),
    (L.Concatenate, _PlanBuilder.lower_concatenate),
    # in front of Conv2D below: the strided layer is the same class
    (lambda lay: isinstance(lay, L.Conv2D) and tuple(lay.strides) == (2, 2), _PlanBuilder.lower_strided_conv),
    (L.DepthwiseConv2D, _PlanBuilder.lower_depthwise),      # SeparableConv2D too: its subclass (neither is a Conv2D)
    (L.Conv2D, _PlanBuilder.lower_conv2d),
    (L.Conv2DTranspose, _PlanBuilder.lower_tconv),
    (L.Cropping2D, _PlanBuilder.lower_crop),
    (L.RowConnected2D, _PlanBuilder.lower_rowconv),
    (L.BatchNormalization, _PlanBuilder.lower_batchnorm),
    (L.Flatten, _PlanBuilder.lower_flatten),
    (L.Dense, _PlanBuilder.lower_dense),
    (L.Dropout, _PlanBuilder.lower_dropout),
    (L._ActivationLayer, _PlanBuilder.lower_activation),
    (L._Merge, _PlanBuilder.lower_merge),
)


def build_plan(inputs, outputs, inference=False, fuse_d2s=True, fuse_lstm=False, fuse_lstm_step=True, transform=None):
    """inputs: [KTensor] (exactly one), outputs: [KTensor].  Returns a Plan.  inference=True additionally moves a
    MaxPooling2D(2) that is the only consumer of a convolution into that convolution's epilogue (the pre-pooling tensor
    is never written; the training plan keeps it because the backward pass needs it).
    transform = (head, tail) (inference plans of a model with one output): the wrapper's imputer / scaler as launches of the model
    call (csrc/scale.hip).  head: a 'scale' op in front reads the input state and writes a buffer of its own, which every consumer
    of the model input reads instead; tail: a 'scale' op at the end rewrites the output slot in place.  The state a rollout feeds
    back therefore stays in unscaled units."""
    if len(inputs) != 1:
        raise NotImplementedError('exactly one model input is supported')
    head, tail = (bool(transform[0]), bool(transform[1])) if transform is not None else (False, False)
    if (head or tail) and not inference:
        raise ValueError('an input / output transform belongs to inference plans: training data is prepared on the host')
    if tail and len(outputs) != 1:
        raise ValueError('an output transform needs a model with exactly one output, got %d' % len(outputs))
    plan = _PlanBuilder(inputs, outputs, inference, fuse_d2s, fuse_lstm, fuse_lstm_step, head).run()
    for o, st in enumerate(plan.output_store):
        if st is None:
            raise RuntimeError('output %d was never produced' % o)
    if tail:
        plan.ops.append(PlanOp('scale', OUT(0), OUT(0), plan.output_store[0], role='tail', out_shape=plan.output_store[0]))
    return plan
