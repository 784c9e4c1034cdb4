"""
The backward pass of one training step (Trainer._backward): the plan's ops in reverse, one adjoint method per op kind, over
three small helpers -- GradBook (which buffer holds which gradient), SideLanes (weight gradients beside the data-gradient
chain) and the weight-gradient / data-gradient pair bracket.  Host Python only: every device launch is a dlwp_amd.ops call.
"""
import os

import torch

from . import _lib, ops
from . import layers as L
from . import plan as P
from .training import _PhaseGrad


class GradBook(object):
    """Which plan buffer holds which gradient.  grads: buffer id -> gradient tensor; written: buffer id -> [(c_off, c)] channel
    windows that already hold a gradient; pending_pool: buffer id -> gradient of its MaxPooling2D(2) image, while that is the
    only gradient so far (the producing convolution then takes pooling + activation backward (+ bias gradient) in one pass)."""

    def __init__(self, trainer, bufs, x, outs):
        self.trainer, self.bufs, self.x, self.outs = trainer, bufs, x, outs
        self.n = None if x is None else x.shape[0]
        self.grads, self.written, self.pending_pool = {}, {}, {}

    def tensor(self, i):
        if i >= 0:
            return self.bufs[i]
        return self.x if i == P.STATE_IN else self.outs[-2 - i]

    def set(self, buf, g, c):
        """g IS the gradient of the whole buffer (c channels)."""
        self.grads[buf] = g
        self.written[buf] = [(0, c)]

    def overlaps(self, buf, c_off, c):
        """some channel of [c_off, +c) already holds a gradient"""
        return any(not (c_off + c <= o or o + k <= c_off) for o, k in self.written.get(buf, ()))

    def covered(self, buf, c_off, c):
        """every channel of [c_off, +c) already holds a gradient"""
        return all(any(o <= ch < o + k for o, k in self.written.get(buf, ())) for ch in range(c_off, c_off + c))

    def materialise(self, buf):
        gp = self.pending_pool.pop(buf, None)
        if gp is not None:
            self.deposit(buf, 0, gp.shape[1], ops.maxpool2_bwd(self.tensor(buf), gp))

    def grad_of(self, buf):
        self.materialise(buf)
        g = self.grads.get(buf)
        if g is None:
            g = self.grads[buf] = torch.empty_like(self.tensor(buf))
        return g

    def claim_window(self, buf, c_off, c):
        """The gradient tensor of `buf` for a kernel that WRITES every element of channels [c_off, +c) itself -- or None where some
        channel of the window already holds a gradient (the caller then produces a dense tensor and deposits it)."""
        self.materialise(buf)
        if self.overlaps(buf, c_off, c):
            return None
        g = self.grad_of(buf)
        self.written.setdefault(buf, []).append((c_off, c))
        return g

    def deposit(self, buf, c_off, c, dense):
        """Put `dense` (n, c, h, w) into window [c_off, +c) of grad[buf]: overwrite on first touch, add after."""
        self.materialise(buf)
        if self.grads.get(buf) is None and c_off == 0 and tuple(dense.shape) == tuple(self.tensor(buf).shape) and \
                dense.is_contiguous():
            self.set(buf, dense, c)           # first gradient of the whole tensor: adopt it, no copy
            return
        g = self.grad_of(buf)
        n = self.n
        full = c_off == 0 and c == g.shape[1]
        if not self.overlaps(buf, c_off, c):
            if full:
                if dense.data_ptr() != g.data_ptr():
                    self.trainer._foreign = True      # (torch's own launch: a recorded step would miss it)
                    g.view(-1).copy_(dense.reshape(-1))
            else:
                ops.copy_channels(dense.reshape((n, c) + tuple(g.shape[2:])), g, c, 0, c_off)
            self.written.setdefault(buf, []).append((c_off, c))
        elif full and self.written[buf] == [(0, g.shape[1])]:
            ops.axpby(dense.reshape(-1), g.view(-1), 1.0, 1.0)
        elif self.covered(buf, c_off, c):
            # the window already holds a gradient everywhere (e.g. h_{t-1}: read by the next layer as part of the
            # whole sequence AND by the recurrent convolution of step t): extract, add, put back
            cur = torch.empty((n, c) + tuple(g.shape[2:]), dtype=torch.float32, device=g.device)
            ops.copy_channels(g, cur, c, c_off, 0)
            ops.axpby(dense.reshape(-1), cur.view(-1), 1.0, 1.0)
            ops.copy_channels(cur, g, c, 0, c_off)
        else:
            raise NotImplementedError('partially overlapping channel windows in the backward pass')


class SideLanes(object):
    """Weight gradients leave the critical path (activation backward -> data gradient -> ...): run(fn) issues fn on a side
    stream that first waits for everything issued on the main stream so far; join() makes the main stream wait for them.
    sides None: fn runs at once, on the main stream.

    Policy 'each' (default): every weight gradient forks as soon as its operands exist, round-robin over the side streams (r3,
    eager steps; batch 64: the last layers' weight gradients no longer pile up behind the end of the chain).
    Policy 'batch' (DLWP_WGRAD_FORKS=batch): they are queued and launched in TWO batches with one fork each -- a fork / join
    costs ~10 us inside a captured graph (profiles/r3_train_b8_timeline.txt): the first half, one after the other, beside the
    second half of the chain; the rest in parallel behind it.  That rule was made for forks inside a captured graph.

    Inside a captured step everything stays on ONE stream: replaying graphs with forked branches crashed inside
    hipGraphLaunch now and then (r3: 2 of 3 full test runs), and the forks bought little there (0.49 vs ~0.47 ms at 8
    samples: a fork / join costs ~10 us in a graph).  The eager step keeps the side streams (batch 64: 1.78 -> 1.68 ms)."""

    def __init__(self, sides, main, n_wgrad, policy='each', capturing=False, wait=None, on_stream=None):
        self.sides = None if capturing or sides is None else sides
        self.main = main
        self.each = policy != 'batch'
        self.first_batch = (n_wgrad + 1) // 2
        self.wait = wait or ops.stream_wait
        self.on_stream = on_stream or torch.cuda.stream
        self.wq, self.used, self.queued = [], [], 0

    def _fork(self, st):
        self.wait(st, self.main)         # behind everything issued on the main stream so far
        if st not in self.used:
            self.used.append(st)

    def run(self, fn):
        if self.sides is None:
            fn()
            return
        self.queued += 1
        if self.each:
            st = self.sides[(self.queued - 1) % len(self.sides)]
            self._fork(st)
            with self.on_stream(st):
                fn()
            return
        self.wq.append(fn)
        if self.queued == self.first_batch:
            self.flush(False)

    def flush(self, parallel):
        """The queued functions: over all side streams (parallel) or one after the other on the first; one fork per stream."""
        started = set()
        for i, fn in enumerate(self.wq):
            st = self.sides[i % len(self.sides)] if parallel else self.sides[0]
            if id(st) not in started:
                self._fork(st)
                started.add(id(st))
            with self.on_stream(st):
                fn()
        del self.wq[:]

    def join(self):
        if self.sides is None:
            return
        self.flush(True)
        for st in self.used:
            self.wait(self.main, st)     # the weight gradients join before anything reads them


class _OpCtx(object):
    """One op of the pass: its index k, the op, its descriptor d, the gradient gD of its output (None: only pooled_grad, the
    gradient of the output's pooled image, exists) and its source tensor."""
    __slots__ = ('k', 'op', 'd', 'gD', 'src', 'pooled_grad')

    def __init__(self, k, op, d, gD, src, pooled_grad):
        self.k, self.op, self.d, self.gD, self.src, self.pooled_grad = k, op, d, gD, src, pooled_grad


class BackwardPass(object):
    """prep (the folded step, Trainer._fold_ok): prepared data-gradient operands, a workspace per deferred final sum
    (key(what, k)), the weight gradients on the side streams; `post` collects the work that needs the final sums -- the caller
    runs it behind ops.reductions_flush."""

    def __init__(self, trainer, x, outs, dys, prep=None):
        tr = self.trainer = trainer
        self.plan, self.device, self.prep = tr.plan, tr.device, prep
        self.ex = tr.model.train_executor
        self.n = n = x.shape[0]
        self.post = []
        main = sides = None
        if prep is not None:
            main = torch.cuda.current_stream(self.device)
            if tr._side is None:
                tr._ensure_side_streams()
            sides = tr._side
        self.lanes = SideLanes(sides, main, sum(1 for op in self.plan.ops if op.kind == 'conv'),
                               os.environ.get('DLWP_WGRAD_FORKS', 'each'),
                               capturing=sides is not None and torch.cuda.is_current_stream_capturing())
        # r4: where the step replays as ONE hipGraph on one stream (small batches: every launch under a round of workgroups), a
        # layer's weight gradient and its data gradient -- both read dz, neither the other's output -- leave in one launch
        # (ops.pair_begin / pair_end, csrc/conv_pair.hip).  The pair opens in front of the weight gradient and closes behind the data
        # gradient's convolution; what is issued in between (bias gradient) depends on neither.
        self.can_pair = (prep is not None and os.environ.get('DLWP_TRAIN_PAIR', '1') != '0' and
                         tr._graph_ok(int(n)) == 'graph')
        self.pair_is_open = False
        self.book = GradBook(tr, self.ex.scratch(n), x.reshape((n,) + self.plan._in_store), outs)
        self.touched = set()     # ids of the layers whose gradients this pass has written
        self.preact = set()      # buffers whose gradient is already a PRE-activation gradient (dlwp_conv2d_bwd_data_act)
        self.phase_db = {}       # convolution op index -> bias gradient of its phase channels, already summed with the loss
        for o, dy in enumerate(dys):
            if isinstance(dy, _PhaseGrad):     # the gradient arrives on the phase channels: the 'd2s' op has no adjoint to run
                self.book.set(dy.buf, dy.dz, dy.dz.shape[1])
                if dy.db is not None:
                    self.phase_db[dy.conv_k] = dy.db
            else:
                self.book.set(P.OUT(o), dy, dy.shape[1])

    def key(self, what, k):
        """the scratch of one deferred sum of the folded step"""
        return (what, k) if self.prep is not None else None

    def pair_open(self):
        if self.can_pair and not self.pair_is_open:
            ops.pair_begin(self.device)
            self.pair_is_open = True

    def pair_close(self):
        if self.pair_is_open:
            self.pair_is_open = False
            ops.pair_end(self.device)

    def touch(self, lay):
        self.touched.add(id(lay))
        if isinstance(lay, L._ConvPart):
            self.touched.add(id(lay.parent))

    def shape4(self, op):
        return _lib.Shape4(self.n, op.xs[0], op.xs[1], op.xs[2])

    def new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def run(self):
        book, tr = self.book, self.trainer
        adjoints = self.adjoints
        descs = self.ex._descriptors()
        for k, (op, d) in reversed(list(enumerate(zip(self.plan.ops, descs)))):
            pooled_grad = None
            if op.dst in book.pending_pool:
                if self._takes_pooled(op):
                    pooled_grad = book.pending_pool.pop(op.dst)
                else:
                    book.materialise(op.dst)
            if op.dst not in book.grads and pooled_grad is None:
                continue                      # nothing downstream of this op contributes to the loss
            adjoint = adjoints.get(op.kind)
            if adjoint is None:
                raise RuntimeError(op.kind)
            adjoint(self, _OpCtx(k, op, d, book.grads.get(op.dst), book.tensor(op.src), pooled_grad))
        self.pair_close()          # (a layer whose data gradient took no convolution)
        # layers that received no gradient this step (unused by any output) must not keep a stale one
        for lay, nm, off, numel, shape in tr.entries:
            if id(lay) not in self.touched:
                tr._foreign = True            # (torch's own launch: a recorded step would miss it)
                tr.flat_grads[off:off + numel].zero_()
        self.lanes.join()
        return self.post

    def _takes_pooled(self, op):
        """The op is the convolution that alone wrote the pooled buffer: it takes the pooling backward with its own."""
        lay = op.layer if op.kind == 'conv' else None
        return (lay is not None and op.wparam is None and op.out_c_off == 0 and
                op.conv_geometry[0] == self.book.tensor(op.dst).shape[1] and
                (lay.bias is None or id(lay) not in self.touched))

    # -- convolution --------------------------------------------------------------------------------------------------- #
    def _conv(self, c):
        op, lay = c.op, c.op.layer
        y = self.book.tensor(op.dst)
        acc = id(lay) in self.touched
        kern = self.ex.conv_weights(op)[0]
        xs = self.shape4(op)
        if self._conv_pooled_first_layer(c, y, acc, xs):
            self.touch(lay)
            return
        dz, fused_bias = self._conv_act_bias(c, y, acc)
        dgrad = op.src != P.STATE_IN and not op.input_image     # (no gradient w.r.t. the model input, or its space-to-depth image)
        if dgrad:
            self.pair_open()           # (closed behind the data gradient's convolution)
        self._conv_wgrad(c, dz, kern, xs, acc, fused_bias)
        self.touch(lay)
        if dgrad:
            self._conv_dgrad(c, dz, kern, xs)

    def _conv_pooled_first_layer(self, c, y, acc, xs):
        """The first layer under MaxPooling2D(2): nobody needs its data gradient, so the pooling + activation backward is
        formed inside the weight gradient's loader and the gradient tensor is never stored (DLWP_WGRAD_POOLED=0: not)."""
        op, lay, pg = c.op, c.op.layer, c.pooled_grad
        if not (pg is not None and op.src == P.STATE_IN and not acc and pg.is_contiguous() and
                os.environ.get('DLWP_WGRAD_POOLED', '1') != '0' and ops.conv2d_bwd_weight_pooled_supported(xs, c.d)):
            return False
        gb = self.trainer._grad_view(lay, 'bias') if lay.bias is not None else None
        gw = self.trainer._grad_view(lay, 'kernel')
        ws_key = self.key('wgrad', c.k)
        self.lanes.run(lambda: ops.conv2d_bwd_weight_pooled(c.src, y, pg, gw, gb, c.d, xs, op.act, ws_key=ws_key))
        return True

    def _conv_act_bias(self, c, y, acc):
        """dy -> dz (in place where there is a dy) and, where the same pass can sum it, the bias gradient.  Returns
        (dz, whether the bias gradient is done)."""
        op, lay, gD = c.op, c.op.layer, c.gD
        gv = self.trainer._grad_view
        if op.dst in self.preact:          # the reader's data gradient left dz and this layer's bias gradient already
            return gD, True
        if c.pooled_grad is not None:      # the layer's only reader is MaxPooling2D(2): its backward rides along
            fused_bias = lay.bias is not None
            dz = ops.pool_act_bwd_bias_grad(y, c.pooled_grad, op.act, gv(lay, 'bias') if fused_bias else None,
                                            ws_key=self.key('bias', c.k))
            return dz, fused_bias
        fused_bias = (lay.activation != 'linear' and lay.bias is not None and not acc and op.wparam is None and
                      gD.shape[1] == lay.filters and tuple(y.shape) == tuple(gD.shape))
        if fused_bias:                     # dz in place of dy and the bias gradient from the same pass
            ops.act_bwd_bias_grad(y, gD, op.act, gv(lay, 'bias'), lay.filters, out=gD, ws_key=self.key('bias', c.k))
        elif lay.activation != 'linear':
            ops.act_bwd(y, gD, op.act, out=gD)          # dz in place of dy
        return gD, fused_bias

    def _conv_wgrad(self, c, dz, kern, xs, acc, fused_bias):
        """Weight gradient on a side lane, then the bias gradient no other pass has summed.  The views into flat_grads are
        taken here, not when a queued launch finally runs (DLWP_WGRAD_FORKS=batch: at the flush) -- the same views, since
        flat_grads is allocated once per trainer and never inside a step."""
        op, lay, d, src = c.op, c.op.layer, c.d, c.src
        gv = self.trainer._grad_view
        if op.wparam is not None:          # the layer runs with phase-summed kernels (plan.phase_params)
            self._conv_wgrad_derived(c, dz, kern, xs, acc, fused_bias)
            return
        gw, wkey = gv(lay, 'kernel'), self.key('wgrad', c.k)
        self.lanes.run(lambda: ops.conv2d_bwd_weight(src, dz, gw, d, xs, accumulate=acc, ws_key=wkey))
        if lay.bias is None or fused_bias:
            return
        gb = gv(lay, 'bias')
        if acc:
            tmp = torch.empty_like(gb)
            ops.bias_grad(dz, tmp, lay.filters)
            ops.axpby(tmp, gb, 1.0, 1.0)
        else:
            bkey = self.key('bias', c.k)
            self.lanes.run(lambda: ops.bias_grad(dz, gb, lay.filters, ws_key=bkey))

    def _conv_wgrad_derived(self, c, dz, kern, xs, acc, fused_bias=False):
        """Gradients of the derived kernels, folded back onto the layer's own."""
        op, lay, d, src = c.op, c.op.layer, c.d, c.src
        gv = self.trainer._grad_view
        n_out = op.conv_geometry[0]
        pp = self.plan.phase_params[op.wparam]
        if pp.get('kind') == 'tconv':
            self._conv_wgrad_tconv(c, dz, kern, xs, acc)
            return
        if pp.get('kind') == 'sconv':
            self._conv_wgrad_sconv(c, dz, kern, xs, acc, fused_bias)
            return
        dw2 = self.new(*kern.shape)
        have_db = c.k in self.phase_db
        db2 = self.phase_db[c.k] if have_db else (self.new(n_out) if lay.bias is not None else None)
        wkey, bkey = self.key('wgrad', c.k), self.key('bias', c.k)

        def derived_grads():
            ops.conv2d_bwd_weight(src, dz, dw2, d, xs, ws_key=wkey)
            if db2 is not None and not have_db:
                ops.bias_grad(dz, db2, n_out, ws_key=bkey)
        self.lanes.run(derived_grads)

        def fold_back():
            ops.phase_weights_bwd(dw2, db2, gv(lay, 'kernel'), gv(lay, 'bias') if lay.bias is not None else None,
                                  pp['pad_top'], pp['pad_left'], accumulate=acc)
        if self.prep is not None:
            self.post.append(fold_back)          # dw2 / db2 are final only behind the deferred sums
        else:
            fold_back()

    def _conv_wgrad_tconv(self, c, dz, kern, xs, acc):
        """Conv2DTranspose: the weight gradient of its phase convolution, gathered onto the layer's kernel (a permutation: no
        sums).  The bias gradient was taken at full resolution by the interleave's adjoint (_d2sc)."""
        op, lay, d, src = c.op, c.op.layer, c.d, c.src
        gk = self.trainer._grad_view(lay, 'kernel')
        dw2 = self.new(*kern.shape)
        wkey = self.key('wgrad', c.k)
        self.lanes.run(lambda: ops.conv2d_bwd_weight(src, dz, dw2, d, xs, ws_key=wkey))

        def gather():
            ops.tconv_weights_bwd(dw2, gk, accumulate=acc)
        if self.prep is not None:
            self.post.append(gather)             # dw2 is final only behind the deferred sums
        else:
            gather()

    def _conv_wgrad_sconv(self, c, dz, kern, xs, acc, fused_bias):
        """Conv2D(strides=2): the weight gradient of its convolution on the space-to-depth image, gathered onto the layer's kernel (a
        permutation: no sums); the bias gradient is the ordinary one (the bias is the layer's own)."""
        op, lay, d, src = c.op, c.op.layer, c.d, c.src
        gv = self.trainer._grad_view
        gk = gv(lay, 'kernel')
        dw2 = self.new(*kern.shape)
        wkey = self.key('wgrad', c.k)
        self.lanes.run(lambda: ops.conv2d_bwd_weight(src, dz, dw2, d, xs, ws_key=wkey))

        def gather():
            ops.sconv_weights_bwd(dw2, gk, accumulate=acc)
        if self.prep is not None:
            self.post.append(gather)             # dw2 is final only behind the deferred sums
        else:
            gather()
        if lay.bias is None or fused_bias:
            return
        gb = gv(lay, 'bias')
        if acc:
            tmp = torch.empty_like(gb)
            ops.bias_grad(dz, tmp, lay.filters)
            ops.axpby(tmp, gb, 1.0, 1.0)
        else:
            bkey = self.key('bias', c.k)
            self.lanes.run(lambda: ops.bias_grad(dz, gb, lay.filters, ws_key=bkey))

    def _conv_dgrad(self, c, dz, kern, xs):
        """The data gradient: its convolution, the pair's close behind it, then the adjoint of how the layer read its source."""
        pb = self.prep['bwd'].get(c.k) if self.prep is not None else None     # (prepared operand, for the stored tensor?)
        if c.op.src_mode == P.SRC_DIRECT:
            self._dgrad_direct(c, dz, kern, xs, pb)
        else:
            self._dgrad_resampled(c, dz, kern, xs, pb)

    def _dgrad_direct(self, c, dz, kern, xs, pb):
        """In place into the layer's channel window of the source's gradient -- or, where that window already holds a gradient,
        into a tensor of its own that is then added."""
        op, d, book = c.op, c.d, self.book
        cin = op.xs[0]
        g = book.grad_of(op.src)
        tmp = None
        if book.overlaps(op.src, op.in_c_off, cin):
            dd = ops.make_conv(d.cout, d.kh, d.kw, (d.dil_h, d.dil_w), d.halo, d.act, 0, 0, d.out_c_off, d.out_c_total,
                               d.src_mode)
            tmp = self.new(self.n, cin, *c.src.shape[2:])
            ops.conv2d_bwd_data(dz, kern, dd, xs, tmp)
        elif not self._dgrad_with_act(c, dz, kern, xs, g, pb):
            ops.conv2d_bwd_data(dz, kern, d, xs, g, prepared=pb[0] if pb else None)
        self.pair_close()
        if tmp is None:
            book.written.setdefault(op.src, []).append((op.in_c_off, cin))
        else:
            book.deposit(op.src, op.in_c_off, cin, tmp)

    def _dgrad_with_act(self, c, dz, kern, xs, g, pb):
        """Where this layer is the only reader of another Conv2D's activation output: the gradient already times act'(that
        output), with that layer's bias gradient from the same pass (DLWP_DGRAD_ACT=1, Trainer._dgrad_act_ops).  Returns
        whether it ran."""
        kp = self.trainer._dgrad_act_ops().get(c.k)
        if kp is None:
            return False
        pop = self.plan.ops[kp]
        done = ops.conv2d_bwd_data_act(dz, kern, c.d, xs, g, c.src, pop.act, self.trainer._grad_view(pop.layer, 'bias'),
                                       prepared=pb[0] if pb else None, ws_key=self.key('dact', c.k))
        if done:
            self.preact.add(c.op.src)
        return done

    def _dgrad_resampled(self, c, dz, kern, xs, pb):
        """The layer read UpSampling2D(2) or MaxPooling2D(2) of its source: the gradient of the resampled tensor, then the
        resampling's adjoint.  The 2x2 sum of the up-sampling's adjoint is fused into the data-gradient kernel where it can be."""
        op, d, src = c.op, c.d, c.src
        cin, n = op.xs[0], self.n
        up = op.src_mode == P.SRC_UPSAMPLE2
        fused = False
        if up:
            dense = self.new(n, cin, op.xs[1], op.xs[2])
            if pb is not None and pb[1]:
                ops.conv2d_bwd_data(dz, kern, d, xs, dense, prepared=pb[0], stored=True)
                fused = True
            elif pb is None:
                fused = ops.conv2d_bwd_data_stored(dz, kern, d, xs, dense)
        if not fused:
            tmp = self.new(n, cin, *((2 * op.xs[1], 2 * op.xs[2]) if up else (op.xs[1] // 2, op.xs[2] // 2)))
            ops.conv2d_bwd_data(dz, kern, d, xs, tmp, prepared=pb[0] if pb else None)
        self.pair_close()
        if not fused and up:
            dense = ops.upsample2_bwd(tmp)
        elif not fused:
            xw = src
            if not (op.in_c_off == 0 and cin == src.shape[1]):     # the pooling's argmax needs the window the layer read
                xw = self.new(n, cin, *src.shape[2:])
                ops.copy_channels(src, xw, cin, op.in_c_off, 0)
            dense = ops.maxpool2_bwd(xw, tmp)
        self.book.deposit(op.src, op.in_c_off, cin, dense)

    # -- the other kinds ----------------------------------------------------------------------------------------------- #
    def _d2s(self, c):
        """adjoint of the depth-to-space interleave of a restated decoder layer"""
        op = c.op
        self.book.set(op.src, ops.space_to_depth2(c.gD, op.xs[0], c_off=op.out_c_off), 4 * op.xs[0])

    def _d2sc(self, c):
        """Conv2DTranspose behind its phase convolution: activation backward and the bias gradient on the layer's full-resolution
        output (dz in place of dy), then the adjoint of the cropping interleave -- every element of the phase gradient is written,
        +0 where the crop dropped it.  The convolution in front finds a pre-activation gradient and a finished bias gradient."""
        op, lay, gD = c.op, c.op.layer, c.gD
        y = self.book.tensor(op.dst)
        f = op.xs[0]
        if lay.bias is not None:
            gb = self.trainer._grad_view(lay, 'bias')
            if lay.activation != 'linear':
                ops.act_bwd_bias_grad(y, gD, op.act, gb, f, c_off=op.out_c_off, out=gD, ws_key=self.key('bias', c.k))
            else:
                ops.bias_grad(gD, gb, f, c_off=op.out_c_off, ws_key=self.key('bias', c.k))
        elif lay.activation != 'linear':
            ops.act_bwd(y, gD, op.act, out=gD)
        dph = ops.space_to_depth2_fill(gD, f, op.xs[1], op.xs[2], op.crop[0], op.crop[1], c_off=op.out_c_off)
        self.book.set(op.src, dph, 4 * f)
        self.preact.add(op.src)

    def _s2dp(self, c):
        """The padded space-to-depth in front of a Conv2D(strides=2): its adjoint folds the halo back and re-interleaves in one
        pass; every element of the layer's channel window is written."""
        op = c.op
        if op.src == P.STATE_IN:
            return
        cin, book = op.xs[0], self.book
        hh, ww, (hp, wp), halo = op.xs[1], op.xs[2], op.out_shape[1:], op.halo
        ph, pw = hh + halo.top + halo.bottom, ww + halo.left + halo.right
        sums = ((halo.mode_h != P.PAD_ZERO and (halo.top or halo.bottom)) or
                (halo.mode_w != P.PAD_ZERO and (halo.left or halo.right)))
        if sums and 2 * hp >= ph and 2 * wp >= pw and os.environ.get('DLWP_SCONV_FUSED_ADJOINT', '0') != '1':
            # a halo that folds back (wrap, edge, mirror) over a phase tensor that covers the padded image: the two existing launches
            # -- interleave to the padded gradient, then the halo's adjoint -- are 1.3 - 1.7 x faster than the fused gather, whose
            # border lanes hold their waves up.  DLWP_SCONV_FUSED_ADJOINT=1 keeps the fused kernel (A/B runs).
            dpad = ops.depth_to_space2_crop(c.gD, cin, 0, 0, ph, pw)
            book.deposit(op.src, op.in_c_off, cin, ops.pad2d_bwd(dpad, (self.n, cin, hh, ww), c.d))
            return
        # a channel window that holds no gradient yet: the kernel writes it in place (every element of the window); the whole
        # tensor (adopted without a copy where it is the first gradient) or a window that holds one: dense, then deposited
        g = book.claim_window(op.src, op.in_c_off, cin) if not (op.in_c_off == 0 and cin == c.src.shape[1]) else None
        if g is not None:
            ops.space_to_depth2_pad_bwd(c.gD, cin, hh, ww, c.d, out=g.view((self.n, -1, hh, ww)), c_off=op.in_c_off)
        else:
            book.deposit(op.src, op.in_c_off, cin, ops.space_to_depth2_pad_bwd(c.gD, cin, hh, ww, c.d))

    def _sep_act_bias(self, c, channels):
        """dy -> dz in place and the bias gradient of the stage that owns the layer's bias and activation (the existing
        dlwp_act_bwd / dlwp_act_bwd_bias_grad / dlwp_bias_grad passes)"""
        op, lay, gD = c.op, c.op.layer, c.gD
        y = self.book.tensor(op.dst)
        gv = self.trainer._grad_view
        if lay.activation != 'linear' and lay.bias is not None:
            ops.act_bwd_bias_grad(y, gD, op.act, gv(lay, 'bias'), channels, out=gD, ws_key=self.key('bias', c.k))
            return
        if lay.activation != 'linear':
            ops.act_bwd(y, gD, op.act, out=gD)
        if lay.bias is not None:
            gb, bkey = gv(lay, 'bias'), self.key('bias', c.k)
            self.lanes.run(lambda: ops.bias_grad(gD, gb, channels, ws_key=bkey))

    def _pwconv(self, c):
        """The 1 x 1 stage of a SeparableConv2D: activation and bias gradient, the pointwise kernel's gradient on a side lane (it reads
        the intermediate tensor the training plan keeps), then the gradient of that intermediate tensor"""
        op, lay, d, gD, src = c.op, c.op.layer, c.d, c.gD, c.src
        self._sep_act_bias(c, lay.filters)
        gw, wkey = self.trainer._grad_view(lay, 'pointwise_kernel'), self.key('wgrad', c.k)
        self.lanes.run(lambda: ops.pointwise2d_bwd_weight(src, gD, gw, d, ws_key=wkey))
        self.touched.add(id(lay))
        self.book.deposit(op.src, 0, op.xs[0], ops.pointwise2d_bwd_data(gD, lay.pointwise_kernel, d))

    def _dwconv(self, c):
        """The depthwise stencil (DepthwiseConv2D, or the first stage of a SeparableConv2D, which has no bias / activation of its
        own): the kernel's gradient on a side lane, then -- not for the model input -- the adjoint in the input, halo included,
        written in place into the layer's channel window where that holds no gradient yet"""
        op, lay, d, gD, src = c.op, c.op.layer, c.d, c.gD, c.src
        cin, hh, ww = op.xs
        if not isinstance(lay, L.SeparableConv2D):
            self._sep_act_bias(c, cin * lay.depth_multiplier)
        gk, wkey = self.trainer._grad_view(lay, 'depthwise_kernel'), self.key('wgrad', c.k)
        self.lanes.run(lambda: ops.depthwise2d_bwd_weight(src, gD, gk, d, ws_key=wkey))
        self.touched.add(id(lay))
        if op.src == P.STATE_IN:       # (a first layer: nobody needs the gradient of the model input)
            return
        book = self.book
        whole = op.in_c_off == 0 and cin == src.shape[1]
        g = book.claim_window(op.src, op.in_c_off, cin) if not whole else None
        if g is not None:
            ops.depthwise2d_bwd_data(gD, lay.depthwise_kernel, d, hh, ww, out=g.view((self.n, -1, hh, ww)))
        else:
            book.deposit(op.src, op.in_c_off, cin, ops.depthwise2d_bwd_data(gD, lay.depthwise_kernel, d, hh, ww))

    def _crop(self, c):
        """Cropping2D: the gradient is zero padding"""
        if c.op.src != P.STATE_IN:
            self.book.deposit(c.op.src, 0, c.src.shape[1], ops.pad2d(c.gD, c.d))

    def _rowconv(self, c):
        """RowConnected2D (reference custom.py:695-837): per-row filters"""
        op, lay, d, gD, src = c.op, c.op.layer, c.d, c.gD, c.src
        gv = self.trainer._grad_view
        n = self.n
        if lay.activation != 'linear':
            ops.act_bwd(self.book.tensor(op.dst), gD, op.act, out=gD)          # dz in place of dy
        xs = self.shape4(op)
        ops.rowconv2d_bwd_weight(src, gD, gv(lay, 'kernel'), gv(lay, 'bias') if lay.bias is not None else None, d, xs,
                                 accumulate=id(lay) in self.touched)
        self.touched.add(id(lay))
        if op.src == P.STATE_IN:
            return
        cin = op.xs[0]
        dd = ops.make_conv(d.cout, d.kh, d.kw, 1, d.halo, d.act, 0, 0, d.out_c_off, d.out_c_total)
        if op.src_mode == P.SRC_UPSAMPLE2:     # gradient of the up-sampled tensor, then the 2x2 sums of its adjoint
            up = self.new(n, cin, 2 * op.xs[1], 2 * op.xs[2])
            ops.rowconv2d_bwd_data(gD, lay.kernel, dd, _lib.Shape4(n, cin, 2 * op.xs[1], 2 * op.xs[2]), up)
            dense = ops.upsample2_bwd(up)
        else:
            dense = self.new(n, cin, *src.shape[2:])
            ops.rowconv2d_bwd_data(gD, lay.kernel, dd, xs, dense)
        self.book.deposit(op.src, op.in_c_off, cin, dense)

    def _dense(self, c):
        """keras Dense: weight and bias gradient, then (not for the model input) dx"""
        op, lay, gD, src = c.op, c.op.layer, c.gD, c.src
        gv = self.trainer._grad_view
        y = self.book.tensor(op.dst)
        ops.dense_bwd_weight(src, gD, y, gv(lay, 'kernel'), gv(lay, 'bias') if lay.bias is not None else None, op.act)
        self.touched.add(id(lay))
        if op.src == P.STATE_IN:
            return
        dx = torch.empty_like(src)
        ops.dense_bwd_data(gD, y, lay.kernel, op.act, out=dx)
        self.book.deposit(op.src, 0, src.shape[1], dx)

    def _dropout(self, c):
        """the mask of the forward: same (seed, layer, step)"""
        if c.op.src == P.STATE_IN:
            return
        lay = c.op.layer
        dx = ops.dropout_bwd(c.gD, lay.rate, lay.mask_seed, self.plan.dropout_layers.index(lay), self.ex.dropout_step)
        self.book.deposit(c.op.src, 0, c.src.shape[1], dx.view(c.src.shape))

    def _bn(self, c):
        """BatchNormalization: dgamma, dbeta and dx from the batch statistics of the forward"""
        op, lay = c.op, c.op.layer
        gv = self.trainer._grad_view
        st = self.ex.bn_state(c.k, int(self.n))
        dx = ops.batchnorm_bwd(c.src, c.gD, lay.gamma, st['mean'], st['invstd'], st['ws'],
                               dgamma=gv(lay, 'gamma') if lay.gamma is not None else None,
                               dbeta=gv(lay, 'beta') if lay.beta is not None else None,
                               want_dx=op.src != P.STATE_IN)
        self.touched.add(id(lay))
        if dx is not None:
            self.book.deposit(op.src, 0, c.src.shape[1], dx)

    def _act(self, c):
        """keras activation layers: dx = dy f'(x), f' from the layer's input, which the training plan keeps"""
        if c.op.src == P.STATE_IN:
            return
        dx = ops.activation_bwd(c.src, c.gD, *c.op.layer.eltwise)
        self.book.deposit(c.op.src, 0, c.src.shape[1], dx)

    def _merge(self, c):
        """keras merge layers: every source's gradient from one pass over the sources and dy.  Each source gets a NEW tensor, also
        where the gradient is dy itself (Add): GradBook.deposit adopts a buffer's first gradient without a copy and later adds into it
        in place, so a tensor handed to two sources would collect both sources' other gradients."""
        op, book = c.op, self.book
        srcs = [op.src] + list(op.aux)
        dxs = ops.merge_bwd(op.layer.kind, [book.tensor(b) for b in srcs], c.gD, want=[b != P.STATE_IN for b in srcs])
        for b, dx in zip(srcs, dxs):
            if dx is not None:
                book.deposit(b, 0, dx.shape[1], dx)

    def _lstm(self, c):
        op, gD, book = c.op, c.gD, self.book
        zh_i, cp_i, co_i = op.aux
        f = op.xs[0]
        if not book.covered(op.dst, op.out_c_off, f):
            if book.overlaps(op.dst, op.out_c_off, f):
                raise NotImplementedError('ConvLSTM2D output used through partially overlapping channel windows')
            book.deposit(op.dst, op.out_c_off, f, torch.zeros((self.n, f) + tuple(gD.shape[2:]), dtype=torch.float32,
                                                              device=self.device))   # this h_t feeds nothing downstream
        dz, dcp = ops.convlstm_gates_bwd(c.src, book.tensor(zh_i) if zh_i is not None else None,
                                         book.tensor(cp_i) if cp_i is not None else None, book.tensor(co_i), gD,
                                         book.grads.get(co_i), f, h_c_off=op.out_c_off, act=op.act, rec_act=op.rec_act)
        book.set(op.src, dz, 4 * f)
        if zh_i is not None:
            book.set(zh_i, dz, 4 * f)          # z = zx + zh: the same gradient flows into both convolutions
        if cp_i is not None:
            book.set(cp_i, dcp, f)

    def _copy(self, c):
        op, gD = c.op, c.gD
        if op.src == P.STATE_IN:
            return
        ch = op.xs[0]
        gw = self.new(self.n, ch, *gD.shape[2:])
        ops.copy_channels(gD, gw, ch, op.out_c_off, 0)
        self.book.deposit(op.src, op.in_c_off, ch, gw)

    def _pad(self, c):
        op, gD, n = c.op, c.gD, self.n
        if op.src == P.STATE_IN:
            return
        if op.inner > 1:
            dense = ops.pad2d_bwd(gD.reshape((n, gD.shape[1], gD.shape[2], -1)) if gD.dim() == 4 else gD,
                                  (n, op.xs[1], op.xs[2], op.inner), c.d, channels_last=True)
        else:
            dense = ops.pad2d_bwd(gD, (n,) + tuple(op.xs), c.d)
        self.book.deposit(op.src, 0, c.src.shape[1], dense)

    def _maxpool(self, c):
        op, book = c.op, self.book
        if op.src == P.STATE_IN:
            return
        if op.src >= 0 and op.src not in book.grads and op.src not in book.pending_pool:
            book.pending_pool[op.src] = c.gD      # (left to the convolution that wrote the source, where it can take it)
        else:
            book.deposit(op.src, 0, c.src.shape[1], ops.maxpool2_bwd(c.src, c.gD))

    def _avgpool(self, c):
        """AveragePooling2D(2): 0.25 * dy to every element of a window, written in one pass (no part in pending_pool: the fused
        pooling backward of the convolutions is max-pooling's)."""
        if c.op.src != P.STATE_IN:
            self.book.deposit(c.op.src, 0, c.src.shape[1], ops.avgpool2_bwd(c.gD, c.src.shape))

    def _upsample(self, c):
        if c.op.src != P.STATE_IN:
            self.book.deposit(c.op.src, 0, c.src.shape[1], ops.upsample2_bwd(c.gD))

    def _bilinear(self, c):
        """UpSampling2D(2, interpolation='bilinear'): the adjoint of the interpolation in gather form, written in one pass."""
        if c.op.src != P.STATE_IN:
            self.book.deposit(c.op.src, 0, c.src.shape[1], ops.upsample2_bilinear_bwd(c.gD, c.src.shape))

    adjoints = {'d2s': _d2s, 'conv': _conv, 'rowconv': _rowconv, 'dense': _dense, 'dropout': _dropout, 'bn': _bn,
                'lstm': _lstm, 'copy': _copy, 'pad': _pad, 'maxpool': _maxpool, 'avgpool': _avgpool, 'upsample': _upsample,
                'bilinear': _bilinear, 'act': _act, 'merge': _merge, 'd2sc': _d2sc, 'crop': _crop, 's2dp': _s2dp, 'dwconv': _dwconv,
                'pwconv': _pwconv}
