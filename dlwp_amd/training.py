"""
The train step behind model.fit / fit_generator / evaluate: forward (activations stay in the plan's buffers), 'mse'
loss + 'mae' metric, backward through the fused plan (dlwp_conv2d_bwd_data / _bwd_weight, activation / pooling /
up-sampling / halo adjoints), Keras-form Adam on ONE flat parameter buffer, and -- under torch.distributed -- one
all-reduce of ONE flat gradient buffer per step (RCCL over xGMI on the GPU box, gloo in the CPU tests).

Reference: keras Model.fit / fit_generator / evaluate as driven by DLWP/model/models.py:188-228, 303-316 and
examples/train.py:240,258-263,274; loss / metric / optimizer strings of examples/train.py:240.
"""
import contextlib
import ctypes
import gc
import os
import time

import numpy as np
import torch

from . import layers as L
from . import plan as P
from .custom import Callback, History


# ------------------------------------------------------------------------------------------------------------------ #
# optimizers (hyper-parameter holders; the update itself is a HIP kernel over the flat buffers)
# ------------------------------------------------------------------------------------------------------------------ #

class Optimizer(object):
    """keras.optimizers.Optimizer: `clipnorm` / `clipvalue` are the only keywords beyond a class's own (Keras raises TypeError for
    any other, and so does this); like Keras the two attributes exist only where they were passed.  The update is
    dlwp_optimizer_step of kind `step_kind()` on `n_slots()` flat slot buffers, in Keras' weight order (include/dlwp_hip.h)."""

    def __init__(self, lr, decay, **kwargs):
        for k in kwargs:
            if k not in ('clipnorm', 'clipvalue'):
                raise TypeError('Unexpected keyword argument passed to optimizer: ' + str(k))
        self.lr, self.decay = float(lr), float(decay)
        self.iterations = 0
        for k, v in kwargs.items():
            if v is not None:
                setattr(self, k, float(v))

    def clips(self):
        """(clipnorm, clipvalue), 0 where Keras would not clip"""
        cn, cv = float(getattr(self, 'clipnorm', 0.0)), float(getattr(self, 'clipvalue', 0.0))
        return (cn if cn > 0 else 0.0), (cv if cv > 0 else 0.0)

    def legacy_kernel(self):
        """True: the update is dlwp_adam_keras / dlwp_sgd_keras, as before the other optimizers existed"""
        return False

    def n_slots(self):
        from . import ops
        return ops.OPT_SLOTS[self.step_kind()]

    def step_depends_on_iteration(self):
        """does a launch argument of the update change from step to step (such a step is never replayed)?"""
        return self.decay != 0.0

    def step_args(self):
        """keyword arguments of ops.optimizer_step beyond kind, buffers, iteration, grad_scale and clipping"""
        raise NotImplementedError

    def after_step(self):
        self.iterations += 1


class Adam(Optimizer):
    """keras.optimizers.Adam (Keras 2.2 form: epsilon outside the sqrt, bias correction folded into lr_t)."""

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0., amsgrad=False, **kwargs):
        super(Adam, self).__init__(lr, decay, **kwargs)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)      # K.epsilon()
        self.amsgrad = bool(amsgrad)

    def legacy_kernel(self):
        return not self.amsgrad and self.clips() == (0.0, 0.0)

    def step_kind(self):
        from . import ops
        return ops.OPT_ADAM_AMSGRAD if self.amsgrad else ops.OPT_ADAM

    def step_depends_on_iteration(self):
        return True      # lr_t

    def step_args(self):
        return dict(lr=self.lr, decay=self.decay, h1=self.beta_1, h2=self.beta_2, epsilon=self.epsilon)


class SGD(Optimizer):
    def __init__(self, lr=0.01, momentum=0., decay=0., nesterov=False, **kwargs):
        super(SGD, self).__init__(lr, decay, **kwargs)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)

    def legacy_kernel(self):
        return not self.nesterov and self.clips() == (0.0, 0.0)

    def step_kind(self):
        from . import ops
        return ops.OPT_SGD_NESTEROV if self.nesterov else ops.OPT_SGD

    def step_args(self):
        return dict(lr=self.lr, decay=self.decay, h1=self.momentum)


class RMSprop(Optimizer):
    """keras.optimizers.RMSprop: a <- rho a + (1 - rho) g^2; p -= lr' g / (sqrt(a) + eps)"""

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0., **kwargs):
        super(RMSprop, self).__init__(lr, decay, **kwargs)
        self.rho = float(rho)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def step_kind(self):
        from . import ops
        return ops.OPT_RMSPROP

    def step_args(self):
        return dict(lr=self.lr, decay=self.decay, h1=self.rho, epsilon=self.epsilon)


class Adagrad(Optimizer):
    """keras.optimizers.Adagrad: a <- a + g^2; p -= lr' g / (sqrt(a) + eps)"""

    def __init__(self, lr=0.01, epsilon=None, decay=0., **kwargs):
        super(Adagrad, self).__init__(lr, decay, **kwargs)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def step_kind(self):
        from . import ops
        return ops.OPT_ADAGRAD

    def step_args(self):
        return dict(lr=self.lr, decay=self.decay, epsilon=self.epsilon)


class Adadelta(Optimizer):
    """keras.optimizers.Adadelta: slots a (squared gradients), d (squared updates)"""

    def __init__(self, lr=1.0, rho=0.95, epsilon=None, decay=0., **kwargs):
        super(Adadelta, self).__init__(lr, decay, **kwargs)
        self.rho = float(rho)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def step_kind(self):
        from . import ops
        return ops.OPT_ADADELTA

    def step_args(self):
        return dict(lr=self.lr, decay=self.decay, h1=self.rho, epsilon=self.epsilon)


class Adamax(Optimizer):
    """keras.optimizers.Adamax: slots m, u (the exponentially weighted infinity norm)"""

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0., **kwargs):
        super(Adamax, self).__init__(lr, decay, **kwargs)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def step_kind(self):
        from . import ops
        return ops.OPT_ADAMAX

    def step_depends_on_iteration(self):
        return True

    def step_args(self):
        return dict(lr=self.lr, decay=self.decay, h1=self.beta_1, h2=self.beta_2, epsilon=self.epsilon)


def nadam_schedule(beta_1, schedule_decay, iteration, m_schedule):
    """(mu_t, mu_{t+1}, ms_new, ms_next) of Keras' Nadam before step `iteration` -- double arithmetic on the float32-rounded
    hyper-parameters, the same expressions dlwp_optimizer_step evaluates"""
    import math
    b1, sd = float(np.float32(beta_1)), float(np.float32(schedule_decay))
    t = float(iteration) + 1.0
    mu_t = b1 * (1.0 - 0.5 * math.pow(0.96, t * sd))
    mu_t1 = b1 * (1.0 - 0.5 * math.pow(0.96, (t + 1.0) * sd))
    ms_new = float(m_schedule) * mu_t
    return mu_t, mu_t1, ms_new, ms_new * mu_t1


class Nadam(Optimizer):
    """keras.optimizers.Nadam: slots m, v; `m_schedule` (the running product of the momentum schedule, 1 before the first step) is a
    host scalar that the npz archive keeps and a Keras HDF5 file does not (Keras re-starts it at 1 too)."""

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=None, schedule_decay=0.004, **kwargs):
        super(Nadam, self).__init__(lr, 0.0, **kwargs)
        del self.decay                     # (Keras' Nadam has none)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)
        self.schedule_decay = float(schedule_decay)
        self.m_schedule = 1.0

    def step_kind(self):
        from . import ops
        return ops.OPT_NADAM

    def step_depends_on_iteration(self):
        return True

    def step_args(self):
        return dict(lr=self.lr, h1=self.beta_1, h2=self.beta_2, epsilon=self.epsilon, schedule_decay=self.schedule_decay,
                    m_schedule=self.m_schedule)

    def after_step(self):
        self.m_schedule = nadam_schedule(self.beta_1, self.schedule_decay, self.iterations, self.m_schedule)[2]
        self.iterations += 1


_OPTIMIZERS = {'sgd': SGD, 'rmsprop': RMSprop, 'adagrad': Adagrad, 'adadelta': Adadelta, 'adam': Adam, 'adamax': Adamax,
               'nadam': Nadam}


def get_optimizer(spec):
    if isinstance(spec, Optimizer):
        return spec
    if isinstance(spec, str):
        if spec.lower() not in _OPTIMIZERS:
            raise ValueError('Could not interpret optimizer identifier: %r (%s are known)' % (spec, ', '.join(sorted(_OPTIMIZERS))))
        return _OPTIMIZERS[spec.lower()]()
    raise TypeError('optimizer must be a name or a dlwp_amd.training.Optimizer instance')


def mean_squared_error(y_true, y_pred):  # marker objects accepted as loss= (the reference passes keras.losses.mean_squared_error)
    raise RuntimeError('marker only: pass it as loss=, the HIP loss kernel computes it')


def mean_absolute_error(y_true, y_pred):
    raise RuntimeError('marker only')


def mean_absolute_percentage_error(y_true, y_pred):
    raise RuntimeError('marker only')


def mean_squared_logarithmic_error(y_true, y_pred):
    raise RuntimeError('marker only')


def logcosh(y_true, y_pred):
    raise RuntimeError('marker only')


def _loss_name(loss):
    """'mse' (dlwp_mse_mae), 'custom' (a LossSpec) or 'elementwise' (another Keras regression loss: dlwp_loss_elementwise)."""
    from .custom import LossSpec, loss_kind
    if isinstance(loss, LossSpec):
        return 'custom'
    kind = loss_kind(loss)
    if kind == 0:
        return 'mse'
    if kind is not None:
        return 'elementwise'
    raise NotImplementedError("loss %r is not implemented on the HIP path ('mse', 'mae', 'mape', 'msle', 'logcosh' and their "
                              "Keras names, dlwp_amd.custom.anomaly_correlation_loss(...), latitude_weighted_loss(...) and "
                              "LatitudeWeightedLoss(...) are)" % (loss,))


_METRIC_NAMES = {'mae': 'mean_absolute_error', 'mean_absolute_error': 'mean_absolute_error',
                 'mse': 'mean_squared_error', 'mean_squared_error': 'mean_squared_error'}


def _metric_entry(m):
    """(log name, what) of one metrics= entry: what = ('kind', k) for a Keras regression loss, ('acc',) for
    custom.anomaly_correlation, ('spec', LossSpec) for a loss object of this package."""
    from . import custom as C
    if isinstance(m, C.LossSpec):
        return m.__name__, ('spec', m)
    if m is C.anomaly_correlation or m == 'anomaly_correlation':
        return 'anomaly_correlation', ('acc',)
    kind = C.loss_kind(m)
    if kind is None:
        raise NotImplementedError('metric %r is not implemented (mse, mae, mape, msle, logcosh, anomaly_correlation and the '
                                  'loss objects of dlwp_amd.custom are)' % (m,))
    return C.KIND_NAMES[kind], ('kind', kind)


# ------------------------------------------------------------------------------------------------------------------ #
# flat parameter storage
# ------------------------------------------------------------------------------------------------------------------ #

def flatten_parameters(model):
    """Re-home every TRAINABLE layer weight as a view into one contiguous fp32 buffer (values preserved).  Returns the buffer
    and [(layer, name, offset, numel, shape)].  Non-trainable weights (the moving statistics of BatchNormalization,
    layer.non_trainable_names) stay where they are: Adam never updates them and the gradient exchange never carries them."""
    entries, total = [], 0
    seen = set()
    for lay in model.layers:
        if id(lay) in seen:
            continue
        seen.add(id(lay))
        for name, w in lay._weights:
            if name in getattr(lay, 'non_trainable_names', ()):
                continue
            entries.append((lay, name, total, w.numel(), tuple(w.shape)))
            total += w.numel()
    flat = torch.empty(max(total, 1), dtype=torch.float32, device=model.device)
    for lay, name, off, numel, shape in entries:
        old = dict(lay._weights)[name]
        view = flat[off:off + numel].view(shape)
        view.copy_(old)
        setattr(lay, name, view)
        lay._weights = [(nm, view if nm == name else t) for nm, t in lay._weights]
    return flat, entries


# ------------------------------------------------------------------------------------------------------------------ #
# trainer
# ------------------------------------------------------------------------------------------------------------------ #

class _StepHandle(object):
    """Owner of a dlwp_train_step_t (csrc/tape.hip)."""

    def __init__(self, h):
        self.h = h

    def close(self):
        from . import _lib
        if self.h is not None:
            _lib.lib.dlwp_train_step_destroy(self.h)
            self.h = None

    def __del__(self):      # (never destroys here: _lib.bury)
        try:
            from . import _lib
            _lib.bury('step', self.h)
            self.h = None
        except Exception:  # noqa: BLE001
            pass


@contextlib.contextmanager
def _no_gc():
    """No garbage collection while a step is recorded or captured: a collection cycle that finalises an OLD model's memory pool,
    graphs, streams, events or device memory (hipGraphExecDestroy, hipStreamDestroy, hipFree ...) inside the recording's
    use_mem_pool block or in the middle of a capture aborts the process or leaves a graph that crashes at launch (r3: seen as
    'Fatal Python error: Aborted ... Garbage-collecting' inside _capture_step and under dlwp_stream_wait, and as segmentation
    faults in replay, 3 of 7 full test runs, once small steps were captured by default).  Collects first."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class _PhaseGrad(object):
    """The loss gradient of an output the plan produces as phase channels + depth-to-space, in phase layout: the gradient of
    plan buffer `buf` (written by convolution op `conv_k`); db: the bias gradient of the phase channels, or None."""

    def __init__(self, buf, conv_k, dz, db):
        self.buf, self.conv_k, self.dz, self.db = buf, conv_k, dz, db


class Trainer(object):
    def __init__(self, model):
        self.model = model
        self.plan = model.plan
        self.device = model.device
        self.loss_kind = _loss_name(model.loss)
        n_out = len(model.outputs)
        lw = model.loss_weights
        if lw is None:
            lw = [1.0] * n_out
        if isinstance(lw, dict):
            raise NotImplementedError('loss_weights as a dict')
        if len(lw) != n_out:
            raise ValueError('loss_weights has %d entries for %d outputs' % (len(lw), n_out))
        self.loss_weights = [float(v) for v in lw]
        self.metric_keys = []
        metrics = []
        for m in model.metrics:
            key, what = _metric_entry(m)
            self.metric_keys.append(key)
            metrics.append(what)
        self._plan_loss_table(metrics)
        out_names = [t.layer.name for t in model.outputs]
        if n_out == 1:
            self.metrics_names = ['loss'] + list(self.metric_keys)
        else:
            self.metrics_names = (['loss'] + ['%s_loss' % nm for nm in out_names] +
                                  ['%s_%s' % (nm, mk) for nm in out_names for mk in self.metric_keys])
        self.flat_params, self.entries = flatten_parameters(model)
        # gradients + (behind them) the [n_out, 7] loss table of a data-parallel step: ONE buffer, ONE all-reduce
        n_par = self.flat_params.numel()
        nc = self.n_cols
        n_x = -(-(n_par + nc * n_out) // 4) * 4       # (whole float4: the library's own exchange moves 16-byte units)
        self._flat_exchange = torch.zeros(n_x, dtype=torch.float32, device=self.device)
        self.flat_grads = self._flat_exchange[:n_par]
        self._loss_tail = self._flat_exchange[n_par:n_par + nc * n_out].view(n_out, nc)
        self.opt_state = None
        self.dp = getattr(model, '_dp', None)
        self._grad_bufs = {}
        self._loss_out = None
        self._phase_out = None        # _phase_outputs(): outputs whose loss is taken on the phase channels
        self._dact_ops = None         # _dgrad_act_ops(): data gradients that carry the producer's activation backward
        self._loss_consts = None      # device copies of a custom loss's climatology / latitude weights
        self._params_dirty = False    # set by Model.set_weights / load: replicas re-align at the next collective step
        self._graphs = {}             # (n_local, n_global) -> captured training step (see _graph_step)
        self._graph_seen = {}
        self._iter_dev = None         # Adam's step number on the device (advanced inside the captured step)
        self._iter_shadow = None
        self._clip_out = None         # {factor, norm, norm^2} of the clipnorm pass, on the device (see _optimizer_step)
        self._fold = None             # see _fold_ok
        self._prep_cache = {}         # batch size -> prepared weights of the step (see _prepare_step)
        self._side = None             # second stream: the weight gradients run beside the data-gradient chain
        self._loader_threads = 0      # > 0 while fit_generator feeds through a DeviceLoader (see _graph_ok)
        self._foreign = False         # set where a step launches through torch instead of the library (see _record_step)
        self._no_tape = set()         # step shapes whose recording was refused
        # the moving statistics a training forward updates in place (BatchNormalization): part of the state a recorded step is
        # validated on (see _validate_step)
        self._bn_stats = [t for lay in self.plan.bn_layers for t in (lay.moving_mean, lay.moving_variance)]
        self.sync_parameters()

    # -- the loss table ------------------------------------------------------------------------------------------------ #
    def _plan_loss_table(self, metrics):
        """Columns of the per-output loss table: 0 the loss value of a custom / elementwise loss, 1 mse, 2 mae, 3-6 the custom
        loss's sums (as before); then the columns of ONE dlwp_loss_metrics pass (the kinds the loss kernel does not leave in 1 / 2,
        in kind order, then mean(p t), mean(p^2), mean(t^2) for anomaly_correlation); then one column per elementwise LossSpec
        metric and seven per dlwp_loss_custom LossSpec metric.  Only today's metrics: the table stays 7 columns wide."""
        from . import _lib, ops
        spec = self.model.loss if self.loss_kind == 'custom' else None
        # (kind, row weights, scale) of a loss lowered to dlwp_loss_elementwise; None: dlwp_mse_mae / dlwp_loss_custom as before
        if self.loss_kind == 'elementwise':
            from .custom import loss_kind
            self._ew = (loss_kind(self.model.loss), None, 1.0)
        elif spec is not None and spec.kind == 0 and spec.inner:
            self._ew = (spec.inner, spec.row_weights, spec.scale)
        else:
            self._ew = None
        have = {0: 1, 1: 2} if self._ew is None else {}       # kinds the loss kernel already leaves in the table (mse, mae)
        mask = 0
        for what in metrics:
            if what[0] == 'kind' and what[1] not in have:
                mask |= 1 << what[1]
            elif what[0] == 'acc':
                mask |= _lib.METRIC_ACC_SUMS | (0 if 0 in have else 1 << _lib.LOSS_MSE)
        col = dict(have)
        c = 7
        for k in range(5):
            if mask & (1 << k):
                col[k] = c
                c += 1
        acc_col = c if mask & _lib.METRIC_ACC_SUMS else None
        c += ops.metric_columns(mask) - ops.metric_columns(mask & 0x1f)
        self._metric_mask = mask
        self._metric_cols = []          # per metric: ('col', c) | ('acc', mse column, first sum column) | ('spec', c, spec)
        self._spec_metrics = []         # (first column, LossSpec)
        self._batch_stat = False        # a metric that is a whole-batch statistic: epoch logs average per-batch values
        for what in metrics:
            if what[0] == 'kind':
                self._metric_cols.append(('col', col[what[1]]))
            elif what[0] == 'acc':
                self._metric_cols.append(('acc', col[0], acc_col))
                self._batch_stat = True
            else:
                ms = what[1]
                self._spec_metrics.append((c, ms))
                self._metric_cols.append(('spec', c, ms))
                if ms.kind == 0 and ms.inner:
                    c += 1
                else:
                    c += 7
                    self._batch_stat = self._batch_stat or ms.kind == 1
        self.n_cols = c
        self._spec_consts = {}

    def _device_consts(self, spec):
        got = self._spec_consts.get(id(spec))
        if got is None:
            mean = None if spec.mean is None else torch.from_numpy(spec.mean).to(self.device).contiguous()
            roww = None if spec.row_weights is None else torch.from_numpy(spec.row_weights).to(self.device).contiguous()
            got = self._spec_consts[id(spec)] = (mean, roww, spec)
        return got[0], got[1]

    def _metric_passes(self, o, yp, yt, phase=False):
        """The metric columns of output o that the loss kernel did not fill: one dlwp_loss_metrics pass, then the LossSpec
        metrics (no gradient)."""
        from . import ops
        row = self._loss_out[o]
        if self._metric_mask:
            ops.loss_metrics(yp, yt, row[7:7 + ops.metric_columns(self._metric_mask)], self._metric_mask, phase=phase,
                             ws_key=o)
        for c, ms in self._spec_metrics:
            mean, roww = self._device_consts(ms)
            yp4, yt4 = self._as4(yp, roww), self._as4(yt, roww)
            if roww is not None and roww.numel() != yp4.shape[2]:
                raise ValueError('latitude weights have %d rows, the model output %d' % (roww.numel(), yp4.shape[2]))
            if mean is not None and mean.numel() != yp4[0].numel():
                raise ValueError('anomaly_correlation_loss mean has %d elements, the model output %d per sample'
                                 % (mean.numel(), yp4[0].numel()))
            if ms.kind == 0 and ms.inner:
                ops.loss_elementwise(yp4, yt4, row[c:c + 1], None, 1.0, ms.inner, roww, ws_key=('metric', o, c))
            else:
                ops.loss_custom(yp4, yt4, row[c:c + 7], None, 1.0, mean, roww, ms.kind, ms.regularize)

    @staticmethod
    def _as4(y, roww=None):
        if y.dim() == 4:
            return y
        if roww is not None:
            raise NotImplementedError('latitude-weighted losses need (n, c, h, w) outputs')
        return y.reshape(y.shape[0], -1, 1, 1)

    # -- replicas ------------------------------------------------------------------------------------------------------ #
    def sync_parameters(self):
        """Data parallel: every replica takes rank 0's parameters (and optimizer state).  Layers draw their initial
        weights from per-process random streams, so without this the replicas would apply the same summed gradient to
        different weights (keras.utils.multi_gpu_model has ONE weight set by construction, models.py:104-109)."""
        dp = self.dp
        self._params_dirty = False
        if dp is None or dp.world <= 1:
            return
        dp.broadcast_(self.flat_params)
        if self.opt_state is not None:
            for t in self.opt_state:
                dp.broadcast_(t)

    # -- helpers ------------------------------------------------------------------------------------------------------ #
    def _grad_view(self, layer, name):
        if isinstance(layer, L._ConvPart):       # a ConvLSTM2D convolution: the weights belong to the parent layer
            layer, name = layer.parent, (layer.which if name == 'kernel' else 'bias')
        for lay, nm, off, numel, shape in self.entries:
            if lay is layer and nm == name:
                return self.flat_grads[off:off + numel].view(shape)
        raise KeyError(name)

    def _to_device(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(self.device, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def _targets(self, y, n):
        ys = list(y) if isinstance(y, (list, tuple)) else [y]
        if len(ys) != len(self.plan.output_store):
            raise ValueError('model has %d outputs but %d target arrays were given' % (len(self.plan.output_store), len(ys)))
        out = []
        for t, store in zip(ys, self.plan.output_store):
            t = self._to_device(t)
            if t.shape[0] != n or t.numel() != n * int(np.prod(store)):
                raise ValueError('target shape %r does not match the model output %r' % (tuple(t.shape), (n,) + tuple(store)))
            out.append(t.reshape((n,) + tuple(store)))
        return out

    # -- forward + loss ------------------------------------------------------------------------------------------------ #
    # -- a step's weight-side helpers in one launch each (csrc/batch.hip) ------------------------------------------------ #
    def _fold_ok(self):
        """The folded step (default; DLWP_TRAIN_FOLD=0 keeps one launch per helper): every prepared form of the weights --
        Winograd / packed-N forms for the forward and data-gradient convolutions, the flipped kernels -- is built by ONE
        launch in front of the forward, every final sum (weight-gradient slabs, bias-gradient and loss partials) by ONE launch
        behind the backward pass, and the weight gradients run on a second stream beside the data-gradient chain.  At 8
        samples per GPU that is 64 -> ~36 launches.  Plans it covers: Conv2D layers used once each (no ConvLSTM2D /
        RowConnected2D / shared layers)."""
        if self._fold is None:
            ok = self.device.type == 'cuda' and os.environ.get('DLWP_TRAIN_FOLD', '1') != '0'
            seen = set()
            for op in self.plan.ops:
                if op.kind in ('lstm', 'rowconv') or (op.kind == 'conv' and (op.lstm_f or isinstance(op.layer, L._ConvPart))):
                    ok = False
                if op.kind == 'conv':
                    ok = ok and id(op.layer) not in seen
                    seen.add(id(op.layer))
            # every deferred sum of a step in ONE flush (csrc/common.h: DLWP_MAX_BATCH_JOBS = 24; an early flush would run on
            # whichever stream filled the table)
            n_red = len(seen) + len(self.plan.sep_layers)     # (a depthwise / separable layer defers its bias sum only)
            ok = ok and 2 * n_red + len(self.plan.output_store) <= 24 and 3 * len(seen) <= 24
            self._fold = bool(ok)
        return self._fold

    def _prepare_step(self, x):
        """Derived (phase-summed) kernels, then every prepared operand of this step's convolutions in one launch.  Returns
        {'fwd': {op index: tensor}, 'bwd': {op index: (tensor, stored)}}; the buffers are cached per batch size."""
        from . import _lib, ops
        ex = self.model.train_executor
        plan = self.plan
        n = int(x.shape[0])
        x = x.reshape((n,) + plan._in_store)
        for op in plan.ops:
            if op.kind == 'phasew':
                w2, b2 = ex.phase_buffers()[op.wparam]
                ops.phase_weights(op.layer.kernel, op.layer.bias, op.halo.top, op.halo.left, w2=w2, b2=b2)
            elif op.kind == 'tphasew':
                w2, b2 = ex.phase_buffers()[op.wparam]
                ops.tconv_weights(op.layer.kernel, op.layer.bias, w2=w2, b2=b2)
            elif op.kind == 'sphasew':
                ops.sconv_weights(op.layer.kernel, w2=ex.phase_buffers()[op.wparam][0])
        cache = self._prep_cache.get(n)
        if cache is None:
            if len(self._prep_cache) > 4:
                self._prep_cache.clear()
            cache = self._prep_cache[n] = {'fwd': {}, 'bwd': {}}
        bufs = ex.scratch(n)
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        ops.prepare_begin(self.device)
        try:
            for k, (op, d) in enumerate(zip(plan.ops, ex._descriptors())):
                if op.kind != 'conv':
                    continue
                kern = ex.conv_weights(op)[0]
                src = x if op.src == P.STATE_IN else bufs[op.src]
                dst_dtype = bufs[op.dst].dtype if op.dst >= 0 else torch.float32
                u = ops.conv2d_prepare(src, kern, d, out_dtype=dst_dtype, x_channels=op.xs[0], out=cache['fwd'].get(k))
                if u is not None:
                    cache['fwd'][k] = u
                if op.src == P.STATE_IN:
                    continue
                xs = _lib.Shape4(n, op.xs[0], op.xs[1], op.xs[2])
                old = cache['bwd'].get(k)
                stored = old[1] if old is not None else (op.src_mode == P.SRC_UPSAMPLE2 and
                                                         ops.conv2d_bwd_data_prepared_bytes(dev, xs, d, True) > 0)
                t = ops.conv2d_bwd_data_prepare(kern, d, xs, stored=stored, out=old[0] if old is not None else None)
                if t is not None:
                    cache['bwd'][k] = (t, stored)
        finally:
            ops.prepare_flush(self.device)
        return cache

    def _forward_loss(self, x, ys, want_grad, weight_scale=1.0, prep=None):
        """Returns (outs, loss table [n_out, n_cols] on device: col 0 custom / elementwise loss value, 1 mse, 2 mae, the metric
        columns of _plan_loss_table, dys or None)."""
        from . import ops
        phase = self._phase_outputs()
        skip = tuple(k for k, _, _ in phase.values())
        if want_grad and self.plan.dropout_layers:      # Dropout masks are keyed by the training step (the optimizer's count)
            self.model.train_executor.dropout_step = int(self.model.optimizer.iterations)
        if prep is not None:
            outs = self.model.train_executor.run(x, prepared=prep['fwd'], skip_phasew=True, skip_ops=skip, training=want_grad)
        else:
            outs = self.model.train_executor.run(x, skip_ops=skip, training=want_grad)
        n_out = len(outs)
        if self._loss_out is None or self._loss_out.shape[0] != n_out:
            self._loss_out = torch.zeros((n_out, self.n_cols), dtype=torch.float32, device=self.device)
        spec = self.model.loss if self.loss_kind == 'custom' else None
        ew = self._ew
        if ew is not None:
            spec = None
            ew_rows = None if ew[1] is None else self._device_consts(self.model.loss)[1]
        if spec is not None and self._loss_consts is None:
            mean = None if spec.mean is None else torch.from_numpy(spec.mean).to(self.device).contiguous()
            roww = None if spec.row_weights is None else torch.from_numpy(spec.row_weights).to(self.device).contiguous()
            self._loss_consts = (mean, roww)
        dys = []
        for o, (yp, yt) in enumerate(zip(outs, ys)):
            lw = self.loss_weights[o] * weight_scale
            if o in phase:       # 'mse' on the phase channels of a restated output layer: no depth-to-space / space-to-depth pass
                _, d2s, conv_k = phase[o]
                lay = self.plan.ops[conv_k].layer
                yph = self.model.train_executor.scratch(x.shape[0])[d2s.src]
                dz = torch.empty_like(yph) if want_grad else None
                db = None
                if want_grad and lay.bias is not None and lay.activation == 'linear':     # db = the sums of dz: same pass
                    db = torch.empty(yph.shape[1], dtype=torch.float32, device=self.device)
                ytp = yt.reshape((yph.shape[0], yph.shape[1] // 4, 2 * yph.shape[2], 2 * yph.shape[3]))
                if ew is None:
                    ops.mse_mae_phase(yph, ytp, self._loss_out[o, 1:3], dz, db, lw, ws_key=('mse', o) if prep is not None else None)
                else:
                    if ew_rows is not None and ew_rows.numel() != ytp.shape[2]:
                        raise ValueError('latitude weights have %d rows, the model output %d' % (ew_rows.numel(), ytp.shape[2]))
                    ops.loss_elementwise_phase(yph, ytp, self._loss_out[o, 0:1], dz, db, lw * ew[2], ew[0], ew_rows, ws_key=o)
                self._metric_passes(o, yph, ytp, phase=True)
                dys.append(_PhaseGrad(d2s.src, conv_k, dz, db) if want_grad else None)
                continue
            dy = torch.empty_like(yp) if want_grad else None
            if ew is not None:
                if ew_rows is not None and ew_rows.numel() != self._as4(yp, ew_rows).shape[2]:
                    raise ValueError('latitude weights have %d rows, the model output %d' % (ew_rows.numel(), yp.shape[2]))
                ops.loss_elementwise(self._as4(yp, ew_rows), self._as4(yt, ew_rows), self._loss_out[o, 0:1],
                                     None if dy is None else self._as4(dy, ew_rows), lw * ew[2], ew[0], ew_rows, ws_key=o)
            elif spec is None:
                ops.mse_mae(yp, yt, self._loss_out[o, 1:3], dy, lw, ws_key=('mse', o) if prep is not None else None)
            else:
                mean, roww = self._loss_consts
                if yp.dim() != 4:
                    raise NotImplementedError('custom losses need (n, c, h, w) outputs')
                if mean is not None and mean.numel() != yp[0].numel():
                    raise ValueError('anomaly_correlation_loss mean has %d elements, the model output %d per sample'
                                     % (mean.numel(), yp[0].numel()))
                if roww is not None and roww.numel() != yp.shape[2]:
                    raise ValueError('latitude weights have %d rows, the model output %d' % (roww.numel(), yp.shape[2]))
                ops.loss_custom(yp, yt, self._loss_out[o, 0:7], dy, lw * spec.scale, mean, roww, spec.kind, spec.regularize)
            self._metric_passes(o, yp, yt)
            dys.append(dy)
        return outs, self._loss_out, dys

    def _dgrad_act_ops(self):
        """{convolution op k: op index of the Conv2D whose activation output k alone reads} -- candidates for
        dlwp_conv2d_bwd_data_act: k's data gradient then multiplies by act'(that output) and sums that layer's bias gradient in its
        store phase, and the producer's dlwp_act_bwd_bias_grad launch disappears.  OFF unless DLWP_DGRAD_ACT=1: measured equal to
        the two launches on config 3 (batch 64: 1.385-1.391 vs 1.382-1.399 ms, batch 8: 0.410 vs 0.409 ms, same box) -- the store
        phase's extra read costs the data gradient what the separate pass cost."""
        if self._dact_ops is None:
            found = {}
            if os.environ.get('DLWP_DGRAD_ACT', '0') == '1':
                ops_ = self.plan.ops
                uses = {}
                for w in ops_:
                    if w.kind == 'conv' and w.layer is not None:
                        uses[id(w.layer)] = uses.get(id(w.layer), 0) + 1
                for k, op in enumerate(ops_):
                    if op.kind != 'conv' or op.src < 0 or op.src_mode != P.SRC_DIRECT or op.lstm_f or op.src2 is not None:
                        continue
                    chans = self.plan.buffers[op.src][0]
                    if op.in_c_off != 0 or op.xs[0] != chans:
                        continue
                    readers = [j for j, r in enumerate(ops_) if r.src == op.src or (r.src2 is not None and r.src2.get('buf') == op.src)
                               or (r.aux is not None and op.src in [a for a in r.aux if a is not None])]
                    writers = [j for j, w in enumerate(ops_) if w.dst == op.src]
                    if readers != [k] or len(writers) != 1:
                        continue
                    pw = ops_[writers[0]]
                    if (pw.kind == 'conv' and not pw.lstm_f and pw.wparam is None and not pw.out_pool and not pw.out_d2s and
                            pw.out_c_off == 0 and pw.conv_geometry[0] == chans and pw.layer is not None and
                            pw.layer.bias is not None and pw.layer.activation in ('tanh', 'relu') and
                            uses.get(id(pw.layer), 0) == 1 and writers[0] < k):
                        found[k] = writers[0]
            self._dact_ops = found
        return self._dact_ops

    def _phase_outputs(self):
        """{output index: (index of its 'd2s' op, that op, index of the convolution in front)} for outputs the plan restates as
        phase channels + depth-to-space (plan.py) and whose loss is the plain 'mse': the step then takes loss,
        gradient and bias gradient on the phase channels (ops.mse_mae_phase).  DLWP_PHASE_LOSS=0 keeps the separate passes."""
        if self._phase_out is None:
            found = {}
            # the new loss kinds and the metrics pass read the phase channels in 8-byte pairs: an even phase width (target % 4)
            extra = self._ew is not None or self._metric_mask
            if ((self.loss_kind == 'mse' or self._ew is not None) and not self._spec_metrics and
                    os.environ.get('DLWP_PHASE_LOSS', '1') != '0'):
                ops_ = self.plan.ops
                for k, op in enumerate(ops_):
                    if op.kind != 'd2s' or op.dst >= 0 or op.dst == P.STATE_IN or op.out_c_off != 0:
                        continue
                    o = -2 - op.dst
                    writers = [j for j, w in enumerate(ops_) if w.dst == op.src]
                    readers = [j for j, r in enumerate(ops_) if r.src == op.src and j != k]
                    store = self.plan.output_store[o] if 0 <= o < len(self.plan.output_store) else None
                    if (len(writers) == 1 and not readers and ops_[writers[0]].kind == 'conv' and
                            ops_[writers[0]].wparam is not None and store is not None and store[0] == op.xs[0] and
                            sum(1 for w in ops_ if w.dst == op.dst) == 1 and not (extra and store[2] % 4)):
                        found[o] = (k, op, writers[0])
            self._phase_out = found
        return self._phase_out

    # -- kernel regularisers (keras.regularizers.l2 on the ConvLSTM2D kernel, examples/train.py:154) --------------------- #
    def _regularized(self):
        from .regularizers import L1L2
        for lay, nm, off, numel, shape in self.entries:
            reg = getattr(lay, 'kernel_regularizer', None)
            if nm == 'kernel' and isinstance(reg, L1L2) and reg.l2 > 0:
                yield reg.l2, off, numel
            if nm in ('depthwise_kernel', 'pointwise_kernel'):      # DepthwiseConv2D / SeparableConv2D: one regulariser per kernel
                reg = getattr(lay, nm[:-len('kernel')] + 'regularizer', None)
                if isinstance(reg, L1L2) and reg.l2 > 0:
                    yield reg.l2, off, numel

    def _add_regularizer_gradients(self):
        from . import ops
        for l2, off, numel in self._regularized():
            ops.axpby(self.flat_params[off:off + numel], self.flat_grads[off:off + numel], 2.0 * l2, 1.0)

    def _regularizer_loss(self):
        """sum over regularised kernels of l2 * sum(w^2) -- Keras adds it to the reported total loss."""
        tot = 0.0
        for l2, off, numel in self._regularized():
            w = self.flat_params[off:off + numel]
            tot += l2 * float(torch.dot(w, w))
        return tot

    def _report(self, loss_vals, reg=None):
        """[loss, (per-output losses), metrics...] as python floats from the device loss table; reg: the kernel
        regularisers' penalty that belongs to it (None: at the current weights)."""
        v = loss_vals.detach().cpu().numpy().astype(np.float64)
        if self.dp is not None and getattr(self.dp, '_xchg', None) is not None:
            self.dp.oneshot_check()       # (a timed-out one-shot exchange: raise here, where the host looks at the step)
        return self._report_from(v, reg)

    def _report_from(self, v, reg=None):
        n_out = v.shape[0]
        if self.loss_kind == 'custom':
            per_out = [float(self.model.loss.scale * v[o, 0]) for o in range(n_out)]
        elif self.loss_kind == 'elementwise':
            per_out = [float(v[o, 0]) for o in range(n_out)]
        else:
            per_out = [float(v[o, 1]) for o in range(n_out)]
        total = float(sum(w * l for w, l in zip(self.loss_weights, per_out))) + (self._regularizer_loss() if reg is None else reg)

        def metric(o, how):
            if how[0] == 'col':
                return float(v[o, how[1]])
            if how[0] == 'acc':      # mse - mean(p t) / sqrt(mean(p^2) mean(t^2))
                c = how[2]
                return float(v[o, how[1]] - v[o, c] / np.sqrt(v[o, c + 1] * v[o, c + 2]))
            return float(how[2].scale * v[o, how[1]])
        if n_out == 1:
            return [total] + [metric(0, how) for how in self._metric_cols]
        return ([total] + per_out + [metric(o, how) for o in range(n_out) for how in self._metric_cols])

    #: side streams of the weight gradients (DLWP_SIDE_STREAMS).  With the loader's copy stream and the main stream that is four -- the
    #: hardware queues a process has by default
    side_streams = 2

    def _ensure_side_streams(self):
        """The streams the weight gradients run on beside the data-gradient chain: probed to sit on hardware queues of their own
        (util.distinct_streams).  fit_generator calls this BEFORE it builds its DeviceLoader, whose copy stream then avoids them."""
        if self._side is None and self.device.type == 'cuda':
            from .util import distinct_streams
            k = max(1, int(os.environ.get('DLWP_SIDE_STREAMS', self.side_streams)))
            self._side = distinct_streams(self.device, k, [torch.cuda.current_stream(self.device)])
        return self._side or []

    # -- backward ------------------------------------------------------------------------------------------------------ #
    def _backward(self, x, outs, dys, prep=None):
        """The plan's ops in reverse (backward.py); gradients in flat_grads.  prep (the folded step, _fold_ok): prepared
        data-gradient operands, a workspace per deferred final sum, the weight gradients on the side streams; the caller brackets
        forward + backward with ops.reductions_begin / _flush and runs the returned callables (work that needs the final sums)
        after the flush."""
        from .backward import BackwardPass
        return BackwardPass(self, x, outs, dys, prep).run()

    def _forward_backward(self, x, ys, scale):
        """Forward + loss + backward of one step; gradients in flat_grads.  Returns (outs, loss table, dys)."""
        from . import ops
        if not self._fold_ok():
            outs, loss_vals, dys = self._forward_loss(x, ys, True, scale)
            self._backward(x, outs, dys)
            return outs, loss_vals, dys
        prep = self._prepare_step(x)
        ops.reductions_begin(self.device)
        post = []
        try:
            outs, loss_vals, dys = self._forward_loss(x, ys, True, scale, prep)
            post = self._backward(x, outs, dys, prep)
        finally:
            ops.reductions_flush(self.device)      # (always: the handle must not stay in recording mode)
        for fn in post:
            fn()
        return outs, loss_vals, dys

    # -- optimizer ----------------------------------------------------------------------------------------------------- #
    def _ensure_opt_state(self):
        opt = self.model.optimizer
        if self.opt_state is None:
            self.opt_state = tuple(torch.zeros_like(self.flat_params) for _ in range(opt.n_slots()))

    def _exchange_and_apply(self, dp):
        """The data-parallel half of a step: the flat gradient buffer (loss table in its tail) summed over the ranks, then the
        optimizer with grad_scale 1 / world.  RCCL (or torch.distributed) + the update as two launches; with DLWP_ALLREDUCE=oneshot
        and Adam ONE launch of the library's own exchange does both (csrc/xchg.hip)."""
        opt = self.model.optimizer
        if dp.wants_oneshot(self._flat_exchange):
            self._ensure_opt_state()
            if isinstance(opt, Adam) and opt.legacy_kernel():
                m, v = self.opt_state
                dp.oneshot_adam_(self._flat_exchange, self.flat_params.numel(), self.flat_params, m, v, opt.lr, opt.beta_1,
                                 opt.beta_2, opt.epsilon, opt.decay, opt.iterations, 1.0 / dp.world)
                opt.iterations += 1
                return
            dp.oneshot_all_reduce_(self._flat_exchange)
        else:
            dp.all_reduce_sum_(self._flat_exchange)        # gradients and loss table: one collective
        self._apply(1.0 / dp.world)

    def _apply(self, grad_scale=1.0):
        from . import ops
        opt = self.model.optimizer
        self._ensure_opt_state()
        if not opt.legacy_kernel():
            self._optimizer_step(grad_scale)
        elif isinstance(opt, Adam):
            m, v = self.opt_state
            ops.adam_keras(self.flat_params, m, v, self.flat_grads, opt.iterations, opt.lr, opt.beta_1, opt.beta_2,
                           opt.epsilon, opt.decay, grad_scale)
        else:
            ops.sgd_keras(self.flat_params, self.opt_state[0], self.flat_grads, opt.iterations, opt.lr, opt.momentum,
                          opt.decay, grad_scale)
        opt.after_step()

    def _optimizer_step(self, grad_scale):
        """dlwp_optimizer_step on the flat buffers, behind the clipnorm pass where the optimizer has one: the factor (and the norm,
        never read back) stays on the device in self._clip_out."""
        from . import ops
        opt = self.model.optimizer
        clipnorm, clipvalue = opt.clips()
        factor = None
        if clipnorm > 0:
            if self._clip_out is None:
                self._clip_out = torch.zeros(3, dtype=torch.float32, device=self.device)
            factor = ops.grad_clip_factor(self.flat_grads, clipnorm, grad_scale, out=self._clip_out, ws_key=id(self))
        ops.optimizer_step(opt.step_kind(), self.flat_params, self.opt_state, self.flat_grads, opt.iterations,
                           grad_scale=grad_scale, clipvalue=clipvalue, factor=factor, **opt.step_args())

    # -- public steps -------------------------------------------------------------------------------------------------- #
    def _host_rows(self, a, lo, hi):
        """rows [lo, hi) of a host array / device tensor WITHOUT touching the others (no upload of foreign rows)"""
        return a[lo:hi]

    def train_on_batch(self, x, y, return_device=False):
        """One optimisation step on a GLOBAL batch.  Under data parallelism every rank passes the same global batch (the
        Keras contract: one script, run by every rank) and trains on its own row shard -- only those rows are uploaded;
        the reported loss is the global-batch value on every rank.  Loaders that hold only the local rows call
        train_on_shard."""
        n_global = int(x.shape[0])
        dp = self.dp
        if dp is not None and dp.world > 1:
            lo, hi = dp.shard(n_global)
            ys = list(y) if isinstance(y, (list, tuple)) else [y]
            x = self._host_rows(x, lo, hi)
            ys = [self._host_rows(t, lo, hi) for t in ys]
            return self.train_on_shard(x, ys if isinstance(y, (list, tuple)) else ys[0], n_global, return_device)
        return self.train_on_shard(x, y, n_global, return_device)

    # -- the step as a hipGraph --------------------------------------------------------------------------------------------- #
    #: a batch shape seen this many times is captured (the first steps run eagerly: lazy allocations, scratch buffers)
    graph_after = 2

    #: DLWP_TRAIN_GRAPH unset: steps of at most this many samples x grid points replay as a captured graph
    # (r4, gpurun s22, ms per step graph / lanes -- the lanes on the streams the step was recorded on, DLWP_STEP_LANES_RECORDED --:
    #  8 samples 0.382 / 0.394, 12: 0.450 / 0.434, 16: 0.560 / 0.536, 24: 0.692 / 0.667, 64: 1.431 / 1.381; the graph form needs 0.04 ms
    #  of host time per step, the lanes 0.18)
    graph_below = 10 * 88 * 180

    def _graph_ok(self, n_local=None):
        """How a step of n_local samples runs: False -- launch by launch from Python (the eager step) -- or the form in which it is
        REPLAYED once its shape has been seen graph_after times:
          'graph' / 'lanes' / 'branches'  the library's step object (csrc/tape.hip, dlwp_train_step_*): the launch sequence is
                    recorded once, while an eager step runs, and replayed with ONE C call -- as one hipGraph on a single stream
                    ('graph'), launch by launch with the weight gradients on the step's side streams ('lanes'), or as one hipGraph
                    with those lanes as branches ('branches').  Plans the folded step covers (_fold_ok).  r4: this replaces both the
                    ~0.6 ms of Python per eager step and the torch.cuda.CUDAGraph capture, which raced a DeviceLoader's thread.
          'torch'   torch.cuda.CUDAGraph around the Python step (r2/r3): plans outside the folded step, DLWP_TRAIN_GRAPH=1 only.
        DLWP_TRAIN_GRAPH: '0' never replay; '1' always; unset: folded plans replay -- small steps (at most graph_below samples x
        grid points) as 'graph', larger ones as 'lanes' (their weight gradients gain from the side streams: batch 64 1.78 ->
        1.68 ms in r3).  DLWP_TRAIN_STEP=graph|lanes|branches|torch picks the form.  Never replayed: kernel regularisers (their
        penalty is read back to the host every step), SGD with decay (its rate is a launch argument), models with Dropout layers
        (the step number that keys their masks is a launch argument), steps on the CPU device.  Of the optimizers behind
        dlwp_optimizer_step, those whose launch arguments do not change with the step number replay -- RMSprop, Adagrad, Adadelta
        and SGD (nesterov or clipped) with decay == 0, clipped or not: the clipnorm factor lives on the device.  Adamax, Nadam,
        amsgrad or clipped Adam and anything with decay > 0 carry step-dependent scalars as launch arguments and stay eager (no
        device-side step counter for them yet), as SGD with decay does."""
        opt = self.model.optimizer
        mode = os.environ.get('DLWP_TRAIN_GRAPH', 'auto')
        if self.device.type != 'cuda' or mode == '0' or n_local is None:
            return False
        if any(True for _ in self._regularized()) or self.plan.dropout_layers:
            return False
        if opt.legacy_kernel():
            if not (isinstance(opt, Adam) or opt.decay == 0.0):
                return False
        elif opt.step_depends_on_iteration():
            return False
        form = os.environ.get('DLWP_TRAIN_STEP')
        if form not in (None, '', 'graph', 'lanes', 'branches', 'torch'):
            raise ValueError('DLWP_TRAIN_STEP=%r (graph, lanes, branches, torch)' % form)
        if not self._fold_ok():
            return 'torch' if (mode == '1' or form == 'torch') else False
        if form:
            return form
        store = self.plan._in_store
        return 'graph' if (mode == '1' or n_local * int(store[-1]) * int(store[-2]) <= self.graph_below) else 'lanes'

    def _step_tail(self, loss_vals, scale, dp):
        """What follows forward + backward inside a recorded or captured step: the update with the step number on the device --
        or, data parallel, the loss table moved behind the gradients (the exchange and the update stay outside: a collective in
        between)."""
        from . import ops
        opt = self.model.optimizer
        if dp is not None:
            ops.axpby(loss_vals.view(-1), self._loss_tail.view(-1), scale, 0.0)
        elif not opt.legacy_kernel():
            self._optimizer_step(1.0)
        elif isinstance(opt, Adam):
            m, v = self.opt_state
            ops.adam_keras_dev(self.flat_params, m, v, self.flat_grads, self._iter_dev, self._lr_t, opt.lr, opt.beta_1,
                               opt.beta_2, opt.epsilon, opt.decay, 1.0)
        else:
            ops.sgd_keras(self.flat_params, self.opt_state[0], self.flat_grads, 0, opt.lr, opt.momentum, 0.0, 1.0)

    # -- the step as a library object (dlwp_train_step_*) ------------------------------------------------------------------ #
    def _record_step(self, x, ys, n_global, scale, dp, form='graph'):
        """Runs ONE real step on (x, ys) while the library records its launches; returns the step entry, or {'refused': True} when
        the step contained device work the tape does not carry (it then stays eager).  Memory: every tensor the step allocates
        while recording comes from a private torch.cuda.MemPool that is kept with the entry, so the addresses the tape holds
        stay valid and nobody else is handed them.
        Two guards against a replay that silently misses a launch.  Structural: every stream-taking entry point of the
        library WITHOUT a tape record marks the tape foreign (DLWP_UNTAPED, csrc/common.h) and dlwp_train_step_create refuses it;
        torch-side launches set self._foreign.  By result (DLWP_TAPE_VALIDATE, default on): before the entry is cached the step
        runs twice more on a DIFFERENT batch from DIFFERENT weights (both derived from the recorded ones: nothing a missing
        launch leaves behind from the recorded step can pass for its result -- not even a weight preparation's) -- once launch by
        launch, once as the replay in the form it will run in (`form`) -- and parameters, optimizer slots, gradients and the loss
        table of the two must agree; the state the recorded step left is put back afterwards.  Two extra steps per recorded shape."""
        from . import _lib, ops
        opt = self.model.optimizer
        gx = x.clone()
        gys = [t.clone() for t in ys]
        if self._iter_dev is None:
            self._iter_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._lr_t = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self.opt_state is None:
            raise RuntimeError('the optimizer slots must exist before the step is recorded')
        if dp is None and isinstance(opt, Adam):
            self._iter_dev.fill_(int(opt.iterations))
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        h = _lib.handle(dev)
        main = torch.cuda.current_stream(self.device)
        pool = torch.cuda.MemPool()
        self._foreign = False
        validate = os.environ.get('DLWP_TAPE_VALIDATE', '1') != '0'
        state0 = [t.clone() for t in [self.flat_params] + list(self.opt_state) + [self._iter_dev] + self._bn_stats] \
            if validate else None

        def body(bx, bys):
            outs_, loss_, dys_ = self._forward_backward(bx, bys, scale)
            self._step_tail(loss_, scale, dp)
            return outs_, loss_, dys_
        with _no_gc():
            with torch.cuda.use_mem_pool(pool, device=self.device):
                _lib.check(_lib.lib.dlwp_train_step_record_begin(h, ctypes.c_void_p(main.cuda_stream)))
                try:
                    outs, loss_vals, dys = body(gx, gys)
                except BaseException:
                    _lib.lib.dlwp_train_step_record_abort(h)
                    raise
                ins = [gx] + gys
                if self._foreign or len(ins) > 8:
                    _lib.lib.dlwp_train_step_record_abort(h)
                    return {'refused': True, 'loss': loss_vals}
                step = ctypes.c_void_p()
                dst = (ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
                floats = (ctypes.c_size_t * len(ins))(*[t.numel() for t in ins])
                rc = _lib.lib.dlwp_train_step_create(h, len(ins), dst, floats, ctypes.byref(step))
                if rc == _lib.EUNSUPPORTED:          # an entry point without a tape record ran inside the step: the shape stays eager
                    return {'refused': True, 'loss': loss_vals, 'why': _lib.lib.dlwp_last_error().decode('utf-8', 'replace')}
                _lib.check(rc)
        keep = (outs, loss_vals, dys, dict(ops._workspaces), dict(ops._workspaces2),
                self.model.train_executor.scratch(int(x.shape[0])), self.model.train_executor.phase_buffers(),
                self._prep_cache.get(int(x.shape[0])), self._side, pool)
        ent = {'step': _StepHandle(step), 'x': gx, 'ys': gys, 'loss': loss_vals, 'keep': keep}
        if validate:
            why = self._validate_step(ent, state0, body, form, dp is not None)
            if why is not None:
                import warnings
                warnings.warn('dlwp_amd: the recorded training step did not reproduce the eager step (%s); batches of %d samples '
                              'keep running launch by launch' % (why, int(x.shape[0])), RuntimeWarning)
                ent['step'] = None                   # (its finaliser destroys the step object)
                return {'refused': True, 'loss': loss_vals, 'why': why}
        return ent

    def _validate_step(self, ent, state0, body, form, data_parallel=False):
        """The freshly recorded step against the launch-by-launch step on a batch and weights neither has seen (see _record_step);
        returns None when they agree, else what differed.  Leaves the state the recorded step left."""
        from . import _lib
        live = [self.flat_params] + list(self.opt_state) + [self._iter_dev] + self._bn_stats
        # (the loss table rides behind the gradients only in a data-parallel step: the recorded launches write it there)
        gbuf = self._flat_exchange if data_parallel else self.flat_grads
        after = [t.clone() for t in live] + [gbuf.clone(), ent['loss'].clone()]
        xv = ent['x'] * 0.75 + 0.125
        yvs = [t * 1.25 - 0.0625 for t in ent['ys']]

        def start():
            for t, t0 in zip(live, state0):
                t.copy_(t0)
            self.flat_params.mul_(1.0 + 2.0 ** -9)          # other weights: every prepared operand changes with them
        why = None
        try:
            start()
            _, loss_e, _ = body(xv, yvs)
            want = [t.clone() for t in live] + [gbuf.clone(), loss_e.clone()]
            start()
            ent['x'].copy_(xv)
            for d_, s_ in zip(ent['ys'], yvs):
                d_.copy_(s_)
            lanes_mode = _lib.STEP_LANES if os.environ.get('DLWP_TRAIN_LANES') == 'own' else _lib.STEP_LANES_RECORDED
            mode = {'lanes': lanes_mode, 'graph': _lib.STEP_GRAPH, 'branches': _lib.STEP_GRAPH_BRANCHES}.get(form, _lib.STEP_GRAPH)
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = _lib.lib.dlwp_train_step_launch(ent['step'].h, None, mode, stream)      # (the inputs are in the step's buffers)
            if rc != _lib.OK:
                why = 'replay failed: ' + _lib.lib.dlwp_last_error().decode('utf-8', 'replace')
            else:
                torch.cuda.synchronize(self.device)
                names = ['parameters'] + ['optimizer slot %d' % i for i in range(len(self.opt_state))] + ['step counter'] + \
                    ['moving statistics %d' % i for i in range(len(self._bn_stats))] + ['gradients', 'loss table']
                for name, got, ref in zip(names, live + [gbuf, ent['loss']], want):
                    if got.dtype.is_floating_point:
                        if not bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()):
                            why = '%s are not finite' % name
                            break
                        if float((got - ref).abs().max()) > 1e-5 * float(ref.abs().max()) + 1e-30:
                            why = '%s differ by %.3g of %.3g' % (name, float((got - ref).abs().max()), float(ref.abs().max()))
                            break
                    elif not torch.equal(got, ref):
                        why = '%s differ' % name
                        break
        finally:
            for t, w in zip(live + [gbuf, ent['loss']], after):
                t.copy_(w)
        return why

    def _capture_step(self, x, ys, n_global, scale, dp):
        gx = x.clone()
        gys = [t.clone() for t in ys]
        if self._iter_dev is None:
            self._iter_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._lr_t = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self.opt_state is None:
            raise RuntimeError('the optimizer slots must exist before the step is captured')
        from ._lib import capture_lock
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with _no_gc():
            return self._capture_locked(g, gx, gys, n_global, scale, dp, capture_lock)

    def _capture_locked(self, g, gx, gys, n_global, scale, dp, capture_lock):
        from . import ops
        x = gx
        with capture_lock, torch.cuda.graph(g, capture_error_mode='thread_local'):
            outs, loss_vals, dys = self._forward_backward(gx, gys, scale)
            self._step_tail(loss_vals, scale, dp)
        # everything the captured launches point into must outlive the graph, whatever the caches do later
        keep = (outs, loss_vals, dys, dict(ops._workspaces), dict(ops._workspaces2),
                self.model.train_executor.scratch(int(x.shape[0])), self.model.train_executor.phase_buffers(),
                self._prep_cache.get(int(x.shape[0])), self._side)
        return {'graph': g, 'x': gx, 'ys': gys, 'loss': loss_vals, 'keep': keep}

    def _graph_step(self, x, ys, n_global, scale, dp):
        """Replays (capturing first, if needed) the step for this batch shape.  Returns the device loss table, or None when
        this shape has not been seen often enough yet (the caller then runs the step eagerly)."""
        from . import _lib
        _lib.drain_graveyard()          # a safe point: nothing is being recorded or replayed yet
        from . import ops
        opt = self.model.optimizer
        # the captured launches carry the optimizer's hyper-parameters as arguments: a changed rate (scheduler, callback,
        # load_model) must not replay the old ones
        hyper = tuple((k, float(getattr(opt, k))) for k in ('lr', 'decay', 'beta_1', 'beta_2', 'epsilon', 'momentum', 'rho',
                                                            'nesterov', 'amsgrad', 'schedule_decay', 'clipnorm', 'clipvalue')
                      if hasattr(opt, k))
        form = self._graph_ok(int(x.shape[0]))
        key = (int(x.shape[0]), int(n_global), 0 if dp is None else dp.world, hyper, 'torch' if form == 'torch' else 'tape')
        if key in self._no_tape:
            return None
        ent = self._graphs.get(key)
        if ent is None:
            seen = self._graph_seen.get(key, 0) + 1
            self._graph_seen[key] = seen
            if seen <= self.graph_after:
                return None
            if len(self._graphs) >= 4:
                self._graphs.clear()
            if form == 'torch':
                ent = self._graphs[key] = self._capture_step(x, ys, n_global, scale, dp)
            else:
                ent = self._record_step(x, ys, n_global, scale, dp, form)     # (this IS a step: on x, ys)
                if ent.get('refused'):
                    self._no_tape.add(key)
                else:
                    self._graphs[key] = ent
                if dp is None:
                    opt.iterations += 1
                    self._iter_shadow = opt.iterations
                return ent['loss']
        if 'step' in ent:
            from . import _lib
            if dp is None and isinstance(opt, Adam) and self._iter_shadow != opt.iterations:
                self._iter_dev.fill_(int(opt.iterations))          # (after load_model / a manual change / eager steps)
            srcs = [x] + list(ys)
            if not all(s_.is_contiguous() and s_.dtype == torch.float32 and s_.numel() == d_.numel()
                       for s_, d_ in zip(srcs, [ent['x']] + ent['ys'])):
                srcs = [s_.to(torch.float32).contiguous() for s_ in srcs]
            ptrs = (ctypes.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
            # ('lanes': on the trainer's own side streams, the ones the step was recorded on -- they are kept in ent['keep'] --: streams
            #  the library creates later may share a hardware queue with the main stream; DLWP_TRAIN_LANES=own picks those)
            lanes_mode = _lib.STEP_LANES if os.environ.get('DLWP_TRAIN_LANES') == 'own' else _lib.STEP_LANES_RECORDED
            mode = {'lanes': lanes_mode, 'graph': _lib.STEP_GRAPH, 'branches': _lib.STEP_GRAPH_BRANCHES}[form]
            _lib.check(_lib.lib.dlwp_train_step_launch(ent['step'].h, ptrs, mode,
                                                       ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            if dp is None:
                opt.iterations += 1
                self._iter_shadow = opt.iterations
            return ent['loss']
        pairs = [(x, ent['x'])] + list(zip(ys, ent['ys']))
        if len(pairs) <= 8 and all(s.is_contiguous() and s.dtype == torch.float32 and s.numel() == d.numel() for s, d in pairs):
            ops.copy_many(pairs)            # the batch and its targets into the graph's buffers: one launch
        else:
            for s, d in pairs:
                d.copy_(s.reshape(d.shape))
        if dp is None and isinstance(opt, Adam) and self._iter_shadow != opt.iterations:
            self._iter_dev.fill_(int(opt.iterations))          # (after load_model / a manual change / eager steps)
        ent['graph'].replay()
        if dp is None:
            opt.iterations += 1
            self._iter_shadow = opt.iterations
        return ent['loss']

    def train_on_shard(self, x, y, n_global, return_device=False):
        """One optimisation step given THIS RANK's rows of a global batch of n_global samples (all of them when not data
        parallel).  Collective under data parallelism: every rank must call it, also with zero rows."""
        from . import ops
        x = self._to_device(x)
        n_local = int(x.shape[0])
        dp = self.dp if (self.dp is not None and self.dp.world > 1) else None
        if dp is None and n_local != int(n_global):
            raise ValueError('%d rows given for a batch of %d without data parallelism' % (n_local, n_global))
        if dp is not None and self._params_dirty:
            self.sync_parameters()
        if n_local > 0 and self._graph_ok(n_local):
            scale_g = 1.0 if dp is None else n_local * dp.world / float(n_global)
            x = x.reshape((n_local,) + tuple(x.shape[1:]))
            loss_vals = self._graph_step(x, self._targets(y, n_local), n_global, scale_g, dp)
            if loss_vals is not None:
                if dp is not None:
                    self._exchange_and_apply(dp)
                    loss_vals = self._loss_tail
                    ops.axpby(loss_vals.view(-1), loss_vals.view(-1), 0.0, 1.0 / dp.world)
                if return_device:
                    return loss_vals, 0.0
                return self._report(loss_vals, 0.0)
        # local means are averaged over ranks: weight each by its share so ragged shards stay exact
        scale = 1.0 if dp is None else n_local * dp.world / float(n_global)
        if n_local > 0:
            ys = self._targets(y, n_local)
            outs, loss_vals, dys = self._forward_backward(x, ys, scale)
            self._add_regularizer_gradients()
        else:                               # a rank without rows still takes part in the exchange: no data gradient, but
            self._flat_exchange.zero_()     # its share of the regularisers' (every rank adds it in full, the sum is / world)
            self._add_regularizer_gradients()
            loss_vals = None
        reg = self._regularizer_loss()      # Keras reports the penalty at the weights the step started from
        if dp is not None:
            if loss_vals is not None:
                ops.axpby(loss_vals.view(-1), self._loss_tail.view(-1), scale, 0.0)
            self._exchange_and_apply(dp)
            loss_vals = self._loss_tail
            ops.axpby(loss_vals.view(-1), loss_vals.view(-1), 0.0, 1.0 / dp.world)
        else:
            self._apply(1.0)
        if return_device:
            return loss_vals, reg
        return self._report(loss_vals, reg)

    def test_on_batch(self, x, y):
        x = self._to_device(x)
        ys = self._targets(y, x.shape[0])
        _, loss_vals, _ = self._forward_loss(x, ys, False)
        return self._report(loss_vals)

    # -- loops --------------------------------------------------------------------------------------------------------- #
    def _callbacks(self, callbacks, params):
        hist = History()
        cbs = [hist] + [c for c in (callbacks or [])]
        for c in cbs:
            if hasattr(c, 'set_model'):
                c.set_model(self.model)
            else:
                c.model = self.model
            if hasattr(c, 'set_params'):
                c.set_params(params)
        self.model.history = hist
        return hist, cbs

    @staticmethod
    def _call(cbs, name, *args):
        for c in cbs:
            fn = getattr(c, name, None)
            if fn is not None:
                fn(*args)

    def _run_epochs(self, epochs, initial_epoch, batches_fn, n_batches_fn, validate_fn, callbacks, verbose, on_epoch_end):
        params = {'epochs': epochs, 'metrics': self.metrics_names, 'verbose': verbose}
        hist, cbs = self._callbacks(callbacks, params)
        self.model.stop_training = False
        self._call(cbs, 'on_train_begin', {})
        for epoch in range(initial_epoch, epochs):
            t0 = time.time()
            self._call(cbs, 'on_epoch_begin', epoch, {})
            sums = None
            seen = 0
            pending = []
            # The epoch's logs are batch-size-weighted means of the per-batch values, and for the per-element losses those are
            # LINEAR in the step's loss table: the tables are summed on the device, weighted, by one small launch per step (r4: a
            # clone per step was a device-to-device memcpy between two graph launches -- 4 us and ~15 us of queue bubbles around it,
            # profiles/r4_loader_timeline.txt) and read once per epoch.  Whole-batch statistics (custom losses) keep their tables.
            acc, reg_sum = None, 0.0
            for bi, (X, y, n_glob) in enumerate(batches_fn(epoch)):      # X, y: this rank's rows of a batch of n_glob
                self._call(cbs, 'on_batch_begin', bi, {'batch': bi, 'size': n_glob})
                lv, reg = self.train_on_shard(X, y, n_glob, return_device=True)
                if (self.loss_kind != 'custom' and not self._batch_stat and lv.is_cuda and lv.dtype == torch.float32 and
                        lv.is_contiguous()):
                    from . import ops
                    if acc is None:
                        acc = torch.zeros_like(lv)
                    ops.axpby(lv.view(-1), acc.view(-1), float(n_glob), 1.0)
                    reg_sum += float(n_glob) * float(reg)
                    seen += n_glob
                else:
                    pending.append((lv.clone(), n_glob, reg))
                # convert lazily: one host sync per epoch unless a callback wants per-batch logs
                if any(getattr(type(c), 'on_batch_end', Callback.on_batch_end) is not Callback.on_batch_end
                       for c in cbs if isinstance(c, Callback)) or any(not isinstance(c, Callback) for c in cbs):
                    vals = self._report(lv, reg)
                    self._call(cbs, 'on_batch_end', bi, dict(zip(self.metrics_names, vals), batch=bi, size=n_glob))
                if self.model.stop_training:
                    break
            if pending:                  # one device-to-host copy for the whole epoch's loss tables
                tables = torch.stack([lv for lv, _, _ in pending]).cpu().numpy().astype(np.float64)
                for tab, (_, bs, reg) in zip(tables, pending):
                    vals = np.asarray(self._report_from(tab, reg), dtype=np.float64)
                    sums = vals * bs if sums is None else sums + vals * bs
                    seen += bs
            if acc is not None:          # sum over the batches of size x table -> size-weighted sums of the reported values
                vals = np.asarray(self._report_from(acc.cpu().numpy().astype(np.float64), 0.0), dtype=np.float64)
                vals[0] += reg_sum
                sums = vals if sums is None else sums + vals
            logs = dict(zip(self.metrics_names, (sums / max(seen, 1)).tolist())) if sums is not None else {}
            if self.dp is not None and getattr(self.dp, '_xchg', None) is not None:
                self.dp.oneshot_check()         # (the epoch's tables are on the host: the device has been synchronised anyway)
            if validate_fn is not None:
                vvals = validate_fn()
                logs.update({'val_' + k: v for k, v in zip(self.metrics_names, vvals)})
            if on_epoch_end is not None:
                on_epoch_end()
            if verbose:
                msg = ' - '.join('%s: %.4f' % (k, v) for k, v in logs.items())
                print('Epoch %d/%d - %.1fs - %s' % (epoch + 1, epochs, time.time() - t0, msg))
            self._call(cbs, 'on_epoch_end', epoch, logs)
            if self.dp is not None and self.dp.world > 1 and getattr(self.dp, 'mirror', False):
                # driver mode: callbacks (EarlyStopping ...) run on rank 0 only -- every rank takes its decision
                self.model.stop_training = bool(self.dp.broadcast_indices(np.array([int(bool(self.model.stop_training))]))[0])
            if self.model.stop_training:
                break
        self._call(cbs, 'on_train_end', {})
        return hist

    #: fit(x, y) keeps the whole training set in HBM when it takes at most this share of the free device memory (288 GB
    #: per MI355X: the reference's multi-year 2-degree sets are tens of GB); 0 disables (host gather + upload per batch)
    resident_fraction = 0.5

    def _make_resident(self, x, ys):
        """Upload numpy training arrays once (float32) if they fit; returns (x, ys, resident)."""
        if self.device.type != 'cuda' or self.resident_fraction <= 0:
            return x, ys, False
        arrays = [x] + list(ys)
        if all(isinstance(a, torch.Tensor) and a.is_cuda for a in arrays):
            return x, ys, True
        if any(isinstance(a, torch.Tensor) for a in arrays):
            return x, ys, False
        arrays = [np.asarray(a) for a in arrays]
        need = sum(int(a.size) * 4 for a in arrays)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > self.resident_fraction * free:
            return x, ys, False
        dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device) for a in arrays]
        return dev[0], dev[1:], True

    def fit(self, x, y, batch_size=None, epochs=1, verbose=1, callbacks=None, validation_data=None, shuffle=True,
            initial_epoch=0):
        batch_size = int(batch_size or 32)
        x = np.asarray(x) if not isinstance(x, torch.Tensor) else x
        n = x.shape[0]
        ys = list(y) if isinstance(y, (list, tuple)) else [y]
        x, ys, resident = self._make_resident(x, ys)

        dp = self.dp if (self.dp is not None and self.dp.world > 1) else None

        def batches(epoch):
            idx = np.arange(n)
            if shuffle:
                np.random.shuffle(idx)
            if dp is not None:             # one shuffle for all replicas: rank 0's
                idx = dp.broadcast_indices(idx)
            for lo in range(0, n, batch_size):
                sel = idx[lo:lo + batch_size]
                n_glob = len(sel)
                if dp is not None:         # this rank's rows of the global batch; nothing else is gathered or uploaded
                    a, b = dp.shard(n_glob)
                    sel = sel[a:b]
                if resident:           # the batch is gathered in HBM: no host copy, no PCIe transfer per step
                    sel = torch.from_numpy(np.ascontiguousarray(sel)).to(self.device)
                    yield x.index_select(0, sel), ([t.index_select(0, sel) for t in ys] if len(ys) > 1
                                                   else ys[0].index_select(0, sel)), n_glob
                else:
                    yield x[sel], ([t[sel] for t in ys] if len(ys) > 1 else ys[0][sel]), n_glob

        val = None
        if validation_data is not None:
            vx, vy = validation_data[0], validation_data[1]
            if not isinstance(vx, torch.Tensor):       # uploaded once, evaluated after every epoch
                vys = list(vy) if isinstance(vy, (list, tuple)) else [vy]
                vx, vys, _ = self._make_resident(np.asarray(vx), vys)
                vy = vys if isinstance(vy, (list, tuple)) else vys[0]
            val = lambda: self.evaluate(vx, vy, batch_size=batch_size, verbose=0, as_list=True)  # noqa: E731
        return self._run_epochs(epochs, initial_epoch, batches, None, val, callbacks, verbose, None)

    def fit_generator(self, generator, steps_per_epoch=None, epochs=1, verbose=1, callbacks=None, validation_data=None,
                      validation_steps=None, shuffle=True, initial_epoch=0):
        from .model.generators import DeviceLoader
        steps = int(steps_per_epoch) if steps_per_epoch is not None else len(generator)

        dp = self.dp if (self.dp is not None and self.dp.world > 1) else None
        shard = None if dp is None else (dp.rank, dp.world)

        loader = [None]          # one loader for the whole call: its pinned / device staging buffers serve every epoch

        def batches(epoch):
            order = list(range(steps))
            if dp is not None and hasattr(generator, '_indices'):
                # the generators shuffle with the process-global numpy RandomState (reference generators.py:103-106):
                # replicas must cut THE SAME batch i, so every rank takes rank 0's index list for this epoch
                generator._indices = dp.broadcast_indices(generator._indices)
            if self.device.type == 'cuda' or shard is not None:
                if loader[0] is None:
                    # (its copy stream on a hardware queue of its own: not the main stream's, not a weight-gradient stream's)
                    avoid = None
                    if self.device.type == 'cuda':
                        avoid = [torch.cuda.current_stream(self.device)] + list(self._ensure_side_streams() if self._fold_ok() else [])
                    loader[0] = DeviceLoader(generator, self.device, order=order, shard=shard, avoid_streams=avoid)
                for X, y, n_glob in loader[0].iter_batches(order):
                    yield X, y, n_glob
            else:
                for i in order:
                    X, y = generator[i]
                    yield X, y, int(X.shape[0])

        def end():
            if hasattr(generator, 'on_epoch_end'):
                generator.on_epoch_end()

        val = None
        if validation_data is not None:
            if isinstance(validation_data, (tuple, list)):
                vx, vy = validation_data[0], validation_data[1]
                val = lambda: self.evaluate(vx, vy, verbose=0, as_list=True)  # noqa: E731
            else:
                vgen = validation_data
                vsteps = int(validation_steps) if validation_steps is not None else len(vgen)
                val = lambda: self.evaluate_generator(vgen, vsteps)  # noqa: E731
        self._loader_threads += 1
        try:
            return self._run_epochs(epochs, initial_epoch, batches, None, val, callbacks, verbose, end)
        finally:
            self._loader_threads -= 1

    def _eval_batches(self, generator, steps):
        """(X, y) of batches 0 .. steps - 1.  A series generator whose batches are plain windows (window_plan) on a single CUDA
        device goes through a DeviceLoader that keeps the series in HBM -- one loader per generator, kept with the trainer, so
        the validation set of a fit_generator call is uploaded once and not after every epoch; everything else is generator[i]."""
        loader = None
        single = self.dp is None or self.dp.world <= 1
        if self.device.type == 'cuda' and single and hasattr(generator, 'window_plan') and 0 < steps <= len(generator):
            from .model.generators import DeviceLoader
            cache = self.__dict__.setdefault('_eval_loaders', {})
            ent = cache.get(id(generator))
            if ent is None or ent[0]() is not generator:
                import weakref
                cache.clear()                 # (one validation generator at a time: an earlier one's series leaves HBM)
                ent = cache[id(generator)] = (weakref.ref(generator), DeviceLoader(generator, self.device))
            if ent[1]._resident_state() is not None:
                loader = ent[1]
        if loader is None:
            for i in range(steps):
                yield generator[i]
        else:
            for X, y, _ in loader.iter_batches(list(range(steps))):
                yield X, y

    def evaluate_generator(self, generator, steps=None):
        steps = int(steps) if steps is not None else len(generator)
        sums, seen = None, 0
        for X, y in self._eval_batches(generator, steps):
            vals = np.asarray(self.test_on_batch(X, y), dtype=np.float64)
            bs = int(np.asarray(X).shape[0]) if not isinstance(X, torch.Tensor) else int(X.shape[0])
            sums = vals * bs if sums is None else sums + vals * bs
            seen += bs
        return (sums / max(seen, 1)).tolist()

    def evaluate(self, x, y, batch_size=None, verbose=1, as_list=False):
        batch_size = int(batch_size or 32)
        if self.loss_kind != 'custom' and not self._batch_stat:   # per-element means do not depend on it; larger chunks fill the GPU.
            batch_size = max(batch_size, 256)    # The anomaly-correlation loss is a whole-batch statistic: keep Keras' batches
        n = x.shape[0]
        ys = list(y) if isinstance(y, (list, tuple)) else [y]
        sums, seen = None, 0
        for lo in range(0, n, batch_size):
            yb = [t[lo:lo + batch_size] for t in ys]
            vals = np.asarray(self.test_on_batch(x[lo:lo + batch_size], yb if len(yb) > 1 else yb[0]), dtype=np.float64)
            bs = min(batch_size, n - lo)
            sums = vals * bs if sums is None else sums + vals * bs
            seen += bs
        out = (sums / max(seen, 1)).tolist()
        return out if (len(out) > 1 or as_list) else out[0]
