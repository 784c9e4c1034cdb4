"""
Forecast error measures of the validation scripts (reference DLWP/model/verify.py:17-102, called from
examples/validate.py / plot_forecasts.py on the output of predict_timeseries).

Two paths, one definition:

* numpy arguments without `device=` run the reference's plain numpy code on the host, bit for bit (pinned by
  tests/golden/verify.npz, the reference's own functions run by oracle/make_golden.py).  That path is no longer cheap next to
  the rollout it scores: a series of 28 leads x 64 samples x 4 x 88 x 180 float32 (454 MB) costs forecast_error 0.73-0.77 s
  against a plain verification series and 1.6 s against a per-lead one (numpy, 16 threads), the device rollout that
  produced it about 4 ms; a series that lives in HBM has to cross the host link first.  Measured on the MI355X box at the
  benchmark's operating point, 56 leads x 256 members (3.6 GB): 2.4 s / 3.2 s on the host with the download, 0.85 ms /
  1.3 ms on the device for the same call (tools/bench_verify.py; DESIGN.md 5.29 has the table).
* CUDA float32 tensors -- what predict_timeseries(..., return_device=True) returns -- or numpy arguments with `device='cuda'`
  are reduced where they are by csrc/verify.hip: one launch yields sum d^2, sum |d| and the number of non-NaN pairs per lead
  (and group) in float64, so 'mse', 'mae' and 'rmse' cost the same pass, and the few hundred doubles are finished here:
  S / count in float64, sqrt for 'rmse', a cast to float32, NaN where nothing was counted (a lead beyond the verification
  series included).  d = a - b is rounded in float32 exactly as numpy rounds it; the sums behind it are float64, so a result
  is within 2^-22 (relative) of the float64 value of the same definition -- closer to it than the host path's float32
  pairwise mean, and therefore not bit-equal to that one.
  The device path covers axis=None and the axis tuple that keeps the lead and the first inner axis ((0, 2, 3) for a 4-D
  `valid`, (1, 3, 4) for the per-lead form; any rank); every other `axis` runs the numpy code on downloaded arrays.

A caveat of return_device=True: the tensor may alias the cached series buffer of the model's captured rollout, which the next
rollout of that model overwrites -- verify it (or clone it) before rolling the model out again.
"""
import collections

import numpy as np
import torch

_METHODS = ('mse', 'mae', 'rmse')


def _error(diff, method, axis):
    if method == 'mae':
        return np.nanmean(np.abs(diff), axis=axis)
    mse = np.nanmean(diff ** 2., axis=axis)
    return np.sqrt(mse) if method == 'rmse' else mse


def _check(method):
    if method not in _METHODS:
        raise ValueError("'method' must be 'mse', 'rmse', or 'mae'")


# -- the device path: (shapes, axis) -> one dlwp_verify_error_sums call ------------------------------------------------------------- #
#: a, b: names of the operands (d = a - b); x_strides = (lead_stride, sample_stride, shift) in elements; lead f has
#: max(count0 - f * count_dec, 0) pairs of sample rows, a sample row is groups x run floats (include/dlwp_hip.h)
Plan = collections.namedtuple('Plan', 'a b a_strides b_strides leads count0 count_dec groups run')


def _prod(shape):
    p = 1
    for s in shape:
        p *= int(s)
    return p


def _groups_run(inner, axis, lead_axes):
    """(groups, run) for a difference of shape (lead_axes leading axes, sample axis, *inner) reduced over `axis`, or None where the
    device path does not cover that axis: None reduces a whole sample row; the tuple of the sample axis and every inner axis but
    the first keeps inner[0] groups."""
    inner = tuple(int(s) for s in inner)
    if not inner or _prod(inner) < 1:
        return None
    if axis is None:
        return 1, _prod(inner)
    rank = lead_axes + 1 + len(inner)
    try:
        ax = sorted(int(a) + rank if int(a) < 0 else int(a) for a in axis)
    except TypeError:
        return None
    if len(inner) >= 2 and ax == [lead_axes] + list(range(lead_axes + 2, rank)):
        return inner[0], _prod(inner[1:])
    return None


def _refuse_or_host(who, shape_a, shape_b):
    """shapes the device path does not take: numpy's own refusal now, as a ValueError -- or None: the host path broadcasts them"""
    try:
        np.broadcast_shapes(tuple(shape_a), tuple(shape_b))
    except ValueError:
        raise ValueError('%s: shapes %r and %r do not match' % (who, tuple(shape_a), tuple(shape_b)))
    return None


def plan_forecast(f_shape, v_shape, axis):
    """forecast_error as a Plan over ('forecast', 'valid'), or None for the host path"""
    f_shape, v_shape = tuple(f_shape), tuple(v_shape)
    if len(f_shape) == len(v_shape):
        if f_shape != v_shape:
            return _refuse_or_host('forecast_error', v_shape, f_shape)
        if len(f_shape) < 3 or f_shape[0] < 1:
            return None
        gr = _groups_run(f_shape[2:], axis, 1)
        if gr is None:
            return None
        n, row = f_shape[1], _prod(f_shape[2:])
        return Plan('forecast', 'valid', (n * row, row, 0), (n * row, row, 0), f_shape[0], n, 0, gr[0], gr[1])
    if len(f_shape) != len(v_shape) + 1 or len(v_shape) < 2 or f_shape[0] < 1:
        return None
    n, nv = f_shape[1], v_shape[0]
    if f_shape[2:] != v_shape[1:] or n < nv:       # step 0 compares valid[0:] with forecast[0, :nv]
        return _refuse_or_host('forecast_error', v_shape, (min(n, nv),) + f_shape[2:])
    gr = _groups_run(v_shape[1:], axis, 0)
    if gr is None:
        return None
    row = _prod(v_shape[1:])
    return Plan('valid', 'forecast', (0, row, 1), (n * row, row, 0), f_shape[0], nv, 1, gr[0], gr[1])


def plan_persistence(p_shape, v_shape, n_fhour, axis):
    """persistence_error as a Plan over ('valid', 'predictors'), or None for the host path"""
    p_shape, v_shape = tuple(p_shape), tuple(v_shape)
    if len(v_shape) < 2 or len(p_shape) != len(v_shape) or int(n_fhour) < 1:
        return None
    nv = v_shape[0]
    if p_shape[1:] != v_shape[1:] or p_shape[0] < nv:
        return _refuse_or_host('persistence_error', v_shape, (min(p_shape[0], nv),) + p_shape[1:])
    gr = _groups_run(v_shape[1:], axis, 0)
    if gr is None:
        return None
    row = _prod(v_shape[1:])
    return Plan('valid', 'predictors', (0, row, 1), (0, row, 0), int(n_fhour), nv, 1, gr[0], gr[1])


def plan_climo(v_shape, n_fhour, axis):
    """climo_error as a Plan over ('valid', 'mean'), mean = the NaN-skipping mean of valid over samples, or None"""
    v_shape = tuple(v_shape)
    if len(v_shape) < 2 or v_shape[0] < 1 or int(n_fhour) < 1:
        return None
    gr = _groups_run(v_shape[1:], axis, 0)
    if gr is None:
        return None
    row = _prod(v_shape[1:])
    return Plan('valid', 'mean', (0, row, 0), (0, 0, 0), int(n_fhour), v_shape[0], 1, gr[0], gr[1])


def finish(sums, method, grouped):
    """(leads, groups, 3) float64 sums d^2, sums |d|, counts -> what the host path returns: float32 (leads,) or (leads, groups)"""
    sums = np.asarray(sums, dtype=np.float64)
    count = sums[..., 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        val = np.where(count > 0, sums[..., 1 if method == 'mae' else 0] / count, np.nan)
        if method == 'rmse':
            val = np.sqrt(val)
        val = val.astype(np.float32)
    return val if grouped else val[:, 0]


def _wants_device(named, device):
    """Does this call take the device path?  Checks what can be checked without a device: a tensor argument must be a CUDA float32
    tensor (TypeError naming it), all tensors on one device, a numpy argument of the device path float32."""
    tensors = [(k, v) for k, v in named if isinstance(v, torch.Tensor)]
    if not tensors and device is None:
        return False
    for k, v in tensors:
        if not v.is_cuda or v.dtype != torch.float32:
            raise TypeError("'%s' must be a CUDA float32 tensor or a numpy array, got %s on %s" % (k, v.dtype, v.device))
    _common_device([v.device for _, v in tensors], device)
    for k, v in named:
        if not isinstance(v, torch.Tensor) and np.asarray(v).dtype != np.float32:
            raise TypeError("'%s' must be float32 on the device path, got %s" % (k, np.asarray(v).dtype))
    return True


def _common_device(devices, device):
    """the one device of the tensors and the keyword (None: no tensor and an index-less keyword -- the current device)"""
    want = None if device is None else torch.device(device)
    if want is not None and want.type != 'cuda':
        raise ValueError("'device' must be a CUDA device, got %r" % (device,))
    seen = {d.index for d in devices}
    if want is not None and want.index is not None:
        seen.add(want.index)
    seen = sorted(seen)
    if len(seen) > 1:
        raise ValueError('arguments on different devices: %s' % ', '.join('cuda:%d' % i for i in seen))
    if seen:
        return torch.device('cuda', seen[0])
    return want


def _to_host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _to_device(x, dev):
    if isinstance(x, torch.Tensor):
        return x.contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _run_plan(plan, named, device):
    from .. import ops
    dev = _common_device([v.device for _, v in named if isinstance(v, torch.Tensor)], device)
    if dev is None or dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):
        t = {k: _to_device(v, dev) for k, v in named}
        if plan.b == 'mean':
            t['mean'] = ops.verify_nanmean_samples(t['valid'])
        sums = ops.verify_error_sums(t[plan.a], plan.a_strides, t[plan.b], plan.b_strides, plan.leads, plan.count0,
                                     plan.count_dec, plan.groups, plan.run)
        return sums.cpu().numpy()


def forecast_error(forecast, valid, method='mse', axis=None, device=None):
    """Error of a time-series forecast (forecast step first).  `valid` either carries the same leading forecast-step axis
    -- then the mean runs over `axis` (default: everything but the step) -- or is the plain verification series, in which
    case forecast step f made from sample i is compared with valid[i + f].
    CUDA float32 tensors, or numpy arrays with device='cuda', are reduced on the device (module docstring)."""
    _check(method)
    named = (('forecast', forecast), ('valid', valid))
    if _wants_device(named, device):
        plan = plan_forecast(forecast.shape, valid.shape, axis)
        if plan is not None:
            return finish(_run_plan(plan, named, device), method, axis is not None)
        forecast, valid = _to_host(forecast), _to_host(valid)
    if forecast.ndim == valid.ndim:
        ax = tuple(range(1, valid.ndim)) if axis is None else axis
        return _error(valid - forecast, method, ax)
    n_val = valid.shape[0]
    return np.array([_error(valid[f:] - forecast[f, :n_val - f], method, axis) for f in range(forecast.shape[0])])


def persistence_error(predictors, valid, n_fhour, method='mse', axis=None, device=None):
    """Error of forecasting "no change": step f compares valid[i + f] with predictors[i]."""
    _check(method)
    named = (('predictors', predictors), ('valid', valid))
    if _wants_device(named, device):
        plan = plan_persistence(predictors.shape, valid.shape, n_fhour, axis)
        if plan is not None:
            return finish(_run_plan(plan, named, device), method, axis is not None)
        predictors, valid = _to_host(predictors), _to_host(valid)
    n = valid.shape[0]
    return np.array([_error(valid[f:] - predictors[:n - f], method, axis) for f in range(n_fhour)])


def climo_error(valid, n_fhour, method='mse', axis=None, device=None):
    """Error of forecasting the mean of the verification data itself, per forecast step (the reference shortens the
    sample window with the step, so the values differ slightly between steps)."""
    _check(method)
    named = (('valid', valid),)
    if _wants_device(named, device):
        plan = plan_climo(valid.shape, n_fhour, axis)
        if plan is not None:
            return finish(_run_plan(plan, named, device), method, axis is not None)
        valid = _to_host(valid)
    n = valid.shape[0]
    mean = np.nanmean(valid, axis=0)
    return np.array([_error(valid[:n - f] - mean, method, axis) for f in range(n_fhour)])
