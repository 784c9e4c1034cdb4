"""
Forecast error measures of the validation scripts (reference DLWP/model/verify.py, called from
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

The rest of the reference module (DLWP/model/verify.py:105-273) follows the same rule, on LabeledArray / SeriesDataset objects
(model/generators.py) where the reference takes xarray objects: monthly_climo_error (the mean per calendar month over the whole
record by dlwp_verify_label_nanmean, the anomaly of the validation times by dlwp_verify_label_error_sums),
verification_from_samples / verification_from_series (one int64 row array from window_rows, executed by numpy take or by
dlwp_gather_rows_fill with the same bits; verification_tensor keeps the result in HBM for forecast_error), and the two host
reshapes predictors_to_time_series / add_metadata_to_forecast.  DESIGN.md 5.30 has the kernels and the measurements.

Beyond the reference module: forecast_skill / persistence_skill score the same series with a weight per latitude row and against a
climatology -- one field, or a table per label (monthly_climatology, month_labels) -- and return a Skill tuple per lead (and variable):
weighted mse, rmse, mae, the bias, the uncentred anomaly correlation of the reference's training metric (custom.anomaly_correlation)
and the centred one.  On the device one pass of dlwp_verify_skill_sums (csrc/skill.hip) leaves ten float64 sums per lead and group,
which finish_skill turns into the scores; the host path computes the same definition in numpy (float32 d = fc - ob, fa = fc - c,
oa = ob - c, float64 sums) and is no fallback of the device path: both refuse an `axis` they do not cover.  An ensemble is scored
through its mean: forecast_skill(ensemble.ensemble_mean_spread(series)[0], valid, ...).  DESIGN.md 5.38 has the kernel and the bounds.
forecast_skill_map / persistence_skill_map give the same scores at every grid point, reduced over the samples of a lead
(dlwp_verify_skill_map, csrc/skill_map.hip, finishes them on the device: CUDA arguments give CUDA maps); skill_map_sums returns the
nine float64 planes, which add over ranks or sample chunks, and finish_skill_map finishes them.  DESIGN.md 5.40.
forecast_spectrum / persistence_spectrum look at the same pairs by scale, which no point-wise score does: per lead (and variable) the
zonal power spectrum of the forecast beside that of the truth, the power of the error and the coherence at every wavenumber, as a
Spectrum tuple.  On the device dlwp_verify_spectrum_sums (csrc/spectrum.hip) transforms the longitude rows of valid and of d =
forecast - valid on the fp32 matrix cores and leaves four float64 sums per wavenumber; spectrum_sums returns them (they add over ranks
or sample chunks), finish_spectrum finishes them; the host path states the definition with np.fft.rfft in float64.  DESIGN.md 5.41.
climatological_quantiles gives the other statistic of the record that verification needs beside the monthly mean: quantiles per grid
point and label (calendar month, a grouping of one's own, or the whole record) -- the per-point `thresholds` of ensemble.event_scores.
On the device dlwp_verify_label_quantiles (csrc/quantile.hip) selects exactly, by bisection on the ordered bits of the values, so the
record is not downloaded; label_quantiles_host is the same definition in numpy, and both return the same bits.  DESIGN.md 5.42.

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


# -- month-aware climatology (reference DLWP/model/verify.py:105-132) --------------------------------------------------------------- #
def _cuda_device(values, device):
    """the device of the device path, or None for the host path"""
    if isinstance(values, torch.Tensor):
        _wants_device((('da', values),), device)
        dev = _common_device([values.device], device)
    elif device is None:
        return None
    else:
        dev = _common_device([], device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _find_times(times, wanted):
    """int64 positions of `wanted` in the time coordinate `times` (any order), -1 where a time is absent: np.searchsorted on the sorted
    times plus an equality check"""
    times, wanted = np.asarray(times), np.asarray(wanted)
    if times.dtype.kind == 'M' and wanted.dtype.kind == 'M':
        common = np.promote_types(times.dtype, wanted.dtype)
        times, wanted = times.astype(common), wanted.astype(common)
    if times.size == 0:
        return np.full(wanted.shape, -1, np.int64)
    order = np.argsort(times, kind='stable')
    ordered = times[order]
    pos = np.minimum(np.searchsorted(ordered, wanted), ordered.size - 1)
    return np.where(ordered[pos] == wanted, order[pos], -1).astype(np.int64)


def _months(times):
    """calendar month - 1 of a datetime64 coordinate"""
    times = np.asarray(times)
    if times.dtype.kind != 'M':
        raise TypeError('the time coordinate must be datetime64, got %s' % times.dtype)
    return (times.astype('datetime64[M]').astype(np.int64) % 12).astype(np.int32)


def label_nanmean_host(x, labels, n_labels):
    """(n_labels,) + x.shape[1:] float32: per label the NaN-skipping mean of its rows, summed in float64 in sample order, divided once
    and rounded once; NaN where a label has no non-NaN sample"""
    out = np.full((n_labels,) + x.shape[1:], np.nan, np.float32)
    for l in range(n_labels):
        rows = np.flatnonzero(labels == l)
        s, n = np.zeros(x.shape[1:], np.float64), np.zeros(x.shape[1:], np.int64)
        for r in rows:
            ok = ~np.isnan(x[r])
            with np.errstate(invalid='ignore'):
                s += np.where(ok, x[r], np.float32(0)).astype(np.float64)
            n += ok
        with np.errstate(divide='ignore', invalid='ignore'):
            out[l] = np.where(n > 0, s / n, np.nan).astype(np.float32)
    return out


def monthly_climo_error(da, val_set, n_fhour=None, method='mse', return_da=False, device=None):
    """Month-aware climatology error: the NaN-skipping mean per calendar month over ALL of `da` (a LabeledArray with a datetime64
    'sample' or 'time' coordinate) is the forecast for the times in `val_set`; one number over everything, repeated n_fhour times if
    that is given, and with return_da the anomaly da.sel(time=val_set) - climatology as a LabeledArray.
    Host path (numpy values): the climatology in float64 rounded once to float32, d in float32, the final mean in float64.  Device
    path (device='cuda', or da.values a CUDA float32 tensor): the record is uploaded once, dlwp_verify_label_nanmean and
    dlwp_verify_label_error_sums reduce it there; only the month labels and the row indices are computed here."""
    _check(method)
    time_dim = 'sample' if 'sample' in da.dims else 'time'
    ax = da.dims.index(time_dim)
    times = np.asarray(da.coords[time_dim])
    months = _months(times)
    wanted = np.asarray(list(val_set) if not isinstance(val_set, np.ndarray) else val_set).reshape(-1)
    rows = _find_times(times, wanted)
    if wanted.size == 0 or (rows < 0).any():
        raise KeyError('time(s) %r not found on dimension %r' % (wanted[rows < 0].tolist() if wanted.size else [], time_dim))
    dev = _cuda_device(da.values, device)
    if dev is None:
        x = np.moveaxis(da.values, ax, 0)
        if x.dtype != np.float32:
            x = x.astype(np.float32)
        climo = label_nanmean_host(x, months, 12)
        with np.errstate(invalid='ignore'):
            anomaly = x[rows] - climo[months[rows]]
        ok = ~np.isnan(anomaly)
        z = np.where(ok, anomaly, np.float32(0)).astype(np.float64)
        count = int(ok.sum())
        with np.errstate(over='ignore', invalid='ignore'):
            total = float(np.abs(z).sum()) if method == 'mae' else float((z * z).sum())
        me = total / count if count else float('nan')
        if method == 'rmse':
            me = float(np.sqrt(me))
        anomaly = np.moveaxis(anomaly, 0, ax)
    else:
        from .. import ops
        if not isinstance(da.values, torch.Tensor) and np.asarray(da.values).dtype != np.float32:
            raise TypeError("'da' must be float32 on the device path, got %s" % np.asarray(da.values).dtype)
        with torch.cuda.device(dev):
            x = _to_device(da.values, dev)
            if ax:
                x = x.movedim(ax, 0).contiguous()
            table = ops.verify_label_nanmean(x, months, 12)
            out = ops.verify_label_error_sums(x, rows, months[rows], table, anomaly=return_da)
            sums, anomaly = out if return_da else (out, None)
            me = float(finish(sums.cpu().numpy().reshape(1, 1, 3), method, False)[0])
            if return_da:
                anomaly = anomaly.movedim(0, ax) if ax else anomaly
                if not isinstance(da.values, torch.Tensor):
                    anomaly = anomaly.cpu().numpy()
    if n_fhour is not None:
        me = np.array([me] * n_fhour)
    if not return_da:
        return me
    from .generators import LabeledArray
    coords = dict(da.coords)
    coords[time_dim] = times[rows]
    return me, LabeledArray(anomaly, coords, da.dims)


# -- reshaping helpers (reference DLWP/model/verify.py:135-198) ---------------------------------------------------------------------- #
def _meta_coord(meta_ds, name):
    c = getattr(meta_ds, name)
    return np.asarray(getattr(c, 'values', c))


def predictors_to_time_series(predictors, time_steps, has_time_dim=True, use_first_step=False, meta_ds=None):
    """Predictors of a model with several input time steps as one continuous series: the last step of every sample (the first with
    use_first_step).  has_time_dim=False: axis 1 is time_steps * channels.  With meta_ds (a SeriesDataset-like object: `dims` and
    coordinates) the result is a LabeledArray over ('time', 'variable', 'level', 'lat', 'lon') or ('time', 'varlev', 'lat', 'lon')."""
    idx = 0 if use_first_step else -1
    if not has_time_dim:
        predictors = predictors.reshape((predictors.shape[0], time_steps, -1) + tuple(predictors.shape[2:]))
    result = predictors[:, idx]
    if meta_ds is None:
        return result
    from .generators import LabeledArray
    if 'level' in meta_ds.dims:
        dims = ('variable', 'level', 'lat', 'lon')
        result = result.reshape((meta_ds.dims['sample'],) + tuple(meta_ds.dims[d] for d in dims))
    else:
        dims = ('varlev', 'lat', 'lon')
    coords = {d: _meta_coord(meta_ds, d) for d in dims}
    coords['time'] = _meta_coord(meta_ds, 'sample')
    return LabeledArray(result, coords, ('time',) + dims)


def add_metadata_to_forecast(forecast, f_hour, meta_ds):
    """A forecast (forecast_hour, time, variable, lat, lon) as a LabeledArray with the initialisation times and coordinates of meta_ds"""
    nf = len(f_hour)
    if nf != forecast.shape[0]:
        raise ValueError("'f_hour' coordinate must have same size as the first axis of 'forecast'")
    from .generators import LabeledArray
    if 'level' in meta_ds.dims:
        dims = ('variable', 'level', 'lat', 'lon')
        forecast = forecast.reshape((nf, meta_ds.dims['sample']) + tuple(meta_ds.dims[d] for d in dims))
    else:
        dims = ('varlev', 'lat', 'lon')
    coords = {d: _meta_coord(meta_ds, d) for d in dims}
    coords['f_hour'] = np.asarray(f_hour)
    coords['time'] = _meta_coord(meta_ds, 'sample')
    return LabeledArray(forecast, coords, ('f_hour', 'time') + dims)


# -- verification windows (reference DLWP/model/verify.py:201-273) ------------------------------------------------------------------- #
def window_rows(times, init_dates, forecast_steps, dt, first):
    """(forecast_steps, n) int64: the row of the record (time coordinate `times`) that holds init_dates[i] + (first + f) * dt hours,
    -1 where the record has no state at that time -- reindex(method=None) as an index array"""
    init_dates = np.asarray(init_dates)
    lead = (np.arange(int(forecast_steps), dtype=np.int64) + int(first)) * int(dt)
    wanted = init_dates[None, :] + lead[:, None].astype('timedelta64[h]')
    return _find_times(times, wanted)


def take_rows_fill_host(record, rows):
    """record[rows] as float32 with NaN rows where rows < 0 (the host executor of window_rows)"""
    out = np.take(record, np.maximum(rows, 0), axis=0).astype(np.float32, copy=False)
    out[rows < 0] = np.nan
    return out


def _verification(ds, all_ds, forecast_steps, dt, first, source, device, as_tensor):
    forecast_steps = int(forecast_steps)
    if forecast_steps < 1:
        raise ValueError("'forecast_steps' must be an integer >= 1")
    dt = int(dt)
    if dt < 1:
        raise ValueError("'dt' must be an integer >= 1")
    dims = [d for d in ds.predictors.dims if d.lower() != 'time_step']
    if not dims or dims[0] != 'sample':
        raise ValueError("the first dimension of 'ds.predictors' must be 'sample', got %r" % (ds.predictors.dims,))
    valid_da = getattr(all_ds if all_ds is not None else ds, source)
    if source == 'targets':
        valid_da = valid_da.isel(time_step=0)
    if valid_da.dims[0] != 'sample' or tuple(valid_da.shape[1:]) != tuple(ds.dims[d] for d in dims[1:]):
        raise ValueError('the verification record %r %r does not match the dataset %r' % (valid_da.dims, tuple(valid_da.shape), ds.dims))
    rows = window_rows(valid_da.coords['sample'], ds.predictors.coords['sample'], forecast_steps, dt, first)
    record = valid_da.values
    on_device = as_tensor or device is not None or isinstance(record, torch.Tensor)
    dev = _cuda_device(record, device or 'cuda') if on_device else None
    if dev is None:
        values = take_rows_fill_host(record, rows)
    else:
        from .. import ops
        if not isinstance(record, torch.Tensor) and np.asarray(record).dtype != np.float32:
            record = np.asarray(record).astype(np.float32)
        with torch.cuda.device(dev):
            values = ops.gather_rows_fill(_to_device(record, dev), rows)
        if as_tensor:
            return values
        values = values.cpu().numpy()
    from .generators import LabeledArray
    coords = {d: ds.predictors.coords[d] for d in dims[1:] if d in ds.predictors.coords}
    coords['time'] = np.asarray(ds.predictors.coords['sample'])
    coords['f_hour'] = np.arange(dt, dt * forecast_steps + 1, dt).astype('timedelta64[h]')
    return LabeledArray(values, coords, ['f_hour', 'time'] + dims[1:])


def verification_from_samples(ds, all_ds=None, forecast_steps=1, dt=6, device=None):
    """Forecast verification (f_hour, time, ...) float32 for a dataset of samples: lead f of initialisation date t is
    targets.isel(time_step=0) of `all_ds` (or `ds`) at t + f * dt hours, f = 0 .. forecast_steps - 1, NaN where there is no such
    state.  device='cuda' gathers on the device (dlwp_gather_rows_fill): the same bits."""
    return _verification(ds, all_ds, forecast_steps, dt, 0, 'targets', device, False)


def verification_from_series(ds, all_ds=None, forecast_steps=1, dt=6, device=None):
    """Forecast verification (f_hour, time, ...) float32 for a series dataset: lead f of initialisation date t is the predictors of
    `all_ds` (or `ds`) at t + (f + 1) * dt hours, NaN where there is no such state.  device='cuda' gathers on the device."""
    return _verification(ds, all_ds, forecast_steps, dt, 1, 'predictors', device, False)


def verification_tensor(ds, all_ds=None, forecast_steps=1, dt=6, kind='series', device='cuda'):
    """The values of verification_from_series (kind='series') or verification_from_samples (kind='samples') as a CUDA float32 tensor
    (forecast_steps, n, ...), never downloaded: forecast_error scores a predict_timeseries(..., return_device=True) rollout against
    it without a host array."""
    if kind not in ('series', 'samples'):
        raise ValueError("'kind' must be 'series' or 'samples'")
    first, source = (1, 'predictors') if kind == 'series' else (0, 'targets')
    return _verification(ds, all_ds, forecast_steps, dt, first, source, device, True)


# -- latitude-weighted skill: rmse, bias, anomaly correlation (csrc/skill.hip) --------------------------------------- #
#: per lead (and group): float32 scores, int64 count of the pairs behind them; NaN where nothing was counted or sum w is 0
Skill = collections.namedtuple('Skill', 'mse rmse mae bias acc acc_centered count')

#: fc, ob: names of the operands; x_strides = (lead_stride, sample_stride, shift) as in Plan; label_strides = (lead_stride, shift):
#: the label of pair (f, i) is labels[f * lead_stride + i + f * shift]
SkillPlan = collections.namedtuple('SkillPlan', 'fc ob fc_strides ob_strides label_strides leads count0 count_dec groups run')


def finish_skill(sums, grouped=True):
    """(..., 10) float64 sums of dlwp_verify_skill_sums (include/dlwp_hip.h) -> Skill, computed in float64 and cast once.  Tables of
    several ranks or chunks add before the finish.  grouped=False drops a groups axis of one: (leads, 1, 10) -> (leads,)."""
    s = np.asarray(sums, dtype=np.float64)
    s0, s1, s2, s3, s4, s5, s6, s7, s8, n = (s[..., k] for k in range(10))
    with np.errstate(all='ignore'):
        some = (n > 0) & (s0 > 0)
        s0 = np.where(some, s0, np.nan)
        mse = s2 / s0
        m_f, m_o = s4 / s0, s5 / s0
        den = np.sqrt(s7 * s8)
        acc = np.where(den > 0, s6 / den, np.nan)
        den = np.sqrt((s7 / s0 - m_f * m_f) * (s8 / s0 - m_o * m_o))
        acc_c = np.where(den > 0, (s6 / s0 - m_f * m_o) / den, np.nan)
        scores = [mse, np.sqrt(mse), s3 / s0, s1 / s0, np.where(some, acc, np.nan), np.where(some, acc_c, np.nan)]
        scores = [v.astype(np.float32) for v in scores]
    out = Skill(*(scores + [n.astype(np.int64)]))
    return out if grouped else Skill(*(v[..., 0] for v in out))


def area_weights(lats):
    """cos(latitude) per row as float32, never negative: in float32 cos(90 degrees) is -4.37e-8, and a negative weight would break
    both the scores and their error bounds"""
    from .. import custom
    return np.maximum(custom.latitude_weights(lats, 'cosine'), 0).astype(np.float32)


def month_labels(times):
    """calendar month - 1 (0 .. 11) of a datetime64 array of any shape, int32: the labels of monthly_climatology's table"""
    return _months(times)


def monthly_climatology(da, device=None):
    """The (12, ...) float32 table monthly_climo_error builds internally: the NaN-skipping mean per calendar month over ALL of `da` (a
    LabeledArray with a datetime64 'sample' or 'time' coordinate, which becomes the leading axis), the same bits.  device='cuda' or
    CUDA values reduce on the device (dlwp_verify_label_nanmean); the result is a CUDA tensor for CUDA values and numpy otherwise."""
    time_dim = 'sample' if 'sample' in da.dims else 'time'
    ax = da.dims.index(time_dim)
    months = _months(np.asarray(da.coords[time_dim]))
    dev = _cuda_device(da.values, device)
    if dev is None:
        x = np.moveaxis(da.values, ax, 0)
        if x.dtype != np.float32:
            x = x.astype(np.float32)
        return label_nanmean_host(x, months, 12)
    from .. import ops
    if not isinstance(da.values, torch.Tensor) and np.asarray(da.values).dtype != np.float32:
        raise TypeError("'da' must be float32 on the device path, got %s" % np.asarray(da.values).dtype)
    with torch.cuda.device(dev):
        x = _to_device(da.values, dev)
        if ax:
            x = x.movedim(ax, 0).contiguous()
        table = ops.verify_label_nanmean(x, months, 12)
        return table if isinstance(da.values, torch.Tensor) else table.cpu().numpy()


# -- climatological quantiles: per-point event thresholds (no counterpart in the reference module) ----------------------------------- #
def _order_keys(x):
    """the unsigned keys that order float32 values by their bits: -0.0 < +0.0, infinities at the ends; NaNs get the largest key"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    keys = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(x), np.uint32(0xffffffff), keys)


def _from_keys(keys):
    return np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32).view(np.float32)


def label_quantiles_host(x, labels, n_labels, q, method='linear', return_count=False):
    """The definition dlwp_verify_label_quantiles implements (include/dlwp_hip.h), in numpy: x (count, ...) float32, integer labels
    (count,) in [0, n_labels), q a scalar or K probabilities -> (K, n_labels) + x.shape[1:] float32.  Per label and column the NaNs are
    dropped, the n values left are sorted by the key of their bits into s, h = (n - 1) * q in float64, and 'lower' / 'higher' /
    'nearest' return s[floor(h)] / s[ceil(h)] / s[rint(h)] with the sample's bits, 'linear' a = s[floor(h)] where h is whole and else
    float32(a + (b - a) * (h - floor(h))) in float64 with b the next sample; NaN where n == 0.  return_count adds the (n_labels,) +
    x.shape[1:] int32 array of n.  numpy.nanquantile on a float64 copy gives the same values; this one fixes the bits as well."""
    from .. import ops
    m = ops.quantile_method(method, 'label_quantiles_host')
    q = ops.quantile_probabilities(q, None, 'label_quantiles_host')
    x, labels = np.asarray(x), np.asarray(labels)
    if x.dtype != np.float32 or x.ndim < 2:
        raise TypeError('label_quantiles_host: x must be a float32 array (count, ...), got %s of rank %d' % (x.dtype, x.ndim))
    if labels.shape != (x.shape[0],) or labels.dtype.kind not in 'iu':
        raise ValueError('label_quantiles_host: labels must be %d integers, got %s %r' % (x.shape[0], labels.dtype, labels.shape))
    if n_labels < 1 or (labels.size and (int(labels.min()) < 0 or int(labels.max()) >= n_labels)):
        raise ValueError('label_quantiles_host: labels must lie in [0, %d)' % n_labels)
    inner = x.shape[1:]
    flat = x.reshape(x.shape[0], -1)
    out = np.full((q.size, n_labels, flat.shape[1]), np.nan, np.float32)
    counts = np.zeros((n_labels, flat.shape[1]), np.int32)
    for l in range(n_labels):
        rows = flat[labels == l]
        if not rows.shape[0]:
            continue
        keys = np.sort(_order_keys(rows), axis=0)            # NaNs last
        n = np.count_nonzero(~np.isnan(rows), axis=0)
        counts[l] = n
        last = np.maximum(n - 1, 0)

        def pick(rank):
            return _from_keys(np.take_along_axis(keys, np.minimum(rank.astype(np.int64), last)[None], axis=0)[0])
        for k in range(q.size):
            h = last.astype(np.float64) * q[k]
            lo = np.floor(h)
            if m == 0:
                a, b, g = pick(lo), pick(lo + 1), h - lo
                with np.errstate(invalid='ignore', over='ignore'):
                    mid = (a.astype(np.float64) + (b.astype(np.float64) - a.astype(np.float64)) * g).astype(np.float32)
                mid = np.where(np.isnan(mid), np.float32(np.nan), mid)         # one NaN: 0x7fc00000
                val = np.where(g == 0, a, mid)
            else:
                val = pick(lo if m == 1 else (np.ceil(h) if m == 2 else np.rint(h)))
            out[k, l] = np.where(n > 0, val, np.float32(np.nan))
    out = out.reshape((q.size, n_labels) + inner)
    return (out, counts.reshape((n_labels,) + inner)) if return_count else out


def climatological_quantiles(da, q, labels='month', n_labels=None, method='linear', return_count=False, device=None):
    """Quantiles of a record per grid point: the per-point `thresholds` of ensemble.event_scores / ensemble_exceedance -- terciles, "the
    95th percentile of this month".  `da` is a LabeledArray with a datetime64 'sample' or 'time' coordinate, which becomes the leading
    axis as in monthly_climatology; q a scalar or a sequence of K probabilities (at most 8 on the device).  labels='month' groups by
    calendar month (12 labels, month_labels), labels=None takes the whole record as one label, an integer array (one label per time)
    with n_labels any other grouping, seasons for instance.  Returns (K, n_labels, ...) float32 -- a scalar q keeps the leading axis of
    length 1 -- NaN where a label has no non-NaN sample at a point, and with return_count the (n_labels, ...) int32 sample counts.
    method: 'linear' | 'lower' | 'higher' | 'nearest' as in numpy.nanquantile.  device='cuda' or CUDA values select on the device
    (dlwp_verify_label_quantiles: the record is not downloaded); the result is a CUDA tensor for CUDA values and numpy otherwise.
    Host and device return the same bits (label_quantiles_host is the definition)."""
    from .. import ops
    who = 'climatological_quantiles'
    on_device = isinstance(da.values, torch.Tensor) or device is not None
    m = ops.quantile_method(method, who)
    q = ops.quantile_probabilities(q, ops.QUANTILE_MAX_K if on_device else None, who)
    time_dim = 'sample' if 'sample' in da.dims else 'time'
    ax = da.dims.index(time_dim)
    count = int(da.values.shape[ax])
    if isinstance(labels, str):
        if labels != 'month':
            raise ValueError("%s: labels %r, expected 'month', None or an integer array" % (who, labels))
        labels, n_labels = _months(np.asarray(da.coords[time_dim])), 12
    elif labels is None:
        labels, n_labels = np.zeros(count, np.int32), 1
    else:
        labels = np.asarray(labels)
        if n_labels is None:
            raise ValueError('%s: an array of labels needs n_labels' % who)
    n_labels = int(n_labels)
    if labels.shape != (count,) or labels.dtype.kind not in 'iu':
        raise ValueError('%s: labels must be %d integers, got %s %r' % (who, count, labels.dtype, labels.shape))
    if not 1 <= n_labels <= ops.VERIFY_MAX_LABELS or (count and (int(labels.min()) < 0 or int(labels.max()) >= n_labels)):
        raise ValueError('%s: labels must lie in [0, n_labels) with n_labels in 1 .. %d' % (who, ops.VERIFY_MAX_LABELS))
    if on_device and not isinstance(da.values, torch.Tensor) and np.asarray(da.values).dtype != np.float32:
        raise TypeError("'da' must be float32 on the device path, got %s" % np.asarray(da.values).dtype)
    dev = _cuda_device(da.values, device)
    if dev is None:
        x = np.moveaxis(da.values, ax, 0)
        if x.dtype != np.float32:
            x = x.astype(np.float32)
        return label_quantiles_host(x, labels, n_labels, q, method, return_count)
    with torch.cuda.device(dev):
        x = _to_device(da.values, dev)
        if ax:
            x = x.movedim(ax, 0).contiguous()
        res = ops.verify_label_quantiles(x, labels, n_labels, q, method, want_count=return_count)
        if isinstance(da.values, torch.Tensor):
            return res
        return tuple(t.cpu().numpy() for t in res) if return_count else res.cpu().numpy()


def _skill_groups_run(who, inner, axis, lead_axes):
    gr = _groups_run(inner, axis, lead_axes)
    if gr is None:
        raise ValueError("%s: 'axis' must be None or the tuple that keeps the lead and the first inner axis of rows %r, got %r"
                         % (who, tuple(inner), axis))
    return gr


def plan_forecast_skill(f_shape, v_shape, axis):
    """forecast_skill as a SkillPlan over ('forecast', 'valid').  Pure host code; ValueError for shapes that do not match and for an
    `axis` other than None or the tuple that keeps the lead and the first inner axis."""
    f_shape, v_shape = tuple(int(s) for s in f_shape), tuple(int(s) for s in v_shape)
    if len(f_shape) == len(v_shape):
        if f_shape != v_shape or len(f_shape) < 3 or f_shape[0] < 1:
            raise ValueError('forecast_skill: shapes %r and %r do not match' % (f_shape, v_shape))
        groups, run = _skill_groups_run('forecast_skill', f_shape[2:], axis, 1)
        n, row = f_shape[1], _prod(f_shape[2:])
        return SkillPlan('forecast', 'valid', (n * row, row, 0), (n * row, row, 0), (n, 0), f_shape[0], n, 0, groups, run)
    n, nv = (f_shape[1], v_shape[0]) if len(f_shape) >= 2 and v_shape else (0, 0)
    if len(f_shape) != len(v_shape) + 1 or len(v_shape) < 2 or f_shape[0] < 1 or f_shape[2:] != v_shape[1:] or n < nv:
        raise ValueError('forecast_skill: shapes %r and %r do not match' % (f_shape, v_shape))
    groups, run = _skill_groups_run('forecast_skill', v_shape[1:], axis, 0)
    row = _prod(v_shape[1:])
    return SkillPlan('forecast', 'valid', (n * row, row, 0), (0, row, 1), (0, 1), f_shape[0], nv, 1, groups, run)


def plan_persistence_skill(p_shape, v_shape, n_fhour, axis):
    """persistence_skill as a SkillPlan over ('predictors', 'valid'): the forecast of every lead is predictors[i]"""
    p_shape, v_shape = tuple(int(s) for s in p_shape), tuple(int(s) for s in v_shape)
    if len(v_shape) < 2 or len(p_shape) != len(v_shape) or p_shape[1:] != v_shape[1:] or p_shape[0] < v_shape[0]:
        raise ValueError('persistence_skill: shapes %r and %r do not match' % (p_shape, v_shape))
    if int(n_fhour) < 1:
        raise ValueError("persistence_skill: 'n_fhour' must be >= 1")
    groups, run = _skill_groups_run('persistence_skill', v_shape[1:], axis, 0)
    row = _prod(v_shape[1:])
    return SkillPlan('predictors', 'valid', (0, row, 0), (0, row, 1), (0, 1), int(n_fhour), v_shape[0], 1, groups, run)


def _skill_extras(who, plan, inner, label_shape, climatology, labels, weights):
    """The optional arguments, checked on the host before anything is uploaded: (table (L, *inner) or None, flat int32 labels or None,
    float32 weights or None).  A table of one field has no labels; a table of several needs labels of `label_shape`."""
    from .. import ops
    inner = tuple(inner)
    table = None
    if climatology is not None:
        shape = tuple(climatology.shape)
        if shape == inner:
            if labels is not None:
                raise ValueError("%s: 'labels' need a (L, ...) climatology table, got one field" % who)
            table = climatology.reshape((1,) + inner)
        elif shape[1:] == inner and 1 <= shape[0] <= ops.VERIFY_MAX_LABELS:
            if labels is None:
                raise ValueError("%s: a climatology table needs 'labels' of shape %r" % (who, tuple(label_shape)))
            table = climatology
        else:
            raise ValueError("%s: 'climatology' must have the shape %r of a sample row or (L <= %d,) + that shape, got %r"
                             % (who, inner, ops.VERIFY_MAX_LABELS, shape))
    elif labels is not None:
        raise ValueError("%s: 'labels' without a climatology table" % who)
    if labels is not None:
        if tuple(np.shape(labels)) != tuple(label_shape):
            raise ValueError("%s: 'labels' must have shape %r, got %r" % (who, tuple(label_shape), tuple(np.shape(labels))))
        labels = ops.skill_labels(labels, table.shape[0])
    if weights is not None:
        weights = ops.skill_weights(weights)
        if len(inner) < 2 or weights.size != inner[-2] or plan.run % (inner[-2] * inner[-1]):
            raise ValueError("%s: 'weights' must hold one weight per row of the second-to-last axis of %r inside a group, got %d"
                             % (who, inner, weights.size))
    return table, labels, weights


def _skill_host(fc_rows, ob_rows, plan, inner, table, labels, weights):
    """the definition in numpy: per lead the float32 d, fa, oa of the rows the plan pairs, float64 sums -> (leads, groups, 10)"""
    out = np.zeros((plan.leads, plan.groups, 10), np.float64)
    grouped = plan.groups > 1 or plan.run != _prod(inner)
    w = 1.0 if weights is None else weights.astype(np.float64).reshape(-1, 1)
    for f in range(plan.leads):
        cnt = max(plan.count0 - f * plan.count_dec, 0)
        if cnt == 0:
            continue
        fc, ob = fc_rows(f, cnt), ob_rows(f, cnt)
        skip = np.zeros(cnt, bool)
        with np.errstate(invalid='ignore'):
            d = fc - ob
            if table is None:
                fa, oa = fc, ob
            else:
                if labels is None:
                    c = table[0]
                else:
                    at = f * plan.label_strides[0] + f * plan.label_strides[1]
                    lab = labels[at:at + cnt]
                    skip = lab < 0
                    c = table[np.maximum(lab, 0)]
                fa, oa = fc - c, ob - c
        assert d.dtype == fa.dtype == oa.dtype == np.float32
        ok = ~(np.isnan(d) | np.isnan(fa) | np.isnan(oa)) & ~skip.reshape((cnt,) + (1,) * len(inner))
        d, fa, oa = (np.where(ok, v, np.float32(0)).astype(np.float64) for v in (d, fa, oa))
        wk = ok * w
        ax = tuple(a for a in range(d.ndim) if not (grouped and a == 1))
        with np.errstate(over='ignore', invalid='ignore'):
            terms = (wk, wk * d, wk * d * d, wk * np.abs(d), wk * fa, wk * oa, wk * fa * oa, wk * fa * fa, wk * oa * oa, ok)
            out[f] = np.stack([np.sum(t, axis=ax, dtype=np.float64) for t in terms], axis=-1).reshape(plan.groups, 10)
    return out


def _skill_device(plan, named, table, labels, weights, w_inner, device):
    from .. import ops
    dev = _common_device([v.device for _, v in named if isinstance(v, torch.Tensor)], device)
    if dev is None or dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):
        t = {k: _to_device(v, dev) for k, v in named}
        sums = ops.verify_skill_sums(t[plan.fc], plan.fc_strides, t[plan.ob], plan.ob_strides, plan.leads, plan.count0, plan.count_dec,
                                     plan.groups, plan.run, climo=None if table is None else _to_device(table, dev), labels=labels,
                                     label_strides=plan.label_strides, weights=weights, w_inner=w_inner)
        return sums.cpu().numpy()


def _skill(who, plan, fc_name, forecast, valid, inner, label_shape, climatology, labels, weights, axis, device, fc_rows, ob_rows):
    named = [(fc_name, forecast), ('valid', valid)] + ([] if climatology is None else [('climatology', climatology)])
    on_device = _wants_device(named, device)
    table, labels, weights = _skill_extras(who, plan, inner, label_shape, climatology, labels, weights)
    if on_device:
        sums = _skill_device(plan, named[:2], table, labels, weights, inner[-1], device)
    else:
        f32 = lambda x: None if x is None else np.asarray(x).astype(np.float32, copy=False)      # noqa: E731
        forecast, valid, table = f32(forecast), f32(valid), f32(table)
        sums = _skill_host(lambda f, cnt: fc_rows(forecast, f, cnt), lambda f, cnt: ob_rows(valid, f, cnt), plan, inner, table, labels,
                           weights)
    return finish_skill(sums, axis is not None)


def forecast_skill(forecast, valid, climatology=None, labels=None, weights=None, axis=None, device=None):
    """Weighted skill of a time-series forecast (forecast step first) per lead -- and per variable with the `axis` tuple that keeps the
    lead and the first inner axis -- as a Skill tuple.  `valid` carries the same leading step axis, or is the plain verification
    series: lead f of sample i then meets valid[i + f].  climatology: None, one field of the shape of a sample row, or a (L, ...) table
    (L <= 64) with integer `labels` of the valid times, shaped (F, N) or (Nv,) like the leading axes of `valid`, entries in [-1, L),
    -1 skips the pair.  weights: one weight per row of the second-to-last axis (area_weights(lats)), finite, >= 0, not all zero.
    d = forecast - valid, fa = forecast - c, oa = valid - c in float32; pairs with a NaN among them are skipped; sums in float64.
    CUDA float32 tensors, or numpy arrays with device='cuda', are reduced on the device; any other `axis` is a ValueError."""
    plan = plan_forecast_skill(forecast.shape, valid.shape, axis)
    per_lead = len(forecast.shape) == len(valid.shape)
    inner = tuple(int(s) for s in valid.shape[2 if per_lead else 1:])
    label_shape = tuple(valid.shape[:2]) if per_lead else tuple(valid.shape[:1])
    ob_rows = (lambda v, f, cnt: v[f, :cnt]) if per_lead else (lambda v, f, cnt: v[f:f + cnt])
    return _skill('forecast_skill', plan, 'forecast', forecast, valid, inner, label_shape, climatology, labels, weights, axis, device,
                  lambda x, f, cnt: x[f, :cnt], ob_rows)


def persistence_skill(predictors, valid, n_fhour, climatology=None, labels=None, weights=None, axis=None, device=None):
    """forecast_skill of forecasting "no change": lead f compares predictors[i] with valid[i + f]; `labels` (Nv,) follow `valid`"""
    plan = plan_persistence_skill(predictors.shape, valid.shape, n_fhour, axis)
    inner = tuple(int(s) for s in valid.shape[1:])
    return _skill('persistence_skill', plan, 'predictors', predictors, valid, inner, tuple(valid.shape[:1]), climatology, labels,
                  weights, axis, device, lambda x, f, cnt: x[:cnt], lambda v, f, cnt: v[f:f + cnt])


# -- skill per grid point: the same sums reduced over the samples of a lead (csrc/skill_map.hip) ---------------------- #
def _skill_map_host(fc_rows, ob_rows, plan, inner, table, labels):
    """the definition in numpy: per lead the float32 d, fa, oa of the rows the plan pairs, float64 sums over the samples at every
    point -> (leads, 9) + inner"""
    out = np.zeros((plan.leads, 9) + tuple(inner), np.float64)
    for f in range(plan.leads):
        cnt = max(plan.count0 - f * plan.count_dec, 0)
        if cnt == 0:
            continue
        fc, ob = fc_rows(f, cnt), ob_rows(f, cnt)
        skip = np.zeros(cnt, bool)
        with np.errstate(invalid='ignore'):
            d = fc - ob
            if table is None:
                fa, oa = fc, ob
            else:
                if labels is None:
                    c = table[0]
                else:
                    at = f * plan.label_strides[0] + f * plan.label_strides[1]
                    lab = labels[at:at + cnt]
                    skip = lab < 0
                    c = table[np.maximum(lab, 0)]
                fa, oa = fc - c, ob - c
        assert d.dtype == fa.dtype == oa.dtype == np.float32
        ok = ~(np.isnan(d) | np.isnan(fa) | np.isnan(oa)) & ~skip.reshape((cnt,) + (1,) * len(inner))
        d, fa, oa = (np.where(ok, v, np.float32(0)).astype(np.float64) for v in (d, fa, oa))
        with np.errstate(over='ignore', invalid='ignore'):
            terms = (d, d * d, np.abs(d), fa, oa, fa * oa, fa * fa, oa * oa, ok)
            out[f] = np.stack([np.sum(t, axis=0, dtype=np.float64) for t in terms])
    return out


def finish_skill_map(sums):
    """A (leads, 9, ...) float64 table of skill_map_sums -> Skill with fields of shape (leads, ...): finish_skill's formulas with
    S0 = the count, computed in float64 and cast once.  Tables of several ranks or sample chunks add before the finish.  A numpy table
    is finished in numpy, a CUDA tensor on the device (dlwp_verify_skill_map_finish) and stays there."""
    if isinstance(sums, torch.Tensor):
        from .. import ops
        if sums.dim() < 3 or sums.shape[1] != 9:
            raise ValueError('finish_skill_map: expected a (leads, 9, ...) table, got %r' % (tuple(sums.shape),))
        shape = (sums.shape[0],) + tuple(sums.shape[2:])
        with torch.cuda.device(sums.device):
            scores, counts = ops.verify_skill_map_finish(sums.contiguous())
        return Skill(*([scores[:, k].reshape(shape) for k in range(6)] + [counts.reshape(shape).to(torch.int64)]))
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim < 3 or s.shape[1] != 9:
        raise ValueError('finish_skill_map: expected a (leads, 9, ...) table, got %r' % (s.shape,))
    s = np.moveaxis(s, 1, -1)
    return finish_skill(np.concatenate([s[..., 8:], s], axis=-1))


def _skill_map(who, plan, fc_name, forecast, valid, inner, label_shape, climatology, labels, device, split, fc_rows, ob_rows, want):
    """want: 'sums' -> the (leads, 9) + inner table; 'scores' -> the Skill.  CUDA arguments give CUDA results, numpy ones numpy."""
    split = int(split)
    if split < 0:
        raise ValueError("%s: 'split' must be >= 0, got %d" % (who, split))
    named = [(fc_name, forecast), ('valid', valid)] + ([] if climatology is None else [('climatology', climatology)])
    on_device = _wants_device(named, device)
    table, labels, _ = _skill_extras(who, plan, inner, label_shape, climatology, labels, None)
    if not on_device:
        f32 = lambda x: None if x is None else np.asarray(x).astype(np.float32, copy=False)      # noqa: E731
        forecast, valid, table = f32(forecast), f32(valid), f32(table)
        sums = _skill_map_host(lambda f, cnt: fc_rows(forecast, f, cnt), lambda f, cnt: ob_rows(valid, f, cnt), plan, inner, table,
                               labels)
        return sums if want == 'sums' else finish_skill_map(sums)
    from .. import ops
    stay = any(isinstance(v, torch.Tensor) for _, v in named)
    dev = _common_device([v.device for _, v in named if isinstance(v, torch.Tensor)], device)
    if dev is None or dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    shape = (plan.leads,) + tuple(inner)
    with torch.cuda.device(dev):
        t = {k: _to_device(v, dev) for k, v in named[:2]}
        sums, scores, counts = ops.verify_skill_map(t[plan.fc], plan.fc_strides, t[plan.ob], plan.ob_strides, plan.leads, plan.count0,
                                                    plan.count_dec, plan.run, climo=None if table is None else _to_device(table, dev),
                                                    labels=labels, label_strides=plan.label_strides, split=split,
                                                    want_sums=want == 'sums', want_scores=want == 'scores')
        if want == 'sums':
            sums = sums.reshape((plan.leads, 9) + tuple(inner))
            return sums if stay else sums.cpu().numpy()
        if stay:
            return Skill(*([scores[:, k].reshape(shape) for k in range(6)] + [counts.reshape(shape).to(torch.int64)]))
        scores, counts = scores.cpu().numpy(), counts.cpu().numpy()      # 28 bytes per point
        return Skill(*([scores[:, k].reshape(shape) for k in range(6)] + [counts.reshape(shape).astype(np.int64)]))


def _forecast_rows(forecast, valid):
    """how a forecast (step first) meets either form of `valid`: (inner shape of a sample row, shape of the labels, rows of the
    forecast, rows of `valid`), the last two as functions of (array, lead, count)"""
    per_lead = len(forecast.shape) == len(valid.shape)
    inner = tuple(int(s) for s in valid.shape[2 if per_lead else 1:])
    label_shape = tuple(valid.shape[:2]) if per_lead else tuple(valid.shape[:1])
    ob_rows = (lambda v, f, cnt: v[f, :cnt]) if per_lead else (lambda v, f, cnt: v[f:f + cnt])
    return inner, label_shape, (lambda x, f, cnt: x[f, :cnt]), ob_rows


def _forecast_skill_map(who, forecast, valid, climatology, labels, device, split, want):
    plan = plan_forecast_skill(forecast.shape, valid.shape, None)
    inner, label_shape, fc_rows, ob_rows = _forecast_rows(forecast, valid)
    return _skill_map(who, plan, 'forecast', forecast, valid, inner, label_shape, climatology, labels, device, split, fc_rows, ob_rows,
                      want)


def forecast_skill_map(forecast, valid, climatology=None, labels=None, device=None):
    """forecast_skill at every grid point: per lead the scores over the SAMPLES at each point of a sample row, as a Skill tuple whose
    fields have the shape (leads,) + the shape of a sample row (count: int64).  Shapes, the two forms of `valid`, `climatology`,
    `labels` and the refusals are forecast_skill's; there are no weights (a weight is constant per point and cancels) and no `axis`.
    d = forecast - valid, fa = forecast - c, oa = valid - c in float32; a pair with a NaN among them, or with label -1, is skipped at
    that point; sums in float64.  NaN where nothing was counted or a variance is not positive (a single sample).  CUDA float32
    tensors are reduced on the device (csrc/skill_map.hip) and give CUDA tensors; numpy arrays give numpy arrays, computed in numpy,
    or on the device with device='cuda'."""
    return _forecast_skill_map('forecast_skill_map', forecast, valid, climatology, labels, device, 0, 'scores')


def persistence_skill_map(predictors, valid, n_fhour, climatology=None, labels=None, device=None):
    """forecast_skill_map of forecasting "no change": lead f compares predictors[i] with valid[i + f]; `labels` (Nv,) follow `valid`"""
    plan = plan_persistence_skill(predictors.shape, valid.shape, n_fhour, None)
    inner = tuple(int(s) for s in valid.shape[1:])
    return _skill_map('persistence_skill_map', plan, 'predictors', predictors, valid, inner, tuple(valid.shape[:1]), climatology, labels,
                      device, 0, lambda x, f, cnt: x[:cnt], lambda v, f, cnt: v[f:f + cnt], 'scores')


def skill_map_sums(forecast, valid, climatology=None, labels=None, device=None, split=0):
    """The (leads, 9) + row-shape float64 table behind forecast_skill_map: sum d, d^2, |d|, fa, oa, fa oa, fa^2, oa^2 and the pairs
    counted, per point.  Tables of several ranks or sample chunks add; finish_skill_map makes the scores.  split (device path): 0 =
    the library's rule, a positive number = that many chunks of the sample axis, each added in sample order and the chunks in chunk
    order -- callers that compare or add tables fix it."""
    return _forecast_skill_map('skill_map_sums', forecast, valid, climatology, labels, device, split, 'sums')


# -- zonal power spectra per lead: power by wavenumber, error power, coherence (csrc/spectrum.hip) ------------------- #
#: per lead (and group): wavenumber (K,) int64; float32 (leads[, groups], K) power of the forecast, of the truth and of the error (their
#: sums over k are the weighted means of fc^2, ob^2, d^2), ratio = power_forecast / power_valid and the coherence |<F conj O>|^2 /
#: (<|F|^2> <|O|^2>); int64 count of the longitude rows behind them.  NaN where nothing was counted or a denominator is not positive
Spectrum = collections.namedtuple('Spectrum', 'wavenumber power_forecast power_valid power_error ratio coherence count')


def finish_spectrum(sums, norm, grouped=True):
    """(..., 4, K) float64 sums and (..., 2) norm of spectrum_sums / dlwp_verify_spectrum_sums (include/dlwp_hip.h) -> Spectrum,
    computed in float64 and cast once.  Tables of several ranks or sample chunks add before the finish.  grouped=False drops a groups
    axis of one: (leads, 1, 4, K) -> fields of (leads, K)."""
    s, nrm = np.asarray(sums, dtype=np.float64), np.asarray(norm, dtype=np.float64)
    if s.ndim < 2 or s.shape[-2] != 4 or nrm.shape != s.shape[:-2] + (2,):
        raise ValueError('finish_spectrum: expected sums (..., 4, K) and norm (..., 2), got %r and %r' % (s.shape, nrm.shape))
    sw, n = nrm[..., 0], nrm[..., 1]
    with np.errstate(all='ignore'):
        some = (n > 0) & (sw > 0)
        den = np.where(some, sw, np.nan)[..., None]
        s0, s1, s2, s3 = (s[..., q, :] / den for q in range(4))
        p_f = s0 + s1 + 2.0 * s2
        ratio = np.where(s0 > 0, p_f / s0, np.nan)
        dd = p_f * s0
        coh = np.where(dd > 0, ((s0 + s2) ** 2 + s3 ** 2) / dd, np.nan)
        fields = [v.astype(np.float32) for v in (p_f, s0, s1, ratio, coh)]
    out = Spectrum(*([np.arange(s.shape[-1], dtype=np.int64)] + fields + [n.astype(np.int64)]))
    if grouped:
        return out
    return Spectrum(*([out.wavenumber] + [v[..., 0, :] for v in out[1:6]] + [out.count[..., 0]]))


def _spectrum_host(fc_rows, ob_rows, plan, inner, weights):
    """the definition in numpy: per lead the float32 d = fc - ob of the rows the plan pairs, np.fft.rfft of ob and d in float64 along the
    last axis, longitude rows with a non-finite fc, ob or d skipped -> (leads, groups, 4, K) sums, (leads, groups, 2) norm"""
    width = int(inner[-1])
    k = width // 2 + 1
    c = np.full(k, 2.0)
    c[0] = 1.0
    if width % 2 == 0:
        c[-1] = 1.0
    c /= float(width) * float(width)
    sums = np.zeros((plan.leads, plan.groups, 4, k), np.float64)
    norm = np.zeros((plan.leads, plan.groups, 2), np.float64)
    lat = plan.run // width if weights is None else weights.size
    w_lat = np.ones(lat, np.float64) if weights is None else weights.astype(np.float64)
    for f in range(plan.leads):
        cnt = max(plan.count0 - f * plan.count_dec, 0)
        if cnt == 0:
            continue
        shape = (cnt, plan.groups, plan.run // (lat * width), lat, width)
        fc, ob = fc_rows(f, cnt).reshape(shape), ob_rows(f, cnt).reshape(shape)
        with np.errstate(invalid='ignore', over='ignore'):
            d = fc - ob
        assert d.dtype == np.float32
        ok = np.isfinite(fc).all(axis=-1) & np.isfinite(ob).all(axis=-1) & np.isfinite(d).all(axis=-1)
        o_k = np.fft.rfft(np.where(ok[..., None], ob, np.float32(0)).astype(np.float64), axis=-1)
        d_k = np.fft.rfft(np.where(ok[..., None], d, np.float32(0)).astype(np.float64), axis=-1)
        w = ok * w_lat
        cross = d_k * np.conj(o_k)
        terms = (o_k.real ** 2 + o_k.imag ** 2, d_k.real ** 2 + d_k.imag ** 2, cross.real, cross.imag)
        for q, term in enumerate(terms):
            sums[f, :, q] = np.einsum('sgrh,sgrhk->gk', w, term) * c
        norm[f, :, 0] = w.sum(axis=(0, 2, 3))
        norm[f, :, 1] = ok.sum(axis=(0, 2, 3))
    return sums, norm


def _spectrum_device(plan, named, width, weights, device):
    from .. import ops
    dev = _common_device([v.device for _, v in named if isinstance(v, torch.Tensor)], device)
    if dev is None or dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):
        t = {k: _to_device(v, dev) for k, v in named}
        sums, norm = ops.verify_spectrum_sums(t[plan.fc], plan.fc_strides, t[plan.ob], plan.ob_strides, plan.leads, plan.count0,
                                              plan.count_dec, plan.groups, plan.run, width, weights=weights)
        return sums.cpu().numpy(), norm.cpu().numpy()


def _spectrum_sums(who, plan, fc_name, forecast, valid, inner, weights, device, fc_rows, ob_rows):
    """(sums, norm) as float64 numpy; every refusal happens here, before anything is uploaded"""
    from .. import ops
    named = [(fc_name, forecast), ('valid', valid)]
    on_device = _wants_device(named, device)
    if len(inner) < 2:
        raise ValueError('%s: a sample row needs a latitude and a longitude axis, got rows of shape %r' % (who, tuple(inner)))
    width = int(inner[-1])
    if width < ops.SPECTRUM_MIN_WIDTH:
        raise ValueError('%s: rows of %d longitudes, at least %d expected' % (who, width, ops.SPECTRUM_MIN_WIDTH))
    if on_device and width > ops.SPECTRUM_MAX_WIDTH:
        raise ValueError('%s: rows of %d longitudes, the device path takes at most %d (the host path has no limit; a resident series '
                         'is not downloaded silently)' % (who, width, ops.SPECTRUM_MAX_WIDTH))
    _, _, weights = _skill_extras(who, plan, inner, (), None, None, weights)
    if on_device:
        return _spectrum_device(plan, named, width, weights, device)
    f32 = lambda x: np.asarray(x).astype(np.float32, copy=False)      # noqa: E731
    forecast, valid = f32(forecast), f32(valid)
    return _spectrum_host(lambda f, cnt: fc_rows(forecast, f, cnt), lambda f, cnt: ob_rows(valid, f, cnt), plan, inner, weights)


def spectrum_sums(forecast, valid, weights=None, axis=None, device=None, n_fhour=None):
    """The float64 tables behind forecast_spectrum (n_fhour=None) or persistence_spectrum (n_fhour given; `forecast` holds the
    predictors): sums (leads, groups, 4, K) = sum w c_k |O_k|^2, sum w c_k |D_k|^2, sum w c_k Re(D_k conj O_k), sum w c_k Im(D_k conj
    O_k) with O = rfft(valid), D = rfft(forecast - valid) along the last axis, K = W // 2 + 1, c_k the one-sided Parseval factors over
    W^2; norm (leads, groups, 2) = sum w and the longitude rows counted.  groups is 1 for axis=None.  Numpy arrays either way; tables
    of several ranks or sample chunks add, finish_spectrum makes the Spectrum."""
    forecast, valid = (x if isinstance(x, torch.Tensor) else np.asarray(x) for x in (forecast, valid))      # lists and the like
    if n_fhour is None:
        plan = plan_forecast_skill(forecast.shape, valid.shape, axis)
        inner, _, fc_rows, ob_rows = _forecast_rows(forecast, valid)
        return _spectrum_sums('forecast_spectrum', plan, 'forecast', forecast, valid, inner, weights, device, fc_rows, ob_rows)
    plan = plan_persistence_skill(forecast.shape, valid.shape, n_fhour, axis)
    inner = tuple(int(s) for s in valid.shape[1:])
    return _spectrum_sums('persistence_spectrum', plan, 'predictors', forecast, valid, inner, weights, device,
                          lambda x, f, cnt: x[:cnt], lambda v, f, cnt: v[f:f + cnt])


def forecast_spectrum(forecast, valid, weights=None, axis=None, device=None):
    """Zonal power spectra of a time-series forecast (forecast step first) per lead -- and per variable with the `axis` tuple that keeps
    the lead and the first inner axis -- as a Spectrum tuple.  A sample row is (..., H, W): the last axis is longitude (periodic), the
    second-to-last latitude.  `valid` carries the same leading step axis, or is the plain verification series: lead f of sample i then
    meets valid[i + f].  Per longitude row d = forecast - valid is rounded once in float32 and valid and d are transformed along
    longitude (the forecast's transform is their sum): power_valid, power_error and power_forecast sum over the wavenumbers to the
    weighted means of valid^2, d^2 and forecast^2; ratio = power_forecast / power_valid falls below 1 where a forecast is smoothed;
    coherence says up to which wavenumber the forecast still carries the phase of the truth.  weights: one weight per latitude row
    (area_weights(lats)), finite, >= 0, not all zero.  A longitude row with a non-finite value in forecast, valid or d is skipped
    whole; `count` says how many rows were counted.  Needs W >= 4.  CUDA float32 tensors, or numpy arrays with device='cuda', are
    transformed on the device (csrc/spectrum.hip, W <= 512; a wider row is a ValueError, never a silent download); the result is a
    tuple of numpy arrays either way."""
    return finish_spectrum(*spectrum_sums(forecast, valid, weights, axis, device), grouped=axis is not None)


def persistence_spectrum(predictors, valid, n_fhour, weights=None, axis=None, device=None):
    """forecast_spectrum of forecasting "no change": lead f compares predictors[i] with valid[i + f]"""
    n_fhour = int(n_fhour)
    if n_fhour < 1:
        raise ValueError("persistence_spectrum: 'n_fhour' must be >= 1")
    return finish_spectrum(*spectrum_sums(predictors, valid, weights, axis, device, n_fhour=n_fhour), grouped=axis is not None)
