"""
TimeSeriesEstimator: the rollout entry point examples/validate.py:197-205 uses (reference DLWP/model/extensions.py:21-303).

It steps a model forward over EVERY sample of a generator, feeding predictions back in as inputs, for models whose
inputs and outputs need not coincide (variable / level selection, fewer output than input time steps, an insolation
input channel that is known analytically).  The reference expresses the feedback with xarray label arithmetic
(`reindex`, `.loc[...] = ...`); xarray is absent from this image, so the same bookkeeping is restated on plain index
arithmetic.  Pinned by tests/golden/estimator.npz: the reference's own predict() run by oracle/make_golden.py under a
numpy-backed stub of the xarray calls it makes (13 cases: same / fewer / more output steps, variable selections,
insolation, interval, impute, keep_time_dim, varlev datasets).  What it reduces to, with
k = es + interval - 1 series steps covered per model call:

    p_{s+1}[i] = p_s[i + k]              rows re-indexed to the later start time; the last k rows run out of data (NaN,
                                         or the sample-mean input when impute=True, for the last `es` rows as the
                                         reference does)
    insolation channel of the last es rows: recomputed from the (known) times
    channels the model predicts (outputs_in_inputs): overwritten with the prediction --
        output_time_steps <= input_time_steps: the last `es` input time steps take all output time steps
        otherwise: the first (prefer_first_times) or last `input_time_steps` output time steps

When inputs == outputs (same channels, same time steps, no insolation) every channel is overwritten and the loop is
exactly DLWPNeuralNet.predict_timeseries: that case is dispatched to the device-resident hipGraph rollout.  Every other
case -- the one examples/validate.py:191-205 runs: insolation inputs, variable selections, interval > 1, fewer or more
output than input steps, impute -- is a FED rollout (engine.Model.fed_rollout_on_device, csrc/feedback.hip): the state
stays in HBM, one launch between two model calls does the row shift, the NaN / mean fill, the insolation of the rows
past the data (a table computed once for all lead times before the rollout: util.insolation depends on the times
only) and the scatter of the predicted channels, all calls in ONE hipGraph.  The reference's form of the same loop --
model.predict (H2D + D2H of the full state) and three host copies of the state per step -- remains for foreign model
objects, scalers the device path does not cover and DLWP_ESTIMATOR_HOST=1 (the parity tests run both and compare bit for bit).
The result carries the reference's coordinates (f_hour, time, [time_step,] varlev | variable, level, lat, lon) in a
LabeledArray.
"""
import warnings

import numpy as np

from ..util import insolation
from .generators import DataGenerator, LabeledArray, SeriesDataGenerator
from .models import DLWPFunctional, DLWPNeuralNet


def _labels(sel, da, dim):
    if dim in sel:
        return np.atleast_1d(np.asarray(sel[dim]))
    return np.asarray(da.coords[dim])


class TimeSeriesEstimator(object):
    def __init__(self, model, generator):
        if not isinstance(model, (DLWPNeuralNet, DLWPFunctional)):
            raise TypeError("'model' must be a valid instance of a DLWP model class")
        if not isinstance(generator, (DataGenerator, SeriesDataGenerator)):
            raise TypeError("'generator' must be a valid instance of a DLWP generator class")
        if isinstance(model, DLWPFunctional):
            warnings.warn('DLWPFunctional models are only partially supported by TimeSeriesEstimator. The '
                          'inputs/outputs to the model must be the same if the model predicts a sequence.')
        self.model = model
        self.generator = generator
        self._add_insolation = bool(getattr(generator, '_add_insolation', False))
        self._is_series = isinstance(generator, SeriesDataGenerator)
        da = generator.ds.predictors
        if not isinstance(da, LabeledArray):
            raise TypeError('TimeSeriesEstimator needs a dataset with coordinates (SeriesDataset / LabeledArray)')
        self._da = da
        self._uses_varlev = 'varlev' in da.dims
        samples = np.asarray(da.coords['sample'])
        self._dt = samples[1] - samples[0]
        self._interval = getattr(generator, '_interval', 1)
        in_sel = getattr(generator, '_input_sel', None) or {}
        out_sel = getattr(generator, '_output_sel', None) or {}
        if self._uses_varlev:
            self._input_sel = {'varlev': _labels(in_sel, da, 'varlev')}
            self._output_sel = {'varlev': _labels(out_sel, da, 'varlev')}
        else:
            self._input_sel = {'variable': _labels(in_sel, da, 'variable'), 'level': _labels(in_sel, da, 'level')}
            self._output_sel = {'variable': _labels(out_sel, da, 'variable'), 'level': _labels(out_sel, da, 'level')}
            for sel in (self._input_sel, self._output_sel):   # flattened 'variable/level' labels, variable-major
                sel['varlev'] = np.array(['/'.join([str(v), str(l)]) for v in sel['variable'] for l in sel['level']])
        self._outputs_in_inputs = {
            k: np.array([v for v in self._output_sel[k] if v in self._input_sel[k]]) for k in self._output_sel}
        if self._add_insolation:
            self._input_sel['varlev'] = np.concatenate([self._input_sel['varlev'], np.array(['SOL'])])
        self._input_time_steps = generator._input_time_steps if self._is_series else model.time_dim
        self._output_time_steps = generator._output_time_steps if self._is_series else model.time_dim

    def _fed_rollout_ok(self, p_shape, t_shape, n, calls=1):
        """Can the whole loop run on the device?  A dlwp_amd network behind a DLWPNeuralNet / single-output DLWPFunctional with
        identity scaling or a scaler / imputer the model call carries itself (DLWPNeuralNet._device_io), stored as (channels, lat,
        lon) with at most 128 state channels, and room in HBM for the two states, the series and the activations of all samples at
        once (the row shift couples the samples: they are not chunked)."""
        import os
        wrapper, net = self.model, getattr(self.model, 'model', None)
        if os.environ.get('DLWP_ESTIMATOR_HOST', '0') == '1' or not hasattr(net, 'fed_rollout_on_device'):
            return False
        if self._wrapper_scales() and not (hasattr(wrapper, '_device_io') and wrapper._device_io()):
            return False                                            # (a scaler / imputer the model call cannot carry: host loop)
        if len(net.outputs) != 1 or tuple(p_shape[1:]) != tuple(net.inputs[0].shape) or \
                tuple(t_shape[1:]) != tuple(net.outputs[0].shape) or net.device.type != 'cuda':
            return False
        state_c = int(np.prod(p_shape[1:-2]))
        if state_c > 128:
            return False
        import torch
        free = torch.cuda.mem_get_info(net.device)[0]
        need = 4 * n * sum(int(np.prod(b)) for b in net.infer_plan.buffers) + 8 * int(np.prod(p_shape)) + \
            4 * int(calls) * int(np.prod(t_shape)) + 8 * int(np.prod(t_shape))         # activations, two states, the series, staging
        return need < 0.8 * free

    def _wrapper_scales(self):
        return bool(getattr(self.model, 'impute', False) or getattr(self.model, 'scaler_type', None) is not None)

    # -- the forecast ------------------------------------------------------------------------------------------------ #
    def predict(self, steps, impute=False, keep_time_dim=False, prefer_first_times=True, **kwargs):
        """Step the model forward `steps` series steps for every sample of the generator.  Returns a LabeledArray with
        dims (f_hour, time, varlev | variable, level, lat, lon) -- or (f_hour, time, time_step, ...) with keep_time_dim
        -- float32, NaN where a forecast needed inputs beyond the end of the data."""
        if int(steps) < 1:
            raise ValueError('must use positive integer for steps')
        steps = int(steps)
        return_device = bool(kwargs.pop('return_device', False))     # (bench.py: the device series of the fed rollout, no D2H)
        t_in, t_out = self._input_time_steps, self._output_time_steps
        if t_out <= t_in:
            keep_inputs, es = True, t_out
            in_times = np.arange(t_in) - (t_in - t_out)
        else:
            keep_inputs = False
            es = t_in if prefer_first_times else t_out
            in_times = np.arange(t_in) + (0 if prefer_first_times else (t_out - t_in))
        effective_steps = int(np.ceil(steps / float(es)))
        k = es + self._interval - 1                                # series steps the window advances per model call

        gen = self.generator
        # the insolation of the rows past the data at every lead depends on the sample times only: its table (one vectorised call of
        # util.insolation, ~9 ms at 28 calls of the 88 x 180 grid) is computed on a thread of its own WHILE the predictors are
        # gathered and uploaded below (numpy releases the interpreter lock inside its kernels); joined where the device loop needs it
        sol_job = None
        if self._add_insolation and effective_steps > 1 and hasattr(getattr(self.model, 'model', None), 'fed_rollout_on_device'):
            import threading
            hw0 = tuple(gen.convolution_shape[-2:])
            coord0 = np.asarray(self._da.coords['sample'])[:gen._n_sample]
            if not self._is_series:
                coord0 = coord0 - self._dt * (t_in - 1)
            box = {}

            def work():
                try:
                    offs = np.array([[(s + 1) * k + m for m in range(t_in)] for s in range(effective_steps - 1)])
                    when = coord0[-es:][np.newaxis, :, np.newaxis] + offs[:, np.newaxis, :] * self._dt
                    uniq, inv = np.unique(when.ravel(), return_inverse=True)
                    box['sol'] = insolation(uniq, self._da.coords.get('lat'), self._da.coords.get('lon'))[inv.ravel()].reshape(
                        (effective_steps - 1, when.shape[1], t_in) + hw0)
                except BaseException as e:  # noqa: BLE001  (raised where the table is asked for)
                    box['error'] = e
            sol_job = (threading.Thread(target=work, daemon=True), box)
            sol_job[0].start()
        made = gen.generate_inputs() if hasattr(gen, 'generate_inputs') else None
        if made is not None:                                    # (the targets are never read here: only their shape)
            p, t_shape = made
        else:
            p, t = gen.generate([], scale_and_impute=False)
            t_shape = tuple((t[0] if isinstance(t, (list, tuple)) else t).shape)
        p_shape = tuple(p.shape)
        n = p_shape[0]
        hw = tuple(gen.convolution_shape[-2:])
        p = np.asarray(p, dtype=np.float32).reshape((n, t_in, -1) + hw)
        sample_coord = np.asarray(self._da.coords['sample'])[:gen._n_sample]
        if not self._is_series:
            sample_coord = sample_coord - self._dt * (t_in - 1)
        lat, lon = self._da.coords.get('lat'), self._da.coords.get('lon')
        in_labels = list(self._input_sel['varlev'])
        out_labels = list(self._output_sel['varlev'])
        shared = list(self._outputs_in_inputs['varlev'])
        idx_in = [in_labels.index(v) for v in shared]
        idx_out = [out_labels.index(v) for v in shared]
        p_mean = p.mean(axis=0) if impute else None
        arranged = None       # the device path hands the series back already in the returned layout
        alloc = lambda: np.full((effective_steps,) + t_shape, np.nan, dtype=np.float32)  # noqa: E731

        same_io = (keep_inputs and t_in == t_out and not self._add_insolation and self._interval == 1 and
                   in_labels == out_labels and isinstance(self.model, DLWPNeuralNet))
        if isinstance(self.model, DLWPFunctional) and self.model._n_steps > 1:
            result = alloc()
            result[:] = self.model.predict_timeseries(p.reshape(p_shape), steps, keep_time_dim=True,
                                                      **kwargs).reshape((-1,) + t_shape)[:effective_steps]
        elif same_io and not impute:
            # every input channel and time step is replaced by the prediction: the plain autoregressive rollout, which
            # DLWPNeuralNet.predict_timeseries keeps on the device (one hipGraph).  The reference's re-indexing blanks the
            # rows past the end of the data and then overwrites ALL of them with the forecast (extensions.py:214-240), so
            # every row stays finite at every lead -- pinned by tests/golden/estimator.npz ('same', 'varlev_same').
            series = self.model.predict_timeseries(p.reshape(p_shape), effective_steps * self.model.time_dim,
                                                   keep_time_dim=True, **kwargs)
            result = np.asarray(series).reshape((effective_steps,) + t_shape)
        elif self._fed_rollout_ok(p_shape, t_shape, n, effective_steps):
            # ---- the whole loop on the device: ONE hipGraph, the feedback launch between the calls (csrc/feedback.hip)
            c_in, c_out = len(in_labels), len(out_labels)
            src = list(range(t_in * c_in))                      # default: the same channel of row i + k
            for j_in, j_out in zip(idx_in, idx_out):
                if keep_inputs:
                    for m in range(es):
                        src[(t_in - es + m) * c_in + j_in] = -1 - (m * c_out + j_out)
                else:
                    first = 0 if prefer_first_times else t_out - t_in
                    for ts in range(t_in):
                        src[ts * c_in + j_in] = -1 - ((first + ts) * c_out + j_out)
            tail = min(es, n)
            sol, sol_map = None, None
            if self._add_insolation:
                sol_idx = in_labels.index('SOL')
                sol_map = [-1] * (t_in * c_in)
                for ts in range(t_in):
                    sol_map[ts * c_in + sol_idx] = ts
                # the times of the rows past the data at every lead: known before the rollout starts
                # (util.insolation is element-wise in the dates: ONE call over the distinct times, then a gather -- started on its own
                #  thread at the top of this method)
                sol = np.empty((max(effective_steps - 1, 1), tail, t_in) + hw, dtype=np.float32)
                if effective_steps > 1:
                    sol_job[0].join()
                    if 'error' in sol_job[1]:
                        raise sol_job[1]['error']
                    sol[:] = sol_job[1]['sol']
            if kwargs.get('verbose', 0) > 0:
                for s in range(effective_steps):
                    print('Time step %d/%d' % (s + 1, effective_steps))
            fed = dict(shift=k, tail=tail, sol=sol, sol_map=sol_map, mean=p_mean.reshape((t_in * c_in,) + hw) if impute else None)
            if self._wrapper_scales():          # the wrapper's imputer / scaler run inside every model call (_fed_rollout_ok)
                fed['scaled'] = True
            if return_device:
                return self.model.model.fed_rollout_on_device(p.reshape((n, t_in * c_in) + hw), effective_steps, src, **fed)
            # the series leaves for the host while the rollout runs, each call's block already in the returned layout: time first,
            # the [:, :, :es] cut, the [:steps] cut, (variable, level) in sorted label order (the tail of this method, on the device)
            perm = None
            if not self._uses_varlev:
                var, lev = np.asarray(self._output_sel['variable']), np.asarray(self._output_sel['level'])
                vo, lo = np.argsort(var, kind='stable'), np.argsort(lev, kind='stable')
                perm = [int(a) * len(lev) + int(b) for a in vo for b in lo]
            arranged = self.model.model.fed_rollout_to_host(
                p.reshape((n, t_in * c_in) + hw), effective_steps, src, t_out=t_out,
                kept=es if (not keep_inputs and prefer_first_times) else t_out, perm=perm, time_major=not keep_time_dim,
                blocks=effective_steps if keep_time_dim else steps, **fed)
        else:
            result = alloc()
            sample_now = sample_coord.copy()
            for s in range(effective_steps):
                if kwargs.get('verbose', 0) > 0:
                    print('Time step %d/%d' % (s + 1, effective_steps))
                result[s] = self.model.predict(p.reshape(p_shape), **kwargs)
                r = result[s].reshape((n, t_out, -1) + hw)
                # re-index the inputs to the start times of the next step: row i takes the data of row i + k
                p_next = np.full_like(p, np.nan)
                if k < n:
                    p_next[:n - k] = p[k:]
                p = p_next
                sample_now = sample_now + k * self._dt
                if impute:
                    p[-es:] = p_mean[np.newaxis]
                if self._add_insolation:
                    sol_idx = in_labels.index('SOL')
                    tail = sample_now[-es:]
                    p[-es:, :, sol_idx] = np.stack([insolation(tail + m * self._dt, lat, lon) for m in range(t_in)], axis=1)
                # feed the predicted channels back in; the others stay what the data (or the imputation) provided
                if keep_inputs:
                    p[:, t_in - es:, idx_in] = r[:, :, idx_out]
                elif prefer_first_times:
                    p[:, :, idx_in] = r[:, :t_in][:, :, idx_out]
                else:
                    p[:, :, idx_in] = r[:, -t_in:][:, :, idx_out]

        # -- coordinates --------------------------------------------------------------------------------------------- #
        time_coord = sample_coord + (t_in - 1) * self._dt
        if arranged is None:
            result = result.reshape((effective_steps, n, t_out, -1) + hw)
        if keep_time_dim:
            f_hour = np.array([self._dt * (1 + e * k) for e in range(effective_steps)])
            dims = ['f_hour', 'time', 'time_step', 'varlev', 'lat', 'lon']
            coords = {'f_hour': f_hour, 'time': time_coord, 'time_step': np.arange(t_out)}
        else:
            kept = es if (not keep_inputs and prefer_first_times) else t_out
            if arranged is None:
                result = result[:, :, :kept]
                result = result.transpose((0, 2, 1, 3, 4, 5)).reshape((-1, n, result.shape[3]) + hw)[:steps]
            f_hour = np.array([self._dt * (m + self._interval + e * (es - 1 + self._interval))
                               for e in range(effective_steps) for m in range(kept)])[:steps]
            dims = ['f_hour', 'time', 'varlev', 'lat', 'lon']
            coords = {'f_hour': f_hour, 'time': time_coord}
        coords.update({'varlev': np.asarray(out_labels)})
        if lat is not None:
            coords['lat'], coords['lon'] = lat, lon
        if not self._uses_varlev:
            # the reference unstacks a pandas MultiIndex.from_product((variable, level)) (extensions.py:298-302): the new
            # coordinates are the index LEVELS, i.e. the labels in sorted order, not in selection order
            var, lev = np.asarray(self._output_sel['variable']), np.asarray(self._output_sel['level'])
            ax = dims.index('varlev')
            vo, lo = np.argsort(var, kind='stable'), np.argsort(lev, kind='stable')
            if arranged is None:
                result = result.reshape(result.shape[:ax] + (len(var), len(lev)) + result.shape[ax + 1:])
                result = np.take(np.take(result, vo, axis=ax), lo, axis=ax + 1)
            else:
                result = arranged.reshape(arranged.shape[:ax] + (len(var), len(lev)) + arranged.shape[ax + 1:])
            dims = dims[:ax] + ['variable', 'level'] + dims[ax + 1:]
            coords.pop('varlev')
            coords.update({'variable': var[vo], 'level': lev[lo]})
        elif arranged is not None:
            result = arranged
        return LabeledArray(result, coords, tuple(dims))
