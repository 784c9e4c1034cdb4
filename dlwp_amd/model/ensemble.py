"""
Ensemble verification: what reduces ACROSS the member axis of a perturbed-initial-condition rollout -- the ensemble mean and
spread, the error of the mean, the spread-skill ratio, the CRPS and the rank histogram.  The reference has no such module: its
examples/plot_ensemble.py:242,269 takes np.mean over members on the host.  Here the series predict_timeseries(...,
return_device=True) leaves in HBM is scored where it is (csrc/ensemble.hip); DESIGN.md 5.35 has the kernels and the measurements.

Definitions (the contract; the host and the device path compute exactly these).  A column is one (lead t, sample s, field point
p): M member values x_0 .. x_{M-1} (float32) and, for the scores, one verifying value y (float32).  All per-column arithmetic is
float64 on the float32 inputs; comparisons are made on the float32 values themselves.

* mean = (sum_i x_i) / M, summed in member order.
* variance: shifted sums with d_i = x_i - x_0 (exact in float64): var_ddof = (sum d_i^2 - (sum d_i)^2 / M) / (M - ddof), and
  spread = sqrt(max(var, 0)).
* CRPS terms: A = (1/M) sum_i |x_i - y| and B = sum_{i<j} |x_i - x_j|, computed as sum_k (2k - M + 1) x_(k) over the ascending
  order x_(0) <= ... <= x_(M-1) (each product of a small integer and a float32 is exact in float64);
  crps = A - B / M^2 and fair_crps = A - B / (M (M - 1)).
* rank r = #{i : x_i < y} in 0 .. M.  Ties count as not below; there is no randomisation, so repeated runs give identical
  histograms.
* NaN rule: the mean and spread FIELDS are NaN where any member is NaN; for the SCORES a column with a NaN y or any NaN member is
  skipped and not counted.

Two paths, as in model/verify.py: numpy arguments without `device=` run the numpy float64 code below; CUDA float32 tensors, or
numpy arrays with device='cuda', are reduced by dlwp_ens_mean_spread / dlwp_ens_score_sums, and only (leads, groups, 6) float64
sums and the int64 histogram come back.  The device path covers 2 <= M <= 256 and, for `axis`, forecast_error's rule: None (one
value per lead) and the tuple that keeps the lead and the first field axis (one value per lead and variable); anything else runs
the host code on downloaded arrays.

Event verification (event_scores, ensemble_exceedance, finish_events; csrc/events.hip): with what probability
does the ensemble say the field exceeds a threshold, and are those probabilities any good.  Thresholds are float32, K of them
(1 <= K <= 8 on the device, any K >= 1 on the host).  A 1-D `thresholds` of K values applies to every point; anything with more
axes is broadcast (numpy rules) to (K, *field): a threshold per point, such as climatological terciles, or per variable through
shape (K, V, 1, 1).  verify.climatological_quantiles(record, [1 / 3, 2 / 3], ...)[:, m] -- the terciles of label (month) m, taken on
the device where the record lives -- is a valid `thresholds` argument as it stands, CUDA tensor or numpy array.

* event='above': member i shows the event when x_i > thr and the event verified when y > thr; event='below': x_i < thr and
  y < thr.  Comparisons are made on the float32 values; ties are no event (the rank rule: ties count as not below).
  n = #{i : event_i} in 0 .. M, and o = 1 if the event verified, else 0.
* table[t, g, k, n, o] (int64): the columns of cell (t, g) with that n and o, over the columns where y is not NaN, no member is
  NaN and thr is not NaN.  Everything below follows from it, so tables of several ranks or files can be added and finished.
* prob[k, t, s, p] = float32(double(n) / double(M)); NaN where any member of the column is NaN or thr is NaN; y plays no part.
* finish_events, in float64 from the integer table, cast once to float32.  Per cell and threshold, with N_n = table[n, 0] +
  table[n, 1], O_n = table[n, 1], N = sum N_n, p_n = n / M and obar = sum O_n / N:
    brier       = (1/N) sum_n [O_n (p_n - 1)^2 + (N_n - O_n) p_n^2]
    fair_brier  = brier - (1/N) sum_n N_n n (M - n) / (M^2 (M - 1))                     (Ferro's finite-ensemble correction)
    reliability = (1/N) sum_{N_n > 0} N_n (p_n - O_n / N_n)^2,   resolution = (1/N) sum_{N_n > 0} N_n (O_n / N_n - obar)^2
    uncertainty = obar (1 - obar),   brier_skill = 1 - brier / uncertainty (NaN where uncertainty is 0),   base_rate = obar
    obs_freq[n] = O_n / N_n (NaN where N_n = 0) and fcst_hist[n] = N_n (int64): the reliability diagram and its sharpness histogram
    ROC, for j = 0 .. M + 1 and the decision "warn when n >= j": hit_rate[j] = sum_{n >= j} O_n / sum O_n, false_alarm_rate[j] =
    sum_{n >= j} (N_n - O_n) / sum (N_n - O_n), roc_area the trapezoid over those M + 2 points; all three NaN where there are no
    events or no non-events
    rps = sum_k brier_k and fair_rps = sum_k fair_brier_k: the ranked probability score for ascending thresholds, NaN where the K
    thresholds of a cell did not count the same N (NaN thresholds);   count = N (int64);   everything NaN where N = 0.
  Both paths produce the same table and share finish_events: they return identical bits.

The generator (perturb_members, ensemble_forecast; csrc/perturb.hip) MAKES such an ensemble:
out[s, m, k, i, j] = x[s, k, i, j] + sign * sigma[k] * zeta, the product and the sum each rounded once to float32.

* global member g = first_member + m.  With `control`, member g == 0 is x itself, bit for bit, and p = g - 1; otherwise p = g.  With
  `antithetic`, draw d = p >> 1 and sign = +1 for even p, -1 for odd p; otherwise d = p and sign = +1.
* white noise z(d, s, k, i, j), defined for every integer virtual row |i| < 32768: Philox-4x32-10 with key (seed lo, seed hi) and
  counter (j >> 2, (i + 32768) + 65536 k, d, s); words (w0, w1) give columns 4q, 4q + 1 and (w2, w3) columns 4q + 2, 4q + 3 by
  u1 = (2 (wa >> 9) + 1) 2^-24, u2 = (wb >> 8) 2^-24 (both exact in float32), r = sqrt(-2 ln u1), z_even = r cos(2 pi u2),
  z_odd = r sin(2 pi u2); |z| <= sqrt(48 ln 2).  white_noise() evaluates the pair in float64; z is that value rounded to float32 (the
  kernel's float32 evaluation is within a few float32 roundings of it).
* smoothing: R = ceil(3 L) <= 16 per axis, taps g_a proportional to exp(-a^2 / 2 L^2), normalised in float64 to sum g^2 = 1 and then
  rounded to float32 (smoothing_taps).  zeta(i, j) = sum_a g_a sum_b g_b z(i + a, (j + b) mod W): the longitude pass first, then
  latitude, taps in ascending order, float32 accumulators from 0, every product and every sum rounded.  Rows beyond the grid exist
  in counter space, so there is no boundary rule.  R_x > W, K >= 65536 and H + R_y >= 32768 are refused.
* NaN in x stays NaN at that element only.
"""
import collections

import numpy as np
import torch

from .verify import _common_device, _groups_run, _prod, _to_device, _to_host, _wants_device

MAX_DEVICE_MEMBERS = 256
MAX_DEVICE_THRESHOLDS = 8
MAX_RADIUS = 16

#: rmse_mean, mae_mean, spread, spread_skill (= spread / rmse_mean), crps, fair_crps: float32 (T,) or (T, G); rank_hist: int64
#: (T[, G], M + 1); count: int64, the columns counted; crps_field: the per-column crps (T, S, *field) or None
EnsembleScores = collections.namedtuple('EnsembleScores', 'rmse_mean mae_mean spread spread_skill crps fair_crps rank_hist count crps_field')

#: brier .. roc_area: float32 (T[, G], K); rps, fair_rps: float32 (T[, G]); obs_freq (float32) and fcst_hist (int64): (T[, G], K,
#: M + 1); hit_rate, false_alarm_rate: float32 (T[, G], K, M + 2); count: int64 (T[, G], K); table: int64 (T[, G], K, M + 1, 2);
#: prob_field: float32 (K, T, S, *field) or None
EventScores = collections.namedtuple('EventScores', 'brier fair_brier reliability resolution uncertainty brier_skill base_rate roc_area '
                                     'rps fair_rps obs_freq fcst_hist hit_rate false_alarm_rate count table prob_field')


def _layout(forecast, member_axis):
    """(T, S, M, field) of a forecast (T, S, M, *field) (member_axis=2) or (T, M, S, *field) (member_axis=1)"""
    if member_axis not in (1, 2):
        raise ValueError("'member_axis' must be 1 or 2, got %r" % (member_axis,))
    shape = tuple(int(s) for s in forecast.shape)
    if len(shape) < 4:
        raise ValueError("'forecast' must be (T, S, M, *field) or (T, M, S, *field) with at least one field axis, got %r" % (shape,))
    t, s, m = shape[0], shape[3 - member_axis], shape[member_axis]
    if m < 2:
        raise ValueError('an ensemble needs at least 2 members, got %d' % m)
    if t < 1 or s < 1 or _prod(shape[3:]) < 1:
        raise ValueError("'forecast' %r has an empty axis" % (shape,))
    return t, s, m, shape[3:]


def _check_ddof(ddof):
    if ddof not in (0, 1):
        raise ValueError("'ddof' must be 0 or 1, got %r" % (ddof,))


def _device_of(named, device):
    dev = _common_device([v.device for _, v in named if isinstance(v, torch.Tensor)], device)
    if dev is None or dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


# -- the host path: numpy float64 on one lead at a time ----------------------------------------------------------------------------- #
def _moments_host(x):
    """x: float32 (S, M, *field) -> float64 (member-order sum, sum d, sum d^2), each (S, *field)"""
    x0 = x[:, 0].astype(np.float64)
    s = np.zeros(x0.shape, np.float64)
    sd = np.zeros(x0.shape, np.float64)
    sdd = np.zeros(x0.shape, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(x.shape[1]):
            xi = x[:, i].astype(np.float64)
            s += xi
            d = xi - x0
            sd += d
            sdd += d * d
    return s, sd, sdd


def _members_second(forecast, t, member_axis):
    x = forecast[t]
    return x if member_axis == 2 else np.moveaxis(x, 0, 1)


def _columns_host(x, y):
    """One lead.  x: float32 (S, M, *field), y: float32 (S, *field) -> float64 (e, var_0, A, B), int64 rank, bool ok, each (S, *field)"""
    m = x.shape[1]
    s, sd, sdd = _moments_host(x)
    with np.errstate(invalid='ignore', over='ignore'):
        yd = y.astype(np.float64)
        e = s / m - yd
        var0 = (sdd - sd * sd / m) / m
        a = np.zeros(yd.shape, np.float64)
        rank = np.zeros(yd.shape, np.int64)
        for i in range(m):
            a += np.abs(x[:, i].astype(np.float64) - yd)
            rank += x[:, i] < y
        a /= m
        xs = np.sort(x, axis=1)                                    # NaNs last; such a column is skipped
        coef = (2.0 * np.arange(m) - m + 1.0).reshape((1, m) + (1,) * (x.ndim - 2))
        b = np.zeros(yd.shape, np.float64)
        for k in range(m):                                         # ascending order, as the device adds them
            b += coef[:, k] * xs[:, k].astype(np.float64)
    ok = ~(np.isnan(y) | np.isnan(x).any(axis=1))
    return e, var0, a, b, rank, ok


def _scores_host(forecast, valid, member_axis, axis, want_field):
    """(sums (*keep, 6) float64, hist (*keep, M + 1) int64, crps field or None) over any `axis` of valid's axes that leaves the lead"""
    t_n, s_n, m, field = _layout(forecast, member_axis)
    ndim = valid.ndim
    if axis is None:
        red = tuple(range(1, ndim))
    else:
        red = tuple(sorted({int(a) + ndim if int(a) < 0 else int(a) for a in (axis if isinstance(axis, (tuple, list)) else (axis,))}))
        if not red or red[0] < 1 or red[-1] >= ndim:
            raise ValueError("'axis' %r must name axes 1 .. %d of 'valid' (the lead axis stays)" % (axis, ndim - 1))
    keep = tuple(a for a in range(1, ndim) if a not in red)
    keep_shape = tuple(valid.shape[a] for a in keep)
    cells = _prod(keep_shape)
    sums = np.zeros((t_n, cells, 6), np.float64)
    hist = np.zeros((t_n, cells, m + 1), np.int64)
    crps = np.full(valid.shape, np.nan, np.float32) if want_field else None
    order = tuple(a - 1 for a in keep) + tuple(a - 1 for a in red)

    def flat(v):
        return np.transpose(v, order).reshape(cells, -1)
    cell_of = np.arange(cells)[:, None]
    for t in range(t_n):
        e, var0, a, b, rank, ok = _columns_host(_members_second(forecast, t, member_axis), valid[t])
        okf = flat(ok)
        with np.errstate(invalid='ignore', over='ignore'):
            for k, v in enumerate((e * e, np.abs(e), var0, a, b)):
                sums[t, :, k] = np.where(okf, flat(v), 0.0).sum(axis=1)
            if want_field:
                crps[t] = np.where(ok, a - b / (float(m) * m), np.nan).astype(np.float32)
        sums[t, :, 5] = okf.sum(axis=1)
        index = (cell_of * (m + 1) + flat(rank))[okf]
        hist[t] = np.bincount(index, minlength=cells * (m + 1)).reshape(cells, m + 1)
    return sums.reshape((t_n,) + keep_shape + (6,)), hist.reshape((t_n,) + keep_shape + (m + 1,)), crps


def finish(sums, hist, members, ddof, crps_field=None):
    """(..., 6) float64 sums and the (..., M + 1) histogram -> EnsembleScores: divisions in float64, one cast to float32, NaN where
    nothing was counted"""
    sums = np.asarray(sums, dtype=np.float64)
    m = float(members)
    count = sums[..., 5]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        n = np.where(count > 0, count, np.nan)
        rmse = np.sqrt(sums[..., 0] / n)
        mae = sums[..., 1] / n
        var = m / (m - ddof) * (sums[..., 2] / n)
        spread = np.sqrt(np.where(var < 0, 0.0, var))
        crps = (sums[..., 3] - sums[..., 4] / (m * m)) / n
        fair = (sums[..., 3] - sums[..., 4] / (m * (m - 1.0))) / n
        vals = [v.astype(np.float32) for v in (rmse, mae, spread, spread / rmse, crps, fair)]
    return EnsembleScores(*vals, rank_hist=np.asarray(hist, dtype=np.int64), count=count.astype(np.int64), crps_field=crps_field)


# -- public ------------------------------------------------------------------------------------------------------------------------- #
def ensemble_mean_spread(forecast, member_axis=2, ddof=1, device=None):
    """Ensemble mean and spread fields.  forecast: (T, S, M, *field) with member_axis=2 or (T, M, S, *field) with member_axis=1 --
    predict_timeseries returns (T, S * M, ...) or (T, M * S, ...), and viewing it in either form is free.  Returns (mean, spread) of
    shape (T, S, *field), float32: CUDA tensors for a CUDA tensor, numpy arrays otherwise.  NaN where any member is NaN."""
    t_n, s_n, m, field = _layout(forecast, member_axis)
    _check_ddof(ddof)
    named = (('forecast', forecast),)
    if _wants_device(named, device):
        from .. import ops
        dev = _device_of(named, device)
        row = _prod(field)
        with torch.cuda.device(dev):
            x = _to_device(forecast, dev)
            mean, spread = ops.ens_mean_spread(x, ops.ens_strides(s_n, m, row, member_axis), t_n, s_n, m, row, ddof)
            mean, spread = mean.view((t_n, s_n) + field), spread.view((t_n, s_n) + field)
            if not isinstance(forecast, torch.Tensor):
                mean, spread = mean.cpu().numpy(), spread.cpu().numpy()
        return mean, spread
    forecast = np.asarray(forecast, dtype=np.float32)
    mean = np.empty((t_n, s_n) + field, np.float32)
    spread = np.empty((t_n, s_n) + field, np.float32)
    for t in range(t_n):
        s, sd, sdd = _moments_host(_members_second(forecast, t, member_axis))
        with np.errstate(invalid='ignore', over='ignore'):
            var = (sdd - sd * sd / m) / (m - ddof)
            mean[t] = (s / m).astype(np.float32)
            spread[t] = np.sqrt(np.where(var < 0, 0.0, var)).astype(np.float32)
    return mean, spread


def ensemble_scores(forecast, valid, member_axis=2, axis=None, ddof=1, crps_field=False, device=None):
    """Scores of an ensemble forecast against the per-lead verification `valid` (T, S, *field) -- what verify.verification_tensor
    leaves in HBM.  `axis` names the axes of `valid` the means run over, by forecast_error's rule: None gives one value per lead, the
    tuple that keeps the lead and the first field axis ((1, 3, 4) for a 5-D `valid`) one value per lead and variable; both run on
    the device for device operands, any other axis on the host.  Returns an EnsembleScores (module docstring): `spread` is
    sqrt(M / (M - ddof) * mean var_0), values are NaN where nothing was counted, and with crps_field=True the per-column crps comes
    back too (a CUDA tensor where `forecast` is one), NaN in skipped columns."""
    t_n, s_n, m, field = _layout(forecast, member_axis)
    _check_ddof(ddof)
    if tuple(int(s) for s in valid.shape) != (t_n, s_n) + field:
        raise ValueError('ensemble_scores: shapes %r (forecast, member_axis=%d) and %r (valid) do not match; valid must be %r'
                         % (tuple(forecast.shape), member_axis, tuple(valid.shape), (t_n, s_n) + field))
    named = (('forecast', forecast), ('valid', valid))
    if _wants_device(named, device):
        gr = _groups_run(field, axis, 1) if m <= MAX_DEVICE_MEMBERS else None
        if gr is not None:
            from .. import ops
            dev = _device_of(named, device)
            with torch.cuda.device(dev):
                x, y = _to_device(forecast, dev), _to_device(valid, dev)
                out = ops.ens_score_sums(x, ops.ens_strides(s_n, m, gr[0] * gr[1], member_axis), y, t_n, s_n, m, gr[0], gr[1],
                                         crps_field=crps_field)
                sums, hist = out[0].cpu().numpy(), out[1].cpu().numpy()
                field_out = None
                if crps_field:
                    field_out = out[2].view((t_n, s_n) + field)
                    if not isinstance(forecast, torch.Tensor):
                        field_out = field_out.cpu().numpy()
            if axis is None:
                sums, hist = sums[:, 0], hist[:, 0]
            return finish(sums, hist, m, ddof, field_out)
        forecast, valid = _to_host(forecast), _to_host(valid)
    forecast, valid = np.asarray(forecast, dtype=np.float32), np.asarray(valid, dtype=np.float32)
    sums, hist, field_out = _scores_host(forecast, valid, member_axis, axis, crps_field)
    return finish(sums, hist, m, ddof, field_out)


# -- event verification: thresholds, the host table, the finish ---------------------------------------------------------------------- #
def _check_event(event):
    if event not in ('above', 'below'):
        raise ValueError("'event' must be 'above' or 'below', got %r" % (event,))
    return event == 'below'


def _thresholds(thresholds, field):
    """(float32 thresholds, per_point): (K,) for a 1-D (or scalar) argument, else broadcast to (K, *field)"""
    thr = np.asarray(_to_host(thresholds), dtype=np.float32)
    if thr.ndim <= 1:
        thr = thr.reshape(-1)
        if thr.size < 1:
            raise ValueError("'thresholds' is empty")
        return np.ascontiguousarray(thr), False
    if thr.ndim != 1 + len(field) or thr.shape[0] < 1:
        raise ValueError("'thresholds' %r must be (K,) or broadcast to (K, *field) = (K,) + %r" % (thr.shape, tuple(field)))
    try:
        full = np.broadcast_to(thr, (thr.shape[0],) + tuple(field))
    except ValueError:
        raise ValueError("'thresholds' %r do not broadcast to (K, *field) = (%d,) + %r" % (thr.shape, thr.shape[0], tuple(field)))
    return np.array(full, dtype=np.float32), True                  # a writable copy: broadcast_to returns a read-only view


def _event_columns_host(x, thr, below):
    """One lead.  x: float32 (S, M, *field), thr: float32 broadcastable to (S, *field) -> (n int64 (S, *field), bad bool (S, *field)):
    the members that show the event, and where a member or the threshold is NaN"""
    n = np.zeros(x.shape[:1] + x.shape[2:], np.int64)
    with np.errstate(invalid='ignore'):
        for i in range(x.shape[1]):
            n += (x[:, i] < thr) if below else (x[:, i] > thr)
    return n, np.isnan(x).any(axis=1) | np.isnan(thr)


def _prob32(n, bad, members):
    return np.where(bad, np.nan, n.astype(np.float64) / float(members)).astype(np.float32)


def _events_host(forecast, valid, thr, per_point, below, member_axis, axis, want_field):
    """(table (T, *keep, K, M + 1, 2) int64, prob (K, T, S, *field) float32 or None) over any `axis` of valid's axes that leaves the lead"""
    t_n, s_n, m, field = _layout(forecast, member_axis)
    ndim = valid.ndim
    if axis is None:
        red = tuple(range(1, ndim))
    else:
        red = tuple(sorted({int(a) + ndim if int(a) < 0 else int(a) for a in (axis if isinstance(axis, (tuple, list)) else (axis,))}))
        if not red or red[0] < 1 or red[-1] >= ndim:
            raise ValueError("'axis' %r must name axes 1 .. %d of 'valid' (the lead axis stays)" % (axis, ndim - 1))
    keep = tuple(a for a in range(1, ndim) if a not in red)
    keep_shape = tuple(valid.shape[a] for a in keep)
    cells = _prod(keep_shape)
    k_n = thr.shape[0]
    order = tuple(a - 1 for a in keep) + tuple(a - 1 for a in red)
    cell_of = np.arange(cells)[:, None]
    bins = (m + 1) * 2
    table = np.zeros((t_n, cells, k_n, m + 1, 2), np.int64)
    prob = np.empty((k_n, t_n, s_n) + field, np.float32) if want_field else None
    for t in range(t_n):
        x, y = _members_second(forecast, t, member_axis), valid[t]
        for k in range(k_n):
            thr_k = thr[k][None] if per_point else thr[k]
            n, bad = _event_columns_host(x, thr_k, below)
            with np.errstate(invalid='ignore'):
                o = ((y < thr_k) if below else (y > thr_k)).astype(np.int64)
            ok = np.transpose(~(bad | np.isnan(y)), order).reshape(cells, -1)
            index = (cell_of * bins + np.transpose(n * 2 + o, order).reshape(cells, -1))[ok]
            table[t, :, k] = np.bincount(index, minlength=cells * bins).reshape(cells, m + 1, 2)
            if want_field:
                prob[k, t] = _prob32(n, bad, m)
    return table.reshape((t_n,) + keep_shape + (k_n, m + 1, 2)), prob


def finish_events64(table, members):
    """The formulas of the module docstring in float64, before the cast: a dict of float64 arrays (fcst_hist, count int64)"""
    table = np.asarray(table, dtype=np.int64)
    m = int(members)
    if m < 2 or table.ndim < 3 or table.shape[-2:] != (m + 1, 2):
        raise ValueError('finish_events: the table %r must end in (K, %d, 2) for %d >= 2 members' % (table.shape, m + 1, m))
    miss_i, o_i, n_i = table[..., 0], table[..., 1], table[..., 0] + table[..., 1]              # N_n - O_n, O_n, N_n: (..., K, M + 1)
    count = n_i.sum(axis=-1)                                                                     # (..., K)
    o_n, n_n = o_i.astype(np.float64), n_i.astype(np.float64)
    k = np.arange(m + 1, dtype=np.float64)
    p = k / m
    zero = np.zeros(table.shape[:-2] + (1,), np.int64)
    hits = np.concatenate((np.cumsum(o_i[..., ::-1], axis=-1)[..., ::-1], zero), axis=-1).astype(np.float64)       # sum_{n >= j} O_n
    falses = np.concatenate((np.cumsum(miss_i[..., ::-1], axis=-1)[..., ::-1], zero), axis=-1).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        n = np.where(count > 0, count, np.nan).astype(np.float64)
        brier = (o_n * (p - 1.0) ** 2 + (n_n - o_n) * p * p).sum(axis=-1) / n
        fair = brier - (n_n * (k * (m - k) / (float(m) * m * (m - 1.0)))).sum(axis=-1) / n
        obar = o_n.sum(axis=-1) / n
        hit = n_n > 0
        freq = np.where(hit, o_n / np.where(hit, n_n, 1.0), np.nan)
        rel = np.where(hit, n_n * (p - freq) ** 2, 0.0).sum(axis=-1) / n
        res = np.where(hit, n_n * (freq - obar[..., None]) ** 2, 0.0).sum(axis=-1) / n
        unc = obar * (1.0 - obar)
        skill = np.where(unc > 0, 1.0 - brier / np.where(unc > 0, unc, 1.0), np.nan)
        both = (hits[..., :1] > 0) & (falses[..., :1] > 0)
        hit_rate = np.where(both, hits / np.where(both, hits[..., :1], 1.0), np.nan)
        false_rate = np.where(both, falses / np.where(both, falses[..., :1], 1.0), np.nan)
        area = ((false_rate[..., :-1] - false_rate[..., 1:]) * (hit_rate[..., :-1] + hit_rate[..., 1:]) * 0.5).sum(axis=-1)
        same = (count == count[..., :1]).all(axis=-1) & (count[..., 0] > 0)
        rps = np.where(same, brier.sum(axis=-1), np.nan)
        fair_rps = np.where(same, fair.sum(axis=-1), np.nan)
    return dict(brier=brier, fair_brier=fair, reliability=rel, resolution=res, uncertainty=unc, brier_skill=skill, base_rate=obar,
                roc_area=area, rps=rps, fair_rps=fair_rps, obs_freq=freq, fcst_hist=n_i, hit_rate=hit_rate, false_alarm_rate=false_rate,
                count=count, table=table)


def finish_events(table, members, prob_field=None):
    """The int64 table (..., K, M + 1, 2) -> EventScores by the formulas of the module docstring: float64 throughout
    (finish_events64), one cast to float32, NaN where nothing was counted.  Tables of several ranks or files can be added and
    finished."""
    v = finish_events64(table, members)
    return EventScores(prob_field=prob_field, **{name: a.astype(np.float32) if a.dtype == np.float64 else a for name, a in v.items()})


def _events_device(forecast, valid, thr, per_point, below, dims, member_axis, groups, run, want_table, want_field, device):
    """dlwp_ens_event_counts on device operands: (table (T, G, K, M + 1, 2) numpy int64 or None, prob (K, T, S, *field) or None)"""
    from .. import ops
    t_n, s_n, m, field = dims
    named = (('forecast', forecast),) + ((('valid', valid),) if want_table else ())
    dev = _device_of(named, device)
    with torch.cuda.device(dev):
        x = _to_device(forecast, dev)
        y = _to_device(valid, dev) if want_table else None
        thr_d = torch.from_numpy(thr if per_point else np.ascontiguousarray(np.repeat(thr[:, None], groups, axis=1))).to(dev)
        table, prob = ops.ens_event_counts(x, ops.ens_strides(s_n, m, groups * run, member_axis), y, thr_d, per_point, below, t_n, s_n, m,
                                           groups, run, want_table=want_table, want_prob=want_field)
        table = table.cpu().numpy() if want_table else None
        if want_field:
            prob = prob.view((thr.shape[0], t_n, s_n) + field)
            if not isinstance(forecast, torch.Tensor):
                prob = prob.cpu().numpy()
    return table, prob


def event_scores(forecast, valid, thresholds, member_axis=2, axis=None, event='above', prob_field=False, device=None):
    """Event scores of an ensemble forecast against the per-lead verification `valid` (T, S, *field), for the events "above" (or
    "below") each of K thresholds: (K,) values for every point, or anything that broadcasts to (K, *field).  Shapes, the device-or-
    host decision and `axis` are those of ensemble_scores.  Returns an EventScores (module docstring); with prob_field=True the
    probability field (K, T, S, *field) comes back too (a CUDA tensor where `forecast` is one).  Only the integer table comes back
    from the device, and finish_events is shared: both paths return identical bits."""
    t_n, s_n, m, field = _layout(forecast, member_axis)
    below = _check_event(event)
    if tuple(int(s) for s in valid.shape) != (t_n, s_n) + field:
        raise ValueError('event_scores: shapes %r (forecast, member_axis=%d) and %r (valid) do not match; valid must be %r'
                         % (tuple(forecast.shape), member_axis, tuple(valid.shape), (t_n, s_n) + field))
    thr, per_point = _thresholds(thresholds, field)
    named = (('forecast', forecast), ('valid', valid))
    if _wants_device(named, device):
        gr = _groups_run(field, axis, 1) if m <= MAX_DEVICE_MEMBERS else None
        if gr is not None:
            if thr.shape[0] > MAX_DEVICE_THRESHOLDS:
                raise ValueError('event_scores: %d thresholds, the device path takes 1 .. %d' % (thr.shape[0], MAX_DEVICE_THRESHOLDS))
            table, prob = _events_device(forecast, valid, thr, per_point, below, (t_n, s_n, m, field), member_axis, gr[0], gr[1], True,
                                         prob_field, device)
            return finish_events(table[:, 0] if axis is None else table, m, prob)
        forecast, valid = _to_host(forecast), _to_host(valid)
    forecast, valid = np.asarray(forecast, dtype=np.float32), np.asarray(valid, dtype=np.float32)
    table, prob = _events_host(forecast, valid, thr, per_point, below, member_axis, axis, prob_field)
    return finish_events(table, m, prob)


def ensemble_exceedance(forecast, thresholds, member_axis=2, event='above', device=None):
    """The fraction of members above (or below) each threshold: float32 (K, T, S, *field) = float32(n / M), NaN where a member or the
    threshold is NaN -- a CUDA tensor for a CUDA tensor, else a numpy array.  thresholds: as in event_scores."""
    t_n, s_n, m, field = _layout(forecast, member_axis)
    below = _check_event(event)
    thr, per_point = _thresholds(thresholds, field)
    named = (('forecast', forecast),)
    if _wants_device(named, device):
        if m <= MAX_DEVICE_MEMBERS:
            if thr.shape[0] > MAX_DEVICE_THRESHOLDS:
                raise ValueError('ensemble_exceedance: %d thresholds, the device path takes 1 .. %d' % (thr.shape[0], MAX_DEVICE_THRESHOLDS))
            return _events_device(forecast, None, thr, per_point, below, (t_n, s_n, m, field), member_axis, 1, _prod(field), False, True,
                                  device)[1]
        forecast = _to_host(forecast)
    forecast = np.asarray(forecast, dtype=np.float32)
    prob = np.empty((thr.shape[0], t_n, s_n) + field, np.float32)
    for t in range(t_n):
        x = _members_second(forecast, t, member_axis)
        for k in range(thr.shape[0]):
            prob[k, t] = _prob32(*_event_columns_host(x, thr[k][None] if per_point else thr[k], below), m)
    return prob


# -- the member generator: the numpy statement of the definition (module docstring) ------------------------------------------------ #
_M32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al., SC'11).  counter: four integer arrays that broadcast together (32-bit values), key: two 32-bit
    integers.  Returns four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M32 for c in counter])
    k0, k1 = np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                            # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def pair_uniforms(wa, wb):
    """(u1, u2) of a word pair, float64: u1 = (2 (wa >> 9) + 1) 2^-24 in (0, 1), u2 = (wb >> 8) 2^-24 in [0, 1); both are float32 values"""
    wa, wb = np.asarray(wa, dtype=np.uint32), np.asarray(wb, dtype=np.uint32)
    return (2.0 * (wa >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24, (wb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def white_noise(seed, draw, sample, channel, rows, width):
    """z(draw, sample, channel, i, j) for the virtual rows `rows` (integers, |i| < 32768) and j < width, evaluated in float64:
    (len(rows), width).  The definition's z is this rounded to float32."""
    seed = int(seed) & 0xffffffffffffffff
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    quads = (int(width) + 3) // 4
    w = philox4x32_10((np.arange(quads, dtype=np.int64)[None, :], (rows + 32768 + 65536 * int(channel))[:, None], int(draw), int(sample)),
                      (seed & 0xffffffff, seed >> 32))
    z = np.empty((rows.size, quads, 4), np.float64)
    for e, (wa, wb) in enumerate(((w[0], w[1]), (w[2], w[3]))):
        u1, u2 = pair_uniforms(wa, wb)
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, :, 2 * e] = r * np.cos(2.0 * np.pi * u2)
        z[:, :, 2 * e + 1] = r * np.sin(2.0 * np.pi * u2)
    return z.reshape(rows.size, 4 * quads)[:, :int(width)]


def smoothing_taps(length):
    """(R, float32 taps g_a for a = -R .. R) of one axis: R = ceil(3 L), g_a proportional to exp(-a^2 / 2 L^2), normalised in float64 to
    sum g^2 = 1, then rounded to float32; L = 0 gives R = 0 and g = [1]"""
    length = float(length)
    if not length >= 0.0:
        raise ValueError("'length' must be >= 0, got %r" % (length,))
    radius = int(np.ceil(3.0 * length))
    if radius > MAX_RADIUS:
        raise ValueError("'length' %r needs a radius of %d grid points, at most %d" % (length, radius, MAX_RADIUS))
    if radius == 0:
        return 0, np.ones(1, np.float32)
    a = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-a * a / (2.0 * length * length))
    return radius, (g / np.sqrt((g * g).sum())).astype(np.float32)


def _smooth_host(seed, draw, sample, channel, height, width, taps_y, taps_x):
    """zeta of one (draw, sample, channel): float32 (height, width)"""
    ry, rx = taps_y.size // 2, taps_x.size // 2
    z = white_noise(seed, draw, sample, channel, np.arange(-ry, height + ry), width).astype(np.float32)
    rowp = np.zeros(z.shape, np.float32)
    for b in range(-rx, rx + 1):                                   # ascending taps; float32 product, float32 sum
        rowp = rowp + taps_x[b + rx] * np.roll(z, -b, axis=1)
    zeta = np.zeros((height, width), np.float32)
    for a in range(-ry, ry + 1):
        zeta = zeta + taps_y[a + ry] * rowp[ry + a:ry + a + height]
    return zeta


def _draw_of(g, control, antithetic):
    """global member -> (draw, sign), or None for the control member"""
    if control and g == 0:
        return None
    p = g - 1 if control else g
    return (p >> 1, -1.0 if p & 1 else 1.0) if antithetic else (p, 1.0)


def _perturb_args(predictors, members, stddev, length, seed, member_axis, first_member):
    shape = tuple(int(s) for s in predictors.shape)
    if len(shape) < 2 or _prod(shape) < 1:
        raise ValueError("'predictors' must be (samples, ..., height, width) or (samples, features) without an empty axis, got %r" % (shape,))
    s_n = shape[0]
    k_n, h_n, w_n = (1, 1, shape[1]) if len(shape) == 2 else (_prod(shape[1:-2]), shape[-2], shape[-1])
    members, first_member = int(members), int(first_member)
    if members < 1:
        raise ValueError("'members' must be >= 1, got %d" % members)
    if first_member < 0 or first_member + members >= 2 ** 31:
        raise ValueError("'first_member' must be >= 0 and first_member + members < 2^31, got %d" % first_member)
    if member_axis not in (1, 2):
        raise ValueError("'member_axis' must be 1 or 2, got %r" % (member_axis,))
    sigma = np.asarray(stddev, dtype=np.float32).reshape(-1)
    if sigma.size == 1:
        sigma = np.repeat(sigma, k_n)
    if sigma.size != k_n:
        raise ValueError("'stddev' holds %d values for %d channels (a scalar broadcasts)" % (sigma.size, k_n))
    ly, lx = (length, length) if np.ndim(length) == 0 else tuple(length)
    (ry, taps_y), (rx, taps_x) = smoothing_taps(ly), smoothing_taps(lx)
    if rx > w_n:
        raise ValueError("'length' %r needs %d columns on either side of a row of %d: more than one wrap" % (lx, rx, w_n))
    if k_n >= 65536 or h_n + ry >= 32768:
        raise ValueError('%d channels (at most 65535) or %d + %d rows (below 32768) do not fit the counter' % (k_n, h_n, ry))
    return shape, (s_n, k_n, h_n, w_n), members, first_member, np.ascontiguousarray(sigma), taps_y, taps_x, int(seed) & 0xffffffffffffffff


def _perturb_host(x, dims, members, first_member, sigma, taps_y, taps_x, seed, control, antithetic):
    """float32 (S, M, K, H, W)"""
    s_n, k_n, h_n, w_n = dims
    x = x.reshape(dims)
    out = np.empty((s_n, members, k_n, h_n, w_n), np.float32)
    cache = {}
    for m in range(members):
        ds = _draw_of(first_member + m, control, antithetic)
        if ds is None:
            out[:, m] = x
            continue
        for s in range(s_n):
            for k in range(k_n):
                key = (ds[0], s, k)
                if key not in cache:                               # the partner of an antithetic pair follows at once
                    cache.clear()
                    cache[key] = _smooth_host(seed, ds[0], s, k, h_n, w_n, taps_y, taps_x)
                with np.errstate(invalid='ignore', over='ignore'):
                    out[s, m, k] = x[s, k] + np.float32(ds[1]) * (sigma[k] * cache[key])
    return out


def perturb_members(predictors, members, stddev=1.0, length=0.0, seed=0, member_axis=2, control=True, antithetic=False,
                    first_member=0, device=None):
    """A perturbed-initial-condition ensemble of `predictors` (S, ..., H, W) -- every axis between the first and the last two counts
    as a channel -- or (S, F) (one channel, one row): `members` copies of every sample, each plus stddev * (spatially correlated,
    longitude-periodic Gaussian noise of unit variance), by the definition of the module docstring.  stddev: a scalar or one value
    per channel; length: the correlation length in grid points, a scalar or (L_y, L_x), 0 for white noise; control: member 0 is the
    unperturbed state; antithetic: members come in +/- pairs; first_member: the global index of this call's first member, so that
    an ensemble can be extended or cut across ranks with the same bits.  Returns the batch predict_timeseries takes, float32:
    (S * M, ...) with members fastest (member_axis=2) or (M * S, ...) with samples fastest (member_axis=1) -- a CUDA tensor for a CUDA
    tensor or device='cuda' (made by dlwp_ens_perturb), else a numpy array (made by the numpy code above)."""
    shape, dims, members, first_member, sigma, taps_y, taps_x, seed = _perturb_args(predictors, members, stddev, length, seed, member_axis,
                                                                                 first_member)
    s_n = dims[0]
    flat = (s_n * members,) + shape[1:]
    named = (('predictors', predictors),)
    if _wants_device(named, device):
        from .. import ops
        dev = _device_of(named, device)
        with torch.cuda.device(dev):
            x = _to_device(predictors, dev).view(dims)
            out = ops.ens_perturb(x, torch.from_numpy(sigma).to(dev), members, first_member, seed, taps_y, taps_x, control, antithetic,
                                  member_axis)
        return out.view(flat)
    x = np.ascontiguousarray(predictors, dtype=np.float32)
    out = _perturb_host(x, dims, members, first_member, sigma, taps_y, taps_x, seed, bool(control), bool(antithetic))
    if member_axis == 1:
        out = np.ascontiguousarray(np.moveaxis(out, 1, 0))
    return out.reshape(flat)


def ensemble_forecast(wrapper, predictors, time_steps, members, stddev=1.0, length=0.0, seed=0, member_axis=2, control=True,
                      antithetic=False, first_member=0, keep_time_dim=False, device=None):
    """Generate -> roll out, without a host array: perturb_members on the device, then wrapper.predict_timeseries(x, time_steps,
    return_device=True) on the S * M rows.  Returns the series as a CUDA tensor viewed as (T, S, M, ...) (member_axis=2) or
    (T, M, S, ...) (member_axis=1): what ensemble_mean_spread and ensemble_scores take."""
    s_n = int(predictors.shape[0])
    x = perturb_members(predictors, members, stddev, length, seed, member_axis, control, antithetic, first_member,
                        device=device if (device is not None or isinstance(predictors, torch.Tensor)) else 'cuda')
    series = wrapper.predict_timeseries(x, time_steps, keep_time_dim=keep_time_dim, return_device=True)
    lead = (s_n, int(members)) if member_axis == 2 else (int(members), s_n)
    return series.view((int(series.shape[0]),) + lead + tuple(series.shape[2:]))
