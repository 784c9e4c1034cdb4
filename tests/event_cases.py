"""Shared by tests/test_events_cpu.py and tests/test_gpu_events.py: an independent brute-force float64 restatement of the event
definitions of dlwp_amd/model/ensemble.py, the inputs, and what a case must exercise.

The restatement is not table-based: per column p = (x > thr).mean(axis=members), o = (y > thr) and (p - o)^2, then plain means over
the counted columns of a cell; the ROC area is the Mann-Whitney statistic over all (event, non-event) column pairs,
P(n_e > n_ne) + P(n_e = n_ne) / 2.  The table itself is a bincount over (n, o) and must be EQUAL to the code's; the probability
field is float32(n / M) and must be bit-equal.

Allowance for the derived values (the budget and the argument of tests/ensemble_cases.py): both sides work in float64 on integers
and on terms in [0, 1], over N <= 2^10 columns per cell, and differ in the order of their sums -- 2^-40 covers (N + M) 2^-53 with a
factor of eight to spare -- and the result is rounded once to float32: 2^-23 |want|.  It uses no output of the code under test."""
import numpy as np

from tests.ensemble_cases import CAST, ORDER, ensemble, verification

MEMBER_NAN_EVERY = 1009
VALID_NAN_EVERY = 89


def inputs(shape, seed, spread=1.0):
    """(x float32 (T, S, M, *field), y float32 (T, S, *field)) with NaNs in both: spread=1.0 fills the interior bins, spread=0.01 puts
    nearly every column in n = 0 or n = M"""
    x = ensemble(shape, seed, spread=spread, nan_every=MEMBER_NAN_EVERY)
    return x, verification(x, seed + 1, spread=spread, nan_every=VALID_NAN_EVERY)


def thresholds(k_n):
    """K ascending float32 thresholds inside the climate of `ensemble` (mean 1, deviation 3); K = 3 is (-1, 1, 3)"""
    return {1: np.array([1.0], np.float32), 3: np.array([-1.0, 1.0, 3.0], np.float32)}.get(
        k_n, np.linspace(-3.0, 4.0, k_n).astype(np.float32))


def per_variable(k_n, field):
    """(K, V, 1, 1): the scalar thresholds shifted per variable"""
    shift = 0.25 * np.arange(field[0], dtype=np.float32).reshape((1, field[0]) + (1,) * (len(field) - 1))
    return thresholds(k_n).reshape((k_n,) + (1,) * len(field)) + shift


def per_point(k_n, field, seed):
    """(K, *field): the scalar thresholds plus a field of small offsets, ascending in k at every point"""
    rng = np.random.default_rng(seed)
    return (thresholds(k_n).reshape((k_n,) + (1,) * len(field)) + 0.2 * rng.standard_normal((1,) + tuple(field))).astype(np.float32)


def full_thresholds(thr, field):
    thr = np.asarray(thr, np.float32)
    if thr.ndim == 1:
        thr = thr.reshape((-1,) + (1,) * len(field))
    return np.broadcast_to(thr, (thr.shape[0],) + tuple(field))


def events64(x, y, thr, below, grouped, derived=True):
    """x: float32 (T, S, M, *field), y: float32 (T, S, *field), thr: (K,) or anything that broadcasts to (K, *field).  Cells are (T,) or,
    grouped, (T, field[0]).  Returns a dict: 'table' int64 (T[, G], K, M + 1, 2), 'count' int64 (T[, G], K), 'prob' float32 (K, T, S,
    *field), and float64 'brier', 'base_rate', 'roc_area' (T[, G], K) and 'rps' (T[, G]) -- NaN with derived=False, for callers that
    compare the table and the field only (the Mann-Whitney statistic is quadratic in a cell's columns)."""
    t_n, s_n, m = x.shape[:3]
    field = x.shape[3:]
    groups = field[0] if grouped else 1
    full = full_thresholds(thr, field)
    k_n = full.shape[0]

    def cells(v):            # (T, S, *field) -> (T, G, columns)
        return np.moveaxis(v.reshape((t_n, s_n, groups, -1)), 2, 1).reshape(t_n, groups, -1)
    table = np.zeros((t_n, groups, k_n, m + 1, 2), np.int64)
    prob = np.empty((k_n, t_n, s_n) + field, np.float32)
    brier = np.full((t_n, groups, k_n), np.nan)
    base = np.full((t_n, groups, k_n), np.nan)
    area = np.full((t_n, groups, k_n), np.nan)
    member_nan = np.isnan(x).any(axis=2)
    for k in range(k_n):
        t_k = full[k][None, None]
        with np.errstate(invalid='ignore'):
            ev = (x < t_k[:, :, None]) if below else (x > t_k[:, :, None])
            o = ((y < t_k) if below else (y > t_k)).astype(np.float64)
        p = ev.mean(axis=2, dtype=np.float64)
        n = ev.sum(axis=2)
        bad = member_nan | np.isnan(t_k)
        prob[k] = np.where(bad, np.nan, p).astype(np.float32)
        ok_c, p_c, o_c, n_c = cells(~(bad | np.isnan(y))), cells(p), cells(o), cells(n)
        for t in range(t_n):
            for g in range(groups):
                ok = ok_c[t, g]
                pp, oo, nn = p_c[t, g][ok], o_c[t, g][ok], n_c[t, g][ok]
                table[t, g, k] = np.bincount(nn * 2 + oo.astype(np.int64), minlength=2 * (m + 1)).reshape(m + 1, 2)
                if pp.size and derived:
                    brier[t, g, k] = np.mean((pp - oo) ** 2)
                    base[t, g, k] = np.mean(oo)
                    n_e, n_ne = nn[oo == 1], nn[oo == 0]
                    if n_e.size and n_ne.size:
                        d = n_e[:, None] - n_ne[None, :]
                        area[t, g, k] = ((d > 0).sum() + 0.5 * (d == 0).sum()) / float(d.size)
    count = table.sum(axis=(-1, -2))
    same = (count == count[..., :1]).all(axis=-1) & (count[..., 0] > 0)
    out = {'table': table, 'count': count, 'brier': brier, 'base_rate': base, 'roc_area': area,
           'rps': np.where(same, brier.sum(axis=-1), np.nan)}
    if not grouped:
        out = {name: v[:, 0] for name, v in out.items()}
    out['prob'] = prob
    return out


def check_case(want, columns, wide):
    """What a case must exercise, asserted on the RESTATEMENT's table (a case that fails here is a bad case, not a pass): for every
    threshold more than half of the `columns` are counted and at least one is skipped, both outcomes occur, and with a wide ensemble
    at least one interior bin 0 < n < M is hit."""
    table = want['table']
    k_n = table.shape[-3]
    per_k = table.reshape((-1, k_n) + table.shape[-2:]).sum(axis=0)          # (K, M + 1, 2)
    for k in range(k_n):
        counted = int(per_k[k].sum())
        assert columns // 2 < counted < columns, (k, counted, columns)
        assert per_k[k, :, 0].sum() > 0 and per_k[k, :, 1].sum() > 0, (k, per_k[k].sum(axis=0))
    if wide:
        assert per_k[:, 1:-1].sum() > 0


def within(got, want, what):
    """got: float32; want: float64.  NaN exactly where want is NaN, else |got - want| <= 2^-23 |want| + 2^-40"""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    bound = CAST * np.abs(want[ok]) + ORDER
    print('%s: error / bound %.3f over %d values' % (what, float((err / bound).max()) if err.size else 0.0, err.size))
    assert (err <= bound).all(), (what, float((err / bound).max()))


def same_bits(a, b):
    """equal float32 arrays bit for bit, NaN payloads aside (NaN exactly where the other has one)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def check_scores(res, want, what):
    """res: EventScores; want: events64(...): the table and the count are equal, the derived values within the allowance, and the
    identities that hold for any table"""
    assert res.table.dtype == np.int64 and np.array_equal(res.table, want['table']), what
    assert res.count.dtype == np.int64 and np.array_equal(res.count, want['count']), what
    assert res.fcst_hist.dtype == np.int64 and np.array_equal(res.fcst_hist, want['table'].sum(axis=-1)), what
    for name in ('brier', 'base_rate', 'roc_area', 'rps'):
        within(getattr(res, name), want[name], '%s %s' % (what, name))
    counted = want['count'] > 0
    assert (res.fair_brier[counted] <= res.brier[counted]).all(), what
    m = res.table.shape[-2] - 1
    assert res.hit_rate.shape == res.false_alarm_rate.shape == res.table.shape[:-2] + (m + 2,), what
    for curve in (res.hit_rate, res.false_alarm_rate):
        c = curve[~np.isnan(curve).any(axis=-1)]
        assert (c[:, 0] == 1).all() and (c[:, -1] == 0).all() and (np.diff(c, axis=-1) <= 0).all(), what

