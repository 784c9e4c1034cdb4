"""Shared by tests/test_ensemble_cpu.py and tests/test_gpu_ensemble.py: an independent float64 restatement of the definitions of
dlwp_amd/model/ensemble.py, and the bound both paths are held to.

The restatement is brute force on purpose: np.mean / np.var for the moments, the O(M^2) pairwise definition of B (not the sorted
identity the module and the kernel use) and (x < y).sum for the ranks.

Bound (derived).  Both sides work in float64 on the same float32 inputs and differ in the order of their sums; the
result is then rounded once to float32.  With u = 2^-53, M <= 256 members and n <= 2^10 columns per cell in these tests:
  * the cast: 2^-24 |value|; taken as 2^-23 |want|.
  * sums of M terms then n columns differ by at most (M + n) u ~ 2^-43 of the magnitudes that enter them.  Those are not the result
    where terms cancel:  mean - y cancels numbers of size X = max(max_i |x_i|, |y|);  A - B / M^2 cancels A against B / M^2, and the
    sorted identity B = sum_k (2k - M + 1) x_(k) adds terms of size M X whose absolute values sum to M^2 X / 2, an error of
    (M / 2) u X = 2^-46 X in B / M^2;  the shifted variance cancels sum d^2 / M against (sum d)^2 / M^2, both at most
    D2 = (1 / M) sum_i (x_i - x_0)^2, and np.var's own mean is off by M u X.
    Through the square roots (d sqrt(v) = dv / (2 sqrt(v)), Cauchy-Schwarz for the mean of |e| X) this gives allowances of
      2^-40 * sqrt(mean X^2)                                  for rmse_mean,
      2^-40 * mean X                                          for mae_mean,
      2^-40 * (sqrt(mean X^2) + mean D2 / spread)             for spread (the second term only where spread > 0),
      2^-40 * (mean A + mean B / M^2 + mean X)                for crps and fair_crps (B / (M (M - 1)) there),
    and the same per column for the crps and spread fields: 2^-40 leaves a factor of eight over (M + n) u.
The bound uses no output of the code under test.  rank_hist and count are integers and must be equal."""
import numpy as np

CAST = 2.0 ** -23
ORDER = 2.0 ** -40


def columns64(x, y):
    """x: float32 (T, S, M, *field), y: float32 (T, S, *field) or None -> dict of float64 per-column arrays (T, S, *field)"""
    xd = x.astype(np.float64)
    m = x.shape[2]
    out = {}
    with np.errstate(invalid='ignore', over='ignore'):
        out['mean'] = np.mean(xd, axis=2)
        out['var0'] = np.var(xd, axis=2)
        out['d2'] = np.mean((xd - xd[:, :, :1]) ** 2, axis=2)
        out['xmax'] = np.max(np.abs(xd), axis=2)
        b = np.zeros(out['mean'].shape)
        for i in range(m - 1):                                   # every pair once: O(M^2)
            b = b + np.abs(xd[:, :, i + 1:] - xd[:, :, i:i + 1]).sum(axis=2)
        out['B'] = b
        if y is not None:
            yd = y.astype(np.float64)
            out['e'] = out['mean'] - yd
            out['A'] = np.abs(xd - yd[:, :, None]).mean(axis=2)
            out['rank'] = (x < y[:, :, None]).sum(axis=2)
            out['ok'] = ~(np.isnan(y) | np.isnan(x).any(axis=2))
            out['X'] = np.maximum(out['xmax'], np.abs(yd))
            out['crps'] = out['A'] - out['B'] / (m * m)
    return out


def member_order_mean32(x):
    """float32(float64 sum in member order / M): the bits ensemble_mean_spread must return"""
    s = np.zeros(x.shape[:2] + x.shape[3:], np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(x.shape[2]):
            s = s + x[:, :, i].astype(np.float64)
        return (s / x.shape[2]).astype(np.float32)


def scores64(x, y, grouped, ddof=1, c=None):
    """The scores in float64 and their allowances: {name: (want, allowance)}, plus 'rank_hist' and 'count' (int64).  Cells are (T,) or,
    grouped, (T, field[0]); means run over the counted columns of a cell.  c: columns64(x, y), if the caller has it already."""
    c = columns64(x, y) if c is None else c
    t_n, m = x.shape[0], x.shape[2]
    groups = x.shape[3] if grouped else 1

    def cells(v):            # (T, S, *field) -> (T, G, columns)
        v = v.reshape((t_n, x.shape[1], groups, -1))
        return np.moveaxis(v, 2, 1).reshape(t_n, groups, -1)
    ok = cells(c['ok'])
    count = ok.sum(axis=2)

    def mean(v):
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            return np.where(ok, cells(v), 0.0).sum(axis=2) / np.where(count > 0, count, np.nan)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        x1, x2 = mean(c['X']), np.sqrt(mean(c['X'] ** 2))
        a, b = mean(c['A']), mean(c['B'])
        spread = np.sqrt(m / (m - ddof) * mean(c['var0']))
        out = {
            'rmse_mean': (np.sqrt(mean(c['e'] ** 2)), ORDER * x2),
            'mae_mean': (mean(np.abs(c['e'])), ORDER * x1),
            'spread': (spread, ORDER * (x2 + np.where(spread > 0, mean(c['d2']) / np.where(spread > 0, spread, 1.0), 0.0))),
            'crps': (a - b / (m * m), ORDER * (a + b / (m * m) + x1)),
            'fair_crps': (a - b / (m * (m - 1.0)), ORDER * (a + b / (m * (m - 1.0)) + x1)),
        }
    rank = cells(c['rank'])
    hist = np.zeros((t_n, groups, m + 1), np.int64)
    for t in range(t_n):
        for g in range(groups):
            hist[t, g] = np.bincount(rank[t, g][ok[t, g]], minlength=m + 1)
    if not grouped:
        out = {k: (v[0][:, 0], v[1][:, 0]) for k, v in out.items()}
        hist, count = hist[:, 0], count[:, 0]
    out['rank_hist'], out['count'] = hist, count.astype(np.int64)
    out['crps_field'] = (np.where(c['ok'], c['crps'], np.nan), ORDER * (c['A'] + c['B'] / (m * m) + c['X']))
    return out


def spread_field64(x, ddof=1):
    """(want, allowance) of the spread field, float64 (T, S, *field)"""
    c = columns64(x, None)
    m = x.shape[2]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        spread = np.sqrt(m / (m - ddof) * c['var0'])
        return spread, ORDER * (c['xmax'] + np.where(spread > 0, c['d2'] / np.where(spread > 0, spread, 1.0), 0.0))


def within(got, want, allowance, what):
    """got: float32; want, allowance: float64.  NaN exactly where want is NaN, else |got - want| <= 2^-23 |want| + allowance.  Prints
    error / bound (pytest -s)."""
    got = np.asarray(got)
    want, allowance = np.asarray(want, np.float64), np.asarray(allowance, np.float64)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    bound = CAST * np.abs(want[ok]) + np.nan_to_num(allowance[ok])
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print('%s: error / bound %.3f over %d values' % (what, float(ratio.max()) if ratio.size else 0.0, ratio.size))
    assert (err <= bound).all(), (what, float(ratio.max()))


def check_scores(res, want, what, field=None):
    """res: EnsembleScores; want: scores64(...).  field: the downloaded crps field, if asked for"""
    assert res.rank_hist.dtype == np.int64 and np.array_equal(res.rank_hist, want['rank_hist']), what
    assert res.count.dtype == np.int64 and np.array_equal(res.count, want['count']), what
    for name in ('rmse_mean', 'mae_mean', 'spread', 'crps', 'fair_crps'):
        within(getattr(res, name), want[name][0], want[name][1], '%s %s' % (what, name))
    if field is not None:
        within(field, want['crps_field'][0], want['crps_field'][1], what + ' crps_field')


def ensemble(shape, seed, spread=0.01, nan_every=0):
    """float32 (T, S, M, *field): a base state per column + spread * noise per member, so that shifted sums are what is exercised"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(shape[:2] + (1,) + shape[3:]) * 3.0 + 1.0
    x = (base + spread * rng.standard_normal(shape)).astype(np.float32)
    if nan_every:
        x.ravel()[seed % nan_every::nan_every] = np.nan
    return x


def verification(x, seed, spread=0.01, nan_every=0):
    """float32 (T, S, *field) near the ensemble: the column's first member + spread * noise"""
    rng = np.random.default_rng(seed)
    y = (x[:, :, 0].astype(np.float64) + spread * rng.standard_normal(x[:, :, 0].shape)).astype(np.float32)
    if nan_every:
        y.ravel()[seed % nan_every::nan_every] = np.nan
    return y
