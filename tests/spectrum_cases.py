"""Shared by tests/test_spectrum_cpu.py and tests/test_gpu_spectrum.py: the float64 restatement of forecast_spectrum /
persistence_spectrum, the inputs, and the derived bounds of DESIGN.md 5.41.

Restatement (independent of verify.py's host path: plain loops over leads and groups, np.fft.rfft of each longitude row in float64):
d = fc - ob rounded once in float32; a longitude row with a non-finite fc, ob or d is skipped; O = rfft(ob), D = rfft(d); the four
weighted sums of the issue's table with the one-sided Parseval factors c_k / W^2, sum w and the rows counted.

Bounds, from reference quantities only.  u = 2^-24.  The device computes X_k (k >= 1) of a row x as a float32 chain over the folded
row: y_j = fl(x_j - m) (one rounding), e_j / o_j = fl(y_j +- y_{W-j}) (one), a twiddle rounded once from float64 (one), and a chain of
n fused multiply-adds (n roundings of partial sums that never exceed sum |y_j|, to first order), n = K = W // 2 + 1 <=
floor((W - 1) / 2) + 2 products (the step that pads K to an even number multiplies exact zeros and adds nothing).  m is the float64
mean rounded once: it is off by at most u |mean|, a constant shift of every y_j, bounded here by W u |mean| in the sum.  So
  delta_x = (n + 4) u (sum_j |x_j - mean| + W u |mean|)          and  |X^_k - X_k| <= delta_x  for k >= 1;
  k = 0 is the float64 row sum itself: delta = 2^-45 sum_j |x_j| (a tree of depth <= W / 8 + 3 at 2^-53 each).
  entry 0:  sum w c_k (2 |O_k| delta_o + delta_o^2);   entry 1: the same with D, delta_d;
  entries 2, 3:  sum w c_k (|D_k| delta_o + |O_k| delta_d + delta_o delta_d);
  each plus 2^-40 sum |terms| for the float64 sums (thousands of additions at 2^-53).
For white and offset inputs the bounds are far below the coefficients; for the red input (amplitudes ~ k^-3) at W >= 180 the
worst-case bound exceeds the smallest coefficients: there the tests show that the error stays inside the bound, not that the tail is
resolved (check_sums prints the share of entries whose bound is below a tenth of the value)."""
import collections
import functools

import numpy as np

from dlwp_amd.model import verify

U = 2.0 ** -24

Ref = collections.namedtuple('Ref', 'sums norm bounds')


# -- inputs -------------------------------------------------------------------------------------------------------------------------- #
def data(shape, seed):
    """the 3 N(0, 1) + 1 generator of tests/skill_cases.py"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 3.0 + 1.0).astype(np.float32)


def red(shape, seed):
    """rows whose zonal amplitudes fall as k^-3 (k >= 1), a mean of order one: irfft of random phases"""
    rng = np.random.default_rng(seed)
    w = shape[-1]
    k = np.arange(w // 2 + 1, dtype=np.float64)
    amp = np.where(k > 0, np.maximum(k, 1.0) ** -3.0, 1.0)
    spec = (rng.standard_normal(shape[:-1] + (k.size,)) + 1j * rng.standard_normal(shape[:-1] + (k.size,))) * amp
    return (np.fft.irfft(spec, n=w, axis=-1) * w).astype(np.float32)


def offset(shape, seed):
    """unscaled geopotential height: N(0, 1) + 5.5e4"""
    return (np.random.default_rng(seed).standard_normal(shape) + 5.5e4).astype(np.float32)


def plant(x, rows, value):
    """x with `value` planted at one longitude of each of the rows given as index tuples of x.shape[:-1]"""
    x = x.copy()
    for n, at in enumerate(rows):
        x[tuple(at) + ((3 * n + 1) % x.shape[-1],)] = value
    return x


def cosine(h):
    return verify.area_weights(np.linspace(-90.0, 90.0, h))


def parseval(width):
    k = width // 2 + 1
    c = np.full(k, 2.0)
    c[0] = 1.0
    if width % 2 == 0:
        c[-1] = 1.0
    return c / (float(width) * float(width))


# -- the restatement and its bounds ------------------------------------------------------------------------------------------------- #
def _row_delta(x64, n):
    """delta_x of every row of x64 (..., W): (n + 4) u (sum |x - mean| + W u |mean|); and the k = 0 delta"""
    w = x64.shape[-1]
    mean = x64.mean(axis=-1, keepdims=True)
    return (n + 4) * U * (np.abs(x64 - mean).sum(axis=-1) + w * U * np.abs(mean[..., 0])), 2.0 ** -45 * np.abs(x64).sum(axis=-1)


def sums64(fc_rows, ob_rows, leads, count, weights, grouped, inner):
    """Ref of (leads, groups, 4, K) sums, (leads, groups, 2) norm and the bounds of the sums; *_rows(f, cnt) give the rows lead f
    pairs, count(f) their number"""
    inner = tuple(inner)
    width, lat = inner[-1], inner[-2]
    k = width // 2 + 1
    groups = inner[0] if grouped else 1
    c = parseval(width)
    w_lat = np.ones(lat) if weights is None else np.asarray(weights, np.float64)
    sums, norm, bounds = np.zeros((leads, groups, 4, k)), np.zeros((leads, groups, 2)), np.zeros((leads, groups, 4, k))
    for f in range(leads):
        cnt = count(f)
        if cnt <= 0:
            continue
        fc = fc_rows(f, cnt).reshape(cnt, groups, -1, lat, width)
        ob = ob_rows(f, cnt).reshape(cnt, groups, -1, lat, width)
        with np.errstate(invalid='ignore', over='ignore'):
            d = fc - ob
        assert d.dtype == np.float32
        for g in range(groups):
            # the longitude rows of the cell, one per line; their latitude index runs fastest
            fcr, obr, dr = (v[:, g].reshape(-1, width) for v in (fc, ob, d))
            w = np.tile(w_lat, fcr.shape[0] // lat)
            ok = np.isfinite(fcr).all(axis=-1) & np.isfinite(obr).all(axis=-1) & np.isfinite(dr).all(axis=-1)
            o64, d64 = obr[ok].astype(np.float64), dr[ok].astype(np.float64)
            wk = w[ok][:, None] * c
            o_k, d_k = np.fft.rfft(o64, axis=-1), np.fft.rfft(d64, axis=-1)
            cross = d_k * np.conj(o_k)
            terms = (np.abs(o_k) ** 2, np.abs(d_k) ** 2, cross.real, cross.imag)
            do, do0 = _row_delta(o64, k)
            dd, dd0 = _row_delta(d64, k)
            do, dd = np.repeat(do[:, None], k, axis=1), np.repeat(dd[:, None], k, axis=1)
            do[:, 0], dd[:, 0] = do0, dd0
            ao, ad = np.abs(o_k), np.abs(d_k)
            cross_b = ad * do + ao * dd + do * dd
            errs = (2 * ao * do + do * do, 2 * ad * dd + dd * dd, cross_b, cross_b)
            for q in range(4):
                sums[f, g, q] = (wk * terms[q]).sum(axis=0)
                bounds[f, g, q] = (wk * errs[q]).sum(axis=0) + 2.0 ** -40 * (wk * np.abs(terms[q])).sum(axis=0)
            norm[f, g, 0] = w[ok].sum()
            norm[f, g, 1] = ok.sum()
    return Ref(sums, norm, bounds)


def forecast64(fc, va, weights=None, grouped=False):
    per_lead = fc.ndim == va.ndim
    inner = va.shape[2 if per_lead else 1:]
    if per_lead:
        count, ob_rows = (lambda f: va.shape[1]), (lambda f, cnt: va[f, :cnt])
    else:
        count, ob_rows = (lambda f: va.shape[0] - f), (lambda f, cnt: va[f:f + cnt])
    return sums64(lambda f, cnt: fc[f, :cnt], ob_rows, fc.shape[0], count, weights, grouped, inner)


def persistence64(pr, va, n_fhour, weights=None, grouped=False):
    return sums64(lambda f, cnt: pr[:cnt], lambda f, cnt: va[f:f + cnt], n_fhour, lambda f: va.shape[0] - f, weights, grouped,
                  va.shape[1:])


# -- the cases both test files use: inputs and reference computed once ------------------------------------------------------------- #
#: name -> (generator of (fc, va), weights or None as a latitude count flag, grouped, persistence leads or 0)
def _per_lead(gen, f, n, inner, seed):
    return gen((f, n) + inner, seed), gen((f, n) + inner, seed + 1)


def _series(gen, f, n, nv, inner, seed):
    return gen((f, n) + inner, seed), gen((nv,) + inner, seed + 1)


def _nonfinite(inner):
    fc, va = _per_lead(data, 2, 3, inner, 81)
    fc = plant(fc, [(0, 0, 0, 1), (1, 2, 1, 0)], np.nan)
    fc = plant(fc, [(0, 1, 1, 2)], np.inf)
    va = plant(va, [(0, 0, 0, 1), (1, 1, 0, 3)], np.nan)           # one row bad in both: counted out once
    va = plant(va, [(1, 0, 1, 4)], -np.inf)
    fc[0, 2, 0, 5, 2], va[0, 2, 0, 5, 2] = np.float32(3e38), np.float32(-3e38)      # both finite, d overflows
    return fc, va


CASES = {
    # name: (inputs, weighted, grouped, persistence leads)
    'w4': (lambda: _per_lead(data, 2, 3, (2, 3, 4), 11), True, False, 0),
    'w5': (lambda: _per_lead(data, 2, 3, (2, 3, 5), 13), True, True, 0),
    'w30': (lambda: _per_lead(data, 2, 3, (2, 6, 30), 15), False, False, 0),
    'w45': (lambda: _per_lead(data, 2, 2, (2, 7, 45), 17), True, True, 0),
    'w180': (lambda: _per_lead(data, 2, 3, (4, 2, 88, 180), 19), True, True, 0),
    'w180_red': (lambda: _per_lead(red, 1, 2, (2, 88, 180), 21), True, False, 0),
    'w360': (lambda: _per_lead(data, 1, 2, (2, 3, 360), 23), True, False, 0),
    'w360_red': (lambda: _per_lead(red, 1, 2, (1, 3, 360), 25), False, False, 0),
    'w512': (lambda: _per_lead(data, 1, 2, (2, 3, 512), 27), True, True, 0),
    'one_tile': (lambda: _per_lead(data, 1, 1, (1, 5, 12), 29), True, False, 0),            # 5 rows: below one 32-row tile
    'ragged_tiles': (lambda: _per_lead(data, 2, 3, (1, 13, 12), 31), False, False, 0),      # 39 rows: a whole tile and 7 rows
    'series': (lambda: _series(data, 7, 6, 5, (2, 6, 12), 33), True, False, 0),             # 5, 4 .. 1 pairs, leads 5 and 6 none
    'series_groups': (lambda: _series(data, 7, 6, 5, (2, 6, 10), 35), True, True, 0),
    'persistence': (lambda: (data((6, 2, 6, 12), 37), data((5, 2, 6, 12), 38)), True, True, 3),
    'offset': (lambda: _per_lead(offset, 2, 2, (2, 6, 180), 39), True, False, 0),
    'offset_odd': (lambda: _per_lead(offset, 1, 2, (1, 4, 45), 41), False, False, 0),
    'nonfinite': (lambda: _nonfinite((2, 6, 12)), True, True, 0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(fc, va, weights, grouped, n_fhour, Ref) of a named case; the arrays are shared between tests and never written"""
    make, weighted, grouped, n_fhour = CASES[name]
    fc, va = make()
    weights = cosine(va.shape[-2]) if weighted else None
    ref = persistence64(fc, va, n_fhour, weights, grouped) if n_fhour else forecast64(fc, va, weights, grouped)
    for a in (fc, va) + ((weights,) if weighted else ()) + tuple(ref):
        a.setflags(write=False)
    return fc, va, weights, grouped, n_fhour, ref


def axis_of(fc, va, grouped, n_fhour=0):
    """the `axis` argument that keeps the lead and the first inner axis, or None"""
    if not grouped:
        return None
    per_lead = not n_fhour and fc.ndim == va.ndim
    rank = va.ndim
    return ((1,) + tuple(range(3, rank))) if per_lead else ((0,) + tuple(range(2, rank)))


# -- checks -------------------------------------------------------------------------------------------------------------------------- #
def check_sums(sums, norm, ref, what):
    """sums, norm of the code under test against a Ref: the derived bounds for the sums, equal counts, sum w within 2^-40.  Prints the
    largest error / bound per entry (visible with -s) and, per entry, the share of coefficients the bound resolves to a tenth"""
    assert sums.dtype == np.float64 and norm.dtype == np.float64, what
    assert sums.shape == ref.sums.shape and norm.shape == ref.norm.shape, (what, sums.shape, ref.sums.shape)
    assert np.array_equal(norm[..., 1], ref.norm[..., 1]), (what, norm[..., 1], ref.norm[..., 1])
    assert (np.abs(norm[..., 0] - ref.norm[..., 0]) <= 2.0 ** -40 * ref.norm[..., 0]).all(), (what, norm[..., 0], ref.norm[..., 0])
    assert np.isfinite(sums).all(), what
    line = []
    for q in range(4):
        err, bound, val = np.abs(sums[..., q, :] - ref.sums[..., q, :]), ref.bounds[..., q, :], np.abs(ref.sums[..., q, :])
        ratio = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())
        resolved = float((bound[val > 0] < 0.1 * val[val > 0]).mean()) if (val > 0).any() else 1.0
        line.append('S%d %.3f (bound < value / 10 at %.0f %%)' % (q, ratio, 100 * resolved))
        assert (err <= bound).all(), (what, q, ratio)
    print('%s: error / bound  %s' % (what, '  '.join(line)))


def finish64(ref):
    """the issue's finish formulas on a Ref in float64 (no cast), with first-order-safe bounds of every field:
    {name: (value, bound)}; NaN values where the definition gives NaN, inf bounds where a bound does not resolve the denominator"""
    s, b = ref.sums, ref.bounds
    sw, n = ref.norm[..., 0], ref.norm[..., 1]
    with np.errstate(all='ignore'):
        some = (n > 0) & (sw > 0)
        den = np.where(some, sw, np.nan)[..., None]
        s0, s1, s2, s3 = (s[..., q, :] / den for q in range(4))
        b0, b1, b2, b3 = (b[..., q, :] / den * (1 + 2.0 ** -39) for q in range(4))          # sum w is within 2^-40
        p_f, b_f = s0 + s1 + 2 * s2, b0 + b1 + 2 * b2

        def quotient(a, da, c, dc):
            val = np.where(c > 0, a / c, np.nan)
            return val, np.where(c - dc > 0, (da + np.abs(val) * dc) / (c - dc), np.inf)

        ratio, b_ratio = quotient(p_f, b_f, s0, b0)
        num = (s0 + s2) ** 2 + s3 ** 2
        b_num = 2 * np.abs(s0 + s2) * (b0 + b2) + (b0 + b2) ** 2 + 2 * np.abs(s3) * b3 + b3 ** 2
        coh, b_coh = quotient(num, b_num, p_f * s0, p_f * b0 + s0 * b_f + b_f * b0)
    return {'power_forecast': (p_f, b_f), 'power_valid': (s0, b0), 'power_error': (s1, b1), 'ratio': (ratio, b_ratio),
            'coherence': (coh, b_coh)}


def check_spectrum(got, ref, grouped, what):
    """a Spectrum of the code under test against the finish of a Ref: every field inside its propagated bound plus the float32 cast
    (2^-24 relative), NaN where the reference is NaN wherever the bound resolves the denominator, equal counts"""
    assert isinstance(got, verify.Spectrum), what
    k = ref.sums.shape[-1]
    assert got.wavenumber.dtype == np.int64 and np.array_equal(got.wavenumber, np.arange(k)), what
    count = ref.norm[..., 1].astype(np.int64)
    assert got.count.dtype == np.int64 and np.array_equal(got.count, count if grouped else count[..., 0]), (what, got.count)
    line = []
    for name, (val, bound) in finish64(ref).items():
        g = getattr(got, name)
        if not grouped:
            val, bound = val[..., 0, :], bound[..., 0, :]
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == val.shape, (what, name, g.shape, val.shape)
        sure = np.isfinite(bound)
        assert np.array_equal(np.isnan(g)[sure], np.isnan(val)[sure]), (what, name)
        ok = sure & ~np.isnan(val)
        err = np.abs(g[ok].astype(np.float64) - val[ok])
        lim = bound[ok] + 2.0 ** -24 * np.abs(val[ok])
        ratio = float(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0)).max()) if err.size else 0.0
        line.append('%s %.3f' % (name, ratio))
        assert (err <= lim).all(), (what, name, ratio)
    print('%s: error / bound  %s' % (what, '  '.join(line)))
