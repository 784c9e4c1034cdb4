"""Shared by tests/test_skill_cpu.py and tests/test_gpu_skill.py: the float64 restatement of forecast_skill / persistence_skill, the
derived bounds of DESIGN.md 5.38, and the inputs (the generator of tests/test_gpu_verify.py: 3 N(0, 1) + 1).

Restatement: per lead d = float64(fc) - float64(ob), fa = float64(fc) - float64(c), oa = float64(ob) - float64(c); a pair with a NaN
among them, or with label -1, is skipped; weighted sums and the scores of the issue's table in float64.

Bounds.  The code under test rounds d, fa, oa once in float32 (2^-24 relative each) and sums in float64 (n 2^-53, negligible), the
result is cast once (2^-24):
  mse, rmse, mae   terms of one sign keep the relative bound: 2^-23 + 2^-24 < 2^-22 |ref|
  bias             terms of both signs: |sum w (d' - d)| <= 2^-24 sum w |d|, so 2^-24 mae_ref, and the cast 2^-24 |bias_ref|; the
                   stated bound 2^-23 mae_ref + 2^-24 |bias_ref| holds it twice over
  acc              numerator: 2^-23 sum w |fa oa| <= 2^-23 sqrt(S7 S8) (Cauchy-Schwarz); denominator: S7, S8 each 2^-23 relative, the
                   root of their product 2^-23; |acc| <= 1; the cast 2^-24: below 2^-22 + 2^-24 < 2^-21 absolute
  acc_centered     the same errors divided by the centred variances instead of the raw second moments: 2^-21 kappa with
                   kappa = max((S7 / S0) / var_f, (S8 / S0) / var_o) of the reference; the tests assert kappa <= 2
Where the reference is 0, NaN or infinite the result is equal to it."""
import collections

import numpy as np

from dlwp_amd.model import verify

Ref = collections.namedtuple('Ref', 'mse rmse mae bias acc acc_centered count kappa')


def data(shape, seed, nan_every=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 3.0 + 1.0).astype(np.float32)
    if nan_every:
        x.ravel()[seed % nan_every::nan_every] = np.nan
    return x


def table_of(inner, seed, n_labels=12):
    return (np.random.default_rng(seed).standard_normal((n_labels,) + tuple(inner)) * 0.5).astype(np.float32)


def labels_of(shape, seed, n_labels=12):
    return np.random.default_rng(seed).integers(0, n_labels, shape).astype(np.int32)


def cosine(h):
    return verify.area_weights(np.linspace(-90.0, 90.0, h))


def sums64(fc_rows, ob_rows, label_rows, leads, count, table, weights, grouped, inner):
    """(leads, groups, 10) float64: *_rows(f, cnt) give the rows lead f pairs; count(f) their number"""
    groups = inner[0] if grouped else 1
    out = np.zeros((leads, groups, 10))
    w = 1.0 if weights is None else np.asarray(weights, np.float64).reshape(-1, 1)
    for f in range(leads):
        cnt = count(f)
        if cnt <= 0:
            continue
        fc, ob = fc_rows(f, cnt).astype(np.float64), ob_rows(f, cnt).astype(np.float64)
        skip = np.zeros(cnt, bool)
        c = 0.0
        if table is not None:
            lab = label_rows(f, cnt) if label_rows is not None else np.zeros(cnt, np.int64)
            skip = lab < 0
            c = table.astype(np.float64)[np.maximum(lab, 0)]
        with np.errstate(invalid='ignore'):
            d, fa, oa = fc - ob, fc - c, ob - c
        ok = ~(np.isnan(d) | np.isnan(fa) | np.isnan(oa)) & ~skip.reshape((cnt,) + (1,) * len(inner))
        d, fa, oa = (np.where(ok, v, 0.0) for v in (d, fa, oa))
        wk = ok * w
        ax = tuple(a for a in range(d.ndim) if not (grouped and a == 1))
        terms = (wk, wk * d, wk * d * d, wk * np.abs(d), wk * fa, wk * oa, wk * fa * oa, wk * fa * fa, wk * oa * oa, ok)
        out[f] = np.stack([np.sum(t, axis=ax) for t in terms], axis=-1).reshape(groups, 10)
    return out


def scores64(s, grouped):
    """the issue's formulas in float64 on (leads, groups, 10) sums, plus kappa"""
    s0, s1, s2, s3, s4, s5, s6, s7, s8, n = (s[..., k] for k in range(10))
    with np.errstate(all='ignore'):
        some = (n > 0) & (s0 > 0)
        s0 = np.where(some, s0, np.nan)
        mf, mo = s4 / s0, s5 / s0
        var_f, var_o = s7 / s0 - mf * mf, s8 / s0 - mo * mo
        den = np.sqrt(s7 * s8)
        acc = np.where(some & (den > 0), s6 / den, np.nan)
        den = np.sqrt(var_f * var_o)
        acc_c = np.where(some & (den > 0), (s6 / s0 - mf * mo) / den, np.nan)
        kappa = np.maximum((s7 / s0) / var_f, (s8 / s0) / var_o)
        vals = [s2 / s0, np.sqrt(s2 / s0), s3 / s0, s1 / s0, acc, acc_c, n.astype(np.int64), kappa]
    return Ref(*(vals if grouped else [v[:, 0] for v in vals]))


def forecast64(fc, va, table=None, labels=None, weights=None, grouped=False):
    per_lead = fc.ndim == va.ndim
    inner = va.shape[2 if per_lead else 1:]
    if per_lead:
        count, ob_rows = (lambda f: va.shape[1]), (lambda f, cnt: va[f, :cnt])
        lab_rows = None if labels is None else (lambda f, cnt: labels[f, :cnt])
    else:
        count, ob_rows = (lambda f: va.shape[0] - f), (lambda f, cnt: va[f:f + cnt])
        lab_rows = None if labels is None else (lambda f, cnt: labels[f:f + cnt])
    if table is not None and table.shape == tuple(inner):
        table = table[None]
    s = sums64(lambda f, cnt: fc[f, :cnt], ob_rows, lab_rows, fc.shape[0], count, table, weights, grouped, inner)
    return scores64(s, grouped)


def persistence64(pr, va, n_fhour, table=None, labels=None, weights=None, grouped=False):
    lab_rows = None if labels is None else (lambda f, cnt: labels[f:f + cnt])
    s = sums64(lambda f, cnt: pr[:cnt], lambda f, cnt: va[f:f + cnt], lab_rows, n_fhour, lambda f: va.shape[0] - f, table, weights,
               grouped, va.shape[1:])
    return scores64(s, grouped)


def check_skill(got, ref, what):
    """got: a Skill of the code under test; ref: a Ref.  Prints error / bound per score (visible with -s) and asserts the bounds"""
    assert isinstance(got, verify.Skill), what
    assert got.count.dtype == np.int64 and np.array_equal(got.count, ref.count), (what, got.count, ref.count)
    with np.errstate(invalid='ignore'):
        bounds = {'mse': 2.0 ** -22 * np.abs(ref.mse), 'rmse': 2.0 ** -22 * np.abs(ref.rmse), 'mae': 2.0 ** -22 * np.abs(ref.mae),
                  'bias': 2.0 ** -23 * ref.mae + 2.0 ** -24 * np.abs(ref.bias), 'acc': np.full(ref.acc.shape, 2.0 ** -21),
                  'acc_centered': 2.0 ** -21 * ref.kappa}
    centred = ~np.isnan(ref.acc_centered)
    assert (ref.kappa[centred] <= 2.0).all(), (what, ref.kappa)
    line = []
    for name, bound in bounds.items():
        g, want = getattr(got, name), getattr(ref, name)
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == want.shape, (what, name, g.shape, want.shape)
        assert np.array_equal(np.isnan(g), np.isnan(want)), (what, name, g, want)
        exact = np.isinf(want) | (want == 0)
        assert np.array_equal(g[exact].astype(np.float64), want[exact]), (what, name)
        ok = ~np.isnan(want) & ~exact
        err = np.abs(g[ok].astype(np.float64) - want[ok])
        ratio = float((err / bound[ok]).max()) if err.size else 0.0
        line.append('%s %.3f' % (name, ratio))
        assert (err <= bound[ok]).all(), (what, name, ratio)
    print('%s: error / bound  %s' % (what, '  '.join(line)))
