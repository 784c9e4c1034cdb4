"""Shared by tests/test_quantiles_cpu.py and tests/test_gpu_quantiles.py: the definition of the label quantiles restated one column at a
time in plain Python / float64 (no code shared with dlwp_amd.model.verify.label_quantiles_host), the data makers, and the cross-check
against numpy.nanquantile.

The definition (include/dlwp_hip.h: dlwp_verify_label_quantiles).  Per (label, column): drop the NaNs (v != v), sort the n values left by
the unsigned key of their bits (sign bit set: u ^ 0xffffffff, else u | 0x80000000 -- a total order, -0.0 < +0.0), h = (n - 1) * q as
one float64 product; 'lower' s[floor(h)], 'higher' s[ceil(h)], 'nearest' s[rint(h)], 'linear' a = s[floor(h)] where g = h - floor(h)
is 0 and float32(a + (b - a) * g) in float64 otherwise, b = s[min(floor(h) + 1, n - 1)]; NaN (0x7fc00000) where n == 0."""
import math

import numpy as np

METHODS = ('linear', 'lower', 'higher', 'nearest')
ORDER_METHODS = METHODS[1:]
QS = (0.0, 0.05, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.95, 1.0)
Q_SETS = {1: (0.5,), 3: (1.0 / 3.0, 2.0 / 3.0, 0.95), 8: QS + (0.25,)}
QNAN = 0x7fc00000
# NaNs of both signs, quiet and signalling, with payloads: none of them may sort low or be counted
NAN_BITS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fc12345], np.uint32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """equal bits everywhere, NaNs included: every NaN the definition returns is 0x7fc00000"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = bits(got), bits(want)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, '%d of %d elements differ, first at %d: %r != %r' % (bad.size, got.size, bad[0], got.reshape(-1)[bad[0]],
                                                                              want.reshape(-1)[bad[0]])


def key_of(u):
    u = int(u)
    return u ^ 0xffffffff if u & 0x80000000 else u | 0x80000000


def column_quantile(col, q, method):
    """one column (float32, any length), one probability -> the bits of the quantile, and n"""
    u = bits(col)
    kept = sorted((key_of(b), int(b)) for b, v in zip(u, col) if v == v)
    n = len(kept)
    if n == 0:
        return QNAN, 0
    s = [b for _, b in kept]
    h = float(n - 1) * float(q)
    lo = int(math.floor(h))
    if method == 'lower':
        return s[lo], n
    if method == 'higher':
        return s[int(math.ceil(h))], n
    if method == 'nearest':
        return s[int(np.rint(h))], n
    g = h - lo
    if g == 0.0:
        return s[lo], n
    a = float(np.array(s[lo], np.uint32).view(np.float32))
    b = float(np.array(s[min(lo + 1, n - 1)], np.uint32).view(np.float32))
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.float32(np.float64(a) + (np.float64(b) - np.float64(a)) * np.float64(g))
    return (QNAN if v != v else int(np.array([v], np.float32).view(np.uint32)[0])), n


def quantiles_restated(x, labels, n_labels, q, method):
    """(K, n_labels) + x.shape[1:] float32 and (n_labels,) + x.shape[1:] int32, one column at a time"""
    q = np.atleast_1d(np.asarray(q, np.float64))
    flat = x.reshape(x.shape[0], -1)
    out = np.empty((q.size, n_labels, flat.shape[1]), np.uint32)
    cnt = np.empty((n_labels, flat.shape[1]), np.int32)
    for l in range(n_labels):
        rows = flat[np.asarray(labels) == l]
        for c in range(flat.shape[1]):
            for k in range(q.size):
                out[k, l, c], cnt[l, c] = column_quantile(rows[:, c], q[k], method)
    return out.view(np.float32).reshape((q.size, n_labels) + x.shape[1:]), cnt.reshape((n_labels,) + x.shape[1:])


# -- data --------------------------------------------------------------------------------------------------------------------------- #
KINDS = ('gauss', 'ties', 'special', 'inf')


def make_data(shape, kind, seed, nan_share=0.1):
    """float32 of `shape` (count, ...).  'gauss': N(1, 3); 'ties': integers in -3 .. 3; 'special': -0.0 and +0.0 mixed with subnormals
    of both signs and a few ordinary values; 'inf': Gaussian with infinities of both signs (for the order-statistic methods: 'linear'
    between two infinities is inf - inf).  NaNs of both signs and with payloads are sprinkled over nan_share of the elements; with more
    than two rows column 0 is all NaN, column 1 one repeated value."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == 'gauss' or kind == 'inf':
        x = (rng.standard_normal(n) * 3.0 + 1.0).astype(np.float32)
        if kind == 'inf':
            where = rng.random(n) < 0.1
            x[where] = np.where(rng.random(int(where.sum())) < 0.5, np.float32(np.inf), np.float32(-np.inf))
    elif kind == 'ties':
        x = rng.integers(-3, 4, n).astype(np.float32)
    elif kind == 'special':
        pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00012345, 0x3f800000, 0xbf800000,
                         0x00800000], np.uint32).view(np.float32)
        x = pool[rng.integers(0, pool.size, n)]
    else:
        raise ValueError(kind)
    u = x.view(np.uint32).copy()
    where = rng.random(n) < nan_share
    u[where] = NAN_BITS[rng.integers(0, NAN_BITS.size, int(where.sum()))]
    u = u.reshape(shape[0], -1)
    if shape[0] > 2 and u.shape[1] > 2:
        u[:, 0] = NAN_BITS[np.arange(shape[0]) % NAN_BITS.size]
        u[:, 1] = np.float32(-2.5).view(np.uint32)
    return u.view(np.float32).reshape(shape)


def labels_for(count, n_labels, seed):
    """half of the samples carry label 0 (a long list), the rest are spread; the last label of three or more carries none"""
    rng = np.random.default_rng(seed)
    top = n_labels - 1 if n_labels >= 3 else n_labels
    lab = rng.integers(0, top, count).astype(np.int32)
    lab[rng.random(count) < 0.5] = 0
    return lab


# -- the cross-check against numpy --------------------------------------------------------------------------------------------------- #
def numpy_columns(seed=0, columns=400, longest=301, n_q=32):
    """400 columns of 1 .. 301 samples as one (301, 400) array whose unused tail is NaN (a dropped NaN is a missing sample); half the
    columns Gaussian, half integers in -3 .. 3, 10 % NaN inside, and 32 probabilities with 0, 1 and the terciles among them"""
    rng = np.random.default_rng(seed)
    x = np.full((longest, columns), np.nan, np.float32)
    for c in range(columns):
        n = int(rng.integers(1, longest + 1))
        col = (rng.standard_normal(n) * 3.0 + 1.0) if c % 2 else rng.integers(-3, 4, n)
        col = col.astype(np.float32)
        col[rng.random(n) < 0.1] = np.nan
        if np.isnan(col).all():
            col[0] = 1.5
        x[:n, c] = col
    q = np.concatenate([[0.0, 1.0, 0.5, 1.0 / 3.0, 2.0 / 3.0, 0.05, 0.95], rng.random(n_q - 7)])
    return x, q


def numpy_quantiles(x, q, method):
    """np.nanquantile on a float64 copy over axis 0, rounded to float32: (K,) + x.shape[1:]"""
    return np.nanquantile(x.astype(np.float64), q, axis=0, method=method).astype(np.float32)
