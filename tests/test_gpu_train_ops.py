"""dlwp_act_bwd, dlwp_bias_grad, dlwp_act_bwd_bias_grad, dlwp_pool_act_bwd_bias_grad, dlwp_mse_mae, dlwp_mse_mae_phase and
dlwp_loss_custom against the float64 oracles of oracle/np_ref.py, on the two input families of tests/test_train_ops_cpu.py: (a)
exact inputs, whose sums must equal the oracle's TO THE BIT, and (b) random inputs inside the bounds DERIVED there (u = 2^-24;
nothing is tuned to what the kernels deliver).  Every output starts as NaN, every tensor lies between guard elements that must keep
their bits, every call is made twice and must give the same bits.  Each test prints `exact` for family (a) and the worst error /
bound ratio for family (b); a ratio above 1 is a finding.  DESIGN.md (parity) holds the measured ratios."""
import numpy as np
import pytest
import torch

from oracle import np_ref
from tests.test_optimizers_cpu import U, f32, worst_ratio
from tests.test_train_ops_cpu import (ACTS, LOSS_SHAPES, PHASE_SHAPES, POOL_SHAPES, SECOND, SLICED_SHAPES, act_bwd_oracle, act_case,
                                      custom_loss_oracle, exact_loss_case, flat_sizes, k_act_bias, k_flat, k_phase, k_sliced,
                                      LIMIT, REAL_MARGIN, exact_condition, loss_combos, loss_exact_condition, mse_mae_oracle,
                                      pool_act_bwd_oracle, pool_case, ratios_of, real_loss_case, small_ints, sum_oracle)

pytestmark = pytest.mark.gpu

GUARD = 64            # floats, a multiple of 4: a slab at `align` 0 starts 16-byte aligned, at 2 8-byte aligned, at 1 4-byte aligned
GUARD_VALUE = np.float32(-7.25e11)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def cu_count():
    import ctypes
    from dlwp_amd import _lib
    cu = ctypes.c_int(0)
    _lib.check(_lib.lib.dlwp_device_info(_lib.handle(torch.cuda.current_device()), ctypes.byref(cu), None, None, 0))
    assert cu.value > 0
    return cu.value


def code(ops, act):
    return ops.ACTIVATIONS[act]


class Slab(object):
    """A float32 tensor of any shape inside a larger flat buffer, `align` elements past a 16-byte boundary, with guard elements on
    both sides that a kernel must leave bit-identical.  values None: filled with NaN (an output)."""

    def __init__(self, values, align=0, shape=None):
        if values is None:
            values = np.full(shape, np.nan, dtype=np.float32)
        values = np.ascontiguousarray(values, dtype=np.float32)
        n, off = values.size, GUARD + align
        host = np.full(n + 2 * GUARD + 4, GUARD_VALUE, dtype=np.float32)
        host[off:off + n] = values.reshape(-1)
        self.host, self.off, self.n, self.shape = host, off, n, values.shape
        self.buf = torch.from_numpy(host.copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[off:off + n].view(values.shape)

    def read(self):
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy()
        lo, hi = self.off, self.off + self.n
        assert np.array_equal(now[:lo].view(np.uint32), self.host[:lo].view(np.uint32)), 'guard below the tensor was written'
        assert np.array_equal(now[hi:].view(np.uint32), self.host[hi:].view(np.uint32)), 'guard above the tensor was written'
        return now[lo:hi].reshape(self.shape).copy()

    def unchanged(self):
        return same_bits(self.read(), self.host[self.off:self.off + self.n].reshape(self.shape))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


EXACT_COMPARED = [0]         # bit comparisons of family (a) that held since the last report()


def exact_equal(got, want64, what):
    """family (a): a float32 result against the float64 sum, to the bit"""
    got = np.atleast_1d(np.asarray(got, np.float64))
    want64 = np.atleast_1d(np.asarray(want64, np.float64))
    assert np.array_equal(got, want64), '%s: exact inputs, yet %r != %r (difference %r)' % (what, got, want64, got - want64)
    EXACT_COMPARED[0] += 1


def exact_inputs(per_channel_terms, unit, what):
    """the exactness condition on the arrays that reach the kernel: per channel, sum |term| / unit is an integer below 2^24"""
    for t in per_channel_terms:
        assert exact_condition(t, unit) < LIMIT, what


def scaled_ok(got, s64, n, what):
    """an exact float32 sum scaled by fl(1 / n): two roundings"""
    assert abs(float(got) - s64 / n) <= 2 * U * SECOND * abs(s64 / n), '%s: %r against %r' % (what, float(got), s64 / n)
    EXACT_COMPARED[0] += 1


def report(what, worst):
    """`exact` is printed only if family (a) comparisons were made, and every one of them held, since the last report"""
    compared, EXACT_COMPARED[0] = EXACT_COMPARED[0], 0
    print('\nMEASURED %s: family (a) %s; family (b) worst error/bound %s' % (
        what, 'exact (%d comparisons)' % compared if compared else 'not run',
        ', '.join('%s %.3f' % kv for kv in sorted(worst.items())) or 'none'))


def merge(worst, name, r, what=''):
    assert r <= 1.0, '%s %s: error / bound = %.3f' % (name, what, r)
    worst[name] = max(worst.get(name, 0.0), r)


def poison_outside(a, c_off, c):
    """NaN in every channel outside [c_off, c_off + c)"""
    a = a.copy()
    a[:, :c_off] = np.nan
    a[:, c_off + c:] = np.nan
    return a


# ---- dlwp_act_bwd ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('act', ACTS)
def test_act_bwd_every_size_and_the_kinks(ops, act):
    """Sizes 1 ... above the grid cap and the step's 64x4x88x180 and (tanh, relu; linear is a copy) 64x32x88x180, the latter on
    reals only: relu / linear bit-equal to the oracle, tanh inside |g| (2 |1 - t^2| + t^2) u; y == 0, -0.0 (relu) and +-1 (tanh)
    give exactly 0."""
    rng = np.random.default_rng(601)
    worst = {}
    for n in flat_sizes(cu_count()):
        if n > 64 * 4 * 88 * 180 and act == 'linear':
            continue
        for exact in (True, False):
            if exact and n > 10 ** 7:
                continue
            y, dy = act_case(rng, (n,), act, exact)
            sy, sdy, sdz = Slab(y, 1), Slab(dy, 3), Slab(None, 1, (n,))
            assert ops.act_bwd(sy.t if act != 'linear' else None, sdy.t, code(ops, act), out=sdz.t) is sdz.t
            got = sdz.read()
            sdz2 = Slab(None, 2, (n,))
            ops.act_bwd(sy.t if act != 'linear' else None, sdy.t, code(ops, act), out=sdz2.t)
            assert same_bits(got, sdz2.read()) and sy.unchanged() and sdy.unchanged()
            want, bound = act_bwd_oracle(y, dy, act)
            if exact:
                exact_equal(got, want, 'act_bwd %s n %d' % (act, n))
            else:
                merge(worst, 'dz', worst_ratio(got, want, bound, 'act_bwd %s' % act), 'n %d' % n)
                if act == 'relu':
                    assert np.all(got[(y == 0)] == 0)
                if act == 'tanh':
                    assert np.all(got[np.abs(y) == 1] == 0)
    report('act_bwd %s' % act, worst)


# ---- the channel-sliced sums ----------------------------------------------------------------------------------------------------- #

def run_bias_grad(ops, dz, c_off, c, align=1):
    sdz, sdb = Slab(dz, align), Slab(None, 1, (c,))
    ops.bias_grad(sdz.t, sdb.t, c, c_off)
    got = sdb.read()
    sdb2 = Slab(None, 3, (c,))
    ops.bias_grad(sdz.t, sdb2.t, c, c_off)
    assert same_bits(got, sdb2.read()) and sdz.unchanged()
    return got


def test_bias_grad_exact_sums_and_derived_bounds(ops):
    """dlwp_bias_grad on every plane shape (hw % 4 == 0, even, odd), N 1 and 64, N hw < 64, channel windows between NaN channels:
    integers and all-ones sum exactly (all-ones: db == N hw), reals inside k u sum |dz|."""
    rng = np.random.default_rng(602)
    worst = {}
    for (n, ct, h, w, c_off, c) in SLICED_SHAPES:
        k = k_sliced(n * h * w)
        ones = poison_outside(np.ones((n, ct, h, w), np.float32), c_off, c)
        exact_equal(run_bias_grad(ops, ones, c_off, c), np.full(c, n * h * w), 'bias_grad ones %r' % ((n, ct, h, w),))
        ints = poison_outside(small_ints(rng, (n, ct, h, w), 1.0), c_off, c)
        exact_inputs([ints[:, ch] for ch in range(c_off, c_off + c)], 1, 'bias_grad')
        exact_equal(run_bias_grad(ops, ints, c_off, c), np_ref.channel_sum(ints, c_off, c), 'bias_grad %r' % ((n, ct, h, w),))
        real = poison_outside(rng.standard_normal((n, ct, h, w)).astype(np.float32), c_off, c)
        want, bound = sum_oracle(real, c_off, c, k)
        merge(worst, 'db', ratios_of(run_bias_grad(ops, real, c_off, c, align=0), want, bound, 'bias_grad'), (n, ct, h, w))
    report('bias_grad', worst)


def vec_of(hw, align):
    """the instance dlwp_act_bwd_bias_grad picks (train_ops.hip:596-598)"""
    if hw % 4 == 0 and align % 4 == 0:
        return 4
    return 2 if hw % 2 == 0 and align % 2 == 0 else 1


def run_act_bwd_bias(ops, y, dy, act, c_off, c, align, in_place):
    """-> (dz of the window, db); checks the guards, the channels outside the window, the inputs and a second call"""
    n, ct, h, w = dy.shape
    results = []
    for _ in range(2):
        sy, sdy, sdb = Slab(y, align), Slab(dy, align), Slab(None, 1, (c,))
        sdz = sdy if in_place else Slab(None, align, dy.shape)
        ops.act_bwd_bias_grad(sy.t if act != 'linear' else None, sdy.t, code(ops, act), sdb.t, c, c_off, out=sdz.t)
        dz, db = sdz.read(), sdb.read()
        before = dy if in_place else np.full(dy.shape, np.nan, np.float32)
        assert same_bits(dz[:, :c_off], before[:, :c_off]) and same_bits(dz[:, c_off + c:], before[:, c_off + c:]), \
            'a channel outside the window was written'
        assert sy.unchanged() and (in_place or sdy.unchanged())
        results.append((dz[:, c_off:c_off + c].copy(), db))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])
    return results[0]


@pytest.mark.parametrize('act', ACTS)
def test_act_bwd_bias_grad_exact_sums_and_derived_bounds(ops, act):
    """dlwp_act_bwd_bias_grad on every plane shape and window, out of place and in place (dz is dy), y and dy NaN outside the window:
    dz as dlwp_act_bwd's oracle, db exact on integers and on all-ones, inside k u sum |dz| of its own dz on reals."""
    rng = np.random.default_rng(603)
    worst = {}
    for (n, ct, h, w, c_off, c) in SLICED_SHAPES:
        shape, win = (n, ct, h, w), slice(c_off, c_off + c)
        for in_place in (False, True):
            y, dy = act_case(rng, shape, act, True)
            y, dy = poison_outside(y, c_off, c), poison_outside(dy, c_off, c)
            dz, db = run_act_bwd_bias(ops, y, dy, act, c_off, c, 0, in_place)
            want, _ = act_bwd_oracle(y[:, win], dy[:, win], act)
            exact_inputs([want[:, ch] for ch in range(c)], 0.25, 'act_bwd_bias_grad')
            exact_equal(dz, want, 'dz %s %r' % (act, shape))
            exact_equal(db, want.sum(axis=(0, 2, 3)), 'db %s %r in_place %r' % (act, shape, in_place))
        if act == 'linear':
            ones = poison_outside(np.ones(shape, np.float32), c_off, c)
            for align in (0, 1, 2):
                _, db = run_act_bwd_bias(ops, ones, ones, act, c_off, c, align, False)
                exact_equal(db, np.full(c, n * h * w), 'db of ones %r align %d' % (shape, align))
        y, dy = act_case(rng, shape, act, False)
        y, dy = poison_outside(y, c_off, c), poison_outside(dy, c_off, c)
        dz, db = run_act_bwd_bias(ops, y, dy, act, c_off, c, 0, True)
        want, bound = act_bwd_oracle(y[:, win], dy[:, win], act)
        merge(worst, 'dz', worst_ratio(dz, want, bound, 'dz'), shape)
        want, bound = sum_oracle(dz, 0, c, k_act_bias(n, h * w, vec_of(h * w, 0)))
        merge(worst, 'db', ratios_of(db, want, bound, 'db'), shape)
    report('act_bwd_bias_grad %s' % act, worst)


@pytest.mark.parametrize('act', ACTS)
def test_act_bwd_bias_grad_float4_float2_and_scalar_instances_on_one_input(ops, act):
    """The same data 0, 2 and 1 elements past a 16-byte boundary (hw % 4 == 0: the float4, float2 and scalar instances run): the
    same dz bits from all three, db exact on integers and inside each instance's own k on reals; the scalar instance also on an
    odd plane at every offset."""
    rng = np.random.default_rng(604)
    worst = {}
    for (n, ct, h, w, c_off, c) in [(6, 3, 44, 90, 1, 2), (64, 2, 22, 90, 0, 2), (3, 3, 2, 6, 1, 2), (5, 3, 7, 9, 1, 2)]:
        shape, win = (n, ct, h, w), slice(c_off, c_off + c)
        for exact in (True, False):
            y, dy = act_case(rng, shape, act, exact)
            y, dy = poison_outside(y, c_off, c), poison_outside(dy, c_off, c)
            want, bound = act_bwd_oracle(y[:, win], dy[:, win], act)
            if exact:
                exact_inputs([want[:, ch] for ch in range(c)], 0.25, 'act_bwd_bias_grad instances')
            first = None
            for align in (0, 2, 1):
                dz, db = run_act_bwd_bias(ops, y, dy, act, c_off, c, align, align == 2)
                first = dz if first is None else first
                assert same_bits(dz, first), 'dz differs between the vector instances (offset %d)' % align
                if exact:
                    exact_equal(dz, want, 'dz')
                    exact_equal(db, want.sum(axis=(0, 2, 3)), 'db %s %r offset %d' % (act, shape, align))
                else:
                    merge(worst, 'dz', worst_ratio(dz, want, bound, 'dz'), shape)
                    ws, bs = sum_oracle(dz, 0, c, k_act_bias(n, h * w, vec_of(h * w, align)))
                    merge(worst, 'db vec%d' % vec_of(h * w, align), ratios_of(db, ws, bs, 'db'), shape)
    report('act_bwd_bias_grad %s instances' % act, worst)


def run_pool(ops, y, dp, act, align, dz_align, with_db=True):
    """dz is a NaN-filled slab of its own alignment between guards: every element must be written, nothing beyond"""
    n, c, h, w = y.shape
    sy, sdp, sdb, sdz = Slab(y, align), Slab(dp, 1), Slab(None, 1, (c,)), Slab(None, dz_align, y.shape)
    assert ops.pool_act_bwd_bias_grad(sy.t, sdp.t, code(ops, act), sdb.t if with_db else None, out=sdz.t) is sdz.t
    dz = sdz.read()
    assert not np.isnan(dz).any(), 'an element of dz was not written'
    assert sy.unchanged() and sdp.unchanged()
    return dz, (sdb.read() if with_db else None)


@pytest.mark.parametrize('act', ACTS)
def test_pool_act_bwd_bias_grad_exact_sums_ties_and_both_instances(ops, act):
    """dlwp_pool_act_bwd_bias_grad: even and odd H / W, N hw < 64, the pair instance (even W, y and dz 8-byte aligned) and the scalar
    one (y or dz one element off) on the same data, dz a NaN-filled tensor between guards of which no NaN may remain; ties (constant windows, -0.0 against 0) go to the first maximum; dz as the oracle (bit
    equal for relu / linear, the tanh bound otherwise), db exact on integers; twice, and without db, the same bits."""
    rng = np.random.default_rng(605)
    worst = {}
    for shape in POOL_SHAPES:
        n, c, h, w = shape
        k = k_sliced(n * ((h + 1) // 2) * ((w + 1) // 2))
        for exact in (True, False):
            y, dp = pool_case(rng, shape, exact)
            want, bound = pool_act_bwd_oracle(y, dp, act)
            if exact:
                exact_inputs([want[:, ch] for ch in range(c)], 0.25, 'pool')
            first = None
            for align, dz_align in ((0, 0), (1, 0), (0, 1), (1, 1)):
                dz, db = run_pool(ops, y, dp, act, align, dz_align)
                dz2, db2 = run_pool(ops, y, dp, act, align, dz_align)
                dz3, _ = run_pool(ops, y, dp, act, align, dz_align, with_db=False)
                assert same_bits(dz, dz2) and same_bits(db, db2) and same_bits(dz, dz3)
                first = dz if first is None else first
                assert same_bits(dz, first), 'dz differs between the pair and the scalar instance'
                assert np.all(dz[:, :, 2 * (h // 2):] == 0) and np.all(dz[:, :, :, 2 * (w // 2):] == 0)
                if exact:
                    exact_equal(dz, want, 'pool dz %s %r' % (act, shape))
                    exact_equal(db, want.sum(axis=(0, 2, 3)), 'pool db %s %r offset %d' % (act, shape, align))
                else:
                    merge(worst, 'dz', worst_ratio(dz, want, bound, 'pool dz'), shape)
                    ws, bs = sum_oracle(dz, 0, c, k)
                    merge(worst, 'db', ratios_of(db, ws, bs, 'pool db'), shape)
    report('pool_act_bwd_bias_grad %s' % act, worst)


# ---- dlwp_mse_mae, dlwp_mse_mae_phase ---------------------------------------------------------------------------------------------- #

def run_mse_mae(ops, syp, syt, lw, want_dy=True):
    """on input slabs that the caller keeps (and checks once, after its last call)"""
    so = Slab(None, 1, (2,))
    sdy = Slab(None, 1, syp.shape) if want_dy else None
    ops.mse_mae(syp.t, syt.t, so.t, sdy.t if want_dy else None, lw)
    return so.read(), (sdy.read() if want_dy else None)


def test_mse_mae_every_size_exact_sums_and_derived_bounds(ops):
    """dlwp_mse_mae at sizes 1 ... above the grid cap and the step's 64x4x88x180 and 64x32x88x180: integers give s2 and s1 exactly
    (the value is then two roundings from s / n), reals stay inside (k + 5) u mse, (k + 3) u mae, 4 u |dy|; d == 0 gives dy == 0;
    with and without dy, and twice, the same bits."""
    rng = np.random.default_rng(606)
    cu = cu_count()
    worst = {}
    for n in flat_sizes(cu):
        lw = f32(0.7) if n % 2 else 1.0
        k = k_flat(n, cu)
        yp, yt, _, _ = exact_loss_case(rng, (1, 1, 1, n))
        assert loss_exact_condition(yp, yt, None, None) < LIMIT
        syp, syt = Slab(yp, 1), Slab(yt, 3)
        out, dy = run_mse_mae(ops, syp, syt, lw)
        assert syp.unchanged() and syt.unchanged()
        (v2, v1), _, wdy, bdy, (s2, s1) = mse_mae_oracle(yp, yt, lw, k)
        scaled_ok(out[0], s2, n, 'mse n %d' % n)
        scaled_ok(out[1], s1, n, 'mae n %d' % n)
        assert worst_ratio(dy, wdy, bdy, 'dy') <= 1.0 and np.all(dy[yp == yt] == 0)
        if n <= 64 * 4 * 88 * 180:
            # s = out / fl(1 / n) recovers the integer sum while s < 2^22 (the two roundings move it by less than half a unit)
            inv_n = float(np.float32(1) / np.float32(n))
            if s2 < 2 ** 21:
                assert round(float(out[0]) / inv_n) == s2 and round(float(out[1]) / inv_n) == s1, (n, out, s2, s1)
        yp, yt, _, _ = real_loss_case(rng, (1, 1, 1, n))
        yp.reshape(-1)[::5] = yt.reshape(-1)[::5]
        syp, syt = Slab(yp, 1), Slab(yt, 3)
        out, dy = run_mse_mae(ops, syp, syt, lw)
        out2, dy2 = run_mse_mae(ops, syp, syt, lw)
        out3, _ = run_mse_mae(ops, syp, syt, lw, want_dy=False)
        assert same_bits(out, out2) and same_bits(dy, dy2) and same_bits(out, out3)
        assert syp.unchanged() and syt.unchanged()
        (v2, v1), (b2, b1), wdy, bdy, _ = mse_mae_oracle(yp, yt, lw, k)
        merge(worst, 'mse', ratios_of(out[0], v2, b2, 'mse'), n)
        merge(worst, 'mae', ratios_of(out[1], v1, b1, 'mae'), n)
        merge(worst, 'dy', worst_ratio(dy, wdy, bdy, 'dy'), n)
        assert np.all(dy.reshape(-1)[::5] == 0)
    report('mse_mae', worst)


def test_mse_mae_phase_exact_sums_and_derived_bounds(ops):
    """dlwp_mse_mae_phase: the phase tensor (n, 4f, h, w) against the target (n, f, 2h, 2w), channel (2a + b) f + co.  Integers:
    s2, s1 and the 4f bias sums exact; reals: values, dz (phase layout) and db (against its own dz) inside their bounds; with and
    without dz / db the same bits."""
    rng = np.random.default_rng(607)
    worst = {}
    for (n, f, h, w) in PHASE_SHAPES:
        kl, kb = k_phase(n, f, h, w)
        numel = 4 * n * f * h * w
        for exact in (True, False):
            yp, yt, _, _ = (exact_loss_case if exact else real_loss_case)(rng, (n, f, 2 * h, 2 * w))
            assert not exact or loss_exact_condition(yp, yt, None, None) < LIMIT
            ph = np_ref.space_to_depth2(yp)
            lw = 1.0 if exact else f32(0.7)
            sph, syt, so = Slab(ph, 1), Slab(yt, 3), Slab(None, 1, (2,))
            sdz, sdb = Slab(None, 1, ph.shape), Slab(None, 3, (4 * f,))
            ops.mse_mae_phase(sph.t, syt.t, so.t, sdz.t, sdb.t, lw)
            out, dz, db = so.read(), sdz.read(), sdb.read()
            so2, sdb2, sdz2 = Slab(None, 3, (2,)), Slab(None, 1, (4 * f,)), Slab(None, 2, ph.shape)
            ops.mse_mae_phase(sph.t, syt.t, so2.t, sdz2.t, sdb2.t, lw)
            assert same_bits(out, so2.read()) and same_bits(db, sdb2.read()) and same_bits(dz, sdz2.read())
            so3, sdb3 = Slab(None, 3, (2,)), Slab(None, 1, (4 * f,))
            ops.mse_mae_phase(sph.t, syt.t, so3.t, None, sdb3.t, lw)
            so4 = Slab(None, 1, (2,))
            ops.mse_mae_phase(sph.t, syt.t, so4.t, None, None, lw)
            assert same_bits(out, so3.read()) and same_bits(db, sdb3.read()) and same_bits(out, so4.read())
            assert sph.unchanged() and syt.unchanged()
            s2, s1, v2, v1, wdz, wdb = np_ref.mse_mae_phase(ph, yt, lw)
            assert worst_ratio(dz, wdz, 4 * U * SECOND * np.abs(wdz), 'phase dz') <= 1.0
            if exact:
                scaled_ok(out[0], s2, numel, 'phase mse')
                scaled_ok(out[1], s1, numel, 'phase mae')
                # db sums g = scale d with d in {-1, 0, 1}: +-scale, not a power of two, so this sum is not exact; it is held to
                # k u sum |dz| of its own dz, which on these sparse fields is below half of one term: a lost element still shows
                scale = float(np.float32(2) * np.float32(lw) * np.float32(1.0 / numel))
                ws, bs = sum_oracle(dz, 0, 4 * f, kb)
                assert ratios_of(db, ws, bs, 'phase db') <= 1.0 and bs.max() < 0.5 * scale
            else:
                merge(worst, 'mse', ratios_of(out[0], v2, (kl + 5) * U * SECOND * v2, 'phase mse'), (n, f, h, w))
                merge(worst, 'mae', ratios_of(out[1], v1, (kl + 3) * U * SECOND * v1, 'phase mae'), (n, f, h, w))
                merge(worst, 'dz', worst_ratio(dz, wdz, 4 * U * SECOND * np.abs(wdz), 'dz'), (n, f, h, w))
                ws, bs = sum_oracle(dz, 0, 4 * f, kb)
                merge(worst, 'db', ratios_of(db, ws, bs, 'phase db'), (n, f, h, w))
    report('mse_mae_phase', worst)


# ---- dlwp_loss_custom ---------------------------------------------------------------------------------------------------------------- #

def run_loss(ops, dev, kind, reg, lw, want_dy=True):
    """-> (stats[7], dy, the kernel's own sums read back from its workspace).  The workspace layout is dlwp_loss_custom's own
    (dlwp_amd/csrc/train_ops.hip: dlwp_loss_workspace, and `extra = partial + cu_count * 8 * 9; plane = extra + 2` in
    dlwp_loss_custom): whoever changes it there changes the offsets here."""
    syp, syt, smean, sroww = dev
    n, c, h, w = syp.shape
    sst = Slab(None, 1, (7,))
    sdy = Slab(None, 1, syp.shape) if want_dy else None
    ops.loss_custom(syp.t, syt.t, sst.t, sdy.t if want_dy else None, lw, None if smean is None else smean.t,
                    None if sroww is None else sroww.t, kind, reg)
    stats = sst.read()
    ws = ops.workspace(syp.t.device, 0).view(torch.float32)         # partials (cu 8 9) | extra (2) | plane sums (2 n c)
    at = cu_count() * 8 * 9
    extra = ws[at:at + 2].cpu().numpy().astype(np.float64)
    plane = ws[at + 2:at + 2 + 2 * n * c].cpu().numpy().astype(np.float64).reshape(n * c, 2)
    sums = {'spt': stats[3], 'spp': stats[4], 'stt': stats[5], 'extra': extra, 'plane': plane}      # (the caller checks the inputs)
    return stats, (sdy.read() if want_dy else None), sums


@pytest.mark.parametrize('shape', LOSS_SHAPES)
def test_loss_custom_all_stats_and_gradient_exact_sums_and_derived_bounds(ops, shape):
    """dlwp_loss_custom, kind 0 and kind 1 x regularize 0 ... 4 x climatology x row weights, loss_weight 1 / 0.7 (at 64x4x88x180:
    both or neither of climatology and weights, family (a) with both).  Integers: S_pt, S_pp, S_tt, the global and the plane sums exact, mse / mae two
    roundings from their exact sums.  Reals: all seven stats inside their bounds, the gradient inside its per-element bound from the
    kernel's OWN sums.  regularize 3 / 4 run on fields with |q| >= 0.01 by construction."""
    rng = np.random.default_rng(608)
    n, c, h, w = shape
    numel = n * c * h * w
    big = numel > 10 ** 6
    cu = cu_count()
    worst = {}
    hosts = {(fam, pos): (exact_loss_case if fam == 'a' else real_loss_case)(rng, shape, pos) for fam in 'ab' for pos in (False, True)}
    devs = {key: tuple(Slab(a, 1) for a in val) for key, val in hosts.items()}
    for pos in (False, True):
        yp, yt, mean, row_w = hosts[('a', pos)]
        assert max(loss_exact_condition(yp, yt, m_, w_) for m_ in (None, mean) for w_ in (None, row_w)) < LIMIT
    for w_ in (None, hosts[('b', True)][3]):                    # family (b), regularize 3 / 4: |q| >= REAL_MARGIN for every plane
        yp, yt = (a.astype(np.float64) * (1.0 if w_ is None else w_.astype(np.float64).reshape(1, 1, h, 1)) for a in hosts[('b', True)][:2])
        sp, st = yp.sum(axis=(2, 3)), yt.sum(axis=(2, 3))
        assert (st > 0).all() and (np.abs((st - sp) / st) >= REAL_MARGIN).all() and abs((st.sum() - sp.sum()) / st.sum()) >= REAL_MARGIN
    for kind, reg, um, uw, lw in loss_combos():
        if big and um != uw:
            continue
        for fam in 'ab':
            if big and fam == 'a' and not um:
                continue
            yp, yt, mean, row_w = hosts[(fam, reg >= 3)]
            syp, syt, smean, sroww = devs[(fam, reg >= 3)]
            mean, row_w, dev = (mean if um else None), (row_w if uw else None), (syp, syt, smean if um else None, sroww if uw else None)
            stats, dy, sums = run_loss(ops, dev, kind, reg, lw)
            want, bstats, wdy, bdy, aux = custom_loss_oracle(yp, yt, mean, row_w, kind, reg, lw, sums, cu)
            what = 'kind %d reg %d mean %r weights %r lw %g %r' % (kind, reg, um, uw, lw, shape)
            if fam == 'a':
                exact_equal(stats[3:6], want[3:6], 'S_pt, S_pp, S_tt ' + what)
                if reg >= 3:
                    exact_equal(sums['extra'], aux['extra'], 'global sums ' + what)
                if reg == 4:
                    exact_equal(sums['plane'], aux['plane'], 'plane sums ' + what)
                scaled_ok(stats[1], want[1] * numel, numel, 'mse ' + what)
                scaled_ok(stats[2], want[2] * numel, numel, 'mae ' + what)
                for j in (0, 6):
                    assert ratios_of(stats[j], want[j], bstats[j], 'stats[%d]' % j) <= 1.0, what
                assert worst_ratio(dy, wdy, bdy, 'dy') <= 1.0, what
            else:
                for j in range(7):
                    merge(worst, 'stats[%d]' % j, ratios_of(stats[j], want[j], bstats[j], 'stats[%d]' % j), what)
                merge(worst, 'dy', worst_ratio(dy, wdy, bdy, 'dy'), what)
                stats2, dy2, _ = run_loss(ops, dev, kind, reg, lw)
                stats3, _, _ = run_loss(ops, dev, kind, reg, lw, want_dy=False)
                assert same_bits(stats, stats2) and same_bits(dy, dy2) and same_bits(stats, stats3), what
    for key, dev in devs.items():
        assert all(s.unchanged() for s in dev)
    report('loss_custom %dx%dx%dx%d' % shape, worst)


# ---- deferred reductions, empty batches ------------------------------------------------------------------------------------------ #

def test_deferred_final_sums_give_the_bits_of_the_immediate_kernels_on_exact_inputs(ops):
    """bias_grad, act_bwd_bias_grad and mse_mae between reductions_begin and reductions_flush (the final sums then run in
    csrc/batch.hip, in another order): on family (a) the sums are exact in any order, so the results are the same bits."""
    rng = np.random.default_rng(609)
    for (n, ct, h, w, c_off, c) in SLICED_SHAPES[1:4] + [(64, 2, 22, 90, 0, 2)]:
        shape = (n, ct, h, w)
        y, dy = act_case(rng, shape, 'tanh', True)
        yp, yt, _, _ = exact_loss_case(rng, shape)
        dzw = np_ref.act_bwd(y, dy, 'tanh')
        exact_inputs([dzw[:, ch] for ch in range(ct)] + [dy[:, ch] for ch in range(ct)], 0.25, 'deferred')
        assert loss_exact_condition(yp, yt, None, None) < LIMIT
        sy, sdy, syp, syt = Slab(y, 0), Slab(dy, 0), Slab(yp, 1), Slab(yt, 1)
        got = {}
        for deferred in (False, True):
            sdb1, sdb2, so, sdz = Slab(None, 1, (c,)), Slab(None, 3, (c,)), Slab(None, 1, (2,)), Slab(None, 0, shape)
            if deferred:
                ops.reductions_begin(sy.t.device)
            try:
                ops.bias_grad(sdy.t, sdb1.t, c, c_off, ws_key='t1' if deferred else None)
                ops.act_bwd_bias_grad(sy.t, sdy.t, ops.ACT_TANH, sdb2.t, c, c_off, out=sdz.t, ws_key='t2' if deferred else None)
                ops.mse_mae(syp.t, syt.t, so.t, None, 1.0, ws_key='t3' if deferred else None)
                if deferred:        # the final sums are recorded, not done: the results are still the NaN they started as
                    assert all(np.isnan(s.read()).all() for s in (sdb1, sdb2, so)), 'a deferred sum was written before the flush'
            finally:
                if deferred:
                    ops.reductions_flush(sy.t.device)
            got[deferred] = (sdb1.read(), sdb2.read(), so.read())
        exact_equal(got[True][0], np_ref.channel_sum(dy, c_off, c), 'deferred bias_grad')
        exact_equal(got[True][1], np_ref.channel_sum(dzw, c_off, c), 'deferred act_bwd_bias_grad')
        for a, b in zip(got[False], got[True]):
            assert same_bits(a, b), (shape, a, b)
    print('\nMEASURED deferred bias_grad / act_bwd_bias_grad / mse_mae: family (a) exact, the bits of the immediate kernels')


def test_empty_batches(ops):
    """n == 0 through ops.*: the backward wrappers return, a bias gradient of nothing is zeros, nothing else is written; a loss of
    nothing is a ValueError."""
    base = Slab(np.arange(32, dtype=np.float32), 1)
    e = base.t[3:3].view(0, 2, 3, 4)
    assert e.numel() == 0
    for fill in range(2):
        sdb = Slab(None, 1, (2,))
        assert ops.act_bwd(e, e, ops.ACT_TANH, out=e) is e
        if fill == 0:
            ops.bias_grad(e, sdb.t, 2)
        else:
            ops.act_bwd_bias_grad(e, e, ops.ACT_RELU, sdb.t, 2, out=e)
        assert same_bits(sdb.read(), np.zeros(2, np.float32))
    sdb = Slab(None, 1, (2,))
    dz = ops.pool_act_bwd_bias_grad(e, base.t[5:5].view(0, 2, 1, 2), ops.ACT_TANH, sdb.t)
    assert tuple(dz.shape) == (0, 2, 3, 4) and same_bits(sdb.read(), np.zeros(2, np.float32))
    assert tuple(ops.pool_act_bwd_bias_grad(e, base.t[5:5].view(0, 2, 1, 2), ops.ACT_TANH).shape) == (0, 2, 3, 4)
    out2, st = Slab(None, 1, (2,)), Slab(None, 1, (7,))
    with pytest.raises(ValueError, match='empty'):
        ops.mse_mae(e, e, out2.t)
    with pytest.raises(ValueError, match='empty'):
        ops.mse_mae_phase(base.t[3:3].view(0, 4, 3, 4), base.t[3:3].view(0, 1, 6, 8), out2.t)
    with pytest.raises(ValueError, match='empty'):
        ops.loss_custom(e, e, st.t)
    assert base.unchanged() and out2.unchanged() and st.unchanged()
