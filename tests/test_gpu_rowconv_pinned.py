"""RowConnected2D's three passes (dlwp_rowconv2d_fwd / _fwd_direct / _bwd_data / _bwd_weight, csrc/rowconv.hip) on guarded slabs,
instance by instance: the table of tests/rowconv_cases.py (the routes themselves are asserted without a GPU by
tests/test_rowconv_cases_cpu.py).  Every tensor lies between guard elements that must keep their bits, every output starts as NaN,
every call is made twice -- 16-byte aligned operands, then each operand 1 to 3 floats past a 16-byte boundary, a different offset
per operand -- and must return the same bits.

 exact        integer inputs (family a): forward (linear, relu), dx, dw, db equal the float64 oracle TO THE BIT; nothing but NaN
              outside a written channel window; accumulate = start + gradient to the bit; db = None changes no bit of dw.
 reals        family (b), tanh: inside FWD_TOL / GRAD_BAR, the project's bars; the worst error / bar is printed.
 containment  NaN in the channels stored around a window, a NaN sample among clean ones, a NaN element of x under the weight gradient:
              the results keep the bits of the clean run wherever the reference is not NaN, and are NaN exactly / wherever it is.
 empty batch  nothing is written; the weight gradient writes exact zeros, or keeps dw and db when it accumulates.

The last test asserts that the rows run here covered every instance and vector kernel of the CPU route test and prints the MEASURED
lines DESIGN.md (parity) quotes."""
import numpy as np
import pytest
import torch

from tests import rowconv_cases as rc
from tests.test_gpu_train_ops import GUARD, Slab, exact_equal, merge, poison_outside, report, same_bits

pytestmark = pytest.mark.gpu
assert GUARD % 4 == 0

ROW_IDS = [r['name'] for r in rc.ROWS]
DGRAD_ROWS = [r for r in rc.ROWS if r['expect']['dgrad'] is not None]
WINDOWED = [r for r in rc.ROWS if r['in_win'][1] > r['cin'] or r['out_win'][1] > r['cout']]
BATCHED = [r for r in rc.ROWS if r['n'] >= 2]
MFMA_FWD = [r for r in rc.ROWS if 'mfma' in r['expect']['fwd']]
ALIGNED = dict(x=0, k=0, bias=0, dz=0, y=0, dx=0, dw=0, db=0)
SHIFTED = dict(x=1, k=3, bias=2, dz=2, y=3, dx=1, dw=2, db=3)       # floats past a 16-byte boundary, operand by operand
RAN = {p: set() for p in rc.PASSES}       # instances the tests below have launched
WORST = {}                                # '<pass> <instance> <tensor>' -> worst error / bar of family (b)
EXACT = {}                                # '<pass> <instance>' -> bit comparisons of family (a) that held
NAN_BITS = np.array([np.nan], np.float32).view(np.uint32)[0]


def names(rows):
    return [r['name'] for r in rows]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def instance(ops, row, p, n=None):
    cd, xs = rc.descriptor(ops, row, n=n)
    return rc.instance_name(p, ops.rowconv2d_launch_info(xs, cd, rc.PASSES.index(p)))


def launched(ops, row, p):
    """the route of this launch is the row's (the report is the decision the entry point launches from)"""
    name = instance(ops, row, p)
    assert name == row['expect'][p], (row['name'], p, name)
    RAN[p].add(name)
    return name


def all_nan_bits(a):
    return bool(np.all(np.ascontiguousarray(a, np.float32).view(np.uint32) == NAN_BITS))


def count_exact(key, before):
    from tests.test_gpu_train_ops import EXACT_COMPARED
    EXACT[key] = EXACT.get(key, 0) + EXACT_COMPARED[0] - before


# ---- one guarded launch of each pass ------------------------------------------------------------------------------------------------ #

def forward(ops, row, x, k, bias, act, al, direct=False):
    """-> the whole output tensor (n, out_c_total, ho, wo), NaN where nothing was written"""
    n = x.shape[0]
    cd, _ = rc.descriptor(ops, row, act, n=n)
    (_, _), (_, _), (ho, wo) = rc.geometry(row)
    sx, sk, sy = Slab(x, al['x']), Slab(k, al['k']), Slab(None, al['y'], (n, row['out_win'][1], ho, wo))
    sb = Slab(bias, al['bias']) if bias is not None else None
    ops.rowconv2d(sx.t, sk.t, sb.t if sb else None, cd, out=sy.t, direct=direct, x_channels=row['cin'])
    got = sy.read()
    assert sx.unchanged() and sk.unchanged() and (sb is None or sb.unchanged())
    return got


def data_gradient(ops, row, dz, k, al):
    """-> dx (n, cin, h, w), NaN where nothing was written"""
    from dlwp_amd._lib import Shape4
    n = dz.shape[0]
    cd, xs = rc.descriptor(ops, row, n=n)
    sz, sk, sdx = Slab(dz, al['dz']), Slab(k, al['k']), Slab(None, al['dx'], xs)
    ops.rowconv2d_bwd_data(sz.t, sk.t, cd, Shape4(*xs), sdx.t)
    got = sdx.read()
    assert sz.unchanged() and sk.unchanged()
    return got


def weight_gradient(ops, row, x, dz, al, start=None, with_db=True, n=None):
    """-> (dw, db or None); start = (dw0, db0): accumulate onto that content, None: outputs start as NaN.  n: the batch the
    descriptor names, where it is not the tensors' (the empty batch: the entry point wants addresses for x and dz all the same)"""
    from dlwp_amd._lib import Shape4
    n = x.shape[0] if n is None else n
    cd, xs = rc.descriptor(ops, row, n=n)
    (_, _), (_, _), (ho, wo) = rc.geometry(row)
    kshape = (ho,) + row['k'] + (row['cin'], row['cout'])
    sx, sz = Slab(x, al['x']), Slab(dz, al['dz'])
    sdw = Slab(start[0] if start else None, al['dw'], kshape)
    sdb = Slab(start[1] if start else None, al['db'], (ho, 1, row['cout'])) if with_db else None
    ops.rowconv2d_bwd_weight(sx.t, sz.t, sdw.t, sdb.t if sdb else None, cd, Shape4(*xs), accumulate=start is not None)
    dw, db = sdw.read(), (sdb.read() if sdb else None)
    assert sx.unchanged() and sz.unchanged()
    return dw, db


def twice(fn):
    """the call on 16-byte aligned operands and on shifted ones: the same bits"""
    a, b = fn(ALIGNED), fn(SHIFTED)
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert (u is None and v is None) or same_bits(u, v), 'the result depends on the operands\' alignment'
    return a


def outside_is_nan(y, row):
    off, c = row['out_win'][0], row['cout']
    return all_nan_bits(y[:, :off]) and all_nan_bits(y[:, off + c:])


def fwd_ratio(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / (rc.FWD_TOL * max(1.0, np.abs(want).max())))


def grad_ratio(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / (rc.GRAD_BAR * np.abs(want).max()))


# ---- exact sums and the bars ---------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_forward(ops, row):
    from tests.test_gpu_train_ops import EXACT_COMPARED
    name = launched(ops, row, 'fwd')
    before = EXACT_COMPARED[0]
    d = rc.inputs(row, 'exact')
    for act in ('linear', 'relu'):
        y = twice(lambda al: forward(ops, row, d['x'], d['k'], d['bias'], act, al))
        exact_equal(rc.window(y, row['out_win'], row['cout']), rc.reference(row, 'exact', act)['y'], '%s forward %s' % (row['name'], act))
        assert outside_is_nan(y, row), 'a channel outside the output window was written'
    count_exact('fwd ' + name, before)
    d, worst = rc.inputs(row, 'real'), {}
    y = twice(lambda al: forward(ops, row, d['x'], d['k'], d['bias'], 'tanh', al))
    assert outside_is_nan(y, row)
    r = fwd_ratio(rc.window(y, row['out_win'], row['cout']), rc.reference(row, 'real', 'tanh')['y'])
    print('\nMEASURED rowconv fwd %s %s: error / FWD_TOL %.3f' % (row['name'], name, r))
    merge(worst, 'y', r, row['name'])
    WORST['fwd %s y' % name] = max(WORST.get('fwd %s y' % name, 0.0), r)
    report('rowconv fwd %s %s' % (row['name'], name), worst)


@pytest.mark.parametrize('row', MFMA_FWD, ids=names(MFMA_FWD))
def test_forward_direct_entry_point(ops, row):
    """dlwp_rowconv2d_fwd_direct (the vector kernel) on the rows whose planned route is the matrix-core kernel"""
    d = rc.inputs(row, 'exact')
    y = twice(lambda al: forward(ops, row, d['x'], d['k'], d['bias'], 'linear', al, direct=True))
    exact_equal(rc.window(y, row['out_win'], row['cout']), rc.reference(row, 'exact')['y'], '%s direct forward' % row['name'])
    assert outside_is_nan(y, row)
    RAN['fwd'].add('fwd_simple: direct')
    report('rowconv fwd direct %s' % row['name'], {})


@pytest.mark.parametrize('row', DGRAD_ROWS, ids=names(DGRAD_ROWS))
def test_data_gradient(ops, row):
    from tests.test_gpu_train_ops import EXACT_COMPARED
    name = launched(ops, row, 'dgrad')
    before = EXACT_COMPARED[0]
    d = rc.inputs(row, 'exact')
    dx = twice(lambda al: data_gradient(ops, row, d['dz'], d['k'], al))
    exact_equal(dx, rc.reference(row, 'exact')['dx'], '%s dx' % row['name'])         # (every element written: none is NaN)
    count_exact('dgrad ' + name, before)
    d, worst = rc.inputs(row, 'real'), {}
    dx = twice(lambda al: data_gradient(ops, row, d['dz'], d['k'], al))
    r = grad_ratio(dx, rc.reference(row, 'real', 'tanh')['dx'])
    print('\nMEASURED rowconv dgrad %s %s: error / GRAD_BAR %.3f' % (row['name'], name, r))
    merge(worst, 'dx', r, row['name'])
    WORST['dgrad %s dx' % name] = max(WORST.get('dgrad %s dx' % name, 0.0), r)
    report('rowconv dgrad %s %s' % (row['name'], name), worst)


@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_weight_gradient(ops, row):
    from tests.test_gpu_train_ops import EXACT_COMPARED
    name = launched(ops, row, 'wgrad')
    RAN['wgrad'].add('bias_grad')
    before = EXACT_COMPARED[0]
    d, ref = rc.inputs(row, 'exact'), rc.reference(row, 'exact')
    dw, db = twice(lambda al: weight_gradient(ops, row, d['x'], d['dz'], al))
    exact_equal(dw, ref['dw'], '%s dw' % row['name'])
    exact_equal(db, ref['db'], '%s db' % row['name'])
    dw2, db2 = twice(lambda al: weight_gradient(ops, row, d['x'], d['dz'], al, start=(d['dw0'], d['db0'])))
    exact_equal(dw2, d['dw0'].astype(np.float64) + ref['dw'], '%s dw accumulate' % row['name'])
    exact_equal(db2, d['db0'].astype(np.float64) + ref['db'], '%s db accumulate' % row['name'])
    dw3, none = twice(lambda al: weight_gradient(ops, row, d['x'], d['dz'], al, with_db=False))
    assert none is None and same_bits(dw3, dw), 'db = None changed dw'
    count_exact('wgrad ' + name, before)
    d, ref, worst = rc.inputs(row, 'real'), rc.reference(row, 'real', 'tanh'), {}
    dw, db = twice(lambda al: weight_gradient(ops, row, d['x'], d['dz'], al))
    rw, rb = grad_ratio(dw, ref['dw']), grad_ratio(db, ref['db'])
    print('\nMEASURED rowconv wgrad %s %s: error / GRAD_BAR dw %.3f db %.3f' % (row['name'], name, rw, rb))
    merge(worst, 'dw', rw, row['name'])
    merge(worst, 'db', rb, row['name'])
    WORST['wgrad %s dw' % name] = max(WORST.get('wgrad %s dw' % name, 0.0), rw)
    WORST['wgrad bias_grad db'] = max(WORST.get('wgrad bias_grad db', 0.0), rb)
    report('rowconv wgrad %s %s' % (row['name'], name), worst)


# ---- containment ----------------------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('row', WINDOWED, ids=names(WINDOWED))
def test_nan_in_the_channels_around_a_window_reaches_nothing(ops, row):
    """x NaN in every stored channel outside [in_c_off, +cin): forward and weight gradient keep their bits; dz NaN outside
    [out_c_off, +cout): data gradient, weight gradient and bias gradient keep theirs."""
    d = rc.inputs(row, 'exact')
    xp = poison_outside(d['x'], row['in_win'][0], row['cin'])
    zp = poison_outside(d['dz'], row['out_win'][0], row['cout'])
    assert np.isnan(xp).any() and np.isnan(zp).any()
    clean = forward(ops, row, d['x'], d['k'], d['bias'], 'linear', ALIGNED)
    assert same_bits(forward(ops, row, xp, d['k'], d['bias'], 'linear', SHIFTED), clean), 'forward read a channel outside its window'
    if row['expect']['dgrad'] is not None:
        clean = data_gradient(ops, row, d['dz'], d['k'], ALIGNED)
        assert same_bits(data_gradient(ops, row, zp, d['k'], SHIFTED), clean), 'the data gradient read dz outside its window'
    dw, db = weight_gradient(ops, row, d['x'], d['dz'], ALIGNED)
    dwp, dbp = weight_gradient(ops, row, xp, zp, SHIFTED)
    assert same_bits(dwp, dw), 'the weight gradient read x or dz outside a window'
    assert same_bits(dbp, db), 'the bias gradient read dz outside its window'


@pytest.mark.parametrize('row', BATCHED, ids=names(BATCHED))
def test_a_nan_sample_stays_in_its_sample(ops, row):
    """sample 1 all NaN (it shares a workgroup's sample group with sample 0 wherever groups hold two): the other samples keep the bits
    of the clean run, the poisoned one is NaN wherever the reference is"""
    d, s = rc.inputs(row, 'exact'), 1
    others = [i for i in range(row['n']) if i != s]
    xp = d['x'].copy()
    xp[s, row['in_win'][0]:row['in_win'][0] + row['cin']] = np.nan
    clean = forward(ops, row, d['x'], d['k'], d['bias'], 'linear', ALIGNED)
    got = forward(ops, row, xp, d['k'], d['bias'], 'linear', ALIGNED)
    assert same_bits(got[others], clean[others]), 'a NaN sample reached another sample\'s forward'
    want = rc.forward_oracle(row, xp, d['k'], d['bias'])
    assert np.isnan(want[s]).all() and np.isnan(rc.window(got, row['out_win'], row['cout'])[s]).all()
    if row['expect']['dgrad'] is None:
        return
    zp = d['dz'].copy()
    zp[s, row['out_win'][0]:row['out_win'][0] + row['cout']] = np.nan
    clean = data_gradient(ops, row, d['dz'], d['k'], ALIGNED)
    got = data_gradient(ops, row, zp, d['k'], ALIGNED)
    assert same_bits(got[others], clean[others]), 'a NaN sample reached another sample\'s data gradient'
    want = rc.grads_oracle(row, d['x'], d['k'], zp)[0]
    assert np.isnan(want[s]).any() and np.isnan(got[s][np.isnan(want[s])]).all()


@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_a_nan_in_x_reaches_the_weight_gradients_that_read_it_and_no_others(ops, row):
    """x NaN at the last stored column of the last row (last sample, last channel of the window) and at the first column of the first
    row (first sample and channel): dw[r, ky, kx, ci, :] is NaN exactly where the float64 reference is -- a product of that element with
    a column of dz that does not exist (the padding of a row to whole k steps) must not count --, every other element keeps its bits."""
    d = rc.inputs(row, 'exact')
    off, cin = row['in_win'][0], row['cin']
    for pos in ((row['n'] - 1, off + cin - 1, row['h'] - 1, row['w'] - 1), (0, off, 0, 0)):
        xp = d['x'].copy()
        xp[pos] = np.nan
        want = rc.grads_oracle(row, xp, d['k'], d['dz'])[1]
        dw, db = weight_gradient(ops, row, xp, d['dz'], ALIGNED)
        bad = np.isnan(want)
        assert np.array_equal(np.isnan(dw), bad), '%s x[%r] = NaN: dw is NaN in %d elements, the reference in %d (%d outside it)' % (
            row['name'], pos, np.isnan(dw).sum(), bad.sum(), (np.isnan(dw) & ~bad).sum())
        assert np.array_equal(dw[~bad].astype(np.float64), want[~bad])
        assert same_bits(db, rc.reference(row, 'exact')['db'].astype(np.float32))


# ---- the empty batch ------------------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_empty_batch(ops, row):
    """n = 0: forward and data gradient launch nothing; the weight gradient runs its vector kernel, which writes exact zeros -- or keeps
    dw and db when it accumulates (its x and dz: one NaN sample that must not be read)."""
    d = rc.inputs(row, 'exact')
    for p in rc.PASSES:
        if row['expect'][p] is not None:
            assert instance(ops, row, p, n=0) == '%s_simple: empty batch' % p
    RAN['wgrad'].add('wgrad_simple: empty batch')
    x0, z0 = d['x'][:0], d['dz'][:0]
    y = forward(ops, row, x0, d['k'], d['bias'], 'linear', SHIFTED)
    assert y.shape[0] == 0
    if row['expect']['dgrad'] is not None:
        assert data_gradient(ops, row, z0, d['k'], SHIFTED).shape[0] == 0
    x1, z1 = np.full_like(d['x'][:1], np.nan), np.full_like(d['dz'][:1], np.nan)
    dw, db = weight_gradient(ops, row, x1, z1, SHIFTED, n=0)
    assert same_bits(dw, np.zeros_like(dw)) and same_bits(db, np.zeros_like(db)), 'the empty batch\'s gradient is not +0.0 everywhere'
    dw, db = weight_gradient(ops, row, x1, z1, ALIGNED, start=(d['dw0'], d['db0']), n=0)
    assert same_bits(dw, d['dw0']) and same_bits(db, d['db0']), 'accumulating an empty batch changed dw / db'


# ---- what ran -------------------------------------------------------------------------------------------------------------------------- #

def test_every_instance_ran_and_the_measured_ratios():
    """after the tests above: the launches covered every compiled instance, all three vector kernels (for every reason a kernel can be
    run for) and the bias gradient; prints the worst family (b) ratios per pass and instance"""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    for p in rc.PASSES:
        runnable = [why for why in rc.REASONS[p] if why != '32-bit offsets' and (why != 'empty batch' or p == 'wgrad')]
        want = set(rc.COMPILED[p]) | {'%s_simple: %s' % (p, why) for why in runnable}
        assert want <= RAN[p], (p, sorted(want - RAN[p]))
    assert 'fwd_simple: direct' in RAN['fwd'] and 'bias_grad' in RAN['wgrad']
    for key in sorted(EXACT):
        print('\nMEASURED rowconv %s: family (a) exact (%d comparisons)' % (key, EXACT[key]))
    for key in sorted(WORST):
        print('\nMEASURED rowconv %s: family (b) worst error / bar %.3f' % (key, WORST[key]))
        assert WORST[key] <= 1.0
    for p in rc.PASSES:                       # every compiled instance has passed bit comparisons of its own
        for name in rc.COMPILED[p]:
            assert EXACT.get('%s %s' % (p, name), 0) > 0, name
