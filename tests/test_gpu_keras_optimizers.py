"""dlwp_optimizer_step (every kind) and dlwp_grad_clip_factor against the float64 oracles of tests/test_keras_optimizers_cpu.py, started
from the kernel's own float32 state, inside the single-step bounds DERIVED there (u = 2^-24; nothing here is tuned to what the
kernels deliver).  Each test prints the worst error / bound ratio it saw (-s); a ratio above 1 is a finding.  DESIGN.md (parity)
holds the measured ratios."""
import numpy as np
import pytest
import torch

from tests.test_gpu_optimizers import cu_count, merge, report, sizes
from tests.test_keras_optimizers_cpu import (CODE, KINDS, N_SLOTS, NAMES, clip_oracle, hypers_of, kind_state, nadam_m_schedule,
                                             oracle, step_scalars)
from tests.test_optimizers_cpu import GRAD_SCALES, ITERATIONS, U, f32, worst_ratio

pytestmark = pytest.mark.gpu

LEAD = 64           # elements in front of a slice: the buffer itself is 256-byte aligned, so the slice starts `off` elements
TAIL = 67           # behind a 16-byte boundary
OFFSETS = (0, 1, 2, 3)
MIXED = (1, 3, 2, 0, 3, 1)      # p, slots..., g at different offsets: no common 16-byte phase
STEP_GRAD_SCALES = (f32(1e-4), 1.0, 1e3)          # (float32 values: the C ABI takes a float)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


class Slice(object):
    """A float32 tensor that is a slice of a larger flat buffer at element offset `off` past a 16-byte boundary (the pattern of
    test_gpu_optimizers.Slab, any offset), with guard elements on both sides that a kernel must leave bit-identical."""

    def __init__(self, values, off):
        n = values.size
        host = np.full(LEAD + off + n + TAIL, np.float32(-7.25e11), dtype=np.float32)
        host[LEAD + off:LEAD + off + n] = values
        self.host, self.lo, self.n = host, LEAD + off, n
        self.buf = torch.from_numpy(host.copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.lo:self.lo + n]

    def read(self):
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy()
        lo, hi = self.lo, self.lo + self.n
        assert np.array_equal(now[:lo].view(np.uint32), self.host[:lo].view(np.uint32)), 'guard below the slice was written'
        assert np.array_equal(now[hi:].view(np.uint32), self.host[hi:].view(np.uint32)), 'guard above the slice was written'
        return now[lo:hi].copy()


def launch(ops, kind, state, iteration, hyper, decay, grad_scale, offs, clipvalue=0.0, factor=None, m_schedule=1.0):
    """One dlwp_optimizer_step on float32 host state (p, slots, g) held in guarded slices at element offsets `offs`; checks guards,
    g's bits and every bound; returns {name: worst error / bound}.  factor: a device tensor (grad_clip_factor's) or None."""
    p, slots, g = state
    arrays = [p] + list(slots) + [g]
    sl = [Slice(a, o) for a, o in zip(arrays, offs)]
    kw = dict(hyper)
    if kind == 'nadam':
        kw['m_schedule'] = m_schedule
    else:
        kw['decay'] = decay
    ops.optimizer_step(CODE[kind], sl[0].t, [s.t for s in sl[1:-1]], sl[-1].t, iteration, grad_scale=grad_scale,
                       clipvalue=clipvalue, factor=factor, **kw)
    got = [s.read() for s in sl]
    assert np.array_equal(got[-1].view(np.uint32), g.view(np.uint32)), 'the gradient was written'
    fac = None if factor is None else factor.cpu().numpy()[0]
    sc = step_scalars(kind, hyper, 0.0 if kind == 'nadam' else decay, iteration, m_schedule)
    want, bound = oracle(kind, p, slots, g, sc, hyper, grad_scale, clipvalue, fac)
    ratios = {}
    for name, a, w, b in zip(NAMES[kind], got[:-1], want, bound):
        r = worst_ratio(a, w, b, '%s %s' % (kind, name))
        assert r <= 1.0, '%s %s: error / bound = %.3f (n %d, offsets %r, iteration %d, decay %g, grad_scale %g, clipvalue %g, %r)' % (
            kind, name, r, p.size, offs, iteration, decay, grad_scale, clipvalue, hyper)
        ratios[name] = r
    zero = (g == 0) & np.logical_and.reduce([s == 0 for s in slots])        # nothing to add: the weight keeps its bits
    assert np.array_equal(got[0][zero].view(np.uint32), p[zero].view(np.uint32))
    return ratios


def schedule_of(kind, hyper, iteration):
    return nadam_m_schedule(hyper['h1'], hyper['schedule_decay'], iteration) if kind == 'nadam' else 1.0


@pytest.mark.parametrize('kind', KINDS)
def test_every_size_at_every_offset_with_guards(ops, kind):
    """Sizes 1 ... above the grid cap, every array at element offset 0, 1, 2, 3 past a 16-byte boundary (head of 0, 3, 2, 1 elements
    in front of the 16-byte body) and once with the arrays at DIFFERENT offsets (the element-wise kernel); state of a run in progress
    (iteration 7), decayed rate, grad_scale 0.5: every element inside its bound, nothing outside the slice touched, g untouched.
    The 16-byte kernel moves four elements per thread: its grid-stride loop repeats from 4 x the cap on, the last size."""
    rng = np.random.default_rng(101 + CODE[kind])
    worst = {}
    hypers = hypers_of(kind)
    big = 4 * 8 * cu_count() * 256 + 12345
    for n in sizes() + [big]:
        for k, off in enumerate((0, 3) if n == big else OFFSETS + (None,)):
            hyper = hypers[k % 2]
            offs = MIXED[:N_SLOTS[kind] + 2] if off is None else (off,) * (N_SLOTS[kind] + 2)
            state = kind_state(rng, kind, n, 7, 1.0)
            merge(worst, launch(ops, kind, state, 7, hyper, f32(1e-3), 0.5, offs, m_schedule=schedule_of(kind, hyper, 7)))
    report('%s sizes and offsets' % kind, worst)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('iteration', ITERATIONS)
def test_iterations_decay_grad_scale_and_gradient_scales(ops, kind, iteration):
    """Zero slots (iteration 0) and later steps up to 10^6, decay 0 and 1e-3, grad_scale 1e-4, 1 and 1e3 on gradients of scale
    1e-4, 1 and 1e3, both hyper-parameter sets, with and without a clipvalue of half the gradient scale; exact zeros and the cancelling
    b1 m ~ -(1 - b1) g mixed in; the written slots are compared as well as the weights."""
    rng = np.random.default_rng(202 + iteration % 1000 + 7 * CODE[kind])
    n = 20011
    worst = {}
    k = 0
    for g_scale in GRAD_SCALES:
        for grad_scale in STEP_GRAD_SCALES:
            for decay in (0.0, f32(1e-3)):
                for hyper in hypers_of(kind):
                    state = kind_state(rng, kind, n, iteration, g_scale)
                    cv = f32(0.5 * g_scale * grad_scale) if k % 2 else 0.0
                    offs = (k % 4,) * (N_SLOTS[kind] + 2)
                    k += 1
                    merge(worst, launch(ops, kind, state, iteration, hyper, decay, grad_scale, offs, clipvalue=cv,
                                        m_schedule=schedule_of(kind, hyper, iteration)))
    report('%s iteration %d' % (kind, iteration), worst)


@pytest.mark.parametrize('kind', KINDS)
def test_zero_gradient_and_zero_slots_keep_every_bit(ops, kind):
    """g = 0 with zero slots: p keeps its bits and the slots stay zero, at an iteration where every step scalar is in play"""
    rng = np.random.default_rng(7)
    for n in (257, 200003):
        p = rng.standard_normal(n).astype(np.float32)
        z = np.zeros(n, np.float32)
        for hyper in hypers_of(kind):
            sl = [Slice(a, 1) for a in [p] + [z] * (N_SLOTS[kind] + 1)]
            kw = dict(hyper)
            if kind == 'nadam':
                kw['m_schedule'] = 0.7
            ops.optimizer_step(CODE[kind], sl[0].t, [s.t for s in sl[1:-1]], sl[-1].t, 3, **kw)
            assert np.array_equal(sl[0].read().view(np.uint32), p.view(np.uint32))
            for s in sl[1:]:
                assert not s.read().any()


def test_empty_tensors_and_bad_arguments(ops):
    buf = torch.arange(16, dtype=torch.float32, device='cuda')
    keep = buf.clone()
    e = [buf[k:k] for k in (3, 5, 7, 9, 11)]
    for kind in KINDS:
        ops.optimizer_step(CODE[kind], e[0], e[1:1 + N_SLOTS[kind]], e[4], 5, **hypers_of(kind)[0])
    out = ops.grad_clip_factor(e[0], 1.0)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    assert out.cpu().numpy().tolist() == [1.0, 0.0, 0.0]            # the norm of nothing is 0: no clipping
    with pytest.raises(ValueError):
        ops.optimizer_step(CODE['adam'], buf[:4], [buf[4:8]], buf[8:12], 0, lr=0.1)       # Adam takes two slot arrays
    with pytest.raises(ValueError):
        ops.optimizer_step(99, buf[:4], [buf[4:8]], buf[8:12], 0, lr=0.1)
    with pytest.raises(ValueError):
        ops.optimizer_step(CODE['sgd'], buf[:4], [buf[4:7]], buf[8:12], 0, lr=0.1)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


# ---- the clip pass ------------------------------------------------------------------------------------------------------------ #

def test_clip_factor_is_bit_reproducible_and_exact_on_integers(ops):
    """Two launches on the same input give the same bits; gradients of +-1 and 0 have exact partial sums in any order, so the device
    sum of squares equals the count; g = (3, 4) at clipnorm 5 takes the n >= c branch with a factor of exactly 1."""
    rng = np.random.default_rng(31)
    for n in (200003, 8 * cu_count() * 256 * 4 + 12345):
        g = (rng.standard_normal(n) * 3).astype(np.float32)
        s = Slice(g, 1)
        a = ops.grad_clip_factor(s.t, 1.0, 0.5).clone()
        b = ops.grad_clip_factor(s.t, 1.0, 0.5, out=torch.empty(3, dtype=torch.float32, device='cuda'))
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
        assert np.array_equal(s.read().view(np.uint32), g.view(np.uint32))
    g = rng.integers(-1, 2, 200003).astype(np.float32)
    count = int((g != 0).sum())
    for off in OFFSETS:
        out = ops.grad_clip_factor(Slice(g, off).t, 1e9).cpu().numpy()
        assert out[2] == np.float32(count) and out[0] == 1.0 and out[1] == np.float32(np.sqrt(count))
    out = ops.grad_clip_factor(torch.tensor([3.0, 4.0], device='cuda'), 5.0).cpu().numpy()
    assert out.tolist() == [1.0, 5.0, 25.0]
    out = ops.grad_clip_factor(torch.tensor([3.0, 4.0], device='cuda'), 5.0, 2.0).cpu().numpy()       # norm 10: halved
    assert out.tolist() == [0.5, 10.0, 100.0]


def test_clip_factor_against_float64_on_every_size_and_offset(ops):
    """Thresholds at 0.5 x and 2 x the norm (never within the norm's own error of it, where oracle and kernel may branch
    differently), grad_scale 1e-4, 1, 1e3, every size and offset: factor, norm and sum of squares inside their bounds; below the
    threshold the factor is exactly 1."""
    rng = np.random.default_rng(32)
    worst = {}
    for n in sizes():
        for k, off in enumerate(OFFSETS):
            g = rng.standard_normal(n).astype(np.float32)
            g[::17] = 0
            gs = STEP_GRAD_SCALES[(k + n) % 3]
            s = Slice(g, off)
            norm = clip_oracle(g, gs, 0.0)[0][1]
            for mult in (0.5, 2.0):
                c = f32(mult * norm) if norm > 0 else 1.0
                got = ops.grad_clip_factor(s.t, c, gs).cpu().numpy()
                want, bound = clip_oracle(g, gs, c)
                for name, a, w, b in zip(('factor', 'norm', 'sumsq'), got, want, bound):
                    r = worst_ratio(np.array([a]), np.array([w]), np.array([b]), 'clip %s' % name)
                    assert r <= 1.0, (name, n, off, gs, mult, a, w, r)
                    merge(worst, {name: r})
                if mult == 2.0 or norm == 0:
                    assert got[0] == 1.0
            assert np.array_equal(s.read().view(np.uint32), g.view(np.uint32))
    report('clip factor', worst)


@pytest.mark.parametrize('kind', KINDS)
def test_clipnorm_then_clipvalue_through_the_update(ops, kind):
    """The whole clipped step as the trainer issues it: dlwp_grad_clip_factor at a threshold of 0.5 x the norm leaves its factor on
    the device, the update reads it and clamps afterwards; the oracle takes the device's float32 factor (its own bound is checked
    above), so the update's bound is that of two roundings on the gradient."""
    rng = np.random.default_rng(33 + CODE[kind])
    worst = {}
    for n, off in ((257, 1), (200003, 0), (200003, 3)):
        for hyper in hypers_of(kind):
            state = kind_state(rng, kind, n, 7, 1.0)
            norm = clip_oracle(state[2], 0.5, 0.0)[0][1]
            gd = torch.from_numpy(state[2]).cuda()
            factor = ops.grad_clip_factor(gd, f32(0.5 * norm), 0.5)
            assert abs(float(factor[0].item()) - 0.5) <= 4 * U
            merge(worst, launch(ops, kind, state, 7, hyper, f32(1e-3), 0.5, (off,) * (N_SLOTS[kind] + 2), clipvalue=f32(0.3),
                                factor=factor, m_schedule=schedule_of(kind, hyper, 7)))
    report('%s clipped' % kind, worst)
