"""dlwp_adam_keras, dlwp_adam_keras_dev, dlwp_sgd_keras and dlwp_axpby against float64 oracles started from the kernel's own float32
state, inside the single-step bounds DERIVED in tests/test_optimizers_cpu.py (u = 2^-24; nothing here is tuned to what the kernels
deliver).  Each test prints the worst error / bound ratio it saw; a ratio above 1 is a finding.  DESIGN.md (parity) holds the
measured ratios."""
import numpy as np
import pytest
import torch

from oracle import np_ref, torch_ref
from tests.test_optimizers_cpu import (GRAD_SCALES, ITERATIONS, adam_lr_t, adam_oracle, axpby_oracle, f32, optimizer_state,
                                       sgd_lr, sgd_oracle, worst_ratio)

pytestmark = pytest.mark.gpu

KERNELS = ('adam_keras', 'adam_keras_dev', 'sgd_keras')


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


def sizes():
    """1, 3, around one block, a large odd size, and one above grid_for's cap of 8 * cu_count blocks of 256 threads (the
    grid-stride loop then runs more than once)"""
    return [1, 3, 255, 256, 257, 200003, 8 * cu_count() * 256 + 12345]


GUARD = 67


class Slab(object):
    """A float32 tensor that is a slice of a larger flat buffer at an ODD element offset (as flat_params[off:off + numel] is),
    with guard elements on both sides that a kernel must leave bit-identical."""

    def __init__(self, values, off):
        assert off % 2 == 1 and off <= GUARD
        n = values.size
        host = np.full(n + 2 * GUARD, np.float32(-7.25e11), dtype=np.float32)
        host[off:off + n] = values
        self.host, self.off, self.n = host, off, n
        self.buf = torch.from_numpy(host.copy()).cuda()
        self.t = self.buf[off:off + n]

    def read(self):
        """the slice on the host; asserts the guards first"""
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy()
        lo, hi = self.off, self.off + self.n
        assert np.array_equal(now[:lo].view(np.uint32), self.host[:lo].view(np.uint32)), 'guard below the slice was written'
        assert np.array_equal(now[hi:].view(np.uint32), self.host[hi:].view(np.uint32)), 'guard above the slice was written'
        return now[lo:hi].copy()


ADAM_DEFAULT = dict(lr=f32(1e-3), beta_1=f32(0.9), beta_2=f32(0.999), epsilon=f32(1e-7))
ADAM_OTHER = dict(lr=f32(2e-3), beta_1=f32(0.8), beta_2=f32(0.99), epsilon=f32(1e-3))


def run_step(ops, kernel, state, iteration, hyper, decay, grad_scale):
    """One launch of `kernel` on float32 host state (p, m | vel, v, g) held in odd-offset slices; returns {name: worst
    error / bound}.  adam_keras_dev: also checks the step number it leaves and the bits of lr_t in its scratch word."""
    p, m, v, g = state
    sp, sm, sv, sg = Slab(p, 1), Slab(m, 3), Slab(v, 5), Slab(g, 7)
    ratios = {}
    if kernel == 'sgd_keras':
        ops.sgd_keras(sp.t, sm.t, sg.t, iteration, lr=hyper['lr'], momentum=hyper['momentum'], decay=decay, grad_scale=grad_scale)
        got = (sp.read(), sm.read())
        want, bound = sgd_oracle(p, m, g, iteration, hyper['lr'], hyper['momentum'], decay, grad_scale)
        names = ('p', 'vel')
        assert np.array_equal(sv.read(), v)
    else:
        lr_t = adam_lr_t(hyper['lr'], hyper['beta_1'], hyper['beta_2'], decay, iteration)
        if kernel == 'adam_keras':
            ops.adam_keras(sp.t, sm.t, sv.t, sg.t, iteration, decay=decay, grad_scale=grad_scale, **hyper)
        else:
            it_dev = torch.tensor([iteration], dtype=torch.int64, device='cuda')
            scratch = torch.zeros(1, dtype=torch.float32, device='cuda')
            ops.adam_keras_dev(sp.t, sm.t, sv.t, sg.t, it_dev, scratch, decay=decay, grad_scale=grad_scale, **hyper)
            torch.cuda.synchronize()
            assert int(it_dev.item()) == iteration + 1
            dev_lr_t = scratch.cpu().numpy()[0]
            # both sides are double arithmetic rounded once to float32: the same bits
            assert dev_lr_t.view(np.uint32) == lr_t.view(np.uint32), \
                'device lr_t %r != host lr_t %r at iteration %d, decay %g, %r' % (dev_lr_t, lr_t, iteration, decay, hyper)
        got = (sp.read(), sm.read(), sv.read())
        want, bound = adam_oracle(p, m, v, g, iteration, decay=decay, grad_scale=grad_scale, **hyper)
        names = ('p', 'm', 'v')
        zero = (g == 0) & (m == 0) & (v == 0)      # nothing to add: the weight keeps its bits
        assert np.array_equal(got[0][zero].view(np.uint32), p[zero].view(np.uint32))
    assert np.array_equal(sg.read().view(np.uint32), g.view(np.uint32)), 'the gradient was written'
    for name, a, w, b in zip(names, got, want, bound):
        r = worst_ratio(a, w, b, '%s %s' % (kernel, name))
        assert r <= 1.0, '%s %s: error / bound = %.3f (n %d, iteration %d, decay %g, grad_scale %g, %r)' % (
            kernel, name, r, p.size, iteration, decay, grad_scale, hyper)
        ratios[name] = r
    return ratios


def hypers_of(kernel):
    if kernel == 'sgd_keras':
        return [dict(lr=f32(0.01), momentum=f32(0.0)), dict(lr=f32(0.01), momentum=f32(0.9))]
    return [ADAM_DEFAULT, ADAM_OTHER]


def merge(worst, ratios):
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)


def report(what, worst):
    print('\nMEASURED %s: worst error/bound %s' % (what, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('kernel', KERNELS)
def test_every_size_on_odd_offset_slices_with_guards(ops, kernel):
    """Sizes 1 ... above the grid cap, state of a run in progress (iteration 7), decayed rate, grad_scale 0.5, both
    hyper-parameter sets: every element inside its bound, nothing outside the slice touched."""
    rng = np.random.default_rng(101)
    worst = {}
    for n in sizes():
        for hyper in hypers_of(kernel):
            state = optimizer_state(rng, n, 7, 1.0)
            ratios = run_step(ops, kernel, state, 7, hyper, f32(1e-3), 0.5)
            merge(worst, ratios)
    report('%s sizes' % kernel, worst)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('iteration', ITERATIONS)
def test_iterations_decay_grad_scale_and_gradient_scales(ops, kernel, iteration):
    """Zero moments (iteration 0) and later steps up to 10^6, decay 0 and 1e-3, grad_scale 1 and 0.5 (the data-parallel
    1 / world), default and non-default hyper-parameters (SGD: momentum 0 and 0.9), gradients of scale 1e-4, 1 and 1e3 with
    exact zeros and the cancelling b1 m ~ -(1 - b1) g mixed in; the written moments are compared as well as the weights."""
    rng = np.random.default_rng(202 + iteration % 1000)
    n = 20011
    worst = {}
    for g_scale in GRAD_SCALES:
        for decay in (0.0, f32(1e-3)):
            for grad_scale in (1.0, 0.5):
                for hyper in hypers_of(kernel):
                    state = optimizer_state(rng, n, iteration, g_scale)
                    ratios = run_step(ops, kernel, state, iteration, hyper, decay, grad_scale)
                    merge(worst, ratios)
    report('%s iteration %d' % (kernel, iteration), worst)


@pytest.mark.parametrize('kernel', KERNELS)
def test_fifty_steps_single_step_bounds_and_free_running_drift(ops, kernel):
    """The kernel carries its own state for 50 steps (device tensors, never re-uploaded); the oracle is re-seeded from that state
    before every step, so the single-step bounds apply at each one.  Beside it the free-running float64 trajectory: the kernel's
    distance to it after 50 steps has no derivable bound, so it is measured against the reference here -- torch_ref's float32 step
    runs the same 50 steps on the CPU, and the kernel may be 4 x as far from the float64 trajectory as that (a different but
    legal rounding order; a wrong formula drifts by orders of magnitude more)."""
    rng = np.random.default_rng(303)
    n, steps, decay = 20011, 50, f32(1e-3)
    sgd = kernel == 'sgd_keras'
    hyper = dict(lr=f32(0.01), momentum=f32(0.9)) if sgd else ADAM_DEFAULT
    p0 = rng.standard_normal(n).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (p0, np.zeros(n, np.float32), np.zeros(n, np.float32))]
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    pt, mt, vt = torch.from_numpy(p0.copy()), torch.zeros(n), torch.zeros(n)
    it_dev = torch.zeros(1, dtype=torch.int64, device='cuda')
    scratch = torch.zeros(1, dtype=torch.float32, device='cuda')
    worst = {}
    for it in range(steps):
        g = rng.standard_normal(n).astype(np.float32)
        g[it % 17::17] = 0
        before = [t.cpu().numpy().copy() for t in dev]
        gd = torch.from_numpy(g).cuda()
        if sgd:
            ops.sgd_keras(dev[0], dev[1], gd, it, decay=decay, **hyper)
            want, bound = sgd_oracle(before[0], before[1], g, it, hyper['lr'], hyper['momentum'], decay, 1.0)
            p64, m64 = np_ref.sgd_keras_step(p64, m64, g.astype(np.float64), it, decay=decay, **hyper)
            torch_ref.sgd_keras_step(pt, mt, torch.from_numpy(g), it, decay=decay, **hyper)
        else:
            if kernel == 'adam_keras':
                ops.adam_keras(dev[0], dev[1], dev[2], gd, it, decay=decay, **hyper)
            else:
                ops.adam_keras_dev(dev[0], dev[1], dev[2], gd, it_dev, scratch, decay=decay, **hyper)
            want, bound = adam_oracle(before[0], before[1], before[2], g, it, decay=decay, grad_scale=1.0, **hyper)
            p64, m64, v64 = np_ref.adam_keras_step(p64, m64, v64, g.astype(np.float64), it, decay=decay, **hyper)
            torch_ref.adam_keras_step(pt, mt, vt, torch.from_numpy(g), it, decay=decay, **hyper)
        torch.cuda.synchronize()
        for name, t, w, b in zip(('p', 'vel') if sgd else ('p', 'm', 'v'), dev, want, bound):
            r = worst_ratio(t.cpu().numpy(), w, b, '%s %s step %d' % (kernel, name, it))
            assert r <= 1.0, (kernel, name, it, r)
            merge(worst, {name: r})
    if kernel == 'adam_keras_dev':
        assert int(it_dev.item()) == steps
        assert scratch.cpu().numpy()[0].view(np.uint32) == adam_lr_t(hyper['lr'], hyper['beta_1'], hyper['beta_2'], decay,
                                                                       steps - 1).view(np.uint32)
    drift_kernel = float(np.abs(dev[0].cpu().numpy() - p64).max())
    drift_ref = float(np.abs(pt.numpy() - p64).max())
    report('%s 50 steps' % kernel, worst)
    print('MEASURED %s drift after 50 steps from the float64 trajectory: kernel %.3e, float32 restatement %.3e (bar 4 x = %.3e)'
          % (kernel, drift_kernel, drift_ref, 4 * drift_ref))
    assert float(np.abs(p64 - p0).max()) > 1e2 * drift_ref          # the run moved the weights far more than it drifted
    assert drift_kernel <= 4 * drift_ref


def test_empty_tensors_return_without_touching_anything(ops):
    """n == 0 (an empty slice has no address): every entry point returns, the buffer around the slice, the device step number and
    the lr_t scratch word keep their bits."""
    buf = torch.arange(16, dtype=torch.float32, device='cuda')
    keep = buf.clone()
    e = [buf[k:k] for k in (3, 5, 7, 9)]
    assert all(t.numel() == 0 for t in e)
    it_dev = torch.tensor([41], dtype=torch.int64, device='cuda')
    scratch = torch.full((1,), 0.375, dtype=torch.float32, device='cuda')
    ops.adam_keras(e[0], e[1], e[2], e[3], 5)
    ops.adam_keras_dev(e[0], e[1], e[2], e[3], it_dev, scratch)
    ops.sgd_keras(e[0], e[1], e[3], 5, momentum=0.9)
    ops.axpby(e[0], e[1], 2.0, 0.0)
    ops.axpby(e[0], e[0], 2.0, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and int(it_dev.item()) == 41 and float(scratch.item()) == 0.375


@pytest.mark.parametrize('a,b', [(1.0, 1.0), (2e-3, 1.0), (0.5, 0.0), (0.0, 0.125)])
def test_axpby_against_float64(ops, a, b):
    """y <- a x + b y: the l2 gradient (2e-3, 1), accumulation (1, 1), the loss tail (a, 0) and the in-place scaling (0, b with
    x is y) of training.py, on every size, odd-offset slices, guards intact."""
    rng = np.random.default_rng(404)
    a, b = f32(a), f32(b)
    worst = 0.0
    for n in sizes():
        x = rng.standard_normal(n).astype(np.float32)
        y = (1e2 * rng.standard_normal(n)).astype(np.float32)
        x[::17] = 0
        sx, sy = Slab(x, 1), Slab(y, 3)
        assert ops.axpby(sx.t, sy.t, a, b) is sy.t
        want, bound = axpby_oracle(x, y, a, b)
        worst = max(worst, worst_ratio(sy.read(), want, bound, 'axpby'))
        assert np.array_equal(sx.read().view(np.uint32), x.view(np.uint32))
        # x is y: y <- (a + b) y, evaluated as a y + b y
        sz = Slab(y, 5)
        ops.axpby(sz.t, sz.t, a, b)
        want, bound = axpby_oracle(y, y, a, b)
        worst = max(worst, worst_ratio(sz.read(), want, bound, 'axpby in place'))
    assert worst <= 1.0, worst
    print('\nMEASURED axpby a=%g b=%g: worst error/bound %.3f' % (a, b, worst))


def test_axpby_with_b_zero_overwrites_whatever_y_held(ops):
    """b == 0 must not multiply: a y full of NaN and Inf (uninitialised memory) gives the finite a x"""
    rng = np.random.default_rng(405)
    for n in (257, 200003):
        x = rng.standard_normal(n).astype(np.float32)
        y = np.full(n, np.nan, dtype=np.float32)
        y[1::3] = np.inf
        y[2::3] = -np.inf
        sx, sy = Slab(x, 1), Slab(y, 3)
        ops.axpby(sx.t, sy.t, 0.5, 0.0)
        got = sy.read()
        assert np.isfinite(got).all()
        want, bound = axpby_oracle(x, y, 0.5, 0.0)
        assert worst_ratio(got, want, bound, 'axpby b == 0') <= 1.0
        assert np.array_equal(got, np.float32(0.5) * x)            # a power of two: exact
