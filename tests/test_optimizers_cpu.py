"""The float64 oracles and the DERIVED single-step error bounds of the optimizer kernels (dlwp_adam_keras, dlwp_adam_keras_dev,
dlwp_sgd_keras, dlwp_axpby), shared with tests/test_gpu_optimizers.py, and their check without a GPU: a float32 numpy
restatement of each update -- every operation rounded once, no contraction -- must stay inside the bounds.

Conventions.  The C ABI receives float hyper-parameters, so every oracle takes them ROUNDED TO FLOAT32 FIRST (f32(0.999), not
0.999: 1 - beta_2 differs by 1.3e-5 relative between the two).  The step sizes lr_t (Adam) and lr' (SGD) are the float32
rounding of the double formula, as the host entry points compute them.  Every comparison starts the oracle from the kernel's own
float32 state, so a bound covers ONE step.  With u = 2^-24 (fused multiply-adds only remove roundings; division and square
root are correctly rounded: csrc/Makefile sets no fast-math flag):
    Adam  m:   |dm| <= 4u (|b1 m| + |(1-b1) g s|)                =: e_m
          v:   |dv| <= 4u v_new
          p:   |dp| <= u |p_new| + 8u |upd| + lr_t e_m / (sqrt(v_new) + eps),   upd = lr_t m_new / (sqrt(v_new) + eps)
    SGD   vel: |dvel| <= 3u (|mom vel| + |lr' g s|),   p: that + u |p_new|
    axpby y:   |dy| <= 2u (|a x| + |b y|)
(the e_m term of the Adam p bound matters where b1 m and (1-b1) g cancel: m_new is then small against its own error).  Where a
bound is exactly 0 the result must be exactly equal."""
import math

import numpy as np
import pytest

U = 2.0 ** -24

ITERATIONS = (0, 1, 7, 999, 10 ** 6)
GRAD_SCALES = (1e-4, 1.0, 1e3)


def f32(v):
    return float(np.float32(v))


def adam_lr_t(lr, beta_1, beta_2, decay, iteration):
    """float32 lr_t of dlwp_adam_keras: the double formula on the float hyper-parameters, rounded once"""
    t = float(iteration) + 1.0
    lr_ = lr / (1.0 + decay * float(iteration))
    return np.float32(lr_ * math.sqrt(1.0 - math.pow(beta_2, t)) / (1.0 - math.pow(beta_1, t)))


def sgd_lr(lr, decay, iteration):
    return np.float32(lr / (1.0 + decay * float(iteration)))


def adam_oracle(p, m, v, g, iteration, lr, beta_1, beta_2, epsilon, decay, grad_scale, lr_t=None):
    """float64 Adam step from float32 state; hyper-parameters already float32-rounded.  Returns ((p, m, v), (bound_p, bound_m,
    bound_v))."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    lr_t = float(adam_lr_t(lr, beta_1, beta_2, decay, iteration) if lr_t is None else lr_t)
    gs = g * grad_scale
    t1, t2 = beta_1 * m, (1.0 - beta_1) * gs
    m_new = t1 + t2
    e_m = 4 * U * (np.abs(t1) + np.abs(t2))
    v_new = beta_2 * v + (1.0 - beta_2) * gs * gs
    den = np.sqrt(v_new) + epsilon
    upd = lr_t * m_new / den
    p_new = p - upd
    e_p = U * np.abs(p_new) + 8 * U * np.abs(upd) + lr_t * e_m / den
    return (p_new, m_new, v_new), (e_p, e_m, 4 * U * v_new)


def sgd_oracle(p, vel, g, iteration, lr, momentum, decay, grad_scale):
    p, vel, g = (np.asarray(a, dtype=np.float64) for a in (p, vel, g))
    lr_ = float(sgd_lr(lr, decay, iteration))
    t1, t2 = momentum * vel, lr_ * g * grad_scale
    vel_new = t1 - t2
    e_v = 3 * U * (np.abs(t1) + np.abs(t2))
    p_new = p + vel_new
    return (p_new, vel_new), (e_v + U * np.abs(p_new), e_v)


def axpby_oracle(x, y, a, b):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if b == 0:      # y is overwritten, whatever it held
        return a * x, 2 * U * np.abs(a * x)
    return a * x + b * y, 2 * U * (np.abs(a * x) + np.abs(b * y))


def worst_ratio(got, want, bound, what=''):
    """max error / bound; a bound of exactly 0 demands exact equality"""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    zero = bound == 0
    assert np.all(err[zero] == 0), '%s: %d results differ where the bound is 0' % (what, int((err[zero] != 0).sum()))
    if zero.all():
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


def optimizer_state(rng, n, iteration, g_scale):
    """float32 (p, m, v, g) as a run could hold them before step `iteration`: zero moments at iteration 0; gradients of the given
    scale with exact zeros mixed in (every 17th; every 34th has zero moments as well -- the bound is 0 there); every 13th element
    has b1 m ~ -(1 - b1) g for beta_1 = 0.9: the cancelling case."""
    p = rng.standard_normal(n).astype(np.float32)
    g = (g_scale * rng.standard_normal(n)).astype(np.float32)
    if iteration == 0:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (0.3 * g_scale * rng.standard_normal(n)).astype(np.float32)
        v = ((g_scale * rng.standard_normal(n)) ** 2).astype(np.float32)
        m[::13] = (-(0.1 / 0.9) * g[::13].astype(np.float64) * (1 + 1e-6 * rng.standard_normal(g[::13].shape))).astype(np.float32)
    g[::17] = 0
    m[::34] = 0
    v[::34] = 0
    return p, m, v, g


def adam_f32(p, m, v, g, lr_t, b1, b2, eps, s):
    """the kernel's update, every operation rounded to float32 (numpy float32 arithmetic does not contract)"""
    b1, b2, eps, s, lr_t, one = (np.float32(a) for a in (b1, b2, eps, s, lr_t, 1))
    gi = g * s
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    return p - lr_t * mi / (np.sqrt(vi) + eps), mi, vi


def sgd_f32(p, vel, g, lr_, mom, s):
    lr_, mom, s = (np.float32(a) for a in (lr_, mom, s))
    vi = mom * vel - lr_ * (g * s)
    return p + vi, vi


@pytest.mark.parametrize('iteration', ITERATIONS)
def test_float32_restatements_stay_inside_the_derived_bounds(iteration):
    """The bounds test_gpu_optimizers.py holds the kernels to, checked against a float32 restatement that rounds after every
    operation: they hold (ratios below 1), and not by a wide margin -- the worst ratio over all cases is above 0.1, so a bound
    cannot hide an error ten times the rounding noise."""
    rng = np.random.default_rng(iteration % 1000 + 40)
    n = 200003
    worst = 0.0
    for g_scale in GRAD_SCALES:
        for decay, s in ((0.0, 1.0), (1e-3, 0.5)):
            for b1, b2, eps in ((0.9, 0.999, 1e-7), (0.8, 0.99, 1e-3)):
                b1, b2, eps, lr, dec = f32(b1), f32(b2), f32(eps), f32(1e-3), f32(decay)
                p, m, v, g = optimizer_state(rng, n, iteration, g_scale)
                lr_t = adam_lr_t(lr, b1, b2, dec, iteration)
                want, bound = adam_oracle(p, m, v, g, iteration, lr, b1, b2, eps, dec, s)
                for got, w, b, name in zip(adam_f32(p, m, v, g, lr_t, b1, b2, eps, s), want, bound, 'pmv'):
                    r = worst_ratio(got, w, b, 'adam %s' % name)
                    assert r <= 1.0, ('adam', name, iteration, g_scale, decay, s, b1, r)
                    worst = max(worst, r)
            for mom in (0.0, 0.9):
                mom, lr, dec = f32(mom), f32(0.01), f32(decay)
                p, vel, _, g = optimizer_state(rng, n, iteration, g_scale)
                want, bound = sgd_oracle(p, vel, g, iteration, lr, mom, dec, s)
                for got, w, b, name in zip(sgd_f32(p, vel, g, sgd_lr(lr, dec, iteration), mom, s), want, bound, ('p', 'vel')):
                    r = worst_ratio(got, w, b, 'sgd %s' % name)
                    assert r <= 1.0, ('sgd', name, iteration, g_scale, decay, s, mom, r)
                    worst = max(worst, r)
    assert worst > 0.1


def test_axpby_restatement_and_the_zero_bound_rule():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(200003).astype(np.float32)
    y = (1e2 * rng.standard_normal(200003)).astype(np.float32)
    for a, b in ((1.0, 1.0), (2e-3, 1.0), (0.5, 0.0), (0.0, 0.125)):
        a, b = f32(a), f32(b)
        got = np.float32(a) * x + np.float32(b) * y if b != 0 else np.float32(a) * x
        want, bound = axpby_oracle(x, y, a, b)
        assert worst_ratio(got, want, bound) <= 1.0
    want, bound = axpby_oracle(x, np.full_like(y, np.nan), f32(0.5), 0.0)
    assert np.isfinite(want).all() and np.isfinite(bound).all()
    # a bound of 0 means exact equality, and worst_ratio says so
    with pytest.raises(AssertionError):
        worst_ratio(np.array([1e-30]), np.zeros(1), np.zeros(1))
    assert worst_ratio(np.zeros(3), np.zeros(3), np.zeros(3)) == 0.0


def test_step_size_formulas():
    """lr_t and lr' on float32 hyper-parameters: bias correction 1 at a large step number, the decayed rate, float32 results"""
    lr, b1, b2 = f32(1e-3), f32(0.9), f32(0.999)
    assert adam_lr_t(lr, b1, b2, 0.0, 10 ** 6) == np.float32(lr)
    assert float(adam_lr_t(lr, b1, b2, 0.0, 0)) == pytest.approx(lr * math.sqrt(1 - b2) / (1 - b1), rel=1e-7)
    assert float(adam_lr_t(lr, b1, b2, f32(1e-3), 999)) == pytest.approx(
        float(adam_lr_t(lr, b1, b2, 0.0, 999)) / (1 + f32(1e-3) * 999), rel=2e-7)
    assert sgd_lr(f32(0.01), f32(1e-2), 4) == np.float32(f32(0.01) / (1 + 4 * f32(1e-2)))
    assert adam_lr_t(lr, b1, b2, 0.0, 7).dtype == np.float32 and sgd_lr(lr, 0.0, 7).dtype == np.float32
