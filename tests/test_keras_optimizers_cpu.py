"""The float64 oracles and the DERIVED single-step error bounds of dlwp_optimizer_step (every kind) and dlwp_grad_clip_factor, shared
with tests/test_gpu_keras_optimizers.py and tests/test_gpu_optimizer_models.py, and their check without a GPU: a float32 numpy
restatement of each update -- every operation rounded once, no contraction -- must stay inside the bounds.  Also the host side:
names, defaults, unknown keywords, the describe() round trip of every class.

Conventions (those of tests/test_optimizers_cpu.py).  Hyper-parameters reach the oracle ROUNDED TO FLOAT32; the step scalars
(lr', lr_t, Nadam's five) are the float32 roundings of the double formulas, as the host entry point evaluates them, and the oracle
uses those float32 values.  Every comparison starts from the kernel's own float32 state: a bound covers ONE step.  u = 2^-24;
fused multiply-adds only remove roundings; division and square root are correctly rounded.

The gradient the update sees is g^ = clamp(g * grad_scale * factor): r roundings (r = 1, or 2 with a clipnorm factor), so
|dg^| <= r u |g^| (the clamp is exact and 1-Lipschitz).  Each bound below counts the roundings on every term and adds ONE u of
slack per term for the second-order terms; e(x) is the bound of x, sq(x, e) = e / (2 sqrt(x)) + u sqrt(x) the bound of a square root
of a quantity known to e (0 at x = 0, where e is 0 too).
    SGD       t1 = mom m, t2 = lr' g^:  e(v) = 3u |t1| + (r + 3) u |t2|;                     e(p) = e(v) + u |p_new|
    nesterov  q = mom v_new - t2:       e(q) = |mom| e(v) + 3u |mom v_new| + (r + 3) u |t2|;  e(p) = e(q) + u |p_new|
    RMSprop   a_new = t1 + t2, t1 = rho a, t2 = (1 - rho) g^2:   e(a) = 3u t1 + (2r + 5) u t2
              den = sqrt(a_new) + eps:  e(den) = sq(a_new, e(a)) + u den
              upd = lr' g^ / den:       e(upd) = |upd| ((r + 3) u + e(den) / den);           e(p) = e(upd) + u |p_new|
    Adagrad   the same with t1 = a:     e(a) = 2u a + (2r + 3) u g^2
    Adadelta  a_new as RMSprop; num = sqrt(d + eps): e(num) = 2u num; den = sqrt(a_new + eps): e(den) = sq(a_new + eps, e(a) +
              u (a_new + eps)); upd = g^ num / den: e(upd) = |upd| ((r + 3) u + e(num) / num + e(den) / den);
              e(p) = lr' e(upd) + u |lr' upd| + u |p_new|;  d_new = rho d + (1 - rho) upd^2:
              e(d) = 3u rho d + 5u (1 - rho) upd^2 + 2 (1 - rho) |upd| e(upd)
    Adam      m: e(m) = 3u |b1 m| + (r + 4) u |(1 - b1) g^|;  v: e(v) = 3u b2 v + (2r + 5) u (1 - b2) g^2
              den = sqrt(v_new) + eps as RMSprop; upd = lr_t m_new / den:
              e(upd) = lr_t e(m) / den + |upd| (3u + e(den) / den);                          e(p) = e(upd) + u |p_new|
    amsgrad   vhat_new = max(vhat, v_new): e(vhat) = e(v) (max is 1-Lipschitz); den from vhat_new
    Adamax    u_new = max(b2 u, |g^|): e(u) = max(2u b2 u, (r + 1) u |g^|); den = u_new + eps: e(den) = e(u) + u den; upd as Adam
    Nadam     A = c2 g^ / c0, B = c3 m_new / c1, v' = v_new / c4 (c0 = 1 - ms_new, c1 = 1 - ms_next, c2 = 1 - mu_t, c3 = mu_t1,
              c4 = 1 - b2^t):  e(A) = (r + 3) u |A|, e(B) = c3 e(m) / c1 + 3u |B|, e(v') = e(v) / c4 + 2u v',
              den = sqrt(v') + eps, e(num) = e(A) + e(B) + u (|A| + |B|),
              e(upd) = lr e(num) / den + lr (|A| + |B|) / den (3u + e(den) / den);          e(p) = e(upd) + u |p_new|
    clip      the sum of squares is taken in double on exact products: its error is far below the one float32 rounding of the
              results.  e(norm) = u norm; e(factor) = 2u factor where the norm clips, else the factor is exactly 1.
Where a bound is exactly 0 the result must be exactly equal (worst_ratio)."""
import math

import numpy as np
import pytest

from tests.test_optimizers_cpu import GRAD_SCALES, ITERATIONS, U, adam_lr_t, f32, optimizer_state, sgd_lr, worst_ratio

KINDS = ('sgd', 'nesterov', 'rmsprop', 'adagrad', 'adadelta', 'adam', 'amsgrad', 'adamax', 'nadam')
CODE = {k: i for i, k in enumerate(KINDS)}                  # DLWP_OPT_* of include/dlwp_hip.h
N_SLOTS = dict(sgd=1, nesterov=1, rmsprop=1, adagrad=1, adadelta=2, adam=2, amsgrad=3, adamax=2, nadam=2)
NAMES = dict(sgd=('p', 'm'), nesterov=('p', 'm'), rmsprop=('p', 'a'), adagrad=('p', 'a'), adadelta=('p', 'a', 'd'),
             adam=('p', 'm', 'v'), amsgrad=('p', 'm', 'v', 'vhat'), adamax=('p', 'm', 'u'), nadam=('p', 'm', 'v'))


def hypers_of(kind):
    """two hyper-parameter sets per kind (Keras' defaults first), float32-rounded: the keywords of ops.optimizer_step"""
    r = lambda **kw: {k: f32(v) for k, v in kw.items()}  # noqa: E731
    return {'sgd': [r(lr=0.01, h1=0.9), r(lr=0.02, h1=0.0)],
            'nesterov': [r(lr=0.01, h1=0.9), r(lr=0.02, h1=0.5)],
            'rmsprop': [r(lr=0.001, h1=0.9, epsilon=1e-7), r(lr=0.002, h1=0.99, epsilon=1e-3)],
            'adagrad': [r(lr=0.01, epsilon=1e-7), r(lr=0.02, epsilon=1e-3)],
            'adadelta': [r(lr=1.0, h1=0.95, epsilon=1e-7), r(lr=0.5, h1=0.9, epsilon=1e-3)],
            'adam': [r(lr=0.001, h1=0.9, h2=0.999, epsilon=1e-7), r(lr=0.002, h1=0.8, h2=0.99, epsilon=1e-3)],
            'amsgrad': [r(lr=0.001, h1=0.9, h2=0.999, epsilon=1e-7), r(lr=0.002, h1=0.8, h2=0.99, epsilon=1e-3)],
            'adamax': [r(lr=0.002, h1=0.9, h2=0.999, epsilon=1e-7), r(lr=0.001, h1=0.8, h2=0.99, epsilon=1e-3)],
            'nadam': [r(lr=0.002, h1=0.9, h2=0.999, epsilon=1e-7, schedule_decay=0.004),
                      r(lr=0.001, h1=0.8, h2=0.99, epsilon=1e-3, schedule_decay=0.01)]}[kind]


def nadam_m_schedule(h1, sd, iteration):
    """the running product mu_1 ... mu_it a run holds before step `iteration` (double, float32-rounded hyper-parameters)"""
    ms = 1.0
    for it in range(min(iteration, 5000)):          # (0.9^5000 has long underflowed to 0)
        ms *= h1 * (1.0 - 0.5 * math.pow(0.96, (it + 1.0) * sd))
    return ms if iteration <= 5000 else 0.0


def step_scalars(kind, hyper, decay, iteration, m_schedule=1.0):
    """float32 launch scalars of dlwp_optimizer_step: double formulas on the float32 hyper-parameters, rounded once"""
    lr, h1, h2 = hyper['lr'], hyper.get('h1', 0.0), hyper.get('h2', 0.0)
    t = float(iteration) + 1.0
    s = {'lr': sgd_lr(lr, decay, iteration)}
    if kind in ('adam', 'amsgrad'):
        s['lr'] = adam_lr_t(lr, h1, h2, decay, iteration)
    elif kind == 'adamax':
        s['lr'] = np.float32(lr / (1.0 + decay * float(iteration)) / (1.0 - math.pow(h1, t)))
    elif kind == 'nadam':
        sd = hyper['schedule_decay']
        mu_t = h1 * (1.0 - 0.5 * math.pow(0.96, t * sd))
        mu_t1 = h1 * (1.0 - 0.5 * math.pow(0.96, (t + 1.0) * sd))
        ms_new = m_schedule * mu_t
        ms_next = ms_new * mu_t1
        s.update(lr=np.float32(lr), c0=np.float32(1.0 - ms_new), c1=np.float32(1.0 - ms_next), c2=np.float32(1.0 - mu_t),
                 c3=np.float32(mu_t1), c4=np.float32(1.0 - math.pow(h2, t)))
    return s


def seen_gradient(g, grad_scale, clipvalue=0.0, factor=None):
    """float64 gradient the update sees and the number of float32 roundings the kernel spends on it"""
    gh = np.asarray(g, dtype=np.float64) * grad_scale
    r = 1
    if factor is not None:
        gh = gh * float(factor)
        r = 2
    if clipvalue > 0:
        gh = np.clip(gh, -clipvalue, clipvalue)
    return gh, r


def _sq(x, e):
    s = np.sqrt(x)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > 0, e / (2 * s), 0.0) + U * s


def oracle(kind, p, slots, g, sc, hyper, grad_scale=1.0, clipvalue=0.0, factor=None):
    """One float64 step of `kind` from float32 state.  sc: step_scalars(...).  Returns ([p_new, slot_new ...], [bounds ...])."""
    p = np.asarray(p, dtype=np.float64)
    s = [np.asarray(a, dtype=np.float64) for a in slots]
    gh, r = seen_gradient(g, grad_scale, clipvalue, factor)
    lr = float(sc['lr'])
    h1, h2, eps = hyper.get('h1', 0.0), hyper.get('h2', 0.0), hyper.get('epsilon', 0.0)
    ag = np.abs(gh)
    if kind in ('sgd', 'nesterov'):
        t1, t2 = h1 * s[0], lr * gh
        v = t1 - t2
        e_v = 3 * U * np.abs(t1) + (r + 3) * U * np.abs(t2)
        if kind == 'sgd':
            p_new = p + v
            return [p_new, v], [e_v + U * np.abs(p_new), e_v]
        q = h1 * v - t2
        p_new = p + q
        e_q = abs(h1) * e_v + 3 * U * np.abs(h1 * v) + (r + 3) * U * np.abs(t2)
        return [p_new, v], [e_q + U * np.abs(p_new), e_v]
    if kind in ('rmsprop', 'adagrad', 'adadelta'):
        if kind == 'adagrad':
            t1, t2 = s[0], gh * gh
            e_a = 2 * U * t1 + (2 * r + 3) * U * t2
        else:
            t1, t2 = h1 * s[0], (1.0 - h1) * gh * gh
            e_a = 3 * U * t1 + (2 * r + 5) * U * t2
        a_new = t1 + t2
        if kind != 'adadelta':
            den = np.sqrt(a_new) + eps
            e_den = _sq(a_new, e_a) + U * den
            upd = lr * gh / den
            e_upd = np.abs(upd) * ((r + 3) * U + e_den / den)
            p_new = p - upd
            return [p_new, a_new], [e_upd + U * np.abs(p_new), e_a]
        num = np.sqrt(s[1] + eps)
        den = np.sqrt(a_new + eps)
        e_den = _sq(a_new + eps, e_a + U * (a_new + eps))
        upd = gh * num / den
        e_upd = np.abs(upd) * ((r + 3) * U + 2 * U + e_den / den)
        p_new = p - lr * upd
        d_new = h1 * s[1] + (1.0 - h1) * upd * upd
        e_d = 3 * U * h1 * s[1] + 5 * U * (1.0 - h1) * upd * upd + 2 * (1.0 - h1) * np.abs(upd) * e_upd
        return [p_new, a_new, d_new], [lr * e_upd + U * np.abs(lr * upd) + U * np.abs(p_new), e_a, e_d]
    # the Adam family
    t1, t2 = h1 * s[0], (1.0 - h1) * gh
    m_new = t1 + t2
    e_m = 3 * U * np.abs(t1) + (r + 4) * U * np.abs(t2)
    if kind == 'adamax':
        u_new = np.maximum(h2 * s[1], ag)
        e_u = np.maximum(2 * U * h2 * s[1], (r + 1) * U * ag)
        den = u_new + eps
        e_den = e_u + U * den
        upd = lr * m_new / den
        e_upd = lr * e_m / den + np.abs(upd) * (3 * U + e_den / den)
        p_new = p - upd
        return [p_new, m_new, u_new], [e_upd + U * np.abs(p_new), e_m, e_u]
    v1, v2 = h2 * s[1], (1.0 - h2) * gh * gh
    v_new = v1 + v2
    e_v = 3 * U * v1 + (2 * r + 5) * U * v2
    if kind in ('adam', 'amsgrad'):
        d, e_dd = v_new, e_v
        if kind == 'amsgrad':
            d = np.maximum(s[2], v_new)
        den = np.sqrt(d) + eps
        e_den = _sq(d, e_dd) + U * den
        upd = lr * m_new / den
        e_upd = lr * e_m / den + np.abs(upd) * (3 * U + e_den / den)
        p_new = p - upd
        if kind == 'adam':
            return [p_new, m_new, v_new], [e_upd + U * np.abs(p_new), e_m, e_v]
        return [p_new, m_new, v_new, d], [e_upd + U * np.abs(p_new), e_m, e_v, e_v]
    c0, c1, c2, c3, c4 = (float(sc[k]) for k in ('c0', 'c1', 'c2', 'c3', 'c4'))
    A = c2 * gh / c0
    B = c3 * m_new / c1
    vp = v_new / c4
    e_vp = e_v / c4 + 2 * U * vp
    den = np.sqrt(vp) + eps
    e_den = _sq(vp, e_vp) + U * den
    absn = np.abs(A) + np.abs(B)
    e_num = (r + 3) * U * np.abs(A) + c3 * e_m / c1 + 3 * U * np.abs(B) + U * absn
    upd = lr * (A + B) / den
    e_upd = lr * e_num / den + lr * absn / den * (3 * U + e_den / den)
    p_new = p - upd
    return [p_new, m_new, v_new], [e_upd + U * np.abs(p_new), e_m, e_v]


def step_f32(kind, p, slots, g, sc, hyper, grad_scale=1.0, clipvalue=0.0, factor=None):
    """the kernel's update with every operation rounded to float32 (numpy float32 arithmetic does not contract)"""
    one = np.float32(1)
    h1, h2, eps = (np.float32(hyper.get(k, 0.0)) for k in ('h1', 'h2', 'epsilon'))
    lr = np.float32(sc['lr'])
    gi = g * np.float32(grad_scale)
    if factor is not None:
        gi = gi * np.float32(factor)
    if clipvalue > 0:
        gi = np.minimum(np.maximum(gi, np.float32(-clipvalue)), np.float32(clipvalue))
    s = list(slots)
    if kind == 'sgd':
        v = h1 * s[0] - lr * gi
        return [p + v, v]
    if kind == 'nesterov':
        t2 = lr * gi
        v = h1 * s[0] - t2
        return [p + (h1 * v - t2), v]
    if kind == 'rmsprop':
        a = h1 * s[0] + (one - h1) * gi * gi
        return [p - lr * gi / (np.sqrt(a) + eps), a]
    if kind == 'adagrad':
        a = s[0] + gi * gi
        return [p - lr * gi / (np.sqrt(a) + eps), a]
    if kind == 'adadelta':
        a = h1 * s[0] + (one - h1) * gi * gi
        upd = gi * np.sqrt(s[1] + eps) / np.sqrt(a + eps)
        return [p - lr * upd, a, h1 * s[1] + (one - h1) * upd * upd]
    m = h1 * s[0] + (one - h1) * gi
    if kind == 'adamax':
        un = np.maximum(h2 * s[1], np.abs(gi))
        return [p - lr * m / (un + eps), m, un]
    v = h2 * s[1] + (one - h2) * gi * gi
    if kind == 'adam':
        return [p - lr * m / (np.sqrt(v) + eps), m, v]
    if kind == 'amsgrad':
        d = np.maximum(s[2], v)
        return [p - lr * m / (np.sqrt(d) + eps), m, v, d]
    c0, c1, c2, c3, c4 = (np.float32(sc[k]) for k in ('c0', 'c1', 'c2', 'c3', 'c4'))
    return [p - lr * (c2 * (gi / c0) + c3 * (m / c1)) / (np.sqrt(v / c4) + eps), m, v]


def kind_state(rng, kind, n, iteration, g_scale):
    """float32 (p, slots, g) of `kind` as a run could hold them before step `iteration`, from optimizer_state: exact-zero gradients,
    elements whose slots are all zero, and b1 m ~ -(1 - b1) g cancellations mixed in"""
    p, m, v, g = optimizer_state(rng, n, iteration, g_scale)
    if kind in ('sgd', 'nesterov'):
        slots = [m]
    elif kind in ('rmsprop', 'adagrad'):
        slots = [v]
    elif kind == 'adadelta':
        slots = [v, (v * np.float32(1e-4) * rng.uniform(0.5, 2.0, n).astype(np.float32))]
    elif kind == 'amsgrad':          # vhat above and below the new v
        slots = [m, v, v * rng.uniform(0.5, 1.5, n).astype(np.float32)]
    elif kind == 'adamax':
        slots = [m, np.sqrt(v) * rng.uniform(0.5, 1.5, n).astype(np.float32)]
    else:
        slots = [m, v]
    return p, [np.ascontiguousarray(a, dtype=np.float32) for a in slots], g


def clip_oracle(g, grad_scale, clipnorm):
    """float64 (factor, norm, norm^2) of Keras' clip_norm on g * grad_scale, and their bounds"""
    gs = np.asarray(g, dtype=np.float64) * float(grad_scale)
    ss = float(np.sum(gs * gs))
    norm = math.sqrt(ss)
    clips = clipnorm > 0 and norm >= clipnorm
    factor = clipnorm / norm if clips else 1.0
    return (factor, norm, ss), (2 * U * factor if clips else 0.0, U * norm, U * ss)


def clip_cases():
    """(iteration-independent) clipping variants of a step: (clipvalue in units of the gradient scale, factor or None)"""
    return [(0.0, None), (0.5, None), (0.0, np.float32(0.3173)), (0.7, np.float32(0.3173))]


def check_case(kind, rng, n, iteration, g_scale, hyper, decay, grad_scale, clipvalue, factor, step):
    """runs `step` (same signature as step_f32) on a fresh state; returns {name: worst error / bound}"""
    p, slots, g = kind_state(rng, kind, n, iteration, g_scale)
    ms = nadam_m_schedule(hyper['h1'], hyper['schedule_decay'], iteration) if kind == 'nadam' else 1.0
    sc = step_scalars(kind, hyper, 0.0 if kind == 'nadam' else decay, iteration, ms)
    cv = f32(clipvalue * g_scale * grad_scale)
    want, bound = oracle(kind, p, slots, g, sc, hyper, grad_scale, cv, factor)
    got = step(kind, p, slots, g, sc, hyper, grad_scale, cv, factor)
    out = {}
    for name, a, w, b in zip(NAMES[kind], got, want, bound):
        r = worst_ratio(a, w, b, '%s %s' % (kind, name))
        assert r <= 1.0, (kind, name, iteration, g_scale, decay, grad_scale, clipvalue, factor, hyper, r)
        out[name] = r
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_float32_restatements_stay_inside_the_derived_bounds(kind):
    """Every kind at iterations 0 ... 10^6, gradient scales 1e-4 ... 1e3, decay and grad_scale, both hyper-parameter sets, with and
    without a clipnorm factor and a clipvalue: the float32 restatement holds every bound (ratio <= 1), and the worst ratio is above
    0.1 -- no bound hides ten times the rounding noise."""
    worst = {}
    for iteration in ITERATIONS:
        rng = np.random.default_rng(iteration % 1000 + 11 * CODE[kind])
        for g_scale in GRAD_SCALES:
            for decay, s in ((0.0, 1.0), (f32(1e-3), 0.5)):
                for hyper in hypers_of(kind):
                    for clipvalue, factor in clip_cases():
                        for k, r in check_case(kind, rng, 20011, iteration, g_scale, hyper, decay, s, clipvalue, factor,
                                               step_f32).items():
                            worst[k] = max(worst.get(k, 0.0), r)
    print('\nMEASURED float32 restatement of %s: worst error/bound %s' % (kind, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) > 0.1, worst


@pytest.mark.parametrize('kind', KINDS)
def test_zero_gradient_and_zero_slots_keep_the_weights(kind):
    """g = 0 with zero slots: the oracle moves nothing, the slot bounds are exactly 0, and the restatement keeps p's bits"""
    rng = np.random.default_rng(5)
    p = rng.standard_normal(1000).astype(np.float32)
    z = np.zeros(1000, np.float32)
    for hyper in hypers_of(kind):
        sc = step_scalars(kind, hyper, 0.0, 3, 0.7)
        slots = [z.copy() for _ in range(N_SLOTS[kind])]
        want, bound = oracle(kind, p, slots, z, sc, hyper)
        got = step_f32(kind, p, slots, z, sc, hyper)
        assert np.array_equal(got[0].view(np.uint32), p.view(np.uint32)) and np.array_equal(want[0], p.astype(np.float64))
        for w, b, a in zip(want[1:], bound[1:], got[1:]):
            assert not w.any() and not b.any() and not a.any()


def test_clipping_oracle_and_the_seen_gradient():
    rng = np.random.default_rng(8)
    g = rng.standard_normal(20011).astype(np.float32)
    (factor, norm, ss), (e_f, e_n, _) = clip_oracle(g, 0.5, 1.0)
    assert norm == pytest.approx(0.5 * math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))) and factor == pytest.approx(1.0 / norm)
    assert e_f > 0 and e_n > 0
    # below the threshold nothing is touched: the factor is exactly 1 and its bound 0
    (factor, _, _), (e_f, _, _) = clip_oracle(g, 0.5, 2.0 * norm)
    assert factor == 1.0 and e_f == 0.0
    # the branch is n >= c: (3, 4) at clipnorm 5 is "clipped" by exactly 1
    (factor, norm, ss), _ = clip_oracle(np.array([3, 4], np.float32), 1.0, 5.0)
    assert (factor, norm, ss) == (1.0, 5.0, 25.0)
    # a float32 pairwise sum of squares, rounded once at the end, sits inside the norm's bound
    (_, norm, _), (_, e_n, _) = clip_oracle(g, 1.0, 1.0)
    assert abs(float(np.float32(math.sqrt(float(np.sum(g.astype(np.float64) ** 2))))) - norm) <= e_n
    # norm first, clamp afterwards
    gh, r = seen_gradient(np.array([3.0, -4.0, 0.25], np.float32), 2.0, clipvalue=0.5, factor=np.float32(0.125))
    assert r == 2 and np.array_equal(gh, [0.5, -0.5, 0.0625])
    gh, r = seen_gradient(np.array([3.0], np.float32), 0.5)
    assert r == 1 and gh[0] == 1.5


def test_step_scalars_are_float32_roundings_of_the_double_formulas():
    h = hypers_of('nadam')[0]
    sc = step_scalars('nadam', h, 0.0, 0)
    mu1 = h['h1'] * (1 - 0.5 * 0.96 ** h['schedule_decay'])
    assert sc['c2'] == np.float32(1 - mu1) and sc['c0'] == np.float32(1 - mu1) and sc['lr'] == np.float32(h['lr'])
    assert all(v.dtype == np.float32 for v in sc.values())
    assert nadam_m_schedule(h['h1'], h['schedule_decay'], 0) == 1.0 and nadam_m_schedule(h['h1'], h['schedule_decay'], 1) == mu1
    assert nadam_m_schedule(h['h1'], h['schedule_decay'], 10 ** 6) == 0.0
    a = hypers_of('adamax')[0]
    assert step_scalars('adamax', a, 0.0, 0)['lr'] == np.float32(a['lr'] / (1 - a['h1']))
    assert step_scalars('adamax', a, 0.0, 10 ** 6)['lr'] == np.float32(a['lr'])
    assert step_scalars('rmsprop', hypers_of('rmsprop')[0], f32(1e-2), 4)['lr'] == np.float32(f32(0.001) / (1 + 4 * f32(1e-2)))
    # the trainer's own schedule (training.nadam_schedule) is the same arithmetic
    from dlwp_amd.training import Nadam, nadam_schedule
    opt = Nadam()
    ms = 1.0
    for it in range(5):
        mu_t, mu_t1, ms_new, ms_next = nadam_schedule(opt.beta_1, opt.schedule_decay, it, ms)
        sc = step_scalars('nadam', hypers_of('nadam')[0], 0.0, it, ms)
        assert sc['c0'] == np.float32(1 - ms_new) and sc['c1'] == np.float32(1 - ms_next) and sc['c3'] == np.float32(mu_t1)
        opt.after_step()
        ms = ms_new
        assert opt.m_schedule == ms and opt.iterations == it + 1


# ---- the host side: names, defaults, keywords, describe() ------------------------------------------------------------------- #

DEFAULTS = {'SGD': dict(lr=0.01, momentum=0.0, decay=0.0, nesterov=False),
            'RMSprop': dict(lr=0.001, rho=0.9, epsilon=1e-7, decay=0.0),
            'Adagrad': dict(lr=0.01, epsilon=1e-7, decay=0.0),
            'Adadelta': dict(lr=1.0, rho=0.95, epsilon=1e-7, decay=0.0),
            'Adam': dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0, amsgrad=False),
            'Adamax': dict(lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0),
            'Nadam': dict(lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule_decay=0.004)}


def test_all_seven_keras_names_resolve_case_insensitively_with_keras_defaults():
    from dlwp_amd import training
    for name, want in DEFAULTS.items():
        for spelled in (name, name.lower(), name.upper()):
            opt = training.get_optimizer(spelled)
            assert type(opt) is getattr(training, name) and opt.iterations == 0
            for k, v in want.items():
                assert getattr(opt, k) == v and type(getattr(opt, k)) is type(v), (name, k)
        assert not hasattr(opt, 'clipnorm') and not hasattr(opt, 'clipvalue') and opt.clips() == (0.0, 0.0)
    assert training.get_optimizer('nadam').m_schedule == 1.0
    with pytest.raises(ValueError):
        training.get_optimizer('lion')
    inst = training.Adagrad(lr=0.5)
    assert training.get_optimizer(inst) is inst


def test_slot_counts_kinds_and_which_optimizers_keep_the_old_kernels():
    from dlwp_amd import ops, training as T
    want = [(T.SGD(), 'sgd', True), (T.SGD(nesterov=True), 'nesterov', False), (T.SGD(clipvalue=1.0), 'sgd', False),
            (T.RMSprop(), 'rmsprop', False), (T.Adagrad(), 'adagrad', False), (T.Adadelta(), 'adadelta', False),
            (T.Adam(), 'adam', True), (T.Adam(clipnorm=1.0), 'adam', False), (T.Adam(amsgrad=True), 'amsgrad', False),
            (T.Adamax(), 'adamax', False), (T.Nadam(), 'nadam', False)]
    for opt, kind, legacy in want:
        assert opt.step_kind() == CODE[kind] and opt.n_slots() == N_SLOTS[kind] == ops.OPT_SLOTS[CODE[kind]]
        assert opt.legacy_kernel() is legacy
    # launch arguments that change with the step number keep a step eager
    assert [o.step_depends_on_iteration() for o, _, _ in want] == [False, False, False, False, False, False, True, True, True,
                                                                    True, True]
    assert T.RMSprop(decay=1e-3).step_depends_on_iteration() and T.SGD(nesterov=True, decay=1e-3).step_depends_on_iteration()


def test_clip_keywords_are_kept_and_unknown_keywords_raise():
    from dlwp_amd import training as T
    for cls in (T.SGD, T.RMSprop, T.Adagrad, T.Adadelta, T.Adam, T.Adamax, T.Nadam):
        opt = cls(clipnorm=1.5, clipvalue=0.25)
        assert opt.clipnorm == 1.5 and opt.clipvalue == 0.25 and opt.clips() == (1.5, 0.25)
        assert cls(clipnorm=0.0).clips() == (0.0, 0.0)              # Keras clips only where the value is positive
        with pytest.raises(TypeError, match='clipnrom'):
            cls(clipnrom=1.0)
        with pytest.raises(TypeError):
            cls(lr=0.1, momentum_schedule=3)
    with pytest.raises(TypeError):
        T.Nadam(decay=1e-3)                                         # Keras' Nadam has schedule_decay, not decay


def test_keras_optimizers_module_exports_every_class():
    from dlwp_amd import compat, training
    import sys
    saved = {k: v for k, v in sys.modules.items() if k == 'keras' or k.startswith('keras.') or k == 'DLWP' or k.startswith('DLWP.')}
    try:
        compat.install()
        import keras.optimizers as ko
        for name in DEFAULTS:
            assert getattr(ko, name) is getattr(training, name)
    finally:
        for k in [k for k in sys.modules if k == 'keras' or k.startswith('keras.') or k == 'DLWP' or k.startswith('DLWP.')]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize('name', sorted(DEFAULTS))
def test_describe_round_trip_rebuilds_the_class_with_its_state(name):
    """serialization.describe()'s optimizer entry -> the constructor (as load_model_file and the driver-mode workers do): every
    hyper-parameter, the booleans, the clip arguments, iterations and Nadam's m_schedule survive; pickling (the worker
    specification of driver mode) too."""
    import json
    import pickle
    from dlwp_amd import training as T
    other = {'SGD': dict(lr=0.05, momentum=0.8, decay=1e-3, nesterov=True), 'RMSprop': dict(lr=0.01, rho=0.8, epsilon=1e-5),
             'Adagrad': dict(lr=0.02, decay=1e-4), 'Adadelta': dict(rho=0.9, epsilon=1e-4), 'Adam': dict(amsgrad=True, beta_1=0.85),
             'Adamax': dict(beta_2=0.99), 'Nadam': dict(schedule_decay=0.01)}[name]
    opt = getattr(T, name)(clipnorm=2.0, clipvalue=0.5, **other)
    for _ in range(3):
        opt.after_step()
    cfg = {k: v for k, v in vars(opt).items() if isinstance(v, (int, float))}          # what describe() stores
    cfg = json.loads(json.dumps(cfg))
    iters = cfg.pop('iterations')
    ms = cfg.pop('m_schedule', None)
    again = getattr(T, name)(**cfg)
    again.iterations = iters
    if ms is not None:
        again.m_schedule = ms
    assert vars(again) == vars(opt) and again.iterations == 3
    assert all(type(getattr(again, k)) is type(v) for k, v in vars(opt).items())
    if name == 'Nadam':
        assert 0 < again.m_schedule < 1
    assert vars(pickle.loads(pickle.dumps(opt))) == vars(opt)
