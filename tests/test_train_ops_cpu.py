"""The float64 oracles' DERIVED error bounds for the helper kernels of the training step (dlwp_amd/csrc/train_ops.hip: dlwp_act_bwd,
dlwp_bias_grad, dlwp_act_bwd_bias_grad, dlwp_pool_act_bwd_bias_grad, dlwp_mse_mae, dlwp_mse_mae_phase, dlwp_loss_custom), shared
with tests/test_gpu_train_ops.py, and their checks without a GPU: the closed-form gradient of np_ref.custom_loss against torch
float64 autograd, its values against every scalar of tests/golden/losses.npz, the exactness condition of every family (a) case, and
a float32 restatement of every kernel -- each operation rounded once, sums taken in the kernel's order -- inside every bound.

Two input families.
 (a) EXACT: small integers (a few +-2), row weights 1/2 and 1, a climatology of multiples of 1/4.  Every product is exact and every
     partial sum is an integer multiple of one power of two (the `unit`), so a float32 sum is exact IN ANY ORDER while the sum of the
     terms' absolute values stays below 2^24 units (exact_condition, asserted for every generated case).  The kernels' sums must
     then equal the float64 sums to the bit; a dropped, doubled or mis-sliced element is an integer error.  Large tensors are made
     sparse (density) so that the condition holds.  What follows an exact sum is one scaling s * (1 / n): two roundings, 2 u.
 (b) REAL: random floats.  u = 2^-24; csrc/Makefile sets no fast-math flag, so division and square root are correctly rounded and
     a fused multiply-add only removes a rounding: every bound below holds with and without contraction.
     Elementwise.  relu / linear backward: no rounding, bound 0 (bit equality).  tanh backward g (1 - t t):
         fl(t t): u t^2;  1 - that: u |1 - t^2|;  the product: u |g| |1 - t^2|   ->   |g| (2 |1 - t^2| + t^2) u.
       mse_mae dy = fl(fl(2 lw inv_n) fl(yp - yt)): inv_n, the scale, d, the product -> 4 u |dy|  (the phase form: the same count).
       loss_grad_kernel, from the kernel's own float32 sums:  eP = u (|w yp| + |P|) for P = fl(fl(w yp) - m) (eT likewise),
         A = T - r P, r = fl(S_pt / S_pp):  eA = eT + |r| eP + 2 u |r P| + u |A|;  g1 = -A fl(1 / sqrt(fl(S_pp S_tt))):
         e1 = eA / sqrt(S_pp S_tt) + 4 u |g1|;  the regulariser's term t2 has 4 (mse: d, w d, inv_n, product), 1 (mae: inv_n),
         1 (global: 1 / St) or 2 (spatial: St planes, 1 / that) roundings, the sum one more: eg = e1 + c u |t2| + u |g|;
         dy = fl(fl(lw w) g):  |lw w| eg + 2 u |dy|.   kind 0: d, w d, inv_n, the product, lw w, the product: 6 u |dy|.
     Sums.  |error| <= (k + c) u sum |term|: k additions on the longest path of the kernel's fixed tree, c roundings inside a term.
       k = per-thread trip count + 6 shuffle steps (wave_sum, train_ops.hip:18) + 3 additions over the 4 waves (block_sum2,
       train_ops.hip:31-32) + the final stage, counted per kernel in the k_* functions below with the lines they restate.
       The bias gradients are compared with the float64 sum of the kernel's OWN float32 dz: c = 0.
     Loss value (kind 1), first order in the sums' errors e_pt, e_pp, e_tt:  a = S_pt / sqrt(S_pp S_tt),
         e_a = e_pt / sqrt(S_pp S_tt) + |a| (e_pp / (2 S_pp) + e_tt / (2 S_tt)) + 3 u |a|,   e_loss = e_reg + e_a + u |loss|.
     Second order: every relative first-order term here is below 2^-16 (k + c < 256), so the neglected products are below 2^-16 of
     the first-order bound: every bound is multiplied by SECOND = 1 + 2^-15.
The line numbers beside the kernel names below (train_ops.hip, batch.hip: both in dlwp_amd/csrc) are those of the commit that added
this file; the kernel names are what to look for after an edit.
Nothing here is tuned to what the kernels deliver; tests/test_gpu_train_ops.py prints the measured error / bound ratios."""
import math

import numpy as np
import pytest

from oracle import np_ref
from tests.test_optimizers_cpu import U, f32, worst_ratio

SECOND = 1.0 + 2.0 ** -15
CU = 256                       # compute units of an MI355X: grid_for caps a flat launch at 8 * CU blocks
BIAS_SPLIT = 64                # train_ops.hip:52
BLOCK_ADDS = 6 + 3             # wave_sum (train_ops.hip:18) + block_sum2's (sa0 + sa1) + (sa2 + sa3) (train_ops.hip:31)
ACTS = ('tanh', 'relu', 'linear')
LIMIT = 2.0 ** 24

LOSS_SHAPES = [(4, 4, 6, 8), (3, 5, 37, 71), (1, 1, 1, 7), (2, 1, 300, 3), (64, 4, 88, 180)]
# (n, c_total, h, w, c_off, c): hw % 4 == 0 | even, not 4 k | odd;  N 1 and 64;  N hw < 64 (empty slices);  N hw = 189, 45
SLICED_SHAPES = [(64, 2, 88, 180, 0, 2), (2, 3, 44, 90, 1, 1), (64, 3, 22, 45, 1, 2), (3, 4, 7, 9, 1, 2), (1, 2, 73, 143, 0, 2),
                 (1, 3, 5, 9, 1, 1), (5, 2, 2, 6, 0, 2)]
POOL_SHAPES = [(64, 2, 88, 180), (3, 3, 22, 45), (2, 3, 7, 9), (2, 2, 7, 10), (1, 2, 6, 11), (1, 1, 2, 2)]
PHASE_SHAPES = [(64, 4, 44, 90), (2, 1, 22, 45), (2, 3, 11, 45), (3, 2, 7, 9), (1, 1, 3, 5)]      # (n, f, h, w) of the phase tensor (n, 4f, h, w)


def ceil_div(a, b):
    return -(-a // b)


def grid_for(items, cu):
    """train_ops.hip:512-517"""
    return int(min(max(ceil_div(items, 256), 1), 8 * cu))


def flat_sizes(cu):
    """1, 3, around one block, a large odd size, one above the grid cap, and the step's two real sizes"""
    return [1, 3, 255, 256, 257, 200003, 8 * cu * 256 + 12345, 64 * 4 * 88 * 180, 64 * 32 * 88 * 180]


# ---- k: additions on the longest path of each fixed tree ------------------------------------------------------------------------- #

def k_flat(n, cu):
    """mse_mae_partial_kernel (train_ops.hip:178-184) + mse_mae_final_kernel (:234-238), and loss_stats_partial_kernel (:281-299) +
    loss_stats_final_kernel (:325-334): grid-stride trips, a block sum, then one block strides over the `grid` partials."""
    grid = grid_for(n, cu)
    return ceil_div(n, grid * 256) + BLOCK_ADDS + ceil_div(grid, 256) + BLOCK_ADDS


def k_sliced(per):
    """bias_grad_partial_kernel (train_ops.hip:57-64) and pool_act_bwd_bias_partial_kernel (:121-124, :164), per = the channel's
    elements / windows: a slice of ceil(per / 64) in strides of 256, a block sum, then bias_grad_final_kernel's wave sum (:169)."""
    return ceil_div(ceil_div(per, BIAS_SPLIT), 256) + BLOCK_ADDS + 6


def k_act_bias(n, hw, vec):
    """act_bwd_bias_partial_kernel<VEC> (train_ops.hip:79-105): a slice rounded up to 4 elements is walked plane segment by plane
    segment, a thread adding VEC values per trip (:101); the worst slice, + block sum + bias_grad_final_kernel (:169)."""
    per = n * hw
    chunk = (ceil_div(per, BIAS_SPLIT) + 3) & ~3
    worst = 0
    for s in range(BIAS_SPLIT):
        base, hi, adds = s * chunk, min(s * chunk + chunk, per), 0
        while base < hi:
            p0 = base % hw
            p1 = min(p0 + hi - base, hw)
            adds += ceil_div(p1 - p0, 256 * vec) * vec
            base += p1 - p0
        worst = max(worst, adds)
    return worst + BLOCK_ADDS + 6


def k_phase(n, f, h, w):
    """mse_mae_phase_partial_kernel (train_ops.hip:205-223): slices of the n h w pixels of a phase channel; loss sums: then
    mse_mae_final_kernel over 4 f 64 partials (:234-238); bias sums: bias_grad_final_kernel (:169).  Returns (k_loss, k_bias)."""
    trips = ceil_div(ceil_div(n * h * w, BIAS_SPLIT), 256)
    return trips + BLOCK_ADDS + ceil_div(4 * f * BIAS_SPLIT, 256) + BLOCK_ADDS, trips + BLOCK_ADDS + 6


def k_plane(hw):
    """loss_plane_sums_kernel (train_ops.hip:308-313)"""
    return ceil_div(hw, 256) + BLOCK_ADDS


def k_spreg(planes):
    """the 'spatial' regulariser's sum over the planes in loss_stats_final_kernel (train_ops.hip:329, :334)"""
    return ceil_div(planes, 256) + BLOCK_ADDS


def k_defer(n, S):
    """The final stage when it is deferred (dlwp_reduce_defer, batch.hip:235-240 picks eb; reduce_job_body, batch.hip:106-126): G =
    256 / eb partial groups; a thread adds ceil(ceil(S / G) / 8) values into each of 8 registers (:115-119), folds them in 3 levels
    (:121), and one thread adds the G group sums in turn (:125).  Replaces the final stage's `trips + BLOCK_ADDS` (flat) or 6 (bias:
    n = c, S = 64 -> eb 16, G 16: 1 + 3 + 16 = 20; mse_mae at the grid cap: n = 2, S = 2048 -> eb 4, G 64: 4 + 3 + 64 = 71)."""
    eb = 16 if (n < 64 * 256 and S >= 64) else 64
    if n <= 1024 and S >= 512:
        eb = 4
    G = 256 // eb
    return ceil_div(ceil_div(S, G), 8) + 3 + G


# ---- oracles with bounds ------------------------------------------------------------------------------------------------------- #

def act_bwd_oracle(y, dy, act):
    """(dz float64, per-element bound): 0 for relu / linear"""
    want = np_ref.act_bwd(y, dy, act)
    if act != 'tanh':
        return want, np.zeros(want.shape)
    t2 = np.asarray(y, np.float64) ** 2
    return want, np.abs(np.asarray(dy, np.float64)) * (2 * np.abs(1 - t2) + t2) * U * SECOND


def pool_act_bwd_oracle(y, dp, act):
    want = np_ref.pool_act_bwd(y, dp, act)
    if act != 'tanh':
        return want, np.zeros(want.shape)
    # the routed gradient times (1 - m m), m = y at the maximum: the bound of act_bwd at that element, 0 elsewhere
    routed = np_ref.maxpool2_grad(np.asarray(y, np.float64), dp)
    t2 = np.asarray(y, np.float64) ** 2
    return want, np.abs(routed) * (2 * np.abs(1 - t2) + t2) * U * SECOND


def sum_oracle(dz_own, c_off, c, k):
    """(db float64, bound) from a kernel's own float32 dz"""
    dz = np.asarray(dz_own, np.float64)
    return np_ref.channel_sum(dz, c_off, c), k * U * SECOND * np_ref.channel_sum(np.abs(dz), c_off, c)


def mse_mae_oracle(yp, yt, lw, k):
    """((mse, mae), (bound_mse, bound_mae), dy, bound_dy, (s2, s1)); lw already float32-rounded.  Terms: d d has 3 roundings (d
    twice, the product), |d| one; the value is s * fl(1 / n): 2 more."""
    s2, s1, v2, v1, dy = np_ref.mse_mae(yp, yt, lw)
    return ((v2, v1), ((k + 5) * U * SECOND * v2, (k + 3) * U * SECOND * v1), dy, 4 * U * SECOND * np.abs(dy), (s2, s1))


def custom_loss_oracle(yp, yt, mean, row_w, kind, reg, lw, sums=None, cu=CU):
    """(stats[7], bound_stats[7], dy, bound_dy, aux) of dlwp_loss_custom; see the module docstring for every term.  sums: the
    kernel's own float32 {'spt', 'spp', 'stt', 'extra', 'plane'} for the gradient."""
    stats, dy, aux = np_ref.custom_loss(yp, yt, mean, row_w, kind, reg, lw, sums)
    yp, yt = np.asarray(yp, np.float64), np.asarray(yt, np.float64)
    n, c, h, w_ = yp.shape
    numel = yp.size
    w = np.ones((1, 1, 1, 1)) if row_w is None else np.asarray(row_w, np.float64).reshape(1, 1, h, 1)
    m = 0.0 if mean is None else np.asarray(mean, np.float64).reshape(1, c, h, w_)
    d = yp - yt
    pw, tw = w * yp, w * yt
    dw = w * d
    P, T = pw - m, tw - m
    eP, eT = U * (np.abs(pw) + np.abs(P)), U * (np.abs(tw) + np.abs(T))
    k = k_flat(numel, cu)
    # ---- the sums and the values
    e_pt = float(np.sum(eP * np.abs(T) + eT * np.abs(P))) + (k + 1) * U * float(np.sum(np.abs(P * T)))
    e_pp = float(np.sum(2 * eP * np.abs(P))) + (k + 1) * U * stats[4]
    e_tt = float(np.sum(2 * eT * np.abs(T))) + (k + 1) * U * stats[5]
    b = np.zeros(7)
    b[1], b[2] = (k + 5) * U * stats[1], (k + 3) * U * stats[2]
    b[3], b[4], b[5] = e_pt, e_pp, e_tt
    mse_w = float(np.sum(dw * dw)) / numel
    e_mse_w = (k + 7) * U * mse_w                       # d, w d: (w d)^2 carries 5 roundings; + inv_n and the scaling
    if kind == 0:
        b[0] = e_mse_w
    else:
        if reg == 1:
            b[6] = e_mse_w
        elif reg == 2:
            b[6] = (k + 4) * U * float(np.sum(np.abs(dw))) / numel
        elif reg == 3:
            sp, st = aux['extra']
            e7, e8 = (k + 1) * U * float(np.sum(np.abs(pw))), (k + 1) * U * float(np.sum(np.abs(tw)))
            q = (st - sp) / st
            b[6] = (e7 + e8) / abs(st) + abs(q) * e8 / abs(st) + 2 * U * abs(q)
        elif reg == 4:
            kp = k_plane(h * w_)
            sp, st = aux['plane'][:, 0], aux['plane'][:, 1]
            e7 = (kp + 1) * U * np.abs(pw).sum(axis=(2, 3)).reshape(-1)
            e8 = (kp + 1) * U * np.abs(tw).sum(axis=(2, 3)).reshape(-1)
            q = (st - sp) / st
            eq = (e7 + e8) / np.abs(st) + np.abs(q) * e8 / np.abs(st) + 2 * U * np.abs(q)
            b[6] = (float(eq.sum()) + (k_spreg(n * c) + 1) * U * float(np.abs(q).sum())) / (n * c)
        a = stats[3] / math.sqrt(stats[4] * stats[5])
        e_a = e_pt / math.sqrt(stats[4] * stats[5]) + abs(a) * (e_pp / (2 * stats[4]) + e_tt / (2 * stats[5])) + 3 * U * abs(a)
        b[0] = b[6] + e_a + U * abs(stats[0])
    # ---- the gradient, from `sums`
    if kind == 0:
        bdy = 6 * U * np.abs(dy)
    else:
        s = sums if sums is not None else {'spt': stats[3], 'spp': stats[4], 'stt': stats[5]}
        spt, spp, stt = float(s['spt']), float(s['spp']), float(s['stt'])
        r, inv_norm = spt / spp, 1.0 / math.sqrt(spp * stt)
        A = T - r * P
        eA = eT + abs(r) * eP + 2 * U * np.abs(r * P) + U * np.abs(A)
        g1 = -A * inv_norm
        eg = eA * inv_norm + 4 * U * np.abs(g1)
        lww = lw * w
        g = dy / np.where(lww == 0, 1.0, lww)
        if reg != 0:
            rounds = {1: 4, 2: 1, 3: 1, 4: 2}[reg]
            eg = eg + rounds * U * np.abs(g - g1) + U * np.abs(g)
        bdy = np.abs(lww) * eg + 2 * U * np.abs(dy)
    return stats, b * SECOND, dy, bdy * SECOND, aux


# ---- inputs ------------------------------------------------------------------------------------------------------------------------ #

def density(numel):
    """the share of non-zero elements of a family (a) tensor: 1 up to 2^18 elements, then thinned so that the sums stay below 2^24"""
    return min(1.0, 2.0 ** 18 / numel)


def small_ints(rng, shape, rho=None, positive=False):
    """float32 integers in {-1, 0, 1} (positive: {0, 1, 2}) with about 1 in 64 of the non-zeros doubled, non-zero with density rho"""
    numel = int(np.prod(shape))
    rho = density(numel) if rho is None else rho
    v = rng.integers(1, 3, size=shape) if positive else rng.choice(np.array([-1, 1]), size=shape)
    v = np.where(rng.random(shape) < 1.0 / 64, 2 * np.sign(v), v)
    v = np.where(rng.random(shape) < rho, v, 0)
    return v.astype(np.float32)


def exact_row_weights(h):
    return np.where(np.arange(h) % 3 == 0, 0.5, 1.0).astype(np.float32)


def exact_loss_case(rng, shape, positive=False):
    """family (a) for dlwp_loss_custom / dlwp_mse_mae: (yp, yt, mean, row_w).  yt small integers, yp = yt + e with e in {-1, 0, 1}
    (positive: yt >= 0 with a 1 at the start of every row and e >= 0 with a 1 at the start of every plane, so every plane has
    St > 0 and Sp > St: the sign of q rests on integers); the climatology is a sparse multiple of 1/4 in [-1/2, 1/2]."""
    n, c, h, w = shape
    rho = density(n * c * h * w)
    yt = small_ints(rng, shape, rho, positive)
    e = small_ints(rng, shape, rho / 2, positive)
    e = np.clip(e, -1, 1)
    if positive:
        yt[..., 0] = 1
        e[:, :, 0, 0] = 1
    mean = (0.25 * rng.integers(-2, 3, size=(c, h, w)) * (rng.random((c, h, w)) < rho)).astype(np.float32)
    return (yt + e).astype(np.float32), yt, mean, exact_row_weights(h)


def exact_condition(terms, unit):
    """sum |terms| in units: every term an integer number of units, the total below 2^24 -> any float32 summation order is exact"""
    t = np.abs(np.asarray(terms, np.float64)) / unit
    assert np.array_equal(t, np.round(t)), 'a term is not a multiple of the unit'
    return float(t.sum())


def loss_exact_condition(yp, yt, mean, row_w):
    """the largest of the nine sums of loss_stats_partial_kernel (and with it the plane sums), in its own unit"""
    yp, yt = yp.astype(np.float64), yt.astype(np.float64)
    w = 1.0 if row_w is None else row_w.astype(np.float64).reshape(1, 1, -1, 1)
    m = 0.0 if mean is None else mean.astype(np.float64)[None]
    d, dw, P, T = yp - yt, w * (yp - yt), w * yp - m, w * yt - m
    return max(exact_condition(d * d, 1), exact_condition(d, 1), exact_condition(dw * dw, 0.25), exact_condition(dw, 0.5),
               exact_condition(P * T, 1.0 / 16), exact_condition(P * P, 1.0 / 16), exact_condition(T * T, 1.0 / 16),
               exact_condition(w * yp, 0.5), exact_condition(w * yt, 0.5))


REAL_MARGIN = 0.01


def real_loss_case(rng, shape, positive=False):
    """family (b): yt ~ N(0, 1), yp = yt + 0.3 N(0, 1), climatology 0.1 N(0, 1), cosine row weights.  positive (regularize 3, 4, as
    the golden *_pos arrays): yt = 3 + clip(N, -2, 2) in [1, 5], yp = yt + 0.05 + 0.3 |N| and the climatology + 3, so that with the
    positive weights every plane has St in [sum w, 5 sum w] and Sp - St >= 0.05 sum w:  |q| = |St - Sp| / St >= 0.01 = REAL_MARGIN
    for every plane and for the whole tensor, four orders of magnitude above the float32 error of the sums."""
    n, c, h, w = shape
    g = rng.standard_normal(shape)
    e = 0.3 * rng.standard_normal(shape)
    mean = 0.1 * rng.standard_normal((c, h, w))
    if positive:
        yt = (3.0 + np.clip(g, -2, 2)).astype(np.float32)
        yp = (yt + np.float32(0.0505) + np.abs(e)).astype(np.float32)
        mean = mean + 3.0
    else:
        yt = g.astype(np.float32)
        yp = (yt + e).astype(np.float32)
    row_w = np_ref.latitude_weights(np.linspace(80., -80., h) if h > 1 else np.array([40.])).astype(np.float32)
    return yp, yt, mean.astype(np.float32), row_w


def loss_combos():
    """(kind, regularize, use_mean, use_row_w, loss_weight): kind 0 with and without row weights; kind 1 with regularize 0 ... 4,
    each with and without a climatology, each with and without row weights; loss_weight alternates between 1 and 0.7"""
    out = [(0, 0, False, False, 1.0), (0, 0, False, True, f32(0.7))]
    for reg in range(5):
        for i, (um, uw) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
            out.append((1, reg, um, uw, 1.0 if (reg + i) % 2 == 0 else f32(0.7)))
    return out


def act_case(rng, shape, act, exact):
    """(y, dy) float32.  exact: dy small integers, y in {-1, -0.5, -0.0, 0, 0.5, 1} (1 - y^2 in {0, 3/4, 1}: dz a multiple of 1/4).
    real: y = tanh(N) | N for relu, dy ~ N, with the kinks planted: y == 0, y == -0.0, y == +-1."""
    if exact:
        dy = small_ints(rng, shape, 1.0)                # dense: a dropped element is then almost surely a non-zero one
        y = rng.choice(np.array([-1, -0.5, -0.0, 0, 0.5, 1], dtype=np.float32), size=shape)
        return y, dy
    z = rng.standard_normal(shape)
    y = (np.tanh(z) if act == 'tanh' else z).astype(np.float32).reshape(-1)
    dy = rng.standard_normal(shape).astype(np.float32)
    for j, v in enumerate((0.0, -0.0, 1.0, -1.0)):
        y[j::29] = v
    return y.reshape(shape), dy


def pool_case(rng, shape, exact):
    """(y, dp): y with plenty of ties inside windows (a third of the elements share one value, every 5th window is constant: a tie
    between the first and the last position), dp small integers (exact) or N(0, 1)"""
    n, c, h, w = shape
    y = rng.choice(np.array([-1, -0.5, 0, 0.5, 1], dtype=np.float32), size=shape) if exact else \
        np.tanh(rng.standard_normal(shape)).astype(np.float32)
    y[rng.random(shape) < 0.3] = 0.5
    flat = y.reshape(-1)
    flat[::7] = -0.0
    h2, w2 = h // 2, w // 2
    const = rng.random((n, c, h2, w2)) < 0.2
    win = y[:, :, :2 * h2, :2 * w2].reshape(n, c, h2, 2, w2, 2)
    first = win[:, :, :, 0, :, 0].copy()
    for a in (0, 1):
        for b in (0, 1):
            win[:, :, :, a, :, b] = np.where(const, first, win[:, :, :, a, :, b])
    y[:, :, :2 * h2, :2 * w2] = win.reshape(n, c, 2 * h2, 2 * w2)
    dp = small_ints(rng, (n, c, h2, w2), density(n * h2 * w2)) if exact else rng.standard_normal((n, c, h2, w2)).astype(np.float32)
    return y, dp


# ---- float32 restatements: every operation rounded once, sums in the kernel's order ------------------------------------------------- #

F1 = np.float32(1)


def wave_sum_f32(v):
    """(..., 64) -> (...): v += shfl_down(v, off) for off = 32 ... 1; lane 0"""
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def block_sum_f32(v):
    """(..., 256) -> (...): block_sum2"""
    wv = wave_sum_f32(v.reshape(v.shape[:-1] + (4, 64)))
    return (wv[..., 0] + wv[..., 1]) + (wv[..., 2] + wv[..., 3])


def strided_f32(x, lanes=256):
    """(..., L) -> (..., lanes): lane t adds x[t], x[t + lanes], ... in turn"""
    trips = max(1, ceil_div(x.shape[-1], lanes))
    pad = np.zeros(x.shape[:-1] + (trips * lanes,), np.float32)
    pad[..., :x.shape[-1]] = x
    pad = pad.reshape(x.shape[:-1] + (trips, lanes))
    acc = np.zeros(x.shape[:-1] + (lanes,), np.float32)
    for t in range(trips):
        acc = acc + pad[..., t, :]
    return acc


def flat_sum_f32(terms, cu=CU):
    """a grid-stride partial kernel followed by a one-block final kernel"""
    terms = terms.reshape(-1)
    grid = grid_for(terms.size, cu)
    trips = ceil_div(terms.size, grid * 256)
    pad = np.zeros(trips * grid * 256, np.float32)
    pad[:terms.size] = terms
    pad = pad.reshape(trips, grid, 256)
    acc = np.zeros((grid, 256), np.float32)
    for t in range(trips):
        acc = acc + pad[t]
    return block_sum_f32(strided_f32(block_sum_f32(acc)))


def sliced_partials_f32(terms):
    """(per,) -> the 64 slice sums of bias_grad_partial_kernel / the pool and phase kernels"""
    per = terms.size
    chunk = max(1, ceil_div(per, BIAS_SPLIT))
    pad = np.zeros(BIAS_SPLIT * chunk, np.float32)
    pad[:per] = terms[:BIAS_SPLIT * chunk]
    return block_sum_f32(strided_f32(pad.reshape(BIAS_SPLIT, chunk)))


def act_bias_partials_f32(dz_channel, vec):
    """(N, hw) of one channel -> the 64 slice sums of act_bwd_bias_partial_kernel<vec>"""
    n, hw = dz_channel.shape
    flat = dz_channel.reshape(-1)
    per = n * hw
    chunk = (ceil_div(per, BIAS_SPLIT) + 3) & ~3
    out = np.zeros(BIAS_SPLIT, np.float32)
    for s in range(BIAS_SPLIT):
        base, hi = s * chunk, min(s * chunk + chunk, per)
        acc = np.zeros(256, np.float32)
        while base < hi:
            p0 = base % hw
            p1 = min(p0 + hi - base, hw)
            seg = flat[base:base + p1 - p0]
            trips = ceil_div(seg.size, 256 * vec)
            pad = np.zeros(trips * 256 * vec, np.float32)
            pad[:seg.size] = seg
            pad = pad.reshape(trips, 256, vec)
            for t in range(trips):
                for k in range(vec):
                    acc = acc + pad[t, :, k]
            base += p1 - p0
        out[s] = block_sum_f32(acc)
    return out


def act_bwd_f32(y, dy, act):
    if act == 'tanh':
        return dy * (F1 - y * y)
    if act == 'relu':
        return np.where(y > 0, dy, np.float32(0))
    return dy.copy()


def mse_mae_f32(yp, yt, lw, cu=CU):
    n = np.float32(yp.size)
    inv_n = F1 / n
    d = yp - yt
    scale = np.float32(2) * np.float32(lw) * inv_n
    return flat_sum_f32(d * d, cu) * inv_n, flat_sum_f32(np.abs(d), cu) * inv_n, scale * d


def loss_custom_f32(yp, yt, mean, row_w, kind, reg, lw, cu=CU):
    """dlwp_loss_custom as the kernels compute it -> (stats[7] float32, dy float32)"""
    n, c, h, w_ = yp.shape
    w = np.ones((1, 1, 1, 1), np.float32) if row_w is None else row_w.reshape(1, 1, h, 1)
    m = np.float32(0) if mean is None else mean.reshape(1, c, h, w_)
    d = yp - yt
    dw = w * d
    P, T = w * yp - m, w * yt - m
    pw, tw = (w * yp) * np.ones(yp.shape, np.float32), (w * yt) * np.ones(yp.shape, np.float32)
    s = [flat_sum_f32(t, cu) for t in (d * d, np.abs(d), dw * dw, np.abs(dw), P * T, P * P, T * T, pw, tw)]
    inv_n = F1 / np.float32(yp.size)
    planes = np.float32(n * c)
    plane = np.stack([block_sum_f32(strided_f32(pw.reshape(n * c, h * w_))), block_sum_f32(strided_f32(tw.reshape(n * c, h * w_)))], 1)
    mse_w, mae_w = s[2] * inv_n, s[3] * inv_n
    regv = np.float32(0)
    if kind == 0:
        loss = mse_w
    else:
        acc = s[4] / np.sqrt(s[5] * s[6])
        if reg == 1:
            regv = mse_w
        elif reg == 2:
            regv = mae_w
        elif reg == 3:
            regv = np.abs((s[8] - s[7]) / s[8])
        elif reg == 4:
            regv = block_sum_f32(strided_f32(np.abs((plane[:, 1] - plane[:, 0]) / plane[:, 1]))) / planes
        loss = regv - acc
    stats = np.array([loss, s[0] * inv_n, s[1] * inv_n, s[4], s[5], s[6], regv], np.float32)
    spt, spp, stt = s[4], s[5], s[6]
    if kind == 0:
        g = np.float32(2) * dw * inv_n
    else:
        inv_norm, ratio = F1 / np.sqrt(spp * stt), spt / spp
        g = -(T - ratio * P) * inv_norm
        if reg == 1:
            g = g + np.float32(2) * dw * inv_n
        elif reg == 2:
            g = g + np.sign(dw) * inv_n
        elif reg == 3:
            g = g + (-np.sign((s[8] - s[7]) / s[8])) / s[8]
        elif reg == 4:
            t2 = (-np.sign((plane[:, 1] - plane[:, 0]) / plane[:, 1])) / (plane[:, 1] * planes)
            g = g + t2.reshape(n, c, 1, 1)
    dy = (np.float32(lw) * w) * g
    sums = {'spt': spt, 'spp': spp, 'stt': stt, 'extra': np.array([s[7], s[8]]), 'plane': plane}
    return stats, dy.astype(np.float32), sums


def ratios_of(got, want, bound, what):
    got, want, bound = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, want, bound))
    return worst_ratio(got, want, bound, what)


# ---- tests -------------------------------------------------------------------------------------------------------------------------- #

def torch_custom_loss(p, yt, mean, row_w, kind, reg, lw):
    import torch
    t = torch.tensor(yt, dtype=torch.float64)
    n, c, h, w_ = yt.shape
    w = torch.ones(1, dtype=torch.float64) if row_w is None else torch.tensor(row_w, dtype=torch.float64).reshape(1, 1, h, 1)
    m = torch.zeros(1, dtype=torch.float64) if mean is None else torch.tensor(mean, dtype=torch.float64)[None]
    pw, tw = p * w, t * w
    if kind == 0:
        return lw * ((pw - tw) ** 2).mean()
    P, T = pw - m, tw - m
    a = (P * T).mean() / torch.sqrt((P * P).mean() * (T * T).mean())
    if reg == 0:
        r = 0.0
    elif reg == 1:
        r = ((pw - tw) ** 2).mean()
    elif reg == 2:
        r = (pw - tw).abs().mean()
    elif reg == 3:
        r = ((tw.mean() - pw.mean()) / tw.mean()).abs()
    else:
        mt, mp = (tw * torch.ones_like(t)).mean(dim=(-2, -1)), (pw * torch.ones_like(t)).mean(dim=(-2, -1))
        r = ((mt - mp) / mt).abs().mean()
    return lw * (r - a)


@pytest.mark.parametrize('shape', [(4, 4, 6, 8), (2, 3, 5, 7), (1, 1, 1, 7), (2, 1, 30, 3)])
def test_closed_form_gradient_of_the_custom_loss_oracle_equals_float64_autograd(shape):
    """np_ref.custom_loss: its value and its closed-form gradient against torch float64 autograd of the loss written out from the
    reference's formula, for every (kind, regularize, climatology, row weights, loss_weight) combination"""
    import torch
    rng = np.random.default_rng(11)
    for kind, reg, um, uw, lw in loss_combos():
        yp, yt, mean, row_w = real_loss_case(rng, shape, positive=reg >= 3)
        mean, row_w = (mean if um else None), (row_w if uw else None)
        stats, dy, _ = np_ref.custom_loss(yp, yt, mean, row_w, kind, reg, lw)
        p = torch.tensor(yp, dtype=torch.float64, requires_grad=True)
        loss = torch_custom_loss(p, yt, mean, row_w, kind, reg, lw)
        loss.backward()
        want = p.grad.numpy()
        assert lw * stats[0] == pytest.approx(float(loss.detach()), rel=1e-12, abs=1e-14), (kind, reg, um, uw)
        assert np.abs(dy - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (kind, reg, um, uw)


def test_custom_loss_oracle_reproduces_every_scalar_of_the_reference_goldens(golden):
    """tests/golden/losses.npz holds the reference's own loss functions evaluated on 4x4x6x8 fields: the oracle, which extends the
    formula to other shapes, gives every one of them (tolerance of tests/test_oracle_golden.py: the goldens are float32 results)"""
    g = golden('losses')
    yt, yp, climo, lats = g['y_true'], g['y_pred'], g['climo'], g['lats']
    seen = set()
    for name, reg in ((None, 0), ('mse', 1), ('mae', 2), ('global', 3)):
        for um in (0, 1):
            key = 'acc_%s_%d' % (name, um)
            got = np_ref.custom_loss(yp, yt, climo[0] if um else None, None, 1, reg, 1.0)[0][0]
            assert np.isclose(got, float(g[key]), rtol=2e-5, atol=2e-6), (key, got, float(g[key]))
            seen.add(key)
    for name, reg in (('global', 3), ('spatial', 4)):
        for um in (0, 1):
            key = 'accpos_%s_%d' % (name, um)
            got = np_ref.custom_loss(g['y_pred_pos'], g['y_true_pos'], (climo[0] + 3.0) if um else None, None, 1, reg, 1.0)[0][0]
            assert np.isclose(got, float(g[key]), rtol=2e-5, atol=2e-6), (key, got, float(g[key]))
            seen.add(key)
    for weighting in ('cosine', 'midlatitude'):
        key = 'latw_%s' % weighting
        stats = np_ref.custom_loss(yp, yt, None, np_ref.latitude_weights(lats, weighting), 0, 0, 1.0)[0]
        assert np.isclose(stats[0], float(g[key]), rtol=2e-5), key
        assert stats[1] == pytest.approx(np_ref.mse(yt, yp), rel=1e-13) and stats[2] == pytest.approx(np_ref.mae(yt, yp), rel=1e-13)
        seen.add(key)
    scalars = {k for k in g.files if g[k].ndim == 0}
    assert seen == scalars, scalars ^ seen


def test_simple_oracles_against_their_definitions():
    """act_bwd, channel_sum, pool_act_bwd (first maximum in row-major order, ties, odd edges), the phase layout"""
    y = np.array([[[[1., 1., 0., -0., 5.], [1., 1., 0., 2., 5.], [9., 9., 9., 9., 9.]]]])
    dp = np.array([[[[3., 7.]]]])
    want = np.zeros(y.shape)
    want[0, 0, 0, 0], want[0, 0, 1, 3] = 3., 7.          # all-tie window: the first position; (0, -0, 0, 2): the last
    assert np.array_equal(np_ref.pool_act_bwd(y, dp, 'linear'), want)
    assert np.array_equal(np_ref.pool_act_bwd(y, dp, 'relu'), want)
    assert np.array_equal(np_ref.pool_act_bwd(y, dp, 'tanh'), want * np.array(1. - y * y))
    assert np.array_equal(np_ref.act_bwd(np.array([0., -0., 1., -1., 0.5]), np.full(5, 2.), 'relu'), [0, 0, 2, 0, 2])
    assert np.array_equal(np_ref.act_bwd(np.array([0., -0., 1., -1., 0.5]), np.full(5, 2.), 'tanh'), [2, 2, 0, 0, 1.5])
    x = np.arange(2 * 3 * 2 * 2, dtype=np.float64).reshape(2, 3, 2, 2)
    assert np.array_equal(np_ref.channel_sum(x, 1, 2), [x[:, 1].sum(), x[:, 2].sum()])
    ph = np.arange(2 * 8 * 3 * 5, dtype=np.float64).reshape(2, 8, 3, 5)
    full = np_ref.depth_to_space2(ph, 2)
    assert full[1, 1, 2 * 2 + 1, 2 * 4 + 0] == ph[1, (2 * 1 + 0) * 2 + 1, 2, 4]
    assert np.array_equal(np_ref.space_to_depth2(full), ph)
    s2, s1, v2, v1, dz, db = np_ref.mse_mae_phase(ph, np.zeros((2, 2, 6, 10)), 0.7)
    assert s2 == (ph ** 2).sum() and s1 == ph.sum() and np.allclose(dz, 0.7 * 2 * ph / ph.size, rtol=1e-15)
    assert np.allclose(db, dz.sum(axis=(0, 2, 3)), rtol=1e-15)


def test_tree_depths_counted_from_the_kernels():
    """the k of a few launches, worked by hand from the lines named in the k_* functions"""
    assert k_flat(768, CU) == 1 + 9 + 1 + 9                              # 3 blocks, one trip each
    assert k_flat(64 * 4 * 88 * 180, CU) == 8 + 9 + 8 + 9                # 15 840 blocks wanted, 2 048 run: 8 trips; 2 048 / 256
    assert k_sliced(64 * 88 * 180) == 62 + 9 + 6                         # a slice of 15 840 elements: 62 trips
    assert k_act_bias(64, 88 * 180, 4) == 16 * 4 + 9 + 6                 # one plane per slice: 15 840 / 1 024 -> 16 trips of 4
    assert k_act_bias(3, 63, 1) == 2 + 9 + 6 and k_sliced(45) == 1 + 9 + 6     # the slice [60, 64) crosses a plane: 2 segments
    assert k_phase(64, 4, 44, 90) == (16 + 9 + 4 + 9, 16 + 9 + 6)
    assert k_plane(88 * 180) == 62 + 9 and k_spreg(256) == 1 + 9
    assert k_defer(32, 64) == 20 and k_defer(2, 2048) == 71 and k_defer(2, 3) == 1 + 3 + 4


def test_family_a_cases_satisfy_the_exactness_condition():
    """every generated exact case: each sum's terms are integer multiples of its unit and their absolute values total below 2^24"""
    rng = np.random.default_rng(21)
    worst = 0.0
    for shape in LOSS_SHAPES:
        for positive in (False, True):
            yp, yt, mean, row_w = exact_loss_case(rng, shape, positive)
            assert np.abs(yp).max() <= 3 and np.abs(yp - yt).max() <= 1
            for m_ in (None, mean):
                for w_ in (None, row_w):
                    worst = max(worst, loss_exact_condition(yp, yt, m_, w_))
            if positive:
                w = row_w.astype(np.float64).reshape(1, 1, -1, 1)
                sp, st = (w * yp).sum(axis=(2, 3)), (w * yt).sum(axis=(2, 3))
                assert (st > 0).all() and (sp > st).all()
    for n in flat_sizes(CU):
        yp, yt, _, _ = exact_loss_case(rng, (1, 1, 1, n))
        worst = max(worst, exact_condition((yp - yt).astype(np.float64) ** 2, 1), exact_condition(yp - yt, 1))
    for (n, ct, h, w, c_off, c) in SLICED_SHAPES:
        for act in ACTS:
            y, dy = act_case(rng, (n, ct, h, w), act, True)
            dz = np_ref.act_bwd(y, dy, act)
            worst = max(worst, max(exact_condition(dz[:, ch], 0.25) for ch in range(ct)))
        worst = max(worst, max(exact_condition(small_ints(rng, (n, ct, h, w), 1.0)[:, ch], 1) for ch in range(ct)))
    for shape in POOL_SHAPES:
        y, dp = pool_case(rng, shape, True)
        dz = np_ref.pool_act_bwd(y, dp, 'tanh')
        worst = max(worst, max(exact_condition(dz[:, ch], 0.25) for ch in range(shape[1])))
    for (n, f, h, w) in PHASE_SHAPES:
        yp, yt, _, _ = exact_loss_case(rng, (n, f, 2 * h, 2 * w))
        d = (yp - yt).astype(np.float64)
        worst = max(worst, exact_condition(d * d, 1))
    assert worst < LIMIT, worst
    # the all-ones case: db = N hw, itself below 2^24
    assert max(n * h * w for (n, _, h, w, _, _) in SLICED_SHAPES) < LIMIT
    # uniform {-1, 0, 1} at the training shape, no thinning: sum d^2 of about 5.4e6 (the figure the design of family (a) rests on)
    a, b = rng.integers(-1, 2, size=(2, 64 * 4 * 88 * 180))
    assert 5.0e6 < float(((a - b) ** 2).sum()) < 5.8e6 < LIMIT


@pytest.mark.parametrize('act', ACTS)
def test_float32_restatements_of_the_backward_kernels_stay_inside_the_bounds(act):
    """act_bwd elementwise; the channel sums of bias_grad / act_bwd_bias_grad<4, 2, 1> / pool_act_bwd_bias_grad in the kernels'
    order against the float64 sum of the restatement's own dz.  The elementwise bound is not loose: worst ratio above 0.1."""
    rng = np.random.default_rng(31)
    worst_el, worst_sum = 0.0, 0.0
    for n in (1, 257, 200003):
        y, dy = act_case(rng, (n,), act, False)
        want, bound = act_bwd_oracle(y, dy, act)
        r = worst_ratio(act_bwd_f32(y, dy, act), want, bound, act)
        assert r <= 1.0
        worst_el = max(worst_el, r)
    assert worst_el > 0.1 or act != 'tanh'
    for (n, ct, h, w, c_off, c) in SLICED_SHAPES[1:]:
        y, dy = act_case(rng, (n, ct, h, w), act, False)
        dz = act_bwd_f32(y, dy, act)
        hw = h * w
        for vec in (4, 2, 1):
            if hw % vec:
                continue
            got = [wave_sum_f32(act_bias_partials_f32(dz[:, ch].reshape(n, hw), vec)) for ch in range(c_off, c_off + c)]
            want, bound = sum_oracle(dz, c_off, c, k_act_bias(n, hw, vec))
            worst_sum = max(worst_sum, ratios_of(got, want, bound, 'act_bwd_bias_grad'))
        got = [wave_sum_f32(sliced_partials_f32(dz[:, ch].reshape(-1))) for ch in range(c_off, c_off + c)]
        want, bound = sum_oracle(dz, c_off, c, k_sliced(n * hw))
        worst_sum = max(worst_sum, ratios_of(got, want, bound, 'bias_grad'))
    for shape in POOL_SHAPES[1:]:
        y, dp = pool_case(rng, shape, False)
        want, bound = pool_act_bwd_oracle(y, dp, act)
        n, c, h, w = shape
        slope = act_bwd_f32(y, np.ones_like(y), act)
        routed = np_ref.maxpool2_grad(y.astype(np.float64), dp).astype(np.float32)
        dz = (routed * slope).astype(np.float32)
        assert worst_ratio(dz, want, bound, 'pool') <= 1.0
        # the kernel sums one value per window, in window order
        h2, w2, hc, wc = h // 2, w // 2, (h + 1) // 2, (w + 1) // 2
        per_win = np.zeros((n, c, hc, wc), np.float32)
        per_win[:, :, :h2, :w2] = dz[:, :, :2 * h2, :2 * w2].reshape(n, c, h2, 2, w2, 2).sum(axis=(3, 5), dtype=np.float32)
        got = [wave_sum_f32(sliced_partials_f32(per_win[:, ch].reshape(-1))) for ch in range(c)]
        want, bound = sum_oracle(dz, 0, c, k_sliced(n * hc * wc))
        worst_sum = max(worst_sum, ratios_of(got, want, bound, 'pool db'))
    assert worst_sum <= 1.0, worst_sum


def test_float32_restatement_of_mse_mae_and_its_phase_form_stays_inside_the_bounds():
    rng = np.random.default_rng(41)
    worst = {}
    for n in [s for s in flat_sizes(CU) if s <= 64 * 4 * 88 * 180]:
        yp, yt, _, _ = real_loss_case(rng, (1, 1, 1, n))
        yp.reshape(-1)[::5] = yt.reshape(-1)[::5]                       # d == 0: the gradient is exactly 0 there
        lw = f32(0.7)
        vals, bvals, dy, bdy, _ = mse_mae_oracle(yp, yt, lw, k_flat(n, CU))
        g2, g1, gdy = mse_mae_f32(yp, yt, lw)
        for name, r in (('mse', ratios_of(g2, vals[0], bvals[0], 'mse')), ('mae', ratios_of(g1, vals[1], bvals[1], 'mae')),
                        ('dy', worst_ratio(gdy, dy, bdy, 'dy'))):
            assert r <= 1.0, (name, n, r)
            worst[name] = max(worst.get(name, 0.0), r)
        assert np.all(gdy.reshape(-1)[::5] == 0)
    assert worst['dy'] > 0.1
    for (n, f, h, w) in PHASE_SHAPES[1:]:
        yp, yt, _, _ = real_loss_case(rng, (n, f, 2 * h, 2 * w))
        ph = np_ref.space_to_depth2(yp)
        kl, kb = k_phase(n, f, h, w)
        s2, s1, v2, v1, dz, db = np_ref.mse_mae_phase(ph, yt, 1.0)
        inv_n = np.float32(1.0 / ph.size)
        d = ph - np_ref.space_to_depth2(yt)
        gdz = (np.float32(2) * inv_n) * d
        assert worst_ratio(gdz, dz, 4 * U * SECOND * np.abs(dz), 'phase dz') <= 1.0
        part2 = np.stack([sliced_partials_f32((d[:, ch] ** 2).reshape(-1)) for ch in range(4 * f)]).reshape(-1)
        got = block_sum_f32(strided_f32(part2)) * inv_n
        assert ratios_of(got, v2, (kl + 5) * U * SECOND * v2, 'phase mse') <= 1.0
        gdb = [wave_sum_f32(sliced_partials_f32(gdz[:, ch].reshape(-1))) for ch in range(4 * f)]
        want, bound = sum_oracle(gdz, 0, 4 * f, kb)
        assert ratios_of(gdb, want, bound, 'phase db') <= 1.0


@pytest.mark.parametrize('shape', LOSS_SHAPES)
def test_float32_restatement_of_the_custom_loss_stays_inside_the_bounds(shape):
    """all seven stats and the gradient (from the restatement's own float32 sums), every combination; at the training shape one
    combination per regulariser.  Family (a) through the same restatement: its sums are exact."""
    rng = np.random.default_rng(51)
    big = int(np.prod(shape)) > 10 ** 6
    cases = {pos: real_loss_case(rng, shape, pos) for pos in (False, True)}
    exact = {pos: exact_loss_case(rng, shape, pos) for pos in (False, True)}
    worst_dy = 0.0
    for kind, reg, um, uw, lw in loss_combos():
        if big and not (um and uw):
            continue
        yp, yt, mean, row_w = cases[reg >= 3]
        mean, row_w = (mean if um else None), (row_w if uw else None)
        got, gdy, sums = loss_custom_f32(yp, yt, mean, row_w, kind, reg, lw)
        stats, bstats, dy, bdy, _ = custom_loss_oracle(yp, yt, mean, row_w, kind, reg, lw, sums)
        for j in range(7):
            assert ratios_of(got[j], stats[j], bstats[j], 'stats[%d]' % j) <= 1.0, (kind, reg, um, uw, j)
        r = worst_ratio(gdy, dy, bdy, 'dy')
        assert r <= 1.0, (kind, reg, um, uw, r)
        worst_dy = max(worst_dy, r)
        yp, yt, mean, row_w = exact[reg >= 3]
        mean, row_w = (mean if um else None), (row_w if uw else None)
        got, gdy, sums = loss_custom_f32(yp, yt, mean, row_w, kind, reg, lw)
        stats, bstats, dy, bdy, aux = custom_loss_oracle(yp, yt, mean, row_w, kind, reg, lw, sums)
        assert np.array_equal(got[3:6].astype(np.float64), stats[3:6])
        assert np.array_equal(sums['plane'].astype(np.float64), aux['plane']) and np.array_equal(sums['extra'], aux['extra'])
        for j in (1, 2):
            assert abs(float(got[j]) - stats[j]) <= 2 * U * SECOND * stats[j]
        for j in (0, 6):
            assert ratios_of(got[j], stats[j], bstats[j], 'exact stats[%d]' % j) <= 1.0
        assert worst_ratio(gdy, dy, bdy, 'exact dy') <= 1.0
    assert worst_dy > 0.05
