"""Activation and merge layers on the GPU (csrc/eltwise.hip through every layer of the stack).

Kernels, in the guarded slabs of tests/test_gpu_train_ops.py (every output starts as NaN between guard elements that must keep
their bits, every call is made twice -- the second time at other alignments -- and must give the same bits):
  * exact family: the relu family (LeakyReLU, the capped leaky ReLU(10, 0.1, 0), ReLU(3, 0.1, 0.5), ThresholdedReLU) and every
    merge, forward and backward, BIT-EQUAL to the float32 numpy restatements of tests/test_eltwise_cpu.py (NaN results compared as
    NaN: the payload of a generated NaN is the hardware's);
  * transcendental family: elu, selu, sigmoid, hard_sigmoid, softplus, softsign, tanh against float64 at the project's float32
    parity bar, max |got - want| <= 1e-5 max |want| per tensor (FWD_TOL / BWD_TOL, tests/test_gpu_convlstm_bwd.py); the worst
    error / bound ratio is printed (-s) and recorded in DESIGN.md section 5.25.
Sizes 1 ... 9, 63 ... 65, 255 ... 257, 1023 ... 1025 and one size that sends every workgroup of the capped grid round its loop
twice and ends in a ragged quad; every operand 0 ... 3 floats past a 16-byte boundary (all combinations where there are at most
64, else the aligned call, each operand alone at each offset, and 16 random combinations: the 16-byte path is taken only when
every operand is aligned, so this reaches it, the element path and every single cause of falling back).

Models (batch 3, 4 channels, 8 x 12 and 6 x 9): predict and one training step against float64 torch, the split
Conv2D + Activation against the fused Conv2D(activation=), a Dense -> ELU -> Dense model, the recorded / replayed step against the
eager one, the captured rollout against the host loop, model files in both formats, and the bfloat16 refusal."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from tests.test_eltwise_cpu import (KINDS, MERGES, RELU_LAYERS, TRANSCENDENTAL, branch_shares, exact_values, np_act_bwd, np_act_fwd,
                                    np_merge_bwd, np_merge_fwd, relu_params)
from tests.test_gpu_batchnorm import EPS, MOM, _bits, _grads_of, _host, _randomise, _ref_params
from tests.test_gpu_convlstm_bwd import BWD_TOL
from tests.test_gpu_dense import TOL
from tests.test_gpu_train_ops import Slab, cu_count, same_bits

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
FWD_TOL = 1e-5          # the project's float32 parity bar, as BWD_TOL
SMALL_SIZES = list(range(1, 10)) + [63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def sizes():
    """... and the size at which every workgroup of the capped grid (8 per CU, 1024 elements per trip) makes a second trip of its
    loop and the last quad is ragged"""
    return SMALL_SIZES + [2 * cu_count() * 8 * 1024 - 5]


def with_specials(x, shift=0):
    """+-0, +-inf and NaN spread over x (from 5 elements on)"""
    x = x.copy()
    if x.size >= 5:
        x[(np.arange(5) * (x.size // 5) + shift) % x.size] = np.roll(SPECIALS, shift)
    return x


def bits_equal(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN in other places' % what
    bad = np.flatnonzero(got[~nan].view(np.uint32) != want[~nan].view(np.uint32))
    assert bad.size == 0, '%s: %d of %d elements differ, first got %r want %r' % (
        what, bad.size, got.size, got[~nan][bad[0]], want[~nan][bad[0]])


def align_combos(k, seed):
    if 4 ** k <= 64:
        return list(itertools.product(range(4), repeat=k))
    rng = np.random.default_rng(seed)
    out = [(0,) * k] + [tuple(a if j == i else 0 for j in range(k)) for i in range(k) for a in (1, 2, 3)]
    return out + [tuple(int(v) for v in rng.integers(0, 4, k)) for _ in range(16)]


def second_aligns(k, n):
    return tuple((n + 1 + 2 * j) % 4 for j in range(k))


def run_act(ops, x, dy, spec, aligns):
    """activation forward (dy None) or backward on slabs at `aligns` = (x[, dy], out)"""
    sx, so = Slab(x, aligns[0]), Slab(None, aligns[-1], x.shape)
    if dy is None:
        assert ops.activation_fwd(sx.t, *spec, out=so.t) is so.t
        got = so.read()
    else:
        sdy = Slab(dy, aligns[1])
        assert ops.activation_bwd(sx.t, sdy.t, *spec, out=so.t) is so.t
        got = so.read()
        assert sdy.unchanged()
    assert sx.unchanged()
    return got


def run_merge(ops, kind, xs, dy, aligns, want=None):
    """merge forward (dy None; aligns = sources + (y,)) or backward (aligns = sources + (dy,) + gradients)"""
    k = len(xs)
    sx = [Slab(x, a) for x, a in zip(xs, aligns[:k])]
    if dy is None:
        so = Slab(None, aligns[k], xs[0].shape)
        assert ops.merge_fwd(kind, [s.t for s in sx], out=so.t) is so.t
        got = so.read()
    else:
        sdy = Slab(dy, aligns[k])
        sd = [Slab(None, a, xs[0].shape) if (want is None or want[i]) else None for i, a in enumerate(aligns[k + 1:2 * k + 1])]
        ops.merge_bwd(kind, [s.t for s in sx], sdy.t, outs=[s.t if s is not None else None for s in sd])
        got = [s.read() if s is not None else None for s in sd]
        assert sdy.unchanged()
    assert all(s.unchanged() for s in sx)
    return got


# ----------------------------------------------------------------------------------------------------------------------- #
# exact family: the relu family
# ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('layer', RELU_LAYERS, ids=lambda c: '%s%r' % c)
def test_relu_family_bit_equal_at_every_size(ops, layer):
    alpha, max_value, theta = relu_params(*layer)
    spec = ('relu', alpha, max_value, theta)
    rng = np.random.default_rng(701)
    for n in sizes():
        x = with_specials(exact_values(rng, n), n % 3)
        dy = rng.standard_normal(n).astype(np.float32)
        if n >= 1023:      # every branch the layer has is taken; theta 0.5, max_value 3: at least 10 % each (about 55 / 22 / 23 %)
            lo, mid, hi = branch_shares(x[np.isfinite(x)], max_value, theta)
            assert lo >= 0.10 and mid >= 0.10 and (max_value is None or hi > 0), (lo, mid, hi)
            assert (max_value, theta) != (3.0, 0.5) or hi >= 0.10, (lo, mid, hi)
        got = run_act(ops, x, None, spec, (0, 0))
        assert same_bits(got, run_act(ops, x, None, spec, second_aligns(2, n)))
        bits_equal(got, np_act_fwd(x, *spec), 'forward %r n %d' % (layer, n))
        if n >= 1023 and max_value is not None:
            assert np.mean(got == np.float32(max_value)) > 0 and ((max_value, theta) != (3.0, 0.5) or np.mean(got == 3) >= 0.10)
        xb = exact_values(rng, n)                                       # the backward pass: numbers only
        got = run_act(ops, xb, dy, spec, (0, 0, 0))
        assert same_bits(got, run_act(ops, xb, dy, spec, second_aligns(3, n)))
        bits_equal(got, np_act_bwd(xb, dy, *spec), 'backward %r n %d' % (layer, n))


def test_relu_family_at_every_alignment(ops):
    spec = ('relu', 0.1, 3.0, 0.5)
    rng = np.random.default_rng(702)
    n = 1025
    x, dy = with_specials(exact_values(rng, n)), rng.standard_normal(n).astype(np.float32)
    xb = exact_values(rng, n)
    want_f, want_b = np_act_fwd(x, *spec), np_act_bwd(xb, dy, *spec)
    for al in align_combos(2, 1):
        bits_equal(run_act(ops, x, None, spec, al), want_f, 'forward at %r' % (al,))
    for al in align_combos(3, 2):
        bits_equal(run_act(ops, xb, dy, spec, al), want_b, 'backward at %r' % (al,))


def test_relu_family_ties_follow_the_table(ops):
    """x == theta takes the negative side (derivative alpha), x == max_value is not capped away (derivative 1)"""
    f = np.float32
    x = np.array([0.5, 3.0, 0.5, 3.0, np.nextafter(f(0.5), f(1)), np.nextafter(f(3), f(4)), np.nextafter(f(3), f(0)), 0.0, -0.0], f)
    dy = np.arange(1, x.size + 1, dtype=f)
    spec = ('relu', 0.1, 3.0, 0.5)
    got = run_act(ops, x, None, spec, (0, 1))
    bits_equal(got, np_act_fwd(x, *spec), 'forward ties')
    assert got[0] == 0 and got[1] == 3 and got[4] == x[4] and got[5] == 3 and got[6] == x[6]
    gb = run_act(ops, x, dy, spec, (0, 2, 0))
    bits_equal(gb, np_act_bwd(x, dy, *spec), 'backward ties')
    assert gb[0] == f(0.1) * dy[0] and gb[1] == dy[1] and gb[4] == dy[4] and gb[5] == 0 and gb[6] == dy[6]
    thr = run_act(ops, np.array([1.0, -np.inf, np.nextafter(f(1), f(2))], f), None, ('relu', 0.0, None, 1.0), (3, 0))
    assert thr[0] == 0 and thr[1] == 0 and thr[2] == np.nextafter(f(1), f(2))         # ThresholdedReLU: x > theta ? x : 0


# ----------------------------------------------------------------------------------------------------------------------- #
# exact family: merges
# ----------------------------------------------------------------------------------------------------------------------- #
def merge_sources(rng, n, k, specials):
    xs = [exact_values(rng, n) for _ in range(k)]
    return [with_specials(x, i) for i, x in enumerate(xs)] if specials else xs


@pytest.mark.parametrize('kind', MERGES)
def test_merge_forward_bit_equal_at_every_size(ops, kind):
    rng = np.random.default_rng(703)
    for n in sizes():
        for k in ((2,) if kind == 'subtract' else ((4,) if n > 2000 else (2, 3, 4))):
            xs = merge_sources(rng, n, k, True)           # +-0, +-inf and NaN at different places of every source
            got = run_merge(ops, kind, xs, None, (0,) * (k + 1))
            assert same_bits(got, run_merge(ops, kind, xs, None, second_aligns(k + 1, n)))
            bits_equal(got, np_merge_fwd(xs, kind), '%s of %d, n %d' % (kind, k, n))
            if kind in ('maximum', 'minimum') and n >= 5:
                ref = {'maximum': np.maximum, 'minimum': np.minimum}[kind]
                w = ref(ref(xs[0], xs[1]), ref(xs[2], xs[3])) if k == 4 else (ref(xs[0], xs[1]) if k == 2 else
                                                                              ref(ref(xs[0], xs[1]), xs[2]))
                assert np.array_equal(np.isnan(got), np.isnan(w)) and np.isnan(got).sum() >= k      # NaN in either operand
                assert np.array_equal(got[~np.isnan(w)], w[~np.isnan(w)])                           # (equal as numbers: 0 == -0)


@pytest.mark.parametrize('kind', MERGES)
def test_merge_backward_bit_equal_at_every_size(ops, kind):
    rng = np.random.default_rng(704)
    for n in sizes():
        for k in ((2,) if kind == 'subtract' else ((4,) if n > 2000 else (2, 3, 4))):
            xs = merge_sources(rng, n, k, False)
            if kind in ('maximum', 'minimum'):            # no ties: source i gets the odd multiples of 2^-7 shifted by i 2^-9
                xs = [x + np.float32(i * 2.0 ** -9) for i, x in enumerate(xs)]
            dy = rng.standard_normal(n).astype(np.float32)
            got = run_merge(ops, kind, xs, dy, (0,) * (2 * k + 1))
            again = run_merge(ops, kind, xs, dy, second_aligns(2 * k + 1, n))
            want = np_merge_bwd(xs, dy, kind)
            for i in range(k):
                assert same_bits(got[i], again[i])
                bits_equal(got[i], want[i], '%s of %d, n %d, input %d' % (kind, k, n, i))
            if kind in ('maximum', 'minimum'):
                assert np.array_equal(sum((g != 0).astype(int) for g in got), (dy != 0).astype(int))   # exactly one taker


def test_merge_at_every_alignment_and_skipped_gradients(ops):
    rng = np.random.default_rng(705)
    n = 1025
    for kind, k in (('add', 2), ('multiply', 3), ('maximum', 4), ('average', 3)):
        xs = merge_sources(rng, n, k, True)
        want = np_merge_fwd(xs, kind)
        for al in align_combos(k + 1, 3):
            bits_equal(run_merge(ops, kind, xs, None, al), want, '%s forward at %r' % (kind, al))
        xs = [x + np.float32(i * 2.0 ** -9) for i, x in enumerate(merge_sources(rng, n, k, False))]
        dy = rng.standard_normal(n).astype(np.float32)
        want = np_merge_bwd(xs, dy, kind)
        for al in align_combos(2 * k + 1, 4):
            for g, w in zip(run_merge(ops, kind, xs, dy, al), want):
                bits_equal(g, w, '%s backward at %r' % (kind, al))
        # a source that needs no gradient (the model input) is skipped, the others are written as before
        skip = [i != 1 for i in range(k)]
        got = run_merge(ops, kind, xs, dy, (0,) * (2 * k + 1), want=skip)
        assert got[1] is None and all(same_bits(got[i], want[i]) for i in range(k) if i != 1)


def test_maximum_minimum_ties_go_to_the_first_input(ops):
    f = np.float32
    a = np.array([1.0, 2.0, 2.0, -1.0, 0.0, 5.0, 5.0], f)
    b = np.array([1.0, 2.0, 3.0, -1.0, -0.0, 5.0, 4.0], f)
    c = np.array([1.0, 1.0, 3.0, -1.0, 0.0, 6.0, 5.0], f)
    dy = np.arange(1, 8, dtype=f)
    for kind in ('maximum', 'minimum'):
        got = run_merge(ops, kind, [a, b, c], dy, (0, 1, 2, 3, 0, 1, 2))
        want = np_merge_bwd([a, b, c], dy, kind)
        for g, w in zip(got, want):
            bits_equal(g, w, kind + ' ties')
        assert np.array_equal(sum((g != 0).astype(int) for g in got), np.ones(7, int))
    gmax = run_merge(ops, 'maximum', [a, b, c], dy, (0,) * 7)
    assert np.array_equal(gmax[0], [1, 2, 0, 4, 5, 0, 7]) and np.array_equal(gmax[1], [0, 0, 3, 0, 0, 0, 0]) and \
        np.array_equal(gmax[2], [0, 0, 0, 0, 0, 6, 0])
    assert same_bits(run_merge(ops, 'add', [a, a], None, (0, 0, 0)), a + a)            # one tensor named as two sources


def test_the_library_refuses_what_the_layers_refuse(ops):
    from dlwp_amd import _lib
    x = torch.zeros(16, device='cuda')
    with pytest.raises(_lib.DlwpError, match='threshold'):
        ops.activation_fwd(x, 'relu', 0.0, None, -1.0)
    with pytest.raises(_lib.DlwpError, match='max_value'):
        ops.activation_fwd(x, 'relu', 0.0, 1.0, 1.0)
    with pytest.raises(_lib.DlwpError, match='alias'):
        ops.activation_fwd(x, 'tanh', out=x)
    with pytest.raises(_lib.DlwpError, match='same tensor'):
        g = torch.empty_like(x)
        ops.merge_bwd('add', [x, x.clone()], torch.ones_like(x), outs=[g, g])
    with pytest.raises(_lib.DlwpError, match='exactly 2'):
        ops.merge_fwd('subtract', [x, x, x])


# ----------------------------------------------------------------------------------------------------------------------- #
# transcendental family
# ----------------------------------------------------------------------------------------------------------------------- #
def transcendental_inputs(rng, n, kind):
    x = (3.0 * rng.standard_normal(n)).astype(np.float32)
    if kind in ('softplus', 'sigmoid') and n >= 8:
        x[:: max(1, n // 4)][:4] = [-100.0, -20.0, 20.0, 100.0]
    if kind == 'hard_sigmoid':                    # at least 2^-7 from the kinks at +-2.5
        near = np.abs(np.abs(x) - 2.5) < 2.0 ** -7
        x[near] = np.sign(x[near]) * np.float32(2.5 + 2.0 ** -6)
    return x


@pytest.mark.parametrize('kind', TRANSCENDENTAL)
def test_transcendental_kinds_against_float64(ops, kind):
    rng = np.random.default_rng(706)
    worst = {'forward': 0.0, 'backward': 0.0}
    for n in sizes():
        for alpha in ((1.0, 0.3) if kind == 'elu' else (0.0,)):
            spec = (kind, alpha, None, 0.0)
            x = transcendental_inputs(rng, n, kind)
            dy = rng.standard_normal(n).astype(np.float32)
            x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
            for what, got, again, want, tol in (
                    ('forward', run_act(ops, x, None, spec, (0, 0)), run_act(ops, x, None, spec, second_aligns(2, n)),
                     np_act_fwd(x64, *spec), FWD_TOL),
                    ('backward', run_act(ops, x, dy, spec, (0, 0, 0)), run_act(ops, x, dy, spec, second_aligns(3, n)),
                     np_act_bwd(x64, dy64, *spec), BWD_TOL)):
                assert same_bits(got, again) and np.isfinite(got).all()
                bound = tol * float(np.abs(want).max())
                err = float(np.abs(got.astype(np.float64) - want).max())
                worst[what] = max(worst[what], err / bound)
                assert err <= bound, '%s %s n %d: error %.3g, bound %.3g' % (kind, what, n, err, bound)
    print('\nMEASURED %s: worst error / bound forward %.4f, backward %.4f' % (kind, worst['forward'], worst['backward']))


def test_nan_in_gives_nan_out_for_every_kind_in_both_passes(ops):
    x = np.array([1.0, np.nan, -2.0, np.nan, 0.25, 7.0, np.nan], np.float32)
    dy = np.ones(7, np.float32)
    for kind in KINDS:
        for spec in ([(kind, 0.0, None, 0.0), (kind, 0.1, 3.0, 0.5)] if kind == 'relu' else [(kind, 1.0, None, 0.0)]):
            for al in ((0, 0, 0), (1, 2, 3)):
                assert np.array_equal(np.isnan(run_act(ops, x, None, spec, al[:2])), np.isnan(x)), spec
                assert np.array_equal(np.isnan(run_act(ops, x, dy, spec, al)), np.isnan(x)), spec


# ----------------------------------------------------------------------------------------------------------------------- #
# models
# ----------------------------------------------------------------------------------------------------------------------- #
def _pads(t):
    from dlwp_amd.custom import PeriodicPadding2D
    return L.ZeroPadding2D(((1, 1), (0, 0)), **CF)(PeriodicPadding2D(((0, 0), (1, 1)), **CF)(t))


def _pads_ref(t):
    return F.pad(torch.cat([t[..., -1:], t, t[..., :1]], dim=-1), (0, 0, 1, 1))


def _conv_ref(t, lay, p):
    return F.conv2d(_pads_ref(t), p[(lay.name, 'kernel')]) + p[(lay.name, 'bias')].view(1, -1, 1, 1)


def _leaky_ref(t, alpha, max_value=None):
    y = torch.where(t > 0, t, alpha * t)
    return y if max_value is None else torch.where(t > max_value, torch.full_like(t, max_value), y)


def net_a(cs):
    """periodic / zero padding + Conv2D(8, 3) -> BatchNormalization -> LeakyReLU(0.1) -> MaxPooling2D -> conv ->
    ReLU(max_value=10, negative_slope=0.1) -> UpSampling2D -> Add([., skip]) -> conv.  On the 6 x 9 grid the pooled and
    up-sampled branch is one column short of the skip tensor: a zero column is padded on before the Add."""
    x0 = L.Input(shape=cs)
    skip = L.Conv2D(8, 3, **CF)(_pads(x0))
    t = L.LeakyReLU(0.1)(L.BatchNormalization(axis=1)(skip))
    t = L.Conv2D(8, 3, **CF)(_pads(L.MaxPooling2D(2, **CF)(t)))
    t = L.UpSampling2D(2, **CF)(L.ReLU(max_value=10, negative_slope=0.1)(t))
    if cs[2] % 2:
        t = L.ZeroPadding2D(((0, 0), (0, 1)), **CF)(t)
    return x0, L.Conv2D(cs[0], 3, **CF)(_pads(L.Add()([t, skip])))


def net_a_ref(model, x, p, training):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    bn = [lay for lay in model.layers if isinstance(lay, L.BatchNormalization)][0]
    skip = _conv_ref(x, convs[0], p)
    t = F.batch_norm(skip, p[(bn.name, 'moving_mean')], p[(bn.name, 'moving_variance')], p[(bn.name, 'gamma')],
                     p[(bn.name, 'beta')], training=training, momentum=1 - MOM, eps=EPS)
    t = _conv_ref(F.max_pool2d(_leaky_ref(t, 0.1), 2), convs[1], p)
    t = F.interpolate(_leaky_ref(t, 0.1, 10.0), scale_factor=2, mode='nearest')
    if x.shape[3] % 2:
        t = F.pad(t, (0, 1, 0, 0))
    return _conv_ref(t + skip, convs[2], p)


def net_b(cs):
    """the skip tensor feeds ELU, the Add and a convolution of its own; the other Add input feeds a further convolution too:
    both inputs of the Add collect gradients from elsewhere.  The output is the Average of three branches."""
    x0 = L.Input(shape=cs)
    skip = L.Conv2D(8, 3, **CF)(_pads(x0))
    t = L.Conv2D(8, 3, **CF)(_pads(L.ELU()(skip)))
    s = L.add([t, skip])
    branches = [L.Conv2D(cs[0], 3, **CF)(_pads(v)) for v in (s, skip, t)]
    return x0, L.Average()(branches)


def net_b_ref(model, x, p, training):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    skip = _conv_ref(x, convs[0], p)
    t = _conv_ref(F.elu(skip), convs[1], p)
    u, v, w = _conv_ref(t + skip, convs[2], p), _conv_ref(skip, convs[3], p), _conv_ref(t, convs[4], p)
    return (u + v + w) / 3.0


NETS = {'a': (net_a, net_a_ref), 'b': (net_b, net_b_ref)}
GRIDS = [(4, 8, 12), (4, 6, 9)]


def _model(which, cs, seed=1, lr=1e-3):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0, out = NETS[which][0](cs)
    m = Model(inputs=x0, outputs=out, seed=seed)
    m.compile(optimizer=Adam(lr=lr), loss='mse')
    _randomise(m, np.random.default_rng(seed + 100))
    return m


def _data(cs, seed, n=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n,) + cs).astype(np.float32), rng.standard_normal((n,) + cs).astype(np.float32))


@pytest.mark.parametrize('cs', GRIDS, ids=lambda c: '%dx%d' % c[1:])
@pytest.mark.parametrize('which', ['a', 'b'])
def test_predict_against_float64(which, cs):
    m = _model(which, cs)
    assert {'act', 'merge'} <= {op.kind for op in m.infer_plan.ops}
    x, _ = _data(cs, 11)
    x[0] *= 4.0                                    # (reach ReLU's cap and both sides of every kink)
    with torch.no_grad():
        want = NETS[which][1](m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False), False).numpy()
    got = m.predict(x)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print('\nMEASURED predict net %s %r: error %.3g of scale %.3g = %.3g' % (which, cs, err, scale, err / scale))
    assert err <= 1e-5 * scale


@pytest.mark.parametrize('cs', GRIDS, ids=lambda c: '%dx%d' % c[1:])
@pytest.mark.parametrize('which', ['a', 'b'])
def test_training_step_against_float64_autograd(monkeypatch, which, cs):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model(which, cs, seed=2)
    x, y = _data(cs, 12)
    p = _ref_params(m)
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    ref = ((NETS[which][1](m, torch.tensor(x, dtype=torch.float64), p, True) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    ref.backward()
    print('\nMEASURED step net %s %r: loss %.8g against %.8g' % (which, cs, loss, float(ref.detach())))
    got = _grads_of(m._trainer)
    assert len(got) == sum(1 for t in p.values() if t.requires_grad)
    worst = 0.0
    for (lname, nm), g in sorted(got.items()):
        r = p[(lname, nm)].grad.numpy()
        r = r.transpose(2, 3, 1, 0) if nm == 'kernel' else r
        ratio = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-6))
        worst = max(worst, ratio)
        print('MEASURED   %s/%s gradient error %.3g of its scale' % (lname, nm, ratio))
    assert loss == pytest.approx(float(ref.detach()), rel=TOL)
    assert worst <= TOL, worst


@pytest.mark.parametrize('act', ['tanh', 'relu'])
def test_split_activation_against_the_fused_convolution(act):
    from dlwp_amd.engine import Sequential
    cs = (4, 6, 9)

    def build(split):
        net = Sequential(seed=3)
        net.add(L.Conv2D(8, 3, padding='same', activation='linear' if split else act, input_shape=cs, **CF))
        if split:
            net.add(L.Activation(act))
        net.add(L.Conv2D(4, 3, padding='same', **CF))
        return net
    fused, split = build(False), build(True)
    _randomise(fused, np.random.default_rng(5))
    split.set_weights(fused.get_weights())
    assert [op.kind for op in split.infer_plan.ops] == ['conv', 'act', 'conv'] and len(fused.infer_plan.ops) == 2
    x, _ = _data(cs, 13)
    a, b = fused.predict(x), split.predict(x)
    print('\nMEASURED split %s against fused: max difference %.3g of scale %.3g, bits %s' % (
        act, float(np.abs(a - b).max()), float(np.abs(a).max()), 'equal' if np.array_equal(_bits(a), _bits(b)) else 'differ'))
    assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()


def test_dense_elu_dense_trains_against_autograd(monkeypatch):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    from tests.test_gpu_dense import _build
    f, n = 45, 7
    d = _build((('Dense', (23,), {'input_shape': (f,)}), ('ELU', None, None), ('Dense', (f,), None)), seed=4)
    assert [op.kind for op in d.model.plan.ops] == ['dense', 'act', 'dense']
    rng = np.random.default_rng(14)
    for lay in d.model.layers:
        if isinstance(lay, L.Dense):
            k, b = lay.get_weights()
            lay.set_weights([k, (0.1 * rng.standard_normal(b.shape)).astype(np.float32)])
    x, y = (3 * rng.standard_normal((n, f))).astype(np.float32), rng.standard_normal((n, f)).astype(np.float32)
    p = {(lay.name, nm): torch.tensor(a.astype(np.float64), requires_grad=True)
         for lay in d.model.layers for (nm, _), a in zip(lay._weights, lay.get_weights())}
    dense = [lay for lay in d.model.layers if isinstance(lay, L.Dense)]

    def ref(xt):
        t = F.elu(xt @ p[(dense[0].name, 'kernel')] + p[(dense[0].name, 'bias')])
        return t @ p[(dense[1].name, 'kernel')] + p[(dense[1].name, 'bias')]
    with torch.no_grad():
        want = ref(torch.tensor(x, dtype=torch.float64)).numpy()
    assert np.abs(d.model.predict(x) - want).max() <= 1e-5 * np.abs(want).max()
    logs = d.model.train_on_batch(x, y)
    torch.cuda.synchronize()
    val = ((ref(torch.tensor(x, dtype=torch.float64)) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    val.backward()
    assert logs[0] == pytest.approx(float(val.detach()), rel=TOL)
    for key, g in _grads_of(d.model._trainer).items():
        r = p[key].grad.numpy()
        ratio = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-6))
        print('MEASURED   %s/%s gradient error %.3g of its scale' % (key + (ratio,)))
        assert ratio <= TOL, key


def _run_steps(monkeypatch, which, cs, form, batches):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)
    m = _model(which, cs, seed=5)
    logs = [m.train_on_batch(x, y) for x, y in batches]
    torch.cuda.synchronize()
    tr = m._trainer
    if form != 'eager':
        n = batches[0][0].shape[0]
        ents = [e for k, e in tr._graphs.items() if k[0] == n and e.get('step') is not None]
        assert len(ents) == 1, 'the step of %d samples was not recorded (refused: %r)' % (n, tr._no_tape)
    return logs, [w.copy() for w in m.get_weights()], [s.cpu().numpy() for s in tr.opt_state]


@pytest.mark.parametrize('which', ['a', 'b'])
def test_replayed_step_equals_the_eager_step(monkeypatch, which):
    """2 eager steps, then the recorded (and validated) one and 2 replayed ones: 3 steps through the tape, nothing marks it foreign"""
    cs = GRIDS[1]
    batches = [_data(cs, 600 + i) for i in range(5)]
    ref = _run_steps(monkeypatch, which, cs, 'eager', batches)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, which, cs, form, batches)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
            assert np.array_equal(_bits(a), _bits(b)), form


@pytest.mark.parametrize('which', ['a', 'b'])
def test_captured_rollout_equals_the_host_loop(which):
    from dlwp_amd.model import DLWPFunctional
    cs = GRIDS[1]
    m = _model(which, cs, seed=6)
    d = DLWPFunctional(is_convolutional=True, is_recurrent=False, time_dim=2)
    d.model = d.base_model = m
    x, _ = _data(cs, 15, n=5)
    assert d._device_rollout_ok(x)
    kept = d.predict_timeseries(x, 8, keep_time_dim=True)            # one hipGraph of 4 forwards
    state, want = x, []
    for _ in range(4):
        state = m.predict(state)
        want.append(state)
    want = np.stack(want)
    assert np.isfinite(want).all() and kept.shape == (4, 5, 2, 2) + cs[1:]
    assert np.array_equal(_bits(kept), _bits(want.reshape(kept.shape)))
    ser = _host(m.rollout_on_device(torch.from_numpy(x).cuda(), 4, graph_cache=False))
    assert np.array_equal(_bits(ser), _bits(want))


@pytest.mark.parametrize('fmt', ['keras', 'npz'])
def test_saved_and_reloaded_model_predicts_and_trains_the_same_bits(tmp_path, monkeypatch, fmt):
    from dlwp_amd import serialization
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    cs = GRIDS[1]
    batches = [_data(cs, 800 + i) for i in range(4)]
    for which in ('a', 'b'):
        m = _model(which, cs, seed=7)
        for x, y in batches[:2]:
            m.train_on_batch(x, y)
        path = str(tmp_path / ('%s.%s' % (which, fmt)))
        m.save(path, format=fmt)
        m2 = serialization.load_model_file(path)
        assert [type(lay).__name__ for lay in m2.layers] == [type(lay).__name__ for lay in m.layers]
        assert [lay.get_config() for lay in m2.layers if isinstance(lay, (L._ActivationLayer, L._Merge))] == \
            [lay.get_config() for lay in m.layers if isinstance(lay, (L._ActivationLayer, L._Merge))]
        assert np.array_equal(_bits(m2.predict(batches[0][0])), _bits(m.predict(batches[0][0])))
        for x, y in batches[2:]:
            a, b = m.train_on_batch(x, y), m2.train_on_batch(x, y)
            assert np.array_equal(np.asarray(a), np.asarray(b)), (which, a, b)
        for a, b in zip(m.get_weights(), m2.get_weights()):
            assert np.array_equal(_bits(a), _bits(b)), which


def test_bfloat16_storage_is_refused_with_the_layers_name():
    from dlwp_amd.engine import Model
    x0 = L.Input(shape=(4, 8, 12))
    t = L.LeakyReLU(0.1, name='leaky_one')(L.Conv2D(8, 3, padding='same', **CF)(x0))
    m = Model(inputs=x0, outputs=L.Conv2D(4, 3, padding='same', **CF)(L.Add(name='the_sum')([t, t])))
    with pytest.raises(NotImplementedError, match='leaky_one, the_sum'):
        m.set_activation_dtype('bfloat16')
    assert m.activation_dtype == 'float32'
