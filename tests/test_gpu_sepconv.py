"""DepthwiseConv2D / SeparableConv2D on the GPU (csrc/sepconv.hip through every layer of the stack).

Kernels, on guarded slabs whose outputs start as NaN, 0 .. 3 floats off a 16-byte boundary: on small-integer inputs (|values| <= 4:
every sum is exact in float32) all six kernels are BIT-EQUAL to the float64 numpy restatements of tests/sepconv_cases.py; on Gaussian
inputs every element lies within (m + 1) 2^-24 sum |terms| of the restatement, m the number of terms of that element (taps or
channels + 1 for the forward, the summed positions for the gradients) -- the order-free float32 bound, so no sum order is pinned.
Forward and data gradient of a sample have the same bits in a batch of 1 and of 3, the weight gradients the same bits on a second
run, and accumulate = 1 gives the float32 sum dw + gradient.

Layers and models (a small U-Net on 4 x 16 x 20 whose 3 x 3 layers are SeparableConv2D, dilation 1 and 2, with one DepthwiseConv2D
and a 'same' layer): the forward against float64 torch at FWD_TOL = 1e-5, one training step against float64 autograd at
TOL / BWD_TOL, the replayed step, the captured rollout and model files bit for bit, bfloat16 storage refused, two data-parallel ranks
against one process."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from tests import sepconv_cases as S
from tests.test_gpu_batchnorm import _bits, _grads_of, _host, _ref_params
from tests.test_gpu_convlstm_bwd import BWD_TOL
from tests.test_gpu_dense import TOL
from tests.test_gpu_train_ops import Slab, same_bits

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
FWD_TOL = 1e-5          # the project's float32 parity bar, as tests/test_gpu_sconv.py uses it
ACT = {None: 0, 'linear': 0, 'tanh': 1, 'relu': 2}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def _within(got, want, terms, sumabs, what):
    """every element within (m + 1) 2^-24 sum |terms|; returns the worst error / bound"""
    bound = (np.asarray(terms, np.float64) + 1.0) * S.EPS * sumabs
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), '%s: error %.3g over a bound of %.3g' % (what, float(err.max()), float(bound[err > bound].min()))
    return float((err / np.maximum(bound, 1e-300)).max())


# ----------------------------------------------------------------------------------------------------------------------- #
# 1. the depthwise stencil
# ----------------------------------------------------------------------------------------------------------------------- #
def _dw_case(ops, rng, n, c, h, w, ks, dil, dm, pad, modes, align=0, c_off=0, c_total=None, z_total=None):
    """forward, data gradient and weight gradient of one geometry on guarded slabs, integers (bit-equal) and Gaussians (bound);
    a halo that does not fit the map, or a kernel larger than the padded map, is refused and the slabs stay untouched"""
    what = (n, c, h, w, ks, dil, dm, pad, modes, align, c_off)
    c_total, z_total = c_total or c, z_total or c * dm
    z_off = c_off
    d = ops.make_depthwise(ks[0], ks[1], dil, dm, ops.make_pad(*pad, *modes), 0, in_c_off=c_off, out_c_off=z_off)
    ho, wo = S.out_hw(h, w, pad, ks, dil)
    fits = S.halo_fits(pad, modes, h, w)
    worst = 0.0
    for kind in ('ints', 'gauss'):
        draw = (lambda shape: S.small_ints(rng, shape)) if kind == 'ints' else (lambda shape: rng.standard_normal(shape).astype(np.float32))
        x, K, b = draw((n, c_total, h, w)), draw(ks + (c, dm)), draw((c * dm,))
        sx, sk, sb = Slab(x, align), Slab(K, align), Slab(b, align)
        if not fits or ho < 1 or wo < 1:
            sy = Slab(None, align, (n, z_total, max(ho, 1), max(wo, 1)))
            with pytest.raises(Exception, match='halo' if not fits else 'larger than the padded input'):
                ops.depthwise2d(sx.t, sk.t, sb.t, d, out=sy.t)
            sdx = Slab(None, align, (n, c_total, h, w))
            with pytest.raises(Exception, match='halo' if not fits else 'larger than the padded input'):
                ops.depthwise2d_bwd_data(sy.t, sk.t, d, h, w, out=sdx.t)
            assert sy.unchanged() and sdx.unchanged() and sx.unchanged(), what
            return None
        xw = x[:, c_off:c_off + c].astype(np.float64)
        K64, b64 = K.astype(np.float64), b.astype(np.float64)
        # forward (bias, linear): every element of the window written, the other channels stay NaN
        sy = Slab(None, align, (n, z_total, ho, wo))
        ops.depthwise2d(sx.t, sk.t, sb.t, d, out=sy.t)
        y = sy.read()
        want = S.depthwise(xw, K64, b64, pad, modes, dil)
        got = y[:, z_off:z_off + c * dm]
        rest = np.delete(y, np.s_[z_off:z_off + c * dm], axis=1)
        assert np.isnan(rest).all() and not np.isnan(got).any(), what
        if kind == 'ints':
            assert same_bits(got, want.astype(np.float32)), ('fwd', what)
        else:
            worst = max(worst, _within(got, want, ks[0] * ks[1] + 1, S.depthwise(np.abs(xw), np.abs(K64), np.abs(b64), pad, modes, dil),
                                       ('fwd', what)))
        if n == 3:          # a sample's bits do not depend on the batch it rides in
            s1 = Slab(None, align, (1, z_total, ho, wo))
            ops.depthwise2d(Slab(x[1:2], align).t, sk.t, sb.t, d, out=s1.t)
            assert same_bits(s1.read()[:, z_off:z_off + c * dm], got[1:2]), ('fwd batch', what)
        # data gradient: the window overwritten (it starts as NaN), the other channels untouched
        dz = draw((n, z_total, ho, wo))
        sdz, sdx = Slab(dz, align), Slab(None, align, (n, c_total, h, w))
        ops.depthwise2d_bwd_data(sdz.t, sk.t, d, h, w, out=sdx.t)
        dx = sdx.read()
        dzw = dz[:, z_off:z_off + c * dm].astype(np.float64)
        want = S.depthwise_bwd_data(dzw, K64, pad, modes, dil, h, w)
        got = dx[:, c_off:c_off + c]
        assert np.isnan(np.delete(dx, np.s_[c_off:c_off + c], axis=1)).all() and not np.isnan(got).any(), what
        if kind == 'ints':
            assert same_bits(got + 0.0, want.astype(np.float32) + 0.0), ('bwd_data', what)
        else:
            terms = S.depthwise_bwd_data(np.ones_like(dzw), np.ones_like(K64), pad, modes, dil, h, w)
            worst = max(worst, _within(got, want, terms, S.depthwise_bwd_data(np.abs(dzw), np.abs(K64), pad, modes, dil, h, w),
                                       ('bwd_data', what)))
        if n == 3:
            s1 = Slab(None, align, (1, c_total, h, w))
            ops.depthwise2d_bwd_data(Slab(dz[1:2], align).t, sk.t, d, h, w, out=s1.t)
            assert same_bits(s1.read()[:, c_off:c_off + c], got[1:2]), ('bwd_data batch', what)
        # weight gradient: overwritten, the same bits on a second run, accumulate = the float32 sum
        sdk = Slab(None, align, ks + (c, dm))
        ops.depthwise2d_bwd_weight(sx.t, sdz.t, sdk.t, d)
        dk = sdk.read()
        want = S.depthwise_bwd_weight(xw, dzw, pad, modes, dil, ks)
        if kind == 'ints':
            assert same_bits(dk + 0.0, want.astype(np.float32) + 0.0), ('bwd_weight', what)
        else:
            worst = max(worst, _within(dk, want, n * ho * wo, S.depthwise_bwd_weight(np.abs(xw), np.abs(dzw), pad, modes, dil, ks),
                                       ('bwd_weight', what)))
            again = Slab(None, align, ks + (c, dm))
            ops.depthwise2d_bwd_weight(sx.t, sdz.t, again.t, d)
            assert same_bits(again.read(), dk), ('bwd_weight twice', what)
            old = draw(ks + (c, dm))
            acc = Slab(old, align)
            ops.depthwise2d_bwd_weight(sx.t, sdz.t, acc.t, d, accumulate=True)
            assert same_bits(acc.read(), old + dk), ('bwd_weight accumulate', what)
        assert sx.unchanged() and sk.unchanged() and sb.unchanged() and sdz.unchanged(), what
    return worst


@pytest.mark.parametrize('pad', S.DW_HALOS)
def test_depthwise_kernels_on_every_map_under_every_mode_pair(ops, pad):
    """3 x 3 taps; dilation, depth multiplier and alignment cycle through their values over the 25 mode pairs x 13 maps"""
    rng = np.random.default_rng(sum(pad) + 1)
    worst, ran, k = 0.0, 0, 0
    for n, c, h, w in S.DW_MAPS:
        for modes in S.MODE_PAIRS:
            if (h, w) == (37, 70) and modes[0] != modes[1] and pad != (1, 0, 0, 3):      # (the large map: 5 + 20 pairs in all)
                continue
            dl = S.DW_DILATIONS[k % 2]
            r = _dw_case(ops, rng, n, c, h, w, (3, 3), (dl, dl), S.DW_MULTIPLIERS[k % 3], pad, modes, align=k % 4)
            k += 1
            if r is not None:
                worst, ran = max(worst, r), ran + 1
    assert ran >= 50
    print('\nMEASURED depthwise kernels, halo %r: %d geometries ran, worst error / bound %.3f' % (pad, ran, worst))


@pytest.mark.parametrize('ks', S.DW_KERNELS, ids=lambda k: '%dx%d' % k)
def test_depthwise_kernels_for_every_kernel_dilation_and_multiplier(ops, ks):
    """maps 5 x 7, 7 x 9 (3 samples of 5 channels: the 8-row tile) and 37 x 70 (more than one 32 x 64 tile on both axes, ragged last tiles); the wrap +
    zero halo of 2 of the U-Net and no halo"""
    rng = np.random.default_rng(10 * ks[0] + ks[1])
    worst, ran, k = 0.0, 0, 0
    for n, c, h, w in ((3, 5, 5, 7), (3, 5, 7, 9), (2, 3, 37, 70)):
        for dil in S.DW_DILATIONS:
            for dm in S.DW_MULTIPLIERS:
                for pad, modes in (((2, 2, 2, 2), (S.ZERO, S.WRAP)), ((0, 0, 0, 0), (S.ZERO, S.ZERO))):
                    r = _dw_case(ops, rng, n, c, h, w, ks, (dil, dil), dm, pad, modes, align=k % 4)
                    k += 1
                    if r is not None:
                        worst, ran = max(worst, r), ran + 1
    assert ran >= 24
    print('\nMEASURED depthwise kernels %r: %d geometries ran, worst error / bound %.3f' % (ks, ran, worst))


def test_depthwise_kernels_through_channel_windows(ops):
    """channels [2, 2 + c) of 8 on the input side, [2, 2 + c dm) of 8 on the output side: the rest of both tensors stays NaN"""
    rng = np.random.default_rng(77)
    for dm in S.DW_MULTIPLIERS:
        for align in range(4):
            assert _dw_case(ops, rng, 3, 2, 7, 9, (3, 3), (1, 1), dm, (1, 0, 0, 3), (S.REFLECT, S.WRAP), align=align, c_off=2,
                            c_total=8, z_total=8) is not None


def test_depthwise_weight_gradient_over_several_partials(ops):
    """2 x 37 x 70 = 5180 positions: two first-stage partials of 4096"""
    assert S.dw_partials(2, 37, 70) == 2 and S.dw_partials(3, 7, 9) == 1
    assert _dw_case(ops, np.random.default_rng(5), 2, 3, 37, 70, (3, 3), (1, 1), 2, (1, 1, 1, 1), (S.EDGE, S.WRAP)) is not None
    # 12 x 70: the 16-row tile of the forward, ragged on both axes
    assert _dw_case(ops, np.random.default_rng(6), 1, 2, 12, 70, (3, 3), (2, 2), 1, (2, 2, 2, 2), (S.SYMMETRIC, S.WRAP), align=3) is not None
    assert _dw_case(ops, np.random.default_rng(7), 1, 2, 12, 70, (5, 2), (1, 1), 2, (2, 2, 0, 1), (S.ZERO, S.REFLECT), align=1) is not None


# ----------------------------------------------------------------------------------------------------------------------- #
# 2. the pointwise product
# ----------------------------------------------------------------------------------------------------------------------- #
def _pw_case(ops, rng, n, q, o, hw, align=0, in_off=0, in_total=None, out_off=0, out_total=None):
    what = (n, q, o, hw, align, in_off, out_off)
    in_total, out_total = in_total or q, out_total or o
    d = ops.make_pointwise(q, o, 0, in_c_off=in_off, out_c_off=out_off)
    worst = 0.0
    for kind in ('ints', 'gauss'):
        draw = (lambda shape: S.small_ints(rng, shape)) if kind == 'ints' else (lambda shape: rng.standard_normal(shape).astype(np.float32))
        x, P, b = draw((n, in_total, hw, 1)), draw((q, o)), draw((o,))
        sx, sp, sb = Slab(x, align), Slab(P, align), Slab(b, align)
        xw, P64, b64 = x[:, in_off:in_off + q, :, 0].astype(np.float64), P.astype(np.float64), b.astype(np.float64)
        sy = Slab(None, align, (n, out_total, hw, 1))
        ops.pointwise2d(sx.t, sp.t, sb.t, d, out=sy.t)
        y = sy.read()[..., 0]
        got, want = y[:, out_off:out_off + o], S.pointwise(xw, P64, b64)
        assert np.isnan(np.delete(y, np.s_[out_off:out_off + o], axis=1)).all() and not np.isnan(got).any(), what
        if kind == 'ints':
            assert same_bits(got, want.astype(np.float32)), ('fwd', what)
        else:
            worst = max(worst, _within(got, want, q + 1, S.pointwise(np.abs(xw), np.abs(P64), np.abs(b64)), ('fwd', what)))
        if n == 3:
            s1 = Slab(None, align, (1, out_total, hw, 1))
            ops.pointwise2d(Slab(x[2:3], align).t, sp.t, sb.t, d, out=s1.t)
            assert same_bits(s1.read()[:, out_off:out_off + o, :, 0], got[2:3]), ('fwd batch', what)
        dz = draw((n, out_total, hw, 1))
        sdz, sdx = Slab(dz, align), Slab(None, align, (n, in_total, hw, 1))
        ops.pointwise2d_bwd_data(sdz.t, sp.t, d, out=sdx.t)
        dx = sdx.read()[..., 0]
        dzw = dz[:, out_off:out_off + o, :, 0].astype(np.float64)
        got, want = dx[:, in_off:in_off + q], S.pointwise_bwd_data(dzw, P64)
        assert np.isnan(np.delete(dx, np.s_[in_off:in_off + q], axis=1)).all() and not np.isnan(got).any(), what
        if kind == 'ints':
            assert same_bits(got + 0.0, want.astype(np.float32) + 0.0), ('bwd_data', what)
        else:
            worst = max(worst, _within(got, want, o, S.pointwise_bwd_data(np.abs(dzw), np.abs(P64)), ('bwd_data', what)))
        if n == 3:
            s1 = Slab(None, align, (1, in_total, hw, 1))
            ops.pointwise2d_bwd_data(Slab(dz[2:3], align).t, sp.t, d, out=s1.t)
            assert same_bits(s1.read()[:, in_off:in_off + q, :, 0], got[2:3]), ('bwd_data batch', what)
        sdw = Slab(None, align, (q, o))
        ops.pointwise2d_bwd_weight(sx.t, sdz.t, sdw.t, d)
        dw = sdw.read()
        want = S.pointwise_bwd_weight(xw, dzw)
        if kind == 'ints':
            assert same_bits(dw + 0.0, want.astype(np.float32) + 0.0), ('bwd_weight', what)
        else:
            worst = max(worst, _within(dw, want, n * hw, S.pointwise_bwd_weight(np.abs(xw), np.abs(dzw)), ('bwd_weight', what)))
            again = Slab(None, align, (q, o))
            ops.pointwise2d_bwd_weight(sx.t, sdz.t, again.t, d)
            assert same_bits(again.read(), dw), ('bwd_weight twice', what)
            old = draw((q, o))
            acc = Slab(old, align)
            ops.pointwise2d_bwd_weight(sx.t, sdz.t, acc.t, d, accumulate=True)
            assert same_bits(acc.read(), old + dw), ('bwd_weight accumulate', what)
        assert sx.unchanged() and sp.unchanged() and sb.unchanged() and sdz.unchanged(), what
    return worst


@pytest.mark.parametrize('q', S.PW_Q)
def test_pointwise_kernels_for_every_channel_count_and_map(ops, q):
    rng = np.random.default_rng(q)
    worst, k = 0.0, 0
    for o in S.PW_O:
        for hw in S.PW_HW:
            for n in S.PW_N:
                worst = max(worst, _pw_case(ops, rng, n, q, o, hw, align=k % 4))
                k += 1
    print('\nMEASURED pointwise kernels, q = %d: worst error / bound %.3f' % (q, worst))


def test_pointwise_kernels_through_channel_windows(ops):
    rng = np.random.default_rng(8)
    for align in range(4):
        _pw_case(ops, rng, 3, 3, 4, 35, align=align, in_off=2, in_total=8, out_off=3, out_total=9)
    _pw_case(ops, rng, 1, 33, 35, 990, align=1, in_off=1, in_total=40, out_off=5, out_total=40)


def test_pointwise_weight_gradient_over_several_partials(ops):
    """3 x 990 pixels = 93 units of 32 pixels: six first-stage partials of 16 units (one sample's 31 units straddle two of them); more
    than 128 output channels: a second channel group of the forward"""
    assert S.pw_partials(3, 990) == 6 and S.pw_partials(1, 35) == 1
    _pw_case(ops, np.random.default_rng(9), 3, 64, 64, 990)
    _pw_case(ops, np.random.default_rng(10), 2, 70, 130, 100)


def test_entry_points_refuse_a_window_outside_the_tensor(ops):
    x = torch.zeros((1, 4, 5, 6), device='cuda')
    k = torch.zeros((3, 3, 3, 1), device='cuda')
    with pytest.raises(Exception, match='channel window'):
        ops.depthwise2d(x, k, None, ops.make_depthwise(3, 3, in_c_off=2))
    with pytest.raises(Exception, match='channel window'):
        ops.pointwise2d(x, torch.zeros((3, 2), device='cuda'), None, ops.make_pointwise(3, 2, in_c_off=2))


# ----------------------------------------------------------------------------------------------------------------------- #
# 3. layers and models
# ----------------------------------------------------------------------------------------------------------------------- #
SHAPE = (4, 16, 20)


def _randomise(model, rng):
    """every bias drawn at random, so that all of them are tested"""
    for lay in model.layers:
        if isinstance(lay, L.DepthwiseConv2D) and lay.bias is not None:
            ws = lay.get_weights()
            lay.set_weights(ws[:-1] + [(0.3 * rng.standard_normal(ws[-1].shape)).astype(np.float32)])


def _unet(l2=None):
    """PeriodicPadding2D + ZeroPadding2D halos in front of every 3 x 3 layer, MaxPooling2D, UpSampling2D, concatenate; the 3 x 3
    layers are SeparableConv2D (dilation 1 and 2), one DepthwiseConv2D(3, depth_multiplier=2, tanh) and a 'same' output layer"""
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.regularizers import l2 as l2_reg
    reg = dict(depthwise_regularizer=l2_reg(l2), pointwise_regularizer=l2_reg(l2)) if l2 else {}

    def halo(t, p):
        return L.ZeroPadding2D((p, 0), **CF)(PeriodicPadding2D((0, p), **CF)(t))
    x0 = L.Input(shape=SHAPE)
    e1 = L.SeparableConv2D(8, 3, activation='tanh', name='e1', **dict(CF, **reg))(halo(x0, 1))
    p1 = L.MaxPooling2D(2, **CF)(e1)
    e2 = L.SeparableConv2D(12, 3, dilation_rate=2, depth_multiplier=2, activation='tanh', name='e2', **dict(CF, **reg))(halo(p1, 2))
    dwl = L.DepthwiseConv2D(3, depth_multiplier=2, activation='tanh', name='dw', **CF)(halo(e2, 1))
    up = L.UpSampling2D(2, **CF)(dwl)
    cat = L.concatenate([up, e1], axis=1)
    d1 = L.SeparableConv2D(8, 3, activation='relu', name='d1', **dict(CF, **reg))(halo(cat, 1))
    return x0, L.SeparableConv2D(4, (3, 2), padding='same', use_bias=False, name='out', **CF)(d1)


def _unet_ref(model, x, p):
    """float64 torch restatement of _unet"""
    lay = {l.name: l for l in model.layers}

    def halo(t, k):
        return F.pad(torch.cat([t[..., -k:], t, t[..., :k]], dim=-1), (0, 0, k, k))

    def dwise(t, name, dil=1):
        K = p[(name, 'depthwise_kernel')]
        kh, kw, cin, dm = K.shape
        return F.conv2d(t, K.permute(2, 3, 0, 1).reshape(cin * dm, 1, kh, kw), None, dilation=dil, groups=cin)

    def sep(t, name, dil=1, act=None):
        t = dwise(t, name, dil)
        P = p[(name, 'pointwise_kernel')]
        t = torch.einsum('nqhw,qo->nohw', t, P[0, 0])
        if lay[name].use_bias:
            t = t + p[(name, 'bias')].reshape(1, -1, 1, 1)
        return torch.tanh(t) if act == 'tanh' else (torch.relu(t) if act == 'relu' else t)
    e1 = sep(halo(x, 1), 'e1', act='tanh')
    e2 = sep(halo(F.max_pool2d(e1, 2), 2), 'e2', dil=2, act='tanh')
    dwl = torch.tanh(dwise(halo(e2, 1), 'dw') + p[('dw', 'bias')].reshape(1, -1, 1, 1))
    cat = torch.cat([F.interpolate(dwl, scale_factor=2, mode='nearest'), e1], dim=1)
    d1 = sep(halo(cat, 1), 'd1', act='relu')
    return sep(F.pad(d1, (0, 1, 1, 1)), 'out')               # 'same' for (3, 2): rows (1, 1), columns (0, 1)


def _model(seed=1, l2=None, lr=1e-3):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0, out = _unet(l2)
    m = Model(inputs=x0, outputs=out, seed=seed)
    m.compile(optimizer=Adam(lr=lr), loss='mse')
    _randomise(m, np.random.default_rng(seed + 100))
    return m


def _data(seed, n=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n,) + SHAPE).astype(np.float32), rng.standard_normal((n,) + SHAPE).astype(np.float32)


def test_plan_of_the_unet():
    m = _model()
    kinds = [op.kind for op in m.plan.ops]
    assert kinds.count('dwconv') == 5 and kinds.count('pwconv') == 4 and 'conv' not in kinds
    first = m.plan.ops[0]
    assert first.kind == 'dwconv' and first.src == -1 and tuple(first.halo) == (1, 1, 1, 1, S.ZERO, S.WRAP)      # the halo is consumed


def test_predict_against_float64():
    m = _model()
    x, _ = _data(11)
    with torch.no_grad():
        want = _unet_ref(m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False)).numpy()
    got = m.predict(x)
    assert got.shape == want.shape == (3,) + SHAPE
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print('\nMEASURED U-Net forward: %.3g of max |want|' % err)
    assert err <= FWD_TOL


def test_single_layers_against_float64():
    """'valid' and 'same', every activation, a non-square kernel, with and without a bias, dilation 2, depth multiplier 3"""
    from dlwp_amd.engine import Model
    rng = np.random.default_rng(3)
    for cls in ('sep', 'dw'):
        for padding in ('valid', 'same'):
            for act, ks, dil, dm, bias in (('tanh', (3, 3), 1, 1, True), ('relu', (2, 5), 2, 3, True), (None, (5, 1), 1, 2, False)):
                x0 = L.Input(shape=(3, 11, 13))
                kw = dict(CF, padding=padding, activation=act, dilation_rate=dil, depth_multiplier=dm, use_bias=bias)
                lay = L.SeparableConv2D(5, ks, **kw) if cls == 'sep' else L.DepthwiseConv2D(ks, **kw)
                m = Model(inputs=x0, outputs=lay(x0), seed=4)
                _randomise(m, rng)
                x = rng.standard_normal((2, 3, 11, 13)).astype(np.float32)
                ws = [a.astype(np.float64) for a in lay.get_weights()]
                pad = S.same_halo(ks, (dil, dil)) if padding == 'same' else (0, 0, 0, 0)
                b = ws[-1] if bias else None
                if cls == 'sep':
                    want = S.separable(x.astype(np.float64), ws[0], ws[1], b, pad, dil=(dil, dil), act=act)
                else:
                    want = S.depthwise(x.astype(np.float64), ws[0], b, pad, dil=(dil, dil), act=act)
                got = m.predict(x)
                assert got.shape == want.shape, (cls, padding, ks)
                assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max(), (cls, padding, act, ks)


@pytest.mark.parametrize('l2', [None, 1e-2], ids=['plain', 'l2'])
def test_training_step_against_float64_autograd(monkeypatch, l2):
    """mse, Adam, l2 on both kernels: the loss (TOL) and every gradient entry -- depthwise_kernel, pointwise_kernel, bias -- (BWD_TOL)"""
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model(seed=2, l2=l2)
    x, y = _data(12)
    p = _ref_params(m)
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    val = ((_unet_ref(m, torch.tensor(x, dtype=torch.float64), p) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    if l2:
        val = val + sum(l2 * (p[(lay.name, nm)] ** 2).sum() for lay in m.layers if isinstance(lay, L.SeparableConv2D)
                        for nm in ('depthwise_kernel', 'pointwise_kernel') if lay.depthwise_regularizer is not None)
    val.backward()
    got = _grads_of(m._trainer)
    assert sorted(got) == sorted(p) and len(got) == 4 * 2 + 3 + 2          # four separable layers (one without a bias), one depthwise
    assert sum(1 for k in got if k[1] == 'depthwise_kernel') == 5
    worst = 0.0
    for key, g in sorted(got.items()):
        r = p[key].grad.numpy()
        assert g.shape == r.shape, key
        ratio = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-6))
        worst = max(worst, ratio)
        print('MEASURED   %s/%s gradient error %.3g of its scale' % (key + (ratio,)))
    print('MEASURED step: loss %.8g against %.8g' % (loss, float(val.detach())))
    assert loss == pytest.approx(float(val.detach()), rel=TOL)
    assert worst <= BWD_TOL, worst


def test_first_layer_launches_no_data_gradient(monkeypatch):
    from dlwp_amd import ops as _ops
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model(seed=3)
    calls = []
    real = _ops.depthwise2d_bwd_data
    monkeypatch.setattr(_ops, 'depthwise2d_bwd_data', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m.train_on_batch(*_data(13))
    torch.cuda.synchronize()
    assert len(calls) == 4              # five depthwise stages, the first reads the model input


def _run_steps(monkeypatch, form, batches):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)
    m = _model(seed=5)                      # (no kernel regulariser: a step with one is never replayed)
    logs = [m.train_on_batch(x, y) for x, y in batches]
    torch.cuda.synchronize()
    tr = m._trainer
    if form != 'eager':
        n = batches[0][0].shape[0]
        ents = [e for k, e in tr._graphs.items() if k[0] == n and e.get('step') is not None]
        assert len(ents) == 1, 'the step of %d samples was not recorded (refused: %r)' % (n, tr._no_tape)
    return logs, [w.copy() for w in m.get_weights()], [s.cpu().numpy() for s in tr.opt_state]


def test_replayed_step_equals_the_eager_step(monkeypatch):
    """2 eager steps, then the recorded (and validated) one and 2 replayed ones: nothing marks the tape foreign"""
    batches = [_data(600 + i) for i in range(5)]
    ref = _run_steps(monkeypatch, 'eager', batches)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, form, batches)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
            assert np.array_equal(_bits(a), _bits(b)), form


def test_captured_rollout_equals_the_host_loop():
    from dlwp_amd.model import DLWPFunctional
    m = _model(seed=6)
    d = DLWPFunctional(is_convolutional=True, is_recurrent=False, time_dim=2)
    d.model = d.base_model = m
    x, _ = _data(15, n=5)
    assert d._device_rollout_ok(x)
    kept = d.predict_timeseries(x, 8, keep_time_dim=True)            # one hipGraph of 4 forwards
    state, want = x, []
    for _ in range(4):
        state = m.predict(state)
        want.append(state)
    want = np.stack(want)
    assert np.isfinite(want).all() and kept.shape == (4, 5, 2, 2, 16, 20)
    assert np.array_equal(_bits(kept), _bits(want.reshape(kept.shape)))
    ser = _host(m.rollout_on_device(torch.from_numpy(x).cuda(), 4, graph_cache=False))
    assert np.array_equal(_bits(ser), _bits(want))


@pytest.mark.parametrize('fmt', ['keras', 'npz'])
def test_saved_and_reloaded_model_predicts_and_trains_the_same_bits(tmp_path, monkeypatch, fmt):
    from dlwp_amd import serialization
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    batches = [_data(800 + i) for i in range(4)]
    m = _model(seed=7, l2=1e-3)
    for x, y in batches[:2]:
        m.train_on_batch(x, y)
    path = str(tmp_path / ('m.%s' % fmt))
    m.save(path, format=fmt)
    m2 = serialization.load_model_file(path)
    assert [type(lay).__name__ for lay in m2.layers] == [type(lay).__name__ for lay in m.layers]
    assert [lay.get_config() for lay in m2.layers] == [lay.get_config() for lay in m.layers]
    assert [getattr(lay.depthwise_regularizer, 'l2', None) for lay in m2.layers if isinstance(lay, L.SeparableConv2D)] == \
        [getattr(lay.depthwise_regularizer, 'l2', None) for lay in m.layers if isinstance(lay, L.SeparableConv2D)]
    assert np.array_equal(_bits(m2.predict(batches[0][0])), _bits(m.predict(batches[0][0])))
    for x, y in batches[2:]:
        a, b = m.train_on_batch(x, y), m2.train_on_batch(x, y)
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(_bits(a), _bits(b))


def test_bfloat16_activation_storage_is_refused():
    m = _model(seed=8)
    with pytest.raises(NotImplementedError, match='DepthwiseConv2D / SeparableConv2D.*e1'):
        m.set_activation_dtype('bfloat16')
    assert m.activation_dtype == 'float32'
    x, _ = _data(33)
    assert np.isfinite(m.predict(x)).all()


# ----------------------------------------------------------------------------------------------------------------------- #
# build_model(gpus > 1)
# ----------------------------------------------------------------------------------------------------------------------- #
DP_SPECS = (('PeriodicPadding2D', ((0, 1),), dict(CF, input_shape=SHAPE)),
            ('ZeroPadding2D', ((1, 0),), dict(CF)),
            ('SeparableConv2D', (8, 3), dict(CF, activation='tanh', depth_multiplier=2)),
            ('DepthwiseConv2D', (3,), dict(CF, padding='same', activation='tanh')),
            ('SeparableConv2D', (4, 3), dict(CF, padding='same', dilation_rate=2)))


def _dp_build(gpus=None):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.training import Adam
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(DP_SPECS, loss='mse', optimizer=Adam(lr=1e-3), **({'gpus': gpus} if gpus else {}))
    return d


def _dp_worker(rank, world, port, ret):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DLWP_SHARE_GPUS='1', DLWP_DIST_BACKEND='gloo')
    from dlwp_amd import parallel
    parallel.init()
    np.random.seed(1000 + 17 * rank)            # different initial weights per rank: compile aligns them on rank 0's
    d = _dp_build(world)
    w0 = [w.copy() for w in d.model.get_weights()]
    x, y = _data(21, n=8)
    logs = [np.atleast_1d(d.model.train_on_batch(x, y)).tolist() for _ in range(3)]
    torch.cuda.synchronize()
    ret[rank] = {'w0': w0, 'w1': d.model.get_weights(), 'logs': logs}
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_training_equals_the_single_process_run():
    """build_model(gpus=2), two ranks on one GPU: tolerances of tests/test_gpu_sconv.py::test_two_rank_training_equals_the_single_process_run"""
    import multiprocessing as mp
    from tests.test_gpu_parallel import _free_port
    port = _free_port()
    ctx = mp.get_context('spawn')
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, ret)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            if p.is_alive():
                p.kill()
                pytest.fail('data-parallel worker timed out')
            assert p.exitcode == 0, 'data-parallel worker failed'
        res = dict(ret)
    for a, b in zip(res[0]['w0'] + res[0]['w1'], res[1]['w0'] + res[1]['w1']):
        assert np.array_equal(a, b)
    assert res[0]['logs'] == res[1]['logs']
    d = _dp_build()
    assert [op.kind for op in d.model.plan.ops] == ['dwconv', 'pwconv', 'dwconv', 'dwconv', 'pwconv']
    d.model.set_weights(res[0]['w0'])
    x, y = _data(21, n=8)
    logs = [np.atleast_1d(d.model.train_on_batch(x, y)).tolist() for _ in range(3)]
    for got, want in zip(res[0]['logs'], logs):
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (got, want)
    for a, b in zip(res[0]['w1'], d.model.get_weights()):
        # identical mathematics, two half-batch gradients against one: float32 round-off per step (tests/test_gpu_parallel.py)
        assert np.abs(a - b).max() <= 1e-6 * 3, np.abs(a - b).max()
