"""Conv2D(strides=2) on the GPU (csrc/sconv.hip through every layer of the stack).

Kernels: the weight map and its gather, the padded space-to-depth pass and -- under zero halos -- its adjoint are BIT-EQUAL to the
numpy restatements of tests/sconv_cases.py (they move and zero-fill, nothing is rounded); the adjoint under summing halos is held
to the order-free float32 summation bound (m - 1) 2^-24 sum |terms| of the float64 restatement, so no sum order is pinned.  All run
on guarded slabs whose outputs start as NaN: an element a kernel does not write shows, and so does one it writes outside.  The
fused pass has the bits of dlwp_pad2d_fwd followed by dlwp_space_to_depth2_fill.

Layers: the forward against float64 torch conv2d(stride=2) at the project's float32 parity bar, max |got - want| <= 1e-5 max |want|
(FWD_TOL); one training step of a strided encoder / transposed decoder against float64 torch autograd (TOL, BWD_TOL
as tests/test_gpu_tconv.py imports them); the replayed step against the eager one, the captured rollout against the host loop
and model files in both formats, bit for bit; the ConvLSTM2D network examples/train_generator.py of the reference carries, at
reduced size; two data-parallel ranks against one process; the bfloat16 storage mode is refused."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from tests import sconv_cases as S
from tests.test_gpu_batchnorm import _bits, _grads_of, _host, _ref_params
from tests.test_gpu_convlstm_bwd import BWD_TOL
from tests.test_gpu_dense import TOL
from tests.test_gpu_train_ops import Slab, cu_count, same_bits

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
FWD_TOL = 1e-5          # the project's float32 parity bar, as tests/test_gpu_tconv.py uses it
MODE_PAIRS = [(mh, mw) for mh in S.MODES for mw in S.MODES]          # the pairs tests/test_gpu_halo.py runs dlwp_pad2d_fwd on
ELEMENT_MAPS = [(1, 1), (2, 3), (5, 4), (7, 6)]
VECTOR_MAPS = [(4, 8), (8, 16)]
HALOS = [(0, 0, 0, 0), (2, 2, 2, 2), (1, 0, 0, 3)]
U = 2.0 ** -24


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ----------------------------------------------------------------------------------------------------------------------- #
# 1. weight map and its adjoint
# ----------------------------------------------------------------------------------------------------------------------- #
def test_weight_map_and_its_adjoint_are_bit_equal(ops):
    rng = np.random.default_rng(1)
    for kh, kw in S.KERNELS:
        th, tw = (kh + 1) // 2, (kw + 1) // 2
        for cin in (1, 3):
            for f in (1, 4):
                K = rng.standard_normal((kh, kw, cin, f)).astype(np.float32)
                for taps in ((th, tw), (3, 3), (5, 5)):                           # T x T, 3 x 3, 5 x 5
                    if taps[0] < th or taps[1] < tw:
                        continue
                    w2 = _nan(taps[0], taps[1], 4 * cin, f)
                    ops.sconv_weights(_dev(K), w2=w2)
                    assert same_bits(_host(w2), S.weight_map(K, taps)), (kh, kw, cin, f, taps)
                    g2 = rng.standard_normal(tuple(w2.shape)).astype(np.float32)
                    gather = S.weight_map_bwd(g2, K.shape)
                    dk = _nan(kh, kw, cin, f)
                    ops.sconv_weights_bwd(_dev(g2), dk)                           # accumulate = 0: a NaN target is overwritten
                    assert same_bits(_host(dk), gather), (kh, kw, cin, f, taps)
                    dw = rng.standard_normal(K.shape).astype(np.float32)
                    dk = _dev(dw)
                    ops.sconv_weights_bwd(_dev(g2), dk, accumulate=True)          # accumulate = 1: the float32 sum dw + gather
                    assert same_bits(_host(dk), dw + gather), (kh, kw, cin, f, taps)
    # more elements than one pass of the 4096-workgroup grid
    K = rng.standard_normal((5, 5, 256, 128)).astype(np.float32)
    w2 = ops.sconv_weights(_dev(K), taps=(3, 3))
    assert w2.numel() > 4096 * 256 and same_bits(_host(w2), S.weight_map(K, (3, 3)))
    g2 = rng.standard_normal(tuple(w2.shape)).astype(np.float32)
    dk = _nan(*K.shape)
    ops.sconv_weights_bwd(_dev(g2), dk)
    assert same_bits(_host(dk), S.weight_map_bwd(g2, K.shape))
    with pytest.raises(ValueError):
        ops.sconv_weights_bwd(_dev(g2[:2]), dk)
    with pytest.raises(ValueError):
        ops.sconv_weights(_dev(K), w2=_nan(3, 3, 64, 512))


# ----------------------------------------------------------------------------------------------------------------------- #
# 2. - 4. the padded space-to-depth pass and its adjoint
# ----------------------------------------------------------------------------------------------------------------------- #
def _fits(pad, modes, h, w):
    return S.pad_fits(pad[0], pad[1], h, modes[0]) and S.pad_fits(pad[2], pad[3], w, modes[1])


def _s2d_case(ops, rng, n, c, h, w, pad, modes, hp, wp, align=0, c_off=0, c_total=None, unfused=False):
    """dlwp_space_to_depth2_pad and its adjoint on guarded slabs `align` floats past a 16-byte boundary, against numpy.  Returns the
    worst error / bound of the adjoint's sums (0 where nothing is summed)."""
    c_total = c_total or c
    what = (n, c, h, w, pad, modes, hp, wp, align, c_off, c_total)
    x = rng.standard_normal((n, c_total, h, w)).astype(np.float32)
    s_in, s_out = Slab(x, align), Slab(None, align, (n, 4 * c, hp, wp))                # NaN: every element must be written
    d = ops.make_pad(*pad, *modes)
    if not _fits(pad, modes, h, w):                                                     # a map too small for this mode's halo
        with pytest.raises(Exception, match='halo'):
            ops.space_to_depth2_pad(s_in.t, c, d, hp, wp, c_off=c_off, out=s_out.t)
        with pytest.raises(Exception, match='halo'):
            ops.space_to_depth2_pad_bwd(s_out.t, c, h, w, d, out=s_in.t, c_off=c_off)
        assert s_in.unchanged() and np.isnan(s_out.read()).all(), what
        return None
    ops.space_to_depth2_pad(s_in.t, c, d, hp, wp, c_off=c_off, out=s_out.t)
    got = s_out.read()
    want = S.s2d_pad(x[:, c_off:c_off + c], pad, modes, hp, wp)
    assert same_bits(got, want), what
    assert s_in.unchanged(), what
    if unfused:              # the parent commit's kernels: dlwp_pad2d_fwd, then dlwp_space_to_depth2_fill(top = left = 0)
        padded = ops.pad2d(_dev(x[:, c_off:c_off + c]), d)
        two = ops.space_to_depth2_fill(padded, c, hp, wp, 0, 0, out=_nan(n, 4 * c, hp, wp))
        assert same_bits(got, _host(two)), what
    # the adjoint, into the layer's channel window of a NaN tensor: the window is written, nothing else
    g = rng.standard_normal((n, 4 * c, hp, wp)).astype(np.float32)
    s_g, s_dx = Slab(g, align), Slab(None, align, (n, c_total, h, w))
    ops.space_to_depth2_pad_bwd(s_g.t, c, h, w, d, out=s_dx.t, c_off=c_off)
    got = s_dx.read()
    assert s_g.unchanged(), what
    assert np.isnan(np.delete(got, np.s_[c_off:c_off + c], axis=1)).all(), what          # the other channels stay untouched
    got = got[:, c_off:c_off + c]
    if modes == (S.ZERO, S.ZERO):
        assert same_bits(got, S.s2d_pad_bwd(g, pad, modes, h, w)), what                  # one term per element: bit-equal
        return 0.0
    want, cnt, mag = S.s2d_pad_bwd(g.astype(np.float64), pad, modes, h, w, stats=True)
    assert same_bits(got[:, :, cnt == 0], np.zeros_like(got[:, :, cnt == 0])), what      # no term: exactly +0
    one = cnt == 1
    assert same_bits(got[:, :, one], want[:, :, one].astype(np.float32)), what           # one term: that term
    bound = (np.maximum(cnt, 1) - 1)[None, None] * U * mag
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (what, float((err - bound).max()))
    many = bound > 0
    return float((err[many] / bound[many]).max()) if many.any() else 0.0


def _cover(h, w, pad):
    """(hp, wp) that just covers the padded image"""
    return (h + pad[0] + pad[1] + 1) // 2, (w + pad[2] + pad[3] + 1) // 2


@pytest.mark.parametrize('halo', HALOS, ids=['none', 'halo2', 'asymmetric'])
def test_space_to_depth_pad_and_its_adjoint_every_mode_pair(ops, halo):
    """maps 1 x 1 ... 7 x 6 (element route), 4 x 8 and 8 x 16 (16-byte route where the left halo is a multiple of 4), n = 1 and 3,
    all 25 mode pairs; a pair whose halo the map is too small for is refused.  The fused pass has the bits of the two launches."""
    rng = np.random.default_rng(2)
    worst, k, refused = 0.0, 0, 0
    pairs = MODE_PAIRS if any(halo) else [(S.ZERO, S.ZERO), (S.WRAP, S.REFLECT)]          # (no halo: the modes do nothing)
    for h, w in ELEMENT_MAPS + VECTOR_MAPS:
        for modes in pairs:
            n, k = (1, 3)[k % 2], k + 1
            hp, wp = _cover(h, w, halo)
            r = _s2d_case(ops, rng, n, 2, h, w, halo, modes, hp, wp, unfused=any(halo))
            refused += r is None
            worst = max(worst, r or 0.0)
    assert not any(halo) or refused > 0                                                  # (1 x 1 under a wrap / mirror halo)
    print('\nMEASURED adjoint under halo %r: worst error / bound %.3g' % (halo, worst))


def test_space_to_depth_pad_vector_route_windows_alignment_and_large_launches(ops):
    rng = np.random.default_rng(3)
    worst = 0.0
    for h, w in VECTOR_MAPS:
        for pad in ((0, 0, 0, 0), (0, 1, 0, 1), (1, 1, 4, 4), (2, 0, 4, 0), (1, 0, 0, 3)):
            for modes in ((S.ZERO, S.ZERO), (S.ZERO, S.WRAP), (S.EDGE, S.SYMMETRIC), (S.REFLECT, S.EDGE), (S.WRAP, S.ZERO)):
                hp, wp = _cover(h, w, pad)
                wp4 = (wp + 3) // 4 * 4                            # 16-byte route: wp % 4 == 0 (reaches beyond the padded image)
                for n, c in ((1, 2), (3, 3)):
                    for align in (0, 1):                           # ... and the same geometry one float off: element route
                        r = _s2d_case(ops, rng, n, c, h, w, pad, modes, hp, wp4, align=align, unfused=True)
                        worst = max(worst, r or 0.0)
                # one row / column beyond the padded image (+0 there), and one short of it
                _s2d_case(ops, rng, 2, 2, h, w, pad, modes, hp + 1, wp + 1, unfused=True)
                if hp > 1 and wp > 1:
                    _s2d_case(ops, rng, 2, 2, h, w, pad, modes, hp - 1, wp - 1)
    for h, w in ELEMENT_MAPS:
        for pad in HALOS:
            hp, wp = _cover(h, w, pad)
            _s2d_case(ops, rng, 2, 2, h, w, pad, (S.ZERO, S.EDGE), hp + 1, wp + 1, unfused=True)
    # a channel window of a wider tensor (a slice_layer in front), both routes
    for h, w in ((7, 6), (8, 16)):
        for pad, modes in (((0, 0, 0, 0), (S.ZERO, S.ZERO)), ((2, 2, 2, 2), (S.ZERO, S.WRAP)), ((0, 1, 4, 4), (S.ZERO, S.ZERO))):
            hp, wp = _cover(h, w, pad)
            _s2d_case(ops, rng, 3, 3, h, w, pad, modes, hp, (wp + 3) // 4 * 4, c_off=1, c_total=5)
    # more work than one pass of the capped grid (16 workgroups of 256 lanes per CU), every kernel
    per_pass = cu_count() * 16 * 256
    n, c, h, w = 2, 4, 1024, 1280
    assert n * c * 2 * (h // 2) * (w // 8) > per_pass and n * c * h * (w // 8) > per_pass
    _s2d_case(ops, rng, n, c, h, w, (0, 0, 0, 0), (S.ZERO, S.ZERO), h // 2, w // 2)               # 16-byte routes
    n, c, h, w = 3, 2, 1200, 601
    assert n * c * (h // 2 + 1) * (w // 2 + 2) > per_pass
    r = _s2d_case(ops, rng, n, c, h, w, (2, 0, 2, 2), (S.ZERO, S.WRAP), h // 2 + 1, w // 2 + 3)   # element routes
    print('\nMEASURED adjoint, vector-route geometries: worst error / bound %.3g (large wrap launch %.3g)' % (worst, r))


def test_null_pointers_and_bad_windows_are_refused_with_a_handle(ops):
    from dlwp_amd import _lib
    lib = _lib.lib
    h = _lib.handle(torch.cuda.current_device())
    x = _dev(np.zeros((1, 3, 6, 8)))
    none = ops.make_pad(0, 0, 0, 0, 0, 0)
    for fn, name in ((lib.dlwp_space_to_depth2_pad, 'dlwp_space_to_depth2_pad'),
                     (lib.dlwp_space_to_depth2_pad_bwd, 'dlwp_space_to_depth2_pad_bwd')):
        for a, b in ((None, x.data_ptr()), (x.data_ptr(), None)):
            assert fn(h, a, b, 1, 3, 6, 8, none, 3, 4, 0, 3, _lib.F32, None) != 0
            assert (name + ': null pointer') in lib.dlwp_last_error().decode()
        assert fn(h, None, None, 0, 3, 6, 8, none, 3, 4, 0, 3, _lib.F32, None) == 0       # an empty batch has no pointers
    for fn, name in ((lib.dlwp_sconv_weights, 'dlwp_sconv_weights'),):
        assert fn(h, None, x.data_ptr(), 3, 3, 4, 2, 3, 3, _lib.F32, None) != 0
        assert (name + ': null pointer') in lib.dlwp_last_error().decode()
    assert lib.dlwp_sconv_weights_bwd(h, x.data_ptr(), None, 3, 3, 4, 2, 3, 3, 0, _lib.F32, None) != 0
    assert 'dlwp_sconv_weights_bwd: null pointer' in lib.dlwp_last_error().decode()
    with pytest.raises(Exception, match='channel window'):
        ops.space_to_depth2_pad(x, 3, none, 3, 4, c_off=1)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------- #
# 5. the layer's forward
# ----------------------------------------------------------------------------------------------------------------------- #
def _randomise(model, rng):
    """every bias drawn at random, so that all of them are tested"""
    for lay in model.layers:
        if isinstance(lay, (L.Conv2D, L.Conv2DTranspose)) and lay.bias is not None:
            k, b = lay.get_weights()
            lay.set_weights([k, (0.3 * rng.standard_normal(b.shape)).astype(np.float32)])


@pytest.mark.parametrize('padding', S.PADDINGS)
@pytest.mark.parametrize('k', [1, 2, 3, 4, 5])
def test_forward_against_float64_strided_convolution(k, padding):
    from dlwp_amd.engine import Model
    rng = np.random.default_rng(10 * k + len(padding))
    worst = 0.0
    for h, w in [(6, 7), (9, 12), (8, 16)]:
        x = (2.0 * rng.standard_normal((3, 3, h, w))).astype(np.float32)
        for use_bias in (True, False):
            for act in ('linear', 'tanh', 'relu'):
                x0 = L.Input(shape=(3, h, w))
                lay = L.Conv2D(2, k, strides=2, padding=padding, activation=act, use_bias=use_bias, **CF)
                m = Model(inputs=x0, outputs=lay(x0), seed=k)
                _randomise(m, rng)
                ws = [a.astype(np.float64) for a in lay.get_weights()]
                want = S.reference(x.astype(np.float64), ws[0], ws[1] if use_bias else None, padding, act)
                got = m.predict(x)
                assert got.shape == want.shape == (3, 2) + tuple(lay.compute_output_shape((3, h, w))[1:])
                err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
                worst = max(worst, err / scale)
                assert err <= FWD_TOL * scale, (h, w, use_bias, act, err, scale)
    print('\nMEASURED Conv2D(k=%d, strides=2, %s) forward: worst error %.3g of the scale' % (k, padding, worst))


def test_forward_of_the_references_padded_block():
    """PeriodicPadding2D((0, 2)) -> ZeroPadding2D((2, 0)) -> Conv2D(., 5, strides=2): the halo rides in the space-to-depth pass"""
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.engine import Model
    rng = np.random.default_rng(9)
    for h, w in [(6, 7), (9, 12), (8, 16)]:
        for padding in S.PADDINGS:
            for act in ('linear', 'tanh', 'relu'):
                x0 = L.Input(shape=(3, h, w))
                lay = L.Conv2D(4, 5, strides=2, padding=padding, activation=act, **CF)
                m = Model(inputs=x0, outputs=lay(L.ZeroPadding2D((2, 0), **CF)(PeriodicPadding2D((0, 2), **CF)(x0))), seed=3)
                _randomise(m, rng)
                kinds = [op.kind for op in m.infer_plan.ops]
                assert kinds == (['sphasew', 's2dp', 'conv'] if padding == 'valid' else ['pad', 'sphasew', 's2dp', 'conv'])
                x = (2.0 * rng.standard_normal((3, 3, h, w))).astype(np.float32)
                ws = [a.astype(np.float64) for a in lay.get_weights()]
                xp = S.pad_np(x.astype(np.float64), (2, 2, 2, 2), (S.ZERO, S.WRAP))
                want = S.reference(xp, ws[0], ws[1], padding, act)
                got = m.predict(x)
                assert got.shape == want.shape
                assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max(), (h, w, padding, act)


# ----------------------------------------------------------------------------------------------------------------------- #
# 6. models
# ----------------------------------------------------------------------------------------------------------------------- #
def _net(l2=None):
    """(a) Conv2D(8, 3, strides=2, 'same', tanh) -> Conv2D(8, 3, 'same') -> Conv2DTranspose(4, 4, strides=2, 'same') on 4 x 8 x 12:
    a strided encoder / transposed decoder that returns the input's shape (a state a rollout can feed back)"""
    from dlwp_amd.regularizers import l2 as l2_reg
    reg = dict(kernel_regularizer=l2_reg(l2)) if l2 else {}
    x0 = L.Input(shape=(4, 8, 12))
    t = L.Conv2D(8, 3, strides=2, padding='same', activation='tanh', **dict(CF, **reg))(x0)
    t = L.Conv2D(8, 3, padding='same', **CF)(t)
    return x0, L.Conv2DTranspose(4, 4, strides=2, padding='same', **dict(CF, **reg))(t)


def _net_ref(model, x, p):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    up = [lay for lay in model.layers if isinstance(lay, L.Conv2DTranspose)][0]
    # 'same', k = 3, stride 2 on 8 x 12: one zero row below and one zero column to the right (TensorFlow: the smaller half first)
    t = torch.tanh(F.conv2d(F.pad(x, (0, 1, 0, 1)), p[(convs[0].name, 'kernel')], p[(convs[0].name, 'bias')], stride=2))
    t = F.conv2d(t, p[(convs[1].name, 'kernel')], p[(convs[1].name, 'bias')], padding=1)
    t = F.conv_transpose2d(t, p[(up.name, 'kernel')], p[(up.name, 'bias')], stride=2)
    return t[:, :, 1:-1, 1:-1]                               # 'same' for k = 4: rows / columns [1, 1 + 2h) of the full result


def _model(seed=1, l2=None, lr=1e-3):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0, out = _net(l2)
    m = Model(inputs=x0, outputs=out, seed=seed)
    m.compile(optimizer=Adam(lr=lr), loss='mse')
    _randomise(m, np.random.default_rng(seed + 100))
    return m


def _data(seed, n=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 4, 8, 12)).astype(np.float32), rng.standard_normal((n, 4, 8, 12)).astype(np.float32))


def _check_step(m, ref, x, y, p, l2=None):
    """one train_on_batch against float64 autograd: the loss (TOL) and the gradient of every kernel and bias (BWD_TOL)"""
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    val = ((ref(torch.tensor(x, dtype=torch.float64)) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    if l2:
        val = val + sum(l2 * (p[(lay.name, 'kernel')] ** 2).sum() for lay in m.layers
                        if getattr(lay, 'kernel_regularizer', None) is not None)
    val.backward()
    print('\nMEASURED step: loss %.8g against %.8g' % (loss, float(val.detach())))
    got = _grads_of(m._trainer)
    assert len(got) == sum(1 for t in p.values() if t.requires_grad) == 2 * sum(1 for lay in m.layers if lay._weights)
    worst = 0.0
    for (lname, nm), g in sorted(got.items()):
        r = p[(lname, nm)].grad.numpy()
        r = r.transpose(2, 3, 1, 0) if nm == 'kernel' else r        # OIHW -> HWIO; (cin, F, kh, kw) -> (kh, kw, F, cin)
        assert g.shape == r.shape, (lname, nm)
        ratio = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-6))
        worst = max(worst, ratio)
        print('MEASURED   %s/%s gradient error %.3g of its scale' % (lname, nm, ratio))
    assert loss == pytest.approx(float(val.detach()), rel=TOL)
    assert worst <= BWD_TOL, worst


def test_predict_of_the_encoder_decoder_against_float64():
    m = _model()
    assert [op.kind for op in m.infer_plan.ops][:3] == ['sphasew', 's2dp', 'conv']
    x, _ = _data(11)
    with torch.no_grad():
        want = _net_ref(m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False)).numpy()
    got = m.predict(x)
    assert got.shape == want.shape == (3, 4, 8, 12)
    assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()


@pytest.mark.parametrize('l2', [None, 1e-2], ids=['plain', 'l2'])
def test_training_step_against_float64_autograd(monkeypatch, l2):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model(seed=2, l2=l2)
    assert [op.kind for op in m.plan.ops] == ['sphasew', 's2dp', 'conv', 'conv', 'tphasew', 'conv', 'd2sc']
    x, y = _data(12)
    p = _ref_params(m)
    _check_step(m, lambda xt: _net_ref(m, xt, p), x, y, p, l2=l2)


@pytest.mark.parametrize('fused', ['0', '1'], ids=['two-launches', 'fused'])
def test_training_step_with_the_halo_in_front_against_float64_autograd(monkeypatch, fused):
    """the adjoint of the padded space-to-depth pass under a periodic halo (its sums), behind a layer that needs the data gradient:
    as the backward pass takes it by default (dlwp_depth_to_space2_crop + dlwp_pad2d_bwd: the phase tensor covers the padded image)
    and through the fused gather (DLWP_SCONV_FUSED_ADJOINT=1)"""
    monkeypatch.setenv('DLWP_SCONV_FUSED_ADJOINT', fused)
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    x0 = L.Input(shape=(3, 9, 12))
    c1, c2 = L.Conv2D(5, 3, padding='same', activation='tanh', **CF), L.Conv2D(4, 5, strides=2, activation='tanh', **CF)
    m = Model(inputs=x0, outputs=c2(L.ZeroPadding2D((2, 0), **CF)(PeriodicPadding2D((0, 2), **CF)(c1(x0)))), seed=3)
    m.compile(optimizer=Adam(lr=1e-3), loss='mse')
    assert [op.kind for op in m.plan.ops] == ['conv', 'sphasew', 's2dp', 'conv']
    _randomise(m, np.random.default_rng(6))
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((3, 3, 9, 12)).astype(np.float32), rng.standard_normal((3, 4, 5, 6)).astype(np.float32)
    p = _ref_params(m)

    def ref(xt):
        t = torch.tanh(F.conv2d(xt, p[(c1.name, 'kernel')], p[(c1.name, 'bias')], padding=1))
        t = F.pad(torch.cat([t[..., -2:], t, t[..., :2]], dim=-1), (0, 0, 2, 2))
        return torch.tanh(F.conv2d(t, p[(c2.name, 'kernel')], p[(c2.name, 'bias')], stride=2))
    _check_step(m, ref, x, y, p)


def test_training_step_through_a_channel_window_against_float64_autograd(monkeypatch):
    """slice_layer in front of two strided layers: each adjoint writes its own channel window of the source's gradient in place
    (dlwp_space_to_depth2_pad_bwd with c_off / c_total), no dense tensor and no copy in between"""
    from dlwp_amd.custom import slice_layer
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    x0 = L.Input(shape=(3, 8, 12))
    c1 = L.Conv2D(6, 3, padding='same', activation='tanh', **CF)
    c2 = L.Conv2D(4, 3, strides=2, padding='same', activation='tanh', **CF)
    c3 = L.Conv2D(4, 2, strides=2, **CF)
    t = c1(x0)
    out = L.concatenate([c2(slice_layer(0, 3, axis=1)(t)), c3(slice_layer(3, 6, axis=1)(t))], axis=1)
    m = Model(inputs=x0, outputs=out, seed=4)
    m.compile(optimizer=Adam(lr=1e-3), loss='mse')
    kinds = [(op.kind, op.in_c_off, op.in_c_total) for op in m.plan.ops if op.kind == 's2dp']
    assert kinds == [('s2dp', 0, 6), ('s2dp', 3, 6)]
    _randomise(m, np.random.default_rng(8))
    rng = np.random.default_rng(9)
    x, y = rng.standard_normal((3, 3, 8, 12)).astype(np.float32), rng.standard_normal((3, 8, 4, 6)).astype(np.float32)
    p = _ref_params(m)

    def ref(xt):
        t = torch.tanh(F.conv2d(xt, p[(c1.name, 'kernel')], p[(c1.name, 'bias')], padding=1))
        a = torch.tanh(F.conv2d(F.pad(t[:, 0:3], (0, 1, 0, 1)), p[(c2.name, 'kernel')], p[(c2.name, 'bias')], stride=2))
        b = F.conv2d(t[:, 3:6], p[(c3.name, 'kernel')], p[(c3.name, 'bias')], stride=2)
        return torch.cat([a, b], dim=1)
    _check_step(m, ref, x, y, p)


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
    """2 eager steps, then the recorded (and validated) one and 2 replayed ones: 3 steps through the tape, nothing marks it foreign"""
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
    assert np.isfinite(want).all() and kept.shape == (4, 5, 2, 2, 8, 12)
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
    assert [lay.strides for lay in m2.layers if isinstance(lay, L.Conv2D)] == [(2, 2), (1, 1)]
    assert np.array_equal(_bits(m2.predict(batches[0][0])), _bits(m.predict(batches[0][0])))
    for x, y in batches[2:]:
        a, b = m.train_on_batch(x, y), m2.train_on_batch(x, y)
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(_bits(a), _bits(b))


def test_the_references_convlstm_network_builds_and_trains_against_autograd():
    """(b) the network examples/train_generator.py of the reference carries commented out, at reduced size: ConvLSTM2D stage ->
    Reshape -> PeriodicPadding2D((0, 2)) + ZeroPadding2D((2, 0)) -> Conv2D(16, 5, strides=2, 'valid', tanh) -> Flatten -> Dense ->
    Reshape.  Loss to TOL; gradients to 3e-4 of their scale, the bound tests/test_gpu_model.py holds the back-propagation through
    time of this ConvLSTM2D stage to (test_convlstm_train_step_matches_autograd_oracle_with_l2)."""
    from dlwp_amd.model import DLWPNeuralNet
    from oracle import torch_ref
    cs = (2, 1, 6, 8)
    front = (('PeriodicPadding3D', ((0, 0, 2),), dict(CF, input_shape=cs)),
             ('ZeroPadding3D', ((0, 2, 0),), dict(CF)),
             ('ConvLSTM2D', (4, 3), dict(CF, dilation_rate=2, padding='valid', activation='tanh', return_sequences=True)),
             ('Reshape', ((8, 6, 8),), None))
    layers = front + (('PeriodicPadding2D', ((0, 2),), dict(CF)),
                      ('ZeroPadding2D', ((2, 0),), dict(CF)),
                      ('Conv2D', (16, 5), dict(CF, strides=2, padding='valid', activation='tanh')),
                      ('Flatten', None, None),
                      ('Dense', (int(np.prod(cs)),), {'activation': 'linear'}),
                      ('Reshape', (cs,), None))
    np.random.seed(4)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=True, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(layers, loss='mse', optimizer='adam')
    m = d.model
    kinds = [op.kind for op in m.plan.ops]
    assert kinds.count('sphasew') == 1 and kinds.count('s2dp') == 1 and 'dense' in kinds and 'lstm' in kinds
    s2dp = [op for op in m.plan.ops if op.kind == 's2dp'][0]
    assert tuple(s2dp.halo) == (2, 2, 2, 2, S.ZERO, S.WRAP) and s2dp.out_shape == (32, 3 + 2, 4 + 2)
    rng = np.random.default_rng(31)
    ws = [(a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32) for a in m.get_weights()]
    m.set_weights(ws)
    lk, lr, lb, ck, cb, dk, db = [torch.tensor(a.astype(np.float64)) for a in ws]
    tw = [t.permute(3, 2, 0, 1).contiguous().requires_grad_(True) for t in (lk, lr, ck)]
    lb, cb, dk, db = [t.requires_grad_(True) for t in (lb, cb, dk, db)]
    x, y = rng.standard_normal((3,) + cs).astype(np.float32), rng.standard_normal((3,) + cs).astype(np.float32)
    t = torch_ref.run_layers(front, torch.tensor(x, dtype=torch.float64), [(tw[0], tw[1], lb)])
    t = F.pad(torch.cat([t[..., -2:], t, t[..., :2]], dim=-1), (0, 0, 2, 2))
    t = torch.tanh(F.conv2d(t, tw[2], cb, stride=2))
    assert tuple(t.shape[1:]) == (16, 3, 4)
    out = (t.reshape(3, -1) @ dk + db).reshape((3,) + cs)
    val = ((out - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    val.backward()
    want = [tw[0].grad.permute(2, 3, 1, 0), tw[1].grad.permute(2, 3, 1, 0), lb.grad, tw[2].grad.permute(2, 3, 1, 0), cb.grad,
            dk.grad, db.grad]
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    assert loss == pytest.approx(float(val.detach()), rel=TOL)
    tr, off = m._trainer, 0
    for g_ref in want:
        g_ref = g_ref.numpy()
        g = tr.flat_grads[off:off + g_ref.size].cpu().numpy().reshape(g_ref.shape)
        off += g_ref.size
        ratio = float(np.abs(g - g_ref).max() / max(np.abs(g_ref).max(), 1e-6))
        print('MEASURED   gradient %r error %.3g of its scale' % (g_ref.shape, ratio))
        assert ratio <= 3e-4, g_ref.shape
    assert off == tr.flat_grads.numel()


def test_bfloat16_activation_storage_is_refused():
    m = _model(seed=8)
    with pytest.raises(NotImplementedError, match='strides=2'):
        m.set_activation_dtype('bfloat16')
    assert m.activation_dtype == 'float32'
    x, _ = _data(33)
    assert np.isfinite(m.predict(x)).all()


# ----------------------------------------------------------------------------------------------------------------------- #
# build_model(gpus > 1)
# ----------------------------------------------------------------------------------------------------------------------- #
DP_SPECS = (('Conv2D', (8, 3), dict(CF, strides=2, padding='same', activation='tanh', input_shape=(4, 8, 12))),
            ('Conv2D', (8, 3), dict(CF, padding='same')),
            ('Conv2DTranspose', (4, 4), dict(CF, strides=2, padding='same')))


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
    """(c) build_model(gpus=2): the all-reduced gradient is that of the layer's own kernel; tolerances of
    tests/test_gpu_tconv.py::test_two_rank_training_equals_the_single_process_run"""
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
    assert [op.kind for op in d.model.plan.ops] == ['sphasew', 's2dp', 'conv', 'conv', 'tphasew', 'conv', 'd2sc']
    d.model.set_weights(res[0]['w0'])
    x, y = _data(21, n=8)
    logs = [np.atleast_1d(d.model.train_on_batch(x, y)).tolist() for _ in range(3)]
    for got, want in zip(res[0]['logs'], logs):
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (got, want)
    for a, b in zip(res[0]['w1'], d.model.get_weights()):
        # identical mathematics, two half-batch gradients against one: float32 round-off per step (tests/test_gpu_parallel.py)
        assert np.abs(a - b).max() <= 1e-6 * 3, np.abs(a - b).max()
