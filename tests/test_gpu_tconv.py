"""Conv2DTranspose(strides=2) and Cropping2D on the GPU (csrc/tconv.hip through every layer of the stack).

Kernels: the weight map and its adjoint, the cropping interleave and its adjoint are BIT-EQUAL to the numpy restatements of
tests/tconv_cases.py (they move and zero-fill, nothing is rounded): every kh, kw in 1 ... 5, cin = 3 / F = 2 and cin = 8 / F = 4,
1 and 3 samples, maps 1 x 1, 2 x 3, 5 x 7 (element path) and 4 x 8 (16-byte path), a pointer one float past a 16-byte boundary, and
launches larger than one pass of the capped grid.  Every output starts as NaN, so an element a kernel does not write shows.

Layers: the forward against the float64 restatement at the project's float32 parity bar, max |got - want| <= 1e-5 max |want|
(FWD_TOL); one training step of a small encoder / decoder against float64 torch autograd (TOL, BWD_TOL as
tests/test_gpu_eltwise.py imports them); the replayed step against the eager one, the captured rollout against the host loop and
model files in both formats, bit for bit; Cropping2D alone and in a 73-row model; two data-parallel ranks against one process;
the bfloat16 storage mode."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dlwp_amd import layers as L
from tests import tconv_cases as T
from tests.test_gpu_batchnorm import _bits, _grads_of, _host, _ref_params
from tests.test_gpu_convlstm_bwd import BWD_TOL
from tests.test_gpu_dense import TOL
from tests.test_gpu_train_ops import Slab, cu_count, same_bits

pytestmark = pytest.mark.gpu

CF = {'data_format': 'channels_first'}
FWD_TOL = 1e-5          # the project's float32 parity bar, as tests/test_gpu_eltwise.py uses it
CHANNELS = [(3, 2), (8, 4)]            # (cin, F): no whole channel tile; 4 F = 16
MAPS = [(1, 1), (2, 3), (5, 7), (4, 8)]


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
# kernels
# ----------------------------------------------------------------------------------------------------------------------- #
def test_weight_map_and_its_adjoint_are_bit_equal(ops):
    rng = np.random.default_rng(1)
    for kh, kw in T.KERNELS:
        for cin, f in CHANNELS:
            K, b = rng.standard_normal((kh, kw, f, cin)).astype(np.float32), rng.standard_normal(f).astype(np.float32)
            th, tw = (kh + 1) // 2, (kw + 1) // 2
            want_w2, want_b2 = T.weight_map(K, b)
            for bias in (b, None):
                w2, b2 = _nan(th, tw, cin, 4 * f), (_nan(4 * f) if bias is not None else None)
                ops.tconv_weights(_dev(K), _dev(bias) if bias is not None else None, w2=w2, b2=b2)
                assert same_bits(_host(w2), want_w2), (kh, kw, cin, f)
                assert bias is None or same_bits(_host(b2), want_b2)
            for taps in ((th, tw), T.stored_taps(th, tw), (5, 5)):           # T x T, what the planner stores, 5 x 5
                w2 = _nan(taps[0], taps[1], cin, 4 * f)
                ops.tconv_weights(_dev(K), None, w2=w2)
                assert same_bits(_host(w2), T.weight_map(K, None, taps)[0]), (kh, kw, cin, f, taps)
                g2 = rng.standard_normal(tuple(w2.shape)).astype(np.float32)
                dk = _nan(kh, kw, f, cin)
                ops.tconv_weights_bwd(_dev(g2), dk)
                want = T.weight_map_bwd(g2, K.shape)
                assert same_bits(_host(dk), want), (kh, kw, cin, f, taps)
                ops.tconv_weights_bwd(_dev(g2), dk, accumulate=True)         # (+)=: one float32 addition per element
                assert same_bits(_host(dk), want + want)
    # more elements than one pass of the 4096-workgroup grid: 3 x 3 taps, 256 x 4 * 128 columns
    K = rng.standard_normal((5, 5, 128, 256)).astype(np.float32)
    w2, _ = ops.tconv_weights(_dev(K), None)
    assert w2.numel() > 4096 * 256 and same_bits(_host(w2), T.weight_map(K)[0])
    g2 = rng.standard_normal(tuple(w2.shape)).astype(np.float32)
    dk = _nan(*K.shape)
    ops.tconv_weights_bwd(_dev(g2), dk)
    assert same_bits(_host(dk), T.weight_map_bwd(g2, K.shape))
    with pytest.raises(ValueError):
        ops.tconv_weights_bwd(_dev(g2[:2]), dk)
    with pytest.raises(ValueError):
        ops.tconv_weights(_dev(K), None, w2=_nan(3, 3, 128, 512))


def _interleave_case(ops, rng, n, f, hp, wp, top, left, hh, ww, align=0, c_off=0, c_total=None):
    """the cropping interleave and its adjoint on guarded slabs `align` floats past a 16-byte boundary, against numpy"""
    c_total = c_total or f
    ph = rng.standard_normal((n, 4 * f, hp, wp)).astype(np.float32)
    s_in, s_out = Slab(ph, align), Slab(None, align, (n, c_total, hh, ww))
    ops.depth_to_space2_crop(s_in.t, f, top, left, hh, ww, out=s_out.t, c_off=c_off)
    got = s_out.read()
    want = T.d2s_crop(ph, f, top, left, hh, ww)
    what = (n, f, hp, wp, top, left, hh, ww, align, c_off)
    assert same_bits(got[:, c_off:c_off + f], want), what
    assert np.isnan(np.delete(got, np.s_[c_off:c_off + f], axis=1)).all(), what          # the other channels stay untouched
    assert s_in.unchanged()
    dy = rng.standard_normal((n, c_total, hh, ww)).astype(np.float32)
    s_dy, s_dp = Slab(dy, align), Slab(None, align, (n, 4 * f, hp, wp))                 # NaN: every element must be written
    ops.space_to_depth2_fill(s_dy.t, f, hp, wp, top, left, c_off=c_off, out=s_dp.t)
    got = s_dp.read()
    want = T.s2d_fill(dy[:, c_off:c_off + f], hp, wp, top, left)
    assert same_bits(got, want), what                                                    # (+0 bits on every cropped position)
    assert s_dy.unchanged()
    return want


@pytest.mark.parametrize('padding', T.PADDINGS)
def test_interleave_and_its_adjoint_are_bit_equal(ops, padding):
    rng = np.random.default_rng(2)
    k = 0
    for kh, kw in T.KERNELS:
        for h, w in MAPS:
            (th, top, hh), (tw, left, ww) = T.geometry(kh, padding, h), T.geometry(kw, padding, w)
            f, n = CHANNELS[k % 2][1], (1, 3)[(k // 2) % 2]
            k += 1
            _interleave_case(ops, rng, n, f, h + th - 1, w + tw - 1, top, left, hh, ww)


def test_interleave_vector_path_alignment_windows_and_large_launches(ops):
    rng = np.random.default_rng(3)
    # the 16-byte path (wp % 4 == 0, left % 4 == 0, W % 4 == 0, aligned pointers), the same geometry one float off (element path),
    # and each single cause of leaving the 16-byte path
    for hp, wp, top, left, hh, ww in [(4, 8, 0, 0, 8, 16), (4, 8, 1, 4, 6, 8), (4, 8, 0, 4, 7, 12), (3, 12, 1, 8, 5, 16),
                                      (3, 12, 0, 0, 6, 20), (4, 8, 0, 2, 8, 12), (4, 8, 0, 0, 8, 14), (4, 6, 0, 0, 8, 12)]:
        for n, f in ((1, 2), (3, 4)):
            a = _interleave_case(ops, rng, n, f, hp, wp, top, left, hh, ww, align=0)
            assert a.shape == (n, 4 * f, hp, wp)
            _interleave_case(ops, rng, n, f, hp, wp, top, left, hh, ww, align=1)
    # a channel window of a wider tensor (a concatenation target)
    _interleave_case(ops, rng, 3, 2, 4, 8, 0, 0, 8, 16, c_off=3, c_total=6)
    _interleave_case(ops, rng, 3, 2, 5, 7, 1, 1, 8, 12, c_off=1, c_total=4)
    # more work than one pass of the capped grid (16 workgroups of 256 lanes per CU): both paths, cropped
    per_pass = cu_count() * 16 * 256
    n, f, hp, wp = 2, 4, 512, 640
    assert n * f * (2 * hp - 2) * (wp // 4) > per_pass
    _interleave_case(ops, rng, n, f, hp, wp, 1, 4, 2 * hp - 2, 2 * wp - 8)
    n, f, hp, wp = 3, 2, 600, 301
    assert n * f * hp * wp > per_pass                                     # (the element path: one lane per phase pixel)
    _interleave_case(ops, rng, n, f, hp, wp, 1, 1, 2 * hp - 2, 2 * wp - 2)


def test_fused_interleave_equals_depth_to_space_followed_by_a_crop(ops):
    rng = np.random.default_rng(4)
    for hp, wp, top, left, hh, ww in [(5, 7, 1, 1, 8, 12), (4, 8, 0, 0, 8, 16), (4, 8, 1, 4, 6, 8), (9, 15, 1, 3, 16, 24)]:
        ph = _dev(rng.standard_normal((3, 8, hp, wp)))
        whole = _host(ops.depth_to_space2(ph, 2))
        got = _host(ops.depth_to_space2_crop(ph, 2, top, left, hh, ww, out=_nan(3, 2, hh, ww)))
        assert same_bits(got, whole[:, :, top:top + hh, left:left + ww])
        two = _host(ops.crop2d(ops.depth_to_space2(ph, 2), ops.make_pad(top, 2 * hp - top - hh, left, 2 * wp - left - ww)))
        assert same_bits(got, two)
    with pytest.raises(Exception, match='crop'):
        ops.depth_to_space2_crop(ph, 2, 1, 0, 2 * hp, 2 * wp)


# ----------------------------------------------------------------------------------------------------------------------- #
# Cropping2D
# ----------------------------------------------------------------------------------------------------------------------- #
def test_cropping2d_alone_is_slicing_forward_and_zero_padding_backward(ops):
    from dlwp_amd.engine import Model
    rng = np.random.default_rng(5)
    for shape, crop in [((3, 2, 9, 10), ((1, 0), (2, 3))), ((1, 1, 2, 2), ((0, 1), (1, 0))), ((2, 3, 8, 16), ((0, 0), (4, 4))),
                        ((2, 3, 73, 144), ((1, 0), (0, 0))), ((3, 4, 16, 28), ((0, 0), (2, 2)))]:
        x = rng.standard_normal(shape).astype(np.float32)
        (t, b), (l, r) = crop
        want = x[:, :, t:shape[2] - b, l:shape[3] - r]
        got = _host(ops.crop2d(_dev(x), ops.make_pad(t, b, l, r), out=_nan(*want.shape)))
        assert same_bits(got, want), (shape, crop)
        x0 = L.Input(shape=shape[1:])
        m = Model(inputs=x0, outputs=L.Cropping2D(crop, **CF)(x0))
        assert [op.kind for op in m.infer_plan.ops] == ['crop'] and same_bits(m.predict(x), want)
        dy = rng.standard_normal(want.shape).astype(np.float32)
        back = _host(ops.pad2d(_dev(dy), ops.make_pad(t, b, l, r)))               # what BackwardPass._crop deposits
        assert same_bits(back, np.pad(dy, ((0, 0), (0, 0), (t, b), (l, r))))


def test_cropping2d_between_two_convolutions_trains_against_autograd(monkeypatch):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    x0 = L.Input(shape=(3, 9, 10))
    c1, c2 = L.Conv2D(5, 3, padding='same', activation='tanh', **CF), L.Conv2D(2, 3, padding='same', **CF)
    m = Model(inputs=x0, outputs=c2(L.Cropping2D(((1, 0), (2, 3)), **CF)(c1(x0))), seed=3)
    m.compile(optimizer=Adam(lr=1e-3), loss='mse')
    assert [op.kind for op in m.plan.ops] == ['conv', 'crop', 'conv']
    _randomise(m, np.random.default_rng(6))
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((3, 3, 9, 10)).astype(np.float32), rng.standard_normal((3, 2, 8, 5)).astype(np.float32)
    p = _ref_params(m)

    def ref(xt):
        t = torch.tanh(F.conv2d(xt, p[(c1.name, 'kernel')], p[(c1.name, 'bias')], padding=1))
        return F.conv2d(t[:, :, 1:, 2:-3], p[(c2.name, 'kernel')], p[(c2.name, 'bias')], padding=1)
    _check_step(m, ref, x, y, p)


# ----------------------------------------------------------------------------------------------------------------------- #
# the layer's forward
# ----------------------------------------------------------------------------------------------------------------------- #
def _randomise(model, rng):
    """every bias drawn at random, so that all of them are tested"""
    for lay in model.layers:
        if isinstance(lay, (L.Conv2D, L.Conv2DTranspose)) and lay.bias is not None:
            k, b = lay.get_weights()
            lay.set_weights([k, (0.3 * rng.standard_normal(b.shape)).astype(np.float32)])


@pytest.mark.parametrize('padding', T.PADDINGS)
@pytest.mark.parametrize('k', [1, 2, 3, 4, 5])
def test_forward_against_the_float64_restatement(k, padding):
    from dlwp_amd.engine import Model
    rng = np.random.default_rng(10 * k + len(padding))
    worst = 0.0
    for h, w in [(2, 3), (5, 7), (8, 12)]:
        x = (2.0 * rng.standard_normal((3, 3, h, w))).astype(np.float32)
        for use_bias in (True, False):
            for act in ('linear', 'tanh', 'relu'):
                x0 = L.Input(shape=(3, h, w))
                lay = L.Conv2DTranspose(2, k, padding=padding, activation=act, use_bias=use_bias, **CF)
                m = Model(inputs=x0, outputs=lay(x0), seed=k)
                _randomise(m, rng)
                ws = [a.astype(np.float64) for a in lay.get_weights()]
                want = T.restated(x.astype(np.float64), ws[0], ws[1] if use_bias else None, padding, act)
                got = m.predict(x)
                assert got.shape == want.shape == (3, 2) + tuple(lay.compute_output_shape((3, h, w))[1:])
                err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
                worst = max(worst, err / scale)
                assert err <= FWD_TOL * scale, (h, w, use_bias, act, err, scale)
    print('\nMEASURED Conv2DTranspose(k=%d, %s) forward: worst error %.3g of the scale' % (k, padding, worst))


def test_interleaved_store_epilogue_gives_the_bits_of_the_two_launch_form():
    """where dlwp_conv2d_supports_out_d2s says yes and nothing is cropped, the inference plan lets the convolution store the phases
    interleaved: the same bits as convolution + interleave"""
    from dlwp_amd import plan as P
    from dlwp_amd.engine import Executor, Model
    rng = np.random.default_rng(8)
    for cin, f, k, h, w in [(8, 4, 6, 8, 12), (16, 4, 6, 6, 8)]:
        x0 = L.Input(shape=(cin, h, w))
        m = Model(inputs=x0, outputs=L.Conv2DTranspose(f, k, activation='tanh', **CF)(x0), seed=2)
        _randomise(m, rng)
        assert [(op.kind, op.out_d2s) for op in m.infer_plan.ops] == [('tphasew', False), ('conv', True)]
        plain = P.build_plan(m.inputs, m.outputs, inference=True, fuse_d2s=False)
        assert [op.kind for op in plain.ops] == ['tphasew', 'conv', 'd2sc']
        x = rng.standard_normal((3, cin, h, w)).astype(np.float32)
        got = m.predict(x)
        two = _host(Executor(plain, m.device).run(_dev(x))[0])
        assert got.shape == two.shape == (3, f, 2 * h + 4, 2 * w + 4) and same_bits(got, two)
        ws = [a.astype(np.float64) for a in m.layers[-1].get_weights()]
        want = T.restated(x.astype(np.float64), ws[0], ws[1], 'valid', 'tanh')
        assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()


# ----------------------------------------------------------------------------------------------------------------------- #
# models
# ----------------------------------------------------------------------------------------------------------------------- #
def _periodic(t):
    return torch.cat([t[..., -1:], t, t[..., :1]], dim=-1)


def _net(pools=1, l2=None):
    """conv -> max-pool (x pools) -> Conv2DTranspose(8, 2) -> PeriodicPadding2D((0, 1)) + Conv2DTranspose(4, 4, 'same') +
    Cropping2D((0, 2)) -> conv, on 4 x 8 x 12.  pools = 2 returns the input's shape (a state a rollout can feed back)."""
    from dlwp_amd.custom import PeriodicPadding2D
    from dlwp_amd.regularizers import l2 as l2_reg
    reg = dict(kernel_regularizer=l2_reg(l2)) if l2 else {}
    x0 = L.Input(shape=(4, 8, 12))
    t = L.Conv2D(8, 3, padding='same', activation='tanh', **CF)(x0)
    for _ in range(pools):
        t = L.MaxPooling2D(2, **CF)(t)
    t = L.Conv2DTranspose(8, 2, activation='tanh', **dict(CF, **reg))(t)
    t = L.Conv2DTranspose(4, 4, padding='same', activation='relu', **dict(CF, **reg))(PeriodicPadding2D((0, 1), **CF)(t))
    t = L.Cropping2D((0, 2), **CF)(t)
    return x0, L.Conv2D(4, 3, padding='same', **CF)(t)


def _net_ref(model, x, p, pools=1):
    convs = [lay for lay in model.layers if isinstance(lay, L.Conv2D)]
    ups = [lay for lay in model.layers if isinstance(lay, L.Conv2DTranspose)]
    t = torch.tanh(F.conv2d(x, p[(convs[0].name, 'kernel')], p[(convs[0].name, 'bias')], padding=1))
    for _ in range(pools):
        t = F.max_pool2d(t, 2)
    t = torch.tanh(F.conv_transpose2d(t, p[(ups[0].name, 'kernel')], p[(ups[0].name, 'bias')], stride=2))
    t = F.conv_transpose2d(_periodic(t), p[(ups[1].name, 'kernel')], p[(ups[1].name, 'bias')], stride=2)
    t = torch.relu(t[:, :, 1:-1, 1:-1])                  # 'same' for k = 4: rows / columns [1, 1 + 2h) of the full result
    return F.conv2d(t[..., 2:-2], p[(convs[1].name, 'kernel')], p[(convs[1].name, 'bias')], padding=1)


def _model(pools=1, seed=1, l2=None, lr=1e-3):
    from dlwp_amd.engine import Model
    from dlwp_amd.training import Adam
    x0, out = _net(pools, l2)
    m = Model(inputs=x0, outputs=out, seed=seed)
    m.compile(optimizer=Adam(lr=lr), loss='mse')
    _randomise(m, np.random.default_rng(seed + 100))
    return m


def _data(pools, seed, n=3):
    rng = np.random.default_rng(seed)
    s = 2 if pools == 1 else 1
    return (rng.standard_normal((n, 4, 8, 12)).astype(np.float32), rng.standard_normal((n, 4, 8 * s, 12 * s)).astype(np.float32))


def _check_step(m, ref, x, y, p, l2=None):
    """one train_on_batch against float64 autograd: the loss (TOL) and the gradient of every kernel and bias (BWD_TOL)"""
    loss = np.atleast_1d(m.train_on_batch(x, y))[0]
    torch.cuda.synchronize()
    val = ((ref(torch.tensor(x, dtype=torch.float64)) - torch.tensor(y, dtype=torch.float64)) ** 2).mean()
    if l2:
        val = val + sum(l2 * (p[(lay.name, 'kernel')] ** 2).sum() for lay in m.layers if isinstance(lay, L.Conv2DTranspose))
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


def test_predict_of_the_small_model_against_float64():
    for pools in (1, 2):
        m = _model(pools)
        kinds = [op.kind for op in m.infer_plan.ops]
        assert kinds.count('tphasew') == 2 and 'crop' not in kinds            # (the crop rides in the second interleave)
        x, _ = _data(pools, 11)
        with torch.no_grad():
            want = _net_ref(m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False), pools).numpy()
        got = m.predict(x)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()


@pytest.mark.parametrize('l2', [None, 1e-2], ids=['plain', 'l2'])
def test_training_step_against_float64_autograd(monkeypatch, l2):
    monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    m = _model(1, seed=2, l2=l2)
    assert [op.kind for op in m.plan.ops] == ['conv', 'maxpool', 'tphasew', 'conv', 'd2sc', 'pad', 'tphasew', 'conv', 'd2sc', 'conv']
    x, y = _data(1, 12)
    p = _ref_params(m)
    _check_step(m, lambda xt: _net_ref(m, xt, p, 1), x, y, p, l2=l2)


def _run_steps(monkeypatch, form, batches):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)
    m = _model(1, seed=5)                   # (no kernel regulariser: a step with one is never replayed)
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
    batches = [_data(1, 600 + i) for i in range(5)]
    ref = _run_steps(monkeypatch, 'eager', batches)
    for form in ('graph', 'lanes'):
        got = _run_steps(monkeypatch, form, batches)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (form, a, b)
        for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
            assert np.array_equal(_bits(a), _bits(b)), form


def test_captured_rollout_equals_the_host_loop():
    from dlwp_amd.model import DLWPFunctional
    m = _model(2, seed=6)
    d = DLWPFunctional(is_convolutional=True, is_recurrent=False, time_dim=2)
    d.model = d.base_model = m
    x, _ = _data(2, 15, n=5)
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
    batches = [_data(1, 800 + i) for i in range(4)]
    m = _model(1, seed=7, l2=1e-3)
    for x, y in batches[:2]:
        m.train_on_batch(x, y)
    path = str(tmp_path / ('m.%s' % fmt))
    m.save(path, format=fmt)
    m2 = serialization.load_model_file(path)
    assert [type(lay).__name__ for lay in m2.layers] == [type(lay).__name__ for lay in m.layers]
    assert [lay.get_config() for lay in m2.layers] == [lay.get_config() for lay in m.layers]
    assert np.array_equal(_bits(m2.predict(batches[0][0])), _bits(m.predict(batches[0][0])))
    for x, y in batches[2:]:
        a, b = m.train_on_batch(x, y), m2.train_on_batch(x, y)
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(_bits(a), _bits(b))


def test_73_row_model_returns_a_73_row_state():
    """Cropping2D(((1, 0), (0, 0))) -> pool / transposed stack -> ZeroPadding2D(((1, 0), (0, 0))): the pole row leaves and returns"""
    from dlwp_amd.engine import Model
    x0 = L.Input(shape=(2, 73, 24))
    c1 = L.Conv2D(4, 3, padding='same', activation='tanh', **CF)
    up = L.Conv2DTranspose(2, 2, **CF)
    t = up(L.MaxPooling2D(2, **CF)(c1(L.Cropping2D(((1, 0), (0, 0)), **CF)(x0))))
    m = Model(inputs=x0, outputs=L.ZeroPadding2D(((1, 0), (0, 0)), **CF)(t), seed=4)
    _randomise(m, np.random.default_rng(9))
    x = np.random.default_rng(10).standard_normal((3, 2, 73, 24)).astype(np.float32)
    got = m.predict(x)
    assert got.shape == (3, 2, 73, 24) and not got[:, :, 0].any()
    p = _ref_params(m, requires_grad=False)
    with torch.no_grad():
        t = torch.tanh(F.conv2d(torch.tensor(x, dtype=torch.float64)[:, :, 1:], p[(c1.name, 'kernel')], p[(c1.name, 'bias')], padding=1))
        want = F.pad(F.conv_transpose2d(F.max_pool2d(t, 2), p[(up.name, 'kernel')], p[(up.name, 'bias')], stride=2), (0, 0, 1, 0)).numpy()
    assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()
    state = x
    for _ in range(2):                                               # the output is a state of the input's shape
        state = m.predict(state)
    assert state.shape == x.shape and np.isfinite(state).all()


# ----------------------------------------------------------------------------------------------------------------------- #
# build_model(gpus > 1)
# ----------------------------------------------------------------------------------------------------------------------- #
DP_SPECS = (('Conv2D', (8, 3), dict(CF, padding='same', activation='tanh', input_shape=(4, 8, 12))),
            ('MaxPooling2D', (2,), dict(CF)),
            ('PeriodicPadding2D', ((0, 1),), dict(CF)),
            ('Conv2DTranspose', (4, 4), dict(CF, strides=2, padding='same')),
            ('Cropping2D', ((0, 2),), dict(CF)))


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
    x, y = _data(2, 21, n=8)
    logs = [np.atleast_1d(d.model.train_on_batch(x, y)).tolist() for _ in range(3)]
    torch.cuda.synchronize()
    ret[rank] = {'w0': w0, 'w1': d.model.get_weights(), 'logs': logs}
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_training_equals_the_single_process_run():
    """build_model(gpus=2): kernel and bias of a Conv2DTranspose are ordinary tensors of the flat gradient the ranks exchange"""
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
    assert [op.kind for op in d.model.plan.ops] == ['conv', 'maxpool', 'pad', 'tphasew', 'conv', 'd2sc']
    d.model.set_weights(res[0]['w0'])
    x, y = _data(2, 21, n=8)
    logs = [np.atleast_1d(d.model.train_on_batch(x, y)).tolist() for _ in range(3)]
    for got, want in zip(res[0]['logs'], logs):
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (got, want)
    for a, b in zip(res[0]['w1'], d.model.get_weights()):
        # identical mathematics, two half-batch gradients against one: float32 round-off per step (tests/test_gpu_parallel.py)
        assert np.abs(a - b).max() <= 1e-6 * 3, np.abs(a - b).max()


def test_bfloat16_storage_keeps_the_phase_tensors_float32():
    """the bf16 mode: no refusal; the phase tensors and what the interleaves write stay float32, the buffers between the other
    convolutions may be bfloat16.  Bounds of a bf16-stored forward as tests/test_gpu_avgpool.py has them: 2^-9 per stored tensor."""
    m = _model(2, seed=8)
    x, _ = _data(2, 33, n=5)
    with torch.no_grad():
        want = _net_ref(m, torch.tensor(x, dtype=torch.float64), _ref_params(m, requires_grad=False), 2).numpy()
    m.set_activation_dtype('bfloat16')
    assert m.activation_dtype == 'bfloat16'
    ops_ = m.infer_plan.ops
    bufs = m.executor.scratch(5)
    for op in ops_:
        if op.kind == 'd2sc':
            assert bufs[op.src].dtype == torch.float32 and (op.dst < 0 or bufs[op.dst].dtype == torch.float32)
    got = m.predict(x)
    scale = max(1.0, float(np.abs(want).max()))
    rel, mean = float(np.abs(got - want).max()) / scale, float(np.abs(got - want).mean())
    print('\nMEASURED bf16 storage: max error %.3g of scale, mean error %.3g (scale %.3g), bf16 buffers %r' % (
        rel, mean, scale, m.infer_plan.bf16_buffers()))
    assert rel < 1e-2
    assert mean < 1e-3 * scale
