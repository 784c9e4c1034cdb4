"""The pooled dilation-2 first layer on Winograd multiplies (csrc/conv_fwd_few_wino.hip, DLWP_OPT_FEW_WINO): the
float64 oracle at the project's bar on ragged tiles, channel windows, every activation and halo mode; closeness to the direct
streaming kernel it replaces; launch info; batch independence; the bits of the general Winograd family; the executor's scoping at
the model level -- and, without a GPU, the item order and the executor's predicate.
Measured on the MI355X against the float64 oracle (bar 1e-5): at most 4.1e-7 per layer, 8.0e-7 for the model's forward and rollout."""
import numpy as np
import pytest
import torch

from oracle import np_ref

CONV_RTOL = 1e-5            # tests/test_gpu_kernels.py: _check_conv, relative to the output scale
ACTS = {'linear': 0, 'tanh': 1, 'relu': 2}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _record(v):
    """the relative error joins the session's record of forward errors (tests.test_gpu_model.MEASURED, which tests/conftest.py writes out)"""
    import os
    from tests import test_gpu_model
    test_gpu_model.MEASURED.setdefault(os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0], []).append(float(v))
    return v


CASES = [
    # (n, stored channels, (cin offset, cin), h, w, cout, (cout offset, total), mode_h, mode_w, act)   modes: 0 zero, 1 wrap, 2 edge
    (5, 4, (0, 4), 20, 52, 32, (0, 0), 0, 1, 'tanh'),          # ragged tiles both ways (3 x 2 positions), 16-byte loads and stores
    (3, 3, (0, 3), 18, 76, 64, (0, 0), 0, 1, 'tanh'),          # three channels, two channel tiles: the weights change in a share
    (70, 1, (0, 1), 10, 36, 32, (0, 0), 0, 1, 'relu'),         # one channel, one item per workgroup
    (300, 4, (0, 4), 12, 68, 32, (0, 0), 0, 1, 'tanh'),        # 1800 items: shares of 3-4 items, the position changes inside a share
    (3, 4, (0, 4), 24, 72, 32, (0, 0), 0, 1, 'linear'),        # pooled width 36 = 2 full column tiles + a quarter
    (4, 4, (0, 4), 16, 44, 32, (0, 0), 1, 2, 'tanh'),          # EDGE columns (element loads), periodic rows
    (4, 4, (0, 4), 13, 37, 32, (0, 0), 2, 0, 'relu'),          # odd height and width (pooled 6 x 18): element loads; edge rows
    (3, 9, (3, 4), 12, 40, 32, (16, 80), 0, 1, 'tanh'),        # channel windows on both sides
    (2, 7, (2, 2), 16, 36, 64, (64, 160), 1, 1, 'linear'),     # ... with two channels and two channel tiles
    (2, 4, (0, 4), 16, 36, 32, (0, 0), 0, 0, 'relu'),          # zero halo all round
]


def _ref(x, w, b, mh, mw, act):
    xp = np_ref.pad2d_modes(np.asarray(x, np.float64), (2, 2, 2, 2), mh, mw)
    return np_ref.maxpool2(np_ref.conv2d(xp, w, b, 2, act))


def _desc(ops, case):
    n, ct, (coff, cin), h, w, cout, (ooff, otot), mh, mw, act = case
    return ops.make_conv(cout, 3, 3, 2, ops.make_pad(2, 2, 2, 2, mh, mw), ACTS[act], in_c_off=coff, in_c_total=ct,
                         out_c_off=ooff, out_c_total=otot, out_pool=True)


def _inputs(case, seed):
    n, ct, (coff, cin), h, w, cout, _, _, _, _ = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ct, h, w)).astype(np.float32)
    wt = np_ref.glorot_uniform((3, 3, cin, cout), rng)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    return x, wt, b


def _run(ops, case, xd, wd, bd, mode, fill=7.0):
    n, ct, (coff, cin), h, w, cout, (ooff, otot), mh, mw, act = case
    cd = _desc(ops, case)
    prev = ops.set_few_wino(mode)
    try:
        info = ops.conv_launch_info((xd.shape[0], cin, h, w), cd)
        y = torch.full((xd.shape[0], otot or cout, h // 2, w // 2), fill, device='cuda')
        ops.conv2d(xd, wd, bd, cd, out=y, x_channels=cin)
    finally:
        ops.set_few_wino(prev)
    return y, info


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_few_wino_tracks_the_oracle_and_the_direct_kernel(ops, case):
    """Option on: the float64 oracle (maxpool of the convolution) at 1e-5 of the output scale, the direct streaming kernel at
    1e-5 of max |want|, sentinels outside the output window untouched, launch-info code -5 with the Winograd FLOP count.
    Measured on the MI355X: see DESIGN 5.26."""
    n, ct, (coff, cin), h, w, cout, (ooff, otot), mh, mw, act = case
    x, wt, b = _inputs(case, 7300 + CASES.index(case))
    xd, wd, bd = dev(x), dev(wt), dev(b)
    assert ops.set_few_wino(0) == 0                           # a handle starts at 0
    y0, info0 = _run(ops, case, xd, wd, bd, 0)
    y1, info1 = _run(ops, case, xd, wd, bd, 1)
    assert info0[0][0] != -5 and len(info1) == 1 and info1[0][0] == -5, (info0, info1)
    items = -(-h // 8) * -(-w // 32) * (cout // 32) * n
    assert info1[0][1] == min(items, 3 * torch.cuda.get_device_properties(0).multi_processor_count) and info1[0][2] == 256
    # 16 positions x 4 channels x Cout per 2x2 tile, times 2: 64 tiles x 32 channels an item, padding included
    assert info1[0][3] == 2.0 * 16 * 4 * 32 * 64 * items
    got, direct = y1.cpu().numpy(), y0.cpu().numpy()
    tot = otot or cout
    keep = [c for c in range(tot) if not ooff <= c < ooff + cout]
    assert np.all(got[:, keep] == 7.0), 'channels outside the output window were written'
    want = _ref(x[:, coff:coff + cin], wt, b, mh, mw, act)
    sub = got[:, ooff:ooff + cout]
    assert sub.shape == want.shape
    scale = max(1.0, float(np.abs(want).max()))
    err = _record(float(np.abs(sub - want).max()) / scale)
    near = float(np.abs(sub - direct[:, ooff:ooff + cout]).max()) / float(np.abs(want).max())
    print('few_wino %s: oracle %.3g, direct kernel %.3g' % (case, err, near))
    assert err <= CONV_RTOL, (case, err)
    assert near <= 1e-5, (case, near)


@pytest.mark.gpu
@pytest.mark.parametrize('act', ['linear', 'tanh', 'relu'])
@pytest.mark.parametrize('modes', [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (2, 1), (0, 2)])
def test_few_wino_every_activation_and_halo_mode(ops, act, modes):
    case = (3, 4, (0, 4), 12, 40, 32, (0, 0), modes[0], modes[1], act)
    x, wt, b = _inputs(case, 7400)
    y1, info1 = _run(ops, case, dev(x), dev(wt), dev(b), 1)
    assert info1[0][0] == -5
    want = _ref(x, wt, b, modes[0], modes[1], act)
    err = _record(float(np.abs(y1.cpu().numpy() - want).max()) / max(1.0, float(np.abs(want).max())))
    assert err <= CONV_RTOL, (act, modes, err)


@pytest.mark.gpu
def test_few_wino_refuses_what_it_does_not_cover(ops):
    prev = ops.set_few_wino(1)
    try:
        pad2 = ops.make_pad(2, 2, 2, 2, 0, 1)
        ok = ops.make_conv(32, 3, 3, 2, pad2, 1, out_pool=True)
        assert ops.conv_launch_info((8, 4, 16, 36), ok)[0][0] == -5
        assert ops.conv_launch_info((1, 1, 16, 36), ok)[0][0] == -5            # every batch size, every channel count up to 4
        assert ops.conv_launch_info((8, 5, 16, 36), ok)[0][0] != -5            # five to eight channels: the direct streaming kernel
        assert ops.conv_launch_info((8, 9, 16, 36), ok)[0][0] != -5
        assert ops.conv_launch_info((8, 4, 16, 36), ops.make_conv(32, 3, 3, 2, pad2, 1))[0][0] != -5                 # unpooled
        assert ops.conv_launch_info((8, 4, 16, 36), ops.make_conv(48, 3, 3, 2, pad2, 1, out_pool=True))[0][0] != -5  # Cout % 32
        assert ops.conv_launch_info((8, 4, 16, 36), ops.make_conv(32, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 1), 1,
                                                                  out_pool=True))[0][0] != -5                        # dilation 1
        assert ops.conv_launch_info((8, 4, 16, 36), ops.make_conv(32, 5, 5, 1, pad2, 1, out_pool=True))[0][0] != -5  # 5x5
    finally:
        ops.set_few_wino(prev)
    assert ops.conv_launch_info((256, 4, 88, 180), ok)[0][0] == -2             # option off: the plain call's kernel


@pytest.mark.gpu
def test_few_wino_bits_do_not_depend_on_batch_mates_or_grid(ops):
    """Sample k of a 70-sample batch (630 workgroups) == the same sample alone (9 workgroups) == inside a batch of 5 (45 workgroups),
    bit for bit; and the same inside a batch of 100 (900 items on 3 workgroups per CU: shares of more than one item)."""
    case = (70, 4, (0, 4), 24, 72, 32, (0, 0), 0, 1, 'tanh')
    x, wt, b = _inputs(case, 7500)
    xd, wd, bd = dev(x), dev(wt), dev(b)
    full, info = _run(ops, case, xd, wd, bd, 1)
    grids = {info[0][1]}
    for lo, hi in ((33, 34), (31, 36), (0, 1), (69, 70), (65, 70)):
        part, pinfo = _run(ops, case, xd[lo:hi].contiguous(), wd, bd, 1)
        grids.add(pinfo[0][1])
        assert torch.equal(part, full[lo:hi]), (lo, hi)
    assert len(grids) == 3, grids
    x100 = torch.cat([xd, xd[:30]])
    big, binfo = _run(ops, case, x100, wd, bd, 1)
    assert binfo[0][1] < 9 * 100 and torch.equal(big[:70], full) and torch.equal(big[70:], full[:30])


@pytest.mark.gpu
@pytest.mark.parametrize('act', ['tanh', 'relu', 'linear'])
def test_few_wino_gives_the_bits_of_the_general_winograd_family(ops, act):
    """ops.force_conv_config cannot put a general dilation-2 Winograd instance on a layer of at most four input channels (the family
    starts at five, conv_fwd.hip: wino_channels_ok; five to eight channels under a 32-channel tile belong to the direct streaming
    kernel).  The general family is reached another way: a 16-channel layer whose channels 4-15 are ZERO in the input -- its chunks
    of 8 channels add exact zeros to the sums of channels 0-3, so its bits are those of the 4-channel Winograd sum.  The reference
    launch must be a dilation-2 Winograd instance (asserted); its pooled image comes from maxpool2 of its own output."""
    n, h, w, cout = 3, 24, 72, 64
    rng = np.random.default_rng(7600)
    x16 = np.zeros((n, 16, h, w), np.float32)
    x16[:, :4] = rng.standard_normal((n, 4, h, w)).astype(np.float32)
    w16 = np_ref.glorot_uniform((3, 3, 16, cout), rng)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    pad = ops.make_pad(2, 2, 2, 2, 0, 1)
    cd16 = ops.make_conv(cout, 3, 3, 2, pad, ACTS[act])
    info = ops.conv_launch_info((n, 16, h, w), cd16)
    cfg = ops.conv_configs()[info[0][0]] if info[0][0] >= 0 else None
    assert cfg is not None and cfg[0] == 3 and cfg[1] == 2 and cfg[5] == 0, (info, cfg)      # a dilation-2 Winograd instance
    ref = ops.maxpool2(ops.conv2d(dev(x16), dev(w16), dev(b), cd16))
    case = (n, 4, (0, 4), h, w, cout, (0, 0), 0, 1, act)
    got, ginfo = _run(ops, case, dev(x16[:, :4]), dev(w16[:, :, :4]), dev(b), 1)
    assert ginfo[0][0] == -5
    assert torch.equal(got, ref), float((got - ref).abs().max())


def _unet(cs, seed=0):
    from dlwp_amd.model import DLWPNeuralNet
    from tests.nets import unet_layers
    np.random.seed(seed)
    layers = unet_layers(cs)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(layers, loss='mse', optimizer='adam', metrics=['mae'])
    return d, layers


def _first_conv(ex):
    return next((op, d) for op, d in zip(ex.plan.ops, ex._descriptors()) if op.kind == 'conv')


@pytest.mark.gpu
def test_model_runs_its_first_layer_on_winograd_multiplies_and_training_does_not(ops, monkeypatch):
    """A PeriodicPadding2D U-Net on 24 x 72 (closes under two poolings): predict and a 3-forward rollout against the float64 oracle
    at FWD_TOL; 1 member == the same member among 9, bit for bit; DLWP_FEW_WINO=0 keeps the direct first layer; the training step
    of the same model takes the direct first layer and leaves the handle's option at 0."""
    from tests.test_gpu_model import FWD_TOL, _rel, _weights_of
    cs = (4, 24, 72)
    rng = np.random.default_rng(7700)
    d, layers = _unet(cs)
    weights = _weights_of(d.model, rng)
    ex = d.model.executor
    op, desc = _first_conv(ex)
    assert ex.few_wino() and ops.conv_launch_info((9,) + tuple(op.xs), desc, ex._conv_dtype(op))[0][0] == -5
    x = rng.standard_normal((9,) + cs).astype(np.float32)
    got = d.predict(x)
    want = np_ref.run_layers(layers, x, weights)
    assert _rel(got, want) < FWD_TOL
    assert np.array_equal(d.predict(x[4:5]), got[4:5])                      # 1 member == the member among 9
    ser = d.model.rollout_on_device(torch.from_numpy(x).cuda(), 3).cpu().numpy()
    state = x
    for k in range(3):
        state = np_ref.run_layers(layers, state, weights)
        assert _rel(ser[k], state) < FWD_TOL, k
    one = d.model.rollout_on_device(torch.from_numpy(x[4:5]).cuda(), 3).cpu().numpy()
    assert np.array_equal(one[:, 0], ser[:, 4])
    assert ops.set_few_wino(0) == 0                                         # the scopes closed behind themselves
    # the rollout really ran the Winograd first layer: another family's round-off than the direct kernel's
    monkeypatch.setenv('DLWP_FEW_WINO', '0')
    d0, _ = _unet(cs)
    d0.model.set_weights(d.model.get_weights())
    ex0 = d0.model.executor
    op0, desc0 = _first_conv(ex0)
    assert not ex0.few_wino()
    assert ops.conv_launch_info((256,) + tuple(op0.xs), desc0, ex0._conv_dtype(op0))[0][0] == -2
    got0 = d0.predict(x)
    assert _rel(got0, want) < FWD_TOL and not np.array_equal(got0, got)
    monkeypatch.delenv('DLWP_FEW_WINO')
    # training: the plan that materialises both tensors; its first layer is not the Winograd kernel, before and after a step
    y = rng.standard_normal((9,) + cs).astype(np.float32)
    vals = d.model.train_on_batch(x, y)
    assert np.isfinite(vals[0])
    tex = d.model.train_executor
    opt, desct = _first_conv(tex)
    assert not tex.few_wino() and not getattr(desct, 'few_wino', False)
    assert all(i[0] != -5 for i in ops.conv_launch_info((9,) + tuple(opt.xs), desct, tex._conv_dtype(opt)))
    assert ops.set_few_wino(0) == 0


def test_few_wino_item_order_visits_every_tile_of_every_sample_once():
    """csrc/conv_fwd_few_wino.hip shares conv_fwd_few.hip's item arithmetic and grid: three workgroups per CU, one item per
    workgroup below that, sample groups as long as a share (at least 4, at most the batch).  Restated here: every (position,
    sample) item exactly once for any batch, tiling and CU count."""
    def visit(n, npos, cus):
        total = npos * n
        grid = min(total, 3 * cus)
        group = (total + grid // 2) // grid
        group = 4 if group < 4 else (n if group > n else group)
        seen = set()
        for b in range(grid):
            xcd, idx, q, r = b & 7, b >> 3, grid >> 3, grid & 7
            lidx = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
            it = total * lidx // grid
            left = total * (lidx + 1) // grid - it
            assert left >= 1                                   # grid <= items: no idle workgroup
            per = npos * group
            sg, rem = divmod(it, per)
            g0 = sg * group
            gs = min(group, n - g0)
            pos, sn = divmod(rem, gs)
            for _ in range(left):
                assert 0 <= pos < npos and 0 <= g0 + sn < n and gs > 0
                assert (pos, g0 + sn) not in seen
                seen.add((pos, g0 + sn))
                sn += 1
                if sn == gs:
                    sn, pos = 0, pos + 1
                    if pos == npos:
                        pos, g0 = 0, g0 + gs
                        gs = min(group, n - g0)
        assert len(seen) == total, (n, npos, cus)
    for n in list(range(1, 12)) + [63, 70, 128, 256, 257, 300, 1031]:
        for npos in (1, 4, 6, 9, 66):
            for cus in (1, 15, 256, 304):
                visit(n, npos, cus)


def test_executor_predicate_refuses_what_the_kernel_does_not_cover():
    """ops.few_wino_qualifies -- what makes an inference executor scope the option: 3x3, dilation 2, at most four input channels,
    whole 32-channel tiles, the pooling epilogue, float32 storage, a plain source."""
    from dlwp_amd import _lib, ops
    pad = ops.make_pad(2, 2, 2, 2, 0, 1)
    ok = ops.make_conv(32, 3, 3, 2, pad, 1, out_pool=True)
    assert ops.few_wino_qualifies(4, ok) and ops.few_wino_qualifies(1, ok) and ops.few_wino_qualifies(3, ops.make_conv(64, 3, 3, 2, pad, 0, out_pool=True))
    assert not ops.few_wino_qualifies(9, ok) and not ops.few_wino_qualifies(5, ok)
    assert not ops.few_wino_qualifies(4, ops.make_conv(32, 5, 5, 2, pad, 1, out_pool=True))            # 5x5
    assert not ops.few_wino_qualifies(4, ops.make_conv(32, 3, 3, 2, pad, 1))                           # unpooled
    assert not ops.few_wino_qualifies(4, ok, in_bf16=True) and not ops.few_wino_qualifies(4, ok, out_bf16=True)   # bf16 storage
    assert not ops.few_wino_qualifies(4, ops.make_conv(48, 3, 3, 2, pad, 1, out_pool=True))            # Cout % 32 != 0
    assert not ops.few_wino_qualifies(4, ops.make_conv(32, 3, 3, 1, pad, 1, out_pool=True))            # dilation 1
    assert not ops.few_wino_qualifies(4, ops.make_conv(32, 3, 3, 2, pad, 1, src_mode=_lib.SRC_UPSAMPLE2, out_pool=True))
    assert _lib.OPT_FEW_WINO == 10
