"""dlwp_conv2d_bwd_weight, dlwp_conv2d_bwd_weight_pooled and the dlwp_conv2d_bwd_data family against the float64 oracle
np_ref.conv_layer_grads at TRAINING size: the layers of presets.unet_layers((4, 88, 180)) at up to 64 samples (oracle/conv_grad_cases.py),
on the two input families of tests/test_conv_grads_cpu.py:
 (a) exact integers -- every kernel of every family must return the float64 sums TO THE BIT (`==`, no tolerance), at both settings of
     DLWP_OPT_WGRAD_FILL, on every compiled configuration that accepts the layer, and in every calling form;
 (b) random reals -- inside the bound derived in tests/test_conv_grads_cpu.py where the path was counted (the 4-channel streaming weight
     gradient with its slab sums), else inside the project's bars: GRAD_BAR 2e-5 of max(1, max |ref|) for weight gradients, FWD_TOL 1e-5
     of max(1, max |ref|) for the data gradient's convolution.
Outputs start as NaN between guard elements, every call runs twice and must give the same bits.  `-s` prints the picked forms and the
measured error / bound ratios; DESIGN.md section 4 holds them."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_ref
from oracle import conv_grad_cases as cases
from tests.test_conv_grads_cpu import (FWD_TOL, GRAD_BAR, U, c4_bound_count, c4_launch, c4_pooled_counts, ceil_div, exact_act_values,
                                       reduce_plan)
from tests.test_gpu_train_ops import Slab, same_bits

pytestmark = pytest.mark.gpu

LAYERS = cases.LAYERS
FORM_NAMES = {0: 'direct', 1: 'winograd', 3: 'channel-block', 4: 'c4'}
# the form the heuristic is expected to pick at 64 samples: (form, packed-N?)
EXPECTED_FORM = {'L1': (4, False), 'L2': (3, False), 'L3': (3, False), 'L4': (3, False), 'L5': (1, False), 'L6': (0, True)}
WORST = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def cd_of(ops, L, **kw):
    lay = L['layer']
    return ops.make_conv(L['cout'], lay['k'], lay['k'], lay['dil'], ops.make_pad(*lay['pads'], lay['mode_h'], lay['mode_w']),
                         ops.ACT_LINEAR, src_mode=lay['src'], **kw)


def shape_of(L, n):
    from dlwp_amd import _lib
    return _lib.Shape4(n, L['cin'], L['hs'], L['ws'])


def pick_of(ops, L, n):
    from dlwp_amd import _lib
    cd = cd_of(ops, L)
    return int(_lib.lib.dlwp_conv2d_wgrad_pick_config(_lib.handle(0), shape_of(L, n), ctypes.byref(cd)))


def set_fill(v):
    from dlwp_amd import _lib
    _lib.set_option(_lib.OPT_WGRAD_FILL, v)


def oracle(L, x, w, dz, **kw):
    return np_ref.conv_layer_grads(x, w, dz, L['layer'], use_torch=x.shape[0] >= 8, **kw)


def oracle_exact(L, x, w, dz, gain, **kw):
    """family (a): the oracle, and the exactness condition asserted on these very arrays"""
    a = oracle(L, x, w, dz, want=('dw',), absolute=True)['dw']
    assert cases.exact_condition(a, gain) < cases.LIMIT, 'gain %g * A %g reaches 2^22' % (gain, a.max())
    return oracle(L, x, w, dz, **kw)


def twice(call, *outs):
    """run `call` (which writes the Slabs `outs`) twice, each time from their initial contents (NaN, or an accumulator's values):
    the same bits, the guards untouched.  Returns the first Slab's result (all of them for several)."""
    res = []
    for _ in range(2):
        for o in outs:
            o.buf.copy_(torch.from_numpy(o.host))
        ret = call()
        res.append([o.read() for o in outs] + [ret])
    for a, b in zip(res[0][:-1], res[1][:-1]):
        assert same_bits(a, b), 'two runs of the same call differ'
    return res[0][0] if len(outs) == 1 else res[0][:-1]


def wgrad(ops, L, xd, dzd, n, cd=None, accumulate=None, ws_key=None):
    k = L['layer']['k']
    out = Slab(accumulate, shape=(k, k, L['cin'], L['cout']))
    cd = cd_of(ops, L) if cd is None else cd
    if accumulate is not None:
        return twice(lambda: ops.conv2d_bwd_weight(xd, dzd, out.t, cd, shape_of(L, n), accumulate=True, ws_key=ws_key), out)
    return twice(lambda: ops.conv2d_bwd_weight(xd, dzd, out.t, cd, shape_of(L, n), ws_key=ws_key), out)


def dgrad(ops, L, dzd, wd, n, cd=None, stored=False, prepared=None, cin_total=None):
    f = {0: 1.0, 1: 1.0 if stored else 2.0, 2: 0.5}[L['layer']['src']]       # the plane the entry point writes (not the output's:
    hin, win = int(L['hs'] * f), int(L['ws'] * f)                               # an asymmetric halo makes that one larger)
    out = Slab(None, shape=(n, cin_total or L['cin'], hin, win))
    cd = cd_of(ops, L) if cd is None else cd
    return twice(lambda: ops.conv2d_bwd_data(dzd, wd, cd, shape_of(L, n), out.t, prepared=prepared, stored=stored), out), f


def equal64(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(got, want), '%s: exact inputs, yet %d of %d elements differ, worst by %r' % (
        what, int((got != want).sum()), got.size, float(np.nanmax(np.abs(got - want))) if np.isfinite(got).any() else 'nan')


def accepted_wgrad_configs(ops, L, n):
    """every compiled weight-gradient configuration that takes the layer when forced"""
    out = []
    try:
        for i in range(len(ops.wgrad_configs())):
            ops.force_wgrad_config(i)
            if pick_of(ops, L, n) == i:
                out.append(i)
    finally:
        ops.force_wgrad_config(-1)
    return out


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


# ------------------------------------------------------------------------------------------------------------------ #
# family (a)
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('n', [1, 3, 8, 64])
@pytest.mark.parametrize('name', ['L1', 'L2', 'L3', 'L4', 'L5', 'L6'])
def test_weight_gradient_exact(ops, name, n):
    """family (a): the heuristic's kernel at both fills -- and at 64 samples every configuration that accepts the layer -- returns
    the float64 weight gradient to the bit."""
    L = LAYERS[name]
    cfgs, forms = ops.wgrad_configs(), ops.wgrad_config_forms()
    pick = pick_of(ops, L, n)
    assert pick >= 0
    form = (forms[pick][1], cfgs[pick][4] < 0)
    if n == 64:
        assert form == EXPECTED_FORM[name], (name, pick, cfgs[pick], forms[pick])
    forced = accepted_wgrad_configs(ops, L, n) if n == 64 else []
    print('\nPICK %s n=%d: config %d %r form %s%s; %d configurations accept the layer' % (
        name, n, pick, cfgs[pick], FORM_NAMES[form[0]], ' packed-N' if form[1] else '', len(forced)))
    gain = L['gain'] if (n == 64 or form[0] in (1, 3)) else L['pick_gain']
    seen_x = seen_z = None
    try:
        for seed in (0, 1):
            x, dz, w = cases.exact_case(L, n, seed, gain)
            seen_x = (x != 0) if seen_x is None else seen_x | (x != 0)
            seen_z = (dz != 0) if seen_z is None else seen_z | (dz != 0)
            ref = oracle_exact(L, x, w, dz, gain, want=('dw',))['dw']
            xd, dzd = dev(x), dev(dz)
            for fill in (1, 4):
                set_fill(fill)
                equal64(wgrad(ops, L, xd, dzd, n), ref, '%s n=%d seed %d fill %d' % (name, n, seed, fill))
            for i in forced:
                ops.force_wgrad_config(i)
                equal64(wgrad(ops, L, xd, dzd, n), ref, '%s n=%d seed %d forced configuration %d %r' % (name, n, seed, i, cfgs[i]))
            ops.force_wgrad_config(-1)
    finally:
        ops.force_wgrad_config(-1)
        set_fill(4)
    assert seen_x.all() and seen_z.all()


@pytest.mark.parametrize('name,n', [('L1', 520), ('L6', 520), ('C1a', 8), ('C1b', 8), ('L1x', 2), ('L5x', 2)])
def test_weight_and_data_gradient_exact_other_sizes(ops, name, n):
    """family (a) at 520 samples (8 distinct samples 65 times over: the oracle's sums are linear in the batch), config 1's 5x5 layers on
    the odd 73 x 144 grid, and the first / fifth layer at 180 x 360."""
    L = LAYERS[name]
    reps = 65 if n == 520 else 1
    nd = n // reps
    forms = ops.wgrad_config_forms()
    pick = pick_of(ops, L, n)
    gain = L['gain'] if forms[pick][1] in (1, 3) else cases.GAIN_WGRAD_DIRECT
    print('\nPICK %s n=%d: config %d form %s' % (name, n, pick, FORM_NAMES[forms[pick][1]]))
    for seed in (0, 1):
        x, dz, w = cases.exact_case(L, nd, seed, gain * reps)     # (thinned for the whole batch's sums)
        r = oracle_exact(L, x, w, dz, gain * reps)
        xd, dzd = dev(x).repeat(reps, 1, 1, 1), dev(dz).repeat(reps, 1, 1, 1)
        equal64(wgrad(ops, L, xd, dzd, n), reps * r['dw'], '%s n=%d seed %d dw' % (name, n, seed))
        if (name, n) != ('L1', 520):                  # (the first layer reads the model input: no data gradient in training)
            got, _ = dgrad(ops, L, dzd, dev(w), n)
            for rep in range(reps):
                equal64(got[rep * nd:(rep + 1) * nd], r['dx'], '%s n=%d seed %d dx, repetition %d' % (name, n, seed, rep))


@pytest.mark.parametrize('act', ['tanh', 'relu', 'linear'])
@pytest.mark.parametrize('n', [3, 64])
def test_first_layer_pooled_weight_and_bias_gradient_exact(ops, act, n):
    """dlwp_conv2d_bwd_weight_pooled on L1, family (a): the layer output y holds multiples of 1/2 in [-1, 1] with ties inside most
    windows (1 - y^2 is then a multiple of 1/4), the pooled gradient small integers: dw and db equal the float64 sums of
    np_ref.pool_act_bwd + conv_layer_grads to the bit."""
    L = LAYERS['L1']
    assert ops.conv2d_bwd_weight_pooled_supported(shape_of(L, n), cd_of(ops, L))
    for seed in (0, 1):
        x, _, w = cases.exact_case(L, n, seed, 4 * cases.GAIN_WGRAD_DIRECT)            # (1/4 units: four times the room)
        rng = np.random.default_rng([n, seed, 99])
        y = exact_act_values(rng, (n, L['cout'], L['ho'], L['wo']))
        dp = cases._ints(rng, (n, L['cout'], L['ho'] // 2, L['wo'] // 2), 1.0)
        dz = np_ref.pool_act_bwd(y, dp, act)
        ref = oracle_exact(L, x, w, dz, 4 * cases.GAIN_WGRAD_DIRECT, want=('dw',))['dw']
        db_ref = np_ref.channel_sum(dz)
        assert 4 * np.abs(np.asarray(dz, np.float64)).sum(axis=(0, 2, 3)).max() < cases.LIMIT
        k = L['layer']['k']
        dw, db = Slab(None, shape=(k, k, L['cin'], L['cout'])), Slab(None, shape=(L['cout'],))
        xd, yd, dpd = dev(x), dev(y), dev(dp)
        for fill in (1, 4):
            set_fill(fill)
            try:
                gw, gb = twice(lambda: ops.conv2d_bwd_weight_pooled(xd, yd, dpd, dw.t, db.t, cd_of(ops, L), shape_of(L, n),
                                                                    ops.ACTIVATIONS[act]) is None, dw, db)
            finally:
                set_fill(4)
            equal64(gw, ref, 'pooled dw %s n=%d seed %d fill %d' % (act, n, seed, fill))
            equal64(gb, db_ref, 'pooled db %s n=%d seed %d fill %d' % (act, n, seed, fill))


@pytest.mark.parametrize('n', [1, 3, 8, 64])
@pytest.mark.parametrize('name', ['L2', 'L3', 'L4', 'L5', 'L6', 'D3'])
def test_data_gradient_exact(ops, name, n):
    """family (a): dlwp_conv2d_bwd_data (dense dx, then dlwp_maxpool2_bwd / dlwp_upsample2_bwd where the source is pooled / up-sampled),
    _stored where the layer has the summing epilogue, _act on the 3x3 decoder shape (refused on the 5x5 layer), and at 64 samples every
    forward configuration that accepts the gradient's convolution."""
    from dlwp_amd._lib import DlwpError
    L = LAYERS[name]
    src = L['layer']['src']
    for seed in (0, 1):
        x, dz, w = cases.exact_case(L, n, seed)
        r = oracle(L, x, w, dz, want=('dx',))
        dzd, wd, xs = dev(dz), dev(w), shape_of(L, n)
        got, _ = dgrad(ops, L, dzd, wd, n)
        equal64(got, r['dx'], '%s n=%d seed %d dx' % (name, n, seed))
        if src == 2:
            routed = ops.maxpool2_bwd(dev(x), dev(got))                      # (integer x: ties in most windows)
            equal64(routed.cpu().numpy(), np_ref.maxpool2_grad(np.asarray(x, np.float64), r['dx']), '%s n=%d maxpool2_bwd' % (name, n))
        if src == 1:
            want = np_ref.upsample2_grad(r['dx'])
            equal64(ops.upsample2_bwd(dev(got)).cpu().numpy(), want, '%s n=%d two-call route' % (name, n))
            out = Slab(None, shape=(n, L['cin'], L['hs'], L['ws']))
            ok = ops.conv2d_bwd_data_stored(dzd, wd, cd_of(ops, L), xs, out.t)
            if ok:
                twice(lambda: ops.conv2d_bwd_data_stored(dzd, wd, cd_of(ops, L), xs, out.t), out)
            print('\nSTORED %s n=%d: %s' % (name, n, 'one kernel' if ok else 'unsupported, two calls'))
            if ok:
                equal64(out.read(), want, '%s n=%d stored' % (name, n))
            else:
                assert out.unchanged()
        if name in ('D3', 'L6'):
            for act in ('tanh', 'relu'):
                xa = exact_act_values(np.random.default_rng([n, seed, 5]), x.shape)
                ra = np_ref.conv_layer_grads(xa, w, dz, L['layer'], act_in=act, want=('dx',), use_torch=n >= 8)
                out, db = Slab(None, shape=ra['dx'].shape), Slab(None, shape=(L['cin'],))
                xad = dev(xa)
                ran = ops.conv2d_bwd_data_act(dzd, wd, cd_of(ops, L), xs, out.t, xad, ops.ACTIVATIONS[act], db.t)
                if ran:
                    twice(lambda: ops.conv2d_bwd_data_act(dzd, wd, cd_of(ops, L), xs, out.t, xad, ops.ACTIVATIONS[act], db.t), out, db)
                # refused on the 5x5 layer; fused on the decoder shape (from 4 samples on, as tests/test_gpu_train_fold.py holds it:
                # below, the heuristic may put the small gradient on an instance without that store phase)
                assert not (ran and name == 'L6') and (ran or name == 'L6' or n < 4), (name, n, act, ran)
                if ran:
                    equal64(out.read(), ra['dx'], '%s n=%d %s act dx' % (name, n, act))
                    equal64(db.read(), ra['db'], '%s n=%d %s act db' % (name, n, act))
                else:
                    assert out.unchanged() and db.unchanged()
        if n == 64 and seed == 0:
            tried = []
            try:
                lay = L['layer']
                for i, c in enumerate(ops.conv_configs()):
                    if c[:2] != (lay['k'], lay['dil']) or c[10] & 24:             # (another geometry; the bfloat16 instances)
                        continue
                    ops.force_conv_config(i)
                    out = Slab(None, shape=r['dx'].shape)
                    try:
                        ops.conv2d_bwd_data(dzd, wd, cd_of(ops, L), xs, out.t)
                    except DlwpError as e:
                        assert out.unchanged(), 'forward configuration %d refused the layer after writing' % i
                        print('forward configuration %d refused %s: %s' % (i, name, str(e)[:100]))
                        continue
                    equal64(twice(lambda: ops.conv2d_bwd_data(dzd, wd, cd_of(ops, L), xs, out.t), out), r['dx'],
                            '%s forced forward configuration %d' % (name, i))
                    tried.append(i)
            finally:
                ops.force_conv_config(-1)
            print('\nFORWARD CONFIGURATIONS %s: %r accept the data gradient' % (name, tried))
            assert len(tried) >= 1


@pytest.mark.parametrize('family', ['a', 'b'])
@pytest.mark.parametrize('name,n', [('D3', 8), ('D3', 64), ('L6', 8), ('L6', 64)])
def test_calling_forms(ops, name, n, family):
    """The 64 -> 32 decoder shape at 44 x 90 and the 5x5 output layer at 88 x 180, both families: accumulate on a pre-filled dw, dz / x
    as windows of wider NaN tensors, dx into a window of a wider NaN buffer, prepared weights (alone and between prepare_begin /
    _flush), the paired launch and the deferred slab sums.  Family (a): all equal the oracle, hence each other; family (b): inside
    GRAD_BAR (dw) and FWD_TOL (dx), the bars of the plain calls on these forms."""
    L = LAYERS[name]
    if family == 'a':
        x, dz, w = cases.exact_case(L, n, 0)
        r = oracle_exact(L, x, w, dz, L['gain'])
        pre = np.random.default_rng(1).integers(-3, 4, size=r['dw'].shape).astype(np.float32)
    else:
        x, dz, w = cases.real_case(L, n, 0)
        r = oracle(L, x, w, dz)
        pre = np.random.default_rng(1).standard_normal(r['dw'].shape).astype(np.float32)

    def same(got, want, what, bar):
        if family == 'a':
            return equal64(got, want, '%s %s n=%d' % (what, name, n))
        err, lim = np.abs(got - want).max(), bar * max(1.0, np.abs(want).max())
        note('%s n=%d forms / bar' % (name, n), err / lim)
        assert err <= lim, (what, name, n, err, lim)
    xd, dzd, wd, xs = dev(x), dev(dz), dev(w), shape_of(L, n)
    device = xd.device
    same(wgrad(ops, L, xd, dzd, n, accumulate=pre), r['dw'] + pre, 'accumulate', GRAD_BAR)
    # dz / x as windows of wider tensors, NaN elsewhere
    wide_z = torch.full((n, L['cout'] + 5, L['ho'], L['wo']), float('nan'), device=device)
    wide_z[:, 3:3 + L['cout']] = dzd
    wide_x = torch.full((n, L['cin'] + 3, L['hs'], L['ws']), float('nan'), device=device)
    wide_x[:, 2:2 + L['cin']] = xd
    cdw = cd_of(ops, L, out_c_off=3, out_c_total=L['cout'] + 5, in_c_off=2, in_c_total=L['cin'] + 3)
    same(wgrad(ops, L, wide_x, wide_z, n, cd=cdw), r['dw'], 'windows dw', GRAD_BAR)
    got, _ = dgrad(ops, L, wide_z, wd, n, cd=cdw, cin_total=L['cin'] + 3)
    same(got[:, 2:2 + L['cin']], r['dx'], 'windows dx', FWD_TOL)
    assert np.isnan(got[:, :2]).all() and np.isnan(got[:, 2 + L['cin']:]).all(), 'dx window: the other channels must stay NaN'
    # prepared, alone and recorded
    prep = ops.conv2d_bwd_data_prepare(wd, cd_of(ops, L), xs)
    assert prep is not None
    same(dgrad(ops, L, dzd, None, n, prepared=prep)[0], r['dx'], 'prepared', FWD_TOL)
    ops.prepare_begin(device)
    prep2 = ops.conv2d_bwd_data_prepare(wd, cd_of(ops, L), xs)
    ops.prepare_flush(device)
    same(dgrad(ops, L, dzd, None, n, prepared=prep2)[0], r['dx'], 'prepared in a batch', FWD_TOL)
    # the paired launch (the layer's weight gradient + its data gradient: two outputs that do not depend on each other)
    k = L['layer']['k']
    dw_p, dx_p = Slab(None, shape=(k, k, L['cin'], L['cout'])), Slab(None, shape=r['dx'].shape)
    fused0 = ops.pair_fused_count(device)

    def pair():
        ops.pair_begin(device)
        ops.conv2d_bwd_weight(xd, dzd, dw_p.t, cd_of(ops, L), xs, ws_key='pair')
        ops.conv2d_bwd_data(dzd, None, cd_of(ops, L), xs, dx_p.t, prepared=prep)
        ops.pair_end(device)
    gw, gx = twice(pair, dw_p, dx_p)
    print('\nPAIR %s n=%d: %d fused launch(es) in two runs' % (name, n, ops.pair_fused_count(device) - fused0))
    same(gw, r['dw'], 'pair dw', GRAD_BAR)
    same(gx, r['dx'], 'pair dx', FWD_TOL)
    # deferred final sums
    dw_r = Slab(None, shape=(k, k, L['cin'], L['cout']))

    def deferred():
        ops.reductions_begin(device)
        ops.conv2d_bwd_weight(xd, dzd, dw_r.t, cd_of(ops, L), xs, ws_key='deferred')
        ops.reductions_flush(device)
    same(twice(deferred, dw_r), r['dw'], 'deferred sums', GRAD_BAR)


@pytest.mark.parametrize('family', ['a', 'b'])
@pytest.mark.parametrize('n', [8, 64])
def test_phase_restated_output_layer(ops, n, family):
    """A 5x5 32 -> 4 layer on an up-sampled 44 x 90 source, restated on the source as training.py does for derived kernels: the 3x3
    layer with 16 phase channels gets its weight gradient from dlwp_conv2d_bwd_weight (dz in phase layout), dlwp_phase_weights_bwd
    gathers it (and the bias sums) onto the 5x5 kernel: against the oracle of the 5x5 layer itself."""
    P = dict(name='P6', cin=32, cout=4, hs=44, ws=90, ho=88, wo=180, layer=np_ref.conv_layer(5, 1, src=1), gain=cases.GAIN_WGRAD_WINO)
    D = dict(name='P6d', cin=32, cout=16, hs=44, ws=90, ho=44, wo=90, layer=np_ref.conv_layer(3, 1), gain=cases.GAIN_WGRAD_WINO)
    assert ops.phase_geometry(5, 2) == (3, -1, 1)
    for seed in (0, 1):
        if family == 'a':
            x, dz, w = cases.exact_case(P, n, seed)
            ref = oracle_exact(P, x, w, dz, P['gain'], want=('dw',))['dw']
        else:
            x, dz, w = cases.real_case(P, n, seed)
            ref = oracle(P, x, w, dz, want=('dw',))['dw']
        db_ref = np_ref.channel_sum(dz)
        dz2 = dev(np_ref.space_to_depth2(dz))
        dw2 = dev(wgrad(ops, D, dev(x), dz2, n))
        db2 = torch.empty(16, device='cuda')
        ops.bias_grad(dz2, db2, 16)
        dw, db = Slab(None, shape=(5, 5, 32, 4)), Slab(None, shape=(4,))
        gw, gb = twice(lambda: ops.phase_weights_bwd(dw2, db2, dw.t, db.t, 2, 2) is None, dw, db)
        if family == 'a':
            equal64(gw, ref, 'phase-restated dw n=%d seed %d' % (n, seed))
            equal64(gb, db_ref, 'phase-restated db n=%d seed %d' % (n, seed))
        else:
            err, lim = np.abs(gw - ref).max(), GRAD_BAR * max(1.0, np.abs(ref).max())
            note('phase-restated n=%d dw / GRAD_BAR' % n, err / lim)
            assert err <= lim and np.abs(gb - db_ref).max() <= GRAD_BAR * max(1.0, np.abs(db_ref).max())


@pytest.mark.parametrize('hw', [(88, 180), (73, 144)])
@pytest.mark.parametrize('pads,mode_h,mode_w', [((1, 1, 1, 1), 2, 1), ((1, 1, 1, 1), 3, 3), ((1, 1, 1, 1), 4, 4), ((1, 2, 2, 1), 0, 1),
                                                ((1, 1, 1, 1), 1, 2)])
def test_fold_back_route_exact(ops, hw, pads, mode_h, mode_w):
    """family (a) through the general route (full correlation into the padded gradient, dlwp_pad2d_bwd folds the halo back): edge,
    reflect, symmetric and asymmetric halos, periodic rows, at the widths where dlwp_pad2d_bwd takes its flat-row kernels; the weight
    gradient's loader maps the same halos."""
    n, cin, cout = 4, 16, 24
    h, w_ = hw
    lay = np_ref.conv_layer(3, 1, pads=pads, mode_h=mode_h, mode_w=mode_w)
    ho, wo = h + pads[0] + pads[1] - 2, w_ + pads[2] + pads[3] - 2
    L = dict(name='fold', cin=cin, cout=cout, hs=h, ws=w_, ho=ho, wo=wo, layer=lay, gain=cases.GAIN_WGRAD_WINO)
    for seed in (0, 1):
        x, dz, w = cases.exact_case(L, n, seed)
        r = oracle(L, x, w, dz)
        a = oracle(L, x, w, dz, want=('dw',), absolute=True)['dw']
        assert cases.exact_condition(a, L['gain']) < cases.LIMIT                    # (the condition, on this case's own halos)
        got, _ = dgrad(ops, L, dev(dz), dev(w), n)
        equal64(got, r['dx'], 'fold-back dx %r %d %d seed %d' % (pads, mode_h, mode_w, seed))
        equal64(wgrad(ops, L, dev(x), dev(dz), n), r['dw'], 'fold-back dw %r %d %d seed %d' % (pads, mode_h, mode_w, seed))


def test_empty_batch(ops):
    """What the entry points do today with a shape of no samples (the tensors themselves hold one sample: an empty torch tensor has no
    address to hand over): every data gradient -- plain, prepared, _stored, _act -- returns success without writing anything (the
    bias gradient of _act included); the weight gradients, plain and pooled, refuse and write nothing."""
    from dlwp_amd._lib import DlwpError
    L = LAYERS['D3']
    x, dz, w = cases.exact_case(L, 1, 0)
    xd, dzd, wd = dev(x), dev(dz), dev(w)
    dx, db = Slab(None, shape=(1, L['cin'], L['hs'], L['ws'])), Slab(None, shape=(L['cin'],))
    ops.conv2d_bwd_data(dzd, wd, cd_of(ops, L), shape_of(L, 0), dx.t)
    assert dx.unchanged()
    prep = ops.conv2d_bwd_data_prepare(wd, cd_of(ops, L), shape_of(L, 1))
    ops.conv2d_bwd_data(dzd, None, cd_of(ops, L), shape_of(L, 0), dx.t, prepared=prep)
    assert dx.unchanged()
    assert ops.conv2d_bwd_data_prepare(wd, cd_of(ops, L), shape_of(L, 0)) is None             # (no prepared form of no samples)
    assert ops.conv2d_bwd_data_act(dzd, wd, cd_of(ops, L), shape_of(L, 0), dx.t, xd, ops.ACT_TANH, db.t) is True
    assert dx.unchanged() and db.unchanged()
    dw = Slab(None, shape=w.shape)
    with pytest.raises(DlwpError):
        ops.conv2d_bwd_weight(xd, dzd, dw.t, cd_of(ops, L), shape_of(L, 0))
    assert dw.unchanged()
    L4 = LAYERS['L4']
    x4, dz4, w4 = cases.exact_case(L4, 1, 0)
    dx4 = Slab(None, shape=x4.shape)
    assert ops.conv2d_bwd_data_stored(dev(dz4), dev(w4), cd_of(ops, L4), shape_of(L4, 0), dx4.t) is True
    assert dx4.unchanged()
    L1 = LAYERS['L1']
    x1, dz1, w1 = cases.exact_case(L1, 1, 0)
    dw1, db1 = Slab(None, shape=w1.shape), Slab(None, shape=(L1['cout'],))
    dp1 = dev(dz1[:, :, ::2, ::2])
    with pytest.raises(DlwpError):
        ops.conv2d_bwd_weight_pooled(dev(x1), dev(dz1), dp1, dw1.t, db1.t, cd_of(ops, L1), shape_of(L1, 0), ops.ACT_TANH)
    assert dw1.unchanged() and db1.unchanged()


# ------------------------------------------------------------------------------------------------------------------ #
# family (b)
# ------------------------------------------------------------------------------------------------------------------ #

def cu_count():
    from dlwp_amd import _lib
    cu = ctypes.c_int(0)
    _lib.check(_lib.lib.dlwp_device_info(_lib.handle(torch.cuda.current_device()), ctypes.byref(cu), None, None, 0))
    return cu.value


@pytest.mark.parametrize('name,n', [(nm, 8) for nm in ('L1', 'L2', 'L3', 'L4', 'L5', 'L6', 'D3')] +
                         [('L1', 64), ('L6', 64)])
def test_gradients_of_random_reals_inside_the_bounds(ops, name, n):
    """family (b).  The 4-channel streaming form (L1): error <= c u A per weight with c counted in tests/test_conv_grads_cpu.py
    (c4_bound_count) and A = sum |x| |dz| from the oracle; the Winograd and packed-N weight gradients: GRAD_BAR; data gradients: FWD_TOL.
    At 8 samples everywhere, at 64 on L1 and L6: with L2 and L5 at 64 samples as well (measured: dw 0.044 and 0.086 of GRAD_BAR, dx 0.037
    and 0.029 of FWD_TOL) this file took 128 s beside 145 s for the rest of the GPU suite, so those two float64 sums were dropped."""
    L = LAYERS[name]
    x, dz, w = cases.real_case(L, n, 0)
    want = ('dw',) if name == 'L1' else ('dw', 'dx')
    r = oracle(L, x, w, dz, want=want)
    cfgs, forms = ops.wgrad_configs(), ops.wgrad_config_forms()
    pick = pick_of(ops, L, n)
    xd, dzd = dev(x), dev(dz)
    for fill in (1, 4):
        set_fill(fill)
        try:
            got = wgrad(ops, L, xd, dzd, n)
        finally:
            set_fill(4)
        err = np.abs(got - r['dw'])
        bar = GRAD_BAR * max(1.0, np.abs(r['dw']).max())
        note('%s n=%d dw / GRAD_BAR' % (name, n), err.max() / bar)
        if forms[pick][1] != 4:                                  # (no counted bound for this form: the project's bar)
            assert err.max() <= bar, (name, n, fill, err.max(), bar)
        else:
            a = oracle(L, x, w, dz, want=('dw',), absolute=True)['dw']
            c = c4_bound_count(n, L['ho'], L['wo'], L['cout'], cfgs[pick][2], cfgs[pick][3], cu_count(), fill)
            ratio = (err / (c * U * a)).max()
            note('%s n=%d fill %d dw / (c u A), c = %d' % (name, n, fill, c), ratio)
            note('%s n=%d fill %d dw / (u A)' % (name, n, fill), (err / (U * a)).max())
            note('%s n=%d fill %d dw error / max |ref|' % (name, n, fill), err.max() / np.abs(r['dw']).max())
            assert ratio <= 1.0, (name, n, fill, ratio)
    if 'dx' in r:
        got, _ = dgrad(ops, L, dzd, dev(w), n)
        err = np.abs(got - r['dx']).max()
        bar = FWD_TOL * max(1.0, np.abs(r['dx']).max())
        note('%s n=%d dx / FWD_TOL' % (name, n), err / bar)
        assert err <= bar, (name, n, err, bar)
    if name == 'D3':
        xa = np.tanh(x).astype(np.float32)
        ra = np_ref.conv_layer_grads(xa, w, dz, L['layer'], act_in='tanh', want=('dx',), use_torch=True)
        out, db = Slab(None, shape=ra['dx'].shape), Slab(None, shape=(L['cin'],))
        assert ops.conv2d_bwd_data_act(dzd, dev(w), cd_of(ops, L), shape_of(L, n), out.t, dev(xa), ops.ACT_TANH, db.t)
        err = np.abs(out.read() - ra['dx']).max()
        note('D3 n=%d act dx / FWD_TOL' % n, err / (FWD_TOL * max(1.0, np.abs(ra['dx']).max())))
        assert err <= FWD_TOL * max(1.0, np.abs(ra['dx']).max())
        errb = np.abs(db.read() - ra['db']).max()
        note('D3 n=%d act db / GRAD_BAR' % n, errb / (GRAD_BAR * max(1.0, np.abs(ra['db']).max())))
        assert errb <= GRAD_BAR * max(1.0, np.abs(ra['db']).max())


@pytest.mark.parametrize('n', [8, 64])
def test_first_layer_pooled_random_reals_inside_the_counted_bounds(ops, n):
    """dlwp_conv2d_bwd_weight_pooled, family (b): y = tanh of normals (float32), the pooled gradient normal; dw inside c_dw u A and db
    inside c_db u sum |dz| with the counts of c4_pooled_counts; A and the float64 dz from np_ref.pool_act_bwd"""
    L = LAYERS['L1']
    x, _, w = cases.real_case(L, n, 1)
    rng = np.random.default_rng([n, 77])
    y = np.tanh(rng.standard_normal((n, L['cout'], L['ho'], L['wo']))).astype(np.float32)
    dp = rng.standard_normal((n, L['cout'], L['ho'] // 2, L['wo'] // 2)).astype(np.float32)
    dz = np_ref.pool_act_bwd(y, dp, 'tanh')
    ref = oracle(L, x, w, dz, want=('dw',))['dw']
    a = oracle(L, x, w, dz, want=('dw',), absolute=True)['dw']
    db_ref, a_db = np_ref.channel_sum(dz), np.abs(dz).sum(axis=(0, 2, 3))
    cfgs = ops.wgrad_configs()
    pick = pick_of(ops, L, n)
    assert ops.wgrad_config_forms()[pick][1] == 4
    k = L['layer']['k']
    dw, db = Slab(None, shape=(k, k, L['cin'], L['cout'])), Slab(None, shape=(L['cout'],))
    xd, yd, dpd = dev(x), dev(y), dev(dp)
    gw, gb = twice(lambda: ops.conv2d_bwd_weight_pooled(xd, yd, dpd, dw.t, db.t, cd_of(ops, L), shape_of(L, n), ops.ACT_TANH) is None,
                   dw, db)
    c_dw, c_db = c4_pooled_counts(n, L['ho'], L['wo'], L['cout'], cfgs[pick][2], cfgs[pick][3], cu_count(), 4)
    r_dw, r_db = (np.abs(gw - ref) / (c_dw * U * a)).max(), (np.abs(gb - db_ref) / (c_db * U * a_db)).max()
    note('L1 pooled n=%d dw / (c u A), c = %d' % (n, c_dw), r_dw)
    note('L1 pooled n=%d db / (c u A), c = %d' % (n, c_db), r_db)
    assert r_dw <= 1.0 and r_db <= 1.0, (n, r_dw, r_db)


def test_first_layer_partial_sums_where_the_round_off_arises(ops):
    """L1 at 64 samples, family (b): the slabs dlwp_conv2d_bwd_weight leaves in its workspace -- one per (split, wave), except that the
    chunked first pass of the slab sums has put each chunk's sum into the chunk's first slab -- against float64 partial sums of the
    same tiles and pixel groups (conv_wgrad_c4_kernel.h: a wave owns GPW consecutive 16-pixel groups of a tile, whole rows here), each
    inside (1 + per TH TW / 4) u A_slab; the chunk sums inside that + depth(cs); the final dw inside c u A.  The slab count read back
    from the workspace size confirms the launch restated in tests/test_conv_grads_cpu.py, and that the chunked pass is taken."""
    from dlwp_amd import _lib
    L, n = LAYERS['L1'], 64
    cfgs = ops.wgrad_configs()
    pick = pick_of(ops, L, n)
    th, tw = cfgs[pick][2], cfgs[pick][3]
    assert ops.wgrad_config_forms()[pick][1] == 4
    x, dz, w = cases.real_case(L, n, 0)
    xd, dzd = dev(x), dev(dz)
    wn = 9 * L['cin'] * L['cout']
    tiles, splits, per = c4_launch(n, L['ho'], L['wo'], L['cout'], th, tw, cu_count(), 4)
    need = ops.conv_bwd_workspace_bytes(0, shape_of(L, n), cd_of(ops, L), 1)
    assert need == 4 * splits * wn * 4, 'the restated launch: %d slabs, the library: %d bytes of %d' % (4 * splits, need, wn * 4)
    gx, cs, ny = reduce_plan(wn, 4 * splits, cu_count())
    assert cs > 0 and gx < 128, 'the first layer at 64 samples must take the chunked first pass of the slab sums'
    got = wgrad(ops, L, xd, dzd, n, ws_key='partials')
    torch.cuda.synchronize()
    slabs = ops.workspace(xd.device, need, 'partials')[:need].view(torch.float32).cpu().numpy().reshape(4 * splits, wn).astype(np.float64)
    # float64 partials per (tile, wave)
    gpr, gpw = tw // 16, th * tw // 64
    assert gpw % gpr == 0
    rpw = gpw // gpr                                                     # whole tile rows per wave
    t_h, t_w = ceil_div(L['ho'], th), ceil_div(L['wo'], tw)
    d = L['layer']['dil']
    xp = np_ref.pad2d_modes(np.asarray(x, np.float64), L['layer']['pads'], 0, 1)

    def tiled(a):                                                        # (n, c, ho, wo) -> (n, c, t_h, 4, rpw, t_w, tw), zero-filled
        full = np.zeros(a.shape[:2] + (t_h * th, t_w * tw))
        full[:, :, :a.shape[2], :a.shape[3]] = a
        return full.reshape(a.shape[0], a.shape[1], t_h, 4, rpw, t_w, tw)
    part = np.zeros((n, t_h, t_w, 4, 9, L['cin'], L['cout']))
    part_abs = np.zeros_like(part)
    z64 = tiled(np.asarray(dz, np.float64))
    for tap in range(9):
        u, v = tap // 3, tap % 3
        xt = tiled(xp[:, :, u * d:u * d + L['ho'], v * d:v * d + L['wo']])
        part[:, :, :, :, tap] = np.einsum('nchwrsq,nohwrsq->nhswco', xt, z64, optimize=True)
        part_abs[:, :, :, :, tap] = np.einsum('nchwrsq,nohwrsq->nhswco', np.abs(xt), np.abs(z64), optimize=True)
    part, part_abs = part.reshape(tiles, 4, wn), part_abs.reshape(tiles, 4, wn)
    want = np.zeros((splits, 4, wn))
    want_abs = np.zeros((splits, 4, wn))
    for s_ in range(splits):
        want[s_] = part[s_ * per:(s_ + 1) * per].sum(0)
        want_abs[s_] = part_abs[s_ * per:(s_ + 1) * per].sum(0)
    want, want_abs = want.reshape(4 * splits, wn), want_abs.reshape(4 * splits, wn)
    first = np.arange(4 * splits) % cs == 0
    c_k = 1 + per * th * tw // 4
    r_slab = (np.abs(slabs - want)[~first] / (c_k * U * np.maximum(want_abs[~first], 1e-300))).max()
    c_c = c_k + ceil_div(ceil_div(cs, 4), 8) + 5
    chunk = np.add.reduceat(want, np.arange(0, 4 * splits, cs), axis=0)
    chunk_abs = np.add.reduceat(want_abs, np.arange(0, 4 * splits, cs), axis=0)
    r_chunk = (np.abs(slabs[first] - chunk) / (c_c * U * np.maximum(chunk_abs, 1e-300))).max()     # (the last splits walk no tile)
    c = c4_bound_count(n, L['ho'], L['wo'], L['cout'], th, tw, cu_count(), 4)
    total, total_abs = want.sum(0), want_abs.sum(0)
    r_final = (np.abs(got.reshape(-1) - total) / (c * U * total_abs)).max()
    rel = lambda e, ref: float(np.abs(e).max() / np.abs(ref).max())
    print('\nMEASURED L1 n=64 partials: %d slabs of %d tiles, chunks of %d; slab error / bound %.4f (c = %d), chunk sums %.4f (c = %d), '
          'dw %.4f (c = %d); error / max |ref|: slabs %.2e, dw %.2e; max |dw| / max A = %.2e' % (
              4 * splits, per, cs, r_slab, c_k, r_chunk, c_c, r_final, c, rel(slabs[~first] - want[~first], want[~first]),
              rel(got.reshape(-1) - total, total), np.abs(total).max() / total_abs.max()))
    note('L1 n=64 slab error / bound', r_slab)
    note('L1 n=64 chunk-sum error / bound', r_chunk)
    assert r_slab <= 1.0 and r_chunk <= 1.0 and r_final <= 1.0


def test_report():
    """prints the worst error / bound ratios of this session's family (b) cases (`-s`)"""
    for k in sorted(WORST):
        print('MEASURED %s: %.4g' % (k, WORST[k]))
