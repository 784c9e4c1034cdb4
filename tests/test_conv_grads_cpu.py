"""The CPU side of tests/test_gpu_conv_grads.py: the oracle np_ref.conv_layer_grads in its two forms, the exactness CONDITION of input
family (a) on every generated case, and the DERIVED bound of family (b) with float32 restatements, in the kernels' order, that stay
inside it.

Family (a) (oracle/conv_grad_cases.py): integer inputs; gain * A < 2^22 with A the absolute-value sum of a result element and `gain` the
largest gain of the transforms on the path (64 Winograd weight gradient, 1 direct forms, 81 data gradient: counted from the matrices in
oracle/conv_grad_cases.py) -- then float32 holds every intermediate exactly and every kernel must return the float64 sum to the bit.

Family (b), u = 2^-24, bound per element c u A:
 * the 4-channel streaming weight gradient (conv_wgrad_c4_kernel.h) + its slab sums (reduce_slabs_kernel): c is COUNTED below
   (c4_bound_count) as the number of roundings on the longest path of one term:
     1                       the product x * dz (counted as rounded, although the matrix instruction may fuse it)
     per * TH * TW / 4       additions into a wave's accumulator: a split walks per = ceil(tiles / splits) tiles, a wave owns a quarter
                             of a tile's TH * TW pixels, and each pixel's product is added in turn (the K = 4 of one
                             v_mfma_f32_16x16x4f32 counted as four sequential additions -- the worst case)
     depth(cs) + depth(Y)    the two passes of reduce_slabs_kernel over S = 4 * splits slabs (chunks of cs, then the Y chunk sums), where
                             depth(s) = ceil(ceil(s / 4) / 8) additions into one of a thread's 8 partial sums + 3 (the tree over the 8) + 2
                             (the tree over the 4 slab groups); one pass of depth(S) where the launcher does not chunk
   with splits, cs and Y restated from pick_wgrad (conv_bwd.hip) and dlwp_launch_reduce_slabs (train_ops.hip).
 * the Winograd weight gradients and the packed-N form were NOT counted (transforms, per-form tile walks): the project's bar GRAD_BAR =
   2e-5 of max(1, max |ref|) holds there; the data gradient is the forward convolution on the flipped kernel: FWD_TOL = 1e-5 of
   max(1, max |ref|), the forward bar of tests/test_gpu_model.py."""
import numpy as np
import pytest

from oracle import np_ref
from oracle import conv_grad_cases as cases

U = 2.0 ** -24
GRAD_BAR = 2e-5
FWD_TOL = 1e-5
CU = 256                      # compute units of an MI355X


def ceil_div(a, b):
    return -(-a // b)


def exact_act_values(rng, shape):
    """activation outputs in {-1, -1/2, 0, 1/2, 1}: 1 - y^2 is 0, 3/4 or 1, so an integer gradient times act'(y) is a multiple of 1/4;
    five values only: ties inside most pooling windows"""
    return (rng.integers(-2, 3, size=shape) * 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ #
# the launch geometry and the rounding count of the 4-channel form
# ------------------------------------------------------------------------------------------------------------------ #

def c4_launch(n, ho, wo, cout, th, tw, cu=CU, fill=4):
    """(tiles, splits, per) of pick_wgrad for a conv_wgrad_c4_kernel.h instance: 4 waves, one input-channel group, 32 output channels
    per workgroup (the 64 MiB slab cap is far away: 9 * 4 * 32 floats per slab)"""
    tiles = n * ceil_div(ho, th) * ceil_div(wo, tw)
    co_tiles = ceil_div(cout, 32)
    splits = max(1, min((cu * 2 * fill) // (4 * co_tiles), tiles // 2))
    return tiles, splits, ceil_div(tiles, splits)


def reduce_plan(n_elems, s, cu=CU):
    """dlwp_launch_reduce_slabs: (gx, cs, Y) -- cs = 0 without the chunked first pass"""
    want = ceil_div(n_elems, 256) if n_elems % 4 == 0 else ceil_div(4 * n_elems, 256)
    gx = max(1, min(want, cu * 8))
    if gx < 128 and s >= 64:
        y = min(512 // gx, s // 16)
        cs = ceil_div(s, y)
        return gx, cs, ceil_div(s, cs)
    return gx, 0, s


def reduce_depth(s):
    return ceil_div(ceil_div(s, 4), 8) + 3 + 2


def c4_bound_count(n, ho, wo, cout, th, tw, cu=CU, fill=4, cin=4):
    _, splits, per = c4_launch(n, ho, wo, cout, th, tw, cu, fill)
    _, cs, y = reduce_plan(9 * cin * cout, 4 * splits, cu)
    red = reduce_depth(cs) + reduce_depth(y) if cs else reduce_depth(y)
    return 1 + per * th * tw // 4 + red + 1          # (+ 1: the addition to dw with accumulate != 0)


# ------------------------------------------------------------------------------------------------------------------ #
# float32 restatements in the kernels' order
# ------------------------------------------------------------------------------------------------------------------ #

def reduce_slabs_f32(slabs, cu=CU):
    """reduce_slabs_kernel as dlwp_launch_reduce_slabs launches it: slabs (S, n) float32 -> (n,) float32, the same order of additions"""
    slabs = np.array(slabs, dtype=np.float32)
    s_all, n = slabs.shape

    def one_pass(sl):
        s = sl.shape[0]
        red = []
        for g in range(4):
            part = [np.zeros(n, np.float32) for _ in range(8)]
            k = g
            while k + 28 < s:
                for j in range(8):
                    part[j] = part[j] + sl[k + 4 * j]
                k += 32
            j = 0
            while k < s:
                part[j] = part[j] + sl[k]
                k += 4
                j += 1
            red.append(((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7])))
        return (red[0] + red[1]) + (red[2] + red[3])
    _, cs, y = reduce_plan(n, s_all, cu)
    if cs:
        slabs = np.stack([one_pass(slabs[i * cs:min((i + 1) * cs, s_all)]) for i in range(y)])
    return one_pass(slabs)


def c4_wgrad_f32(x, dz, dil, th, tw, splits):
    """conv2d_wgrad_c4_f32 on a plain source with zero rows / periodic columns, float32 in the kernel's order: split -> tiles in
    order -> wave (a quarter of the tile's 16-pixel groups) -> group -> r -> the four pixels 16 g + 4 kq + r of one matrix instruction,
    added one after the other; one slab per (split, wave).  Returns the slabs (4 * splits, 9 * cin * cout)."""
    n, cin, h, w = x.shape
    cout = dz.shape[1]
    xp = np_ref.pad2d_modes(x.astype(np.float32), (dil, dil, dil, dil), np_ref.PAD_ZERO, np_ref.PAD_WRAP).astype(np.float32)
    tiles_h, tiles_w = ceil_div(h, th), ceil_div(w, tw)
    total = n * tiles_h * tiles_w
    per = ceil_div(total, splits)
    gpr, gpw = tw // 16, th * tw // 16 // 4
    slabs = np.zeros((splits * 4, 9, cin, cout), np.float32)
    for split in range(splits):
        for t in range(split * per, min(total, (split + 1) * per)):
            ni, thi, twi = t // (tiles_h * tiles_w), (t // tiles_w) % tiles_h, t % tiles_w
            for wave in range(4):
                acc = slabs[split * 4 + wave]
                for k in range(gpw):
                    row = thi * th + (wave * gpw + k) // gpr
                    col0 = twi * tw + ((wave * gpw + k) % gpr) * 16
                    for r in range(4):
                        for kq in range(4):
                            col = col0 + 4 * kq + r
                            if row >= h or col >= w:
                                continue
                            for tap in range(9):
                                u, v = tap // 3, tap % 3
                                xv = xp[ni, :, row + u * dil, col + v * dil]
                                acc[tap] = acc[tap] + (xv[:, None] * dz[ni, :, row, col][None, :]).astype(np.float32)
    return slabs.reshape(splits * 4, -1)


# ------------------------------------------------------------------------------------------------------------------ #
# tests
# ------------------------------------------------------------------------------------------------------------------ #

SMALL = [  # cin, cout, k, dil, pads, mode_h, mode_w, src
    (3, 5, 3, 1, None, 0, 1, 0), (4, 6, 3, 2, None, 0, 1, 0), (3, 2, 5, 1, None, 0, 1, 0), (5, 4, 3, 1, None, 0, 1, 1),
    (5, 4, 3, 1, None, 0, 1, 2), (3, 4, 3, 2, (2, 1, 3, 2), 2, 1, 0), (2, 3, 3, 1, (1, 1, 1, 1), 3, 4, 0), (4, 3, 3, 1, (1, 1, 1, 1), 1, 2, 1)]


@pytest.mark.parametrize('case', SMALL)
def test_einsum_and_torch_forms_of_the_oracle_agree(case):
    """np_ref.conv_layer_grads: the einsum sums and torch's CPU float64 convolution gradients within 1e-12, with channel windows, the
    stored form of an up-sampled source, the activation form, and the absolute-value sums"""
    cin, cout, k, dil, pads, mh, mw, src = case
    rng = np.random.default_rng(cin * 100 + cout)
    n, hs, ws = 2, 10, 14
    lay = np_ref.conv_layer(k, dil, pads=pads, mode_h=mh, mode_w=mw, src=src, in_c_off=1, in_c=cin, out_c_off=2, out_c=cout)
    x = np.tanh(rng.standard_normal((n, cin + 2, hs, ws)))
    f = {0: 1.0, 1: 2.0, 2: 0.5}[src]
    p = lay['pads']
    ho, wo = int(hs * f) + p[0] + p[1] - dil * (k - 1), int(ws * f) + p[2] + p[3] - dil * (k - 1)
    dz = rng.standard_normal((n, cout + 3, ho, wo))
    w = rng.standard_normal((k, k, cin, cout))
    for kw in [dict(), dict(absolute=True)] + ([dict(stored=True)] if src == 1 else []) + ([dict(act_in='tanh'), dict(act_in='relu')] if src == 0 else []):
        a = np_ref.conv_layer_grads(x, w, dz, lay, **kw)
        b = np_ref.conv_layer_grads(x, w, dz, lay, use_torch=True, **kw)
        assert sorted(a) == sorted(b)
        for key in a:
            assert a[key].shape == b[key].shape
            assert np.abs(a[key] - b[key]).max() <= 1e-12 * max(1.0, np.abs(a[key]).max()), (case, kw, key)
    # against the forward oracle: <conv(x; w), dz> == <w, dw> == <x after the source transform, dx>
    r = np_ref.conv_layer_grads(x, w, dz, lay)
    xw, dzw = x[:, 1:1 + cin], dz[:, 2:2 + cout]
    xt = {0: xw, 1: np_ref.upsample2(xw), 2: np_ref.maxpool2(xw)}[src]
    y = np_ref.conv2d(np_ref.pad2d_modes(xt, lay['pads'], mh, mw), w, None, dil)
    lhs = float((y * dzw).sum())
    assert abs(lhs - float((w * r['dw']).sum())) <= 1e-10 * max(1.0, abs(lhs))
    assert abs(lhs - float((xt * r['dx']).sum())) <= 1e-10 * max(1.0, abs(lhs))
    # the absolute sums bound the sums
    a = np_ref.conv_layer_grads(x, w, dz, lay, absolute=True)
    assert (np.abs(r['dw']) <= a['dw'] * (1 + 1e-12)).all() and (np.abs(r['dx']) <= a['dx'] * (1 + 1e-12)).all()


@pytest.mark.parametrize('n', [1, 8, 64])
@pytest.mark.parametrize('name', ['L1', 'L2', 'L3', 'L4', 'L5', 'L6'])
def test_exactness_condition_of_family_a_at_training_size(name, n):
    """gain * A < 2^22 for the weight gradient of every generated case (A from the oracle's absolute-value sums, on the arrays the
    GPU test uploads), the data gradient's A bounded by k^2 cout max|dz| max|w| = 4 k^2 cout; over the two seeds every element of x and
    of dz is non-zero at least once"""
    L = cases.LAYERS[name]
    seen_x = seen_z = None
    for seed in (0, 1):
        x, dz, w = cases.exact_case(L, n, seed)
        assert np.array_equal(x, np.round(x)) and np.array_equal(dz, np.round(dz)) and np.array_equal(w, np.round(w))
        assert max(np.abs(x).max(), np.abs(dz).max(), np.abs(w).max()) <= 2
        a = np_ref.conv_layer_grads(x, w, dz, L['layer'], want=('dw',), absolute=True, use_torch=n >= 8)['dw']
        assert cases.exact_condition(a, L['gain']) < cases.LIMIT, (name, n, seed)
        seen_x = (x != 0) if seen_x is None else seen_x | (x != 0)
        seen_z = (dz != 0) if seen_z is None else seen_z | (dz != 0)
    assert seen_x.all() and seen_z.all()
    k = L['layer']['k']
    assert cases.GAIN_DGRAD * 4 * k * k * L['cout'] < cases.LIMIT


def test_exactness_condition_of_the_other_sizes():
    """520 samples (8 distinct ones 65 times: A is 65 times the 8 samples'), the 73 x 144 layers, 180 x 360 with 2 samples -- at the
    gain of the form the heuristic picks there (direct for the 4-channel and the 5x5 layers, Winograd for L5)"""
    for name, nd, reps, gain in [('L1', 8, 65, 1.0), ('L6', 8, 65, 1.0), ('C1a', 8, 1, 1.0), ('C1b', 8, 1, 1.0), ('L1x', 2, 1, 1.0),
                                 ('L5x', 2, 1, 64.0)]:
        L = cases.LAYERS[name]
        for seed in (0, 1):
            x, dz, w = cases.exact_case(L, nd, seed, gain * reps)
            a = np_ref.conv_layer_grads(x, w, dz, L['layer'], want=('dw',), absolute=True, use_torch=True)['dw']
            assert cases.exact_condition(a, gain * reps) < cases.LIMIT, (name, seed)


def test_pooled_first_layer_condition():
    """dlwp_conv2d_bwd_weight_pooled, family (a): terms are multiples of 1/4 -- four times the room"""
    L = cases.LAYERS['L1']
    x, _, w = cases.exact_case(L, 64, 0, 4 * cases.GAIN_WGRAD_DIRECT)
    rng = np.random.default_rng([64, 0, 99])
    y = exact_act_values(rng, (64, L['cout'], L['ho'], L['wo']))
    dp = cases._ints(rng, (64, L['cout'], L['ho'] // 2, L['wo'] // 2), 1.0)
    dz = np_ref.pool_act_bwd(y, dp, 'tanh')
    assert np.array_equal(4 * dz, np.round(4 * dz))
    a = np_ref.conv_layer_grads(x, w, dz, L['layer'], want=('dw',), absolute=True, use_torch=True)['dw']
    assert cases.exact_condition(a, 4 * cases.GAIN_WGRAD_DIRECT) < cases.LIMIT
    assert 4 * np.abs(dz).sum(axis=(0, 2, 3)).max() < cases.LIMIT


def test_reduce_slabs_restatement_two_pass_tree():
    """the chunked in-place first pass is taken for the first layer's slab count; integers come out exact, reals inside depth * u * A"""
    n_el, s = 9 * 4 * 32, 2048
    gx, cs, y = reduce_plan(n_el, s)
    assert (gx, cs, y) == (5, 21, 98)                                      # gx < 128 and S >= 64: chunked
    assert reduce_plan(9 * 64 * 128, 512)[1] == 0                          # many elements: one pass
    rng = np.random.default_rng(0)
    ints = rng.integers(-40, 41, size=(s, 64)).astype(np.float32)
    assert np.array_equal(reduce_slabs_f32(ints).astype(np.float64), ints.astype(np.float64).sum(0))
    reals = rng.standard_normal((s, 64)).astype(np.float32)
    err = np.abs(reduce_slabs_f32(reals).astype(np.float64) - reals.astype(np.float64).sum(0))
    bound = (reduce_depth(cs) + reduce_depth(y)) * U * np.abs(reals.astype(np.float64)).sum(0)
    assert (err <= bound).all()
    print('\nMEASURED reduce_slabs restatement: worst error / bound %.3f' % (err / bound).max())


def test_c4_restatement_stays_inside_the_counted_bound():
    """conv2d_wgrad_c4_f32 + reduce_slabs_kernel restated in float32 at a reduced size (2 x 4 x 16 x 40 -> 8 channels, tiles of 8 x 32
    with ragged columns): exact on family (a), inside c u A on family (b)"""
    n, cin, cout, h, w, dil, th, tw = 2, 4, 8, 16, 40, 2, 8, 32
    L = dict(cin=cin, cout=cout, hs=h, ws=w, ho=h, wo=w, layer=np_ref.conv_layer(3, dil), gain=1.0)
    tiles, splits, per = c4_launch(n, h, w, cout, th, tw, cu=4, fill=1)
    assert (tiles, splits, per) == (8, 2, 4)
    c = c4_bound_count(n, h, w, cout, th, tw, cu=4, fill=1)
    assert c == 1 + 4 * 64 + reduce_depth(8) + 1
    x, dz, wt = cases.exact_case(L, n, 0)
    ref = np_ref.conv_layer_grads(x, wt, dz, L['layer'], want=('dw',))['dw']
    got = reduce_slabs_f32(c4_wgrad_f32(x, dz, dil, th, tw, splits), cu=4).reshape(ref.shape)
    assert np.array_equal(got.astype(np.float64), ref)
    x, dz, wt = cases.real_case(L, n, 0)
    ref = np_ref.conv_layer_grads(x, wt, dz, L['layer'], want=('dw',))
    a = np_ref.conv_layer_grads(x, wt, dz, L['layer'], want=('dw',), absolute=True)['dw']
    got = reduce_slabs_f32(c4_wgrad_f32(x, dz, dil, th, tw, splits), cu=4).reshape(a.shape)
    ratio = (np.abs(got - ref['dw']) / (c * U * a)).max()
    print('\nMEASURED c4 restatement: worst error / (c u A) %.4f with c = %d' % (ratio, c))
    assert ratio <= 1.0


def test_counts_at_training_size():
    """the first layer at 64 samples: 4224 tiles over 512 splits of 9 tiles, 2048 slabs summed in chunks of 21 -> c = 593"""
    assert c4_launch(64, 88, 180, 32, 8, 32) == (4224, 512, 9)
    assert c4_bound_count(64, 88, 180, 32, 8, 32) == 1 + 9 * 64 + reduce_depth(21) + reduce_depth(98) + 1


# ------------------------------------------------------------------------------------------------------------------ #
# the pooled first layer's counts, and a Winograd weight gradient restated
# ------------------------------------------------------------------------------------------------------------------ #

def c4_pooled_counts(n, ho, wo, cout, th, tw, cu=CU, fill=4, cin=4):
    """dlwp_conv2d_bwd_weight_pooled (conv_wgrad_c4_kernel.h, FUSE): (c_dw, c_db).  dz is formed in float32 in the loader -- m * m,
    1 - m^2, g * (1 - m^2): 3 roundings on every term in front of c4_bound_count's path.  The bias gradient: a lane adds its 2 windows
    of GPW / 2 group pairs per tile (GPW = TH * TW / 64 additions per tile) over `per` tiles, 2 shuffle additions join the 4 pixel-quad
    lanes, then the slab sums of the weight gradient's launch (same S, cout elements: always chunked) and the addition to db."""
    _, splits, per = c4_launch(n, ho, wo, cout, th, tw, cu, fill)
    _, cs, y = reduce_plan(cout, 4 * splits, cu)
    red = reduce_depth(cs) + reduce_depth(y) if cs else reduce_depth(y)
    return 3 + c4_bound_count(n, ho, wo, cout, th, tw, cu, fill, cin), 3 + per * (th * tw // 64) + 2 + red + 1


BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)      # input tile, conv_wgrad_kernel.h
AZ = np.array([[1, 0], [1, 1], [1, -1], [0, -1]], np.float32)                                 # dz tile (4 x 2)
GT = np.array([[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, 1]], np.float32)                  # output (3 x 4): T[0] = u0 + (u1 + u2) / 2 ...


def wino_wgrad_f32(x, dz, splits):
    """The Winograd F(2x2, 3x3) weight gradient (conv_wgrad_kernel.h) in float32, 3x3 dilation 1, zero rows / periodic columns: per
    2 x 2 tile of dz the 4 x 4 input tile is transformed (B^T d B), the dz tile too (A z A^T), their products are accumulated tile after
    tile per split into 16 positions per channel pair, each split's sum goes through the output transform G^T M G with its two halvings
    -> one slab per split."""
    n, cin, h, w = x.shape
    cout = dz.shape[1]
    xp = np_ref.pad2d_modes(x.astype(np.float32), (1, 1, 1, 1), np_ref.PAD_ZERO, np_ref.PAD_WRAP).astype(np.float32)
    tiles = [(ni, i, j) for ni in range(n) for i in range(0, h, 2) for j in range(0, w, 2)]
    per = ceil_div(len(tiles), splits)
    slabs = np.zeros((splits, 3, 3, cin, cout), np.float32)
    for s in range(splits):
        m = np.zeros((4, 4, cin, cout), np.float32)
        for ni, i, j in tiles[s * per:(s + 1) * per]:
            d = xp[ni, :, i:i + 4, j:j + 4]
            z = dz[ni, :, i:i + 2, j:j + 2].astype(np.float32)
            v = np.einsum('ab,cbd,ed->aec', BT, d, BT).astype(np.float32)                      # (4, 4, cin): sums of +-1 terms
            t = np.einsum('ab,obd,ed->aeo', AZ, z, AZ).astype(np.float32)
            m = m + (v[:, :, :, None] * t[:, :, None, :]).astype(np.float32)
        t1 = np.stack([m[0] + np.float32(.5) * (m[1] + m[2]), np.float32(.5) * (m[1] - m[2]), np.float32(.5) * (m[1] + m[2]) + m[3]])
        slabs[s] = np.stack([t1[:, 0] + np.float32(.5) * (t1[:, 1] + t1[:, 2]), np.float32(.5) * (t1[:, 1] - t1[:, 2]),
                             np.float32(.5) * (t1[:, 1] + t1[:, 2]) + t1[:, 3]], axis=1)
    return slabs.reshape(splits, -1)


def test_winograd_weight_gradient_restatement():
    """exact on family (a) (which also shows the three matrices above are the weight gradient's), inside GRAD_BAR on family (b) -- the
    bar the GPU file applies to the Winograd forms, whose path was not counted"""
    n, cin, cout, h, w = 2, 3, 5, 12, 20
    L = dict(cin=cin, cout=cout, hs=h, ws=w, ho=h, wo=w, layer=np_ref.conv_layer(3, 1), gain=cases.GAIN_WGRAD_WINO)
    x, dz, wt = cases.exact_case(L, n, 0)
    ref = np_ref.conv_layer_grads(x, wt, dz, L['layer'], want=('dw',))['dw']
    a = np_ref.conv_layer_grads(x, wt, dz, L['layer'], want=('dw',), absolute=True)['dw']
    assert cases.exact_condition(a, L['gain']) < cases.LIMIT
    got = reduce_slabs_f32(wino_wgrad_f32(x, dz, 6)).reshape(ref.shape)
    assert np.array_equal(got.astype(np.float64), ref)
    x, dz, wt = cases.real_case(L, n, 0)
    ref = np_ref.conv_layer_grads(x, wt, dz, L['layer'], want=('dw',))['dw']
    got = reduce_slabs_f32(wino_wgrad_f32(x, dz, 6)).reshape(ref.shape)
    ratio = np.abs(got - ref).max() / (GRAD_BAR * max(1.0, np.abs(ref).max()))
    print('\nMEASURED Winograd weight-gradient restatement: worst error / GRAD_BAR %.4f' % ratio)
    assert ratio <= 1.0


def test_pooled_counts_at_training_size():
    assert c4_pooled_counts(64, 88, 180, 32, 8, 32) == (3 + c4_bound_count(64, 88, 180, 32, 8, 32), 3 + 9 * 4 + 2 + reduce_depth(2048 // 128) + reduce_depth(128) + 1)
