"""The forward convolutions (dlwp_conv2d_fwd, _fwd_direct, _fwd_prepared, _fwd_pool2) on guarded slabs: the case table of
tests/test_conv_fwd_cpu.py and tests/test_gpu_conv_fwd.py -- one row per forward ROUTE at the smallest geometry that reaches it --,
the two input families, the float64 reference, the exactness measure and the poison patterns.

(a) exact: x from {-2, -1, 1, 2}, small non-zero integer weights and biases.  Every product, every Winograd transform (whose only
non-integer constants are the filter transform's 1/2, twice) and every partial sum is a multiple of 1/4 below 2^22 as long as
GAIN_FWD * A < LIMIT, A the absolute-value sum of an output element: float32 holds all of them exactly, in any summation order, so
EVERY family -- direct tiles, packed-N, all Winograd forms (the 9-position up-sampled form and the few-channel kernel's in-kernel
filter transform included), split-K, the bf16 matrix cores (these integers are exact in bfloat16), the pooled epilogues -- must
return the float64 sums to the bit.
(b) reals: standard-normal x, glorot-uniform kernels, tanh: FWD_TOL of max(1, max |reference|), the project's bar.

A row names the route dlwp_conv2d_launch_info must report: a negative route code of the library, or the FAMILY of the reported
registry index (family_of); rows with `force` run every compiled configuration of one family through DLWP_OPT_FORCE_CONV_CONFIG and
must then see exactly the forced index.  Every row runs on a batch of 3."""
import zlib

import numpy as np

from oracle import np_ref
from tests.sconv_cases import map_coord, pad_fits

LIMIT = 2.0 ** 22
# filter G g G^T: absolute row sums 3/2 per axis = 9/4; input B^T d B: 2 per axis = 4; output A^T m A: 3 per axis = 9
# (oracle/conv_grad_cases.py: GAIN_DGRAD, the same kernels).  The direct families gain 1; one bound serves all.
GAIN_FWD = 81.0
FWD_TOL = 1e-5
N = 3
EXTRA = 3                      # foreign channels on each side of a window (p3 / p4); 8 where the storage is in channel octets
R_VECTOR, R_FEW_STREAM, R_FLAT, R_FEW_WINO = -1, -2, -4, -5          # include/dlwp_hip.h: dlwp_launch_info.config
DENSE_VALUES = np.array([-2., -1., 1., 2.], dtype=np.float32)


def family_of(c):
    """the family of a compiled configuration (ops.conv_configs() entry)"""
    ks, dil, th, tw, waves, fa, bnf, ck, pool, lds, flags = c
    if flags & 2:
        return 'cell-update'
    if pool >= 2:
        return 'octet' if flags & 24 else 'bf16'
    if pool == 1:
        return 'pooled-loader'
    if bnf < 0:
        return 'packed-n'
    if fa == 0:
        return 'wino-split' if (flags & 5) == 1 else 'wino'
    return 'direct'


def _row(name, cin, h, w, cout, k=3, dil=1, pads=None, mh=0, mw=1, src=0, pools='auto', d2s=False, route=None, opts=None,
         force=None, storage=('f32', 'f32'), compute_bf16=False, entries=('fwd', 'prepared'), split=None, loader=None):
    p = dil * (k - 1) // 2
    return dict(name=name, cin=cin, h=h, w=w, cout=cout, k=k, dil=dil, pads=tuple(pads) if pads else (p, p, p, p), mh=mh, mw=mw,
                src=src, pools=pools, d2s=d2s, route=route, opts=dict(opts or {}), force=force, storage=storage,
                compute_bf16=compute_bf16, entries=tuple(entries), split=split, loader=loader)


def _forced_rows():
    rows = []
    for k, dil in ((3, 1), (3, 2), (5, 1)):
        tag = 'k%dd%d' % (k, dil)
        rows.append(_row('tiles-direct-' + tag, 20, 19, 50, 36, k, dil, force=dict(family='direct', k=k, dil=dil)))
        rows.append(_row('tiles-pooled-loader-' + tag, 20, 39, 101, 36, k, dil, src=2, force=dict(family='pooled-loader', k=k, dil=dil)))
    for k, dil, cmax in ((3, 1, 4), (3, 1, 8), (3, 2, 4), (3, 2, 8), (5, 1, 2), (5, 1, 4), (5, 1, 8)):
        rows.append(_row('tiles-packed-n-k%dd%d-c%d' % (k, dil, cmax), 20, 19, 50, cmax - 1, k, dil,
                         force=dict(family='packed-n', k=k, dil=dil, cmax=cmax)))
    for dil in (1, 2):
        rows.append(_row('tiles-wino-k3d%d' % dil, 24, 19, 50, 64, 3, dil, force=dict(family='wino', k=3, dil=dil)))
    rows.append(_row('tiles-wino-split-k3d1', 24, 19, 50, 48, 3, 1, force=dict(family='wino-split', k=3, dil=1)))
    # the 64-channel Winograd blocks exist for the 9-position (up-sampled) form only
    rows.append(_row('tiles-wino-up-k3d1', 24, 10, 25, 64, 3, 1, src=1, force=dict(family='wino', k=3, dil=1)))
    # the bf16 matrix-core instances: bfloat16-stored input, or (in32) a float32 input rounded by the loader
    for k, dil in ((3, 1), (3, 2), (5, 1)):
        tag = 'k%dd%d' % (k, dil)
        rows.append(_row('bf16-' + tag, 52, 19, 50, 36, k, dil, storage=('bf16', 'f32'),
                         force=dict(family='bf16', k=k, dil=dil, in32=False, ck8=False)))
        rows.append(_row('bf16-in32-' + tag, 52, 19, 50, 36, k, dil, compute_bf16=True,
                         force=dict(family='bf16', k=k, dil=dil, in32=True, ck8=False)))
    for dil in (1, 2):
        rows.append(_row('bf16-in32-taps-k3d%d' % dil, 6, 19, 50, 36, 3, dil, compute_bf16=True,
                         force=dict(family='bf16', k=3, dil=dil, in32=True, ck8=True)))
        # octet storage: the forced instance fixes the layout of x (flag bit 3) and of the output (bit 4)
        rows.append(_row('octet-k3d%d' % dil, 56, 19, 50, 40, 3, dil, storage=('bf16', 'f32'),
                         force=dict(family='octet', k=3, dil=dil, in32=False)))
        rows.append(_row('octet-in32-k3d%d' % dil, 8, 19, 50, 40, 3, dil, compute_bf16=True,
                         force=dict(family='octet', k=3, dil=dil, in32=True)))
    return rows


def _xloader_rows():
    tile = dict(family='wino', k=3, dil=1, tile=(8, 32, 4))
    rows = []
    for mask in (0, 7):
        rows.append(_row('xloader%d-odd-12x45' % mask, 16, 12, 45, 32, opts=dict(wino_xloader=mask), force=tile,
                         loader=0 if mask == 0 else None))
        rows.append(_row('xloader%d-up-11x23' % mask, 16, 11, 23, 64, src=1, opts=dict(wino_xloader=mask), force=tile,
                         loader=0 if mask == 0 else None))
    # the two-output launch (dlwp_conv2d_fwd_pool2) of that instance where the pooled map's right edge cuts a 16-byte quad after 2 and
    # after 3 columns (pooled widths 22 and 23; the 12 x 45 rows above: 22 as well, 19 x 50 of the tile rows: after 1)
    for w in (44, 46):
        rows.append(_row('pool2-wino-12x%d' % w, 16, 12, w, 32, force=tile, pools=(False,), entries=('fwd', 'prepared', 'pool2')))
    return rows


def _heuristic_rows():
    rows = [
        # (flat runs stand in for the 8 x 32 rectangles only: a plain source of 3 samples gets those from half a workgroup per CU
        #  on -- 2 x 4 tiles x 11 channel tiles x 3 >= 256 --, below that the position-split instances run, with or without the option)
        _row('flat-9x33', 16, 9, 33, 352, mh=1, mw=0, route=R_FLAT, opts=dict(wino_flat=2), pools=(False,)),
        _row('flat-up-9x33', 16, 9, 33, 64, src=1, mh=0, mw=2, route=R_FLAT, opts=dict(wino_flat=2), pools=(False,)),
        _row('few-stream-d1-pooled', 4, 20, 52, 32, dil=1, route=R_FEW_STREAM, opts=dict(few_stream=2), pools=(True,)),
        _row('few-stream-d2-pooled', 4, 20, 52, 32, dil=2, route=R_FEW_STREAM, opts=dict(few_stream=2), pools=(True,)),
        _row('few-stream-6ch-pooled', 6, 20, 52, 32, dil=2, route=R_FEW_STREAM, opts=dict(few_stream=2), pools=(True,)),
        _row('few-stream-d1-plain', 4, 20, 52, 32, dil=1, route=R_FEW_STREAM, opts=dict(few_stream=2), pools=(False,),
             entries=('fwd', 'prepared', 'pool2')),
        _row('few-stream-d2-plain', 4, 20, 52, 32, dil=2, route=R_FEW_STREAM, opts=dict(few_stream=2), pools=(False,),
             entries=('fwd', 'prepared', 'pool2')),
        _row('few-wino-4ch', 4, 20, 52, 32, dil=2, route=R_FEW_WINO, opts=dict(few_wino=1), pools=(True,)),
        _row('few-wino-3ch', 3, 18, 76, 64, dil=2, route=R_FEW_WINO, opts=dict(few_wino=1), pools=(True,)),
        # (a plain source of 3 samples runs on the position-split instances, which have no split-K variant: the up-sampled form)
        _row('splitk-up-32x11x23', 32, 11, 23, 64, src=1, route='wino', opts=dict(splitk=2), split=2),
        _row('d2s-24to16', 24, 20, 70, 16, d2s=True, route='wino-split', pools=(False,)),
        # the one-thread-per-output vector kernel (dlwp_conv2d_fwd_direct): any kernel size, halo and source
        _row('vector-asym-d2', 5, 9, 11, 7, dil=2, pads=(2, 1, 3, 2), mh=2, mw=1, route=R_VECTOR, pools=(False,), entries=('direct',)),
        _row('vector-pooled-source', 8, 12, 20, 16, src=2, mh=3, mw=1, route=R_VECTOR, pools=(False,), entries=('direct',)),
        _row('vector-up-k5', 6, 6, 10, 8, k=5, src=1, mh=4, mw=3, route=R_VECTOR, pools=(False,), entries=('direct',)),
        # bfloat16 storage on the fp32 families (DLWP_OPT_BF16_MFMA off)
        _row('bf16-storage-direct', 20, 19, 50, 36, route='direct', opts=dict(bf16_mfma=0), storage=('bf16', 'bf16')),
        _row('bf16-storage-wino', 24, 19, 50, 64, route='wino', opts=dict(bf16_mfma=0), storage=('bf16', 'bf16')),
    ]
    # ragged input-channel counts on Winograd: planes past Cin are read through the descriptor's range check.  5 channels of a
    # plain source belong to the direct family.
    for cin in (5, 13, 22):
        for dil, src in ((1, 0), (2, 0), (1, 1)):
            fam = 'direct' if (cin <= 8 and src == 0) else 'wino'
            rows.append(_row('ragged-c%d-d%d-s%d' % (cin, dil, src), cin, 12, 20, 64, dil=dil, src=src, route=fam))
    return rows


ROWS = _forced_rows() + _xloader_rows() + _heuristic_rows()
BY_NAME = {r['name']: r for r in ROWS}

# the two ConvLSTM2D pins: (filters, (h, w), first step?) at the smallest shapes of tests/test_gpu_kernels.py:
# test_convlstm_cell_update_in_the_convolution_epilogue, and (filters, state channels, h, w) of tests/test_gpu_bf16_octets.py:
# test_whole_convlstm_step_in_one_launch_equals_the_two_launch_step
LSTM_CONV_ROWS = [(16, (16, 24), False), (24, (20, 72), True)]
LSTM_STEP_ROWS = [(16, 4, 18, 36)]


def forced_configs(row, cfgs):
    """registry indices a row with `force` runs (cfgs: ops.conv_configs())"""
    f = row['force']
    out = []
    for i, c in enumerate(cfgs):
        ks, dil, th, tw, waves, fa, bnf, ck, pool, lds, flags = c
        if family_of(c) != f['family'] or (ks, dil) != (f['k'], f['dil']):
            continue
        if 'cmax' in f and 16 // (-bnf) != f['cmax']:
            continue
        if 'in32' in f and (pool == 3) != f['in32']:
            continue
        if 'ck8' in f and (ck == 8) != f['ck8']:
            continue
        if 'tile' in f and ((th, tw, waves) != f['tile'] or ck != 8 or bnf != (4 if row['src'] == 1 and row['cout'] % 64 == 0 else 2)):
            continue
        if f['family'] == 'wino' and 'tile' not in f and (bnf == 4) != (row['src'] == 1):
            continue
        out.append(i)
    return out


def storage_of(row, c=None):
    """(input, output) storage of a launch: 'f32', 'bf16' or 'o8'; a forced octet instance fixes both"""
    sin, sout = row['storage']
    if c is not None and family_of(c) == 'octet':
        sin = 'o8' if c[10] & 8 else sin
        sout = 'o8' if c[10] & 16 else sout
    return sin, sout


def extra_of(row, c=None):
    return 8 if 'o8' in storage_of(row, c) or (row['force'] or {}).get('family') == 'octet' else EXTRA


def out_shape(row, pool, n=N):
    """(channels, height, width) of the output WINDOW"""
    hs, ws = {0: (row['h'], row['w']), 1: (2 * row['h'], 2 * row['w']), 2: (row['h'] // 2, row['w'] // 2)}[row['src']]
    t, b, l, r = row['pads']
    span = row['dil'] * (row['k'] - 1)
    ho, wo = hs + t + b - span, ws + l + r - span
    if pool:
        ho, wo = ho // 2, wo // 2
    if row['d2s']:
        return row['cout'] // 4, 2 * ho, 2 * wo
    return row['cout'], ho, wo


def _rng(row, *key):
    return np.random.default_rng([zlib.crc32(row['name'].encode())] + [int(k) for k in key])


def exact_inputs(row, seed=0, n=N):
    """family (a): no zero anywhere"""
    rng = _rng(row, seed, 1)
    k = row['k']
    x = DENSE_VALUES[rng.integers(0, 4, size=(n, row['cin'], row['h'], row['w']))]
    w = DENSE_VALUES[rng.integers(0, 4, size=(k, k, row['cin'], row['cout']))]
    b = np.array([-3., -2., -1., 1., 2., 3.], dtype=np.float32)[rng.integers(0, 6, size=row['cout'])]
    return x.astype(np.float32), w.astype(np.float32), b


def real_inputs(row, seed=0, n=N):
    """family (b); rows of the bf16 matrix cores multiply bfloat16-rounded operands: their inputs are rounded here, once"""
    rng = _rng(row, seed, 2)
    k = row['k']
    x = rng.standard_normal((n, row['cin'], row['h'], row['w'])).astype(np.float32)
    w = np.asarray(np_ref.glorot_uniform((k, k, row['cin'], row['cout']), rng), np.float32)
    b = (0.1 * rng.standard_normal(row['cout'])).astype(np.float32)
    if rounds_operands(row):
        x = np_ref.round_bf16(x).astype(np.float32)
    return x, w, b


def rounds_operands(row):
    return row['storage'][0] != 'f32' or row['compute_bf16']


def multiplied_weights(row, w):
    """the weights as the row's family multiplies them: rounded to bfloat16 on the bf16 matrix cores"""
    on16 = rounds_operands(row) and row['opts'].get('bf16_mfma', 1) != 0
    return np_ref.round_bf16(w) if on16 else np.asarray(w, np.float64)


def source(row, x):
    x = np.asarray(x, np.float64)
    if row['src'] == 1:
        return np_ref.upsample2(x)
    if row['src'] == 2:
        return np_ref.maxpool2(x)
    return x


def reference(row, x, w, b, act, pool):
    """float64, NaN propagating as numpy does: [max-pool | up-sample] -> halo -> valid cross-correlation + bias -> activation
    [-> max-pool] [-> depth to space]"""
    xp = np_ref.pad2d_modes(source(row, x), row['pads'], row['mh'], row['mw'])
    y = np_ref.conv2d(xp, w, b, row['dil'], act)
    if pool:
        y = np_ref.maxpool2(y)
    if row['d2s']:
        y = np_ref.depth_to_space2(y, row['cout'] // 4)
    return y


def exact_measure(row, x, w, b):
    """GAIN_FWD * the largest absolute-value sum of an output element, on these very arrays: below LIMIT every intermediate of every
    family is a multiple of 1/4 that float32 holds exactly"""
    xp = np_ref.pad2d_modes(np.abs(source(row, x)), row['pads'], row['mh'], row['mw'])
    a = np_ref.conv2d(xp, np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(b, np.float64)), row['dil'], 'linear')
    return GAIN_FWD * float(a.max())


# ---- poison patterns: ordinary NaN inside tensors the kernels are entitled to read -------------------------------------------- #

def poison_p1(x):
    """sample 1 of 3 entirely NaN"""
    x = np.array(x, np.float32)
    x[1] = np.nan
    return x


def p2_pixels(row):
    """(channel, [(row, column)]): a corner and an interior pixel of the STORED plane"""
    return min(1, row['cin'] - 1), [(0, 0), (row['h'] // 2 + 1, row['w'] // 2 + 1)]


def poison_p2(row, x):
    """one NaN at a corner pixel and one at an interior pixel of sample 1, in one channel"""
    x = np.array(x, np.float32)
    c, pix = p2_pixels(row)
    for i, j in pix:
        x[1, c, i, j] = np.nan
    return x


def store_wide(x, extra, fill):
    """(p3) the window inside a tensor with `extra` more channels on each side, those filled with `fill` (NaN, or finite numbers)"""
    n, c, h, w = x.shape
    wide = np.empty((n, c + 2 * extra, h, w), np.float32)
    wide[:] = fill
    wide[:, extra:extra + c] = x
    return wide


def footprint(row, pool):
    """(p2): the output pixels (of one plane of sample 1, before depth-to-space) whose receptive field holds a poisoned pixel, from
    the index maps alone: halo (dlwp_map_coord), source transform, taps, pooled epilogue"""
    hs, ws = {0: (row['h'], row['w']), 1: (2 * row['h'], 2 * row['w']), 2: (row['h'] // 2, row['w'] // 2)}[row['src']]
    bad = np.zeros((hs, ws), bool)
    for i, j in p2_pixels(row)[1]:
        if row['src'] == 1:
            bad[2 * i:2 * i + 2, 2 * j:2 * j + 2] = True
        elif row['src'] == 2:
            if i // 2 < hs and j // 2 < ws:
                bad[i // 2, j // 2] = True
        else:
            bad[i, j] = True
    t, b, l, r = row['pads']
    span = row['dil'] * (row['k'] - 1)
    ho, wo = hs + t + b - span, ws + l + r - span
    out = np.zeros((ho, wo), bool)
    for oi in range(ho):
        rs = [map_coord(oi + u * row['dil'] - t, hs, row['mh']) for u in range(row['k'])]
        for oj in range(wo):
            cs = [map_coord(oj + v * row['dil'] - l, ws, row['mw']) for v in range(row['k'])]
            out[oi, oj] = any(a >= 0 and c >= 0 and bad[a, c] for a in rs for c in cs)
    if pool:
        out = out[:ho // 2 * 2, :wo // 2 * 2].reshape(ho // 2, 2, wo // 2, 2).any(axis=(1, 3))
    return out


def halos_fit(row):
    hs, ws = {0: (row['h'], row['w']), 1: (2 * row['h'], 2 * row['w']), 2: (row['h'] // 2, row['w'] // 2)}[row['src']]
    t, b, l, r = row['pads']
    return pad_fits(t, b, hs, row['mh']) and pad_fits(l, r, ws, row['mw'])
