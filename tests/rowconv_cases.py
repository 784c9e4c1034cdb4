"""RowConnected2D (dlwp_rowconv2d_fwd, _bwd_data, _bwd_weight; csrc/rowconv.hip) on guarded slabs: the case table of
tests/test_rowconv_cases_cpu.py and tests/test_gpu_rowconv_pinned.py -- one row per kernel INSTANCE, fall-back reason and window
arrangement at the smallest geometry that reaches it --, the two input families, the float64 oracles and the exactness measure.

(a) exact: x, dz and the kernel are integers in [-A, A] (A a power of two chosen per row, amplitude()), the bias a multiple of
BIAS_UNIT.  Every product and every partial sum of every pass is then a multiple of BIAS_UNIT whose magnitude stays below
LIMIT = 2^24 units in ANY order of summation (exact_condition: the sum of the absolute values of the terms of the worst output
element, with ROOM to spare), so float32 holds all of them exactly: the matrix-core kernels (whatever their k split), the vector
kernels, the halo fold and the bias tree must return the float64 oracle's values to the bit.
(b) reals: standard-normal x and dz, glorot-uniform kernels x 3, tanh.  Forward: FWD_TOL of max(1, max |reference|); gradients:
GRAD_BAR of the tensor's largest reference magnitude (tests/test_conv_grads_cpu.py) -- the project's bars, not tuned here.

A row names the instance dlwp_rowconv2d_launch_info must report for each pass (instance_name()); the CPU test asserts that the
table reaches every compiled instance, every vector kernel and every fall-back reason.  The 32-bit-offset reason needs tensors of
2 GB and more: the host-only report is asked about those geometries (OFFSET_PROBES), no kernel is run on them."""
import functools

import numpy as np

from oracle import np_ref

LIMIT = 2.0 ** 24
ROOM = 8.0                     # the worst sum of absolute terms stays below LIMIT / ROOM units
BIAS_UNIT = 0.25
FWD_TOL = 1e-5
GRAD_BAR = 2e-5                # tests/test_conv_grads_cpu.py
PASSES = ('fwd', 'dgrad', 'wgrad')
K_MAX_SLOTS = 7                # csrc/rowconv.hip: kMaxSlots

# every instance csrc/rowconv.hip compiles, as instance_name() spells them
COMPILED = {
    'fwd': ['fwd_mfma<2,1>', 'fwd_mfma<2,2>', 'fwd_mfma<4,1>', 'fwd_mfma<4,2>', 'fwd_mfma<7,1>'],
    'dgrad': ['dgrad_mfma<1>', 'dgrad_mfma<2>'],
    'wgrad': ['wgrad_mfma<3,4>', 'wgrad_mfma<3,8>', 'wgrad_mfma<3,0>', 'wgrad_mfma<7,4>', 'wgrad_mfma<7,0>'],
}
# ... and the reasons for which each pass hands over to its vector kernel ('empty batch' of the forward and the data gradient
# launches nothing)
REASONS = {
    'fwd': ['kernel height', 'staged width', 'LDS footprint', '32-bit offsets', 'empty batch'],
    'dgrad': ['kernel height', 'staged width', 'LDS footprint', '32-bit offsets', 'empty batch'],
    'wgrad': ['staged width', 'LDS footprint', '32-bit offsets', 'empty batch'],
}
# instances the dispatch names but no geometry reaches (proved by the sweep of tests/test_rowconv_cases_cpu.py): none -- the
# forward's <kMaxSlots, 2> was one and is no longer compiled
UNREACHABLE = []


def instance_name(which, info):
    """the kernel a launch report (ops.rowconv2d_launch_info) names: 'fwd_mfma<4,1>', 'dgrad_mfma<2>', 'wgrad_simple: LDS footprint'"""
    p = PASSES[which] if isinstance(which, int) else which
    if info['kind'] == 'mfma':
        return '%s_mfma<%d>' % (p, info['targ'][0]) if p == 'dgrad' else '%s_mfma<%d,%d>' % ((p,) + tuple(info['targ']))
    return '%s_simple: %s' % (p, info['reason'])


def _row(name, n, cin, h, w, cout, k, pads, modes=(0, 0), src=0, in_win=None, out_win=None, bias=True, fwd=None, dgrad=None, wgrad=None,
         **extra):
    """h, w: the STORED input (src 1: keras UpSampling2D(2) in front, resolved by the loaders; such a row has no data gradient).
    in_win / out_win: (offset, total channels) of the window, None: the tensor is the window.  extra: further fields the report
    must show, '<pass>_<field>' (dgrad_circ, fwd_n_cg, ...)."""
    return dict(name=name, n=n, cin=cin, h=h, w=w, cout=cout, k=tuple(k), pads=tuple(pads), modes=tuple(modes), src=src,
                in_win=tuple(in_win) if in_win else (0, cin), out_win=tuple(out_win) if out_win else (0, cout), bias=bias,
                expect=dict(fwd=fwd, dgrad=dgrad, wgrad=wgrad), extra=extra)


SAME3, SAME5, NONE = (1, 1, 1, 1), (2, 2, 2, 2), (0, 0, 0, 0)

ROWS = [
    # ---- one row per instance / fall-back reason
    _row('pack4-narrow', 3, 8, 6, 30, 4, (3, 3), SAME3, fwd='fwd_mfma<2,1>', dgrad='dgrad_mfma<1>', wgrad='wgrad_mfma<3,4>'),
    _row('pack4-callsite', 2, 8, 4, 180, 4, (5, 5), SAME5, (0, 1), fwd='fwd_mfma<4,1>', dgrad='dgrad_mfma<1>', wgrad='wgrad_mfma<3,4>',
         dgrad_circ=True, dgrad_fold=False),
    _row('pack8-wide', 2, 6, 4, 300, 2, (3, 3), SAME3, fwd='fwd_mfma<7,1>', dgrad='dgrad_mfma<1>', wgrad='wgrad_mfma<7,4>'),
    _row('cout12-cin3', 2, 3, 5, 40, 12, (3, 3), SAME3, fwd='fwd_mfma<2,1>', dgrad='dgrad_mfma<1>', wgrad='wgrad_mfma<3,4>'),
    _row('cout33-cin20', 2, 20, 4, 50, 33, (3, 3), SAME3, fwd='fwd_mfma<2,2>', dgrad='dgrad_simple: LDS footprint',
         wgrad='wgrad_mfma<3,8>', fwd_n_cg=3, wgrad_n_cg=3),
    _row('wide-cin40', 1, 40, 3, 250, 5, (3, 3), SAME3, fwd='fwd_mfma<4,2>', dgrad='dgrad_mfma<2>', wgrad='wgrad_mfma<7,0>', fwd_n_cb=2),
    _row('wide-cin24', 1, 24, 3, 250, 5, (3, 3), SAME3, fwd='fwd_mfma<4,2>', dgrad='dgrad_mfma<2>', wgrad='wgrad_mfma<7,0>'),
    _row('deep-cin256', 1, 256, 3, 96, 2, (3, 3), SAME3, fwd='fwd_mfma<4,2>', dgrad='dgrad_mfma<2>', wgrad='wgrad_simple: LDS footprint'),
    _row('too-wide', 1, 2, 3, 460, 1, (3, 3), SAME3, fwd='fwd_simple: staged width', dgrad='dgrad_mfma<1>',
         wgrad='wgrad_simple: staged width'),
    _row('tall-kernel', 2, 5, 8, 20, 3, (6, 3), (0, 0, 1, 1), fwd='fwd_simple: kernel height', dgrad='dgrad_simple: kernel height',
         wgrad='wgrad_mfma<3,4>'),
    _row('cin64-k5x7', 1, 64, 5, 100, 40, (5, 7), NONE, fwd='fwd_mfma<2,2>', dgrad='dgrad_simple: LDS footprint',
         wgrad='wgrad_mfma<3,0>', wgrad_n_mg=3, wgrad_n_cg=3),
    # a 64-column kernel: the forward's filters alone overflow the LDS budget, the data gradient's staged dz row its two slots
    _row('kw64', 1, 1, 5, 70, 16, (5, 64), NONE, fwd='fwd_simple: LDS footprint', dgrad='dgrad_simple: staged width',
         wgrad='wgrad_mfma<3,4>', wgrad_n_mg=6),
    # ---- loaders, halos, batches
    _row('upsampled-6x23', 2, 8, 6, 23, 4, (3, 3), SAME3, (0, 1), src=1, fwd='fwd_mfma<2,1>', wgrad='wgrad_mfma<3,4>'),
    _row('fold-mirror-edge', 2, 5, 7, 19, 3, (3, 5), (2, 0, 1, 3), (3, 2), fwd='fwd_mfma<2,1>', dgrad='dgrad_mfma<1>',
         wgrad='wgrad_mfma<3,4>', dgrad_fold=True, dgrad_circ=False),
    _row('fold-symmetric-wrap', 3, 6, 5, 21, 9, (2, 4), (0, 1, 3, 0), (4, 1), bias=False, fwd='fwd_mfma<2,1>', dgrad='dgrad_mfma<1>',
         wgrad='wgrad_mfma<3,4>', dgrad_fold=True, dgrad_circ=False),
    _row('batch5-groups', 5, 4, 5, 17, 3, (3, 3), SAME3, (1, 1), fwd='fwd_mfma<2,1>', dgrad='dgrad_mfma<1>', wgrad='wgrad_mfma<3,4>',
         fwd_samples=2, fwd_n_sg=3, dgrad_samples=3, dgrad_n_sg=2),
    # ---- channel windows on both sides, with channels stored in front of and behind each window
    _row('win-pack4-circ', 2, 8, 5, 22, 4, (3, 3), SAME3, (0, 1), in_win=(3, 14), out_win=(2, 9), fwd='fwd_mfma<2,1>',
         dgrad='dgrad_mfma<1>', wgrad='wgrad_mfma<3,4>', dgrad_circ=True),
    _row('win-cout20-cin20', 3, 20, 4, 37, 20, (3, 3), SAME3, (2, 0), in_win=(5, 27), out_win=(1, 24), fwd='fwd_mfma<2,1>',
         dgrad='dgrad_mfma<2>', wgrad='wgrad_mfma<3,8>', fwd_n_cg=2, wgrad_n_cg=2),
    _row('win-tall-kernel', 2, 5, 8, 20, 3, (6, 3), (0, 0, 1, 1), in_win=(2, 9), out_win=(3, 7), fwd='fwd_simple: kernel height',
         dgrad='dgrad_simple: kernel height', wgrad='wgrad_mfma<3,4>'),
    _row('win-too-wide', 1, 2, 2, 460, 1, (2, 3), (1, 0, 1, 1), in_win=(1, 4), out_win=(2, 4), fwd='fwd_simple: staged width',
         dgrad='dgrad_mfma<1>', wgrad='wgrad_simple: staged width'),
    _row('win-wide-cin40', 1, 40, 2, 200, 5, (2, 3), (0, 1, 1, 1), in_win=(2, 43), out_win=(1, 7), fwd='fwd_mfma<4,2>',
         dgrad='dgrad_mfma<2>', wgrad='wgrad_mfma<7,0>'),
]

# geometries past the 32-bit descriptor offsets of each pass (report only: 2 GB tensors): (pass, xs, cout, (kh, kw), pads)
OFFSET_PROBES = [
    ('fwd', (1, 1000, 500, 500), 16, (3, 3), SAME3),         # two samples' channel windows: 1000 x 500 x 500 x 8 bytes
    ('dgrad', (3, 8, 7000, 24), 1000, (3, 3), SAME3),        # a sample group of dz: 3 x 1000 x 7000 x 24 x 4 bytes
    ('wgrad', (1, 1000, 1250, 400), 4, (3, 3), SAME3),       # one sample's channel window: 1000 x 1250 x 400 x 4 bytes
]


def row_named(name):
    return [r for r in ROWS if r['name'] == name][0]


def geometry(row):
    """(H, W) as the layer sees the input, (Hp, Wp) behind the halo, (Ho, Wo)"""
    kh, kw = row['k']
    t, b, l, r = row['pads']
    H, W = row['h'] << row['src'], row['w'] << row['src']
    Hp, Wp = H + t + b, W + l + r
    return (H, W), (Hp, Wp), (Hp - kh + 1, Wp - kw + 1)


def descriptor(ops, row, act='linear', n=None):
    """(the dlwp_conv2d of the row, the shape (n, cin, h, w) of its input window)"""
    t, b, l, r = row['pads']
    acts = {'linear': ops.ACT_LINEAR, 'tanh': ops.ACT_TANH, 'relu': ops.ACT_RELU}
    cd = ops.make_conv(row['cout'], row['k'][0], row['k'][1], 1, ops.make_pad(t, b, l, r, row['modes'][0], row['modes'][1]), acts[act],
                       in_c_off=row['in_win'][0], in_c_total=row['in_win'][1], out_c_off=row['out_win'][0],
                       out_c_total=row['out_win'][1], src_mode=ops.SRC_UPSAMPLE2 if row['src'] else ops.SRC_DIRECT)
    return cd, (row['n'] if n is None else n, row['cin'], row['h'], row['w'])


def reports(ops, row, n=None):
    """{pass: launch report} of the passes the row has"""
    cd, xs = descriptor(ops, row, n=n)
    return {p: ops.rowconv2d_launch_info(xs, cd, i) for i, p in enumerate(PASSES) if row['expect'][p] is not None}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------- #

def amplitude(row):
    """family (a): the largest power of two A <= 16 whose worst-case sums A^2 x (terms of an output element; the halo fold of the data
    gradient counted with its multiplicity) x (1 / BIAS_UNIT) leave ROOM below LIMIT.  An upper bound from the shape alone;
    exact_condition() measures the inputs actually drawn."""
    kh, kw = row['k']
    t, b, l, r = row['pads']
    (_, _), (_, _), (ho, wo) = geometry(row)
    fold = (1 + t + b) * (1 + l + r)
    terms = max(kh * kw * row['cin'] + 1, kh * kw * row['cout'] * fold, row['n'] * wo)
    a = 16
    while a > 1 and a * a * terms / BIAS_UNIT * ROOM > LIMIT:
        a //= 2
    return a


def _ints(rng, shape, a):
    return rng.integers(-a, a + 1, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(name, family):
    row = row_named(name)
    import zlib
    rng = np.random.default_rng(zlib.crc32(('%s/%s' % (name, family)).encode()))
    kh, kw = row['k']
    (_, _), (_, _), (ho, wo) = geometry(row)
    xshape = (row['n'], row['in_win'][1], row['h'], row['w'])
    zshape = (row['n'], row['out_win'][1], ho, wo)
    kshape = (ho, kh, kw, row['cin'], row['cout'])
    if family == 'exact':
        a = amplitude(row)
        x, dz, k = _ints(rng, xshape, a), _ints(rng, zshape, a), _ints(rng, kshape, a)
        bias = (_ints(rng, (ho, 1, row['cout']), 4 * a) * BIAS_UNIT).astype(np.float32)
        dw0 = _ints(rng, kshape, 64)                       # what an accumulating weight gradient starts from
        db0 = _ints(rng, (ho, 1, row['cout']), 64)
    else:
        x = rng.standard_normal(xshape).astype(np.float32)
        dz = rng.standard_normal(zshape).astype(np.float32)
        k, bias = np_ref.init_row_connected_weights(ho, (kh, kw), row['cin'], row['cout'], rng, bias_scale=0.5)
        k = (k * 3).astype(np.float32)
        dw0 = rng.standard_normal(kshape).astype(np.float32)
        db0 = rng.standard_normal((ho, 1, row['cout'])).astype(np.float32)
    out = dict(x=x, dz=dz, k=k, bias=bias if row['bias'] else None, dw0=dw0, db0=db0)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def inputs(row, family):
    """family 'exact' | 'real' -> dict(x (n, in_c_total, h, w) STORED, every channel finite; dz (n, out_c_total, ho, wo); k; bias or
    None; dw0, db0: the content an accumulating weight gradient starts from).  Read-only, shared."""
    return _inputs(row['name'], family)


# ---- oracles ------------------------------------------------------------------------------------------------------------------------ #

def window(a, win, c):
    """channels [off, off + c) of a stored tensor (win = (off, total))"""
    return a[:, win[0]:win[0] + c]


def padded_input(row, x):
    """the float64 tensor the 'valid' row convolution reads: window, up-sampling, halo"""
    xw = np.asarray(window(x, row['in_win'], row['cin']), np.float64)
    if row['src']:
        xw = np_ref.upsample2(xw)
    return np_ref.pad2d_modes(xw, row['pads'], row['modes'][0], row['modes'][1])


def forward_oracle(row, x, k, bias, act='linear'):
    """(n, cout, ho, wo) float64: the output WINDOW"""
    return np_ref.row_connected2d(padded_input(row, x), k, bias, act)


def grads_oracle(row, x, k, dz):
    """-> dx (n, cin, h, w) dense (None for an up-sampled source), dw, db (ho, 1, cout), float64"""
    dzw = np.asarray(window(dz, row['out_win'], row['cout']), np.float64)
    dxp, dw, db = np_ref.row_connected2d_grads(padded_input(row, x), k, dzw)
    dx = None
    if not row['src']:
        dx = np_ref.pad2d_modes_grad(dxp, (row['n'], row['cin'], row['h'], row['w']), row['pads'], row['modes'][0], row['modes'][1])
    return dx, dw, db


@functools.lru_cache(maxsize=None)
def _reference(name, family, act):
    row = row_named(name)
    d = inputs(row, family)
    y = forward_oracle(row, d['x'], d['k'], d['bias'], act)
    out = dict(y=y)
    if act == 'linear' or family == 'real':
        out['dx'], out['dw'], out['db'] = grads_oracle(row, d['x'], d['k'], d['dz'])
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def reference(row, family, act='linear'):
    """the float64 results on inputs(row, family), computed once and shared (read-only): y (activation `act`), dx, dw, db"""
    return _reference(row['name'], family, act)


def exact_condition(row, d=None):
    """family (a): {pass: the largest sum of |terms| of one output element, in units of BIAS_UNIT}, measured on the absolute values of
    the inputs (the accumulating weight gradient's starting content included).  Each must stay below LIMIT / ROOM."""
    d = d or inputs(row, 'exact')
    ab = {k: (None if v is None else np.abs(v)) for k, v in d.items()}
    y = forward_oracle(row, ab['x'], ab['k'], ab['bias'])
    dx, dw, db = grads_oracle(row, ab['x'], ab['k'], ab['dz'])
    cond = dict(fwd=y.max(), wgrad=max((dw + ab['dw0']).max(), (db + ab['db0']).max()))
    if dx is not None:
        cond['dgrad'] = dx.max()
    return {p: float(v) / BIAS_UNIT for p, v in cond.items()}
