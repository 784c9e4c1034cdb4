"""Conv2D(strides=2), restated in numpy the way csrc/sconv.hip runs it -- the weight map, the padded space-to-depth pass and its
adjoint, one stride-1 'valid' cross-correlation on the 4 cin phase channels -- and the float64 torch reference.  Every helper
returns the dtype it was given (float64 in: float64 arithmetic)."""
import numpy as np

PADDINGS = ('valid', 'same')
KERNELS = [(kh, kw) for kh in range(1, 6) for kw in range(1, 6)]
MAPS = ((5, 5), (6, 7), (7, 6), (9, 12))
ZERO, WRAP, EDGE, REFLECT, SYMMETRIC = 0, 1, 2, 3, 4          # DLWP_PAD_* (include/dlwp_hip.h)
MODES = (ZERO, WRAP, EDGE, REFLECT, SYMMETRIC)
NP_MODE = {ZERO: 'constant', WRAP: 'wrap', EDGE: 'edge', REFLECT: 'reflect', SYMMETRIC: 'symmetric'}


def geometry(k, padding, n):
    """(T, pad_lo, pad_hi, out) of one axis: TensorFlow's rule for stride 2 (ValueError where a 'valid' kernel does not fit)"""
    if padding == 'same':
        out = -(-n // 2)
        tot = max((out - 1) * 2 + k - n, 0)
        return (k + 1) // 2, tot // 2, tot - tot // 2, out
    if n < k:
        raise ValueError('a valid kernel of %d does not fit an axis of %d' % (k, n))
    return (k + 1) // 2, 0, 0, (n - k) // 2 + 1


def stored_taps(th, tw):
    """the taps the planner stores the derived kernel with (plan.tconv_taps): 3 x 3, 5 x 5, or T itself beyond"""
    t = max(th, tw)
    return (th, tw) if t > 5 else ((3, 3) if t <= 3 else (5, 5))


def pad_fits(lo, hi, n, mode):
    """halo amounts a mode can serve on an axis of n (dlwp_pad_fits)"""
    m = max(lo, hi)
    if mode in (WRAP, SYMMETRIC):
        return m <= n
    if mode == REFLECT:
        return m <= n - 1
    return True


def map_coord(p, n, mode):
    """source coordinate of padded coordinate p - lo, or -1 for 'zero' (dlwp_map_coord)"""
    if 0 <= p < n:
        return p
    if mode == ZERO:
        return -1
    if mode == EDGE:
        return 0 if p < 0 else n - 1
    if mode == REFLECT:
        return -p if p < 0 else 2 * n - 2 - p
    if mode == SYMMETRIC:
        return -p - 1 if p < 0 else 2 * n - 1 - p
    return p % n


def weight_map(K, taps=None):
    """K (kh, kw, cin, F) -> w2 (sh, sw, 4 cin, F), w2[ti][tj][(2a+b) cin + c][o] = K[2ti+a][2tj+b][c][o], zeros elsewhere"""
    kh, kw, cin, f = K.shape
    th, tw = (kh + 1) // 2, (kw + 1) // 2
    sh, sw = taps if taps is not None else (th, tw)
    assert sh >= th and sw >= tw
    w2 = np.zeros((sh, sw, 4 * cin, f), dtype=K.dtype)
    for u in range(kh):
        for v in range(kw):
            ph = 2 * (u & 1) + (v & 1)
            w2[u >> 1, v >> 1, ph * cin:(ph + 1) * cin] = K[u, v]
    return w2


def weight_map_bwd(dw2, kshape):
    """the gather dK[u][v][c][o] = dw2[u >> 1][v >> 1][(2(u&1) + (v&1)) cin + c][o]"""
    kh, kw, cin, f = kshape
    dk = np.zeros(kshape, dtype=dw2.dtype)
    for u in range(kh):
        for v in range(kw):
            ph = 2 * (u & 1) + (v & 1)
            dk[u, v] = dw2[u >> 1, v >> 1, ph * cin:(ph + 1) * cin]
    return dk


def _axis_index(n, lo, hi, mode, length):
    """[a][i] -> source coordinate of padded coordinate 2i + a, n (the appended zero) where it is zero / beyond the padded image"""
    idx = np.full((2, length), n, dtype=np.int64)
    for a in (0, 1):
        for i in range(length):
            p = 2 * i + a
            if p < n + lo + hi:
                m = map_coord(p - lo, n, mode)
                idx[a, i] = n if m < 0 else m
    return idx


def s2d_pad(x, pad, modes, hp, wp):
    """x (n, c, H, W) under the halo pad = (top, bottom, left, right), modes = (mode_h, mode_w) -> P (n, 4c, hp, wp) phase-major,
    +0 beyond the padded image"""
    n, c, hh, ww = x.shape
    t, b, l, r = pad
    assert pad_fits(t, b, hh, modes[0]) and pad_fits(l, r, ww, modes[1])
    xz = np.zeros((n, c, hh + 1, ww + 1), dtype=x.dtype)
    xz[:, :, :hh, :ww] = x
    ri, si = _axis_index(hh, t, b, modes[0], hp), _axis_index(ww, l, r, modes[1], wp)
    out = np.empty((n, 4 * c, hp, wp), dtype=x.dtype)
    for a in (0, 1):
        for bb in (0, 1):
            ph = 2 * a + bb
            out[:, ph * c:(ph + 1) * c] = xz[:, :, ri[a][:, None], si[bb][None, :]]
    return out


def _fold(g_full, pad_lo, n_src, mode, axis):
    """the adjoint of one axis: padded coordinate p of `axis` adds to source coordinate map(p - pad_lo), zero drops"""
    shape = list(g_full.shape)
    shape[axis] = n_src
    out = np.zeros(shape, dtype=g_full.dtype)
    src, dst = [slice(None)] * g_full.ndim, [slice(None)] * g_full.ndim
    for p in range(g_full.shape[axis]):
        m = map_coord(p - pad_lo, n_src, mode)
        if m >= 0:
            src[axis], dst[axis] = p, m
            out[tuple(dst)] += g_full[tuple(src)]
    return out


def s2d_pad_bwd(g, pad, modes, hh, ww, stats=False):
    """adjoint of s2d_pad: g (n, 4c, hp, wp) -> dx (n, c, hh, ww): the phases interleaved back to the padded grid, clipped to the
    padded image, then each axis folded onto the source (rows first).  stats=True: also the number of terms of every element
    (hh, ww) and the sum of their magnitudes (float64)."""
    n, c4, hp, wp = g.shape
    c = c4 // 4
    t, b, l, r = pad
    full = np.zeros((n, c, 2 * hp, 2 * wp), dtype=g.dtype)
    for a in (0, 1):
        for bb in (0, 1):
            ph = 2 * a + bb
            full[:, :, a::2, bb::2] = g[:, ph * c:(ph + 1) * c]
    full = full[:, :, :min(2 * hp, hh + t + b), :min(2 * wp, ww + l + r)]

    def fold(v):
        return _fold(_fold(v, t, hh, modes[0], 2), l, ww, modes[1], 3)
    dx = fold(full)
    if stats:
        cnt = fold(np.ones((1, 1) + full.shape[2:], dtype=np.int64))[0, 0]
        return dx, cnt, fold(np.abs(full).astype(np.float64))
    return dx


def pad_np(x, pad, modes):
    """the halo as np.pad applies it, rows first (corners follow from applying the two axes in turn)"""
    t, b, l, r = pad
    x = np.pad(x, ((0, 0), (0, 0), (t, b), (0, 0)), mode=NP_MODE[modes[0]])
    return np.pad(x, ((0, 0), (0, 0), (0, 0), (l, r)), mode=NP_MODE[modes[1]])


def compose(halo, modes, own):
    """the lazy halo in front of the layer composed with the layer's own zeros (plan._compose_halo), None where they do not compose"""
    def axis(lo0, hi0, m0, lo1, hi1):
        if lo1 == 0 and hi1 == 0:
            return lo0, hi0, m0
        if lo0 == 0 and hi0 == 0:
            return lo1, hi1, ZERO
        if m0 == ZERO:
            return lo0 + lo1, hi0 + hi1, ZERO
        return None
    ah = axis(halo[0], halo[1], modes[0], own[0], own[1])
    aw = axis(halo[2], halo[3], modes[1], own[2], own[3])
    if ah is None or aw is None:
        return None
    return (ah[0], ah[1], aw[0], aw[1]), (ah[2], aw[2])


def activate(y, activation):
    if activation in (None, 'linear'):
        return y
    return np.tanh(y) if activation == 'tanh' else np.maximum(y, 0)


def restated(x, K, bias=None, padding='valid', activation=None, taps=None, halo=None):
    """the layer as the library runs it: padded space-to-depth (the halo in front composed in, or applied first where it does
    not compose), weight map, ONE stride-1 'valid' cross-correlation with sh x sw taps, bias, activation.  halo = (pad, modes)."""
    kh, kw, cin, f = K.shape
    pad, modes = halo if halo is not None else ((0, 0, 0, 0), (ZERO, ZERO))
    hl, wl = x.shape[2] + pad[0] + pad[1], x.shape[3] + pad[2] + pad[3]
    (th, pt, pb, ho), (tw, pl, pr, wo) = geometry(kh, padding, hl), geometry(kw, padding, wl)
    both = compose(pad, modes, (pt, pb, pl, pr))
    if both is None:
        x = pad_np(x, pad, modes)
        both = ((pt, pb, pl, pr), (ZERO, ZERO))
    sh, sw = taps if taps is not None else (th, tw)
    p = s2d_pad(x, both[0], both[1], ho + sh - 1, wo + sw - 1)
    w2 = weight_map(K, (sh, sw))
    y = np.zeros((x.shape[0], f, ho, wo), dtype=x.dtype)
    for ti in range(sh):
        for tj in range(sw):
            y += np.einsum('ncij,cf->nfij', p[:, :, ti:ti + ho, tj:tj + wo], w2[ti, tj])
    if bias is not None:
        y += bias.reshape(1, f, 1, 1)
    return activate(y, activation)


def reference(x, K, bias=None, padding='valid', activation=None):
    """float64 torch.nn.functional.conv2d(F.pad(x, TensorFlow's 'same'), w, stride=2) on the CPU"""
    import torch
    import torch.nn.functional as F
    kh, kw, cin, f = K.shape
    (_, pt, pb, _), (_, pl, pr, _) = geometry(kh, padding, x.shape[2]), geometry(kw, padding, x.shape[3])
    xt = F.pad(torch.from_numpy(np.asarray(x, dtype=np.float64)), (pl, pr, pt, pb))
    w = torch.from_numpy(np.ascontiguousarray(np.asarray(K, dtype=np.float64).transpose(3, 2, 0, 1)))
    b = torch.from_numpy(np.asarray(bias, dtype=np.float64)) if bias is not None else None
    y = F.conv2d(xt, w, b, stride=2)
    if activation == 'tanh':
        y = torch.tanh(y)
    elif activation == 'relu':
        y = torch.relu(y)
    return y.numpy()
