"""DepthwiseConv2D / SeparableConv2D restated in numpy: the depthwise stencil and the pointwise product of csrc/sepconv.hip, their three
adjoints each, the halo maps, and the case tables of tests/test_sepconv_cpu.py and tests/test_gpu_sepconv.py.  Every helper returns
the dtype it was given (float64 in: float64 arithmetic)."""
import numpy as np

ZERO, WRAP, EDGE, REFLECT, SYMMETRIC = 0, 1, 2, 3, 4          # DLWP_PAD_* (include/dlwp_hip.h)
MODES = (ZERO, WRAP, EDGE, REFLECT, SYMMETRIC)
MODE_PAIRS = [(mh, mw) for mh in MODES for mw in MODES]
EPS = 2.0 ** -24

# ---- depthwise cases ----------------------------------------------------------------------------------------------------------------- #
DW_TILE = (32, 64)                                             # csrc/sepconv.hip: the largest output tile (rows 32 | 16 | 8 by the map's height)
DW_MAPS = [(n, c, h, w) for (h, w) in ((1, 1), (5, 7), (7, 9)) for n in (1, 3) for c in (1, 5)] + [(2, 3, 37, 70)]
DW_KERNELS = ((3, 3), (5, 5), (1, 3), (3, 1), (2, 2))
DW_DILATIONS = (1, 2)
DW_MULTIPLIERS = (1, 2, 3)
DW_HALOS = ((0, 0, 0, 0), (2, 2, 2, 2), (1, 0, 0, 3))
DW_SPAN = 4096                                                 # positions per first-stage partial of the depthwise weight gradient

# ---- pointwise cases ----------------------------------------------------------------------------------------------------------------- #
PW_Q = (1, 3, 33, 64)
PW_O = (1, 4, 35, 64)
PW_HW = (1, 35, 990)
PW_N = (1, 3)
PW_UNIT, PW_UNITS = 32, 16                                     # a unit = 32 pixels of one sample; 16 units per first-stage partial


def pw_partials(n, hw):
    """first-stage partials of the pointwise weight gradient (dlwp_pointwise2d_bwd_workspace / (q o 4))"""
    units = n * -(-hw // PW_UNIT)
    return max(-(-units // PW_UNITS), 1)


def dw_partials(n, ho, wo):
    return max(-(-(n * ho * wo) // DW_SPAN), 1)


# ---- halo maps ----------------------------------------------------------------------------------------------------------------------- #
def pad_fits(lo, hi, n, mode):
    """halo amounts a mode can serve on an axis of n (dlwp_pad_fits)"""
    m = max(lo, hi)
    if mode in (WRAP, SYMMETRIC):
        return m <= n
    if mode == REFLECT:
        return m <= n - 1
    return True


def halo_fits(pad, modes, h, w):
    return pad_fits(pad[0], pad[1], h, modes[0]) and pad_fits(pad[2], pad[3], w, modes[1])


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


def _axis(n, lo, hi, mode):
    return np.array([map_coord(p - lo, n, mode) for p in range(n + lo + hi)], dtype=np.int64)


def pad_np(x, pad, modes):
    """x (..., h, w) under the halo: rows through modes[0], columns through modes[1], +0 where a map says zero"""
    h, w = x.shape[-2:]
    ri, ci = _axis(h, pad[0], pad[1], modes[0]), _axis(w, pad[2], pad[3], modes[1])
    y = x[..., np.maximum(ri, 0), :][..., np.maximum(ci, 0)]
    y = y * (ri >= 0)[:, None].astype(x.dtype) * (ci >= 0)[None, :].astype(x.dtype)
    return y


def pad_bwd(g, pad, modes, h, w):
    """adjoint of pad_np: wrap adds the periodic images, edge adds to the border, the mirrors add their reflections, zero drops"""
    ri, ci = _axis(h, pad[0], pad[1], modes[0]), _axis(w, pad[2], pad[3], modes[1])
    rows = np.zeros(g.shape[:-2] + (h, g.shape[-1]), dtype=g.dtype)
    np.add.at(rows, (Ellipsis, ri[ri >= 0], slice(None)), g[..., ri >= 0, :])
    out = np.zeros(g.shape[:-2] + (h, w), dtype=g.dtype)
    np.add.at(out, (Ellipsis, ci[ci >= 0]), rows[..., ci >= 0])
    return out


def act_np(y, act):
    if act == 'tanh':
        return np.tanh(y)
    if act == 'relu':
        return np.maximum(y, 0)
    return y


def out_hw(h, w, pad, ks, dil):
    return h + pad[0] + pad[1] - dil[0] * (ks[0] - 1), w + pad[2] + pad[3] - dil[1] * (ks[1] - 1)


# ---- the depthwise stencil ----------------------------------------------------------------------------------------------------------- #
def depthwise(x, K, b=None, pad=(0, 0, 0, 0), modes=(ZERO, ZERO), dil=(1, 1), act=None):
    """y[n][c dm + m][i][j] = act(b[c dm + m] + sum_{u,v} xpad[n][c][i + u dh][j + v dw] K[u][v][c][m]);  K (kh, kw, cin, dm)"""
    kh, kw, cin, dm = K.shape
    n, c, h, w = x.shape
    assert c == cin
    xp = pad_np(x, pad, modes)
    ho, wo = out_hw(h, w, pad, (kh, kw), dil)
    assert ho >= 1 and wo >= 1
    y = np.zeros((n, cin, dm, ho, wo), dtype=x.dtype)
    if b is not None:
        y += b.reshape(1, cin, dm, 1, 1)
    for u in range(kh):
        for v in range(kw):
            y += xp[:, :, None, u * dil[0]:u * dil[0] + ho, v * dil[1]:v * dil[1] + wo] * K[u, v][None, :, :, None, None]
    return act_np(y.reshape(n, cin * dm, ho, wo), act)


def depthwise_bwd_data(dz, K, pad, modes, dil, h, w):
    """the adjoint of depthwise (linear activation) in x, halo included"""
    kh, kw, cin, dm = K.shape
    n = dz.shape[0]
    ho, wo = dz.shape[2:]
    g = np.zeros((n, cin, h + pad[0] + pad[1], w + pad[2] + pad[3]), dtype=dz.dtype)
    dzr = dz.reshape(n, cin, dm, ho, wo)
    for u in range(kh):
        for v in range(kw):
            g[:, :, u * dil[0]:u * dil[0] + ho, v * dil[1]:v * dil[1] + wo] += (dzr * K[u, v][None, :, :, None, None]).sum(axis=2)
    return pad_bwd(g, pad, modes, h, w)


def depthwise_bwd_weight(x, dz, pad, modes, dil, ks):
    """dK[u][v][c][m] = sum_{n,i,j} xpad[n][c][i + u dh][j + v dw] dz[n][c dm + m][i][j]"""
    n, cin, h, w = x.shape
    ho, wo = dz.shape[2:]
    dm = dz.shape[1] // cin
    xp = pad_np(x, pad, modes)
    dzr = dz.reshape(n, cin, dm, ho, wo)
    dk = np.zeros((ks[0], ks[1], cin, dm), dtype=x.dtype)
    for u in range(ks[0]):
        for v in range(ks[1]):
            dk[u, v] = (xp[:, :, None, u * dil[0]:u * dil[0] + ho, v * dil[1]:v * dil[1] + wo] * dzr).sum(axis=(0, 3, 4))
    return dk


# ---- the pointwise product ----------------------------------------------------------------------------------------------------------- #
def pointwise(x, P, b=None, act=None):
    """y[n][o][p] = act(b[o] + sum_q x[n][q][p] P[q][o]);  x (n, q, ...), P (q, o)"""
    n, q = x.shape[:2]
    y = np.einsum('nqp,qo->nop', x.reshape(n, q, -1), P)
    if b is not None:
        y = y + b.reshape(1, -1, 1)
    return act_np(y.reshape((n, P.shape[1]) + x.shape[2:]), act)


def pointwise_bwd_data(dz, P):
    n, o = dz.shape[:2]
    return np.einsum('nop,qo->nqp', dz.reshape(n, o, -1), P).reshape((n, P.shape[0]) + dz.shape[2:])


def pointwise_bwd_weight(x, dz):
    n = x.shape[0]
    return np.einsum('nqp,nop->qo', x.reshape(n, x.shape[1], -1), dz.reshape(n, dz.shape[1], -1))


# ---- both stages --------------------------------------------------------------------------------------------------------------------- #
def separable(x, K, P, b=None, pad=(0, 0, 0, 0), modes=(ZERO, ZERO), dil=(1, 1), act=None):
    return pointwise(depthwise(x, K, None, pad, modes, dil), P.reshape(P.shape[-2:]), b, act)


def same_halo(ks, dil):
    """Keras 'same' at stride 1: dil (k - 1) zeros per axis, the smaller half first"""
    th, tw = dil[0] * (ks[0] - 1), dil[1] * (ks[1] - 1)
    return (th // 2, th - th // 2, tw // 2, tw - tw // 2)


def fans(shape):
    """keras.initializers._compute_fans on a convolution kernel shape: receptive field x shape[-2], x shape[-1]"""
    rf = int(np.prod(shape[:-2]))
    return rf * shape[-2], rf * shape[-1]


def small_ints(rng, shape, dtype=np.float32):
    """integers in [-4, 4]: every sum of products the kernels form is exact in float32"""
    return rng.integers(-4, 5, size=shape).astype(dtype)
