"""Conv2DTranspose(strides=2) and Cropping2D restated on the host, for tests/test_tconv_cpu.py and tests/test_gpu_tconv.py (a helper
module, not a test file).

Keras 2.2.4 / TensorFlow, channels_first: y_full[n, o, 2i+u, 2j+v] += x[n, c, i, j] K[u, v, o, c] (no flip) on Hf = 2h + max(kh-2, 0)
rows; 'same' keeps rows [pt, pt + 2h), pt = max(kh-2, 0) // 2.  The package runs the layer as a stride-1 cross-correlation with
4 F phase channels (T = ceil(k / 2) taps per axis, zero halo T - 1) + an interleave that crops (csrc/tconv.hip); the functions here
restate every step in numpy, dtype in = dtype out, so that float32 inputs give the bits the kernels must give (they move and
zero-fill only) and float64 inputs give the reference of the layer's arithmetic."""
import numpy as np

KERNELS = [(kh, kw) for kh in range(1, 6) for kw in range(1, 6)]          # every kh, kw in 1 ... 5, (2, 3) and (5, 1) among them
MAPS = [(1, 1), (2, 3), (5, 4)]
PADDINGS = ['valid', 'same']


def geometry(k, padding, length):
    """(T, crop, out_len) of one axis: taps on the source, offset of the output in the interleaved phase tensor, Keras' deconv_length"""
    extra = max(k - 2, 0)
    return (k + 1) // 2, (extra // 2 if padding == 'same' else 0), (2 * length if padding == 'same' else 2 * length + extra)


def stored_taps(th, tw):
    """the taps the planner stores the derived kernel with: 3 x 3 (T <= 3), 5 x 5 (T <= 5) -- the sizes the library's matrix-core
    forward and weight-gradient kernels exist for -- else T itself"""
    t = max(th, tw)
    return (3, 3) if t <= 3 else ((5, 5) if t <= 5 else (th, tw))


def weight_map(K, bias=None, taps=None):
    """K (kh, kw, F, cin) -> w2 (Th, Tw, cin, 4F): w2[ti, tj, c, (2a+b) F + o] = K[a + 2(Th-1-ti), b + 2(Tw-1-tj), o, c], zero where
    that index is outside K; b2 = the bias once per phase (None without a bias).  taps = (sh, sw) >= (Th, Tw): w2 is stored with
    sh x sw taps, the Th x Tw block at offset ((sh - Th) // 2, (sw - Tw) // 2) and zeros around it"""
    kh, kw, f, cin = K.shape
    th, tw = (kh + 1) // 2, (kw + 1) // 2
    sh, sw = taps or (th, tw)
    oh, ow = (sh - th) // 2, (sw - tw) // 2
    w2 = np.zeros((sh, sw, cin, 4 * f), dtype=K.dtype)
    for ti in range(th):
        for tj in range(tw):
            for a in range(2):
                for b in range(2):
                    u, v = a + 2 * (th - 1 - ti), b + 2 * (tw - 1 - tj)
                    if u < kh and v < kw:
                        w2[oh + ti, ow + tj, :, (2 * a + b) * f:(2 * a + b + 1) * f] = K[u, v].T
    return w2, (None if bias is None else np.tile(bias, 4))


def weight_map_bwd(dw2, kshape):
    """the adjoint: every element of K sits in exactly one element of w2 -- a gather, no sums (the stored taps are dw2's)"""
    kh, kw, f, cin = kshape
    th, tw = (kh + 1) // 2, (kw + 1) // 2
    oh, ow = (dw2.shape[0] - th) // 2, (dw2.shape[1] - tw) // 2
    dk = np.empty(kshape, dtype=dw2.dtype)
    for u in range(kh):
        for v in range(kw):
            ph = 2 * (u & 1) + (v & 1)
            dk[u, v] = dw2[oh + th - 1 - u // 2, ow + tw - 1 - v // 2, :, ph * f:(ph + 1) * f].T
    return dk


def depth_to_space(ph, f):
    """(n, 4F, hp, wp) phase-major -> (n, F, 2hp, 2wp)"""
    n, _, hp, wp = ph.shape
    out = np.empty((n, f, 2 * hp, 2 * wp), dtype=ph.dtype)
    for a in range(2):
        for b in range(2):
            out[:, :, a::2, b::2] = ph[:, (2 * a + b) * f:(2 * a + b + 1) * f]
    return out


def d2s_crop(ph, f, top, left, out_h, out_w):
    return np.ascontiguousarray(depth_to_space(ph, f)[:, :, top:top + out_h, left:left + out_w])


def s2d_fill(dy, hp, wp, top, left):
    """the adjoint of d2s_crop: (n, F, H, W) -> (n, 4F, hp, wp), +0 where the crop dropped the pixel"""
    n, f, hh, ww = dy.shape
    full = np.zeros((n, f, 2 * hp, 2 * wp), dtype=dy.dtype)
    full[:, :, top:top + hh, left:left + ww] = dy
    out = np.empty((n, 4 * f, hp, wp), dtype=dy.dtype)
    for a in range(2):
        for b in range(2):
            out[:, (2 * a + b) * f:(2 * a + b + 1) * f] = full[:, :, a::2, b::2]
    return out


def phase_tensor(x, K, bias=None, taps=None):
    """the stride-1 cross-correlation of x (zero halo T - 1) with the derived kernel: (n, 4F, h + Th - 1, w + Tw - 1).  With more
    stored taps the zero halo grows by the block's offset above / left and by the rest below / right: the same tensor"""
    w2, b2 = weight_map(K, bias, taps)
    th, tw = (K.shape[0] + 1) // 2, (K.shape[1] + 1) // 2
    sh, sw = w2.shape[:2]
    oh, ow = (sh - th) // 2, (sw - tw) // 2
    xp = np.pad(x, ((0, 0), (0, 0), (th - 1 + oh, th - 1 + sh - th - oh), (tw - 1 + ow, tw - 1 + sw - tw - ow)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (sh, sw), axis=(2, 3))        # (n, c, hp, wp, sh, sw)
    ph = np.einsum('nchwij,ijco->nohw', win, w2)
    return ph if b2 is None else ph + b2.reshape(1, -1, 1, 1)


def restated(x, K, bias=None, padding='valid', activation='linear', full=False, taps=None):
    """the layer as the package computes it, in the dtype of its arguments.  full: the whole depth-to-space image instead"""
    kh, kw, f, _ = K.shape
    ph = phase_tensor(x, K, bias, taps)
    if full:
        return depth_to_space(ph, f)
    (_, top, ho), (_, left, wo) = geometry(kh, padding, x.shape[2]), geometry(kw, padding, x.shape[3])
    return activate(d2s_crop(ph, f, top, left, ho, wo), activation)


def activate(y, activation):
    return {'linear': lambda t: t, None: lambda t: t, 'tanh': np.tanh, 'relu': lambda t: np.maximum(t, 0)}[activation](y)


def reference(x, K, bias=None, padding='valid'):
    """float64 torch on the CPU: 'valid' is conv_transpose2d(stride=2) (for k = 1 Keras' deconv_length is one row / column short of
    it: none in that case); 'same' is the autograd gradient of a SAME-padded stride-2 conv2d (TensorFlow's padding: total
    max(k - 2, 0), the smaller half first)"""
    import torch
    import torch.nn.functional as F
    kh, kw, f, cin = K.shape
    xt = torch.tensor(np.asarray(x, np.float64))
    wt = torch.tensor(np.ascontiguousarray(np.asarray(K, np.float64).transpose(3, 2, 0, 1)))       # (cin, F, kh, kw)
    n, _, h, w = x.shape
    if padding == 'valid':
        y = F.conv_transpose2d(xt, wt, stride=2)
        ho, wo = geometry(kh, 'valid', h)[2], geometry(kw, 'valid', w)[2]
        y = F.pad(y, (0, max(wo - y.shape[3], 0), 0, max(ho - y.shape[2], 0)))[:, :, :ho, :wo]      # (k = 1: a zero last row / column)
    else:
        z = torch.zeros((n, f, 2 * h, 2 * w), dtype=torch.float64, requires_grad=True)
        th, tw_ = max(kh - 2, 0), max(kw - 2, 0)
        zp = F.pad(z, (tw_ // 2, tw_ - tw_ // 2, th // 2, th - th // 2))
        out = F.conv2d(zp, wt, stride=2)                      # conv2d weight (cin, F, kh, kw): out channel c, in channel o
        assert tuple(out.shape) == tuple(xt.shape)
        (y,) = torch.autograd.grad(out, z, xt)
    y = y.detach().numpy()
    return y if bias is None else y + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
