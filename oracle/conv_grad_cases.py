"""The layers and the two input families of tests/test_conv_grads_cpu.py and tests/test_gpu_conv_grads.py: the six convolutions of
presets.unet_layers((4, 88, 180)) as training.py drives them (PeriodicPadding2D + ZeroPadding2D halos: zero rows, periodic columns;
pooled and up-sampled sources read through the loader), config 1's two 5x5 layers on the odd 73 x 144 grid, the 3x3 decoder shape the
fused activation backward runs on, and the first / fifth layer at 180 x 360.

(a) exact: small integers.  Every product, every Winograd transform and every partial sum is a multiple of 1/4 (the transforms' only
non-integer constants are 1/2, twice) and stays below 2^22 in size as long as  gain * A < 2^22,  A the absolute-value sum of the
result element and `gain` the product of the transforms' largest absolute row sums: float32 holds all of them exactly, in any order.
(b) reals: standard-normal x and dz, glorot-uniform kernels."""
import numpy as np

from . import np_ref

LIMIT = 2.0 ** 22

# Largest gain of the value range on a path, from the matrices in the kernels' headers (rows: absolute row sums)
#   weight gradient, Winograd F(2x2, 3x3) (conv_wgrad_kernel.h, _cb_, _cbu_):  input tile  B^T d B,  B^T rows (1, 0, -1, 0) (0, 1, 1, 0)
#   (0, -1, 1, 0) (0, 1, 0, -1): 2 per axis = 4;  dz tile  A dz A^T,  A rows (1, 0) (1, 1) (1, -1) (0, -1): 2 per axis = 4;  output
#   G^T M G,  G^T rows (1, 1/2, 1/2, 0) (0, 1/2, -1/2, 0) (0, 1/2, 1/2, 1): 2 per axis = 4  ->  64.  The direct forms (conv_wgrad_c4_kernel.h,
#   packed-N, 5x5): products and sums only  ->  1.
#   data gradient = the forward convolution (conv_fwd_wino_kernel.h / conv_fwd.hip):  filter  G g G^T,  G rows (1, 0, 0) (1/2, 1/2, 1/2)
#   (1/2, -1/2, 1/2) (0, 0, 1): 3/2 per axis = 9/4;  input tile B^T d B: 4;  output  A^T m A,  A^T rows (1, 1, 1, 0) (0, 1, -1, -1): 3 per
#   axis = 9  ->  81.
GAIN_WGRAD_WINO, GAIN_WGRAD_DIRECT, GAIN_DGRAD = 64.0, 1.0, 81.0


def _layer(name, cin, cout, k, dil, src, hs, ws, pick_gain=None):
    """hs, ws: the STORED input's plane; the convolution sees it pooled (src 2) or up-sampled (src 1)"""
    f = {0: 1.0, 1: 2.0, 2: 0.5}[src]
    gain = GAIN_WGRAD_WINO if k == 3 else GAIN_WGRAD_DIRECT
    return dict(name=name, cin=cin, cout=cout, hs=hs, ws=ws, ho=int(hs * f), wo=int(ws * f), layer=np_ref.conv_layer(k, dil, src=src),
                gain=gain, pick_gain=gain if pick_gain is None else pick_gain)


LAYERS = {
    'L1': _layer('L1', 4, 32, 3, 2, 0, 88, 180, pick_gain=GAIN_WGRAD_DIRECT),       # the 4-channel streaming form at every size
    'L2': _layer('L2', 32, 64, 3, 1, 2, 88, 180),
    'L3': _layer('L3', 64, 128, 3, 1, 2, 44, 90),
    'L4': _layer('L4', 128, 64, 3, 1, 1, 22, 45),
    'L5': _layer('L5', 64, 32, 3, 2, 1, 44, 90),
    'L6': _layer('L6', 32, 4, 5, 1, 0, 88, 180),
    'D3': _layer('D3', 64, 32, 3, 1, 0, 44, 90),                                    # dlwp_conv2d_bwd_data_act runs fused here
    'C1a': _layer('C1a', 4, 32, 5, 1, 0, 73, 144),
    'C1b': _layer('C1b', 32, 4, 5, 1, 0, 73, 144),
    'L1x': _layer('L1x', 4, 32, 3, 2, 0, 180, 360, pick_gain=GAIN_WGRAD_DIRECT),
    'L5x': _layer('L5x', 64, 32, 3, 2, 1, 90, 180),
}

DENSE_VALUES = np.array([-2., -1., 1., 2.], dtype=np.float32)                       # mean |v| = 3/2


def thin_density(L, n, gain):
    """The density of the thinned operand of a weight gradient: with the other operand dense (|v| <= 2, mean 3/2) the expected
    A = n ho wo * p * 9/4 stays at half of LIMIT / gain; the condition itself is checked on the generated arrays (exact_condition)."""
    return min(1.0, 0.5 * LIMIT / (gain * n * L['ho'] * L['wo'] * 2.25))


def _ints(rng, shape, p):
    v = DENSE_VALUES[rng.integers(0, 4, size=shape)]
    if p < 1.0:
        v = v * (rng.random(shape, dtype=np.float32) < p)
    return v.astype(np.float32)


def exact_case(L, n, seed, gain=None):
    """family (a).  seed 0: x dense (no zero at all), dz thinned; seed 1: dz dense, x thinned -- over the two seeds every element of
    both tensors is non-zero at least once.  The kernel: integers in [-2, 2]."""
    gain = L['gain'] if gain is None else gain
    rng = np.random.default_rng([n, seed, L['cin'], L['cout'], L['hs']])
    p = thin_density(L, n, gain)
    px = p / 4 if L['layer']['src'] == np_ref.SRC_MAXPOOL2 and p < 1.0 else p       # a pooled window is non-zero ~4 times as often
    x = _ints(rng, (n, L['cin'], L['hs'], L['ws']), 1.0 if seed == 0 else px)
    dz = _ints(rng, (n, L['cout'], L['ho'], L['wo']), p if seed == 0 else 1.0)
    k = L['layer']['k']
    w = rng.integers(-2, 3, size=(k, k, L['cin'], L['cout'])).astype(np.float32)
    return x, dz, w


def real_case(L, n, seed):
    """family (b)"""
    rng = np.random.default_rng([n, seed, L['cin'], L['cout'], L['hs'], 7])
    x = rng.standard_normal((n, L['cin'], L['hs'], L['ws']), dtype=np.float32)
    dz = rng.standard_normal((n, L['cout'], L['ho'], L['wo']), dtype=np.float32)
    k = L['layer']['k']
    w = np_ref.glorot_uniform((k, k, L['cin'], L['cout']), rng)
    return x, dz, np.asarray(w, np.float32)


def exact_condition(abs_sums, gain):
    """gain * (largest absolute-value sum): below LIMIT, every intermediate of the path is a multiple of 1/4 that float32 holds exactly"""
    return gain * float(np.max(abs_sums))
