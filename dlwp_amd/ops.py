"""
Tensor-level wrappers over the C ABI.  torch is used ONLY as plumbing here: device allocations (torch.empty), the
current HIP stream, and device indices.  Every arithmetic / data-movement operation is a libdlwp_hip.so kernel.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_LINEAR, ACT_RELU, ACT_TANH, PAD_EDGE, PAD_REFLECT, PAD_SYMMETRIC, PAD_WRAP, PAD_ZERO,  # noqa: F401
                   SRC_DIRECT, SRC_MAXPOOL2,
                   SRC_UPSAMPLE2, Conv2d, Pad2d, Shape4)
from .plan import _phase_geometry

ACTIVATIONS = {None: ACT_LINEAR, 'linear': ACT_LINEAR, 'tanh': ACT_TANH, 'relu': ACT_RELU}


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(t):
    """the current HIP stream of t's device (torch.cuda.current_stream builds a Stream object per call: ~5 us, 50 times per
    training step; the raw handle is what the C ABI wants anyway)"""
    if _raw_stream is not None:
        idx = t.device.index
        return ctypes.c_void_p(_raw_stream(idx if idx is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(t):
    if not t.is_cuda:
        raise RuntimeError('dlwp_amd ops need device (HIP) tensors; there is no CPU fallback')
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _check_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('expected contiguous float32 tensors, got %s contiguous=%s' % (t.dtype, t.is_contiguous()))


def _check_act(*ts):
    """activation tensors: contiguous float32 or bfloat16 (storage types of the forward convolutions / max-pooling)"""
    for t in ts:
        if t is None:
            continue
        if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous():
            raise ValueError('expected contiguous float32 / bfloat16 tensors, got %s contiguous=%s' %
                             (t.dtype, t.is_contiguous()))


def storage_code(t):
    return _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32


def make_pad(top=0, bottom=0, left=0, right=0, mode_h=PAD_ZERO, mode_w=PAD_ZERO):
    return Pad2d(int(top), int(bottom), int(left), int(right), int(mode_h), int(mode_w))


def make_conv(cout, kh, kw, dil=1, halo=None, act=ACT_LINEAR, in_c_off=0, in_c_total=0, out_c_off=0, out_c_total=0,
              src_mode=SRC_DIRECT, out_pool=False, out_d2s=False, lstm_f=0, lstm_rec_act=0):
    dh, dw = (dil, dil) if isinstance(dil, int) else dil
    return Conv2d(int(cout), int(kh), int(kw), int(dh), int(dw), halo if halo is not None else make_pad(), int(act),
                  int(in_c_off), int(in_c_total), int(out_c_off), int(out_c_total), int(src_mode), int(bool(out_pool)),
                  int(bool(out_d2s)), int(lstm_f), int(lstm_rec_act))


def supports_out_pool(xs_chw, cd):
    """Planner hint: can a compiled kernel apply a following MaxPooling2D(2) in this convolution's epilogue?"""
    return bool(_lib.lib.dlwp_conv2d_supports_out_pool(_lib.handle_or_none(), Shape4(1, int(xs_chw[0]), int(xs_chw[1]), int(xs_chw[2])),
                                                       ctypes.byref(cd)))


def supports_out_d2s(xs_chw, cd):
    """Planner hint: can a compiled kernel store this convolution's 4 F phase channels interleaved (depth-to-space)?"""
    return bool(_lib.lib.dlwp_conv2d_supports_out_d2s(_lib.handle_or_none(), Shape4(1, int(xs_chw[0]), int(xs_chw[1]), int(xs_chw[2])),
                                                      ctypes.byref(cd)))


def conv_out_shape(xs, cd):
    ys = Shape4()
    _lib.check(_lib.lib.dlwp_conv2d_out_shape(xs, ctypes.byref(cd), ctypes.byref(ys)))
    return ys


def pad2d(x, pad, channels_last=False, out=None):
    """x: NCHW (or NHWC with channels_last=True) -> padded copy."""
    _check_f32(x)
    if channels_last:
        n, h, w, c = x.shape
        outer, inner = n, c
        oshape = (n, h + pad.top + pad.bottom, w + pad.left + pad.right, c)
    else:
        n, c, h, w = x.shape
        outer, inner = n * c, 1
        oshape = (n, c, h + pad.top + pad.bottom, w + pad.left + pad.right)
    y = out if out is not None else torch.empty(oshape, dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib.dlwp_pad2d_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), outer, h, w, inner, pad, _lib.F32,
                                       _stream(x)))
    return y


def pad2d_bwd(dy, x_shape, pad, channels_last=False):
    _check_f32(dy)
    if channels_last:
        n, h, w, c = x_shape
        outer, inner = n, c
    else:
        n, c, h, w = x_shape
        outer, inner = n * c, 1
    dx = torch.empty(tuple(x_shape), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.lib.dlwp_pad2d_bwd(_lib.handle(_dev(dy)), _ptr(dy), _ptr(dx), outer, h, w, inner, pad, _lib.F32,
                                       _stream(dy)))
    return dx


def _code(t, o8=False):
    return _lib.BF16_O8 if o8 else storage_code(t)


def conv2d_prepare(x, w_hwio, cd, out_dtype=None, x_channels=None, compute_bf16=False, out=None, in_o8=False, out_o8=False):
    """Prepared weights for conv2d(x, ...) calls with exactly this input shape / storage (dlwp_conv2d_prepare), or None
    when the layer's kernel reads the HWIO weights directly.  out: a buffer an earlier call returned (refilled in place)."""
    _check_f32(w_hwio)
    n, c_total, h, w = x.shape
    cin = int(x_channels) if x_channels is not None else c_total
    if cd.in_c_total == 0 and cin != c_total:
        cd.in_c_total = c_total
    xs = Shape4(n, cin, h, w)
    out_code = storage_code(x) if out_dtype is None else {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[out_dtype]
    dt = _lib.dtype_io(_code(x, in_o8), _lib.BF16_O8 if out_o8 else out_code, compute_bf16)
    nbytes = _lib.lib.dlwp_conv2d_prepared_bytes(_lib.handle(_dev(x)), xs, ctypes.byref(cd), dt)
    if nbytes == 0:
        return None
    u = out if out is not None else torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    if u.numel() * 4 < nbytes:
        raise ValueError('conv2d_prepare: the buffer holds %d bytes, %d needed' % (u.numel() * 4, nbytes))
    _lib.check(_lib.lib.dlwp_conv2d_prepare(_lib.handle(_dev(x)), _ptr(w_hwio), _ptr(u), xs, ctypes.byref(cd), dt,
                                            _stream(x)))
    return u


def conv2d(x, w_hwio, bias, cd, out=None, direct=False, x_channels=None, compute_bf16=False, prepared=None, in_o8=False,
           out_o8=False, out_pool2=None):
    """x: stored input (n, in_c_total, h, w); the conv reads `x_channels` (default: all) channels from cd.in_c_off.
    Returns (n, out_c_total, ho, wo); writes channels [out_c_off, out_c_off+cout).  compute_bf16: a float32 x may be
    rounded to bfloat16 so that the layer runs on the bf16 matrix cores (DLWP_COMPUTE_BF16).  prepared: the tensor
    conv2d_prepare returned for this call (the weights are then not transformed again).  in_o8 / out_o8: the bfloat16
    tensor x / out holds channel OCTETS, (n, C/8, h, w, 8) in the memory of an (n, C, h, w) tensor (DLWP_BF16_O8).
    out_pool2: a float32 (n, out_c_total, ho/2, wo/2) tensor that receives MaxPooling2D(2) of the output from the same launch
    (dlwp_conv2d_fwd_pool2); returns None -- nothing written -- where the layer's kernel cannot store both."""
    _check_act(x, out)
    _check_f32(w_hwio, bias)
    n, c_total, h, w = x.shape
    cin = int(x_channels) if x_channels is not None else c_total
    if tuple(w_hwio.shape) != (cd.kh, cd.kw, cin, cd.cout):
        raise ValueError('kernel shape %s does not match (kh,kw,cin,cout)=(%d,%d,%d,%d)' %
                         (tuple(w_hwio.shape), cd.kh, cd.kw, cin, cd.cout))
    if cd.in_c_total == 0 and cin != c_total:
        cd.in_c_total = c_total
    xs = Shape4(n, cin, h, w)
    ys = conv_out_shape(xs, cd)
    oc = cd.out_c_total if cd.out_c_total > 0 else ys.c
    if out is None:
        out = torch.empty((n, oc, ys.h, ys.w), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (n, oc, ys.h, ys.w):
        raise ValueError('output buffer shape %s != %s' % (tuple(out.shape), (n, oc, ys.h, ys.w)))
    fn = _lib.lib.dlwp_conv2d_fwd_direct if direct else _lib.lib.dlwp_conv2d_fwd
    if (in_o8 and x.dtype != torch.bfloat16) or (out_o8 and out.dtype != torch.bfloat16):
        raise ValueError('the octet layout is a bfloat16 storage')
    dt = _lib.dtype_io(_code(x, in_o8), _code(out, out_o8), compute_bf16)      # storage of x / y
    if out_pool2 is not None:
        _check_f32(x, out, out_pool2)
        if tuple(out_pool2.shape) != (n, oc, ys.h // 2, ys.w // 2) or not out_pool2.is_contiguous():
            raise ValueError('pooled output buffer shape %s != %s' % (tuple(out_pool2.shape), (n, oc, ys.h // 2, ys.w // 2)))
        rc = _lib.lib.dlwp_conv2d_fwd_pool2(_lib.handle(_dev(x)), _ptr(x), _ptr(w_hwio), _ptr(prepared), _ptr(bias), _ptr(out),
                                            _ptr(out_pool2), xs, ctypes.byref(cd), dt, _stream(x))
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc)
        return out
    with few_wino_scope_of(cd, _dev(x)):
        if prepared is not None and not direct:
            _lib.check(_lib.lib.dlwp_conv2d_fwd_prepared(_lib.handle(_dev(x)), _ptr(x), _ptr(w_hwio), _ptr(prepared),
                                                         _ptr(bias), _ptr(out), xs, ctypes.byref(cd), dt, _stream(x)))
            return out
        _lib.check(fn(_lib.handle(_dev(x)), _ptr(x), _ptr(w_hwio), _ptr(bias), _ptr(out), xs, ctypes.byref(cd), dt,
                      _stream(x)))
    return out


def convlstm_conv_supported(xs_chw, cd, in_bf16, compute_bf16=False):
    """Planner hint: can this convolution (cd.lstm_f set) carry the ConvLSTM2D cell update in its epilogue, given the storage
    of its input (bfloat16, or float32 rounded by the loader)?"""
    dt = _lib.dtype_io(_lib.BF16 if in_bf16 else _lib.F32, _lib.BF16, compute_bf16)
    return bool(_lib.lib.dlwp_convlstm_conv_supported(_lib.handle_or_none(), Shape4(1, int(xs_chw[0]), int(xs_chw[1]), int(xs_chw[2])),
                                                      ctypes.byref(cd), dt))


def convlstm_conv(x, w_hwio, bias, cd, h_out, c_out, z_add=None, c_prev=None, x_channels=None, compute_bf16=False,
                  prepared=None, in_o8=False, out_o8=False):
    """One of the two convolutions of a ConvLSTM2D step with the cell update in its epilogue (dlwp_convlstm_conv_fwd):
    z = conv(x) + bias (+ z_add) is not stored; writes c_out (float32 (n, F, ho, wo)) and channels [cd.out_c_off, +F) of
    h_out.  z_add: bfloat16 (n, 4F, ho, wo) or None; c_prev: float32 or None."""
    _check_f32(w_hwio, bias, c_out, c_prev)
    n, c_total, h, w = x.shape
    cin = int(x_channels) if x_channels is not None else c_total
    f = int(cd.lstm_f)
    if tuple(w_hwio.shape) != (cd.kh, cd.kw, cin, 4 * f):
        raise ValueError('kernel shape %s does not match (kh,kw,cin,4F)=(%d,%d,%d,%d)' % (tuple(w_hwio.shape), cd.kh, cd.kw, cin, 4 * f))
    if cd.in_c_total == 0 and cin != c_total:
        cd.in_c_total = c_total
    xs = Shape4(n, cin, h, w)
    ys = conv_out_shape(xs, cd)
    if tuple(c_out.shape) != (n, f, ys.h, ys.w) or tuple(h_out.shape[2:]) != (ys.h, ys.w) or h_out.shape[0] != n:
        raise ValueError('convlstm_conv: c_out %s / h_out %s do not match (%d, %d, %d, %d)' %
                         (tuple(c_out.shape), tuple(h_out.shape), n, f, ys.h, ys.w))
    if z_add is not None and (z_add.dtype != torch.bfloat16 or tuple(z_add.shape) != (n, 4 * f, ys.h, ys.w)):
        raise ValueError('convlstm_conv: z_add must be bfloat16 (n, 4F, ho, wo)')
    if c_prev is not None and tuple(c_prev.shape) != tuple(c_out.shape):
        raise ValueError('convlstm_conv: c_prev shape')
    # out_o8: h_out AND z_add hold channel octets, c_prev / c_out float32 octets (n, F/8, h, w, 8)
    dt = _lib.dtype_io(_code(x, in_o8), _code(h_out, out_o8), compute_bf16)
    _lib.check(_lib.lib.dlwp_convlstm_conv_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(w_hwio), _ptr(prepared), _ptr(bias),
                                               _ptr(z_add), _ptr(c_prev), _ptr(c_out), _ptr(h_out), xs, ctypes.byref(cd), dt,
                                               _stream(x)))
    return h_out


def _step_args(h_seq, x, cd_h, cd_x, x_channels):
    n, _, hh, ww = h_seq.shape
    f = int(cd_h.lstm_f)
    if x.shape[0] != n or tuple(x.shape[2:]) != (hh, ww):
        raise ValueError('convlstm_step: state %r does not match the h sequence %r' % (tuple(x.shape), tuple(h_seq.shape)))
    if cd_h.in_c_total == 0 or cd_h.out_c_total == 0:
        cd_h.in_c_total = cd_h.out_c_total = h_seq.shape[1]
    if cd_x.in_c_total == 0:
        cd_x.in_c_total = x.shape[1]
    return Shape4(n, f, hh, ww), Shape4(n, int(x_channels), hh, ww), _lib.dtype_io(_lib.BF16_O8, _lib.BF16_O8)


def convlstm_step_supported(xs_h_chw, cd_h, xs_x_chw, cd_x):
    """Planner hint: can ONE launch run this ConvLSTM2D step (recurrent + input convolution + cell update,
    dlwp_convlstm_step_fwd)?  Octet layout only."""
    return bool(_lib.lib.dlwp_convlstm_step_supported(
        _lib.handle_or_none(), Shape4(1, *[int(v) for v in xs_h_chw]), ctypes.byref(cd_h), Shape4(1, *[int(v) for v in xs_x_chw]),
        ctypes.byref(cd_x), _lib.dtype_io(_lib.BF16_O8, _lib.BF16_O8)))


def convlstm_step_prepare(h_seq, x, w_h, w_x, cd_h, cd_x, x_channels):
    """Arranged weights of both kernels for convlstm_step calls of this geometry (dlwp_convlstm_step_prepare)."""
    _check_f32(w_h, w_x)
    xs_h, xs_x, dt = _step_args(h_seq, x, cd_h, cd_x, x_channels)
    hd = _lib.handle(_dev(h_seq))
    nbytes = _lib.lib.dlwp_convlstm_step_prepared_bytes(hd, xs_h, ctypes.byref(cd_h), xs_x, ctypes.byref(cd_x), dt)
    if nbytes == 0:
        raise _lib.DlwpError(_lib.EUNSUPPORTED, 'convlstm_step_prepare: this step has no dual-source instance')
    u = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=h_seq.device)
    _lib.check(_lib.lib.dlwp_convlstm_step_prepare(hd, _ptr(w_h), _ptr(w_x), _ptr(u), xs_h, ctypes.byref(cd_h), xs_x,
                                                   ctypes.byref(cd_x), dt, _stream(h_seq)))
    return u


def convlstm_step(h_seq, x, w_h, w_x, bias, cd_h, cd_x, c_prev, c_out, x_channels, prepared=None):
    """One ConvLSTM2D step t >= 1 in one launch (dlwp_convlstm_step_fwd): h_seq is the bfloat16 h sequence IN OCTETS -- cd_h's
    input window holds h_{t-1}, its output window receives h_t; x the float32 state (cd_x's channel window = x_t); c_prev / c_out
    the float32 cell state in octets."""
    _check_f32(w_h, w_x, bias, c_prev, c_out, x)
    if h_seq.dtype != torch.bfloat16 or not h_seq.is_contiguous():
        raise ValueError('convlstm_step: the h sequence must be a contiguous bfloat16 tensor (octet layout)')
    xs_h, xs_x, dt = _step_args(h_seq, x, cd_h, cd_x, x_channels)
    _lib.check(_lib.lib.dlwp_convlstm_step_fwd(_lib.handle(_dev(h_seq)), _ptr(h_seq), _ptr(x), _ptr(w_h), _ptr(w_x), _ptr(prepared),
                                               _ptr(bias), _ptr(c_prev), _ptr(c_out), _ptr(h_seq), xs_h, ctypes.byref(cd_h), xs_x,
                                               ctypes.byref(cd_x), dt, _stream(h_seq)))
    return h_seq


def maxpool2(x, out=None):
    _check_act(x, out)
    n, c, h, w = x.shape
    y = out if out is not None else torch.empty((n, c, h // 2, w // 2), dtype=x.dtype, device=x.device)
    if y.dtype != x.dtype:
        raise ValueError('maxpool2: input %s and output %s storage differ' % (x.dtype, y.dtype))
    _lib.check(_lib.lib.dlwp_maxpool2_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), Shape4(n, c, h, w), storage_code(x),
                                          _stream(x)))
    return y


def maxpool2_bwd(x, dy):
    _check_f32(x, dy)
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    _lib.check(_lib.lib.dlwp_maxpool2_bwd(_lib.handle(_dev(x)), _ptr(x), _ptr(dy), _ptr(dx), Shape4(n, c, h, w),
                                          _lib.F32, _stream(x)))
    return dx


def avgpool2(x, out=None):
    """keras AveragePooling2D(2): ((a + b) + (c + d)) * 0.25 per 2x2 window, float32 or bfloat16 storage (dlwp_avgpool2_fwd)."""
    _check_act(x, out)
    n, c, h, w = x.shape
    y = out if out is not None else torch.empty((n, c, h // 2, w // 2), dtype=x.dtype, device=x.device)
    if y.dtype != x.dtype:
        raise ValueError('avgpool2: input %s and output %s storage differ' % (x.dtype, y.dtype))
    if y.numel() != n * c * (h // 2) * (w // 2):
        raise ValueError('avgpool2: output %r for an input %r' % (tuple(y.shape), tuple(x.shape)))
    _lib.check(_lib.lib.dlwp_avgpool2_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), Shape4(n, c, h, w), storage_code(x),
                                          _stream(x)))
    return y


def avgpool2_bwd(dy, shape, out=None):
    """dx of the given (n, c, h, w) shape from dy (n, c, h//2, w//2): every element written, an odd last row / column +0."""
    _check_f32(dy, out)
    n, c, h, w = (int(v) for v in shape)
    if dy.numel() != n * c * (h // 2) * (w // 2) or (out is not None and out.numel() != n * c * h * w):
        raise ValueError('avgpool2_bwd: gradient %r for an input %r' % (tuple(dy.shape), (n, c, h, w)))
    dx = out if out is not None else torch.empty((n, c, h, w), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.lib.dlwp_avgpool2_bwd(_lib.handle(_dev(dy)), _ptr(dy), _ptr(dx), Shape4(n, c, h, w), _lib.F32,
                                          _stream(dy)))
    return dx


def upsample2(x, out=None):
    _check_f32(x)
    n, c, h, w = x.shape
    y = out if out is not None else torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib.dlwp_upsample2_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), Shape4(n, c, h, w), _lib.F32,
                                           _stream(x)))
    return y


def upsample2_bwd(dy):
    _check_f32(dy)
    n, c, h2, w2 = dy.shape
    dx = torch.empty((n, c, h2 // 2, w2 // 2), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.lib.dlwp_upsample2_bwd(_lib.handle(_dev(dy)), _ptr(dy), _ptr(dx), Shape4(n, c, h2 // 2, w2 // 2),
                                           _lib.F32, _stream(dy)))
    return dx


def upsample2_bilinear(x, out=None):
    """keras UpSampling2D(2, interpolation='bilinear'): even outputs copy x, odd ones are a + (b - a) * 0.5 of two neighbours
    (the last clamped), rows then columns; float32 or bfloat16 storage (dlwp_upsample2_bilinear_fwd)."""
    _check_act(x, out)
    n, c, h, w = x.shape
    y = out if out is not None else torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    if y.dtype != x.dtype:
        raise ValueError('upsample2_bilinear: input %s and output %s storage differ' % (x.dtype, y.dtype))
    if y.numel() != n * c * 2 * h * 2 * w:
        raise ValueError('upsample2_bilinear: output %r for an input %r' % (tuple(y.shape), tuple(x.shape)))
    _lib.check(_lib.lib.dlwp_upsample2_bilinear_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), Shape4(n, c, h, w), storage_code(x),
                                                    _stream(x)))
    return y


def upsample2_bilinear_bwd(dy, shape, out=None):
    """dx of the given (n, c, h, w) shape from dy (n, c, 2h, 2w): the adjoint in gather form, every element written once."""
    _check_f32(dy, out)
    n, c, h, w = (int(v) for v in shape)
    if dy.numel() != n * c * 2 * h * 2 * w or (out is not None and out.numel() != n * c * h * w):
        raise ValueError('upsample2_bilinear_bwd: gradient %r for an input %r' % (tuple(dy.shape), (n, c, h, w)))
    dx = out if out is not None else torch.empty((n, c, h, w), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.lib.dlwp_upsample2_bilinear_bwd(_lib.handle(_dev(dy)), _ptr(dy), _ptr(dx), Shape4(n, c, h, w), _lib.F32,
                                                    _stream(dy)))
    return dx


def copy_channels(src, dst, c, src_c_off=0, dst_c_off=0):
    _check_f32(src, dst)
    n, sc, h, w = src.shape
    _lib.check(_lib.lib.dlwp_copy_channels(_lib.handle(_dev(src)), _ptr(src), _ptr(dst), n, int(c), h * w,
                                           int(src_c_off), sc, int(dst_c_off), dst.shape[1], _lib.F32, _stream(src)))
    return dst


REC_HARD_SIGMOID, REC_SIGMOID = 0, 1


def convlstm_gates(zx, zh, c_prev, c_out, h_out, f, h_c_off=0, act=1, rec_act=REC_HARD_SIGMOID):
    """ConvLSTM2D cell update: zx/zh (n, 4F, h, w) gate pre-activations (zh, c_prev may be None on the first step),
    c_out (n, F, h, w), h written to channels [h_c_off, +F) of h_out (n, h_c_total, h, w); h_out and zx / zh (both the
    same type) may be bfloat16 tensors (config 4 storage), the cell state is float32."""
    _check_f32(c_out)
    for t in (h_out, zx):
        if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous():
            raise ValueError('convlstm_gates: zx / h_out must be contiguous float32 or bfloat16 tensors')
    n, f4, h, w = zx.shape
    if f4 != 4 * f or tuple(c_out.shape) != (n, f, h, w) or tuple(h_out.shape[2:]) != (h, w) or h_out.shape[0] != n:
        raise ValueError('convlstm_gates: inconsistent shapes zx %r c_out %r h_out %r (F=%d)' %
                         (tuple(zx.shape), tuple(c_out.shape), tuple(h_out.shape), f))
    if c_prev is not None:
        _check_f32(c_prev)
    if zh is not None and (zh.dtype != zx.dtype or not zh.is_contiguous()):
        raise ValueError('convlstm_gates: zh must be stored like zx')
    nul = ctypes.c_void_p(0)
    _lib.check(_lib.lib.dlwp_convlstm_gates(_lib.handle(_dev(zx)), _ptr(zx), _ptr(zh) if zh is not None else nul,
                                            _ptr(c_prev) if c_prev is not None else nul, _ptr(c_out), _ptr(h_out), n,
                                            int(f), h * w, int(h_c_off), h_out.shape[1], int(act), int(rec_act),
                                            _lib.dtype_io(storage_code(zx), storage_code(h_out)), _stream(zx)))
    return h_out


def convlstm_gates_bwd(zx, zh, c_prev, c, dh, dc_in, f, h_c_off=0, act=1, rec_act=REC_HARD_SIGMOID, want_dc_prev=True):
    """Backward of convlstm_gates: returns (dz (n, 4F, h, w), dc_prev | None)."""
    _check_f32(zx, c, dh)
    n, f4, h, w = zx.shape
    dz = torch.empty_like(zx)
    dcp = torch.empty_like(c) if (c_prev is not None and want_dc_prev) else None
    _lib.check(_lib.lib.dlwp_convlstm_gates_bwd(_lib.handle(_dev(zx)), _ptr(zx), _ptr(zh), _ptr(c_prev), _ptr(c), _ptr(dh),
                                                _ptr(dc_in), _ptr(dz), _ptr(dcp), n, int(f), h * w, int(h_c_off),
                                                dh.shape[1], int(act), int(rec_act), _lib.F32, _stream(zx)))
    return dz, dcp


def series_merge_time(series, time_dim):
    """(T, N, time_dim*V, ...) -> (T*time_dim, N, V, ...)  -- DLWP/model/models.py:294-300."""
    _check_f32(series)
    t, n, c = series.shape[:3]
    v = c // time_dim
    rest = tuple(series.shape[3:])
    hw = 1
    for d in rest:
        hw *= d
    out = torch.empty((t * time_dim, n, v) + rest, dtype=series.dtype, device=series.device)
    _lib.check(_lib.lib.dlwp_series_merge_time(_lib.handle(_dev(series)), _ptr(series), _ptr(out), t, n, time_dim, v,
                                               hw, _lib.F32, _stream(series)))
    return out


def make_feedback(rows, state_c, out_c, hw, src, shift=0, tail=0, sol=None, sol_planes=0):
    """dlwp_feedback (include/dlwp_hip.h): src[c] >= 0 -> channel of the old state (row i + shift); -1 - j -> channel j of the
    model output of row i; sol[c] >= 0 -> plane of the tail rows' insolation block."""
    if state_c > _lib.FB_MAX_CHANNELS:
        raise ValueError('a fed rollout carries at most %d state channels, got %d' % (_lib.FB_MAX_CHANNELS, state_c))
    fb = _lib.Feedback()
    fb.rows, fb.state_c, fb.out_c, fb.hw = int(rows), int(state_c), int(out_c), int(hw)
    fb.shift, fb.tail, fb.sol_planes = int(shift), int(min(tail, rows)), int(sol_planes)
    for c in range(state_c):
        fb.src[c] = int(src[c])
        fb.sol[c] = int(sol[c]) if sol is not None else -1
    return fb


def state_feedback(old_state, out, fb, sol=None, mean=None, new_state=None):
    """The next input state of a forecast whose inputs and outputs differ (TimeSeriesEstimator.predict,
    DLWP/model/extensions.py:206-240; models.py:280-290): one launch, planes copied bit for bit.  old_state (rows, state_c, h, w),
    out (rows, out_c, h, w), sol (tail, sol_planes, h, w) | None, mean (state_c, h, w) | None."""
    _check_f32(old_state, out, sol, mean)
    if new_state is None:
        new_state = torch.empty_like(old_state)
    _check_f32(new_state)
    if old_state.numel() != fb.rows * fb.state_c * fb.hw or out.numel() != fb.rows * fb.out_c * fb.hw or \
            new_state.numel() != old_state.numel():
        raise ValueError('state_feedback: tensors of %d / %d elements for %d rows of %d -> %d channels x %d' %
                         (old_state.numel(), out.numel(), fb.rows, fb.state_c, fb.out_c, fb.hw))
    if sol is not None and sol.numel() != fb.tail * fb.sol_planes * fb.hw:
        raise ValueError('state_feedback: insolation block of %d elements, %d x %d x %d expected' %
                         (sol.numel(), fb.tail, fb.sol_planes, fb.hw))
    if mean is not None and mean.numel() != fb.state_c * fb.hw:
        raise ValueError('state_feedback: mean state of %d elements, %d x %d expected' % (mean.numel(), fb.state_c, fb.hw))
    _lib.check(_lib.lib.dlwp_state_feedback(_lib.handle(_dev(old_state)), _ptr(old_state), _ptr(out), _ptr(new_state), _ptr(sol),
                                            _ptr(mean), ctypes.byref(fb), _lib.F32, _stream(old_state)))
    return new_state


def conv_configs():
    """[(ks, dil, th, tw, waves, frags_per_wave, cout_frags, channel_chunk, pooled_loader, lds_bytes, flags)] of the
    compiled MFMA tiles (flags bit 0: position-split Winograd instance, dlwp_conv2d_config_flags)."""
    out = []
    info = (ctypes.c_int * 9)()
    lds = ctypes.c_int()
    for i in range(_lib.lib.dlwp_conv2d_num_configs()):
        _lib.check(_lib.lib.dlwp_conv2d_config_info(i, info, ctypes.byref(lds)))
        out.append(tuple(info) + (lds.value, int(_lib.lib.dlwp_conv2d_config_flags(i))))
    return out


def conv_launch_info(x_shape, cd, dtype=None, device_index=0):
    """What conv2d on a stored input of shape (n, cin, h, w) launches: [(config index, grid, block threads, executed
    matrix-core FLOPs, on the bf16 matrix cores?, input loader of a Winograd 8 x 32 launch: 0 elements / 1 column pairs / 2 source
    resolution)], one entry per kernel launch (dlwp_conv2d_launch_info)."""
    out = (_lib.LaunchInfo * 2)()
    n = ctypes.c_int(0)
    with few_wino_scope_of(cd, device_index):
        _lib.check(_lib.lib.dlwp_conv2d_launch_info(_lib.handle(device_index), Shape4(*[int(v) for v in x_shape]),
                                                    ctypes.byref(cd), _lib.F32 if dtype is None else int(dtype), out,
                                                    ctypes.byref(n)))
    return [(o.config, o.grid, o.block_threads, o.matrix_flops, bool(o.bf16_matrix), int(o.x_loader)) for o in out[:n.value]]


def force_conv_config(i):
    _lib.set_option(_lib.OPT_FORCE_CONV_CONFIG, int(i))


def set_few_stream(mode):
    """DLWP_OPT_FEW_STREAM: the streaming kernel for pooled 3x3 layers of at most four input channels (csrc/conv_fwd_few.hip):
    0 never, 1 from 8 tiles per workgroup on (default), 2 whenever the layer qualifies.  Returns the previous setting."""
    return int(_lib.set_option(_lib.OPT_FEW_STREAM, int(mode)))


def set_few_wino(mode, device_index=None):
    """DLWP_OPT_FEW_WINO: the pooled dilation-2 first layer (3x3, at most four input channels, whole 32-channel tiles, float32) on
    Winograd multiplies (csrc/conv_fwd_few_wino.hip, launch-info config -5): 0 (default on a handle) keeps the direct family's
    kernel and bits, 1 takes the kernel at every batch size.  Returns the previous setting."""
    return int(_lib.set_option(_lib.OPT_FEW_WINO, int(mode), device_index))


def few_wino_qualifies(cin, cd, in_bf16=False, out_bf16=False):
    """Host restatement of dlwp_conv_few_wino_covers' geometry part: does DLWP_OPT_FEW_WINO = 1 change how a convolution with
    descriptor `cd` on `cin` stored input channels runs?  (The library has the last word: map sizes past its 32-bit offsets, odd
    pooled widths.)"""
    return bool(cd.kh == 3 and cd.kw == 3 and cd.dil_h == 2 and cd.dil_w == 2 and 1 <= int(cin) <= 4 and cd.cout % 32 == 0 and
                cd.out_pool == 1 and cd.src_mode == _lib.SRC_DIRECT and not cd.out_d2s and not cd.lstm_f and
                not in_bf16 and not out_bf16)


class few_wino_scope(object):
    """`with few_wino_scope(on, device_index):` -- DLWP_OPT_FEW_WINO = 1 on that device's handle (default: the current device) for
    the launches (or the graph capture) inside, the previous setting afterwards; on = False: nothing changes."""

    def __init__(self, on, device_index=None):
        self.on, self.dev, self.prev = bool(on), device_index, None

    def __enter__(self):
        if self.on:
            self.prev = set_few_wino(1, self.dev)
        return self

    def __exit__(self, *exc):
        if self.on:
            set_few_wino(self.prev, self.dev)
        return False


def few_wino_scope_of(cd, device_index=None):
    """The scope of a launch with descriptor `cd`: on for the descriptor an inference Executor marked (its plan's first
    convolution, `cd.few_wino`), so that the layer runs -- and is timed and described -- as in that executor's rollout."""
    return few_wino_scope(getattr(cd, 'few_wino', False), device_index)


def set_wino_xloader(mask):
    """DLWP_OPT_WINO_XLOADER: which input loaders the Winograd 8 x 32 instances may take -- bit 0 image-aligned column pairs, bit 1 an
    up-sampled source at source resolution, bit 2 edge pairs (the half-used last tile row's blocks take two column tiles each);
    7 = all (default), 0 = as before r5.  The same bits whatever the setting.  Returns
    the previous setting."""
    return int(_lib.set_option(_lib.OPT_WINO_XLOADER, int(mask)))


def set_wino_flat(mode):
    """DLWP_OPT_WINO_FLAT: 3x3 float32 Winograd layers of narrow maps run on runs of 64 consecutive tiles (csrc/conv_fwd_wino_flat.hip,
    launch-info config -4): 0 never, 1 from one workgroup per CU on (default), 2 whenever the layer qualifies.  The same bits
    whatever the setting.  Returns the previous setting."""
    return int(_lib.set_option(_lib.OPT_WINO_FLAT, int(mode)))


def set_splitk(mode):
    """DLWP_OPT_SPLITK: Winograd launches on small grids divide the input channels over several workgroups per output tile, the
    last arrival sums the partial tiles in index order (csrc/conv_fwd_k3d1s.hip): 0 never (default since r5), 1 by the library's rule,
    k >= 2 that many wherever the layer is eligible.  Returns the previous setting."""
    return int(_lib.set_option(_lib.OPT_SPLITK, int(mode)))


def conv_split_count(x_shape, cd, dtype=None, device_index=0):
    """The split regime of conv2d on a stored input of shape (n, cin, h, w): workgroups per output tile, 1 = unsplit
    (dlwp_conv2d_split_count).  Equal counts -> equal bits for a sample; across counts float32 round-off."""
    return int(_lib.lib.dlwp_conv2d_split_count(_lib.handle(device_index), Shape4(*[int(v) for v in x_shape]), ctypes.byref(cd),
                                                _lib.F32 if dtype is None else int(dtype)))


def prefers_unfused_pool(cin, cout, kh, kw, dil_h, dil_w):
    """Planner hint: materialise a MaxPooling2D in front of this convolution instead of fusing it into the loader?"""
    return bool(_lib.lib.dlwp_conv2d_prefers_unfused_pool(_lib.handle_or_none(), cin, cout, kh, kw, dil_h, dil_w))


def set_winograd(enable):
    """3x3 convolutions with >= 16 input and output channels run as Winograd F(2x2,3x3) by default."""
    _lib.set_option(_lib.OPT_WINOGRAD, 1 if enable else 0)


def set_bf16_mfma(enable):
    """Convolutions whose input is stored as bfloat16 multiply on the bf16 matrix cores (weights rounded to bf16) by
    default; False keeps them on the fp32 families.  Returns the previous setting."""
    return bool(_lib.set_option(_lib.OPT_BF16_MFMA, 1 if enable else 0))


phase_geometry = _phase_geometry    # (k, pad) -> (k2, lo, hi): the planner's formula (plan.py imports without the library)


def phase_weights(w_hwio, bias, pad_top, pad_left, w2=None, b2=None):
    """Kernels of a Conv2D on a 2x up-sampled tensor restated on the tensor itself: (kh2, kw2, cin, 4*cout) with column
    (2a + b)*cout + co for output phase (a, b), and the bias repeated per phase (include/dlwp_hip.h: dlwp_phase_weights)."""
    _check_f32(w_hwio, bias)
    kh, kw, cin, cout = w_hwio.shape
    kh2, kw2 = phase_geometry(kh, pad_top)[0], phase_geometry(kw, pad_left)[0]
    if w2 is None:
        w2 = torch.empty((kh2, kw2, cin, 4 * cout), dtype=torch.float32, device=w_hwio.device)
    if b2 is None and bias is not None:
        b2 = torch.empty(4 * cout, dtype=torch.float32, device=w_hwio.device)
    _lib.check(_lib.lib.dlwp_phase_weights(_lib.handle(_dev(w_hwio)), _ptr(w_hwio), _ptr(bias), _ptr(w2), _ptr(b2), kh, kw,
                                           cin, cout, int(pad_top), int(pad_left), _lib.F32, _stream(w_hwio)))
    return w2, b2


def depth_to_space2(src, f, out=None, c_off=0):
    """(n, 4F, h, w) phase-major -> (n, F, 2h, 2w): out[:, c_off + co, 2i + a, 2j + b] = src[:, (2a + b)*F + co, i, j]."""
    _check_f32(src)
    n, c4, h, w = src.shape
    if c4 != 4 * f:
        raise ValueError('depth_to_space2: %d channels is not 4 x %d' % (c4, f))
    if out is None:
        out = torch.empty((n, f, 2 * h, 2 * w), dtype=torch.float32, device=src.device)
    _check_f32(out)
    if tuple(out.shape[2:]) != (2 * h, 2 * w) or out.shape[0] != n:
        raise ValueError('depth_to_space2: output shape %r' % (tuple(out.shape),))
    _lib.check(_lib.lib.dlwp_depth_to_space2(_lib.handle(_dev(src)), _ptr(src), _ptr(out), n, int(f), h, w, int(c_off),
                                             out.shape[1], _lib.F32, _stream(src)))
    return out


def space_to_depth2(src, f, c_off=0):
    """(n, c_total, 2h, 2w)[c_off:+f] -> (n, 4f, h, w) phase-major: the adjoint (= inverse) of depth_to_space2."""
    _check_f32(src)
    n, c_total, h2, w2 = src.shape
    out = torch.empty((n, 4 * f, h2 // 2, w2 // 2), dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib.dlwp_space_to_depth2(_lib.handle(_dev(src)), _ptr(src), _ptr(out), n, int(f), h2 // 2, w2 // 2,
                                             int(c_off), c_total, _lib.F32, _stream(src)))
    return out


def phase_weights_bwd(dw2, db2, dw, db, pad_top, pad_left, accumulate=False):
    """Adjoint of phase_weights: dw (kh,kw,cin,cout) (+)= gather of dw2 over the 4 phases; db (+)= fold of db2."""
    _check_f32(dw2, dw, db2, db)
    kh, kw, cin, cout = dw.shape
    _lib.check(_lib.lib.dlwp_phase_weights_bwd(_lib.handle(_dev(dw2)), _ptr(dw2), _ptr(db2), _ptr(dw), _ptr(db), kh, kw, cin,
                                               cout, int(pad_top), int(pad_left), 1 if accumulate else 0, _lib.F32,
                                               _stream(dw2)))
    return dw


def tconv_geometry(k, padding, length):
    """(T, crop, out_len) of one axis of Conv2DTranspose(k, strides=2, padding): T = ceil(k / 2) taps on the source, the output's
    offset in the interleaved phase tensor (2 (length + T - 1) long) and the output length (include/dlwp_hip.h:
    dlwp_tconv_geometry; host only)."""
    t, crop, out = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.dlwp_tconv_geometry(int(k), 1 if padding == 'same' else 0, int(length), ctypes.byref(t),
                                            ctypes.byref(crop), ctypes.byref(out)))
    return t.value, crop.value, out.value


def tconv_weights(k_hwoi, bias, w2=None, b2=None, taps=None):
    """Kernels of a Conv2DTranspose(strides=2) restated as a stride-1 convolution with 4 F phase channels: K (kh, kw, F, cin) ->
    w2 (sh, sw, cin, 4F), and the bias once per phase (include/dlwp_hip.h: dlwp_tconv_weights).  taps = (sh, sw) >= (Th, Tw): the
    stored taps (those of w2 when it is given, else Th x Tw), the Th x Tw block at ((sh - Th) // 2, (sw - Tw) // 2)."""
    _check_f32(k_hwoi, bias, w2, b2)
    kh, kw, f, cin = k_hwoi.shape
    sh, sw = taps if taps is not None else (tuple(w2.shape[:2]) if w2 is not None else ((kh + 1) // 2, (kw + 1) // 2))
    if w2 is None:
        w2 = torch.empty((sh, sw, cin, 4 * f), dtype=torch.float32, device=k_hwoi.device)
    if b2 is None and bias is not None:
        b2 = torch.empty(4 * f, dtype=torch.float32, device=k_hwoi.device)
    if tuple(w2.shape) != (sh, sw, cin, 4 * f) or (b2 is not None and b2.numel() != 4 * f):
        raise ValueError('tconv_weights: derived kernel %r does not belong to a kernel %r' % (tuple(w2.shape), tuple(k_hwoi.shape)))
    _lib.check(_lib.lib.dlwp_tconv_weights(_lib.handle(_dev(k_hwoi)), _ptr(k_hwoi), _ptr(bias), _ptr(w2), _ptr(b2), kh, kw, cin, f,
                                           int(sh), int(sw), _lib.F32, _stream(k_hwoi)))
    return w2, b2


def tconv_weights_bwd(dw2, dk, accumulate=False):
    """Adjoint of tconv_weights: dk (kh, kw, F, cin) (+)= the gather of dw2 (sh, sw, cin, 4F)."""
    _check_f32(dw2, dk)
    kh, kw, f, cin = dk.shape
    sh, sw = int(dw2.shape[0]), int(dw2.shape[1])
    if dw2.dim() != 4 or tuple(dw2.shape[2:]) != (cin, 4 * f) or sh < (kh + 1) // 2 or sw < (kw + 1) // 2:
        raise ValueError('tconv_weights_bwd: derived gradient %r does not belong to a kernel %r' % (tuple(dw2.shape), tuple(dk.shape)))
    _lib.check(_lib.lib.dlwp_tconv_weights_bwd(_lib.handle(_dev(dw2)), _ptr(dw2), _ptr(dk), kh, kw, cin, f, sh, sw,
                                               1 if accumulate else 0, _lib.F32, _stream(dw2)))
    return dk


def depth_to_space2_crop(src, f, top, left, out_h, out_w, out=None, c_off=0):
    """(n, 4F, hp, wp) phase-major -> (n, F, out_h, out_w): rows [top, top + out_h) and columns [left, left + out_w) of the
    depth-to-space image, out[:, c_off + co, r, s] = src[:, (2((r+top)&1) + ((s+left)&1))*F + co, (r+top)>>1, (s+left)>>1]."""
    _check_f32(src, out)
    n, c4, hp, wp = src.shape
    if c4 != 4 * f:
        raise ValueError('depth_to_space2_crop: %d channels is not 4 x %d' % (c4, f))
    if out is None:
        out = torch.empty((n, f, int(out_h), int(out_w)), dtype=torch.float32, device=src.device)
    if tuple(out.shape[2:]) != (int(out_h), int(out_w)) or out.shape[0] != n:
        raise ValueError('depth_to_space2_crop: output shape %r' % (tuple(out.shape),))
    _lib.check(_lib.lib.dlwp_depth_to_space2_crop(_lib.handle(_dev(src)), _ptr(src), _ptr(out), n, int(f), hp, wp, int(top),
                                                  int(left), int(out_h), int(out_w), int(c_off), out.shape[1], _lib.F32,
                                                  _stream(src)))
    return out


def space_to_depth2_fill(src, f, hp, wp, top, left, c_off=0, out=None):
    """Adjoint of depth_to_space2_crop: (n, c_total, H, W)[c_off:+f] -> (n, 4f, hp, wp) phase-major; every element is written,
    +0 where the crop dropped the pixel."""
    _check_f32(src, out)
    n, c_total, hh, ww = src.shape
    if out is None:
        out = torch.empty((n, 4 * f, int(hp), int(wp)), dtype=torch.float32, device=src.device)
    if tuple(out.shape) != (n, 4 * f, int(hp), int(wp)):
        raise ValueError('space_to_depth2_fill: output shape %r' % (tuple(out.shape),))
    _lib.check(_lib.lib.dlwp_space_to_depth2_fill(_lib.handle(_dev(src)), _ptr(src), _ptr(out), n, int(f), int(hp), int(wp),
                                                  int(top), int(left), hh, ww, int(c_off), c_total, _lib.F32, _stream(src)))
    return out


def crop2d(x, crop, out=None):
    """keras Cropping2D on NCHW: the adjoint of zero padding (dlwp_pad2d_bwd with PAD_ZERO: 'zero drops').  crop: a Pad2d."""
    _check_f32(x, out)
    n, c, h, w = x.shape
    ho, wo = h - crop.top - crop.bottom, w - crop.left - crop.right
    if ho <= 0 or wo <= 0:
        raise ValueError('crop2d: nothing is left of %d x %d' % (h, w))
    y = out if out is not None else torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.dlwp_pad2d_bwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), n * c, ho, wo, 1, crop, _lib.F32, _stream(x)))
    return y


def sconv_geometry(k, padding, length):
    """(T, pad_lo, pad_hi, out_len) of one axis of Conv2D(k, strides=2, padding): T = ceil(k / 2) taps on the space-to-depth image,
    the layer's own zero padding (TensorFlow's 'same' rule for stride 2) and the output length (include/dlwp_hip.h:
    dlwp_sconv_geometry; host only).  ValueError where a 'valid' kernel does not fit."""
    t, lo, hi, out = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib.dlwp_sconv_geometry(int(k), 1 if padding == 'same' else 0, int(length), ctypes.byref(t), ctypes.byref(lo),
                                      ctypes.byref(hi), ctypes.byref(out))
    if rc != 0:
        raise ValueError(_lib.lib.dlwp_last_error().decode())
    return t.value, lo.value, hi.value, out.value


def sconv_weights(k_hwio, w2=None, taps=None):
    """Kernel of a Conv2D(strides=2) restated as a stride-1 convolution on the space-to-depth image of its input: K (kh, kw, cin, F)
    -> w2 (sh, sw, 4 cin, F) (include/dlwp_hip.h: dlwp_sconv_weights).  taps = (sh, sw) >= (Th, Tw): the stored taps (those of w2
    when it is given, else Th x Tw), the Th x Tw block at (0, 0)."""
    _check_f32(k_hwio, w2)
    kh, kw, cin, f = k_hwio.shape
    sh, sw = taps if taps is not None else (tuple(w2.shape[:2]) if w2 is not None else ((kh + 1) // 2, (kw + 1) // 2))
    if w2 is None:
        w2 = torch.empty((sh, sw, 4 * cin, f), dtype=torch.float32, device=k_hwio.device)
    if tuple(w2.shape) != (sh, sw, 4 * cin, f):
        raise ValueError('sconv_weights: derived kernel %r does not belong to a kernel %r' % (tuple(w2.shape), tuple(k_hwio.shape)))
    _lib.check(_lib.lib.dlwp_sconv_weights(_lib.handle(_dev(k_hwio)), _ptr(k_hwio), _ptr(w2), kh, kw, cin, f, int(sh), int(sw),
                                           _lib.F32, _stream(k_hwio)))
    return w2


def sconv_weights_bwd(dw2, dk, accumulate=False):
    """Adjoint of sconv_weights: dk (kh, kw, cin, F) (+)= the gather of dw2 (sh, sw, 4 cin, F)."""
    _check_f32(dw2, dk)
    kh, kw, cin, f = dk.shape
    sh, sw = int(dw2.shape[0]), int(dw2.shape[1])
    if dw2.dim() != 4 or tuple(dw2.shape[2:]) != (4 * cin, f) or sh < (kh + 1) // 2 or sw < (kw + 1) // 2:
        raise ValueError('sconv_weights_bwd: derived gradient %r does not belong to a kernel %r' % (tuple(dw2.shape), tuple(dk.shape)))
    _lib.check(_lib.lib.dlwp_sconv_weights_bwd(_lib.handle(_dev(dw2)), _ptr(dw2), _ptr(dk), kh, kw, cin, f, sh, sw,
                                               1 if accumulate else 0, _lib.F32, _stream(dw2)))
    return dk


def space_to_depth2_pad(src, c, pad, hp, wp, c_off=0, out=None):
    """(n, c_total, H, W)[c_off:+c] under the halo `pad` (a Pad2d, the five modes per axis) -> (n, 4c, hp, wp) phase-major:
    out[:, (2a+b) c + ch, i, j] = padded[:, ch, 2i+a, 2j+b], +0 beyond the padded image (include/dlwp_hip.h:
    dlwp_space_to_depth2_pad) -- the padding in front of a strided Conv2D, its 'same' zeros and the de-interleave in one pass."""
    _check_f32(src, out)
    n, c_total, hh, ww = src.shape
    if out is None:
        out = torch.empty((n, 4 * int(c), int(hp), int(wp)), dtype=torch.float32, device=src.device)
    if tuple(out.shape) != (n, 4 * int(c), int(hp), int(wp)):
        raise ValueError('space_to_depth2_pad: output shape %r' % (tuple(out.shape),))
    _lib.check(_lib.lib.dlwp_space_to_depth2_pad(_lib.handle(_dev(src)), _ptr(src), _ptr(out), n, int(c), hh, ww, pad, int(hp),
                                                 int(wp), int(c_off), c_total, _lib.F32, _stream(src)))
    return out


def space_to_depth2_pad_bwd(dout, c, in_h, in_w, pad, out=None, c_off=0):
    """Adjoint of space_to_depth2_pad: (n, 4c, hp, wp) -> channels [c_off, +c) of `out` (n, c_total, in_h, in_w) (a new
    (n, c, in_h, in_w) tensor when None).  Every element of the window is written (overwritten, as pad2d_bwd does)."""
    _check_f32(dout, out)
    n, c4, hp, wp = dout.shape
    if c4 != 4 * int(c):
        raise ValueError('space_to_depth2_pad_bwd: %d channels is not 4 x %d' % (c4, c))
    if out is None:
        out = torch.empty((n, int(c), int(in_h), int(in_w)), dtype=torch.float32, device=dout.device)
    if out.shape[0] != n or tuple(out.shape[2:]) != (int(in_h), int(in_w)):
        raise ValueError('space_to_depth2_pad_bwd: output shape %r' % (tuple(out.shape),))
    _lib.check(_lib.lib.dlwp_space_to_depth2_pad_bwd(_lib.handle(_dev(dout)), _ptr(dout), _ptr(out), n, int(c), int(in_h),
                                                     int(in_w), pad, hp, wp, int(c_off), out.shape[1], _lib.F32, _stream(dout)))
    return out


def make_depthwise(kh, kw, dil=1, depth_multiplier=1, halo=None, act=ACT_LINEAR, in_c_off=0, in_c_total=0, out_c_off=0,
                   out_c_total=0):
    """A dlwp_depthwise2d descriptor (include/dlwp_hip.h); channel totals of 0 = the window itself."""
    dh, dw = (dil, dil) if isinstance(dil, int) else dil
    return _lib.Depthwise2d(int(kh), int(kw), int(dh), int(dw), int(depth_multiplier), halo if halo is not None else make_pad(),
                            int(act), int(in_c_off), int(in_c_total), int(out_c_off), int(out_c_total))


def make_pointwise(q, o, act=ACT_LINEAR, in_c_off=0, in_c_total=0, out_c_off=0, out_c_total=0):
    """A dlwp_pointwise2d descriptor (include/dlwp_hip.h); channel totals of 0 = the window itself."""
    return _lib.Pointwise2d(int(q), int(o), int(act), int(in_c_off), int(in_c_total), int(out_c_off), int(out_c_total))


def depthwise_out_shape(xs, d):
    """Shape4 of the output of a depthwise stencil on the input window xs (host only; DlwpError where the descriptor is refused)."""
    ys = Shape4()
    _lib.check(_lib.lib.dlwp_depthwise2d_out_shape(xs, d, ctypes.byref(ys)))
    return ys


def depthwise2d(x, k, bias, d, out=None):
    """keras DepthwiseConv2D forward: channels [d.in_c_off, +cin) of x (n, c_total, h, w) under d.halo, kernel k (kh, kw, cin, dm),
    bias (cin dm) or None -> channels [d.out_c_off, +cin dm) of `out` (a new dense tensor when None).  include/dlwp_hip.h:
    dlwp_depthwise2d_fwd."""
    _check_f32(x, k, bias, out)
    n, c_total, hh, ww = x.shape
    cin = int(k.shape[2])
    xs = Shape4(n, cin, hh, ww)
    d = _lib.Depthwise2d.from_buffer_copy(d)
    d.in_c_total = c_total
    if out is not None:
        d.out_c_total = int(out.shape[1])
    ys = depthwise_out_shape(xs, d)
    if out is None:
        out = torch.empty((n, d.out_c_total if d.out_c_total > 0 else ys.c, ys.h, ys.w), dtype=torch.float32, device=x.device)
    if out.shape[0] != n or tuple(out.shape[2:]) != (ys.h, ys.w):
        raise ValueError('depthwise2d: output shape %r, expected (%d, *, %d, %d)' % (tuple(out.shape), n, ys.h, ys.w))
    _lib.check(_lib.lib.dlwp_depthwise2d_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(k), _ptr(bias), _ptr(out), xs, d, _lib.F32,
                                             _stream(x)))
    return out


def depthwise2d_bwd_data(dz, k, d, in_h, in_w, out=None):
    """Adjoint of depthwise2d in its input, halo included: dz (n, z_total, ho, wo)[d.out_c_off:+cin dm] -> channels
    [d.in_c_off, +cin) of `out` (n, c_total, in_h, in_w) (a new dense tensor when None).  The window is overwritten."""
    _check_f32(dz, k, out)
    n = dz.shape[0]
    cin = int(k.shape[2])
    xs = Shape4(n, cin, int(in_h), int(in_w))
    d = _lib.Depthwise2d.from_buffer_copy(d)
    d.out_c_total = int(dz.shape[1])
    if out is None:
        d.in_c_off, d.in_c_total = 0, cin
        out = torch.empty((n, cin, int(in_h), int(in_w)), dtype=torch.float32, device=dz.device)
    else:
        d.in_c_total = int(out.shape[1])
    ys = depthwise_out_shape(xs, d)
    if out.shape[0] != n or tuple(out.shape[2:]) != (int(in_h), int(in_w)) or tuple(dz.shape[2:]) != (ys.h, ys.w):
        raise ValueError('depthwise2d_bwd_data: gradient %r / output %r do not belong to an input of %d x %d'
                         % (tuple(dz.shape), tuple(out.shape), in_h, in_w))
    _lib.check(_lib.lib.dlwp_depthwise2d_bwd_data(_lib.handle(_dev(dz)), _ptr(dz), _ptr(k), _ptr(out), xs, d, _lib.F32, _stream(dz)))
    return out


def depthwise2d_bwd_weight(x, dz, dk, d, accumulate=False, ws_key=None):
    """dk (kh, kw, cin, dm) (+)= the depthwise kernel's gradient from the layer input x (its window d.in_c_off) and dz (its window
    d.out_c_off): two launches, a fixed tree, the same bits on every run (include/dlwp_hip.h: dlwp_depthwise2d_bwd_weight)."""
    _check_f32(x, dz, dk)
    n, c_total, hh, ww = x.shape
    cin = int(dk.shape[2])
    xs = Shape4(n, cin, hh, ww)
    d = _lib.Depthwise2d.from_buffer_copy(d)
    d.in_c_total, d.out_c_total = c_total, int(dz.shape[1])
    ys = depthwise_out_shape(xs, d)
    if dz.shape[0] != n or tuple(dz.shape[2:]) != (ys.h, ys.w) or tuple(dk.shape) != (d.kh, d.kw, cin, d.depth_multiplier):
        raise ValueError('depthwise2d_bwd_weight: shapes %r, %r, %r do not belong together'
                         % (tuple(x.shape), tuple(dz.shape), tuple(dk.shape)))
    ws = workspace(x.device, _lib.lib.dlwp_depthwise2d_bwd_workspace(xs, d), ('dw_wgrad', ws_key))
    _lib.check(_lib.lib.dlwp_depthwise2d_bwd_weight(_lib.handle(_dev(x)), _ptr(x), _ptr(dz), _ptr(dk), xs, d, _ptr(ws),
                                                    int(bool(accumulate)), _lib.F32, _stream(x)))
    return dk


def pointwise2d(x, w, bias, d, out=None):
    """The 1 x 1 product of a SeparableConv2D on the matrix cores: channels [d.in_c_off, +q) of x (n, c_total, h, w), w (q, o) (or
    keras' (1, 1, q, o)), bias (o) or None -> channels [d.out_c_off, +o) of `out` (a new dense tensor when None)."""
    _check_f32(x, w, bias, out)
    n, c_total, hh, ww = x.shape
    d = _lib.Pointwise2d.from_buffer_copy(d)
    d.in_c_total = c_total
    if w.numel() != d.q * d.o:
        raise ValueError('pointwise2d: kernel %r is not (%d, %d)' % (tuple(w.shape), d.q, d.o))
    if out is None:
        out = torch.empty((n, d.out_c_total if d.out_c_total > 0 else d.o, hh, ww), dtype=torch.float32, device=x.device)
    d.out_c_total = int(out.shape[1])
    if out.shape[0] != n or tuple(out.shape[2:]) != (hh, ww):
        raise ValueError('pointwise2d: output shape %r' % (tuple(out.shape),))
    _lib.check(_lib.lib.dlwp_pointwise2d_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(w), _ptr(bias), _ptr(out), n, hh * ww, d, _lib.F32,
                                             _stream(x)))
    return out


def pointwise2d_bwd_data(dz, w, d, out=None):
    """dx[n][q][p] = sum_o dz[n][o][p] w[q][o]: dz (n, z_total, h, w)[d.out_c_off:+o] -> channels [d.in_c_off, +q) of `out` (a new
    dense tensor when None); the window is overwritten."""
    _check_f32(dz, w, out)
    n, z_total, hh, ww = dz.shape
    d = _lib.Pointwise2d.from_buffer_copy(d)
    d.out_c_total = z_total
    if out is None:
        d.in_c_off, d.in_c_total = 0, d.q
        out = torch.empty((n, d.q, hh, ww), dtype=torch.float32, device=dz.device)
    else:
        d.in_c_total = int(out.shape[1])
    if out.shape[0] != n or tuple(out.shape[2:]) != (hh, ww) or w.numel() != d.q * d.o:
        raise ValueError('pointwise2d_bwd_data: shapes %r, %r, %r' % (tuple(dz.shape), tuple(w.shape), tuple(out.shape)))
    _lib.check(_lib.lib.dlwp_pointwise2d_bwd_data(_lib.handle(_dev(dz)), _ptr(dz), _ptr(w), _ptr(out), n, hh * ww, d, _lib.F32,
                                                  _stream(dz)))
    return out


def pointwise2d_bwd_weight(x, dz, dw, d, accumulate=False, ws_key=None):
    """dw (q, o) (+)= sum over samples and pixels of x[n][q][p] dz[n][o][p]: a fixed split over (sample, pixel) and a deterministic
    final sum (include/dlwp_hip.h: dlwp_pointwise2d_bwd_weight)."""
    _check_f32(x, dz, dw)
    n, c_total, hh, ww = x.shape
    d = _lib.Pointwise2d.from_buffer_copy(d)
    d.in_c_total, d.out_c_total = c_total, int(dz.shape[1])
    if dz.shape[0] != n or tuple(dz.shape[2:]) != (hh, ww) or dw.numel() != d.q * d.o:
        raise ValueError('pointwise2d_bwd_weight: shapes %r, %r, %r' % (tuple(x.shape), tuple(dz.shape), tuple(dw.shape)))
    ws = workspace(x.device, _lib.lib.dlwp_pointwise2d_bwd_workspace(n, hh * ww, d), ('pw_wgrad', ws_key))
    _lib.check(_lib.lib.dlwp_pointwise2d_bwd_weight(_lib.handle(_dev(x)), _ptr(x), _ptr(dz), _ptr(dw), n, hh * ww, d, _ptr(ws),
                                                    int(bool(accumulate)), _lib.F32, _stream(x)))
    return dw


def uses_bf16_weights(xs, cd, dtype):
    """Does conv2d on an input of shape xs = (n, c, h, w) stored as `dtype` (a _lib.dtype_io code) multiply with weights
    rounded to bfloat16 (the bf16 matrix-core kernels)?  Host logic only."""
    return bool(_lib.lib.dlwp_conv2d_uses_bf16_weights(_lib.handle_or_none(), _lib.Shape4(*[int(v) for v in xs]),
                                                       ctypes.byref(cd), int(dtype)))


# ------------------------------------------------------------------------------------------------------------------ #
# training kernels
# ------------------------------------------------------------------------------------------------------------------ #

_workspaces = {}


def workspace(device, nbytes, key=None):
    """A growable per-device scratch allocation (bytes) for the *_bwd / loss kernels.  key: a scratch of its own for this
    caller (a deferred final sum reads its partials at dlwp_reductions_flush: nothing else may write there meanwhile)."""
    key = (device.type, device.index) if key is None else (device.type, device.index, key)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


_workspaces2 = {}


def workspace2(device, nbytes, key=None):
    """A second, small scratch allocation (reduction partials) that may be live next to `workspace`."""
    key = (device.type, device.index) if key is None else (device.type, device.index, key)
    ws = _workspaces2.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
        _workspaces2[key] = ws
    return ws


def conv_bwd_workspace_bytes(dev_index, xs, cd, which):
    out = ctypes.c_size_t()
    _lib.check(_lib.lib.dlwp_conv2d_bwd_workspace(_lib.handle(dev_index), xs, ctypes.byref(cd), int(which),
                                                  ctypes.byref(out)))
    return out.value


def conv2d_bwd_data(dz, w_hwio, cd, xs, dx, prepared=None, stored=False):
    """dz: (n, out_c_total, ho, wo); dx: preallocated gradient buffer (see include/dlwp_hip.h for its layout).
    prepared: the tensor conv2d_bwd_data_prepare built for (w_hwio, xs, cd, stored) -- the gradient's convolution is then the
    only launch; stored: gradient w.r.t. the STORED tensor of an up-sampled source (see conv2d_bwd_data_stored)."""
    _check_f32(dz, w_hwio, dx, prepared)
    d = _dev(dz)
    need = conv_bwd_workspace_bytes(d, xs, cd, 0)
    ws = workspace(dz.device, need)
    if prepared is not None:
        _lib.check(_lib.lib.dlwp_conv2d_bwd_data_prepared(_lib.handle(d), _ptr(dz), _ptr(prepared), _ptr(dx), xs,
                                                          ctypes.byref(cd), _lib.F32, _ptr(ws), ws.numel(),
                                                          1 if stored else 0, _stream(dz)))
        return dx
    fn = _lib.lib.dlwp_conv2d_bwd_data_stored if stored else _lib.lib.dlwp_conv2d_bwd_data
    _lib.check(fn(_lib.handle(d), _ptr(dz), _ptr(w_hwio), _ptr(dx), xs, ctypes.byref(cd), _lib.F32, _ptr(ws), ws.numel(),
                  _stream(dz)))
    return dx


def conv2d_bwd_data_act(dz, w_hwio, cd, xs, dx, x, act_in, db_in=None, prepared=None, ws_key=None):
    """conv2d_bwd_data whose result is multiplied by act'(x) in the store phase -- x: the layer's input = the activation output of
    the layer in front -- with that layer's bias gradient db_in (xs.c floats) from the same pass (dlwp_conv2d_bwd_data_act).
    Returns False, nothing written, where the gradient does not run on the instance with that store phase."""
    _check_f32(dz, w_hwio, dx, x, db_in, prepared)
    d = _dev(dz)
    need = conv_bwd_workspace_bytes(d, xs, cd, 3)
    ws = workspace(dz.device, need, ws_key)
    rc = _lib.lib.dlwp_conv2d_bwd_data_act(_lib.handle(d), _ptr(dz), _ptr(w_hwio), _ptr(prepared), _ptr(dx), xs, ctypes.byref(cd),
                                           _ptr(x), int(act_in), _ptr(db_in), _lib.F32, _ptr(ws), ws.numel(), _stream(dz))
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc)
    return True


def conv2d_bwd_data_prepared_bytes(dev_index, xs, cd, stored=False):
    """Bytes of the prepared operand of a data gradient (0: this gradient has no prepared form, e.g. `stored` on a layer
    without the summing epilogue)."""
    return int(_lib.lib.dlwp_conv2d_bwd_data_prepared_bytes(_lib.handle(dev_index), xs, ctypes.byref(cd), 1 if stored else 0))


def conv2d_bwd_data_prepare(w_hwio, cd, xs, stored=False, out=None):
    """The data gradient's operand from the layer's HWIO kernel (dlwp_conv2d_bwd_data_prepare); between prepare_begin /
    prepare_flush the work is only recorded."""
    _check_f32(w_hwio, out)
    d = _dev(w_hwio)
    nbytes = conv2d_bwd_data_prepared_bytes(d, xs, cd, stored)
    if nbytes == 0:
        return None
    u = out if out is not None else torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=w_hwio.device)
    if u.numel() * 4 < nbytes:
        raise ValueError('conv2d_bwd_data_prepare: the buffer holds %d bytes, %d needed' % (u.numel() * 4, nbytes))
    _lib.check(_lib.lib.dlwp_conv2d_bwd_data_prepare(_lib.handle(d), _ptr(w_hwio), _ptr(u), xs, ctypes.byref(cd),
                                                     1 if stored else 0, _stream(w_hwio)))
    return u


def _dev_index(device):
    return device.index if device.index is not None else torch.cuda.current_device()


def stream_wait(waiter, signaler):
    """`waiter` (a torch.cuda.Stream) waits for everything issued on `signaler` so far -- torch's Stream.wait_stream through the
    library (dlwp_stream_wait), so that a step being recorded (Trainer._record_step) keeps its fork / join edges."""
    dev = waiter.device.index if waiter.device.index is not None else torch.cuda.current_device()
    _lib.check(_lib.lib.dlwp_stream_wait(_lib.handle(dev), ctypes.c_void_p(waiter.cuda_stream), ctypes.c_void_p(signaler.cuda_stream)))


def prepare_begin(device):
    """Weight preparations from now on are recorded and built by ONE launch at prepare_flush (csrc/batch.hip)."""
    _lib.check(_lib.lib.dlwp_prepare_begin(_lib.handle(_dev_index(device))))


def _device_stream(device):
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(_dev_index(device)))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def prepare_flush(device):
    _lib.check(_lib.lib.dlwp_prepare_flush(_lib.handle(_dev_index(device)), _device_stream(device)))


def reductions_begin(device):
    """The final sums of conv2d_bwd_weight / the bias gradients / mse_mae from now on are recorded and done by ONE launch at
    reductions_flush; every such call needs a workspace of its own until then (ws_key)."""
    _lib.check(_lib.lib.dlwp_reductions_begin(_lib.handle(_dev_index(device))))


def reductions_flush(device):
    _lib.check(_lib.lib.dlwp_reductions_flush(_lib.handle(_dev_index(device)), _device_stream(device)))


def pair_begin(device):
    """From now until pair_end ONE conv2d_bwd_weight and ONE conv2d_bwd_data of INDEPENDENT tensors hand their launch over; pair_end
    issues both -- as one grid where a fused instance exists (dlwp_pair_begin / dlwp_pair_end, csrc/conv_pair.hip)."""
    _lib.check(_lib.lib.dlwp_pair_begin(_lib.handle(_dev_index(device))))


def pair_end(device):
    _lib.check(_lib.lib.dlwp_pair_end(_lib.handle(_dev_index(device)), _device_stream(device)))


def pair_fused_count(device):
    """pairs the device's handle has issued as ONE launch so far"""
    return int(_lib.lib.dlwp_pair_fused_count(_lib.handle(_dev_index(device))))


# ---- RowConnected2D (reference DLWP/custom.py:695-896) ------------------------------------------------------------------ #
def rowconv2d(x, kernel, bias, cd, out=None, direct=False, x_channels=None):
    """RowConnected2D.call / row_conv2d, channels_first: x stored (n, in_c_total, h, w); kernel (ho, kh, kw, cin, cout) --
    one filter set per OUTPUT ROW (custom.py:800-805); bias the stored (ho, 1, cout) array or None.  Returns
    (n, out_c_total, ho, wo), channels [out_c_off, +cout) written.  direct=True: the vector-ALU cross-check kernel."""
    _check_f32(x, kernel, bias, out)
    n, c_total, h, w = x.shape
    cin = int(x_channels) if x_channels is not None else c_total
    if cd.in_c_total == 0 and cin != c_total:
        cd.in_c_total = c_total
    xs = Shape4(n, cin, h, w)
    ys = conv_out_shape(xs, cd)
    if tuple(kernel.shape) != (ys.h, cd.kh, cd.kw, cin, cd.cout):
        raise ValueError('kernel shape %s does not match (rows,kh,kw,cin,cout)=%r' %
                         (tuple(kernel.shape), (ys.h, cd.kh, cd.kw, cin, cd.cout)))
    if bias is not None and bias.numel() != ys.h * cd.cout:
        raise ValueError('bias of %d elements, expected (rows, 1, cout) = %d' % (bias.numel(), ys.h * cd.cout))
    oc = cd.out_c_total if cd.out_c_total > 0 else ys.c
    if out is None:
        out = torch.empty((n, oc, ys.h, ys.w), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, oc, ys.h, ys.w):
        raise ValueError('output buffer shape %s != %s' % (tuple(out.shape), (n, oc, ys.h, ys.w)))
    fn = _lib.lib.dlwp_rowconv2d_fwd_direct if direct else _lib.lib.dlwp_rowconv2d_fwd
    _lib.check(fn(_lib.handle(_dev(x)), _ptr(x), _ptr(kernel), _ptr(bias), _ptr(out), xs, ctypes.byref(cd), _lib.F32,
                  _stream(x)))
    return out


def rowconv2d_uses_matrix_cores(xs_nchw, cd, which=0):
    """Host logic: does pass `which` (0 forward, 1 data gradient, 2 weight gradient) of this geometry run on the MFMA kernels?"""
    return bool(_lib.lib.dlwp_rowconv2d_uses_matrix_cores(_lib.handle_or_none(), Shape4(*[int(v) for v in xs_nchw]),
                                                          ctypes.byref(cd), int(which)))


ROWCONV_REASONS = ('', 'kernel height', 'staged width', 'LDS footprint', '32-bit offsets', 'empty batch')


def rowconv2d_launch_info(xs_nchw, cd, which=0):
    """Host logic (no GPU needed): what pass `which` (0 forward, 1 data gradient, 2 weight gradient) of this geometry launches
    (dlwp_rowconv2d_launch_info) -> dict(kind 'mfma' | 'simple', targ (template arguments of the matrix-core instance), grid,
    block, lds, circ, fold, reason (of the vector fall-back, ROWCONV_REASONS), n_cb, n_sg, n_cg, n_mg, samples)."""
    info = _lib.RowconvLaunchInfo()
    _lib.check(_lib.lib.dlwp_rowconv2d_launch_info(_lib.handle_or_none(), Shape4(*[int(v) for v in xs_nchw]), ctypes.byref(cd),
                                                   int(which), ctypes.byref(info)))
    return dict(kind='mfma' if info.kind else 'simple', targ=(info.targ[0], info.targ[1]), grid=info.grid, block=info.block_threads,
                lds=info.lds_bytes, circ=bool(info.circ), fold=bool(info.fold), reason=ROWCONV_REASONS[info.reason], n_cb=info.n_cb,
                n_sg=info.n_sg, n_cg=info.n_cg, n_mg=info.n_mg, samples=info.samples)


def rowconv2d_bwd_data(dz, kernel, cd, xs, dx):
    """dx: dense (n, cin, h, w) <- dL/dx of the row-connected layer (halo adjoint included)."""
    _check_f32(dz, kernel, dx)
    d = _dev(dz)
    need = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dlwp_rowconv2d_bwd_workspace(_lib.handle(d), xs, ctypes.byref(cd), ctypes.byref(need)))
    ws = workspace(dz.device, need.value)
    _lib.check(_lib.lib.dlwp_rowconv2d_bwd_data(_lib.handle(d), _ptr(dz), _ptr(kernel), _ptr(dx), xs, ctypes.byref(cd),
                                                _lib.F32, _ptr(ws), ws.numel(), _stream(dz)))
    return dx


def rowconv2d_bwd_weight(x, dz, dw, db, cd, xs, accumulate=False):
    """dw (rows, kh, kw, cin, cout), db (rows, 1, cout) or None <- gradients of the kernel and the stored bias."""
    _check_f32(x, dz, dw, db)
    _lib.check(_lib.lib.dlwp_rowconv2d_bwd_weight(_lib.handle(_dev(x)), _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), xs,
                                                  ctypes.byref(cd), 1 if accumulate else 0, _lib.F32, _stream(x)))
    return dw


def conv2d_bwd_data_stored(dz, w_hwio, cd, xs, dx):
    """Up-sampled sources: gradient w.r.t. the stored tensor (n, cin, xs.h, xs.w) in one kernel.  Returns False when the
    layer has no kernel with the summing epilogue (nothing was written; use conv2d_bwd_data + upsample2_bwd)."""
    _check_f32(dz, w_hwio, dx)
    d = _dev(dz)
    need = conv_bwd_workspace_bytes(d, xs, cd, 0)
    ws = workspace(dz.device, need)
    rc = _lib.lib.dlwp_conv2d_bwd_data_stored(_lib.handle(d), _ptr(dz), _ptr(w_hwio), _ptr(dx), xs, ctypes.byref(cd),
                                              _lib.F32, _ptr(ws), ws.numel(), _stream(dz))
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc)
    return True


def conv2d_bwd_weight(x, dz, dw, cd, xs, accumulate=False, ws_key=None):
    _check_f32(x, dz, dw)
    d = _dev(x)
    need = conv_bwd_workspace_bytes(d, xs, cd, 1)
    ws = workspace(x.device, need, ws_key)
    _lib.check(_lib.lib.dlwp_conv2d_bwd_weight(_lib.handle(d), _ptr(x), _ptr(dz), _ptr(dw), xs, ctypes.byref(cd),
                                               int(bool(accumulate)), _lib.F32, _ptr(ws), ws.numel(), _stream(x)))
    return dw


def conv2d_bwd_weight_pooled_supported(xs, cd, dev_index=None):
    """Can dlwp_conv2d_bwd_weight_pooled take this layer (3x3, at most 4 input channels)?"""
    out = ctypes.c_size_t()
    d = torch.cuda.current_device() if dev_index is None else dev_index
    return _lib.lib.dlwp_conv2d_bwd_workspace(_lib.handle(d), xs, ctypes.byref(cd), 2, ctypes.byref(out)) == _lib.OK


def conv2d_bwd_weight_pooled(x, y, dpool, dw, db, cd, xs, act, accumulate=False, ws_key=None):
    """dw (and db, unless None) of a layer whose only reader is MaxPooling2D(2) and whose data gradient nobody needs, from its
    output y and the pooled tensor's gradient dpool (n, cout, ho/2, wo/2): the gradient tensor in between is never stored
    (include/dlwp_hip.h: dlwp_conv2d_bwd_weight_pooled)."""
    _check_f32(x, y, dpool, dw, db)
    n, cout, hp, wp = dpool.shape
    if cout != cd.cout or not dpool.is_contiguous() or (hp, wp) != (y.shape[2] // 2, y.shape[3] // 2):
        raise ValueError('conv2d_bwd_weight_pooled: pooled gradient %r does not match the layer output %r' %
                         (tuple(dpool.shape), tuple(y.shape)))
    d = _dev(x)
    need = conv_bwd_workspace_bytes(d, xs, cd, 2)
    ws = workspace(x.device, need, ws_key)
    _lib.check(_lib.lib.dlwp_conv2d_bwd_weight_pooled(_lib.handle(d), _ptr(x), _ptr(y), _ptr(dpool), _ptr(dw), _ptr(db), xs,
                                                     ctypes.byref(cd), int(act), int(bool(accumulate)), _lib.F32, _ptr(ws),
                                                     ws.numel(), _stream(x)))
    return dw


def act_bwd(y, dy, act, out=None):
    _check_f32(y, dy)
    dz = out if out is not None else torch.empty_like(dy)
    if dy.numel() == 0:     # (an empty tensor has no address for the C ABI to check)
        return dz
    _lib.check(_lib.lib.dlwp_act_bwd(_lib.handle(_dev(dy)), _ptr(y), _ptr(dy), _ptr(dz), dy.numel(), int(act), _lib.F32,
                                     _stream(dy)))
    return dz


def bias_grad(dz, db, c, c_off=0, ws_key=None):
    _check_f32(dz, db)
    n, c_total, h, w = dz.shape
    if dz.numel() == 0:     # the sum of nothing
        return db.zero_()
    ws = workspace2(dz.device, _lib.lib.dlwp_bias_grad_workspace(int(c)), ws_key)
    _lib.check(_lib.lib.dlwp_bias_grad(_lib.handle(_dev(dz)), _ptr(dz), _ptr(db), n, int(c), int(c_off), c_total, h * w,
                                       _ptr(ws), ws.numel(), _lib.F32, _stream(dz)))
    return db


def act_bwd_bias_grad(y, dy, act, db, c, c_off=0, out=None, ws_key=None):
    """dz = dy * act'(y) on channels [c_off, c_off + c) and db = sum of dz over (n, h, w), in one pass (dz may be dy)."""
    _check_f32(y, dy, db)
    dz = out if out is not None else torch.empty_like(dy)
    n, c_total, h, w = dy.shape
    if dy.numel() == 0:     # nothing to write but the sum of nothing
        db.zero_()
        return dz
    ws = workspace2(dy.device, _lib.lib.dlwp_bias_grad_workspace(int(c)), ws_key)
    _lib.check(_lib.lib.dlwp_act_bwd_bias_grad(_lib.handle(_dev(dy)), _ptr(y), _ptr(dy), _ptr(dz), _ptr(db), n, int(c),
                                               int(c_off), c_total, h * w, int(act), _ptr(ws), ws.numel(), _lib.F32,
                                               _stream(dy)))
    return dz


def pool_act_bwd_bias_grad(y, dp, act, db=None, ws_key=None, out=None):
    """Backward of MaxPooling2D(2) + activation (+ bias gradient) of the convolution that produced y, in one pass:
    returns dz (shape of y; `out`, which must not be y, or a new tensor) from the pooled tensor's gradient dp."""
    _check_f32(y, dp, db, out)
    n, c, h, w = y.shape
    assert tuple(dp.shape) == (n, c, h // 2, w // 2) and y.is_contiguous() and dp.is_contiguous()
    if out is not None and tuple(out.shape) != tuple(y.shape):
        raise ValueError('pool_act_bwd_bias_grad: out %r does not have the shape of y %r' % (tuple(out.shape), tuple(y.shape)))
    dz = out if out is not None else torch.empty_like(y)
    if y.numel() == 0:      # (dlwp_pool_act_bwd_bias_grad returns before it writes db)
        if db is not None:
            db.zero_()
        return dz
    ws = workspace2(y.device, _lib.lib.dlwp_bias_grad_workspace(int(c)), ws_key)
    _lib.check(_lib.lib.dlwp_pool_act_bwd_bias_grad(_lib.handle(_dev(y)), _ptr(y), _ptr(dp), _ptr(dz),
                                                    _ptr(db), _lib.Shape4(n, c, h, w), int(act),
                                                    _ptr(ws), ws.numel(), _lib.F32, _stream(y)))
    return dz


def mse_mae(y_pred, y_true, out2, dy=None, loss_weight=1.0, ws_key=None):
    """out2 (device, 2 floats) <- [mse, mae]; dy <- loss_weight * 2 (y_pred - y_true) / numel."""
    _check_f32(y_pred, y_true, out2, dy)
    if y_pred.numel() == 0:
        raise ValueError('mse_mae: the loss of an empty batch is undefined')
    d = _dev(y_pred)
    h = _lib.handle(d)
    need = _lib.lib.dlwp_mse_mae_workspace(h)
    ws = workspace(y_pred.device, need, ws_key)
    _lib.check(_lib.lib.dlwp_mse_mae(h, _ptr(y_pred), _ptr(y_true), y_pred.numel(), _ptr(out2), _ptr(dy),
                                     float(loss_weight), _ptr(ws), ws.numel(), _lib.F32, _stream(y_pred)))
    return out2


def mse_mae_phase(y_phase, y_true, out2, dz=None, db=None, loss_weight=1.0, ws_key=None):
    """dlwp_mse_mae on the phase channels (n, 4f, h, w) of a restated output layer against the target (n, f, 2h, 2w); dz
    (phase layout) and db (4f: the sums of dz) are optional outputs."""
    _check_f32(y_phase, y_true, out2, dz, db)
    n, f4, hh, ww = y_phase.shape
    f = f4 // 4
    if f4 != 4 * f or tuple(y_true.shape) != (n, f, 2 * hh, 2 * ww):
        raise ValueError('mse_mae_phase: phase tensor %r does not match the target %r' % (tuple(y_phase.shape), tuple(y_true.shape)))
    if y_phase.numel() == 0:
        raise ValueError('mse_mae_phase: the loss of an empty batch is undefined')
    h = _lib.handle(_dev(y_phase))
    ws = workspace(y_phase.device, _lib.lib.dlwp_mse_mae_phase_workspace(f), ws_key)
    _lib.check(_lib.lib.dlwp_mse_mae_phase(h, _ptr(y_phase), _ptr(y_true), n, f, hh, ww, _ptr(out2), _ptr(dz), _ptr(db),
                                           float(loss_weight), _ptr(ws), ws.numel(), _lib.F32, _stream(y_phase)))
    return out2


def loss_custom(y_pred, y_true, stats7, dy=None, loss_weight=1.0, mean=None, row_weights=None, kind=0, regularize=0):
    """The reference's custom losses (include/dlwp_hip.h: dlwp_loss_custom).  y: (n, c, h, w) device tensors."""
    _check_f32(y_pred, y_true, stats7, dy, mean, row_weights)
    n, c, hh, ww = y_pred.shape
    if y_pred.numel() == 0:
        raise ValueError('loss_custom: the loss of an empty batch is undefined')
    d = _dev(y_pred)
    h = _lib.handle(d)
    ws = workspace(y_pred.device, _lib.lib.dlwp_loss_workspace(h, n, c))
    _lib.check(_lib.lib.dlwp_loss_custom(h, _ptr(y_pred), _ptr(y_true), n, c, hh, ww, _ptr(mean), _ptr(row_weights),
                                         int(kind), int(regularize), _ptr(stats7), _ptr(dy), float(loss_weight), _ptr(ws),
                                         ws.numel(), _lib.F32, _stream(y_pred)))
    return stats7


def loss_elementwise(y_pred, y_true, out1, dy=None, loss_weight=1.0, kind=1, row_weights=None, ws_key=None):
    """include/dlwp_hip.h: dlwp_loss_elementwise.  y: (n, c, h, w) device tensors; out1 (device, 1 float) <- the mean of kind
    (_lib.LOSS_*) over w*y_pred, w*y_true (w = row_weights[h] or 1); dy <- loss_weight * dL/dy_pred."""
    _check_f32(y_pred, y_true, out1, dy, row_weights)
    n, c, hh, ww = y_pred.shape
    if tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError('loss_elementwise: target %r does not match the prediction %r' % (tuple(y_true.shape), tuple(y_pred.shape)))
    h = _lib.handle(_dev(y_pred))
    ws = workspace2(y_pred.device, _lib.lib.dlwp_loss_elementwise_workspace(h), ('loss_ew', ws_key))
    _lib.check(_lib.lib.dlwp_loss_elementwise(h, _ptr(y_pred), _ptr(y_true), n, c, hh, ww, _ptr(row_weights), int(kind),
                                              _ptr(out1), _ptr(dy), float(loss_weight), _ptr(ws), ws.numel(), _lib.F32,
                                              _stream(y_pred)))
    return out1


def loss_elementwise_phase(y_phase, y_true, out1, dz=None, db=None, loss_weight=1.0, kind=1, row_weights=None, ws_key=None):
    """loss_elementwise on the phase channels (n, 4f, h, w) of a restated output layer against the target (n, f, 2h, 2w) (w
    even); dz (phase layout) and db (4f: the sums of dz) are optional outputs, as for mse_mae_phase."""
    _check_f32(y_phase, y_true, out1, dz, db, row_weights)
    n, f4, hh, ww = y_phase.shape
    f = f4 // 4
    if f4 != 4 * f or tuple(y_true.shape) != (n, f, 2 * hh, 2 * ww):
        raise ValueError('loss_elementwise_phase: phase tensor %r does not match the target %r'
                         % (tuple(y_phase.shape), tuple(y_true.shape)))
    h = _lib.handle(_dev(y_phase))
    ws = workspace2(y_phase.device, _lib.lib.dlwp_loss_elementwise_phase_workspace(f), ('loss_ew_phase', ws_key))
    _lib.check(_lib.lib.dlwp_loss_elementwise_phase(h, _ptr(y_phase), _ptr(y_true), n, f, hh, ww, _ptr(row_weights), int(kind),
                                                    _ptr(out1), _ptr(dz), _ptr(db), float(loss_weight), _ptr(ws), ws.numel(),
                                                    _lib.F32, _stream(y_phase)))
    return out1


def metric_columns(mask):
    """Number of floats dlwp_loss_metrics writes for `mask`."""
    return bin(int(mask) & 0x1f).count('1') + (3 if int(mask) & _lib.METRIC_ACC_SUMS else 0)


def loss_metrics(y_pred, y_true, out, mask, phase=False, ws_key=None):
    """include/dlwp_hip.h: dlwp_loss_metrics -- one pass over (y_pred, y_true) fills out[:metric_columns(mask)] with the selected
    means (mse, mae, mape, msle, logcosh, then mean(p t), mean(p^2), mean(t^2)).  phase: y_pred is the phase form
    (n, 4f, h, w) of the (n, f, 2h, 2w) target."""
    _check_f32(y_pred, y_true, out)
    n, c, hh, ww = y_true.shape
    if phase:
        if tuple(y_pred.shape) != (n, 4 * c, hh // 2, ww // 2):
            raise ValueError('loss_metrics: phase tensor %r does not match the target %r' % (tuple(y_pred.shape), tuple(y_true.shape)))
    elif tuple(y_pred.shape) != tuple(y_true.shape):
        raise ValueError('loss_metrics: target %r does not match the prediction %r' % (tuple(y_true.shape), tuple(y_pred.shape)))
    if out.numel() < metric_columns(mask):
        raise ValueError('loss_metrics: %d output floats for %d metric columns' % (out.numel(), metric_columns(mask)))
    h = _lib.handle(_dev(y_pred))
    ws = workspace2(y_pred.device, _lib.lib.dlwp_loss_metrics_workspace(h), ('loss_metrics', ws_key))
    _lib.check(_lib.lib.dlwp_loss_metrics(h, _ptr(y_pred), _ptr(y_true), n, c, hh, ww, 1 if phase else 0, int(mask), _ptr(out),
                                          _ptr(ws), ws.numel(), _lib.F32, _stream(y_pred)))
    return out


def adam_keras(p, m, v, g, iteration, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0, grad_scale=1.0):
    _check_f32(p, m, v, g)
    if p.numel() == 0:      # (an empty tensor has no address for the C ABI to check)
        return
    _lib.check(_lib.lib.dlwp_adam_keras(_lib.handle(_dev(p)), _ptr(p), _ptr(m), _ptr(v), _ptr(g), p.numel(), lr, beta_1,
                                        beta_2, epsilon, decay, int(iteration), grad_scale, _stream(p)))


def adam_keras_dev(p, m, v, g, iteration_dev, lr_t_scratch, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0,
                   grad_scale=1.0):
    """adam_keras with the step number in device memory (int64 tensor of one element, advanced by the call) -- the form a
    captured training step replays."""
    _check_f32(p, m, v, g, lr_t_scratch)
    if iteration_dev.dtype != torch.int64 or iteration_dev.numel() != 1:
        raise ValueError('iteration_dev must be one int64 on the device')
    if p.numel() == 0:      # nothing is touched, the step number included (as dlwp_adam_keras_dev itself has it)
        return
    _lib.check(_lib.lib.dlwp_adam_keras_dev(_lib.handle(_dev(p)), _ptr(p), _ptr(m), _ptr(v), _ptr(g), p.numel(), lr, beta_1,
                                            beta_2, epsilon, decay, _ptr(iteration_dev), _ptr(lr_t_scratch), grad_scale,
                                            _stream(p)))


def sgd_keras(p, vel, g, iteration, lr=0.01, momentum=0.0, decay=0.0, grad_scale=1.0):
    _check_f32(p, vel, g)
    if p.numel() == 0:
        return
    _lib.check(_lib.lib.dlwp_sgd_keras(_lib.handle(_dev(p)), _ptr(p), _ptr(vel), _ptr(g), p.numel(), lr, momentum, decay,
                                       int(iteration), grad_scale, _stream(p)))


#: dlwp_optimizer_step kinds (include/dlwp_hip.h: DLWP_OPT_*) and the slot arrays each takes
OPT_SGD, OPT_SGD_NESTEROV, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADADELTA, OPT_ADAM, OPT_ADAM_AMSGRAD, OPT_ADAMAX, OPT_NADAM = range(9)
OPT_SLOTS = (1, 1, 1, 1, 2, 2, 3, 2, 2)


def grad_clip_factor(g, clipnorm, grad_scale=1.0, out=None, ws_key=None):
    """out (3 device floats) <- {factor, norm, norm^2} of the gradient g * grad_scale: factor = clipnorm / norm where norm >=
    clipnorm, else exactly 1 (Keras' clip_norm).  A fixed double-precision tree: the same input gives the same bits.  Nothing
    comes back to the host: optimizer_step reads the factor from `out`."""
    _check_f32(g, out)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=g.device)
    if out.numel() < 3:
        raise ValueError('grad_clip_factor: 3 output floats, please')
    h = _lib.handle(_dev(out))
    ws = workspace2(out.device, _lib.lib.dlwp_grad_clip_factor_workspace(h), ('clip', ws_key))
    _lib.check(_lib.lib.dlwp_grad_clip_factor(h, _ptr(g) if g.numel() else None, g.numel(), float(grad_scale), float(clipnorm),
                                              _ptr(ws), ws.numel(), _ptr(out), _stream(out)))
    return out


def optimizer_step(kind, p, slots, g, iteration, lr, decay=0.0, h1=0.0, h2=0.0, epsilon=1e-7, schedule_decay=0.0,
                   m_schedule=1.0, grad_scale=1.0, clipvalue=0.0, factor=None):
    """One update of kind OPT_* (dlwp_optimizer_step: the formulas are in include/dlwp_hip.h) in one launch.  slots: OPT_SLOTS[kind]
    tensors like p; factor: the device tensor grad_clip_factor filled, or None."""
    kind = int(kind)
    slots = tuple(slots)
    if not 0 <= kind < len(OPT_SLOTS) or len(slots) != OPT_SLOTS[kind]:
        raise ValueError('optimizer_step: kind %r takes %s slot arrays, %d given'
                         % (kind, OPT_SLOTS[kind] if 0 <= kind < len(OPT_SLOTS) else 'no', len(slots)))
    _check_f32(p, g, factor, *slots)
    if any(t.numel() != p.numel() for t in slots + (g,)):
        raise ValueError('optimizer_step: parameters, slots and gradient must have the same number of elements')
    if p.numel() == 0:
        return
    s = [_ptr(t) for t in slots] + [None] * (3 - len(slots))
    _lib.check(_lib.lib.dlwp_optimizer_step(_lib.handle(_dev(p)), kind, _ptr(p), s[0], s[1], s[2], _ptr(g), p.numel(), lr, decay,
                                            h1, h2, epsilon, schedule_decay, float(m_schedule), int(iteration), grad_scale,
                                            clipvalue, _ptr(factor) if factor is not None else None, _stream(p)))


def copy_many(pairs):
    """[(src, dst), ...] (at most 8 contiguous float32 tensors of equal element counts per pair) copied by ONE launch."""
    pairs = list(pairs)
    if not pairs:
        return
    for s, d in pairs:
        _check_f32(s, d)
        if s.numel() != d.numel() or not s.is_contiguous() or not d.is_contiguous():
            raise ValueError('copy_many: contiguous tensors of equal size, please')
    k = len(pairs)
    srcs = (ctypes.c_void_p * k)(*[s.data_ptr() for s, _ in pairs])
    dsts = (ctypes.c_void_p * k)(*[d.data_ptr() for _, d in pairs])
    cnt = (ctypes.c_size_t * k)(*[s.numel() for s, _ in pairs])
    dst0 = pairs[0][1]
    _lib.check(_lib.lib.dlwp_copy_many(_lib.handle(_dev(dst0)), srcs, dsts, cnt, k, _stream(dst0)))


def axpby(x, y, a=1.0, b=1.0):
    """y <- a*x + b*y"""
    _check_f32(x, y)
    if x.numel() == 0:
        return y
    _lib.check(_lib.lib.dlwp_axpby(_lib.handle(_dev(x)), _ptr(x), _ptr(y), x.numel(), float(a), float(b), _stream(x)))
    return y


def wgrad_configs():
    """[(ks, dil, th, tw, cout_frags, waves, lds_bytes)] of the compiled weight-gradient tiles."""
    out = []
    info = (ctypes.c_int * 6)()
    lds = ctypes.c_int()
    for i in range(_lib.lib.dlwp_conv2d_wgrad_num_configs()):
        _lib.check(_lib.lib.dlwp_conv2d_wgrad_config_info(i, info, ctypes.byref(lds)))
        out.append(tuple(info) + (lds.value,))
    return out


def wgrad_config_forms():
    """[(input channels per workgroup, form)] per compiled weight-gradient instance; form 0 direct, 1 Winograd, 3 channel-block
    Winograd, 4 the streaming form for at most 4 input channels."""
    out = []
    cib, form = ctypes.c_int(), ctypes.c_int()
    for i in range(_lib.lib.dlwp_conv2d_wgrad_num_configs()):
        _lib.check(_lib.lib.dlwp_conv2d_wgrad_config_form(i, ctypes.byref(cib), ctypes.byref(form)))
        out.append((cib.value, form.value))
    return out


def force_wgrad_config(i):
    _lib.set_option(_lib.OPT_FORCE_WGRAD_CONFIG, int(i))


# ------------------------------------------------------------------------------------------------------------------ #
# BatchNormalization(axis=1) (csrc/batchnorm.hip)
# ------------------------------------------------------------------------------------------------------------------ #

def batchnorm_desc(x, momentum=0.99, epsilon=1e-3):
    n, c = int(x.shape[0]), int(x.shape[1])
    hw = 1
    for d in x.shape[2:]:
        hw *= int(d)
    return _lib.BatchNorm(n, c, hw, float(momentum), float(epsilon))


def batchnorm_workspace_bytes(d):
    return int(_lib.lib.dlwp_batchnorm_workspace(d))


def batchnorm_fwd_train(x, gamma, beta, moving_mean, moving_var, save_mean, save_invstd, ws, momentum=0.99, epsilon=1e-3,
                        out=None):
    """Training forward with the batch's statistics; updates moving_mean / moving_var in place and keeps the batch's mean and
    1 / sqrt(var + eps) in save_mean / save_invstd for batchnorm_bwd.  ws: a uint8 device tensor of batchnorm_workspace_bytes."""
    _check_f32(x, gamma, beta, moving_mean, moving_var, save_mean, save_invstd, out)
    y = out if out is not None else torch.empty_like(x)
    d = batchnorm_desc(x, momentum, epsilon)
    _lib.check(_lib.lib.dlwp_batchnorm_fwd_train(_lib.handle(_dev(x)), _ptr(x), _ptr(y), _ptr(gamma), _ptr(beta),
                                                 _ptr(moving_mean), _ptr(moving_var), _ptr(save_mean), _ptr(save_invstd),
                                                 _ptr(ws), ws.numel() * ws.element_size(), d, _stream(x)))
    return y


def batchnorm_fwd_infer(x, gamma, beta, moving_mean, moving_var, epsilon=1e-3, out=None):
    """Inference: the same affine map with the moving statistics."""
    _check_f32(x, gamma, beta, moving_mean, moving_var, out)
    y = out if out is not None else torch.empty_like(x)
    d = batchnorm_desc(x, 0.0, epsilon)
    _lib.check(_lib.lib.dlwp_batchnorm_fwd_infer(_lib.handle(_dev(x)), _ptr(x), _ptr(y), _ptr(gamma), _ptr(beta),
                                                 _ptr(moving_mean), _ptr(moving_var), d, _stream(x)))
    return y


def batchnorm_bwd(x, dy, gamma, save_mean, save_invstd, ws, dgamma=None, dbeta=None, dx=None, want_dx=True):
    """dx (None when want_dx is False), writing dgamma / dbeta (nullable) -- the backward of batchnorm_fwd_train."""
    _check_f32(x, dy, gamma, save_mean, save_invstd, dgamma, dbeta, dx)
    if want_dx and dx is None:
        dx = torch.empty_like(x)
    d = batchnorm_desc(x)
    _lib.check(_lib.lib.dlwp_batchnorm_bwd(_lib.handle(_dev(x)), _ptr(x), _ptr(dy), _ptr(dx if want_dx else None), _ptr(gamma),
                                           _ptr(save_mean), _ptr(save_invstd), _ptr(dgamma), _ptr(dbeta), _ptr(ws),
                                           ws.numel() * ws.element_size(), d, _stream(x)))
    return dx if want_dx else None


# ------------------------------------------------------------------------------------------------------------------ #
# the wrapper's scaler and imputer (csrc/scale.hip)
# ------------------------------------------------------------------------------------------------------------------ #
SCALE_KINDS = {'standard': _lib.SCALE_STANDARD, 'minmax': _lib.SCALE_MINMAX}


def _scale_desc(x, kind, *params):
    """x: (n, ...) float32 -- a sample's features are everything behind the first axis; params: float64 vectors of that length"""
    if x.dtype != torch.float32 or x.dim() < 1:
        raise ValueError('expected a float32 tensor of samples, got %s' % x.dtype)
    n = int(x.shape[0])
    f = 1
    for s in x.shape[1:]:
        f *= int(s)
    for p in params:
        if p is not None and (p.dtype != torch.float64 or not p.is_contiguous() or p.numel() != f or p.device != x.device):
            raise ValueError('scaler parameters are contiguous float64 vectors of %d features on the device of x' % f)
    return _lib.Scale(n, f, SCALE_KINDS[kind] if not isinstance(kind, int) else int(kind))


def _scale_out(x, out):
    if not x.is_contiguous():
        raise ValueError('expected a contiguous tensor')
    y = out if out is not None else torch.empty_like(x)
    if y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != x.numel():
        raise ValueError('out must be a contiguous float32 tensor of the size of x')
    return y


def scale_fwd(x, kind, fill=None, shift=None, scale=None, out=None):
    """SimpleImputer.transform (fill = statistics_), then the scaler's transform: 'standard' (x - shift) / scale with shift / scale =
    mean_ / scale_, 'minmax' x * scale + shift with shift / scale = min_ / scale_.  Every parameter is a float64 device vector or
    None (that stage is left out); sklearn's arithmetic bit for bit (include/dlwp_hip.h).  out may be x."""
    d = _scale_desc(x, kind, fill, shift, scale)
    y = _scale_out(x, out)
    _lib.check(_lib.lib.dlwp_scale_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), _ptr(fill), _ptr(shift), _ptr(scale), d, _stream(x)))
    return y


def scale_inv(x, kind, shift=None, scale=None, out=None):
    """The scaler's inverse_transform: 'standard' x * scale + shift, 'minmax' (x - shift) / scale.  out may be x."""
    d = _scale_desc(x, kind, shift, scale)
    y = _scale_out(x, out)
    _lib.check(_lib.lib.dlwp_scale_inv(_lib.handle(_dev(x)), _ptr(x), _ptr(y), _ptr(shift), _ptr(scale), d, _stream(x)))
    return y


# ------------------------------------------------------------------------------------------------------------------ #
# Dense and Dropout (csrc/dense.hip)
# ------------------------------------------------------------------------------------------------------------------ #

def _dense_desc(m, kernel, act):
    k, n = (int(v) for v in kernel.shape)
    return _lib.Dense(int(m), k, n, ACTIVATIONS[act] if not isinstance(act, int) else int(act))


def _rows(t):
    """samples of a (n, ...) tensor whose per-sample block is read as one row"""
    return int(t.shape[0])


def dense_fwd(x, kernel, bias, act=None, out=None):
    """y = act(x kernel + bias): x (m, ...) with prod(...) = k features per sample, kernel (k, units) in Keras layout, bias
    (units,) or None.  out: any contiguous tensor of m * units floats (default (m, units))."""
    _check_f32(x, kernel, bias, out)
    d = _dense_desc(_rows(x), kernel, act)
    if x.numel() != d.m * d.k:
        raise ValueError('dense_fwd: input of %r does not hold %d features per sample' % (tuple(x.shape), d.k))
    y = out if out is not None else torch.empty((d.m, d.n), dtype=torch.float32, device=x.device)
    if y.numel() != d.m * d.n:
        raise ValueError('dense_fwd: output of %r does not hold %d units per sample' % (tuple(y.shape), d.n))
    _lib.check(_lib.lib.dlwp_dense_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(kernel), _ptr(bias), _ptr(y), d, _stream(x)))
    return y


def dense_bwd_data(dy, y, kernel, act=None, out=None):
    """dx = (dy o act'(y)) kernel^T, (m, k) unless out is given; y: the forward's output (not read when act is linear)."""
    _check_f32(dy, y, kernel, out)
    d = _dense_desc(_rows(dy), kernel, act)
    if dy.numel() != d.m * d.n or (y is not None and y.numel() != dy.numel()):
        raise ValueError('dense_bwd_data: gradient of %r does not match %d units per sample' % (tuple(dy.shape), d.n))
    dx = out if out is not None else torch.empty((d.m, d.k), dtype=torch.float32, device=dy.device)
    if dx.numel() != d.m * d.k:
        raise ValueError('dense_bwd_data: output of %r does not hold %d features per sample' % (tuple(dx.shape), d.k))
    _lib.check(_lib.lib.dlwp_dense_bwd_data(_lib.handle(_dev(dy)), _ptr(dy), _ptr(y), _ptr(kernel), _ptr(dx), d, _stream(dy)))
    return dx


def dense_bwd_weight(x, dy, y, dkernel, dbias=None, act=None):
    """dkernel (k, units) = x^T (dy o act'(y)), dbias (units,) = its column sums (None: not wanted); both overwritten."""
    _check_f32(x, dy, y, dkernel, dbias)
    d = _dense_desc(_rows(x), dkernel, act)
    if x.numel() != d.m * d.k or dy.numel() != d.m * d.n or (y is not None and y.numel() != dy.numel()):
        raise ValueError('dense_bwd_weight: x %r / dy %r do not match a (%d, %d) kernel' % (tuple(x.shape), tuple(dy.shape), d.k, d.n))
    if dbias is not None and dbias.numel() != d.n:
        raise ValueError('dense_bwd_weight: bias gradient of %d elements for %d units' % (dbias.numel(), d.n))
    _lib.check(_lib.lib.dlwp_dense_bwd_weight(_lib.handle(_dev(x)), _ptr(x), _ptr(dy), _ptr(y), _ptr(dkernel), _ptr(dbias), d,
                                              _stream(x)))
    return dkernel


def dropout_desc(rate, seed, layer, step):
    """The launch descriptor of keras Dropout(rate): threshold = floor(rate 2^32) (an element is kept when its Philox word is >=
    it), scale = float32(1 / (1 - rate)); seed a 64-bit integer, layer / step 32-bit."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError('dropout rate must be in [0, 1), got %r' % (rate,))
    thr = min(int(rate * 4294967296.0), 4294967295)
    return _lib.Dropout(int(seed) & 0xffffffffffffffff, int(layer) & 0xffffffff, int(step) & 0xffffffff, thr, 1.0 / (1.0 - rate))


def dropout_fwd(x, rate, seed, layer, step, out=None):
    """y = x * mask / (1 - rate), the mask of (seed, layer, step); rate 0 copies."""
    _check_f32(x, out)
    y = out if out is not None else torch.empty_like(x)
    _lib.check(_lib.lib.dlwp_dropout_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), x.numel(), dropout_desc(rate, seed, layer, step),
                                         _stream(x)))
    return y


def dropout_bwd(dy, rate, seed, layer, step, out=None):
    """dx = dy * mask / (1 - rate) with the mask the forward of (seed, layer, step) drew."""
    _check_f32(dy, out)
    dx = out if out is not None else torch.empty_like(dy)
    _lib.check(_lib.lib.dlwp_dropout_bwd(_lib.handle(_dev(dy)), _ptr(dy), _ptr(dx), dy.numel(), dropout_desc(rate, seed, layer, step),
                                         _stream(dy)))
    return dx


# ------------------------------------------------------------------------------------------------------------------ #
# Activation and merge layers (csrc/eltwise.hip)
# ------------------------------------------------------------------------------------------------------------------ #

ELT_KINDS = {'relu': _lib.ELT_RELU, 'elu': _lib.ELT_ELU, 'selu': _lib.ELT_SELU, 'sigmoid': _lib.ELT_SIGMOID,
             'hard_sigmoid': _lib.ELT_HARD_SIGMOID, 'softplus': _lib.ELT_SOFTPLUS, 'softsign': _lib.ELT_SOFTSIGN,
             'tanh': _lib.ELT_TANH}
MERGE_KINDS = {'add': _lib.MERGE_ADD, 'subtract': _lib.MERGE_SUBTRACT, 'multiply': _lib.MERGE_MULTIPLY,
               'average': _lib.MERGE_AVERAGE, 'maximum': _lib.MERGE_MAXIMUM, 'minimum': _lib.MERGE_MINIMUM}


def activation_desc(kind, alpha=0.0, max_value=None, theta=0.0):
    """dlwp_activation of (kind, alpha, max_value | None, theta) -- a layer's `eltwise` tuple; no cap is max_value = +inf"""
    return _lib.Activation(ELT_KINDS[kind] if not isinstance(kind, int) else int(kind), float(alpha),
                           float('inf') if max_value is None else float(max_value), float(theta))


def activation_fwd(x, kind, alpha=0.0, max_value=None, theta=0.0, out=None):
    """y = f(x), element by element (include/dlwp_hip.h: DLWP_ELT_*); out: a contiguous tensor of x.numel() floats, not x."""
    _check_f32(x, out)
    y = out if out is not None else torch.empty_like(x)
    if y.numel() != x.numel():
        raise ValueError('activation_fwd: output of %r for an input of %r' % (tuple(y.shape), tuple(x.shape)))
    _lib.check(_lib.lib.dlwp_activation_fwd(_lib.handle(_dev(x)), _ptr(x), _ptr(y), x.numel(),
                                            activation_desc(kind, alpha, max_value, theta), _stream(x)))
    return y


def activation_bwd(x, dy, kind, alpha=0.0, max_value=None, theta=0.0, out=None):
    """dx = dy f'(x) from the forward's INPUT x; out: not x, not dy."""
    _check_f32(x, dy, out)
    if dy.numel() != x.numel():
        raise ValueError('activation_bwd: gradient of %r for an input of %r' % (tuple(dy.shape), tuple(x.shape)))
    dx = out if out is not None else torch.empty_like(x)
    if dx.numel() != x.numel():
        raise ValueError('activation_bwd: output of %r for an input of %r' % (tuple(dx.shape), tuple(x.shape)))
    _lib.check(_lib.lib.dlwp_activation_bwd(_lib.handle(_dev(x)), _ptr(x), _ptr(dy), _ptr(dx), x.numel(),
                                            activation_desc(kind, alpha, max_value, theta), _stream(x)))
    return dx


def _merge_args(who, kind, xs):
    xs = list(xs)
    if not 2 <= len(xs) <= 4:
        raise ValueError('%s: %d sources (2 to 4)' % (who, len(xs)))
    _check_f32(*xs)
    if any(t.numel() != xs[0].numel() for t in xs):
        raise ValueError('%s: sources of different sizes %r' % (who, [tuple(t.shape) for t in xs]))
    return xs, _lib.Merge(MERGE_KINDS[kind] if not isinstance(kind, int) else int(kind), len(xs))


def merge_fwd(kind, xs, out=None):
    """y = ((x0 o x1) o x2) o x3 over 2 to 4 tensors of one size, left to right ('average': that sum / float32(len(xs)))."""
    xs, d = _merge_args('merge_fwd', kind, xs)
    _check_f32(out)
    y = out if out is not None else torch.empty_like(xs[0])
    if y.numel() != xs[0].numel():
        raise ValueError('merge_fwd: output of %r for sources of %r' % (tuple(y.shape), tuple(xs[0].shape)))
    p = [_ptr(t) for t in xs] + [_ptr(None)] * (4 - len(xs))
    _lib.check(_lib.lib.dlwp_merge_fwd(_lib.handle(_dev(y)), p[0], p[1], p[2], p[3], _ptr(y), y.numel(), d, _stream(y)))
    return y


def merge_bwd(kind, xs, dy, outs=None, want=None):
    """The gradient of every source in one pass: a list with one NEW tensor per source (None where want[i] is false), or the
    tensors of `outs` (None entries are not written).  No two sources share a gradient tensor."""
    xs, d = _merge_args('merge_bwd', kind, xs)
    _check_f32(dy)
    if dy.numel() != xs[0].numel():
        raise ValueError('merge_bwd: gradient of %r for sources of %r' % (tuple(dy.shape), tuple(xs[0].shape)))
    if outs is None:
        outs = [torch.empty_like(t) if (want is None or want[i]) else None for i, t in enumerate(xs)]
    outs = list(outs)
    _check_f32(*outs)
    if len(outs) != len(xs) or any(o is not None and o.numel() != dy.numel() for o in outs):
        raise ValueError('merge_bwd: one gradient tensor (or None) of the sources\' size per source')
    p = [_ptr(t) for t in xs] + [_ptr(None)] * (4 - len(xs))
    q = [_ptr(t) for t in outs] + [_ptr(None)] * (4 - len(xs))
    _lib.check(_lib.lib.dlwp_merge_bwd(_lib.handle(_dev(dy)), p[0], p[1], p[2], p[3], _ptr(dy), q[0], q[1], q[2], q[3],
                                       dy.numel(), d, _stream(dy)))
    return outs


def verify_extent(strides, leads, count0, count_dec, groups, run):
    """Elements an operand of dlwp_verify_error_sums must hold: one past the last offset a lead with pairs addresses (0: none)."""
    ls, ss, shift = (int(v) for v in strides)
    need = 0
    for f in range(int(leads)):
        cnt = int(count0) - f * int(count_dec)
        if cnt <= 0:
            break
        need = max(need, f * ls + (cnt - 1 + f * shift) * ss + int(groups) * int(run))
    return need


def _window_operands(who, leads, count0, count_dec, groups, run, operands, table=None, label_strides=(0, 0),
                     sizes='leads, groups, run'):
    """The operand block of the windowed wrappers.  operands: (name, tensor, (lead_stride, sample_stride, shift)) each; all of them
    and `table` on one device, every size >= 1 (`sizes` names them in the refusal) and no stride, shift or count_dec below 0,
    every element the strides address inside its tensor.  Returns (device index, leads, count0, count_dec, groups, run) as ints."""
    d = _dev(operands[0][1])
    if any(_dev(t) != d for _, t, _ in operands[1:]) or (table is not None and _dev(table) != d):
        raise ValueError('%s: operands on different devices' % who)
    leads, count0, count_dec, groups, run = int(leads), int(count0), int(count_dec), int(groups), int(run)
    if (leads < 1 or groups < 1 or run < 1 or count_dec < 0 or min(label_strides) < 0
            or any(min(st) < 0 for _, _, st in operands)):
        raise ValueError('%s: %s must be >= 1; strides, shifts and count_dec >= 0' % (who, sizes))
    for name, t, st in operands:
        need = verify_extent(st, leads, count0, count_dec, groups, run)
        if need > t.numel():
            raise ValueError('%s: operand %s holds %d elements, the strides address %d' % (who, name, t.numel(), need))
    return d, leads, count0, count_dec, groups, run


def verify_error_sums(a, a_strides, b, b_strides, leads, count0, count_dec, groups, run):
    """include/dlwp_hip.h: dlwp_verify_error_sums.  a, b: contiguous float32 device tensors read as flat arrays through
    x_strides = (lead_stride, sample_stride, shift) in elements.  Returns a NEW (leads, groups, 3) float64 device tensor: sum d^2,
    sum |d| and the pairs counted (d = a - b; NaN pairs skipped) per lead and group, enqueued on the current stream."""
    _check_f32(a, b)
    if _dev(b) != _dev(a):      # this wrapper names the devices
        raise ValueError('verify_error_sums: operands on devices %d and %d' % (_dev(a), _dev(b)))
    d, leads, count0, count_dec, groups, run = _window_operands('verify_error_sums', leads, count0, count_dec, groups, run,
                                                                (('a', a, a_strides), ('b', b, b_strides)))
    h = _lib.handle(d)
    ws = torch.empty(max(int(_lib.lib.dlwp_verify_error_workspace(h, leads, groups)), 8), dtype=torch.uint8, device=a.device)
    sums = torch.empty((leads, groups, 3), dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib.dlwp_verify_error_sums(h, _ptr(a), int(a_strides[0]), int(a_strides[1]), int(a_strides[2]),
                                               _ptr(b), int(b_strides[0]), int(b_strides[1]), int(b_strides[2]),
                                               leads, count0, count_dec, groups, run, _ptr(sums), _ptr(ws), ws.numel(), _stream(a)))
    return sums


SKILL_SUMS = 10


def verify_label_extent(strides, leads, count0, count_dec):
    """Labels dlwp_verify_skill_sums reads through strides = (lead_stride, shift): one past the last index of a lead with pairs"""
    ls, shift = (int(v) for v in strides)
    need = 0
    for f in range(int(leads)):
        cnt = int(count0) - f * int(count_dec)
        if cnt <= 0:
            break
        need = max(need, f * ls + cnt - 1 + f * shift + 1)
    return need


def skill_labels(labels, n_labels):
    """HOST labels of dlwp_verify_skill_sums as a flat int32 array: an integer dtype, every entry in [-1, n_labels), -1 = skip the
    pair.  ValueError otherwise."""
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise ValueError('verify_skill_sums: labels must be integers, got %s' % labels.dtype)
    if labels.size and (int(labels.min()) < -1 or int(labels.max()) >= int(n_labels)):
        raise ValueError('verify_skill_sums: labels must lie in [-1, %d), got %d .. %d' % (n_labels, labels.min(), labels.max()))
    return np.ascontiguousarray(labels.reshape(-1), dtype=np.int32)


def skill_weights(weights):
    """HOST weights of dlwp_verify_skill_sums as a float32 array: 1-D, finite, >= 0 and not all zero.  ValueError otherwise."""
    weights = np.asarray(weights)
    if weights.ndim != 1 or weights.size < 1 or weights.dtype.kind not in 'fiu':
        raise ValueError('verify_skill_sums: weights must be a 1-D real array, got %s of shape %r' % (weights.dtype, weights.shape))
    weights = np.ascontiguousarray(weights, dtype=np.float32)
    if not np.isfinite(weights).all():
        raise ValueError('verify_skill_sums: weights must be finite')
    if (weights < 0).any():
        raise ValueError('verify_skill_sums: weights must be >= 0, got %g' % weights.min())
    if not (weights > 0).any():
        raise ValueError('verify_skill_sums: weights are all zero')
    return weights


def _climo_labels(who, climo, labels, label_strides, leads, count0, count_dec, trow):
    """The climatology block of verify_skill_sums and verify_skill_map: the table has rows of `trow` floats and at most
    VERIFY_MAX_LABELS of them, labels need a table, lie in [-1, n_labels) and hold every index label_strides address.  Returns
    (n_labels, the labels as a flat HOST int32 array or None)."""
    n_labels = 0
    if climo is not None:
        n_labels, have = _rows_of(climo, who)
        if have != trow:
            raise ValueError('%s: table rows of %d floats, sample rows of %d' % (who, have, trow))
        if n_labels > VERIFY_MAX_LABELS:
            raise ValueError('%s: %d labels, at most %d' % (who, n_labels, VERIFY_MAX_LABELS))
    elif labels is not None:
        raise ValueError('%s: labels without a climatology table' % who)
    if labels is not None:
        labels = skill_labels(labels, n_labels)
        need = verify_label_extent(label_strides, leads, count0, count_dec)
        if need > labels.size:
            raise ValueError('%s: %d labels, the strides address %d' % (who, labels.size, need))
    return n_labels, labels


def verify_skill_sums(fc, fc_strides, ob, ob_strides, leads, count0, count_dec, groups, run, climo=None, labels=None,
                      label_strides=(0, 0), weights=None, w_inner=1):
    """include/dlwp_hip.h: dlwp_verify_skill_sums.  fc, ob: contiguous float32 device tensors read as flat arrays through
    x_strides = (lead_stride, sample_stride, shift) in elements, as in verify_error_sums.  climo: a (n_labels, ...) float32 device
    tensor whose rows hold groups * run floats, or None; labels: a HOST integer array read flat through label_strides =
    (lead_stride, shift), entries in [-1, n_labels) with -1 = skip the pair, or None (label 0); weights: a HOST 1-D array, finite,
    >= 0, not all zero -- element e of a run has weight weights[(e // w_inner) % len(weights)] -- or None.  Labels and weights are
    checked here and then uploaded.  Returns a NEW (leads, groups, 10) float64 device tensor: sum w, w d, w d^2, w |d|, w fa, w oa,
    w fa oa, w fa^2, w oa^2 and the pairs counted (d = fc - ob, fa = fc - c, oa = ob - c), enqueued on the current stream."""
    _check_f32(fc, ob, climo)
    d, leads, count0, count_dec, groups, run = _window_operands(
        'verify_skill_sums', leads, count0, count_dec, groups, run, (('fc', fc, fc_strides), ('ob', ob, ob_strides)),
        table=climo, label_strides=label_strides)
    n_labels, labels = _climo_labels('verify_skill_sums', climo, labels, label_strides, leads, count0, count_dec, groups * run)
    w_len, w_inner = 0, int(w_inner)
    if weights is not None:
        weights = skill_weights(weights)
        w_len = int(weights.size)
        if w_inner < 1 or run % (w_inner * w_len):
            raise ValueError('verify_skill_sums: %d weights of %d elements each do not divide a run of %d' % (w_len, w_inner, run))
    h = _lib.handle(d)
    labels_d = None if labels is None else torch.from_numpy(labels).to(fc.device)
    weights_d = None if weights is None else torch.from_numpy(weights).to(fc.device)
    ws = torch.empty(max(int(_lib.lib.dlwp_verify_skill_workspace(h, leads, groups)), 8), dtype=torch.uint8, device=fc.device)
    sums = torch.empty((leads, groups, SKILL_SUMS), dtype=torch.float64, device=fc.device)
    _lib.check(_lib.lib.dlwp_verify_skill_sums(h, _ptr(fc), int(fc_strides[0]), int(fc_strides[1]), int(fc_strides[2]),
                                               _ptr(ob), int(ob_strides[0]), int(ob_strides[1]), int(ob_strides[2]),
                                               leads, count0, count_dec, groups, run, _ptr(climo), n_labels, _ptr(labels_d),
                                               int(label_strides[0]), int(label_strides[1]), _ptr(weights_d), w_len, w_inner,
                                               _ptr(sums), _ptr(ws), ws.numel(), _stream(fc)))
    return sums


SKILL_MAP_SUMS, SKILL_MAP_SCORES = 9, 6


def verify_skill_map(fc, fc_strides, ob, ob_strides, leads, count0, count_dec, row, climo=None, labels=None, label_strides=(0, 0),
                     split=0, want_sums=True, want_scores=True):
    """include/dlwp_hip.h: dlwp_verify_skill_map.  Operands, table and labels as in verify_skill_sums with groups = 1 and run = row:
    checked here (every addressed element exists, labels in [-1, n_labels)) before anything is uploaded or launched.  split: 0 = the
    library's rule, a positive number = that many chunks of the sample axis (capped at count0).  Returns (sums, scores, counts):
    NEW device tensors (leads, 9, row) float64, (leads, 6, row) float32 and (leads, row) int32, enqueued on the current stream; sums
    is None without want_sums, scores and counts are None without want_scores."""
    _check_f32(fc, ob, climo)
    split = int(split)
    if split < 0:
        raise ValueError('verify_skill_map: split must be >= 0, got %d' % split)
    if not (want_sums or want_scores):
        raise ValueError('verify_skill_map: neither sums nor scores wanted')
    d, leads, count0, count_dec, _, row = _window_operands(
        'verify_skill_map', leads, count0, count_dec, 1, row, (('fc', fc, fc_strides), ('ob', ob, ob_strides)),
        table=climo, label_strides=label_strides, sizes='leads and row')
    n_labels, labels = _climo_labels('verify_skill_map', climo, labels, label_strides, leads, count0, count_dec, row)
    h = _lib.handle(d)
    labels_d = None if labels is None else torch.from_numpy(labels).to(fc.device)
    ws = torch.empty(max(int(_lib.lib.dlwp_verify_skill_map_workspace(h, leads, count0, row, split)), 8), dtype=torch.uint8,
                     device=fc.device)
    sums = torch.empty((leads, SKILL_MAP_SUMS, row), dtype=torch.float64, device=fc.device) if want_sums else None
    scores = torch.empty((leads, SKILL_MAP_SCORES, row), dtype=torch.float32, device=fc.device) if want_scores else None
    counts = torch.empty((leads, row), dtype=torch.int32, device=fc.device) if want_scores else None
    _lib.check(_lib.lib.dlwp_verify_skill_map(h, _ptr(fc), int(fc_strides[0]), int(fc_strides[1]), int(fc_strides[2]),
                                              _ptr(ob), int(ob_strides[0]), int(ob_strides[1]), int(ob_strides[2]),
                                              leads, count0, count_dec, row, _ptr(climo), n_labels, _ptr(labels_d),
                                              int(label_strides[0]), int(label_strides[1]), split, _ptr(sums), _ptr(scores),
                                              _ptr(counts), _ptr(ws), ws.numel(), _stream(fc)))
    return sums, scores, counts


def verify_skill_map_finish(sums):
    """include/dlwp_hip.h: dlwp_verify_skill_map_finish on a (leads, 9, ...) float64 device table (one that was added over ranks or
    sample chunks): one launch per lead on the current stream.  Returns NEW (leads, 6, row) float32 scores and (leads, row) int32
    counts with row = the points of a plane."""
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or not sums.is_contiguous():
        raise TypeError('verify_skill_map_finish: expected a contiguous float64 tensor')
    if sums.dim() < 3 or sums.shape[1] != SKILL_MAP_SUMS or sums.shape[0] < 1 or sums[0, 0].numel() < 1:
        raise ValueError('verify_skill_map_finish: expected (leads >= 1, 9, ...) with non-empty planes, got %r' % (tuple(sums.shape),))
    leads, row = int(sums.shape[0]), int(sums[0, 0].numel())
    h = _lib.handle(_dev(sums))
    scores = torch.empty((leads, SKILL_MAP_SCORES, row), dtype=torch.float32, device=sums.device)
    counts = torch.empty((leads, row), dtype=torch.int32, device=sums.device)
    stream = _stream(sums)
    for f in range(leads):
        _lib.check(_lib.lib.dlwp_verify_skill_map_finish(h, _ptr(sums[f]), row, _ptr(scores[f]), _ptr(counts[f]), stream))
    return scores, counts


SPECTRUM_MIN_WIDTH, SPECTRUM_MAX_WIDTH = 4, 512


def spectrum_twiddles(width):
    """HOST table of dlwp_verify_spectrum_sums: cos(2 pi m / width) for m < width, then sin(2 pi m / width), computed in float64 and
    rounded once to float32"""
    a = 2.0 * np.pi * np.arange(int(width), dtype=np.float64) / float(width)
    return np.concatenate([np.cos(a), np.sin(a)]).astype(np.float32)


_SPECTRUM_TWIDDLES = {}


def _spectrum_twiddles_on(device, width):
    """the table of spectrum_twiddles(width) on `device`, made and uploaded once per (device, width) and never written afterwards"""
    key = (device.index, int(width))
    tw = _SPECTRUM_TWIDDLES.get(key)
    if tw is None:
        tw = _SPECTRUM_TWIDDLES[key] = torch.from_numpy(spectrum_twiddles(width)).to(device)
    return tw


def verify_spectrum_sums(fc, fc_strides, ob, ob_strides, leads, count0, count_dec, groups, run, width, weights=None):
    """include/dlwp_hip.h: dlwp_verify_spectrum_sums.  fc, ob: contiguous float32 device tensors read as flat arrays through
    x_strides = (lead_stride, sample_stride, shift) in elements, as in verify_skill_sums; a group's run is run / width longitude rows
    of `width` floats, 4 <= width <= 512.  weights: a HOST 1-D array, finite, >= 0, not all zero, whose length divides run / width --
    longitude row r of a run has weight weights[r % len(weights)] -- or None.  Everything is checked here (every addressed element
    exists) before anything is uploaded or launched.  Returns NEW device tensors (sums (leads, groups, 4, width // 2 + 1), norm
    (leads, groups, 2)), float64, enqueued on the current stream."""
    _check_f32(fc, ob)
    leads, count0, groups, run, width = int(leads), int(count0), int(groups), int(run), int(width)
    if width < SPECTRUM_MIN_WIDTH or width > SPECTRUM_MAX_WIDTH:
        raise ValueError('verify_spectrum_sums: rows of %d longitudes, the device kernel takes %d .. %d'
                         % (width, SPECTRUM_MIN_WIDTH, SPECTRUM_MAX_WIDTH))
    if run % width:
        raise ValueError('verify_spectrum_sums: rows of %d longitudes do not divide a run of %d' % (width, run))
    if max(count0, 0) * (run // width) >= 2 ** 31 - 32 or leads * groups > 2 ** 20:
        raise ValueError('verify_spectrum_sums: %d longitude rows in a cell, %d cells: at most 2^31 and 2^20'
                         % (max(count0, 0) * (run // width), leads * groups))
    d, leads, count0, count_dec, groups, run = _window_operands('verify_spectrum_sums', leads, count0, count_dec, groups, run,
                                                                (('fc', fc, fc_strides), ('ob', ob, ob_strides)))
    w_len = 0
    if weights is not None:
        weights = skill_weights(weights)
        w_len = int(weights.size)
        if (run // width) % w_len:
            raise ValueError('verify_spectrum_sums: %d weights do not divide the %d longitude rows of a run' % (w_len, run // width))
    h = _lib.handle(d)
    weights_d = None if weights is None else torch.tensor(weights, device=fc.device)      # a copy: the caller's array may be read-only
    tw = _spectrum_twiddles_on(fc.device, width)
    k = width // 2 + 1
    ws = torch.empty(max(int(_lib.lib.dlwp_verify_spectrum_workspace(h, leads, groups, width)), 8), dtype=torch.uint8,
                     device=fc.device)
    sums = torch.empty((leads, groups, 4, k), dtype=torch.float64, device=fc.device)
    norm = torch.empty((leads, groups, 2), dtype=torch.float64, device=fc.device)
    _lib.check(_lib.lib.dlwp_verify_spectrum_sums(h, _ptr(fc), int(fc_strides[0]), int(fc_strides[1]), int(fc_strides[2]),
                                                  _ptr(ob), int(ob_strides[0]), int(ob_strides[1]), int(ob_strides[2]),
                                                  leads, count0, count_dec, groups, run, width, _ptr(weights_d), w_len, _ptr(tw),
                                                  _ptr(sums), _ptr(norm), _ptr(ws), ws.numel(), _stream(fc)))
    return sums, norm


def verify_nanmean_samples(x):
    """include/dlwp_hip.h: dlwp_verify_nanmean_samples.  x: (count, ...) contiguous float32 device tensor -> a NEW float32 tensor
    of x.shape[1:], the NaN-skipping mean over the first axis (float64 sums in sample order; NaN where no sample is finite-or-inf)."""
    _check_f32(x)
    if x.dim() < 2 or x.shape[0] < 1 or x[0].numel() < 1:
        raise ValueError('verify_nanmean_samples: expected (count >= 1, ...) with a non-empty row, got %r' % (tuple(x.shape),))
    mean = torch.empty(tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.dlwp_verify_nanmean_samples(_lib.handle(_dev(x)), _ptr(x), int(x.shape[0]), mean.numel(), _ptr(mean),
                                                    _stream(x)))
    return mean


VERIFY_MAX_LABELS = 64


def label_lists(labels, n_labels):
    """Host side of dlwp_verify_label_nanmean: int labels[count] in [0, n_labels) -> (offsets int32 (n_labels + 1,), index int32
    (count,)): the samples of label l are index[offsets[l]:offsets[l + 1]], ascending.  ValueError for a label out of range."""
    labels = np.asarray(labels)
    n_labels = int(n_labels)
    if labels.ndim != 1 or labels.dtype.kind not in 'iu':
        raise ValueError('label_lists: expected a 1-D integer array, got %s of rank %d' % (labels.dtype, labels.ndim))
    if not 1 <= n_labels <= VERIFY_MAX_LABELS:
        raise ValueError('label_lists: n_labels %d, expected 1 .. %d' % (n_labels, VERIFY_MAX_LABELS))
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= n_labels):
        raise ValueError('label_lists: labels must lie in [0, %d), got %d .. %d' % (n_labels, labels.min(), labels.max()))
    index = np.argsort(labels, kind='stable').astype(np.int32)
    offsets = np.zeros(n_labels + 1, np.int32)
    np.cumsum(np.bincount(labels.astype(np.int64), minlength=n_labels), out=offsets[1:])
    return offsets, index


def _rows_of(x, who):
    if x.dim() < 2 or x.shape[0] < 1 or x[0].numel() < 1:
        raise ValueError('%s: expected (count >= 1, ...) with a non-empty row, got %r' % (who, tuple(x.shape)))
    if x.shape[0] > 0x7fffffff:
        raise ValueError('%s: %d rows, at most 2^31 - 1' % (who, x.shape[0]))
    return int(x.shape[0]), int(x[0].numel())


def verify_label_nanmean_workspace(x, n_labels):
    """bytes of workspace dlwp_verify_label_nanmean needs for x (count, ...) on x's device"""
    count, row = _rows_of(x, 'verify_label_nanmean')
    return int(_lib.lib.dlwp_verify_label_nanmean_workspace(_lib.handle(_dev(x)), count, row, int(n_labels)))


def verify_label_nanmean(x, labels, n_labels, ws=None):
    """include/dlwp_hip.h: dlwp_verify_label_nanmean.  x: (count, ...) contiguous float32 device tensor; labels: HOST integer array
    (count,) in [0, n_labels), checked here before anything is uploaded.  Returns a NEW float32 tensor (n_labels,) + x.shape[1:]: the
    NaN-skipping mean of the rows of each label (NaN for a label without a non-NaN sample).  ws: a uint8 workspace, or None."""
    _check_f32(x)
    count, row = _rows_of(x, 'verify_label_nanmean')
    offsets, index = label_lists(labels, n_labels)
    if index.size != count:
        raise ValueError('verify_label_nanmean: %d labels for %d samples' % (index.size, count))
    h = _lib.handle(_dev(x))
    if ws is None:
        ws = torch.empty(max(verify_label_nanmean_workspace(x, n_labels), 8), dtype=torch.uint8, device=x.device)
    index_d = torch.from_numpy(index).to(x.device)
    mean = torch.empty((int(n_labels),) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.dlwp_verify_label_nanmean(h, _ptr(x), count, row, offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                  _ptr(index_d), int(n_labels), _ptr(mean), _ptr(ws), ws.numel(), _stream(x)))
    return mean


QUANTILE_METHODS = ('linear', 'lower', 'higher', 'nearest')      # DLWP_QUANTILE_* of include/dlwp_hip.h, in that order
QUANTILE_MAX_K = 8


def quantile_probabilities(q, max_k=None, who='verify_label_quantiles'):
    """q (a scalar or a 1-D sequence) as a contiguous float64 array of K >= 1 finite probabilities in [0, 1]; at most max_k of them"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.size < 1:
        raise ValueError('%s: q must be a scalar or a 1-D sequence of at least one probability, got shape %r' % (who, q.shape))
    if not np.all(np.isfinite(q)) or q.min() < 0.0 or q.max() > 1.0:
        raise ValueError('%s: every q must be finite and lie in [0, 1], got %r' % (who, q.tolist()))
    if max_k is not None and q.size > max_k:
        raise ValueError('%s: %d probabilities, at most %d on the device' % (who, q.size, max_k))
    return np.ascontiguousarray(q)


def quantile_method(method, who='verify_label_quantiles'):
    if method not in QUANTILE_METHODS:
        raise ValueError("%s: method %r, expected one of %s" % (who, method, ', '.join(QUANTILE_METHODS)))
    return QUANTILE_METHODS.index(method)


def verify_label_quantiles_plan(max_len, row, route=0, device_index=None):
    """include/dlwp_hip.h: dlwp_verify_label_quantiles_plan.  (route, cols) the kernel takes for a longest label list of max_len rows of
    `row` floats: route 1 (LDS, tiles of cols = 64 / 32 / 16 columns) or 2 (streaming).  Host logic: runs without a GPU."""
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    h = _lib.handle_or_none(device_index)
    _lib.check(_lib.lib.dlwp_verify_label_quantiles_plan(h, int(max_len), int(row), int(route), ctypes.byref(r), ctypes.byref(c)))
    return r.value, c.value


def verify_label_quantiles(x, labels, n_labels, q, method='linear', route=0, want_count=False, ws=None):
    """include/dlwp_hip.h: dlwp_verify_label_quantiles.  x: (count, ...) contiguous float32 device tensor; labels: HOST integer array
    (count,) in [0, n_labels); q: a scalar or up to 8 probabilities in [0, 1]; all of it checked here before anything is uploaded.
    Returns a NEW float32 tensor (K, n_labels) + x.shape[1:], the NaN-skipping quantiles of the rows of each label (NaN where a label
    has no non-NaN sample) -- and with want_count a NEW int32 tensor (n_labels,) + x.shape[1:] of the samples counted.  method:
    'linear' | 'lower' | 'higher' | 'nearest' as in numpy.nanquantile; route: 0 planner, 1 LDS, 2 streaming (same bits)."""
    _check_f32(x)
    m = quantile_method(method)
    q = quantile_probabilities(q, QUANTILE_MAX_K)
    if route not in (0, 1, 2):
        raise ValueError('verify_label_quantiles: route %r, expected 0 (planner), 1 (LDS) or 2 (streaming)' % (route,))
    count, row = _rows_of(x, 'verify_label_quantiles')
    offsets, index = label_lists(labels, n_labels)
    if index.size != count:
        raise ValueError('verify_label_quantiles: %d labels for %d samples' % (index.size, count))
    n_labels, k = int(n_labels), int(q.size)
    h = _lib.handle(_dev(x))
    if ws is None:
        need = int(_lib.lib.dlwp_verify_label_quantiles_workspace(h, count, row, n_labels, k))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    index_d = torch.from_numpy(index).to(x.device)
    out = torch.empty((k, n_labels) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    counts = torch.empty((n_labels,) + tuple(x.shape[1:]), dtype=torch.int32, device=x.device) if want_count else None
    _lib.check(_lib.lib.dlwp_verify_label_quantiles(h, _ptr(x), count, row, offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                    _ptr(index_d), n_labels, q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), k, m,
                                                    int(route), _ptr(out), _ptr(counts), _ptr(ws), ws.numel(), _stream(x)))
    return (out, counts) if want_count else out


def verify_label_error_sums(x, rows, labels, table, anomaly=False, ws=None):
    """include/dlwp_hip.h: dlwp_verify_label_error_sums.  x: (count_x, ...) and table: (n_labels, ...) contiguous float32 device
    tensors with equal rows; rows, labels: HOST integer arrays (m,), checked here against count_x and n_labels before they are
    uploaded.  Returns a NEW (3,) float64 device tensor (sum d^2, sum |d|, pairs counted; d = x[rows[i]] - table[labels[i]], NaN pairs
    skipped) -- and, with anomaly=True, a NEW (m,) + x.shape[1:] float32 tensor of every d."""
    _check_f32(x, table)
    d = _dev(x)
    if _dev(table) != d:
        raise ValueError('verify_label_error_sums: operands on devices %d and %d' % (d, _dev(table)))
    count_x, row = _rows_of(x, 'verify_label_error_sums')
    n_labels, trow = _rows_of(table, 'verify_label_error_sums')
    if trow != row:
        raise ValueError('verify_label_error_sums: rows of %d and %d floats' % (row, trow))
    if n_labels > VERIFY_MAX_LABELS:
        raise ValueError('verify_label_error_sums: %d labels, at most %d' % (n_labels, VERIFY_MAX_LABELS))
    rows, labels = np.asarray(rows), np.asarray(labels)
    if rows.ndim != 1 or labels.shape != rows.shape or rows.size < 1 or rows.dtype.kind not in 'iu' or labels.dtype.kind not in 'iu':
        raise ValueError('verify_label_error_sums: rows and labels must be 1-D integer arrays of one length >= 1')
    if int(rows.min()) < 0 or int(rows.max()) >= count_x:
        raise ValueError('verify_label_error_sums: rows must lie in [0, %d), got %d .. %d' % (count_x, rows.min(), rows.max()))
    if int(labels.min()) < 0 or int(labels.max()) >= n_labels:
        raise ValueError('verify_label_error_sums: labels must lie in [0, %d), got %d .. %d' % (n_labels, labels.min(), labels.max()))
    m = int(rows.size)
    h = _lib.handle(d)
    if ws is None:
        ws = torch.empty(max(int(_lib.lib.dlwp_verify_error_workspace(h, 1, 1)), 8), dtype=torch.uint8, device=x.device)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(x.device)
    labels_d = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(x.device)
    out = torch.empty((m,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device) if anomaly else None
    sums = torch.empty((3,), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib.dlwp_verify_label_error_sums(h, _ptr(x), count_x, row, _ptr(rows_d), _ptr(labels_d), m, _ptr(table), n_labels,
                                                     _ptr(out), _ptr(sums), _ptr(ws), ws.numel(), _stream(x)))
    return (sums, out) if anomaly else sums


def gather_rows_fill(src, rows, out=None):
    """include/dlwp_hip.h: dlwp_gather_rows_fill.  src: (src_rows, ...) contiguous float32 device tensor; rows: HOST integer array of
    any shape, -1 (any negative) for "no such row"; an index >= src_rows is refused here, before the upload.  Returns a NEW float32
    tensor rows.shape + src.shape[1:] (or fills `out` of that size): the rows of src with their bits, NaN rows for the negatives."""
    _check_f32(src, out)
    src_rows, row = _rows_of(src, 'gather_rows_fill')
    rows = np.ascontiguousarray(rows)
    if rows.dtype.kind not in 'iu':
        raise ValueError('gather_rows_fill: rows must be integers, got %s' % rows.dtype)
    rows = rows.astype(np.int64, copy=False)
    if rows.size and int(rows.max()) >= src_rows:
        raise ValueError('gather_rows_fill: row index %d, the source has %d rows' % (rows.max(), src_rows))
    shape = tuple(rows.shape) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif out.numel() != rows.size * row or out.device != src.device:
        raise ValueError('gather_rows_fill: out holds %d elements on %s, expected %d on %s' % (out.numel(), out.device, rows.size * row,
                                                                                               src.device))
    rows_d = torch.from_numpy(rows.reshape(-1)).to(src.device)
    _lib.check(_lib.lib.dlwp_gather_rows_fill(_lib.handle(_dev(src)), _ptr(src), src_rows, row, _ptr(rows_d), int(rows.size), _ptr(out),
                                              _stream(src)))
    return out


# -- ensemble verification (csrc/ensemble.hip) --------------------------------------------------------------------------------------- #
ENS_MAX_MEMBERS = 256


def ens_strides(samples, members, row, member_axis=2):
    """(lead_stride, sample_stride, member_stride) in elements of a contiguous series viewed as (T, S, M, row) (member_axis=2) or
    (T, M, S, row) (member_axis=1): the table of include/dlwp_hip.h"""
    samples, members, row = int(samples), int(members), int(row)
    if member_axis == 2:
        return samples * members * row, members * row, row
    if member_axis == 1:
        return members * samples * row, row, samples * row
    raise ValueError("'member_axis' must be 1 or 2, got %r" % (member_axis,))


def ens_extent(strides, leads, samples, members, row):
    """Elements the ensemble operand must hold: one past the last offset the strides address"""
    ls, ss, ms = (int(v) for v in strides)
    return (int(leads) - 1) * ls + (int(samples) - 1) * ss + (int(members) - 1) * ms + int(row)


def _ens_check(who, x, strides, leads, samples, members, row):
    if leads < 1 or samples < 1 or row < 1 or min(strides) < 0:
        raise ValueError('%s: leads, samples and the row must be >= 1 and the strides >= 0' % who)
    need = ens_extent(strides, leads, samples, members, row)
    if need > x.numel():
        raise ValueError('%s: the ensemble holds %d elements, the strides address %d' % (who, x.numel(), need))


def ens_mean_spread(x, strides, leads, samples, members, row, ddof=1, want_mean=True, want_spread=True):
    """include/dlwp_hip.h: dlwp_ens_mean_spread.  x: contiguous float32 device tensor read as a flat array through strides =
    (lead_stride, sample_stride, member_stride) in elements.  Returns NEW float32 tensors (mean, spread) of shape (leads, samples,
    row) (None for the one not wanted), enqueued on the current stream."""
    _check_f32(x)
    d = _dev(x)
    leads, samples, members, row, ddof = int(leads), int(samples), int(members), int(row), int(ddof)
    if members < 2:
        raise ValueError('ens_mean_spread: %d members, at least 2' % members)
    if ddof not in (0, 1):
        raise ValueError('ens_mean_spread: ddof must be 0 or 1, got %d' % ddof)
    if not (want_mean or want_spread):
        raise ValueError('ens_mean_spread: neither the mean nor the spread is wanted')
    _ens_check('ens_mean_spread', x, strides, leads, samples, members, row)
    mean = torch.empty((leads, samples, row), dtype=torch.float32, device=x.device) if want_mean else None
    spread = torch.empty((leads, samples, row), dtype=torch.float32, device=x.device) if want_spread else None
    _lib.check(_lib.lib.dlwp_ens_mean_spread(_lib.handle(d), _ptr(x), leads, samples, members, int(strides[0]), int(strides[1]),
                                             int(strides[2]), row, ddof, _ptr(mean), _ptr(spread), _stream(x)))
    return mean, spread


def ens_score_workspace(device_index, leads, groups, members):
    """bytes of workspace dlwp_ens_score_sums needs on that device (any sample count)"""
    return int(_lib.lib.dlwp_ens_score_workspace(_lib.handle(int(device_index)), int(leads), int(groups), int(members)))


def ens_score_sums(x, strides, y, leads, samples, members, groups, run, crps_field=False, ws=None):
    """include/dlwp_hip.h: dlwp_ens_score_sums.  x: the ensemble as in ens_mean_spread; y: contiguous float32 device tensor of
    leads * samples * groups * run elements.  Returns NEW device tensors (sums (leads, groups, 6) float64, hist (leads, groups,
    members + 1) int64) and, with crps_field, the per-column crps (leads, samples, groups * run) float32 as a third."""
    _check_f32(x, y)
    d = _dev(x)
    if _dev(y) != d:
        raise ValueError('ens_score_sums: operands on devices %d and %d' % (d, _dev(y)))
    leads, samples, members, groups, run = int(leads), int(samples), int(members), int(groups), int(run)
    if not 2 <= members <= ENS_MAX_MEMBERS:
        raise ValueError('ens_score_sums: %d members, expected 2 .. %d' % (members, ENS_MAX_MEMBERS))
    if groups < 1 or run < 1:
        raise ValueError('ens_score_sums: groups and run must be >= 1')
    _ens_check('ens_score_sums', x, strides, leads, samples, members, groups * run)
    if y.numel() != leads * samples * groups * run:
        raise ValueError('ens_score_sums: the verification holds %d elements, expected %d' % (y.numel(), leads * samples * groups * run))
    h = _lib.handle(d)
    need = max(int(_lib.lib.dlwp_ens_score_workspace(h, leads, groups, members)), 8)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif ws.numel() * ws.element_size() < need or ws.device != x.device:
        raise ValueError('ens_score_sums: the workspace holds %d bytes on %s, expected %d on %s' % (ws.numel() * ws.element_size(),
                                                                                                  ws.device, need, x.device))
    sums = torch.empty((leads, groups, 6), dtype=torch.float64, device=x.device)
    hist = torch.empty((leads, groups, members + 1), dtype=torch.int64, device=x.device)
    crps = torch.empty((leads, samples, groups * run), dtype=torch.float32, device=x.device) if crps_field else None
    _lib.check(_lib.lib.dlwp_ens_score_sums(h, _ptr(x), int(strides[0]), int(strides[1]), int(strides[2]), _ptr(y), leads, samples,
                                            members, groups, run, _ptr(sums), _ptr(hist), _ptr(crps), _ptr(ws),
                                            ws.numel() * ws.element_size(), _stream(x)))
    return (sums, hist, crps) if crps_field else (sums, hist)


# -- ensemble event verification (csrc/events.hip) ----------------------------------------------------------------------------------- #
ENS_MAX_THRESHOLDS = 8


def ens_event_workspace(device_index, leads, groups, members, thresholds):
    """bytes of workspace dlwp_ens_event_counts needs on that device for a table (any sample count)"""
    return int(_lib.lib.dlwp_ens_event_workspace(_lib.handle(int(device_index)), int(leads), int(groups), int(members), int(thresholds)))


def ens_event_counts(x, strides, y, thr, per_point, below, leads, samples, members, groups, run, want_table=True, want_prob=False,
                     ws=None):
    """include/dlwp_hip.h: dlwp_ens_event_counts.  x: the ensemble as in ens_mean_spread; y: contiguous float32 device tensor of
    leads * samples * groups * run elements (None where no table is wanted); thr: contiguous float32 device tensor whose first axis
    is the K thresholds, K * groups elements, or K * groups * run with per_point.  Returns NEW device tensors (table (leads, groups,
    K, members + 1, 2) int64 or None, prob (K, leads, samples, groups * run) float32 or None)."""
    if not (want_table or want_prob):
        raise ValueError('ens_event_counts: neither the table nor the probability field is wanted')
    if want_table and y is None:
        raise ValueError('ens_event_counts: the table needs the verification y')
    y = y if want_table else None
    _check_f32(*(t for t in (x, y, thr) if t is not None))
    d = _dev(x)
    for t in (y, thr):
        if t is not None and _dev(t) != d:
            raise ValueError('ens_event_counts: operands on devices %d and %d' % (d, _dev(t)))
    leads, samples, members, groups, run = int(leads), int(samples), int(members), int(groups), int(run)
    if not 2 <= members <= ENS_MAX_MEMBERS:
        raise ValueError('ens_event_counts: %d members, expected 2 .. %d' % (members, ENS_MAX_MEMBERS))
    if groups < 1 or run < 1:
        raise ValueError('ens_event_counts: groups and run must be >= 1')
    k_n = int(thr.shape[0]) if thr.dim() >= 1 else 0
    if not 1 <= k_n <= ENS_MAX_THRESHOLDS:
        raise ValueError('ens_event_counts: %d thresholds, expected 1 .. %d' % (k_n, ENS_MAX_THRESHOLDS))
    _ens_check('ens_event_counts', x, strides, leads, samples, members, groups * run)
    if y is not None and y.numel() != leads * samples * groups * run:
        raise ValueError('ens_event_counts: the verification holds %d elements, expected %d' % (y.numel(), leads * samples * groups * run))
    thr_need = k_n * groups * (run if per_point else 1)
    if thr.numel() != thr_need:
        raise ValueError('ens_event_counts: the thresholds hold %d elements, expected %d (%s)'
                         % (thr.numel(), thr_need, 'K x groups x run' if per_point else 'K x groups'))
    h = _lib.handle(d)
    table = prob = None
    ws_bytes = 0
    if want_table:
        need = max(int(_lib.lib.dlwp_ens_event_workspace(h, leads, groups, members, k_n)), 4)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        elif ws.numel() * ws.element_size() < need or ws.device != x.device:
            raise ValueError('ens_event_counts: the workspace holds %d bytes on %s, expected %d on %s' % (ws.numel() * ws.element_size(),
                                                                                                        ws.device, need, x.device))
        ws_bytes = ws.numel() * ws.element_size()
        table = torch.empty((leads, groups, k_n, members + 1, 2), dtype=torch.int64, device=x.device)
    else:
        ws = None
    if want_prob:
        prob = torch.empty((k_n, leads, samples, groups * run), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.dlwp_ens_event_counts(h, _ptr(x), int(strides[0]), int(strides[1]), int(strides[2]), _ptr(y), _ptr(thr),
                                              1 if per_point else 0, 1 if below else 0, leads, samples, members, groups, run, k_n,
                                              _ptr(table), _ptr(prob), _ptr(ws), ws_bytes, _stream(x)))
    return table, prob


# -- the ensemble member generator (csrc/perturb.hip) -------------------------------------------------------------------------------- #
ENS_MAX_RADIUS = _lib.ENS_MAX_RADIUS


def ens_perturb_desc(samples, channels, height, width, members, first_member, seed, taps_y, taps_x, control, antithetic,
                     sample_stride, member_stride):
    """The by-value descriptor of dlwp_ens_perturb; taps_*: odd-length float32 tables (model.ensemble.smoothing_taps)."""
    d = _lib.EnsPerturb()
    d.samples, d.channels, d.height, d.width = int(samples), int(channels), int(height), int(width)
    d.members, d.first_member, d.seed = int(members), int(first_member), int(seed) & 0xffffffffffffffff
    for name, taps in (('y', taps_y), ('x', taps_x)):
        taps = np.asarray(taps, dtype=np.float32).reshape(-1)
        if taps.size % 2 != 1 or taps.size > 2 * ENS_MAX_RADIUS + 1:
            raise ValueError('ens_perturb: %d taps on axis %s, expected an odd count up to %d' % (taps.size, name, 2 * ENS_MAX_RADIUS + 1))
        setattr(d, 'radius_' + name, taps.size // 2)
        table = getattr(d, 'taps_' + name)
        for i, v in enumerate(taps.tolist()):
            table[i] = v
    d.control, d.antithetic = int(bool(control)), int(bool(antithetic))
    d.sample_stride, d.member_stride = int(sample_stride), int(member_stride)
    return d


def ens_perturb(x, sigma, members, first_member=0, seed=0, taps_y=(1.0,), taps_x=(1.0,), control=True, antithetic=False,
                member_axis=2, out=None):
    """include/dlwp_hip.h: dlwp_ens_perturb.  x: contiguous float32 device tensor (S, K, H, W); sigma: float32 device tensor of K
    elements.  Returns a float32 tensor (S, M, K, H, W) (member_axis=2) or (M, S, K, H, W) (member_axis=1), new or `out` (any
    contiguous float32 tensor of that many elements), enqueued on the current stream."""
    _check_f32(x, sigma, out)
    d = _dev(x)
    if x.dim() != 4:
        raise ValueError('ens_perturb: x must be (samples, channels, height, width), got %r' % (tuple(x.shape),))
    s_n, k_n, h_n, w_n = (int(v) for v in x.shape)
    members = int(members)
    if members < 1:
        raise ValueError('ens_perturb: %d members, at least 1' % members)
    if _dev(sigma) != d or sigma.numel() != k_n:
        raise ValueError('ens_perturb: sigma holds %d elements on device %d, expected %d on device %d' % (sigma.numel(), _dev(sigma), k_n, d))
    row = k_n * h_n * w_n
    _, sample_stride, member_stride = ens_strides(s_n, members, row, member_axis)
    desc = ens_perturb_desc(s_n, k_n, h_n, w_n, members, first_member, seed, taps_y, taps_x, control, antithetic, sample_stride,
                            member_stride)
    shape = (s_n, members, k_n, h_n, w_n) if member_axis == 2 else (members, s_n, k_n, h_n, w_n)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif out.numel() != s_n * members * row or out.device != x.device:
        raise ValueError('ens_perturb: out holds %d elements on %s, expected %d on %s' % (out.numel(), out.device, s_n * members * row,
                                                                                        x.device))
    _lib.check(_lib.lib.dlwp_ens_perturb(_lib.handle(d), _ptr(x), _ptr(sigma), _ptr(out), desc, _stream(x)))
    return out.view(shape)


# -- batches of a series generator out of an HBM-resident series (csrc/series.hip) --------------------------------------------------- #
SERIES_CHUNK_UNITS = 1024          # units (16 bytes, or one float on the scalar path) a block moves per turn


def series_window_gather_host(plan, samples):
    """The segment table of include/dlwp_hip.h: dlwp_series_window_gather restated in numpy -- the kernel's oracle and what the CPU
    tests compare with SeriesDataGenerator.generate.  plan: sources (2-D float32 arrays), shapes, segments (model.generators.
    WindowPlan); samples: integer start positions.  Returns [X, y0, ...] as float32 arrays (n,) + shape.  Bits are copied as words;
    a run whose first or last time is no row of its source is filled with quiet NaNs (0x7fc00000)."""
    samples = np.asarray(samples).reshape(-1).astype(np.int64)
    n = samples.size
    outs = [np.zeros((n, int(np.prod(s))), np.uint32) for s in plan.shapes]
    for src, dst, shift, src_at, dst_at, ln in np.asarray(plan.segments, dtype=np.int64).reshape(-1, 6).tolist():
        a = plan.sources[src]
        rows, row = a.shape
        flat = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)
        span = (src_at + ln - 1) // row
        for i in range(n):
            t = int(samples[i]) + shift
            if t < 0 or t + span > rows - 1:
                outs[dst][i, dst_at:dst_at + ln] = 0x7fc00000
            else:
                outs[dst][i, dst_at:dst_at + ln] = flat[t * row + src_at:t * row + src_at + ln]
    return [o.view(np.float32).reshape((n,) + tuple(s)) for o, s in zip(outs, plan.shapes)]


def series_chunks(segments, vec):
    """chunks of SERIES_CHUNK_UNITS units that one sample of a segment table is cut into (the launch is n * this many block turns)"""
    w = 4 if vec else 1
    return sum((int(s[5]) // w + SERIES_CHUNK_UNITS - 1) // SERIES_CHUNK_UNITS for s in np.asarray(segments).reshape(-1, 6))


def series_grid_cap(device=None):
    """blocks the launch of dlwp_series_window_gather is capped at on `device` (the library's own figure)"""
    idx = torch.cuda.current_device() if device is None or torch.device(device).index is None else torch.device(device).index
    return int(_lib.lib.dlwp_series_gather_grid_cap(_lib.handle(idx)))


class SeriesTables(object):
    """The descriptor tables of one dlwp_series_window_gather call site, built once: sources and destinations are device tensors
    that this object keeps alive; a launch only adds the sample positions.  dsts[d] is (capacity, row): a launch of n <= capacity
    samples fills its first n rows."""

    def __init__(self, srcs, dsts, segments):
        srcs, dsts = list(srcs), list(dsts)
        segments = np.ascontiguousarray(segments, dtype=np.int64).reshape(-1, 6)
        if not 1 <= len(srcs) <= _lib.SERIES_MAX_SRCS or not 1 <= len(dsts) <= _lib.SERIES_MAX_DSTS or \
                not 1 <= len(segments) <= _lib.SERIES_MAX_SEGS:
            raise ValueError('series_window_gather: %d sources, %d destinations, %d segments; at most %d, %d, %d and at least one of each'
                             % (len(srcs), len(dsts), len(segments), _lib.SERIES_MAX_SRCS, _lib.SERIES_MAX_DSTS, _lib.SERIES_MAX_SEGS))
        _check_f32(*(srcs + dsts))
        self.device = srcs[0].device
        dev = _dev(srcs[0])
        for t in srcs + dsts:
            if _dev(t) != dev:
                raise ValueError('series_window_gather: tensors on devices %d and %d' % (dev, _dev(t)))
            if t.dim() != 2 or t.shape[1] < 1:
                raise ValueError('series_window_gather: expected 2-D (rows, row) tensors, got %r' % (tuple(t.shape),))
        if any(t.shape[0] < 1 for t in srcs):
            raise ValueError('series_window_gather: a source without rows')
        self.capacity = min(int(t.shape[0]) for t in dsts)
        for g, (src, dst, shift, src_at, dst_at, ln) in enumerate(segments.tolist()):
            if not (0 <= src < len(srcs) and 0 <= dst < len(dsts)):
                raise ValueError('series_window_gather: segment %d names source %d, destination %d' % (g, src, dst))
            if ln < 1 or not 0 <= src_at < srcs[src].shape[1] or dst_at < 0 or dst_at + ln > dsts[dst].shape[1]:
                raise ValueError('series_window_gather: segment %d (src_at %d, dst_at %d, len %d) leaves its rows' % (g, src_at, dst_at, ln))
        self.keep = (srcs, dsts)
        self.n_src, self.n_dst, self.n_seg = len(srcs), len(dsts), len(segments)
        self.srcs = (_lib.SeriesSrc * len(srcs))(*[_lib.SeriesSrc(t.data_ptr(), int(t.shape[0]), int(t.shape[1])) for t in srcs])
        self.dsts = (_lib.SeriesDst * len(dsts))(*[_lib.SeriesDst(t.data_ptr(), int(t.shape[1])) for t in dsts])
        self.segs = (_lib.SeriesSeg * len(segments))(*[_lib.SeriesSeg(*[int(v) for v in s]) for s in segments.tolist()])
        self.handle = _lib.handle(dev)
        self.vec = all(t.data_ptr() % 16 == 0 and t.shape[1] % 4 == 0 for t in srcs + dsts) and \
            bool((segments[:, 3:] % 4 == 0).all())

    def launch(self, samples, n=None, offset=0):
        """samples: int64 device tensor; positions offset .. offset + n of it start the n samples.  Enqueued on the current stream."""
        n = int(samples.numel() - offset if n is None else n)
        offset = int(offset)
        if samples.dtype != torch.int64 or not samples.is_contiguous() or samples.device != self.device:
            raise ValueError('series_window_gather: samples must be a contiguous int64 tensor on %s' % (self.device,))
        if n < 0 or offset < 0 or offset + n > samples.numel() or n > self.capacity:
            raise ValueError('series_window_gather: %d samples from position %d of %d into destinations of %d rows'
                             % (n, offset, samples.numel(), self.capacity))
        _lib.check(_lib.lib.dlwp_series_window_gather(self.handle, self.srcs, self.n_src, self.dsts, self.n_dst, self.segs, self.n_seg,
                                                      ctypes.c_void_p(samples.data_ptr() + 8 * offset), n, _stream(samples)))


def series_window_gather(srcs, segments, shapes, samples, out=None):
    """include/dlwp_hip.h: dlwp_series_window_gather.  srcs: float32 device tensors (rows, ...) (their rows flattened); segments:
    HOST int64 (n_seg, 6) table of src, dst, shift, src_at, dst_at, len; shapes: per-sample shapes of the destinations; samples:
    integer start positions, a host array (uploaded here) or an int64 device tensor.  Returns NEW float32 tensors (n,) + shape --
    or fills `out`, 2-D (>= n, row) tensors -- on the current stream.  Times outside a source give quiet-NaN runs."""
    if not isinstance(samples, torch.Tensor):
        samples = np.ascontiguousarray(samples)
        if samples.dtype.kind not in 'iu':
            raise ValueError('series_window_gather: samples must be integers, got %s' % samples.dtype)
        samples = torch.from_numpy(samples.reshape(-1).astype(np.int64)).to(srcs[0].device)
    n = int(samples.numel())
    rows = [int(np.prod(s)) for s in shapes]
    made = out is None
    if made:
        out = [torch.empty((max(n, 1), r), dtype=torch.float32, device=srcs[0].device) for r in rows]
    elif len(out) != len(rows) or any(o.dim() != 2 or o.shape[1] != r for o, r in zip(out, rows)):
        raise ValueError('series_window_gather: out must hold one (n, row) tensor per destination')
    SeriesTables([s.reshape(s.shape[0], -1) for s in srcs], out, segments).launch(samples, n)
    return [o[:n].view((n,) + tuple(s)) for o, s in zip(out, shapes)] if made else out
