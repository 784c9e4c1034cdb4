// tconv.hip -- keras Conv2DTranspose(filters, k, strides=2), restated as a stride-1 convolution on the layer's own input.
//
// Definition (channels_first, kernel K (kh, kw, F, cin), no flip):  y_full[n][o][2i+u][2j+v] += x[n][c][i][j] * K[u][v][o][c].
// Output pixel (2i'+a, 2j'+b) only receives the taps u = a, a+2, ... and v = b, b+2, ...: with T = ceil(k / 2) per axis, phase
// (a, b) of y_full is a stride-1 cross-correlation of x (zero halo T-1 on every side) with
//   w2[ti][tj][c][(2a+b)*F + o] = K[a + 2(Th-1-ti)][b + 2(Tw-1-tj)][o][c]      (zero where that index is >= kh / kw)
// -- a permutation with zero fill, no sums.  The 4 phases read the same window, so the layer runs as ONE convolution with 4 F
// phase-major output channels on the existing forward / data-gradient / weight-gradient kernels (as phase.hip does for a
// convolution on an up-sampled tensor), followed by an interleave that also crops ('same' padding, the extra row / column of an
// odd kernel, a Cropping2D folded in behind the layer):
//   dlwp_tconv_weights:          K, bias -> w2 (Th, Tw, cin, 4F), b2 (4F)
//   dlwp_tconv_weights_bwd:      dw2 -> dK: every element of K sits in exactly one element of w2, a pure gather
//   dlwp_depth_to_space2_crop:   (n, 4F, hp, wp) -> (n, c_total, H, W)[c_off:+F], out (r, s) = phase ((r+top)&1, (s+left)&1) at
//                                ((r+top)>>1, (s+left)>>1)
//   dlwp_space_to_depth2_fill:   its adjoint; EVERY element of the phase gradient is written, +0 where the crop dropped it
// All four move and zero-fill only: bit-exact by construction.
//
// The derived kernel may be stored with MORE taps than T: (Sh, Sw, cin, 4F), Sh >= Th, Sw >= Tw, the Th x Tw block at offset
// ((Sh - Th) / 2, (Sw - Tw) / 2) and zeros around it -- the library's matrix-core forward and weight-gradient kernels exist for
// 3 x 3 and 5 x 5 taps, so the planner stores 3 x 3 (k <= 6) or 5 x 5 (k <= 10) taps and widens the zero halo to match: a zero tap
// times anything finite adds +-0, the sums are those of the T x T kernel.
//
// Access pattern of the two interleaves (HBM-bound, float32): one lane moves 4 phase pixels of each of the two column phases of
// one phase row = 8 output pixels of one output row, as 2 + 2 16-byte accesses, where wp % 4 == 0, left % 4 == 0, W % 4 == 0 and
// both pointers are 16-byte aligned (then every quad of output pixels is wholly inside or wholly outside the crop, and every
// access is aligned); element accesses otherwise, one lane per phase pixel and its 2 x 2 output pixels, as dlwp_depth_to_space2.
#include "common.h"
#include "tape.h"

namespace {

__global__ __launch_bounds__(256) void tconv_weights_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ w2, float* __restrict__ b2, int kh, int kw,
                                                            int cin, int F, int Th, int Tw, int Sh, int Sw) {
  const long long total = (long long)Sh * Sw * cin * 4 * F;
  const int oh = (Sh - Th) / 2, ow = (Sw - Tw) / 2;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int col = (int)(e % (4 * F));
    long long q = e / (4 * F);
    const int c = (int)(q % cin);
    q /= cin;
    const int tj = (int)(q % Sw) - ow, ti = (int)(q / Sw) - oh;
    const int ph = col / F, o = col - ph * F;
    const int u = (ph >> 1) + 2 * (Th - 1 - ti), v = (ph & 1) + 2 * (Tw - 1 - tj);
    const bool in = ti >= 0 && ti < Th && tj >= 0 && tj < Tw && u < kh && v < kw;
    w2[e] = in ? w[((long long)(u * kw + v) * F + o) * cin + c] : 0.f;
  }
  if (b2 && blockIdx.x == 0)
    for (int c = threadIdx.x; c < 4 * F; c += 256) b2[c] = bias ? bias[c % F] : 0.f;
}

// dK[u][v][o][c] (+)= dw2[oh + Th-1-(u>>1)][ow + Tw-1-(v>>1)][c][(2(u&1) + (v&1))*F + o]
__global__ __launch_bounds__(256) void tconv_weights_bwd_kernel(const float* __restrict__ dw2, float* __restrict__ dw, int kh,
                                                                int kw, int cin, int F, int Th, int Tw, int Sh, int Sw,
                                                                int accumulate) {
  const long long total = (long long)kh * kw * F * cin;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e % cin);
    long long q = e / cin;
    const int o = (int)(q % F);
    q /= F;
    const int v = (int)(q % kw), u = (int)(q / kw);
    const int si = (Sh - Th) / 2 + Th - 1 - (u >> 1), sj = (Sw - Tw) / 2 + Tw - 1 - (v >> 1);
    const float g = dw2[(((long long)si * Sw + sj) * cin + c) * (4 * F) + (2 * (u & 1) + (v & 1)) * F + o];
    dw[e] = accumulate ? dw[e] + g : g;
  }
}

struct D2sGeom {
  int F, hp, wp, top, left, H, W, c_off, c_total;
};

// one lane per PHASE pixel (n, co, i, j): its 4 values, one per phase plane (coalesced loads), go to the 2 x 2 output pixels at
// (2i - top, 2j - left) that the crop keeps; the two column phases of a row are neighbours (8 contiguous bytes per lane)
__global__ __launch_bounds__(256) void d2s_crop_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total,
                                                       D2sGeom g) {
  const long long plane = (long long)g.hp * g.wp, fp = (long long)g.F * plane;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int j = (int)(e % g.wp);
    long long q = e / g.wp;
    const int i = (int)(q % g.hp);
    q /= g.hp;
    const int co = (int)(q % g.F);
    const long long n = q / g.F;
    const int r0 = 2 * i - g.top, c0 = 2 * j - g.left;
    const bool ra = r0 >= 0 && r0 < g.H, rb = r0 + 1 >= 0 && r0 + 1 < g.H;
    const bool ca = c0 >= 0 && c0 < g.W, cb = c0 + 1 >= 0 && c0 + 1 < g.W;
    const float* s = src + (n * 4 * g.F + co) * plane + (long long)i * g.wp + j;
    const long long d = ((n * g.c_total + g.c_off + co) * g.H + r0) * (long long)g.W + c0;     // (used only where in range)
    if (ra && ca) dst[d] = s[0];
    if (ra && cb) dst[d + 1] = s[fp];
    if (rb && ca) dst[d + g.W] = s[2 * fp];
    if (rb && cb) dst[d + g.W + 1] = s[3 * fp];
  }
}

// one lane per 4 phase pixels of the two column phases of one OUTPUT row: 8 output pixels (see the header for the conditions)
__global__ __launch_bounds__(256) void d2s_crop_vec_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           long long total, D2sGeom g) {
  const long long plane = (long long)g.hp * g.wp;
  const int quads = g.wp >> 2;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int qd = (int)(e % quads);
    long long q = e / quads;
    const int r = (int)(q % g.H);
    q /= g.H;
    const int co = (int)(q % g.F);
    const long long n = q / g.F;
    const int c0 = 8 * qd - g.left;                 // first of the 8 output columns (a multiple of 4)
    if (c0 + 8 <= 0 || c0 >= g.W) continue;
    const int rr = r + g.top;
    const float* s0 = src + (n * 4 * g.F + (long long)(2 * (rr & 1)) * g.F + co) * plane + (long long)(rr >> 1) * g.wp + 4 * qd;
    const float4 e0 = *reinterpret_cast<const float4*>(s0);                             // column phase 0
    const float4 e1 = *reinterpret_cast<const float4*>(s0 + (long long)g.F * plane);    // column phase 1
    float* d = dst + ((n * g.c_total + g.c_off + co) * g.H + r) * (long long)g.W + c0;
    if (c0 >= 0) *reinterpret_cast<float4*>(d) = make_float4(e0.x, e1.x, e0.y, e1.y);
    if (c0 + 8 <= g.W) *reinterpret_cast<float4*>(d + 4) = make_float4(e0.z, e1.z, e0.w, e1.w);
  }
}

// one lane per PHASE pixel (n, co, i, j): the 2 x 2 gradient pixels at (2i - top, 2j - left), +0 where the crop dropped one, to the 4
// phase planes (coalesced stores)
__global__ __launch_bounds__(256) void s2d_fill_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total,
                                                       D2sGeom g) {
  const long long plane = (long long)g.hp * g.wp, fp = (long long)g.F * plane;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int j = (int)(e % g.wp);
    long long q = e / g.wp;
    const int i = (int)(q % g.hp);
    q /= g.hp;
    const int co = (int)(q % g.F);
    const long long n = q / g.F;
    const int r0 = 2 * i - g.top, c0 = 2 * j - g.left;
    const bool ra = r0 >= 0 && r0 < g.H, rb = r0 + 1 >= 0 && r0 + 1 < g.H;
    const bool ca = c0 >= 0 && c0 < g.W, cb = c0 + 1 >= 0 && c0 + 1 < g.W;
    const long long o = ((n * g.c_total + g.c_off + co) * g.H + r0) * (long long)g.W + c0;     // (used only where in range)
    const float v00 = (ra && ca) ? src[o] : 0.f, v01 = (ra && cb) ? src[o + 1] : 0.f;
    const float v10 = (rb && ca) ? src[o + g.W] : 0.f, v11 = (rb && cb) ? src[o + g.W + 1] : 0.f;
    float* d = dst + (n * 4 * g.F + co) * plane + (long long)i * g.wp + j;
    d[0] = v00;
    d[fp] = v01;
    d[2 * fp] = v10;
    d[3 * fp] = v11;
  }
}

// one lane per 4 phase pixels of both column phases of one phase row (a, i): 8 gradient pixels of one row, or zeros
__global__ __launch_bounds__(256) void s2d_fill_vec_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           long long total, D2sGeom g) {
  const long long plane = (long long)g.hp * g.wp;
  const int quads = g.wp >> 2;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int qd = (int)(e % quads);
    long long q = e / quads;
    const int i = (int)(q % g.hp);
    q /= g.hp;
    const int a = (int)(q & 1);
    q >>= 1;
    const int co = (int)(q % g.F);
    const long long n = q / g.F;
    const int r = 2 * i + a - g.top, c0 = 8 * qd - g.left;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (r >= 0 && r < g.H) {
      const float* s = src + ((n * g.c_total + g.c_off + co) * g.H + r) * (long long)g.W + c0;
      if (c0 >= 0 && c0 + 4 <= g.W) lo = *reinterpret_cast<const float4*>(s);
      if (c0 + 4 >= 0 && c0 + 8 <= g.W) hi = *reinterpret_cast<const float4*>(s + 4);
    }
    float* d = dst + (n * 4 * g.F + (long long)(2 * a) * g.F + co) * plane + (long long)i * g.wp + 4 * qd;
    *reinterpret_cast<float4*>(d) = make_float4(lo.x, lo.z, hi.x, hi.z);
    *reinterpret_cast<float4*>(d + (long long)g.F * plane) = make_float4(lo.y, lo.w, hi.y, hi.w);
  }
}

bool vec_ok(const void* a, const void* b, const D2sGeom& g) {
  return g.wp % 4 == 0 && g.left % 4 == 0 && g.W % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

int check_interleave(const char* who, dlwp_handle_t h, const void* src, const void* dst, int n, int f, int hp, int wp, int top,
                     int left, int H, int W, int c_off, int c_total, int dtype) {
  // (shape checks first: they need no device, and a wrong crop must never reach a launch)
  DLWP_CHECK_ARG(dtype == DLWP_F32 && n >= 0 && f > 0 && hp > 0 && wp > 0 && H > 0 && W > 0 && c_off >= 0 && c_off + f <= c_total,
                 "%s: bad arguments", who);
  DLWP_CHECK_ARG(top >= 0 && left >= 0 && (long long)top + H <= 2ll * hp && (long long)left + W <= 2ll * wp,
                 "%s: the crop (top %d, left %d, %d x %d) is larger than the interleaved tensor %d x %d", who, top, left, H, W,
                 2 * hp, 2 * wp);
  DLWP_CHECK_ARG(h && (n == 0 || (src && dst)), "%s: null handle or pointer", who);
  return DLWP_OK;
}

int grid_of(dlwp_handle_t h, long long total) {
  const long long blocks = (total + 255) / 256, cap = (long long)h->cu_count * 16;
  return (int)(blocks < cap ? blocks : cap);
}

}  // namespace

extern "C" {

// per axis: T = ceil(k / 2) taps on the source, the crop offset into the interleaved phase tensor and the output length
int dlwp_tconv_geometry(int k, int same, int len, int* t, int* crop, int* out_len) {
  DLWP_CHECK_ARG(k > 0 && len > 0 && t && crop && out_len, "dlwp_tconv_geometry: bad arguments");
  const int extra = k > 2 ? k - 2 : 0;
  *t = (k + 1) / 2;
  *crop = same ? extra / 2 : 0;
  *out_len = same ? 2 * len : 2 * len + extra;
  return DLWP_OK;
}

int dlwp_tconv_weights(dlwp_handle_t h, const void* w, const void* bias, void* w2, void* b2, int kh, int kw, int cin, int f,
                       int sh, int sw, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_tconv_weights, h, w, bias, w2, b2, kh, kw, cin, f, sh, sw, dtype);
  DLWP_CHECK_ARG(dtype == DLWP_F32 && kh > 0 && kw > 0 && cin > 0 && f > 0, "dlwp_tconv_weights: bad arguments");
  DLWP_CHECK_ARG(sh >= (kh + 1) / 2 && sw >= (kw + 1) / 2 && sh <= 64 && sw <= 64,
                 "dlwp_tconv_weights: %d x %d stored taps do not hold the %d x %d taps of a %d x %d kernel", sh, sw, (kh + 1) / 2,
                 (kw + 1) / 2, kh, kw);
  DLWP_CHECK_ARG(h && w && w2, "dlwp_tconv_weights: null handle or pointer");
  const int Th = (kh + 1) / 2, Tw = (kw + 1) / 2;
  const long long total = (long long)sh * sw * cin * 4 * f;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  tconv_weights_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>((const float*)w, (const float*)bias, (float*)w2,
                                                                      (float*)b2, kh, kw, cin, f, Th, Tw, sh, sw);
  DLWP_LAUNCH_CHECK("tconv_weights_kernel");
  return DLWP_OK;
}

int dlwp_tconv_weights_bwd(dlwp_handle_t h, const void* dw2, void* dw, int kh, int kw, int cin, int f, int sh, int sw,
                           int accumulate, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_tconv_weights_bwd, h, dw2, dw, kh, kw, cin, f, sh, sw, accumulate, dtype);
  DLWP_CHECK_ARG(dtype == DLWP_F32 && kh > 0 && kw > 0 && cin > 0 && f > 0, "dlwp_tconv_weights_bwd: bad arguments");
  DLWP_CHECK_ARG(sh >= (kh + 1) / 2 && sw >= (kw + 1) / 2 && sh <= 64 && sw <= 64,
                 "dlwp_tconv_weights_bwd: %d x %d stored taps do not hold the %d x %d taps of a %d x %d kernel", sh, sw,
                 (kh + 1) / 2, (kw + 1) / 2, kh, kw);
  DLWP_CHECK_ARG(h && dw2 && dw, "dlwp_tconv_weights_bwd: null handle or pointer");
  const int Th = (kh + 1) / 2, Tw = (kw + 1) / 2;
  const long long total = (long long)kh * kw * f * cin;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  tconv_weights_bwd_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>((const float*)dw2, (float*)dw, kh, kw, cin, f, Th, Tw,
                                                                          sh, sw, accumulate ? 1 : 0);
  DLWP_LAUNCH_CHECK("tconv_weights_bwd_kernel");
  return DLWP_OK;
}

int dlwp_depth_to_space2_crop(dlwp_handle_t h, const void* src, void* dst, int n, int f, int hp, int wp, int top, int left,
                              int out_h, int out_w, int c_off, int c_total, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_depth_to_space2_crop, h, src, dst, n, f, hp, wp, top, left, out_h, out_w, c_off, c_total, dtype);
  const int rc = check_interleave("dlwp_depth_to_space2_crop", h, src, dst, n, f, hp, wp, top, left, out_h, out_w, c_off, c_total,
                                  dtype);
  if (rc != DLWP_OK) return rc;
  if (n == 0) return DLWP_OK;
  const D2sGeom g{f, hp, wp, top, left, out_h, out_w, c_off, c_total};
  if (vec_ok(src, dst, g)) {
    const long long total = (long long)n * f * out_h * (wp / 4);
    d2s_crop_vec_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)src, (float*)dst, total, g);
  } else {
    const long long total = (long long)n * f * hp * wp;
    d2s_crop_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)src, (float*)dst, total, g);
  }
  DLWP_LAUNCH_CHECK("d2s_crop_kernel");
  return DLWP_OK;
}

int dlwp_space_to_depth2_fill(dlwp_handle_t h, const void* src, void* dst, int n, int f, int hp, int wp, int top, int left,
                              int in_h, int in_w, int c_off, int c_total, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_space_to_depth2_fill, h, src, dst, n, f, hp, wp, top, left, in_h, in_w, c_off, c_total, dtype);
  const int rc = check_interleave("dlwp_space_to_depth2_fill", h, src, dst, n, f, hp, wp, top, left, in_h, in_w, c_off, c_total,
                                  dtype);
  if (rc != DLWP_OK) return rc;
  if (n == 0) return DLWP_OK;
  const D2sGeom g{f, hp, wp, top, left, in_h, in_w, c_off, c_total};
  if (vec_ok(src, dst, g)) {
    const long long total = (long long)n * f * 2 * hp * (wp / 4);
    s2d_fill_vec_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)src, (float*)dst, total, g);
  } else {
    const long long total = (long long)n * f * hp * wp;
    s2d_fill_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)src, (float*)dst, total, g);
  }
  DLWP_LAUNCH_CHECK("s2d_fill_kernel");
  return DLWP_OK;
}

}  // extern "C"
