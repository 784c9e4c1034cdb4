// scale.hip -- the wrapper's scaler and imputer on the device (include/dlwp_hip.h: dlwp_scale_fwd / dlwp_scale_inv).
//
// Reference: DLWPNeuralNet.predict (DLWP/model/models.py:230-245) runs sklearn's SimpleImputer.transform and the scaler's
// transform on the host in front of every model.predict and the scaler's inverse_transform behind it; predict_timeseries does that
// once per forecast step (:277-293).  Per feature these are a NaN fill and an affine map, so one pure streaming launch per
// direction keeps a scaled model's rollout in HBM.
//
// The arithmetic is PINNED: it is numpy's when sklearn updates a float32 array in place with float64 parameters (X -= mean_;
// X /= scale_ | X *= scale_; X += min_) -- each stage in double, rounded to float32 before the next one.  Two primitive forms serve
// both scalers in both directions: "subtract, divide" and "multiply, add".  IEEE double division (the library is built without
// fast-math) and no contraction: the rounding between the stages leaves nothing to fuse, the pragma below keeps it so.
//
// Layout: a thread owns one feature (four adjacent ones on the float4 path), reads that feature's parameters once and walks down
// its share of the samples; blockIdx.y cuts the samples into shares so that small batches of wide samples and large batches of
// narrow ones both fill the chip.
#include "common.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int SCALE_THREADS = 256;
constexpr int SCALE_BLOCKS = 1024;   // workgroups a launch aims for (256 CUs x 4)

// one element through the stages.  MULADD false: t = x - p0, y = t / p1; true: t = x * p0, y = t + p1 (p0 / p1 absent: stage left out)
template <bool MULADD>
__device__ __forceinline__ float scale_one(float x, bool has_fill, float fill, bool has0, double p0, bool has1, double p1) {
  if (has_fill && x != x) x = fill;
  if (MULADD) {
    if (has0) x = (float)((double)x * p0);
    if (has1) x = (float)((double)x + p1);
  } else {
    if (has0) x = (float)((double)x - p0);
    if (has1) x = (float)((double)x / p1);
  }
  return x;
}

// V = 4: f % 4 == 0 and x, y 16-byte aligned; V = 1: any float alignment
template <int V, bool MULADD>
__global__ __launch_bounds__(SCALE_THREADS) void scale_kernel(const float* xin, float* yout, const double* __restrict__ fill,
                                                               const double* __restrict__ p0, const double* __restrict__ p1, int n, int f,
                                                               int rows) {
  // (x and y may be the same memory: every element is read before it is written by the one thread that owns it)
  const int col = (blockIdx.x * SCALE_THREADS + threadIdx.x) * V;
  if (col >= f) return;
  const int r0 = blockIdx.y * rows;
  const int r1 = r0 + rows < n ? r0 + rows : n;
  float fl[V];
  double a[V], b[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    fl[k] = fill ? (float)fill[col + k] : 0.f;
    a[k] = p0 ? p0[col + k] : 0.0;
    b[k] = p1 ? p1[col + k] : 0.0;
  }
  const bool hf = fill != nullptr, h0 = p0 != nullptr, h1 = p1 != nullptr;
  for (int r = r0; r < r1; ++r) {
    const size_t at = (size_t)r * f + col;
    if constexpr (V == 4) {
      const float4 v = *reinterpret_cast<const float4*>(xin + at);
      float4 o;
      o.x = scale_one<MULADD>(v.x, hf, fl[0], h0, a[0], h1, b[0]);
      o.y = scale_one<MULADD>(v.y, hf, fl[1], h0, a[1], h1, b[1]);
      o.z = scale_one<MULADD>(v.z, hf, fl[2], h0, a[2], h1, b[2]);
      o.w = scale_one<MULADD>(v.w, hf, fl[3], h0, a[3], h1, b[3]);
      *reinterpret_cast<float4*>(yout + at) = o;
    } else {
      yout[at] = scale_one<MULADD>(xin[at], hf, fl[0], h0, a[0], h1, b[0]);
    }
  }
}

int launch_scale(const char* who, dlwp_handle_t h, const void* x, void* y, const void* fill, const void* p0, const void* p1,
                 bool muladd, dlwp_scale d, void* stream) {
  DLWP_CHECK_ARG(h && x && y, "%s: null handle or pointer", who);
  DLWP_CHECK_ARG(d.n >= 0 && d.f > 0, "%s: %d samples of %d features", who, d.n, d.f);
  DLWP_CHECK_ARG(((uintptr_t)x | (uintptr_t)y) % 4 == 0, "%s: x and y must be float aligned", who);
  DLWP_CHECK_ARG(((uintptr_t)fill | (uintptr_t)p0 | (uintptr_t)p1) % 8 == 0, "%s: the parameter arrays are float64 (8-byte aligned)", who);
  if (d.n == 0) return DLWP_OK;
  const bool vec = d.f % 4 == 0 && ((uintptr_t)x | (uintptr_t)y) % 16 == 0;
  const int cols = vec ? d.f / 4 : d.f;
  const int gx = dlwp_ceil_div(cols, SCALE_THREADS);
  int gy = SCALE_BLOCKS / gx;
  gy = gy < 1 ? 1 : (gy > d.n ? d.n : gy);
  const int rows = dlwp_ceil_div(d.n, gy);
  gy = dlwp_ceil_div(d.n, rows);
  DLWP_CHECK_ARG(gy <= 65535, "%s: %d samples of %d features do not fit one launch", who, d.n, d.f);
  const dim3 grid((unsigned)gx, (unsigned)gy);
  hipStream_t s = (hipStream_t)stream;
  const float* xf = (const float*)x;
  float* yf = (float*)y;
  const double *fd = (const double*)fill, *a = (const double*)p0, *b = (const double*)p1;
  if (vec) {
    if (muladd) scale_kernel<4, true><<<grid, SCALE_THREADS, 0, s>>>(xf, yf, fd, a, b, d.n, d.f, rows);
    else scale_kernel<4, false><<<grid, SCALE_THREADS, 0, s>>>(xf, yf, fd, a, b, d.n, d.f, rows);
  } else {
    if (muladd) scale_kernel<1, true><<<grid, SCALE_THREADS, 0, s>>>(xf, yf, fd, a, b, d.n, d.f, rows);
    else scale_kernel<1, false><<<grid, SCALE_THREADS, 0, s>>>(xf, yf, fd, a, b, d.n, d.f, rows);
  }
  DLWP_LAUNCH_CHECK("scale kernel");
  return DLWP_OK;
}

}  // namespace

extern "C" {

int dlwp_scale_fwd(dlwp_handle_t h, const void* x, void* y, const void* fill, const void* shift, const void* scale, dlwp_scale d,
                   void* stream) {
  DLWP_UNTAPED(dlwp_scale_fwd);
  DLWP_CHECK_ARG(d.kind == DLWP_SCALE_STANDARD || d.kind == DLWP_SCALE_MINMAX, "dlwp_scale_fwd: kind %d", d.kind);
  // StandardScaler: (x - mean) / scale;  MinMaxScaler: x * scale + min
  if (d.kind == DLWP_SCALE_STANDARD) return launch_scale("dlwp_scale_fwd", h, x, y, fill, shift, scale, false, d, stream);
  return launch_scale("dlwp_scale_fwd", h, x, y, fill, scale, shift, true, d, stream);
}

int dlwp_scale_inv(dlwp_handle_t h, const void* x, void* y, const void* shift, const void* scale, dlwp_scale d, void* stream) {
  DLWP_UNTAPED(dlwp_scale_inv);
  DLWP_CHECK_ARG(d.kind == DLWP_SCALE_STANDARD || d.kind == DLWP_SCALE_MINMAX, "dlwp_scale_inv: kind %d", d.kind);
  // StandardScaler: x * scale + mean;  MinMaxScaler: (x - min) / scale
  if (d.kind == DLWP_SCALE_STANDARD) return launch_scale("dlwp_scale_inv", h, x, y, nullptr, scale, shift, true, d, stream);
  return launch_scale("dlwp_scale_inv", h, x, y, nullptr, shift, scale, false, d, stream);
}

}  // extern "C"
