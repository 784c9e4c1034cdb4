// losses.hip -- the Keras 2.2 regression losses beyond 'mse' (gfx950): mean_absolute_error, mean_absolute_percentage_error,
// mean_squared_logarithmic_error, logcosh -- value, gradient, the fused form on a restated output layer's phase channels, and
// one pass that fills every requested metric column of an output.
//
// Reference: keras/losses.py (Keras 2.2) as called by DLWPNeuralNet.compile / fit (DLWP/model/models.py:188-228) and wrapped by
// DLWP.custom.latitude_weighted_loss / LatitudeWeightedLoss (DLWP/custom.py:899-991).  The 'mse' / custom-loss kernels of
// train_ops.hip are untouched.
// Every sum is two-stage with a fixed tree (per-block partials, one final block or the handle's deferred flush), no atomics:
// repeated launches give identical bits.  Loads are 16 bytes wide where the layout allows it.
#include "common.h"
#include "tape.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr float KERAS_EPS = 1e-7f;        // K.epsilon()
constexpr int LOSS_SPLIT = 128;           // slices per phase channel pair of dlwp_loss_elementwise_phase
constexpr int METRIC_SLOTS = 8;           // mse, mae, mape, msle, logcosh, S_pt, S_pp, S_tt

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// block-wide sum of (a, b); result valid in thread 0.  256 threads.
__device__ __forceinline__ void block_sum2(float& a, float& b) {
  __shared__ float sa[4], sb[4];
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sa[wave] = a; sb[wave] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sa[0] + sa[1] + sa[2] + sa[3];
    b = sb[0] + sb[1] + sb[2] + sb[3];
  }
  __syncthreads();
}

// w * y rounded on its own, as the reference's y_true * w, y_pred * w: never contracted into the subtraction behind it (equal
// operands stay equal -- the mae gradient at x = 0 is 0 -- and every path rounds the same).  (__fmul_rn is a plain product
// here, which the default -ffp-contract=fast-honor-pragmas may fuse: the pragma keeps this one apart.)
__device__ __forceinline__ float wmul(float w, float y) {
#pragma clang fp contract(off)
  return w * y;
}

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// value of one element and d value / d yp (before the 1/N of the mean), x = p - t
template <int KIND>
__device__ __forceinline__ float loss_term(float p, float t, float& g) {
  const float x = p - t;
  if (KIND == DLWP_LOSS_MSE) {
    g = 2.f * x;
    return x * x;
  } else if (KIND == DLWP_LOSS_MAE) {
    g = sgn(x);
    return fabsf(x);
  } else if (KIND == DLWP_LOSS_MAPE) {
    const float den = fmaxf(fabsf(t), KERAS_EPS);
    g = 100.f * sgn(x) / den;
    return 100.f * fabsf(x) / den;
  } else if (KIND == DLWP_LOSS_MSLE) {
    const float pc = fmaxf(p, KERAS_EPS);
    const float d = log1pf(pc) - log1pf(fmaxf(t, KERAS_EPS));
    g = p < KERAS_EPS ? 0.f : 2.f * d / (pc + 1.f);      // clip_by_value passes no gradient below the bound
    return d * d;
  } else {   // DLWP_LOSS_LOGCOSH: x + softplus(-2x) - log 2 in the form that cannot overflow
    const float ax = fabsf(x);
    g = tanhf(x);
    return ax + log1pf(expf(-2.f * ax)) - 0.69314718055994531f;
  }
}

// ------------------------------------------------------------------------------------------------------------------ //
// dlwp_loss_elementwise: grid-stride over float4 units (VEC) or single elements, row weight w[(i / W) % H] on both operands
// ------------------------------------------------------------------------------------------------------------------ //
template <int KIND, bool VEC, bool ROWW>
__global__ __launch_bounds__(256) void loss_ew_partial_kernel(const float* __restrict__ yp, const float* __restrict__ yt,
                                                              const float* __restrict__ roww, float* __restrict__ dy,
                                                              float* __restrict__ partial, unsigned n, int H, int W,
                                                              float grad_scale) {
  float s = 0.f, dummy = 0.f;
  const unsigned stride = gridDim.x * 256u;
  const unsigned n4 = VEC ? n / 4u : 0u;
  for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < n4; q += stride) {
    const f32x4 p = reinterpret_cast<const f32x4*>(yp)[q];
    const f32x4 t = reinterpret_cast<const f32x4*>(yt)[q];
    f32x4 w = {1.f, 1.f, 1.f, 1.f};
    if (ROWW) {
      const unsigned i0 = 4u * q, r0 = i0 / (unsigned)W;
      int col = (int)(i0 - r0 * (unsigned)W), row = (int)(r0 % (unsigned)H);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = roww[row];
        if (++col == W) {
          col = 0;
          row = row + 1 == H ? 0 : row + 1;
        }
      }
    }
    f32x4 g;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk;
      s += loss_term<KIND>(wmul(w[k], p[k]), wmul(w[k], t[k]), gk);
      g[k] = grad_scale * w[k] * gk;
    }
    if (dy) reinterpret_cast<f32x4*>(dy)[q] = g;
  }
  for (unsigned i = 4u * n4 + blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const float w = ROWW ? roww[(i / (unsigned)W) % (unsigned)H] : 1.f;
    float g;
    s += loss_term<KIND>(wmul(w, yp[i]), wmul(w, yt[i]), g);
    if (dy) dy[i] = grad_scale * w * g;
  }
  block_sum2(s, dummy);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// stage 2: out[0] = scale * (sum of the partials), in a fixed order
__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ partial, int nblocks, float scale,
                                                         float* __restrict__ out) {
  float s = 0.f, dummy = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
  block_sum2(s, dummy);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// per-channel sums of the slice partials: db[c] = sum_s partial[c * S + s], one wave per channel
__global__ __launch_bounds__(64) void split_final_kernel(const float* __restrict__ partial, int S, float* __restrict__ db) {
  float v = 0.f;
  for (int s = threadIdx.x; s < S; s += 64) v += partial[blockIdx.x * S + s];
  v = wave_sum(v);
  if (threadIdx.x == 0) db[blockIdx.x] = v;
}

// ------------------------------------------------------------------------------------------------------------------ //
// dlwp_loss_elementwise_phase.  yp (N, 4F, h, w): output pixel (2i + a, 2j + b) of field co sits in channel (2a + b) F + co;
// yt (N, F, 2h, 2w).  Block (a F + co, s) owns slice s of the N h (w / 2) units of BOTH channels (2a) F + co and (2a + 1) F + co:
// a unit is target pixels (2i + a, 4m .. 4m + 3) -- one 16-byte target load -- and the two 8-byte phase loads j = 2m, 2m + 1.
// w even (checked by the host).  Loss partials [blk], bias partials [c4 * LOSS_SPLIT + s] for c4 = (2a + b) F + co.
// ------------------------------------------------------------------------------------------------------------------ //
template <int KIND, bool ROWW>
__global__ __launch_bounds__(256) void loss_phase_partial_kernel(const float* __restrict__ yp, const float* __restrict__ yt,
                                                                 const float* __restrict__ roww, float* __restrict__ dz,
                                                                 float* __restrict__ partial, float* __restrict__ bias_partial,
                                                                 int N, int F, int h, int w, float grad_scale) {
  const int pc = blockIdx.x, sidx = blockIdx.y;
  const int pa = pc / F, co = pc - pa * F;
  const unsigned hw = (unsigned)h * (unsigned)w, w2 = (unsigned)w / 2u;
  const unsigned per = (unsigned)N * (unsigned)h * w2;   // (< 2^31: checked by the host)
  const unsigned chunk = (per + LOSS_SPLIT - 1) / LOSS_SPLIT;
  const unsigned lo = sidx * chunk, hi = lo + chunk < per ? lo + chunk : per;
  const int c0 = (2 * pa) * F + co, c1 = c0 + F;
  float s = 0.f, sb0 = 0.f, sb1 = 0.f, dummy = 0.f;
  for (unsigned e = lo + threadIdx.x; e < hi; e += 256) {
    const unsigned q = e / w2;
    const unsigned m = e - q * w2;
    const unsigned n = q / (unsigned)h;
    const unsigned i = q - n * (unsigned)h;
    const size_t p0 = ((size_t)n * 4 * F + c0) * hw + (size_t)i * w + 2 * m;
    const size_t p1 = p0 + (size_t)F * hw;
    const size_t ti = (((size_t)n * F + co) * 2 * h + 2 * i + pa) * (2 * (size_t)w) + 4 * m;
    const f32x2 a0 = *reinterpret_cast<const f32x2*>(yp + p0);
    const f32x2 a1 = *reinterpret_cast<const f32x2*>(yp + p1);
    const f32x4 t = *reinterpret_cast<const f32x4*>(yt + ti);
    const float wr = ROWW ? roww[2 * i + pa] : 1.f;
    float g00, g10, g01, g11;    // g<b><j - 2m>
    s += loss_term<KIND>(wmul(wr, a0.x), wmul(wr, t.x), g00);
    s += loss_term<KIND>(wmul(wr, a1.x), wmul(wr, t.y), g10);
    s += loss_term<KIND>(wmul(wr, a0.y), wmul(wr, t.z), g01);
    s += loss_term<KIND>(wmul(wr, a1.y), wmul(wr, t.w), g11);
    const float k = grad_scale * wr;
    const f32x2 d0 = {k * g00, k * g01}, d1 = {k * g10, k * g11};
    if (dz) {
      *reinterpret_cast<f32x2*>(dz + p0) = d0;
      *reinterpret_cast<f32x2*>(dz + p1) = d1;
    }
    sb0 += d0.x + d0.y;
    sb1 += d1.x + d1.y;
  }
  block_sum2(s, dummy);
  block_sum2(sb0, sb1);
  if (threadIdx.x == 0) {
    partial[pc * LOSS_SPLIT + sidx] = s;
    if (bias_partial) {
      bias_partial[c0 * LOSS_SPLIT + sidx] = sb0;
      bias_partial[c1 * LOSS_SPLIT + sidx] = sb1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ //
// dlwp_loss_metrics: one pass, the requested slots of {mse, mae, mape, msle, logcosh, S_pt, S_pp, S_tt} per block.
// PHASE: yp in phase layout (as above) and the unit is the u-th float4 of the target (2w % 4 == 0 checked by the host).
// ------------------------------------------------------------------------------------------------------------------ //
struct MetricAcc {
  float s[METRIC_SLOTS];
};

__device__ __forceinline__ void metric_add(MetricAcc& a, unsigned mask, float p, float t) {
  float g;
  if (mask & (1u << DLWP_LOSS_MSE)) a.s[0] += loss_term<DLWP_LOSS_MSE>(p, t, g);
  if (mask & (1u << DLWP_LOSS_MAE)) a.s[1] += loss_term<DLWP_LOSS_MAE>(p, t, g);
  if (mask & (1u << DLWP_LOSS_MAPE)) a.s[2] += loss_term<DLWP_LOSS_MAPE>(p, t, g);
  if (mask & (1u << DLWP_LOSS_MSLE)) a.s[3] += loss_term<DLWP_LOSS_MSLE>(p, t, g);
  if (mask & (1u << DLWP_LOSS_LOGCOSH)) a.s[4] += loss_term<DLWP_LOSS_LOGCOSH>(p, t, g);
  if (mask & DLWP_METRIC_ACC_SUMS) {
    a.s[5] += p * t;
    a.s[6] += p * p;
    a.s[7] += t * t;
  }
}

template <bool VEC, bool PHASE>
__global__ __launch_bounds__(256) void loss_metrics_partial_kernel(const float* __restrict__ yp, const float* __restrict__ yt,
                                                                   float* __restrict__ partial, unsigned n, unsigned mask,
                                                                   int F, int h, int w) {
  MetricAcc a;
#pragma unroll
  for (int k = 0; k < METRIC_SLOTS; ++k) a.s[k] = 0.f;
  const unsigned stride = gridDim.x * 256u;
  const unsigned n4 = VEC ? n / 4u : 0u;
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < n4; u += stride) {
    const f32x4 t = reinterpret_cast<const f32x4*>(yt)[u];
    f32x4 p;
    if (PHASE) {
      const unsigned w2 = (unsigned)w / 2u;
      const unsigned q = u / w2, m = u - q * w2;          // q: target row over all (sample, field) planes
      const unsigned plane = q / (2u * (unsigned)h), r = q - plane * 2u * (unsigned)h;
      const unsigned nn = plane / (unsigned)F, co = plane - nn * (unsigned)F;
      const unsigned pa = r & 1u, i = r >> 1;
      const size_t hw = (size_t)h * w;
      const size_t p0 = ((size_t)nn * 4 * F + 2 * pa * F + co) * hw + (size_t)i * w + 2 * m;
      const f32x2 a0 = *reinterpret_cast<const f32x2*>(yp + p0);
      const f32x2 a1 = *reinterpret_cast<const f32x2*>(yp + p0 + (size_t)F * hw);
      p = f32x4{a0.x, a1.x, a0.y, a1.y};
    } else {
      p = reinterpret_cast<const f32x4*>(yp)[u];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) metric_add(a, mask, p[k], t[k]);
  }
  if (!PHASE)
    for (unsigned i = 4u * n4 + blockIdx.x * 256u + threadIdx.x; i < n; i += stride) metric_add(a, mask, yp[i], yt[i]);
  block_sum2(a.s[0], a.s[1]);
  block_sum2(a.s[2], a.s[3]);
  block_sum2(a.s[4], a.s[5]);
  block_sum2(a.s[6], a.s[7]);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < METRIC_SLOTS; ++k) partial[METRIC_SLOTS * blockIdx.x + k] = a.s[k];
}

// stage 2: the requested slots, in slot order, as means
__global__ __launch_bounds__(256) void loss_metrics_final_kernel(const float* __restrict__ partial, int nblocks, unsigned mask,
                                                                 float inv_n, float* __restrict__ out) {
  MetricAcc a;
#pragma unroll
  for (int k = 0; k < METRIC_SLOTS; ++k) a.s[k] = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256)
#pragma unroll
    for (int k = 0; k < METRIC_SLOTS; ++k) a.s[k] += partial[METRIC_SLOTS * i + k];
  block_sum2(a.s[0], a.s[1]);
  block_sum2(a.s[2], a.s[3]);
  block_sum2(a.s[4], a.s[5]);
  block_sum2(a.s[6], a.s[7]);
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (mask & (1u << k)) out[c++] = a.s[k] * inv_n;
    if (mask & DLWP_METRIC_ACC_SUMS) {
      out[c++] = a.s[5] * inv_n;
      out[c++] = a.s[6] * inv_n;
      out[c++] = a.s[7] * inv_n;
    }
  }
}

inline int grid_for(long long items, int cu) {
  long long want = (items + 255) / 256;
  const long long cap = (long long)cu * 8;
  if (want < 1) want = 1;
  return (int)(want < cap ? want : cap);
}

inline bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }
inline bool aligned8(const void* p) { return p == nullptr || ((uintptr_t)p & 7) == 0; }

template <int KIND>
void launch_ew(const float* yp, const float* yt, const float* roww, float* dy, float* partial, unsigned n, int H, int W,
               float grad_scale, bool vec, int grid, hipStream_t s) {
  if (vec && roww)
    loss_ew_partial_kernel<KIND, true, true><<<grid, 256, 0, s>>>(yp, yt, roww, dy, partial, n, H, W, grad_scale);
  else if (vec)
    loss_ew_partial_kernel<KIND, true, false><<<grid, 256, 0, s>>>(yp, yt, roww, dy, partial, n, H, W, grad_scale);
  else if (roww)
    loss_ew_partial_kernel<KIND, false, true><<<grid, 256, 0, s>>>(yp, yt, roww, dy, partial, n, H, W, grad_scale);
  else
    loss_ew_partial_kernel<KIND, false, false><<<grid, 256, 0, s>>>(yp, yt, roww, dy, partial, n, H, W, grad_scale);
}

template <int KIND>
void launch_phase(const float* yp, const float* yt, const float* roww, float* dz, float* lp, float* bp, int n, int f, int hh,
                  int ww, float grad_scale, hipStream_t s) {
  const dim3 grid(2 * f, LOSS_SPLIT);
  if (roww)
    loss_phase_partial_kernel<KIND, true><<<grid, 256, 0, s>>>(yp, yt, roww, dz, lp, bp, n, f, hh, ww, grad_scale);
  else
    loss_phase_partial_kernel<KIND, false><<<grid, 256, 0, s>>>(yp, yt, roww, dz, lp, bp, n, f, hh, ww, grad_scale);
}

}  // namespace

extern "C" {

size_t dlwp_loss_elementwise_workspace(dlwp_handle_t h) { return h ? (size_t)h->cu_count * 8 * sizeof(float) : 0; }

int dlwp_loss_elementwise(dlwp_handle_t h, const void* y_pred, const void* y_true, int n, int c, int hh, int ww,
                          const void* row_weights, int kind, void* out1, void* dy, float loss_weight, void* ws,
                          size_t ws_bytes, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_loss_elementwise, h, y_pred, y_true, n, c, hh, ww, row_weights, kind, out1, dy, loss_weight, ws,
            ws_bytes, dtype);
  DLWP_CHECK_ARG(h && y_pred && y_true && out1 && ws, "dlwp_loss_elementwise: null handle or pointer");
  DLWP_CHECK_ARG(dtype == DLWP_F32 && n > 0 && c > 0 && hh > 0 && ww > 0, "dlwp_loss_elementwise: bad dtype / shape");
  DLWP_CHECK_ARG(kind >= DLWP_LOSS_MSE && kind <= DLWP_LOSS_LOGCOSH, "dlwp_loss_elementwise: bad kind %d", kind);
  const long long total = (long long)n * c * hh * ww;
  DLWP_CHECK_ARG(total < (1ll << 31), "dlwp_loss_elementwise: more than 2^31 elements");
  const int grid = grid_for((total + 3) / 4, h->cu_count);
  DLWP_CHECK_ARG(ws_bytes >= (size_t)grid * sizeof(float), "dlwp_loss_elementwise: workspace too small (%zu < %zu)", ws_bytes,
                 (size_t)grid * sizeof(float));
  const bool vec = aligned16(y_pred) && aligned16(y_true) && aligned16(dy);
  const float inv_n = (float)(1.0 / (double)total);
  const float* yp = (const float*)y_pred;
  const float* yt = (const float*)y_true;
  const float* rw = (const float*)row_weights;
  float* partial = (float*)ws;
  const float gs = loss_weight * inv_n;
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case DLWP_LOSS_MSE: launch_ew<DLWP_LOSS_MSE>(yp, yt, rw, (float*)dy, partial, (unsigned)total, hh, ww, gs, vec, grid, s); break;
    case DLWP_LOSS_MAE: launch_ew<DLWP_LOSS_MAE>(yp, yt, rw, (float*)dy, partial, (unsigned)total, hh, ww, gs, vec, grid, s); break;
    case DLWP_LOSS_MAPE: launch_ew<DLWP_LOSS_MAPE>(yp, yt, rw, (float*)dy, partial, (unsigned)total, hh, ww, gs, vec, grid, s); break;
    case DLWP_LOSS_MSLE: launch_ew<DLWP_LOSS_MSLE>(yp, yt, rw, (float*)dy, partial, (unsigned)total, hh, ww, gs, vec, grid, s); break;
    default: launch_ew<DLWP_LOSS_LOGCOSH>(yp, yt, rw, (float*)dy, partial, (unsigned)total, hh, ww, gs, vec, grid, s); break;
  }
  loss_final_kernel<<<1, 256, 0, s>>>(partial, grid, inv_n, (float*)out1);
  DLWP_LAUNCH_CHECK("loss_elementwise kernels");
  return DLWP_OK;
}

size_t dlwp_loss_elementwise_phase_workspace(int f) {
  return (size_t)(f > 0 ? f : 0) * LOSS_SPLIT * (2 + 4) * sizeof(float);
}

int dlwp_loss_elementwise_phase(dlwp_handle_t h, const void* y_phase, const void* y_true, int n, int f, int hh, int ww,
                                const void* row_weights, int kind, void* out1, void* dz_phase, void* db4f, float loss_weight,
                                void* ws, size_t ws_bytes, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_loss_elementwise_phase, h, y_phase, y_true, n, f, hh, ww, row_weights, kind, out1, dz_phase, db4f,
            loss_weight, ws, ws_bytes, dtype);
  DLWP_CHECK_ARG(h && y_phase && y_true && out1 && ws, "dlwp_loss_elementwise_phase: null handle or pointer");
  DLWP_CHECK_ARG(dtype == DLWP_F32 && n > 0 && f > 0 && hh > 0 && ww > 0 && ww % 2 == 0,
                 "dlwp_loss_elementwise_phase: bad dtype / shape (the phase width must be even)");
  DLWP_CHECK_ARG(kind >= DLWP_LOSS_MSE && kind <= DLWP_LOSS_LOGCOSH, "dlwp_loss_elementwise_phase: bad kind %d", kind);
  DLWP_CHECK_ARG(4ll * n * f * hh * ww < (1ll << 31), "dlwp_loss_elementwise_phase: more than 2^31 elements");
  DLWP_CHECK_ARG(aligned16(y_true) && aligned8(y_phase) && aligned8(dz_phase),
                 "dlwp_loss_elementwise_phase: y_true must be 16-byte aligned, the phase tensors 8-byte aligned");
  DLWP_CHECK_ARG(ws_bytes >= dlwp_loss_elementwise_phase_workspace(f), "dlwp_loss_elementwise_phase: workspace too small (%zu < %zu)",
                 ws_bytes, dlwp_loss_elementwise_phase_workspace(f));
  const float inv_n = (float)(1.0 / (4.0 * n * f * hh * ww));
  float* lp = (float*)ws;
  float* bp = lp + (size_t)2 * f * LOSS_SPLIT;
  const float* yp = (const float*)y_phase;
  const float* yt = (const float*)y_true;
  const float* rw = (const float*)row_weights;
  float* dz = (float*)dz_phase;
  float* bpp = db4f ? bp : nullptr;
  const float gs = loss_weight * inv_n;
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case DLWP_LOSS_MSE: launch_phase<DLWP_LOSS_MSE>(yp, yt, rw, dz, lp, bpp, n, f, hh, ww, gs, s); break;
    case DLWP_LOSS_MAE: launch_phase<DLWP_LOSS_MAE>(yp, yt, rw, dz, lp, bpp, n, f, hh, ww, gs, s); break;
    case DLWP_LOSS_MAPE: launch_phase<DLWP_LOSS_MAPE>(yp, yt, rw, dz, lp, bpp, n, f, hh, ww, gs, s); break;
    case DLWP_LOSS_MSLE: launch_phase<DLWP_LOSS_MSLE>(yp, yt, rw, dz, lp, bpp, n, f, hh, ww, gs, s); break;
    default: launch_phase<DLWP_LOSS_LOGCOSH>(yp, yt, rw, dz, lp, bpp, n, f, hh, ww, gs, s); break;
  }
  loss_final_kernel<<<1, 256, 0, s>>>(lp, 2 * f * LOSS_SPLIT, inv_n, (float*)out1);
  if (db4f) {
    const int rd = dlwp_reduce_defer(h, bp, (float*)db4f, 4 * f, LOSS_SPLIT, LOSS_SPLIT, 1, 1.0f, 0, s);
    if (rd < 0) return rd;
    if (rd == 0) split_final_kernel<<<4 * f, 64, 0, s>>>(bp, LOSS_SPLIT, (float*)db4f);
  }
  DLWP_LAUNCH_CHECK("loss_elementwise_phase kernels");
  return DLWP_OK;
}

size_t dlwp_loss_metrics_workspace(dlwp_handle_t h) { return h ? (size_t)h->cu_count * 8 * METRIC_SLOTS * sizeof(float) : 0; }

int dlwp_loss_metrics(dlwp_handle_t h, const void* y_pred, const void* y_true, int n, int c, int hh, int ww, int phase,
                      unsigned mask, void* out, void* ws, size_t ws_bytes, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_loss_metrics, h, y_pred, y_true, n, c, hh, ww, phase, mask, out, ws, ws_bytes, dtype);
  DLWP_CHECK_ARG(h && y_pred && y_true && out && ws, "dlwp_loss_metrics: null handle or pointer");
  DLWP_CHECK_ARG(dtype == DLWP_F32 && n > 0 && c > 0 && hh > 0 && ww > 0, "dlwp_loss_metrics: bad dtype / shape");
  DLWP_CHECK_ARG(mask != 0 && (mask & ~(0x1fu | DLWP_METRIC_ACC_SUMS)) == 0, "dlwp_loss_metrics: bad metric mask 0x%x", mask);
  const long long total = (long long)n * c * hh * ww;
  DLWP_CHECK_ARG(total < (1ll << 31), "dlwp_loss_metrics: more than 2^31 elements");
  const int grid = grid_for((total + 3) / 4, h->cu_count);
  DLWP_CHECK_ARG(ws_bytes >= (size_t)grid * METRIC_SLOTS * sizeof(float), "dlwp_loss_metrics: workspace too small (%zu < %zu)",
                 ws_bytes, (size_t)grid * METRIC_SLOTS * sizeof(float));
  const float* yp = (const float*)y_pred;
  const float* yt = (const float*)y_true;
  float* partial = (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  if (phase) {   // (n, c, hh, ww) is the TARGET's shape; y_pred is (n, 4c, hh / 2, ww / 2)
    DLWP_CHECK_ARG(hh % 2 == 0 && ww % 4 == 0 && aligned16(y_true) && aligned8(y_pred),
                   "dlwp_loss_metrics: the phase form needs a target width divisible by 4, a 16-byte aligned target and an "
                   "8-byte aligned phase tensor");
    loss_metrics_partial_kernel<true, true><<<grid, 256, 0, s>>>(yp, yt, partial, (unsigned)total, mask, c, hh / 2, ww / 2);
  } else if (aligned16(y_pred) && aligned16(y_true)) {
    loss_metrics_partial_kernel<true, false><<<grid, 256, 0, s>>>(yp, yt, partial, (unsigned)total, mask, c, hh, ww);
  } else {
    loss_metrics_partial_kernel<false, false><<<grid, 256, 0, s>>>(yp, yt, partial, (unsigned)total, mask, c, hh, ww);
  }
  loss_metrics_final_kernel<<<1, 256, 0, s>>>(partial, grid, mask, (float)(1.0 / (double)total), (float*)out);
  DLWP_LAUNCH_CHECK("loss_metrics kernels");
  return DLWP_OK;
}

}  // extern "C"
