// batchnorm.hip -- keras BatchNormalization(axis=1) on NCHW float32 tensors (gfx950).
//
// Reference: the `('BatchNormalization', None, {'axis': 1})` entry after every Conv2D of the reference's training scripts
// (examples/train.py:170-210, train_generator.py:172-212, Azure/train_tf.py:219-259; commented out there, one keystroke away).
// A channel c of an (N, C, H, W) tensor is N contiguous runs of H*W floats; its M = N*H*W values are cut into S contiguous
// SLABS (the same cut in the forward statistics and the backward sums, a function of the shape alone), one workgroup per
// (channel, slab).  All merges run in a fixed order -- lanes by a fixed shuffle tree, waves in index order, slabs in index
// order -- and no floating-point atomics are used: the same inputs give the same bits, launch after launch.
//
//   training forward : stats_partial (count, mean, M2 per slab; 16-byte loads from the first 16-byte boundary on, a scalar
//                      head / tail) -> stats_final (Chan's parallel merge in double: mean, invstd, scale = gamma invstd,
//                      shift = beta - mean scale, the moving statistics updated in place) -> apply (y = x scale[c] + shift[c])
//   inference        : apply, the per-channel scale / shift formed by each workgroup from the moving statistics
//   backward         : bwd_partial (sum dy, sum dy xhat per slab) -> bwd_final (dgamma, dbeta, the element pass's coefficients)
//                      -> bwd_apply (dx = scale (dy - (sum_dy + xhat sum_dy_xhat) / M))
// Every kernel is bound by HBM: the element passes move 8 (forward) / 12 (backward) bytes per element.
#include "common.h"
#include "tape.h"

#include <initializer_list>

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_SPLIT = 64;         // slabs per channel
constexpr int BN_TARGET_BLOCKS = 2048;   // workgroups the reduction passes aim at (8 per CU)
constexpr int BN_MIN_SLAB = 2048;        // elements a slab holds at least
constexpr int BN_APPLY_VEC = 4;          // float4 per thread per step of the element passes ...
constexpr int BN_APPLY_ELEMS = BN_THREADS * 4 * BN_APPLY_VEC;   // ... so a workgroup covers 4096 elements of one plane

typedef float f32x4 __attribute__((ext_vector_type(4)));

// slabs per channel: a function of the shape only (the workspace size and every pass agree on it)
inline int bn_split(const dlwp_batchnorm& d) {
  const long long m = (long long)d.n * d.hw;
  int s = (BN_TARGET_BLOCKS + d.c - 1) / d.c;
  if (s > BN_MAX_SPLIT) s = BN_MAX_SPLIT;
  const long long by_size = m / BN_MIN_SLAB;
  if (s > by_size) s = (int)(by_size > 0 ? by_size : 1);
  return s < 1 ? 1 : s;
}

inline long long bn_chunk(long long m, int s) { return (m + s - 1) / s; }

// floats of the workspace: two partial sums per (channel, slab), then four coefficients per channel
inline size_t bn_ws_floats(const dlwp_batchnorm& d) {
  return (size_t)2 * d.c * bn_split(d) + (size_t)4 * d.c;
}

struct Stat {
  float n, mean, m2;
};

// Chan et al.: the statistics of the union of two disjoint sets
__device__ __forceinline__ Stat merge(Stat a, Stat b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float delta = b.mean - a.mean;
  const float wb = b.n / n;
  Stat r;
  r.n = n;
  r.mean = a.mean + delta * wb;
  r.m2 = a.m2 + b.m2 + delta * delta * a.n * wb;
  return r;
}

__device__ __forceinline__ Stat stat_of4(f32x4 v) {
  const float m = ((v[0] + v[1]) + (v[2] + v[3])) * 0.25f;
  const float d0 = v[0] - m, d1 = v[1] - m, d2 = v[2] - m, d3 = v[3] - m;
  return Stat{4.f, m, (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)};
}

__device__ __forceinline__ Stat shfl_down(Stat s, int off) {
  return Stat{__shfl_down(s.n, off, 64), __shfl_down(s.mean, off, 64), __shfl_down(s.m2, off, 64)};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One segment of a channel: elements [g0, g0 + len) of the flat tensor, all in one plane.  The 16-byte body starts at the first
// element whose ADDRESS is a multiple of 16: `align` = the base addresses' offset in floats from a 16-byte boundary (the same for
// every tensor of the launch), or -1 when they differ (then everything is the scalar head).  Threads take head elements t,
// t + 256, ..., body vectors t, t + 256, ... and tail element t.
struct Segment {
  long long g0;
  int head, nvec, tail;
};
__device__ __forceinline__ Segment segment(long long g0, int len, int align) {
  Segment s;
  s.g0 = g0;
  const int h = align < 0 ? len : (int)((4 - ((g0 + align) & 3)) & 3);
  s.head = h < len ? h : len;
  s.nvec = (len - s.head) >> 2;
  s.tail = len - s.head - 4 * s.nvec;
  return s;
}

// (channel c, slab s) -> partial (mean, M2) of x over the slab's elements
__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ pmean,
                                                                      float* __restrict__ pm2, int C, int hw, long long m,
                                                                      long long chunk, int S, int align) {
  const int c = blockIdx.x, sidx = blockIdx.y, t = threadIdx.x;
  const long long lo = (long long)sidx * chunk, hi = lo + chunk < m ? lo + chunk : m;
  Stat acc{0.f, 0.f, 0.f};
  for (long long base = lo; base < hi;) {
    const long long n = base / hw;
    const int p0 = (int)(base - n * hw);
    const int len = (int)((hi - base) < (long long)(hw - p0) ? (hi - base) : (hw - p0));
    const Segment sg = segment((n * C + c) * hw + p0, len, align);
    for (int i = t; i < sg.head; i += BN_THREADS) acc = merge(acc, Stat{1.f, x[sg.g0 + i], 0.f});
    const f32x4* xv = (const f32x4*)(x + sg.g0 + sg.head);
    int v = t;
    for (; v + 3 * BN_THREADS < sg.nvec; v += 4 * BN_THREADS) {   // four 16-byte loads in flight per lane
      const f32x4 a = xv[v], b = xv[v + BN_THREADS], cc = xv[v + 2 * BN_THREADS], d = xv[v + 3 * BN_THREADS];
      acc = merge(acc, merge(merge(stat_of4(a), stat_of4(b)), merge(stat_of4(cc), stat_of4(d))));
    }
    for (; v < sg.nvec; v += BN_THREADS) acc = merge(acc, stat_of4(xv[v]));
    if (t < sg.tail) acc = merge(acc, Stat{1.f, x[sg.g0 + sg.head + 4 * (long long)sg.nvec + t], 0.f});
    base += len;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = merge(acc, shfl_down(acc, off));
  __shared__ Stat waves[BN_THREADS / 64];
  if ((t & 63) == 0) waves[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    Stat r = waves[0];
#pragma unroll
    for (int w = 1; w < BN_THREADS / 64; ++w) r = merge(r, waves[w]);
    pmean[c * S + sidx] = r.mean;
    pm2[c * S + sidx] = r.m2;
  }
}

// one thread per channel: the slabs merged in index order (double), then everything per channel the other passes need
__global__ void bn_stats_final_kernel(const float* __restrict__ pmean, const float* __restrict__ pm2, const float* gamma,
                                      const float* beta, float* moving_mean, float* moving_var, float* save_mean,
                                      float* save_invstd, float* __restrict__ coef, int C, long long m, long long chunk, int S,
                                      float momentum, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int s = 0; s < S; ++s) {
    const long long lo = (long long)s * chunk;
    const long long hi = lo + chunk < m ? lo + chunk : m;
    const double nb = hi > lo ? (double)(hi - lo) : 0.0;
    if (nb == 0.0) continue;
    const double tot = n + nb, delta = (double)pmean[c * S + s] - mean;
    mean += delta * (nb / tot);
    m2 += (double)pm2[c * S + s] + delta * delta * n * (nb / tot);
    n = tot;
  }
  const double var = m2 / (double)m;                          // biased: what the batch is normalised with
  const double invstd = 1.0 / sqrt(var + (double)eps);
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float scale = (float)((double)g * invstd);
  save_mean[c] = (float)mean;
  save_invstd[c] = (float)invstd;
  coef[c] = scale;
  coef[C + c] = (float)((double)b - mean * (double)scale);
  // moving statistics: m * moving + (1 - m) * batch, the variance unbiased by M / (M - 1) (torch's F.batch_norm with
  // momentum 1 - m; the M > 1 check is the entry point's)
  const double mo = (double)momentum;
  moving_mean[c] = (float)(mo * (double)moving_mean[c] + (1.0 - mo) * mean);
  moving_var[c] = (float)(mo * (double)moving_var[c] + (1.0 - mo) * var * ((double)m / (double)(m - 1)));
}

// y = x * scale[c] + shift[c] over one 4096-element piece of one (sample, channel) plane.  INFER: scale / shift formed here
// from gamma, beta and the moving statistics (one reciprocal square root per workgroup); else read from coef[c], coef[C + c].
template <bool INFER>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              const float* __restrict__ coef, const float* gamma,
                                                              const float* beta, const float* mmean, const float* mvar,
                                                              float eps, int C, int hw, int pieces, int align) {
  const long long plane = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - plane * pieces);
  const int c = (int)(plane % C);
  float scale, shift;
  if (INFER) {
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    scale = g / sqrtf(mvar[c] + eps);
    shift = b - mmean[c] * scale;
  } else {
    scale = coef[c];
    shift = coef[C + c];
  }
  const int p0 = piece * BN_APPLY_ELEMS;
  const int len = hw - p0 < BN_APPLY_ELEMS ? hw - p0 : BN_APPLY_ELEMS;
  const Segment sg = segment(plane * hw + p0, len, align);
  const int t = threadIdx.x;
  for (int i = t; i < sg.head; i += BN_THREADS) y[sg.g0 + i] = x[sg.g0 + i] * scale + shift;
  const f32x4* xv = (const f32x4*)(x + sg.g0 + sg.head);
  f32x4* yv = (f32x4*)(y + sg.g0 + sg.head);
  f32x4 r[BN_APPLY_VEC];
#pragma unroll
  for (int u = 0; u < BN_APPLY_VEC; ++u)
    if (t + u * BN_THREADS < sg.nvec) r[u] = xv[t + u * BN_THREADS];
#pragma unroll
  for (int u = 0; u < BN_APPLY_VEC; ++u)
    if (t + u * BN_THREADS < sg.nvec) yv[t + u * BN_THREADS] = r[u] * scale + shift;
  if (t < sg.tail) {
    const long long i = sg.g0 + sg.head + 4 * (long long)sg.nvec + t;
    y[i] = x[i] * scale + shift;
  }
}

// (channel c, slab s) -> partial sums of dy and dy * xhat, xhat = (x - mean) invstd
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    const float* __restrict__ save_mean,
                                                                    const float* __restrict__ save_invstd,
                                                                    float* __restrict__ p1, float* __restrict__ p2, int C, int hw,
                                                                    long long m, long long chunk, int S, int align) {
  const int c = blockIdx.x, sidx = blockIdx.y, t = threadIdx.x;
  const long long lo = (long long)sidx * chunk, hi = lo + chunk < m ? lo + chunk : m;
  const float mean = save_mean[c], invstd = save_invstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (long long base = lo; base < hi;) {
    const long long n = base / hw;
    const int p0 = (int)(base - n * hw);
    const int len = (int)((hi - base) < (long long)(hw - p0) ? (hi - base) : (hw - p0));
    const Segment sg = segment((n * C + c) * hw + p0, len, align);
    for (int i = t; i < sg.head; i += BN_THREADS) {
      const float g = dy[sg.g0 + i];
      s1 += g;
      s2 += g * ((x[sg.g0 + i] - mean) * invstd);
    }
    const f32x4* xv = (const f32x4*)(x + sg.g0 + sg.head);
    const f32x4* gv = (const f32x4*)(dy + sg.g0 + sg.head);
    int v = t;
    for (; v + BN_THREADS < sg.nvec; v += 2 * BN_THREADS) {        // two vectors of each operand in flight per lane
      const f32x4 xa = xv[v], xb = xv[v + BN_THREADS], ga = gv[v], gb = gv[v + BN_THREADS];
      const f32x4 ha = (xa - mean) * invstd, hb = (xb - mean) * invstd;
      s1 += ((ga[0] + ga[1]) + (ga[2] + ga[3])) + ((gb[0] + gb[1]) + (gb[2] + gb[3]));
      s2 += ((ga[0] * ha[0] + ga[1] * ha[1]) + (ga[2] * ha[2] + ga[3] * ha[3])) +
            ((gb[0] * hb[0] + gb[1] * hb[1]) + (gb[2] * hb[2] + gb[3] * hb[3]));
    }
    for (; v < sg.nvec; v += BN_THREADS) {
      const f32x4 xa = xv[v], ga = gv[v];
      const f32x4 ha = (xa - mean) * invstd;
      s1 += (ga[0] + ga[1]) + (ga[2] + ga[3]);
      s2 += (ga[0] * ha[0] + ga[1] * ha[1]) + (ga[2] * ha[2] + ga[3] * ha[3]);
    }
    if (t < sg.tail) {
      const long long i = sg.g0 + sg.head + 4 * (long long)sg.nvec + t;
      const float g = dy[i];
      s1 += g;
      s2 += g * ((x[i] - mean) * invstd);
    }
    base += len;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  __shared__ float w1[BN_THREADS / 64], w2[BN_THREADS / 64];
  if ((t & 63) == 0) {
    w1[t >> 6] = s1;
    w2[t >> 6] = s2;
  }
  __syncthreads();
  if (t == 0) {
    p1[c * S + sidx] = (w1[0] + w1[1]) + (w1[2] + w1[3]);
    p2[c * S + sidx] = (w2[0] + w2[1]) + (w2[2] + w2[3]);
  }
}

// one thread per channel: dbeta = sum dy, dgamma = sum dy xhat (slabs in index order, double); coef = {k, a, b} of the element
// pass dx = k dy - (a + xhat b), k = gamma invstd, a = k sum_dy / M, b = k sum_dy_xhat / M
__global__ void bn_bwd_final_kernel(const float* __restrict__ p1, const float* __restrict__ p2, const float* gamma,
                                    const float* __restrict__ save_invstd, float* dgamma, float* dbeta, float* __restrict__ coef,
                                    int C, long long m, int S) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < S; ++s) {
    s1 += (double)p1[c * S + s];
    s2 += (double)p2[c * S + s];
  }
  if (dbeta) dbeta[c] = (float)s1;
  if (dgamma) dgamma[c] = (float)s2;
  const double k = (double)(gamma ? gamma[c] : 1.f) * (double)save_invstd[c];
  coef[c] = (float)k;
  coef[C + c] = (float)(k * s1 / (double)m);
  coef[2 * C + c] = (float)(k * s2 / (double)m);
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  float* __restrict__ dx, const float* __restrict__ save_mean,
                                                                  const float* __restrict__ save_invstd,
                                                                  const float* __restrict__ coef, int C, int hw, int pieces,
                                                                  int align) {
  const long long plane = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - plane * pieces);
  const int c = (int)(plane % C);
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float k = coef[c], a = coef[C + c], b = coef[2 * C + c];
  const int p0 = piece * BN_APPLY_ELEMS;
  const int len = hw - p0 < BN_APPLY_ELEMS ? hw - p0 : BN_APPLY_ELEMS;
  const Segment sg = segment(plane * hw + p0, len, align);
  const int t = threadIdx.x;
  for (int j = t; j < sg.head; j += BN_THREADS) {
    const long long i = sg.g0 + j;
    dx[i] = k * dy[i] - (a + ((x[i] - mean) * invstd) * b);
  }
  const f32x4* xv = (const f32x4*)(x + sg.g0 + sg.head);
  const f32x4* gv = (const f32x4*)(dy + sg.g0 + sg.head);
  f32x4* dv = (f32x4*)(dx + sg.g0 + sg.head);
  f32x4 rx[BN_APPLY_VEC], rg[BN_APPLY_VEC];
#pragma unroll
  for (int u = 0; u < BN_APPLY_VEC; ++u)
    if (t + u * BN_THREADS < sg.nvec) {
      rx[u] = xv[t + u * BN_THREADS];
      rg[u] = gv[t + u * BN_THREADS];
    }
#pragma unroll
  for (int u = 0; u < BN_APPLY_VEC; ++u)
    if (t + u * BN_THREADS < sg.nvec) dv[t + u * BN_THREADS] = k * rg[u] - (a + ((rx[u] - mean) * invstd) * b);
  if (t < sg.tail) {
    const long long i = sg.g0 + sg.head + 4 * (long long)sg.nvec + t;
    dx[i] = k * dy[i] - (a + ((x[i] - mean) * invstd) * b);
  }
}

// the tensors' common offset in floats from a 16-byte boundary, -1 when they differ (NULL pointers do not count)
int shift_of(std::initializer_list<const void*> ps) {
  int s = -2;
  for (const void* p : ps) {
    if (!p) continue;
    const int q = (int)(((uintptr_t)p >> 2) & 3);
    if (s == -2) s = q;
    else if (s != q) return -1;
  }
  return s < 0 ? -1 : s;
}
bool aligned4(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 3) return false;
  return true;
}

int check_desc(const dlwp_batchnorm& d, const char* who) {
  DLWP_CHECK_ARG(d.n >= 0 && d.c > 0 && d.hw > 0 && d.epsilon >= 0.f, "%s: bad shape (n %d, c %d, hw %d) or epsilon", who, d.n,
                 d.c, d.hw);
  return DLWP_OK;
}

inline int pieces_of(int hw) { return (hw + BN_APPLY_ELEMS - 1) / BN_APPLY_ELEMS; }

}  // namespace

extern "C" {

size_t dlwp_batchnorm_workspace(dlwp_batchnorm d) {
  if (d.n < 0 || d.c <= 0 || d.hw <= 0) return 0;
  return bn_ws_floats(d) * sizeof(float);
}

int dlwp_batchnorm_fwd_train(dlwp_handle_t h, const void* x, void* y, const void* gamma, const void* beta, void* moving_mean,
                             void* moving_var, void* save_mean, void* save_invstd, void* ws, size_t ws_bytes, dlwp_batchnorm d,
                             void* stream) {
  DLWP_TAPE(h, stream, dlwp_batchnorm_fwd_train, h, x, y, gamma, beta, moving_mean, moving_var, save_mean, save_invstd, ws,
            ws_bytes, d);
  const int rc = check_desc(d, "dlwp_batchnorm_fwd_train");
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && x && y && moving_mean && moving_var && save_mean && save_invstd && ws,
                 "dlwp_batchnorm_fwd_train: null handle or pointer");
  DLWP_CHECK_ARG(aligned4({x, y}), "dlwp_batchnorm_fwd_train: x and y must be float aligned");
  const int align = shift_of({x, y});
  const long long m = (long long)d.n * d.hw;
  DLWP_CHECK_ARG(m > 1, "dlwp_batchnorm_fwd_train: %lld values per channel (the unbiased moving variance needs 2 or more)", m);
  DLWP_CHECK_ARG(ws_bytes >= dlwp_batchnorm_workspace(d), "dlwp_batchnorm_fwd_train: workspace too small");
  const int S = bn_split(d);
  const long long chunk = bn_chunk(m, S);
  float* pm = (float*)ws;
  float* p2 = pm + (size_t)d.c * S;
  float* coef = p2 + (size_t)d.c * S;
  hipStream_t s = (hipStream_t)stream;
  bn_stats_partial_kernel<<<dim3(d.c, S), BN_THREADS, 0, s>>>((const float*)x, pm, p2, d.c, d.hw, m, chunk, S, align);
  bn_stats_final_kernel<<<dlwp_ceil_div(d.c, 64), 64, 0, s>>>(pm, p2, (const float*)gamma, (const float*)beta,
                                                              (float*)moving_mean, (float*)moving_var, (float*)save_mean,
                                                              (float*)save_invstd, coef, d.c, m, chunk, S, d.momentum,
                                                              d.epsilon);
  const int pieces = pieces_of(d.hw);
  bn_apply_kernel<false><<<dim3((unsigned)((long long)d.n * d.c * pieces)), BN_THREADS, 0, s>>>(
      (const float*)x, (float*)y, coef, nullptr, nullptr, nullptr, nullptr, 0.f, d.c, d.hw, pieces, align);
  DLWP_LAUNCH_CHECK("batchnorm_fwd_train kernels");
  return DLWP_OK;
}

int dlwp_batchnorm_fwd_infer(dlwp_handle_t h, const void* x, void* y, const void* gamma, const void* beta,
                             const void* moving_mean, const void* moving_var, dlwp_batchnorm d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_batchnorm_fwd_infer, h, x, y, gamma, beta, moving_mean, moving_var, d);
  const int rc = check_desc(d, "dlwp_batchnorm_fwd_infer");
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && x && y && moving_mean && moving_var, "dlwp_batchnorm_fwd_infer: null handle or pointer");
  DLWP_CHECK_ARG(aligned4({x, y}), "dlwp_batchnorm_fwd_infer: x and y must be float aligned");
  const int align = shift_of({x, y});
  if (d.n == 0) return DLWP_OK;
  const int pieces = pieces_of(d.hw);
  bn_apply_kernel<true><<<dim3((unsigned)((long long)d.n * d.c * pieces)), BN_THREADS, 0, (hipStream_t)stream>>>(
      (const float*)x, (float*)y, nullptr, (const float*)gamma, (const float*)beta, (const float*)moving_mean,
      (const float*)moving_var, d.epsilon, d.c, d.hw, pieces, align);
  DLWP_LAUNCH_CHECK("batchnorm_fwd_infer kernel");
  return DLWP_OK;
}

int dlwp_batchnorm_bwd(dlwp_handle_t h, const void* x, const void* dy, void* dx, const void* gamma, const void* save_mean,
                       const void* save_invstd, void* dgamma, void* dbeta, void* ws, size_t ws_bytes, dlwp_batchnorm d,
                       void* stream) {
  DLWP_TAPE(h, stream, dlwp_batchnorm_bwd, h, x, dy, dx, gamma, save_mean, save_invstd, dgamma, dbeta, ws, ws_bytes, d);
  const int rc = check_desc(d, "dlwp_batchnorm_bwd");
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && x && dy && save_mean && save_invstd && ws, "dlwp_batchnorm_bwd: null handle or pointer");
  DLWP_CHECK_ARG(aligned4({x, dy, dx}), "dlwp_batchnorm_bwd: tensors must be float aligned");
  DLWP_CHECK_ARG(dx != x && dx != dy, "dlwp_batchnorm_bwd: dx must not alias x or dy");
  DLWP_CHECK_ARG(ws_bytes >= dlwp_batchnorm_workspace(d), "dlwp_batchnorm_bwd: workspace too small");
  const long long m = (long long)d.n * d.hw;
  DLWP_CHECK_ARG(m > 0, "dlwp_batchnorm_bwd: empty batch");
  const int S = bn_split(d);
  const long long chunk = bn_chunk(m, S);
  float* p1 = (float*)ws;
  float* p2 = p1 + (size_t)d.c * S;
  float* coef = p2 + (size_t)d.c * S;
  hipStream_t s = (hipStream_t)stream;
  bn_bwd_partial_kernel<<<dim3(d.c, S), BN_THREADS, 0, s>>>((const float*)x, (const float*)dy, (const float*)save_mean,
                                                            (const float*)save_invstd, p1, p2, d.c, d.hw, m, chunk, S,
                                                            shift_of({x, dy}));
  bn_bwd_final_kernel<<<dlwp_ceil_div(d.c, 64), 64, 0, s>>>(p1, p2, (const float*)gamma, (const float*)save_invstd,
                                                            (float*)dgamma, (float*)dbeta, coef, d.c, m, S);
  if (dx) {
    const int pieces = pieces_of(d.hw);
    bn_bwd_apply_kernel<<<dim3((unsigned)((long long)d.n * d.c * pieces)), BN_THREADS, 0, s>>>(
        (const float*)x, (const float*)dy, (float*)dx, (const float*)save_mean, (const float*)save_invstd, coef, d.c, d.hw,
        pieces, shift_of({x, dy, dx}));
  }
  DLWP_LAUNCH_CHECK("batchnorm_bwd kernels");
  return DLWP_OK;
}

}  // extern "C"
