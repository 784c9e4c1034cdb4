// optimizers.hip -- the Keras 2.2.4 optimizers beyond plain Adam / SGD (keras/optimizers.py get_updates) and Keras' gradient
// clipping (Optimizer.get_gradients) on flat float32 buffers: ONE update entry with a kind code, ONE clip entry.
//
// The reference compiles its models with 'adam' (examples/train.py:240); a Keras user passes any of the seven names, amsgrad,
// nesterov and clipnorm / clipvalue.  dlwp_adam_keras / dlwp_sgd_keras (train_ops.hip) stay the path of unclipped Adam / SGD.
//
// The update of 215 M parameters (the dense model of tools/bench_dense.py) is an HBM stream of 3-6 arrays: where p, the slots and g
// sit at the same offset inside a 16-byte unit the body moves float4, head (< 4 elements) and tail (< 4) go one by one in block 0;
// arrays at different offsets take the element-wise kernel.  Nothing outside [0, n) is touched, g is only read.
#include "common.h"
#include "tape.h"

namespace {

struct OptArgs {
  float lr;       // lr' = lr / (1 + decay it) (Nadam: lr); Adam / Adamax: lr_t -- double on the host, rounded once
  float h1, h2;   // momentum | rho | beta_1, beta_2
  float eps;
  float c0, c1, c2, c3, c4;   // Nadam: 1 - ms_new, 1 - ms_next, 1 - mu_t, mu_{t+1}, 1 - b2^t
  float gs, clip;             // grad_scale; clipvalue (<= 0: none)
  const float* factor;        // device: the clipnorm factor of dlwp_grad_clip_factor, or null
};

// the gradient the update sees: g * grad_scale, times the clipnorm factor, clamped to +-clipvalue
__device__ __forceinline__ float seen_grad(float g, const OptArgs& a, float factor, bool has_factor) {
  float gi = g * a.gs;
  if (has_factor) gi = gi * factor;
  if (a.clip > 0.f) gi = fminf(fmaxf(gi, -a.clip), a.clip);
  return gi;
}

template <int KIND>
struct Slots {
  static constexpr int n = (KIND == DLWP_OPT_ADAM_AMSGRAD) ? 3
                           : (KIND == DLWP_OPT_ADADELTA || KIND == DLWP_OPT_ADAM || KIND == DLWP_OPT_ADAMAX ||
                              KIND == DLWP_OPT_NADAM)
                                 ? 2
                                 : 1;
};

// one element; gi is the clipped gradient.  The operation order is the contract of tests/test_keras_optimizers_cpu.py.
template <int KIND>
__device__ __forceinline__ void update(float& p, float& s0, float& s1, float& s2, float gi, const OptArgs& a) {
  if constexpr (KIND == DLWP_OPT_SGD) {  // v = mom m - lr g; m <- v; p += v
    const float v = a.h1 * s0 - a.lr * gi;
    s0 = v;
    p = p + v;
  } else if constexpr (KIND == DLWP_OPT_SGD_NESTEROV) {  // p += mom v - lr g
    const float t2 = a.lr * gi;
    const float v = a.h1 * s0 - t2;
    s0 = v;
    p = p + (a.h1 * v - t2);
  } else if constexpr (KIND == DLWP_OPT_RMSPROP) {
    const float an = a.h1 * s0 + (1.f - a.h1) * gi * gi;
    s0 = an;
    p = p - a.lr * gi / (sqrtf(an) + a.eps);
  } else if constexpr (KIND == DLWP_OPT_ADAGRAD) {
    const float an = s0 + gi * gi;
    s0 = an;
    p = p - a.lr * gi / (sqrtf(an) + a.eps);
  } else if constexpr (KIND == DLWP_OPT_ADADELTA) {
    const float an = a.h1 * s0 + (1.f - a.h1) * gi * gi;
    const float upd = gi * sqrtf(s1 + a.eps) / sqrtf(an + a.eps);
    s0 = an;
    p = p - a.lr * upd;
    s1 = a.h1 * s1 + (1.f - a.h1) * upd * upd;
  } else if constexpr (KIND == DLWP_OPT_ADAM || KIND == DLWP_OPT_ADAM_AMSGRAD) {
    const float mi = a.h1 * s0 + (1.f - a.h1) * gi;
    const float vi = a.h2 * s1 + (1.f - a.h2) * gi * gi;
    s0 = mi;
    s1 = vi;
    float d = vi;
    if constexpr (KIND == DLWP_OPT_ADAM_AMSGRAD) {
      d = fmaxf(s2, vi);
      s2 = d;
    }
    p = p - a.lr * mi / (sqrtf(d) + a.eps);
  } else if constexpr (KIND == DLWP_OPT_ADAMAX) {
    const float mi = a.h1 * s0 + (1.f - a.h1) * gi;
    const float ui = fmaxf(a.h2 * s1, fabsf(gi));
    s0 = mi;
    s1 = ui;
    p = p - a.lr * mi / (ui + a.eps);
  } else {  // DLWP_OPT_NADAM
    const float gp = gi / a.c0;
    const float mi = a.h1 * s0 + (1.f - a.h1) * gi;
    const float mp = mi / a.c1;
    const float vi = a.h2 * s1 + (1.f - a.h2) * gi * gi;
    const float vp = vi / a.c4;
    s0 = mi;
    s1 = vi;
    p = p - a.lr * (a.c2 * gp + a.c3 * mp) / (sqrtf(vp) + a.eps);
  }
}

template <int KIND>
__device__ __forceinline__ void update_at(float* __restrict__ p, float* __restrict__ s0, float* __restrict__ s1,
                                          float* __restrict__ s2, const float* __restrict__ g, long long i, const OptArgs& a,
                                          float factor, bool has_factor) {
  constexpr int NS = Slots<KIND>::n;
  float pi = p[i], a0 = s0[i], a1 = 0.f, a2 = 0.f;
  if constexpr (NS >= 2) a1 = s1[i];
  if constexpr (NS >= 3) a2 = s2[i];
  update<KIND>(pi, a0, a1, a2, seen_grad(g[i], a, factor, has_factor), a);
  p[i] = pi;
  s0[i] = a0;
  if constexpr (NS >= 2) s1[i] = a1;
  if constexpr (NS >= 3) s2[i] = a2;
}

// arrays at different offsets inside a 16-byte unit: one element per thread and trip
template <int KIND>
__global__ __launch_bounds__(256) void opt_step_kernel(float* __restrict__ p, float* __restrict__ s0, float* __restrict__ s1,
                                                       float* __restrict__ s2, const float* __restrict__ g, long long n,
                                                       const OptArgs a) {
  const bool has_factor = a.factor != nullptr;
  const float factor = has_factor ? *a.factor : 1.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    update_at<KIND>(p, s0, s1, s2, g, i, a, factor, has_factor);
}

// every array 16-byte aligned at element `head` (< 4): elements [head, head + 4 nv) as float4, the others in block 0
template <int KIND>
__global__ __launch_bounds__(256) void opt_step_vec_kernel(float* __restrict__ p, float* __restrict__ s0, float* __restrict__ s1,
                                                           float* __restrict__ s2, const float* __restrict__ g, long long n,
                                                           int head, long long nv, const OptArgs a) {
  constexpr int NS = Slots<KIND>::n;
  const bool has_factor = a.factor != nullptr;
  const float factor = has_factor ? *a.factor : 1.f;
  if (blockIdx.x == 0) {
    const long long rest = n - head - 4 * nv;          // < 4
    const int t = threadIdx.x;
    if (t < head) update_at<KIND>(p, s0, s1, s2, g, t, a, factor, has_factor);
    else if (t - head < rest) update_at<KIND>(p, s0, s1, s2, g, head + 4 * nv + (t - head), a, factor, has_factor);
  }
  float4* __restrict__ pv = reinterpret_cast<float4*>(p + head);
  float4* __restrict__ v0 = reinterpret_cast<float4*>(s0 + head);
  float4* __restrict__ v1 = NS >= 2 ? reinterpret_cast<float4*>(s1 + head) : nullptr;
  float4* __restrict__ v2 = NS >= 3 ? reinterpret_cast<float4*>(s2 + head) : nullptr;
  const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
    float4 P = pv[i], A0 = v0[i], A1 = make_float4(0.f, 0.f, 0.f, 0.f), A2 = A1;
    const float4 G = gv[i];
    if constexpr (NS >= 2) A1 = v1[i];
    if constexpr (NS >= 3) A2 = v2[i];
    update<KIND>(P.x, A0.x, A1.x, A2.x, seen_grad(G.x, a, factor, has_factor), a);
    update<KIND>(P.y, A0.y, A1.y, A2.y, seen_grad(G.y, a, factor, has_factor), a);
    update<KIND>(P.z, A0.z, A1.z, A2.z, seen_grad(G.z, a, factor, has_factor), a);
    update<KIND>(P.w, A0.w, A1.w, A2.w, seen_grad(G.w, a, factor, has_factor), a);
    pv[i] = P;
    v0[i] = A0;
    if constexpr (NS >= 2) v1[i] = A1;
    if constexpr (NS >= 3) v2[i] = A2;
  }
}

inline int blocks_for(long long items, int cu) {
  long long want = (items + 255) / 256;
  const long long cap = (long long)cu * 8;
  if (want < 1) want = 1;
  return (int)(want < cap ? want : cap);
}

template <int KIND>
void launch_step(dlwp_handle_t h, float* p, float* s0, float* s1, float* s2, const float* g, long long n, const OptArgs& a,
                 hipStream_t s) {
  constexpr int NS = Slots<KIND>::n;
  const uintptr_t off = (uintptr_t)p & 15;
  bool same = ((uintptr_t)g & 15) == off && ((uintptr_t)s0 & 15) == off;
  if (NS >= 2) same = same && ((uintptr_t)s1 & 15) == off;
  if (NS >= 3) same = same && ((uintptr_t)s2 & 15) == off;
  const int head = (int)(((16 - off) & 15) / 4);
  const long long nv = n > head ? (n - head) / 4 : 0;
  if (same && nv > 0)
    opt_step_vec_kernel<KIND><<<blocks_for(nv, h->cu_count), 256, 0, s>>>(p, s0, s1, s2, g, n, head, nv, a);
  else
    opt_step_kernel<KIND><<<blocks_for(n, h->cu_count), 256, 0, s>>>(p, s0, s1, s2, g, n, a);
}

// ---- clipnorm: sum over i of (g_i grad_scale)^2 by a fixed tree, in double (the products are exact there) ------------------- //
__device__ __forceinline__ double block_sum(double v, double* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];      // (every thread: the same order)
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long long n, int head, long long nv,
                                                            double gs, double* __restrict__ partial) {
  __shared__ double lds[4];
  double acc = 0.0;
  if (blockIdx.x == 0) {
    const long long rest = n - head - 4 * nv;
    const int t = threadIdx.x;
    long long i = -1;
    if (t < head) i = t;
    else if (t - head < rest) i = head + 4 * nv + (t - head);
    if (i >= 0) {
      const double d = (double)g[i] * gs;
      acc = d * d;
    }
  }
  const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
    const float4 G = gv[i];
    const double x = (double)G.x * gs, y = (double)G.y * gs, z = (double)G.z * gs, w = (double)G.w * gs;
    acc += (x * x + y * y) + (z * z + w * w);
  }
  const double tot = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// out3 <- {factor, norm, sum of squares}: factor = clipnorm / norm where norm >= clipnorm, else exactly 1
__global__ __launch_bounds__(256) void clip_factor_kernel(const double* __restrict__ partial, int count, float clipnorm,
                                                          float* __restrict__ out3) {
  __shared__ double lds[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];
  const double tot = block_sum(acc, lds);
  if (threadIdx.x == 0) {
    const double norm = sqrt(tot);
    out3[0] = (clipnorm > 0.f && norm >= (double)clipnorm) ? (float)((double)clipnorm / norm) : 1.f;
    out3[1] = (float)norm;
    out3[2] = (float)tot;
  }
}

}  // namespace

extern "C" {

size_t dlwp_grad_clip_factor_workspace(dlwp_handle_t h) { return h ? (size_t)h->cu_count * 8 * sizeof(double) : 0; }

int dlwp_grad_clip_factor(dlwp_handle_t h, const void* g, size_t n, float grad_scale, float clipnorm, void* ws, size_t ws_bytes,
                          float* factor_dev, void* stream) {
  DLWP_TAPE(h, stream, dlwp_grad_clip_factor, h, g, n, grad_scale, clipnorm, ws, ws_bytes, factor_dev);
  DLWP_CHECK_ARG(h && ws && factor_dev && (g || n == 0), "dlwp_grad_clip_factor: null handle or pointer");
  DLWP_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)ws & 7) == 0, "dlwp_grad_clip_factor: misaligned gradient or workspace");
  DLWP_CHECK_ARG(ws_bytes >= dlwp_grad_clip_factor_workspace(h), "dlwp_grad_clip_factor: workspace too small (%zu < %zu)", ws_bytes,
                 dlwp_grad_clip_factor_workspace(h));
  const int head = n == 0 ? 0 : (int)(((16 - ((uintptr_t)g & 15)) & 15) / 4);
  const long long nv = (long long)n > head ? ((long long)n - head) / 4 : 0;
  const int grid = blocks_for(nv, h->cu_count);
  hipStream_t s = (hipStream_t)stream;
  sumsq_partial_kernel<<<grid, 256, 0, s>>>((const float*)g, (long long)n, nv > 0 ? head : 0, nv, (double)grad_scale, (double*)ws);
  clip_factor_kernel<<<1, 256, 0, s>>>((const double*)ws, grid, clipnorm, factor_dev);
  DLWP_LAUNCH_CHECK("clip factor kernels");
  return DLWP_OK;
}

int dlwp_optimizer_step(dlwp_handle_t h, int kind, void* p, void* s0, void* s1, void* s2, const void* g, size_t n, float lr,
                        float decay, float h1, float h2, float epsilon, float schedule_decay, double m_schedule,
                        long long iteration, float grad_scale, float clipvalue, const float* factor_dev, void* stream) {
  DLWP_TAPE(h, stream, dlwp_optimizer_step, h, kind, p, s0, s1, s2, g, n, lr, decay, h1, h2, epsilon, schedule_decay, m_schedule,
            iteration, grad_scale, clipvalue, factor_dev);
  DLWP_CHECK_ARG(h && p && s0 && g, "dlwp_optimizer_step: null handle or pointer");
  DLWP_CHECK_ARG(kind >= DLWP_OPT_SGD && kind <= DLWP_OPT_NADAM, "dlwp_optimizer_step: unknown kind %d", kind);
  const int ns = kind == DLWP_OPT_ADAM_AMSGRAD ? 3
                 : (kind == DLWP_OPT_ADADELTA || kind == DLWP_OPT_ADAM || kind == DLWP_OPT_ADAMAX || kind == DLWP_OPT_NADAM) ? 2 : 1;
  DLWP_CHECK_ARG((ns < 2 || s1) && (ns < 3 || s2), "dlwp_optimizer_step: kind %d needs %d slot arrays", kind, ns);
  DLWP_CHECK_ARG((((uintptr_t)p | (uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)g) & 3) == 0,
                 "dlwp_optimizer_step: arrays must be float-aligned");
  if (n == 0) return DLWP_OK;
  // step-dependent scalars: double on the host, rounded once (as dlwp_adam_keras has lr_t)
  const double it = (double)iteration, t = it + 1.0;
  const double lr_ = (double)lr / (1.0 + (double)decay * it);
  OptArgs a;
  memset(&a, 0, sizeof(a));
  a.lr = (float)lr_;
  a.h1 = h1;
  a.h2 = h2;
  a.eps = epsilon;
  a.gs = grad_scale;
  a.clip = clipvalue;
  a.factor = factor_dev;
  if (kind == DLWP_OPT_ADAM || kind == DLWP_OPT_ADAM_AMSGRAD) {
    a.lr = (float)(lr_ * sqrt(1.0 - pow((double)h2, t)) / (1.0 - pow((double)h1, t)));
  } else if (kind == DLWP_OPT_ADAMAX) {
    a.lr = (float)(lr_ / (1.0 - pow((double)h1, t)));
  } else if (kind == DLWP_OPT_NADAM) {
    const double sd = (double)schedule_decay;
    const double mu_t = (double)h1 * (1.0 - 0.5 * pow(0.96, t * sd));
    const double mu_t1 = (double)h1 * (1.0 - 0.5 * pow(0.96, (t + 1.0) * sd));
    const double ms_new = m_schedule * mu_t, ms_next = ms_new * mu_t1;
    a.lr = lr;          // (Keras' Nadam has no decay)
    a.c0 = (float)(1.0 - ms_new);
    a.c1 = (float)(1.0 - ms_next);
    a.c2 = (float)(1.0 - mu_t);
    a.c3 = (float)mu_t1;
    a.c4 = (float)(1.0 - pow((double)h2, t));
  }
  hipStream_t s = (hipStream_t)stream;
  float *P = (float*)p, *S0 = (float*)s0, *S1 = (float*)s1, *S2 = (float*)s2;
  const float* G = (const float*)g;
  const long long N = (long long)n;
  switch (kind) {
    case DLWP_OPT_SGD: launch_step<DLWP_OPT_SGD>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_SGD_NESTEROV: launch_step<DLWP_OPT_SGD_NESTEROV>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_RMSPROP: launch_step<DLWP_OPT_RMSPROP>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_ADAGRAD: launch_step<DLWP_OPT_ADAGRAD>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_ADADELTA: launch_step<DLWP_OPT_ADADELTA>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_ADAM: launch_step<DLWP_OPT_ADAM>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_ADAM_AMSGRAD: launch_step<DLWP_OPT_ADAM_AMSGRAD>(h, P, S0, S1, S2, G, N, a, s); break;
    case DLWP_OPT_ADAMAX: launch_step<DLWP_OPT_ADAMAX>(h, P, S0, S1, S2, G, N, a, s); break;
    default: launch_step<DLWP_OPT_NADAM>(h, P, S0, S1, S2, G, N, a, s); break;
  }
  DLWP_LAUNCH_CHECK("optimizer step kernel");
  return DLWP_OK;
}

}  // extern "C"
