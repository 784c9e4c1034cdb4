// eltwise.hip -- keras activation layers (Activation, LeakyReLU, ReLU, ELU, ThresholdedReLU) and merge layers (Add, Subtract,
// Multiply, Average, Maximum, Minimum) on flat contiguous float32 tensors: four HBM-bound kernels, forward and backward of each
// family.  gfx950 only.
//
// One shape for all four: 256 threads, lane q of the grid owns the QUAD of elements [4 q, 4 q + 4), the grid is
// min(ceil(n / 1024), 8 CUs) workgroups that stride over the quads.  With every operand pointer 16-byte aligned a whole quad moves
// as one 16-byte load / store per operand; the last, ragged quad and every quad of a misaligned call go element by element.  The
// kind (and the number of merge sources) is a template argument: a launch dispatches ONCE on the descriptor, the loop has no
// per-element branch on it (what such branches cost: the convlstm epilogue history).  No LDS, no atomics,
// every element is written by exactly one lane: two runs give the same bits.
//
// Arithmetic is the closed forms of DESIGN.md section 5.25, rounded once per operation in the order written there: nothing here
// can contract into a fused multiply-add (no product feeds a sum), divisions are IEEE (correctly rounded).
#include "common.h"
#include "conv_fwd_kernel.h"  // dlwp_tanh
#include "tape.h"

#include <cmath>
#include <initializer_list>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int ELT_THREADS = 256;

constexpr float SELU_ALPHA = 1.6732632423543772f, SELU_SCALE = 1.0507009873554805f;

struct act_par {
  float alpha, max_value, theta;
};

__device__ __forceinline__ float elt_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// y = f(x).  NaN in, NaN out: every branch either computes with x or hands x through.
template <int KIND>
__device__ __forceinline__ float act_fwd1(float x, const act_par p) {
  if constexpr (KIND == DLWP_ELT_RELU) {
    if (x > p.theta) return fminf(x, p.max_value);        // (x is a number here; max_value = +inf: no cap)
    if (p.alpha == 0.f) return x != x ? x : 0.f;          // (0 (x - theta) would turn -inf into NaN)
    return p.alpha * (x - p.theta);
  } else if constexpr (KIND == DLWP_ELT_ELU) {
    return x > 0.f ? x : p.alpha * (expf(x) - 1.f);
  } else if constexpr (KIND == DLWP_ELT_SELU) {
    return SELU_SCALE * (x > 0.f ? x : SELU_ALPHA * (expf(x) - 1.f));
  } else if constexpr (KIND == DLWP_ELT_SIGMOID) {
    return elt_sigmoid(x);
  } else if constexpr (KIND == DLWP_ELT_HARD_SIGMOID) {
    const float t = 0.2f * x + 0.5f;
    return x != x ? x : (t < 0.f ? 0.f : (t > 1.f ? 1.f : t));
  } else if constexpr (KIND == DLWP_ELT_SOFTPLUS) {
    return (x > 0.f ? x : 0.f) + log1pf(expf(-fabsf(x)));  // log(1 + e^x) without the overflow of e^x
  } else if constexpr (KIND == DLWP_ELT_SOFTSIGN) {
    return x / (1.f + fabsf(x));
  } else {
    return dlwp_tanh(x);
  }
}

// dy/dx from the stored INPUT x
template <int KIND>
__device__ __forceinline__ float act_slope1(float x, const act_par p) {
  float d;
  if constexpr (KIND == DLWP_ELT_RELU) {
    d = x > p.theta ? (x <= p.max_value ? 1.f : 0.f) : p.alpha;
  } else if constexpr (KIND == DLWP_ELT_ELU) {
    d = x > 0.f ? 1.f : p.alpha * expf(x);
  } else if constexpr (KIND == DLWP_ELT_SELU) {
    d = SELU_SCALE * (x > 0.f ? 1.f : SELU_ALPHA * expf(x));
  } else if constexpr (KIND == DLWP_ELT_SIGMOID) {
    const float y = elt_sigmoid(x);
    d = y * (1.f - y);
  } else if constexpr (KIND == DLWP_ELT_HARD_SIGMOID) {
    d = (x > -2.5f && x < 2.5f) ? 0.2f : 0.f;
  } else if constexpr (KIND == DLWP_ELT_SOFTPLUS) {
    d = elt_sigmoid(x);
  } else if constexpr (KIND == DLWP_ELT_SOFTSIGN) {
    const float t = 1.f + fabsf(x);
    d = 1.f / (t * t);
  } else {
    const float y = dlwp_tanh(x);
    d = 1.f - y * y;
  }
  return x != x ? x : d;
}

template <int KIND, bool BWD>
__global__ __launch_bounds__(ELT_THREADS) void activation_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 float* __restrict__ out, long long n, act_par p, int vec) {
  const long long quads = (n + 3) >> 2, stride = (long long)gridDim.x * ELT_THREADS;
  for (long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x; q < quads; q += stride) {
    const long long i0 = q << 2;
    if (vec && i0 + 4 <= n) {
      const f32x4 v = *(const f32x4*)(x + i0);
      f32x4 o;
      if constexpr (BWD) {
        const f32x4 g = *(const f32x4*)(dy + i0);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = g[i] * act_slope1<KIND>(v[i], p);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = act_fwd1<KIND>(v[i], p);
      }
      *(f32x4*)(out + i0) = o;
    } else {
      const int m = n - i0 < 4 ? (int)(n - i0) : 4;
      for (int i = 0; i < m; ++i) {
        if constexpr (BWD) out[i0 + i] = dy[i0 + i] * act_slope1<KIND>(x[i0 + i], p);
        else out[i0 + i] = act_fwd1<KIND>(x[i0 + i], p);
      }
    }
  }
}

// ---- merge layers: ((a o b) o c) o d, left to right -------------------------------------------------------------------------
// Maximum / Minimum propagate NaN like np.maximum / np.minimum (fmaxf / fminf would drop it); of two equal operands the LEFT one
// is kept, so the sign of a zero is the left operand's
template <int KIND>
__device__ __forceinline__ float merge2(float a, float b) {
  if constexpr (KIND == DLWP_MERGE_ADD || KIND == DLWP_MERGE_AVERAGE) return a + b;
  else if constexpr (KIND == DLWP_MERGE_SUBTRACT) return a - b;
  else if constexpr (KIND == DLWP_MERGE_MULTIPLY) return a * b;
  else if constexpr (KIND == DLWP_MERGE_MAXIMUM) return (a >= b || a != a) ? a : b;
  else return (a <= b || a != a) ? a : b;
}

template <int KIND, int NS>
__device__ __forceinline__ float merge_fwd1(const float* v) {
  float r = merge2<KIND>(v[0], v[1]);
#pragma unroll
  for (int s = 2; s < NS; ++s) r = merge2<KIND>(r, v[s]);
  if constexpr (KIND == DLWP_MERGE_AVERAGE) r = r / (float)NS;
  return r;
}

// every input's gradient of one element
template <int KIND, int NS>
__device__ __forceinline__ void merge_bwd1(const float* v, float g, float* d) {
  if constexpr (KIND == DLWP_MERGE_ADD) {
#pragma unroll
    for (int s = 0; s < NS; ++s) d[s] = g;
  } else if constexpr (KIND == DLWP_MERGE_SUBTRACT) {
    d[0] = g;
    d[1] = -g;
  } else if constexpr (KIND == DLWP_MERGE_AVERAGE) {
    const float ga = g / (float)NS;
#pragma unroll
    for (int s = 0; s < NS; ++s) d[s] = ga;
  } else if constexpr (KIND == DLWP_MERGE_MULTIPLY) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {       // dy times the product of the OTHER inputs, multiplied up in input order
      float p = 1.f;
      bool first = true;
#pragma unroll
      for (int t = 0; t < NS; ++t) {
        if (t == s) continue;
        p = first ? v[t] : p * v[t];
        first = false;
      }
      d[s] = g * p;
    }
  } else {                               // Maximum / Minimum: the FIRST input that attains the result takes dy
    const float r = merge_fwd1<KIND, NS>(v);
    bool found = false;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bool hit = !found && v[s] == r;
      d[s] = hit ? g : 0.f;
      found = found || hit;
    }
  }
}

struct merge_ptrs {
  const float* x[4];
  float* dx[4];      // backward only; a null entry is not written
};

template <int KIND, int NS>
__global__ __launch_bounds__(ELT_THREADS) void merge_fwd_kernel(merge_ptrs P, float* __restrict__ y, long long n, int vec) {
  const long long quads = (n + 3) >> 2, stride = (long long)gridDim.x * ELT_THREADS;
  for (long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x; q < quads; q += stride) {
    const long long i0 = q << 2;
    if (vec && i0 + 4 <= n) {
      f32x4 v[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) v[s] = *(const f32x4*)(P.x[s] + i0);
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float e[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) e[s] = v[s][i];
        o[i] = merge_fwd1<KIND, NS>(e);
      }
      *(f32x4*)(y + i0) = o;
    } else {
      const int m = n - i0 < 4 ? (int)(n - i0) : 4;
      for (int i = 0; i < m; ++i) {
        float e[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) e[s] = P.x[s][i0 + i];
        y[i0 + i] = merge_fwd1<KIND, NS>(e);
      }
    }
  }
}

template <int KIND, int NS>
__global__ __launch_bounds__(ELT_THREADS) void merge_bwd_kernel(merge_ptrs P, const float* __restrict__ dy, long long n, int vec) {
  const long long quads = (n + 3) >> 2, stride = (long long)gridDim.x * ELT_THREADS;
  for (long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x; q < quads; q += stride) {
    const long long i0 = q << 2;
    if (vec && i0 + 4 <= n) {
      f32x4 v[NS], o[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) v[s] = *(const f32x4*)(P.x[s] + i0);
      const f32x4 g = *(const f32x4*)(dy + i0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float e[NS], d[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) e[s] = v[s][i];
        merge_bwd1<KIND, NS>(e, g[i], d);
#pragma unroll
        for (int s = 0; s < NS; ++s) o[s][i] = d[s];
      }
#pragma unroll
      for (int s = 0; s < NS; ++s)
        if (P.dx[s]) *(f32x4*)(P.dx[s] + i0) = o[s];
    } else {
      const int m = n - i0 < 4 ? (int)(n - i0) : 4;
      for (int i = 0; i < m; ++i) {
        float e[NS], d[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) e[s] = P.x[s][i0 + i];
        merge_bwd1<KIND, NS>(e, dy[i0 + i], d);
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (P.dx[s]) P.dx[s][i0 + i] = d[s];
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
bool elt_aligned(std::initializer_list<const void*> ps, uintptr_t mask) {
  for (const void* p : ps)
    if ((uintptr_t)p & mask) return false;
  return true;
}

int elt_grid(long long n, int cu) {
  const long long want = (n + 4 * ELT_THREADS - 1) / (4 * ELT_THREADS), cap = (long long)(cu > 0 ? cu : 256) * 8;
  return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}

int act_check(const dlwp_activation& d, long long n, const char* who) {
  DLWP_CHECK_ARG(n >= 0 && n < (1ll << 40), "%s: bad element count %lld", who, n);
  DLWP_CHECK_ARG(d.kind >= DLWP_ELT_RELU && d.kind <= DLWP_ELT_TANH, "%s: bad activation kind %d", who, d.kind);
  if (d.kind == DLWP_ELT_RELU) {
    DLWP_CHECK_ARG(d.alpha >= 0.f && std::isfinite(d.alpha), "%s: negative slope %g (finite, >= 0)", who, (double)d.alpha);
    DLWP_CHECK_ARG(d.theta >= 0.f && std::isfinite(d.theta), "%s: threshold %g (finite, >= 0)", who, (double)d.theta);
    DLWP_CHECK_ARG(d.max_value > d.theta, "%s: max_value %g must exceed the threshold %g (+inf: no cap)", who, (double)d.max_value,
                   (double)d.theta);
  }
  if (d.kind == DLWP_ELT_ELU) DLWP_CHECK_ARG(std::isfinite(d.alpha), "%s: alpha %g", who, (double)d.alpha);
  return DLWP_OK;
}

template <bool BWD>
int act_launch(const char* who, dlwp_handle_t h, const void* x, const void* dy, void* out, long long n, const dlwp_activation& d,
               void* stream) {
  const int rc = act_check(d, n, who);
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && (n == 0 || (x && out && (!BWD || dy))), "%s: null handle or pointer", who);
  DLWP_CHECK_ARG(elt_aligned({x, dy, out}, 3), "%s: tensors must be float aligned", who);
  DLWP_CHECK_ARG(n == 0 || (out != x && out != dy), "%s: the result must not alias an operand", who);
  if (n == 0) return DLWP_OK;
  const int vec = elt_aligned({x, dy, out}, 15) ? 1 : 0, grid = elt_grid(n, h->cu_count);
  const act_par p{d.alpha, d.max_value, d.theta};
  hipStream_t s = (hipStream_t)stream;
#define ELT_ACT_CASE(K)                                                                                                   \
  case K:                                                                                                                 \
    activation_kernel<K, BWD><<<grid, ELT_THREADS, 0, s>>>((const float*)x, (const float*)dy, (float*)out, n, p, vec);   \
    break;
  switch (d.kind) {
    ELT_ACT_CASE(DLWP_ELT_RELU)
    ELT_ACT_CASE(DLWP_ELT_ELU)
    ELT_ACT_CASE(DLWP_ELT_SELU)
    ELT_ACT_CASE(DLWP_ELT_SIGMOID)
    ELT_ACT_CASE(DLWP_ELT_HARD_SIGMOID)
    ELT_ACT_CASE(DLWP_ELT_SOFTPLUS)
    ELT_ACT_CASE(DLWP_ELT_SOFTSIGN)
    ELT_ACT_CASE(DLWP_ELT_TANH)
  }
#undef ELT_ACT_CASE
  DLWP_LAUNCH_CHECK(who);
  return DLWP_OK;
}

int merge_check(const dlwp_merge& d, long long n, const char* who) {
  DLWP_CHECK_ARG(n >= 0 && n < (1ll << 40), "%s: bad element count %lld", who, n);
  DLWP_CHECK_ARG(d.kind >= DLWP_MERGE_ADD && d.kind <= DLWP_MERGE_MINIMUM, "%s: bad merge kind %d", who, d.kind);
  DLWP_CHECK_ARG(d.n_src >= 2 && d.n_src <= 4, "%s: %d sources (2 to 4)", who, d.n_src);
  DLWP_CHECK_ARG(d.kind != DLWP_MERGE_SUBTRACT || d.n_src == 2, "%s: Subtract takes exactly 2 sources, got %d", who, d.n_src);
  return DLWP_OK;
}

template <bool BWD, int KIND>
void merge_launch_n(int n_src, int grid, hipStream_t s, const merge_ptrs& P, const float* dy, float* y, long long n, int vec) {
  if constexpr (BWD) {
    if (n_src == 2) merge_bwd_kernel<KIND, 2><<<grid, ELT_THREADS, 0, s>>>(P, dy, n, vec);
    else if (n_src == 3) merge_bwd_kernel<KIND, 3><<<grid, ELT_THREADS, 0, s>>>(P, dy, n, vec);
    else merge_bwd_kernel<KIND, 4><<<grid, ELT_THREADS, 0, s>>>(P, dy, n, vec);
  } else {
    if (n_src == 2) merge_fwd_kernel<KIND, 2><<<grid, ELT_THREADS, 0, s>>>(P, y, n, vec);
    else if (n_src == 3) merge_fwd_kernel<KIND, 3><<<grid, ELT_THREADS, 0, s>>>(P, y, n, vec);
    else merge_fwd_kernel<KIND, 4><<<grid, ELT_THREADS, 0, s>>>(P, y, n, vec);
  }
}

template <bool BWD>
int merge_launch(const char* who, dlwp_handle_t h, const void* const* x, const void* dy, void* y, void* const* dx, long long n,
                 const dlwp_merge& d, void* stream) {
  const int rc = merge_check(d, n, who);
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h, "%s: null handle", who);
  merge_ptrs P{};
  bool vec = elt_aligned({dy, y}, 15), any_dx = false;
  for (int s = 0; s < d.n_src; ++s) {
    DLWP_CHECK_ARG(n == 0 || x[s], "%s: source %d is null", who, s);
    DLWP_CHECK_ARG(elt_aligned({x[s], BWD ? dx[s] : nullptr}, 3), "%s: tensors must be float aligned", who);
    DLWP_CHECK_ARG(BWD || n == 0 || y != x[s], "%s: y must not alias source %d", who, s);
    P.x[s] = (const float*)x[s];
    vec = vec && elt_aligned({x[s]}, 15);
    if (BWD) {
      P.dx[s] = (float*)dx[s];
      vec = vec && elt_aligned({dx[s]}, 15);
      any_dx = any_dx || dx[s];
      // one tensor per input: two inputs sharing a gradient tensor would each lose what the other wrote
      for (int t = 0; t < s; ++t) DLWP_CHECK_ARG(!dx[s] || dx[s] != dx[t], "%s: dx%d and dx%d are the same tensor", who, t, s);
      for (int t = 0; t < d.n_src; ++t) DLWP_CHECK_ARG(!dx[s] || dx[s] != x[t], "%s: dx%d aliases source %d", who, s, t);
      DLWP_CHECK_ARG(!dx[s] || dx[s] != dy, "%s: dx%d aliases dy", who, s);
    }
  }
  DLWP_CHECK_ARG(elt_aligned({dy, y}, 3), "%s: tensors must be float aligned", who);
  DLWP_CHECK_ARG(n == 0 || (BWD ? dy != nullptr : y != nullptr), "%s: null %s", who, BWD ? "dy" : "y");
  if (n == 0 || (BWD && !any_dx)) return DLWP_OK;
  const int grid = elt_grid(n, h->cu_count);
  hipStream_t s = (hipStream_t)stream;
#define ELT_MERGE_CASE(K)                                                                                        \
  case K:                                                                                                        \
    merge_launch_n<BWD, K>(d.n_src, grid, s, P, (const float*)dy, (float*)y, n, vec ? 1 : 0);                    \
    break;
  switch (d.kind) {
    ELT_MERGE_CASE(DLWP_MERGE_ADD)
    ELT_MERGE_CASE(DLWP_MERGE_SUBTRACT)
    ELT_MERGE_CASE(DLWP_MERGE_MULTIPLY)
    ELT_MERGE_CASE(DLWP_MERGE_AVERAGE)
    ELT_MERGE_CASE(DLWP_MERGE_MAXIMUM)
    ELT_MERGE_CASE(DLWP_MERGE_MINIMUM)
  }
#undef ELT_MERGE_CASE
  DLWP_LAUNCH_CHECK(who);
  return DLWP_OK;
}

}  // namespace

extern "C" {

int dlwp_activation_fwd(dlwp_handle_t h, const void* x, void* y, long long n, dlwp_activation d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_activation_fwd, h, x, y, n, d);
  return act_launch<false>("dlwp_activation_fwd", h, x, nullptr, y, n, d, stream);
}

int dlwp_activation_bwd(dlwp_handle_t h, const void* x, const void* dy, void* dx, long long n, dlwp_activation d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_activation_bwd, h, x, dy, dx, n, d);
  return act_launch<true>("dlwp_activation_bwd", h, x, dy, dx, n, d, stream);
}

int dlwp_merge_fwd(dlwp_handle_t h, const void* x0, const void* x1, const void* x2, const void* x3, void* y, long long n,
                   dlwp_merge d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_merge_fwd, h, x0, x1, x2, x3, y, n, d);
  const void* const x[4] = {x0, x1, x2, x3};
  return merge_launch<false>("dlwp_merge_fwd", h, x, nullptr, y, nullptr, n, d, stream);
}

int dlwp_merge_bwd(dlwp_handle_t h, const void* x0, const void* x1, const void* x2, const void* x3, const void* dy, void* dx0,
                   void* dx1, void* dx2, void* dx3, long long n, dlwp_merge d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_merge_bwd, h, x0, x1, x2, x3, dy, dx0, dx1, dx2, dx3, n, d);
  const void* const x[4] = {x0, x1, x2, x3};
  void* const dx[4] = {dx0, dx1, dx2, dx3};
  return merge_launch<true>("dlwp_merge_bwd", h, x, dy, nullptr, dx, n, d, stream);
}

}  // extern "C"
