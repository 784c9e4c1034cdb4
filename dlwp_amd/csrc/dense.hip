// dense.hip -- keras Dense (forward, data gradient, weight gradient) and Dropout for the non-convolutional models of the reference
// (examples/train_generator.py:224-233: Dense(n_features // 2, tanh, l2) -> Dropout(0.25) -> Dense(n_features)).  gfx950 only.
//
// All three products run on v_mfma_f32_32x32x2_f32: float32 operands, float32 accumulation, every output element a k-ordered fmaf
// chain.  No atomics, no split that depends on the batch: row i of a product is the same bits whatever batch it rides in.
//
//   forward        y[M, N]  = act(x[M, K] W[K, N] + b)       W rows are contiguous along N: the B operand of a wave is two coalesced
//                                                              128-byte runs of W per matrix instruction, straight from global memory
//   data gradient  dx[M, K] = (dy o act'(y))[M, N] W^T        the sum runs along the contiguous axis of W: the 32 rows of W a
//                                                              workgroup needs are read in coalesced runs and transposed through
//                                                              LDS (per-lane row streaming measured 1.05 - 1.3x slower)
//   weight gradient dW[K, N] = x^T (dy o act'(y)), db = sum_m  the sum is over the batch only; a wave owns a 32 x 128 block of dW,
//                                                              both operands staged through LDS in chunks of 32 samples
//
// forward and data gradient share one kernel (dense_mm_kernel<MT, TRANS>): a workgroup of 8 waves owns 32 output columns and up
// to 32 MT rows; the left operand is staged through LDS in chunks of 128 reduction elements, of which each wave multiplies 16; the
// eight partial tiles are summed through LDS in wave order.  The split over the waves is the same for every shape.
#include "common.h"
#include "philox.h"
#include "tape.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DN_THREADS = 256;
constexpr int DN_MM_THREADS = 512;       // forward / data gradient: 8 waves share one 32-column strip
constexpr int DN_WAVES = DN_MM_THREADS / 64;
constexpr int DN_RW = 16;                // reduction elements one wave multiplies per chunk
constexpr int DN_RC = DN_WAVES * DN_RW;  // reduction elements staged per chunk (128)
constexpr int DN_PITCH = DN_RC + 1;      // LDS row pitch of the staged operand (odd: the 32 rows of a read hit 32 banks)

__device__ inline float dn_act(float v, int act) {
  return act == DLWP_ACT_TANH ? tanhf(v) : (act == DLWP_ACT_RELU ? dlwp_nmax(v, 0.f) : v);
}
__device__ inline float dn_act_grad(float y, int act) {
  return act == DLWP_ACT_TANH ? 1.f - y * y : (act == DLWP_ACT_RELU ? (y > 0.f ? 1.f : 0.f) : 1.f);
}

// out[M, O] = epilogue(a'[M, R] B), a' = a o act'(ya) when ya is given.
//   TRANS = false: B[r][o] = w[r * O + o]   (forward: R = K, O = N)
//   TRANS = true : B[r][o] = w[o * R + r]   (data gradient: R = N, O = K)
// Workgroup b: column strip b / row_blocks, row block b % row_blocks (the row blocks of a strip run side by side and share its
// weights through the L2).  The operands of chunk c + 1 are fetched into registers while chunk c is multiplied.
template <int MT, bool TRANS>
__global__ __launch_bounds__(DN_MM_THREADS) void dense_mm_kernel(const float* __restrict__ a, const float* __restrict__ ya,
                                                                 int act_in, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, int act_out,
                                                                 float* __restrict__ out, int M, int R, int O, int row_blocks) {
  constexpr int ROWS = 32 * MT;
  constexpr int XS = ROWS * DN_PITCH;
  constexpr int XPT = ROWS * DN_RC / DN_MM_THREADS;     // staged elements per thread and chunk (8 MT)
  constexpr int WS = TRANS ? 32 * DN_PITCH : 0;         // data gradient: the strip's 32 rows of w, staged like the left operand
  __shared__ float smem[XS + WS > DN_WAVES * 1024 ? XS + WS : DN_WAVES * 1024];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j = lane & 31, hh = lane >> 5;
  const int m0 = ((int)blockIdx.x % row_blocks) * ROWS;
  const int o0 = ((int)blockIdx.x / row_blocks) * 32;
  const int oc = o0 + j;
  const bool o_ok = oc < O;
  const int rl0 = wave * DN_RW;          // this wave's 16 reduction elements of a chunk
  const int scol = t & (DN_RC - 1), srow = t / DN_RC;   // staging: thread t holds rows srow + 4 i of column scol
  f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

  float xr[XPT], b0[8], b1[8], b2[8];
  auto fetch_x = [&](int c) {
    const int r0 = c * DN_RC;
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int m = m0 + srow + (DN_MM_THREADS / DN_RC) * i, r = r0 + scol;
      float v = 0.f;
      if (m < M && r < R) {
        const size_t idx = (size_t)m * R + r;
        v = a[idx];
        if (ya) v *= dn_act_grad(ya[idx], act_in);
      }
      xr[i] = v;
    }
  };
  // forward: matrix instruction s multiplies reduction elements rl0 + 2 s and rl0 + 2 s + 1 (lane halves), each lane half one
  // coalesced 128-byte run of a row of w.  data gradient: the reduction runs ALONG the rows of w, so the strip's 32 rows are read
  // in coalesced 256-byte runs (thread t: element scol of rows srow + 4 i) and transposed through LDS
  auto fetch_w = [&](int c, float* bw) {
    const int r0 = c * DN_RC;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (!TRANS) {
        const int r = r0 + rl0 + 2 * s + hh;
        bw[s] = (o_ok && r < R) ? w[(size_t)r * O + oc] : 0.f;
      } else {
        const int o = o0 + srow + (DN_MM_THREADS / DN_RC) * s, r = r0 + scol;
        bw[s] = (o < O && r < R) ? w[(size_t)o * R + r] : 0.f;
      }
    }
  };

  const int nchunks = (R + DN_RC - 1) / DN_RC;
  // forward, chunk c: its staged operand goes to LDS, the staged operand of chunk c + 1 and the weights of chunk c + 2 are
  // requested, then the chunk is multiplied with the weights that arrived two steps ago (three register sets in rotation).
  // data gradient: both operands go through LDS, one chunk ahead.
  auto step = [&](int c, float* bc, float* bf) {
    __syncthreads();                     // the previous chunk has been read
#pragma unroll
    for (int i = 0; i < XPT; ++i) smem[(srow + (DN_MM_THREADS / DN_RC) * i) * DN_PITCH + scol] = xr[i];
    if (TRANS) {
#pragma unroll
      for (int s = 0; s < 8; ++s) smem[XS + (srow + (DN_MM_THREADS / DN_RC) * s) * DN_PITCH + scol] = bc[s];
    }
    __syncthreads();
    if (c + 1 < nchunks) fetch_x(c + 1);
    if (TRANS) {
      if (c + 1 < nchunks) fetch_w(c + 1, bc);
    } else {
      if (c + 2 < nchunks) fetch_w(c + 2, bf);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int col = rl0 + 2 * s + hh;
      const float bv = TRANS ? smem[XS + j * DN_PITCH + col] : bc[s];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(smem[(mt * 32 + j) * DN_PITCH + col], bv, acc[mt], 0, 0, 0);
    }
  };
  fetch_x(0);
  fetch_w(0, b0);
  if (TRANS) {
    for (int c = 0; c < nchunks; ++c) step(c, b0, b0);
  } else {
    if (nchunks > 1) fetch_w(1, b1);
    for (int c = 0; c < nchunks; c += 3) {
      step(c, b0, b2);
      if (c + 1 < nchunks) step(c + 1, b1, b0);
      if (c + 2 < nchunks) step(c + 2, b2, b1);
    }
  }

  // the eight waves' partial tiles, summed in wave order; bias and activation; coalesced stores
  const float bv = (bias && o_ok) ? bias[oc] : 0.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
      smem[wave * 1024 + row * 32 + j] = acc[mt][r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 1024 / DN_MM_THREADS; ++i) {
      const int e = t + i * DN_MM_THREADS;
      const int row = e >> 5;            // (e & 31 == j: this thread's column is the one it multiplied)
      const int m = m0 + mt * 32 + row;
      float v = smem[e];
#pragma unroll
      for (int wv = 1; wv < DN_WAVES; ++wv) v += smem[wv * 1024 + e];
      if (m < M && o_ok) out[(size_t)m * O + oc] = dn_act(v + bv, act_out);
    }
  }
}

// dw[K, N] = x^T g, g = dy o act'(y).  A workgroup owns rows [kb, kb + 128) x columns [n0, n0 + 128) of dw, wave w the 32 rows
// from kb + 32 w.  The batch is walked in chunks of 32 samples: x[:, kb ...] and g[:, n0 ...] of a chunk are read in coalesced
// 512-byte rows (the next chunk's while this one is multiplied), staged in LDS, and multiplied two samples per matrix
// instruction, in sample order.
constexpr int WG_MC = 32;
constexpr int WG_PITCH = 160;            // 128 + 32: the two lane halves (samples m, m + 1) read different banks
__global__ __launch_bounds__(DN_THREADS) void dense_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const float* __restrict__ y, int act, float* __restrict__ dw,
                                                                 int M, int K, int N) {
  __shared__ float xs[WG_MC * WG_PITCH], gs[WG_MC * WG_PITCH];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j = lane & 31, hh = lane >> 5;
  const int kb = blockIdx.y * 128, n0 = blockIdx.x * 128;
  const int k0 = kb + wave * 32;
  const int scol = t & 127, srow = t >> 7;              // staging: thread t holds column scol of samples srow + 2 i
  constexpr int PT = WG_MC * 128 / DN_THREADS;          // 16
  f32x16 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  float xr[PT], gr[PT];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int m = c * WG_MC + srow + 2 * i;
      xr[i] = (m < M && kb + scol < K) ? x[(size_t)m * K + kb + scol] : 0.f;
      float g = 0.f;
      if (m < M && n0 + scol < N) {
        const size_t idx = (size_t)m * N + n0 + scol;
        g = dy[idx];
        if (y) g *= dn_act_grad(y[idx], act);
      }
      gr[i] = g;
    }
  };
  const int nchunks = (M + WG_MC - 1) / WG_MC;
  if (nchunks > 0) fetch(0);
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      xs[(srow + 2 * i) * WG_PITCH + scol] = xr[i];
      gs[(srow + 2 * i) * WG_PITCH + scol] = gr[i];
    }
    __syncthreads();
    if (c + 1 < nchunks) fetch(c + 1);
#pragma unroll 4
    for (int p = 0; p < WG_MC / 2; ++p) {
      const float av = xs[(2 * p + hh) * WG_PITCH + wave * 32 + j];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, gs[(2 * p + hh) * WG_PITCH + 32 * q + j], acc[q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + 32 * q + j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (k < K && n < N) dw[(size_t)k * N + n] = acc[q][r];
    }
  }
}

// db[n] = sum_m g[m][n], in sample order
__global__ __launch_bounds__(DN_THREADS) void dense_bgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, int act,
                                                                 float* __restrict__ db, int M, int N) {
  const int n = blockIdx.x * DN_THREADS + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int m = 0; m < M; ++m) {
    const size_t i = (size_t)m * N + n;
    float g = dy[i];
    if (y) g *= dn_act_grad(y[i], act);
    s += g;
  }
  db[n] = s;
}

// ---- Dropout: Philox-4x32-10 (philox.h), counter (q lo, q hi, step, layer), key (seed lo, seed hi); word i of block q
//      decides element 4 q + i: kept when word >= threshold, and then multiplied by scale ------------
__global__ __launch_bounds__(DN_THREADS) void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long long n,
                                                             dlwp_dropout d, int vec) {
  const long long q = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
  const long long i0 = 4 * q;
  if (i0 >= n) return;
  unsigned r[4];
  philox4x32_10((unsigned)((unsigned long long)q & 0xffffffffull), (unsigned)((unsigned long long)q >> 32), d.step, d.layer,
                (unsigned)(d.seed & 0xffffffffull), (unsigned)(d.seed >> 32), r);
  if (vec && i0 + 4 <= n) {
    const f32x4 v = *(const f32x4*)(x + i0);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = r[i] >= d.threshold ? v[i] * d.scale : 0.f;
    *(f32x4*)(y + i0) = o;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i0 + i < n) y[i0 + i] = r[i] >= d.threshold ? x[i0 + i] * d.scale : 0.f;
  }
}

bool dn_aligned(std::initializer_list<const void*> ps, uintptr_t mask) {
  for (const void* p : ps)
    if ((uintptr_t)p & mask) return false;
  return true;
}

int dn_check(const dlwp_dense& d, const char* who) {
  DLWP_CHECK_ARG(d.m >= 0 && d.k > 0 && d.n > 0, "%s: bad shape (m %d, k %d, n %d)", who, d.m, d.k, d.n);
  DLWP_CHECK_ARG(d.act == DLWP_ACT_LINEAR || d.act == DLWP_ACT_TANH || d.act == DLWP_ACT_RELU, "%s: bad activation %d", who, d.act);
  return DLWP_OK;
}

template <bool TRANS>
void dn_launch_mm(const float* a, const float* ya, int act_in, const float* w, const float* bias, int act_out, float* out, int M,
                  int R, int O, hipStream_t s) {
  // 32 rows per workgroup (measured: 64 rows per workgroup took 3.3x the time of 32, not 2x); the row blocks of a column strip
  // are neighbours in the grid and share the strip's weights through the L2
  const int row_blocks = dlwp_ceil_div(M, 32);
  const dim3 grid((unsigned)((long long)dlwp_ceil_div(O, 32) * row_blocks));
  dense_mm_kernel<1, TRANS><<<grid, DN_MM_THREADS, 0, s>>>(a, ya, act_in, w, bias, act_out, out, M, R, O, row_blocks);
}

int dn_dropout(const char* who, dlwp_handle_t h, const void* x, void* y, long long n, const dlwp_dropout& d, void* stream) {
  DLWP_CHECK_ARG(h && (n == 0 || (x && y)), "%s: null handle or pointer", who);
  DLWP_CHECK_ARG(n >= 0 && n < (1ll << 40), "%s: bad element count %lld", who, n);
  DLWP_CHECK_ARG(dn_aligned({x, y}, 3), "%s: tensors must be float aligned", who);
  DLWP_CHECK_ARG(d.scale > 0.f, "%s: scale must be positive", who);
  if (n == 0) return DLWP_OK;
  const long long groups = (n + 3) / 4;
  dropout_kernel<<<dim3((unsigned)((groups + DN_THREADS - 1) / DN_THREADS)), DN_THREADS, 0, (hipStream_t)stream>>>(
      (const float*)x, (float*)y, n, d, dn_aligned({x, y}, 15) ? 1 : 0);
  DLWP_LAUNCH_CHECK(who);
  return DLWP_OK;
}

}  // namespace

extern "C" {

int dlwp_dense_fwd(dlwp_handle_t h, const void* x, const void* w, const void* b, void* y, dlwp_dense d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_dense_fwd, h, x, w, b, y, d);
  const int rc = dn_check(d, "dlwp_dense_fwd");
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && w && (d.m == 0 || (x && y)), "dlwp_dense_fwd: null handle or pointer");
  DLWP_CHECK_ARG(dn_aligned({x, w, b, y}, 3), "dlwp_dense_fwd: tensors must be float aligned");
  DLWP_CHECK_ARG(x != y, "dlwp_dense_fwd: y must not alias x");
  if (d.m == 0) return DLWP_OK;
  dn_launch_mm<false>((const float*)x, nullptr, 0, (const float*)w, (const float*)b, d.act, (float*)y, d.m, d.k, d.n,
                      (hipStream_t)stream);
  DLWP_LAUNCH_CHECK("dense_fwd kernel");
  return DLWP_OK;
}

int dlwp_dense_bwd_data(dlwp_handle_t h, const void* dy, const void* y, const void* w, void* dx, dlwp_dense d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_dense_bwd_data, h, dy, y, w, dx, d);
  const int rc = dn_check(d, "dlwp_dense_bwd_data");
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && w && (d.m == 0 || (dy && dx)), "dlwp_dense_bwd_data: null handle or pointer");
  DLWP_CHECK_ARG(d.act == DLWP_ACT_LINEAR || y, "dlwp_dense_bwd_data: the activation's derivative needs y");
  DLWP_CHECK_ARG(dn_aligned({dy, y, w, dx}, 3), "dlwp_dense_bwd_data: tensors must be float aligned");
  DLWP_CHECK_ARG(dx != dy && dx != y, "dlwp_dense_bwd_data: dx must not alias dy or y");
  if (d.m == 0) return DLWP_OK;
  dn_launch_mm<true>((const float*)dy, d.act == DLWP_ACT_LINEAR ? nullptr : (const float*)y, d.act, (const float*)w, nullptr,
                     DLWP_ACT_LINEAR, (float*)dx, d.m, d.n, d.k, (hipStream_t)stream);
  DLWP_LAUNCH_CHECK("dense_bwd_data kernel");
  return DLWP_OK;
}

int dlwp_dense_bwd_weight(dlwp_handle_t h, const void* x, const void* dy, const void* y, void* dw, void* db, dlwp_dense d,
                          void* stream) {
  DLWP_TAPE(h, stream, dlwp_dense_bwd_weight, h, x, dy, y, dw, db, d);
  const int rc = dn_check(d, "dlwp_dense_bwd_weight");
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(h && dw && (d.m == 0 || (x && dy)), "dlwp_dense_bwd_weight: null handle or pointer");
  DLWP_CHECK_ARG(d.act == DLWP_ACT_LINEAR || y, "dlwp_dense_bwd_weight: the activation's derivative needs y");
  DLWP_CHECK_ARG(dn_aligned({x, dy, y, dw, db}, 3), "dlwp_dense_bwd_weight: tensors must be float aligned");
  const float* yy = d.act == DLWP_ACT_LINEAR ? nullptr : (const float*)y;
  hipStream_t s = (hipStream_t)stream;
  dense_wgrad_kernel<<<dim3(dlwp_ceil_div(d.n, 128), dlwp_ceil_div(d.k, 128)), DN_THREADS, 0, s>>>(
      (const float*)x, (const float*)dy, yy, d.act, (float*)dw, d.m, d.k, d.n);
  if (db)
    dense_bgrad_kernel<<<dlwp_ceil_div(d.n, DN_THREADS), DN_THREADS, 0, s>>>((const float*)dy, yy, d.act, (float*)db, d.m, d.n);
  DLWP_LAUNCH_CHECK("dense_bwd_weight kernels");
  return DLWP_OK;
}

int dlwp_dropout_fwd(dlwp_handle_t h, const void* x, void* y, long long n, dlwp_dropout d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_dropout_fwd, h, x, y, n, d);
  return dn_dropout("dlwp_dropout_fwd", h, x, y, n, d, stream);
}

int dlwp_dropout_bwd(dlwp_handle_t h, const void* dy, void* dx, long long n, dlwp_dropout d, void* stream) {
  DLWP_TAPE(h, stream, dlwp_dropout_bwd, h, dy, dx, n, d);
  return dn_dropout("dlwp_dropout_bwd", h, dy, dx, n, d, stream);
}

}  // extern "C"
