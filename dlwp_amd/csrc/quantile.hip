// quantile.hip -- climatological quantiles where the record is (gfx950): per label (calendar month) and grid point the order
// statistics of a long float32 record, and what numpy.nanquantile makes of them for the methods 'linear', 'lower', 'higher' and
// 'nearest'.  The thresholds of dlwp_ens_event_counts ("upper tercile", "above the 95th percentile of this month") come from here.
//
// Selection is exact and integer: a value is ordered by the monotone key of its bits (sign bit set: ~u, else u | 0x80000000; a total
// order with -0.0 < +0.0), NaNs (v != v) become key 0xffffffff, and the key of the sample of rank r is found by bisection, most
// significant bit first: bit b of the prefix is set where (number of keys < prefix | 1 << b) <= r.  A column needs at most 2 K <= 16
// ranks, they differ per column (NaN counts do) and live in registers, and one sweep over the column's keys serves all of them.
// There is ONE selection loop (quantile_kernel) with two sources of keys:
//   LDS route        a workgroup owns (label, tile of cols = 64 / 32 / 16 adjacent columns), gathers the label's rows of the tile
//                    into LDS once as keys -- one pass over HBM -- and bisects there;
//   streaming route  for a list too long for LDS at the narrowest tile: the same sweeps read x through the index list, 33 times.
// Lanes and layout.  A wave owns CW = cols / 4 columns and T = 64 / CW shares of the rows: lane l has column l % CW and the rows
// l / CW, l / CW + T, ...  The LDS image is wave-private, row-major over the wave's OWN columns: key (row i, column cc) of wave w at
// dword (w * len_pad + i) * CW + cc.  One ds_read_b32 of a sweep therefore reads the 64 consecutive dwords it * 64 + lane: every
// bank once per 32-lane group, no conflict at any tile width, and the counts of a column's T lanes are added by lane shuffles
// inside the wave, so the selection needs no barrier and no LDS besides the keys.
// Counts are integers: the result does not depend on scheduling, there are no atomics and no float64 sums.  The interpolation of
// 'linear' is three float64 operations, each rounded once (contraction into an fma is switched off), and one rounding to float32.
#include "verify_common.h"      // mult4, aligned16

#include <cmath>

// No contraction anywhere in this file.  The compiler's default fuses a float64 product with the sum behind it into an fma (the
// __dmul_rn / __dadd_rn intrinsics are plain operators to it and fuse as well): h - floor(h) would see the unrounded product
// (n - 1) * q, and a + (b - a) * g would change its last float64 bit and with it, at times, the float32 result.  The host rounds
// every operation once, and so does this file; nothing else here would gain from an fma.
#pragma clang fp contract(off)

namespace {

constexpr int QUANT_THREADS = 256;                // four waves
constexpr int QUANT_MAX_LABELS = 64;
constexpr int QUANT_MAX_K = 8;
// LDS budget of one workgroup: half of the CU's 160 KiB, so that two workgroups (two waves per SIMD) share a CU
constexpr int QUANT_LDS_BYTES = 80 * 1024;
// streaming route: a wave reads 64-byte pieces of four rows per instruction.  The sweeps are bound by the bytes in flight, and the
// narrow piece buys twice the waves of a 128-byte one (four per SIMD on a 63 360-float row); eight loads are in flight per lane
constexpr int QUANT_STREAM_CW = 16;
constexpr int QUANT_STREAM_BATCH = 8;
constexpr unsigned QUANT_NAN_KEY = 0xffffffffu;   // no non-NaN value has this key (it would be -0.0 without its sign bit set)
constexpr unsigned QUANT_QNAN = 0x7fc00000u;

typedef unsigned qu32x4 __attribute__((ext_vector_type(4)));

struct QuantArgs {
  const unsigned* x;                              // float32 bits
  const int* index;                               // sample indices grouped by label
  unsigned* out;                                  // (k, n_labels, row) float32 bits
  int* counts;                                    // (n_labels, row) non-NaN samples
  long long row;
  int count, n_labels, k, method, tiles, len_pad, vec;
  double q[QUANT_MAX_K];
  int off[QUANT_MAX_LABELS + 1];
};

__device__ __forceinline__ unsigned quant_key(unsigned u) {
  const float v = __uint_as_float(u);
  const unsigned key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return v != v ? QUANT_NAN_KEY : key;
}

__device__ __forceinline__ unsigned quant_unkey(unsigned key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// float32(a + (b - a) * g), every operation rounded once in float64
__device__ __forceinline__ float quant_lerp(double a, double b, double g) {
  const double d = b - a;
  const double m = d * g;
  return (float)(a + m);
}

// the label's rows of the tile as keys into the wave-private images; rows len .. len_pad, columns beyond the row and indices outside
// the record hold the NaN key.  VEC: a unit is four adjacent columns (they stay in one wave's image: CW % 4 == 0), else one.
template <int CW, bool VEC>
__device__ __forceinline__ void quant_fill(const QuantArgs& p, unsigned* lds, int lo, int len, long long col0) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int UNITS = 4 * CW / W;               // per row of the tile
  const int items = p.len_pad * UNITS;
  for (int base = threadIdx.x; base < items; base += 4 * QUANT_THREADS) {
    qu32x4 v[4];
    int at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int item = base + u * QUANT_THREADS;
      at[u] = -1;
      v[u] = (qu32x4)QUANT_NAN_KEY;
      if (item < items) {
        const int i = item / UNITS, cl = (item - i * UNITS) * W;
        at[u] = ((cl / CW) * p.len_pad + i) * CW + cl % CW;
        const long long c = col0 + cl;
        if (i < len && c < p.row) {
          const int r = p.index[lo + i];
          if ((unsigned)r < (unsigned)p.count) {
            const unsigned* src = p.x + (long long)r * p.row + c;
            if (VEC)
              v[u] = *reinterpret_cast<const qu32x4*>(src);
            else
              v[u][0] = src[0];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (at[u] < 0) continue;
      if (VEC) {
        qu32x4 key;
#pragma unroll
        for (int e = 0; e < 4; ++e) key[e] = quant_key(v[u][e]);
        *reinterpret_cast<qu32x4*>(lds + at[u]) = key;
      } else {
        lds[at[u]] = quant_key(v[u][0]);
      }
    }
  }
}

// cnt[k] <- the number of the column's keys below thr[k], for R thresholds in one sweep; valid in every lane of the column
template <int CW, int R, bool LDS>
__device__ __forceinline__ void quant_sweep(const QuantArgs& p, const unsigned* keys, int lo, int len, long long c,
                                            const unsigned (&thr)[R], unsigned (&cnt)[R]) {
  constexpr int T = 64 / CW;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < R; ++k) cnt[k] = 0;
  if (LDS) {
    const int turns = p.len_pad / T;              // len_pad * CW / 64
    const unsigned* src = keys + lane;
#pragma unroll 4
    for (int it = 0; it < turns; ++it) {
      const unsigned key = src[it * 64];
#pragma unroll
      for (int k = 0; k < R; ++k) cnt[k] += key < thr[k] ? 1u : 0u;
    }
  } else {
    const bool live = c < p.row;
    const unsigned* px = p.x + (live ? c : 0);
    const int* list = p.index + lo;
    int i = lane / CW;
    constexpr int B = QUANT_STREAM_BATCH;
    for (; i + (B - 1) * T < len; i += B * T) {
      unsigned key[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int r = list[i + u * T];
        const bool in = live && (unsigned)r < (unsigned)p.count;
        const unsigned v = px[(long long)(in ? r : 0) * p.row];
        key[u] = in ? quant_key(v) : QUANT_NAN_KEY;
      }
#pragma unroll
      for (int u = 0; u < B; ++u)
#pragma unroll
        for (int k = 0; k < R; ++k) cnt[k] += key[u] < thr[k] ? 1u : 0u;
    }
    for (; i < len; i += T) {
      const int r = list[i];
      const bool in = live && (unsigned)r < (unsigned)p.count;
      const unsigned v = px[(long long)(in ? r : 0) * p.row];
      const unsigned key = in ? quant_key(v) : QUANT_NAN_KEY;
#pragma unroll
      for (int k = 0; k < R; ++k) cnt[k] += key < thr[k] ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = CW; off < 64; off <<= 1)
#pragma unroll
    for (int k = 0; k < R; ++k) cnt[k] += __shfl_xor(cnt[k], off, 64);
}

// One workgroup per (label, tile of 4 CW columns).  R: the ranks carried (1, 2, 4, 8, 16 >= k, or 2 k for 'linear'); ranks beyond
// the ones needed repeat rank 0.
template <int CW, int R, bool LDS>
__global__ __launch_bounds__(QUANT_THREADS) void quantile_kernel(QuantArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned quant_lds[];
  const unsigned label = blockIdx.x / (unsigned)p.tiles;
  const unsigned tile = blockIdx.x - label * (unsigned)p.tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = p.off[label], len = p.off[label + 1] - lo;
  const long long col0 = (long long)tile * (4 * CW);
  const long long c = col0 + wave * CW + lane % CW;
  if (LDS) {
    if (p.vec)
      quant_fill<CW, true>(p, quant_lds, lo, len, col0);
    else
      quant_fill<CW, false>(p, quant_lds, lo, len, col0);
    __syncthreads();
  }
  const unsigned* keys = quant_lds + wave * p.len_pad * CW;

  // n: the keys below the NaN key
  unsigned n;
  {
    const unsigned thr[1] = {QUANT_NAN_KEY};
    unsigned cnt[1];
    quant_sweep<CW, 1, LDS>(p, keys, lo, len, c, thr, cnt);
    n = cnt[0];
  }
  // the probabilities an instance can carry: one rank each, or two for 'linear' (the host picks R >= the ranks needed)
  constexpr int KN = R < QUANT_MAX_K ? R : QUANT_MAX_K, KL = R / 2;
  const bool linear = p.method == DLWP_QUANTILE_LINEAR;
  unsigned rank[R];
  double frac[KL > 0 ? KL : 1];
#pragma unroll
  for (int k = 0; k < R; ++k) rank[k] = 0;
  if (linear) {
#pragma unroll
    for (int k = 0; k < KL; ++k) {
      frac[k] = 0.0;
      if (k < p.k && n > 0) {
        const double h = (double)(n - 1) * p.q[k];
        const double fl = floor(h);
        const unsigned a = (unsigned)fl;
        frac[k] = h - fl;                         // exact
        rank[2 * k] = a;
        rank[2 * k + 1] = a + 1 < n ? a + 1 : n - 1;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < KN; ++k) {
      if (k < p.k && n > 0) {
        const double h = (double)(n - 1) * p.q[k];
        rank[k] = (unsigned)(p.method == DLWP_QUANTILE_LOWER ? floor(h) : (p.method == DLWP_QUANTILE_HIGHER ? ceil(h) : rint(h)));
      }
    }
  }

  unsigned prefix[R];
#pragma unroll
  for (int k = 0; k < R; ++k) prefix[k] = 0;
  for (int bit = 31; bit >= 0; --bit) {
    unsigned thr[R], cnt[R];
#pragma unroll
    for (int k = 0; k < R; ++k) thr[k] = prefix[k] | (1u << bit);
    quant_sweep<CW, R, LDS>(p, keys, lo, len, c, thr, cnt);
#pragma unroll
    for (int k = 0; k < R; ++k) prefix[k] = cnt[k] <= rank[k] ? thr[k] : prefix[k];
  }

  if (lane >= CW || c >= p.row) return;           // one lane per column stores
  const long long plane = (long long)p.n_labels * p.row;
  const long long o = (long long)label * p.row + c;
  p.counts[o] = (int)n;
  if (linear) {
#pragma unroll
    for (int k = 0; k < KL; ++k) {
      if (k >= p.k) continue;
      unsigned res = QUANT_QNAN;
      if (n > 0) {
        const unsigned ua = quant_unkey(prefix[2 * k]), ub = quant_unkey(prefix[2 * k + 1]);
        res = ua;
        if (frac[k] != 0.0) {
          const double a = (double)__uint_as_float(ua), b = (double)__uint_as_float(ub);
          const float v = quant_lerp(a, b, frac[k]);
          res = v != v ? QUANT_QNAN : __float_as_uint(v);
        }
      }
      p.out[(long long)k * plane + o] = res;
    }
  } else {
#pragma unroll
    for (int k = 0; k < KN; ++k)
      if (k < p.k) p.out[(long long)k * plane + o] = n > 0 ? quant_unkey(prefix[k]) : QUANT_QNAN;
  }
}

inline int quant_round_up(int v, int m) { return (v + m - 1) / m * m; }

// the widest tile whose image of max_len rows fits the budget: 64, 32, 16 columns, or 0
inline int quant_lds_cols(int max_len) {
  for (int cols = 64; cols >= 16; cols >>= 1) {
    const int t = QUANT_THREADS / cols;           // shares of a column = 64 / CW
    if ((long long)quant_round_up(max_len, t) * cols * 4 <= QUANT_LDS_BYTES) return cols;
  }
  return 0;
}

typedef void (*quant_kernel_t)(QuantArgs);

template <int CW, bool LDS>
quant_kernel_t quant_pick_r(int ranks, int* slot) {
  if (ranks <= 1) return *slot += 0, quantile_kernel<CW, 1, LDS>;
  if (ranks <= 2) return *slot += 1, quantile_kernel<CW, 2, LDS>;
  if (ranks <= 4) return *slot += 2, quantile_kernel<CW, 4, LDS>;
  if (ranks <= 8) return *slot += 3, quantile_kernel<CW, 8, LDS>;
  return *slot += 4, quantile_kernel<CW, 16, LDS>;
}

inline size_t quant_ws_bytes(long long row, int n_labels) { return ((size_t)n_labels * (size_t)row * sizeof(int) + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int dlwp_verify_label_quantiles_plan(dlwp_handle_t, int max_len, long long row, int route, int* route_out, int* cols_out) {
  DLWP_CHECK_ARG(max_len >= 1 && row >= 1, "dlwp_verify_label_quantiles_plan: max_len %d and row %lld must be >= 1", max_len, row);
  DLWP_CHECK_ARG(route >= 0 && route <= 2, "dlwp_verify_label_quantiles_plan: route %d, expected 0 (planner), 1 (LDS) or 2 (streaming)",
                 route);
  DLWP_CHECK_ARG(route_out && cols_out, "dlwp_verify_label_quantiles_plan: null pointer");
  const int cols = quant_lds_cols(max_len);
  DLWP_CHECK_ARG(route != 1 || cols > 0,
                 "dlwp_verify_label_quantiles_plan: the LDS route holds at most %d rows of a label (16 columns in %d bytes), got %d",
                 QUANT_LDS_BYTES / (16 * 4), QUANT_LDS_BYTES, max_len);
  const bool lds = route == 1 || (route == 0 && cols > 0);
  *route_out = lds ? 1 : 2;
  *cols_out = lds ? cols : 4 * QUANT_STREAM_CW;
  return DLWP_OK;
}

size_t dlwp_verify_label_quantiles_workspace(dlwp_handle_t, int count, long long row, int n_labels, int k) {
  if (count < 1 || row < 1 || n_labels < 1 || n_labels > QUANT_MAX_LABELS || k < 1 || k > QUANT_MAX_K) return 0;
  return quant_ws_bytes(row, n_labels);
}

int dlwp_verify_label_quantiles(dlwp_handle_t h, const void* x, int count, long long row, const int* offsets, const void* index,
                                int n_labels, const double* q, int k, int method, int route, void* out, void* counts /* may be NULL */,
                                void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_label_quantiles);
  DLWP_CHECK_ARG(count >= 1 && row >= 1, "dlwp_verify_label_quantiles: count %d and row %lld must be >= 1", count, row);
  DLWP_CHECK_ARG(n_labels >= 1 && n_labels <= QUANT_MAX_LABELS, "dlwp_verify_label_quantiles: n_labels %d, expected 1 .. %d", n_labels,
                 QUANT_MAX_LABELS);
  DLWP_CHECK_ARG(k >= 1 && k <= QUANT_MAX_K, "dlwp_verify_label_quantiles: k %d, expected 1 .. %d probabilities", k, QUANT_MAX_K);
  DLWP_CHECK_ARG(q != nullptr, "dlwp_verify_label_quantiles: null pointer (q)");
  for (int i = 0; i < k; ++i)
    DLWP_CHECK_ARG(std::isfinite(q[i]) && q[i] >= 0.0 && q[i] <= 1.0, "dlwp_verify_label_quantiles: q[%d] = %g is not in [0, 1]", i, q[i]);
  DLWP_CHECK_ARG(method >= DLWP_QUANTILE_LINEAR && method <= DLWP_QUANTILE_NEAREST, "dlwp_verify_label_quantiles: unknown method %d",
                 method);
  DLWP_CHECK_ARG(route >= 0 && route <= 2, "dlwp_verify_label_quantiles: route %d, expected 0 (planner), 1 (LDS) or 2 (streaming)", route);
  DLWP_CHECK_ARG(x && offsets && index && out && ws, "dlwp_verify_label_quantiles: null pointer");
  DLWP_CHECK_ARG(offsets[0] == 0 && offsets[n_labels] == count,
                 "dlwp_verify_label_quantiles: offsets must run from 0 to count %d, got %d .. %d", count, offsets[0], offsets[n_labels]);
  int max_len = 0;
  for (int l = 0; l < n_labels; ++l) {
    DLWP_CHECK_ARG(offsets[l] <= offsets[l + 1], "dlwp_verify_label_quantiles: offsets decrease at label %d", l);
    if (offsets[l + 1] - offsets[l] > max_len) max_len = offsets[l + 1] - offsets[l];
  }
  const int lds_cols = quant_lds_cols(max_len);
  const bool lds = route == 1 || (route == 0 && lds_cols > 0);
  const int cols = lds ? lds_cols : 4 * QUANT_STREAM_CW;
  // (the narrowest tile has the most workgroups: the bound holds for every route)
  DLWP_CHECK_ARG((long long)n_labels * ((row + 15) / 16) < (1ll << 31), "dlwp_verify_label_quantiles: row %lld too long", row);
  DLWP_CHECK_ARG(!lds || lds_cols > 0,
                 "dlwp_verify_label_quantiles: the LDS route holds at most %d rows of a label (16 columns in %d bytes), got %d",
                 QUANT_LDS_BYTES / (16 * 4), QUANT_LDS_BYTES, max_len);
  const size_t ws_need = quant_ws_bytes(row, n_labels);
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_verify_label_quantiles: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(aligned16(ws), "dlwp_verify_label_quantiles: workspace must be 16-byte aligned");
  DLWP_CHECK_ARG(h, "dlwp_verify_label_quantiles: null handle");
  QuantArgs p;
  p.x = (const unsigned*)x;
  p.index = (const int*)index;
  p.out = (unsigned*)out;
  p.counts = counts ? (int*)counts : (int*)ws;    // the kernel always stores the counts: one store path
  p.row = row;
  p.count = count, p.n_labels = n_labels, p.k = k, p.method = method;
  p.tiles = (int)((row + cols - 1) / cols);
  p.len_pad = lds ? quant_round_up(max_len, QUANT_THREADS / cols) : 0;
  p.vec = mult4(row) && aligned16(x);
  for (int i = 0; i < QUANT_MAX_K; ++i) p.q[i] = i < k ? q[i] : 0.0;
  for (int l = 0; l <= QUANT_MAX_LABELS; ++l) p.off[l] = offsets[l < n_labels ? l : n_labels];
  const int ranks = method == DLWP_QUANTILE_LINEAR ? 2 * k : k;
  int slot = 0;
  quant_kernel_t kern;
  if (!lds)
    kern = quant_pick_r<QUANT_STREAM_CW, false>(ranks, &slot);
  else if (cols == 64)
    slot = 5, kern = quant_pick_r<16, true>(ranks, &slot);
  else if (cols == 32)
    slot = 10, kern = quant_pick_r<8, true>(ranks, &slot);
  else
    slot = 15, kern = quant_pick_r<4, true>(ranks, &slot);
  const size_t lds_bytes = (size_t)p.len_pad * cols * 4;
  if (lds) {
    // images beyond 64 KiB are allowed once per instance and device.  Setting the attribute twice is harmless, so no lock
    static unsigned lds_allowed[20];
    const unsigned dev_bit = 1u << (h->device & 31);
    if (!(lds_allowed[slot] & dev_bit)) {
      const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, QUANT_LDS_BYTES);
      if (e != hipSuccess) DLWP_FAIL(DLWP_EHIP, "dlwp_verify_label_quantiles: hipFuncSetAttribute failed (%d)", (int)e);
      lds_allowed[slot] |= dev_bit;
    }
  }
  const unsigned grid = (unsigned)((long long)n_labels * p.tiles);
  kern<<<grid, QUANT_THREADS, lds_bytes, (hipStream_t)stream>>>(p);
  DLWP_LAUNCH_CHECK("verify_label_quantiles kernel");
  return DLWP_OK;
}

}  // extern "C"
