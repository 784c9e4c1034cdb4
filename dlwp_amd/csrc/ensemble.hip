// ensemble.hip -- ensemble verification where the series is (gfx950): reductions ACROSS the member axis of a rollout that stays in
// HBM.  dlwp_ens_mean_spread writes the ensemble mean and spread fields; dlwp_ens_score_sums reduces, per (lead, group) cell, the
// error of the mean, the variance, the two CRPS terms and the rank histogram against a per-lead verification.
//
// Reference: examples/plot_ensemble.py:242,269 averages the members on the host (np.mean over the member axis); the scores follow
// the definitions of DESIGN.md 5.35 (include/dlwp_hip.h has the strides).  A column is one (lead, sample, point) with M float32
// member values `member_stride` elements apart; lanes map to consecutive points, so every global load is a coalesced run.  All
// per-column arithmetic is float64 on the float32 values, comparisons are made on the float32 values themselves.
//
// The ascending order that B = sum_k (2k - M + 1) x_(k) needs: a lane keeps 32 members of its column in registers as
// order-preserving integer keys (v_min_i32 / v_max_i32 need no NaN canonicalisation) and sorts them with a fully unrolled bitonic
// network.  M <= 32 ends there (instances of 2, 4, 8, 16, 32 keys, padded with INT_MAX).  Above, the sorted runs of 32 go to LDS as
// [member][point] -- a lane only ever touches its own column, whatever row it reads, so there are no bank conflicts, no barriers and
// no cross-lane traffic -- and up to 8 run heads held in registers are merged: M steps of "smallest head, one LDS read".  The first
// key of every run stays in its head register, which keeps M = 256 at 8 x 31 x 256 B + the histogram below 64 KB of static LDS.
//
// Conventions of verify.hip: 64-bit offsets, entry points that never synchronise and read no size from the device, two-stage sums
// on the fixed tree of verify_common.h (a block is one wave here, so the block stage is the lane tree alone), no global atomics and
// no "last block" scheme.  The histogram uses integer LDS atomics inside a block (integer adds commute) and the same second kernel:
// repeated launches give identical bits.
#include "verify_common.h"

#include <climits>

namespace {

constexpr int ENS_THREADS = 256;           // mean / spread and the final kernel
constexpr int ENS_RUN = 32;                // members a lane sorts in registers
constexpr int ENS_MAX_MEMBERS = 256;       // 8 runs
constexpr int ENS_LDS_PER_CU = 160 * 1024;

// ---- mean and spread fields --------------------------------------------------------------------------------------------------------- //
struct MomentArgs {
  const float* x;
  float* mean;                             // either may be null
  float* spread;
  long long ls, ss, ms, row;
  int samples, members, ddof, tiles;       // tiles: blocks per (lead, sample) row
};

// One pass over the members: the sum in member order and the shifted sums of d_i = x_i - x_0 (exact in float64).  A NaN member
// makes every sum NaN, and `v < 0 ? 0 : v` keeps a NaN where fmax would drop it.
template <bool VEC>
__global__ __launch_bounds__(ENS_THREADS) void ens_mean_spread_kernel(MomentArgs p) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned r = blockIdx.x / (unsigned)p.tiles, tile = blockIdx.x - r * (unsigned)p.tiles;
  const unsigned t = r / (unsigned)p.samples, s = r - t * (unsigned)p.samples;
  const long long c = ((long long)tile * ENS_THREADS + threadIdx.x) * W;
  if (c >= p.row) return;
  const float* px = p.x + (long long)t * p.ls + (long long)s * p.ss + c;
  double x0[W], sum[W], sd[W], sdd[W];
  if (VEC) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(px);
#pragma unroll
    for (int k = 0; k < W; ++k) x0[k] = (double)v[k];
  } else {
    x0[0] = (double)px[0];
  }
#pragma unroll
  for (int k = 0; k < W; ++k) sum[k] = x0[k], sd[k] = 0.0, sdd[k] = 0.0;
#pragma unroll 8
  for (int i = 1; i < p.members; ++i) {
    float v[W];
    if (VEC) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(px + (long long)i * p.ms);
#pragma unroll
      for (int k = 0; k < W; ++k) v[k] = q[k];
    } else {
      v[0] = px[(long long)i * p.ms];
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double xd = (double)v[k], d = xd - x0[k];
      sum[k] += xd;
      sd[k] += d;
      sdd[k] = fma(d, d, sdd[k]);
    }
  }
  const double m = (double)p.members;
  float om[W], os[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    double var = (sdd[k] - sd[k] * sd[k] / m) / (double)(p.members - p.ddof);
    var = var < 0.0 ? 0.0 : var;
    om[k] = (float)(sum[k] / m);
    os[k] = (float)sqrt(var);
  }
  const long long o = (long long)r * p.row + c;
  if (VEC) {
    if (p.mean) *reinterpret_cast<f32x4*>(p.mean + o) = f32x4{om[0], om[1], om[2], om[3]};
    if (p.spread) *reinterpret_cast<f32x4*>(p.spread + o) = f32x4{os[0], os[1], os[2], os[3]};
  } else {
    if (p.mean) p.mean[o] = om[0];
    if (p.spread) p.spread[o] = os[0];
  }
}

// ---- scores ------------------------------------------------------------------------------------------------------------------------- //
struct ScoreArgs {
  const float* x;
  const float* y;
  float* crps;                             // may be null
  long long ls, ss, ms, run;
  int samples, members, groups, bpc;       // bpc: blocks per (lead, group) cell
  unsigned tiles_per_row;                  // 64-point tiles of one group in one sample row
  double inv_m;                            // 1 / members
};

// float32 bits as a signed integer with the same order (-0 below +0; NaNs at the ends, and a column with one is skipped anyway)
__device__ __forceinline__ int key_of(float v) {
  const int b = __float_as_int(v);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float value_of(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// data-independent network with compile-time indices: `v` stays in registers
template <int N>
__device__ __forceinline__ void bitonic_sort(int (&v)[N]) {
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const int a = v[i], b = v[l];
          const int lo = min(a, b), hi = max(a, b);
          const bool up = (i & k) == 0;
          v[i] = up ? lo : hi;
          v[l] = up ? hi : lo;
        }
      }
    }
  }
}

constexpr int ens_run_rows(int K) { return K > 1 ? K * (ENS_RUN - 1) : 1; }

// bytes of static LDS of an instance with K runs: the runs without their heads (K > 1) and the histogram
inline int ens_lds_bytes(int K) { return (K > 1 ? ens_run_rows(K) * 64 * 4 : 0) + (ENS_MAX_MEMBERS + 1) * 4; }

// stage 1.  A block is ONE wave.  Block blk of cell (lead f, group g) takes the 64-point tiles blk, blk + bpc, ... of the cell's
// samples x tiles_per_row grid; lane l owns point 64 * tile + l of the group.  Lanes past the end of the run read point 0 of the row
// (in bounds) and neither count nor store.  MP: keys of the register network; K: runs of 32 (MP == 32 where K > 1).
template <int MP, int K>
__global__ __launch_bounds__(64) void ens_score_kernel(ScoreArgs p, double* __restrict__ psums,
                                                       unsigned long long* __restrict__ phist) {
  __shared__ int runs[ens_run_rows(K) * 64];
  __shared__ unsigned hist[ENS_MAX_MEMBERS + 1];
  const int lane = threadIdx.x;
  const int M = p.members;
  const unsigned cell = blockIdx.x / (unsigned)p.bpc, blk = blockIdx.x - cell * (unsigned)p.bpc;
  const unsigned f = cell / (unsigned)p.groups, g = cell - f * (unsigned)p.groups;
  for (int b = lane; b <= M; b += 64) hist[b] = 0u;
  __syncthreads();
  const unsigned tiles = (unsigned)p.samples * p.tiles_per_row;          // < 2^31: checked by the host
  const double inv_m = p.inv_m, inv_m2 = p.inv_m * p.inv_m;
  double s_e2 = 0.0, s_e1 = 0.0, s_var = 0.0, s_a = 0.0, s_b = 0.0, s_n = 0.0;
  for (unsigned tile = blk; tile < tiles; tile += (unsigned)p.bpc) {
    const unsigned s = tile / p.tiles_per_row, tp = tile - s * p.tiles_per_row;
    const long long col = (long long)tp * 64 + lane;
    const bool active = col < p.run;
    const long long pc = active ? col : 0;
    const float* px = p.x + (long long)f * p.ls + (long long)s * p.ss + (long long)g * p.run + pc;
    const long long yo = (((long long)f * p.samples + s) * p.groups + g) * p.run + pc;
    const float yv = p.y[yo];
    const double yd = (double)yv;
    const double x0 = (double)px[0];
    double sum = 0.0, sd = 0.0, sdd = 0.0, sa = 0.0, B = 0.0;
    int rank = 0;
    bool bad = yv != yv;
    int head[K], pos[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      float v[MP];
#pragma unroll
      for (int j = 0; j < MP; ++j) {          // every load of the run is issued before the first use
        const int i = r * ENS_RUN + j;
        v[j] = px[(long long)(i < M ? i : M - 1) * p.ms];
      }
      int key[MP];
#pragma unroll
      for (int j = 0; j < MP; ++j) {          // member order
        const int i = r * ENS_RUN + j;
        key[j] = INT_MAX;
        if (i < M) {                          // uniform
          const double xd = (double)v[j], d = xd - x0;
          sum += xd;
          sd += d;
          sdd = fma(d, d, sdd);
          sa += fabs(xd - yd);
          rank += v[j] < yv ? 1 : 0;
          bad = bad || v[j] != v[j];
          key[j] = key_of(v[j]);
        }
      }
      bitonic_sort<MP>(key);
      if (K == 1) {
#pragma unroll
        for (int k = 0; k < MP; ++k)          // ascending order; the pads sit behind the M real keys
          if (k < M) B = fma((double)(2 * k - M + 1), (double)value_of(key[k]), B);      // int x float32: exact in float64
      } else {
        head[r] = key[0];
        pos[r] = 1;
#pragma unroll
        for (int j = 1; j < MP; ++j) runs[(r * (ENS_RUN - 1) + j - 1) * 64 + lane] = key[j];
      }
    }
    if (K > 1) {
      // M steps: the smallest head is x_(k); its run's next key comes from LDS, INT_MAX once the run is used up.  The M real keys are
      // below every pad, so exactly they are taken; the row index is clamped, so no key can move a read out of the lane's column.
      for (int k = 0; k < M; ++k) {
        int mn = head[0], rm = 0;
#pragma unroll
        for (int r = 1; r < K; ++r) {
          const bool lt = head[r] < mn;
          mn = lt ? head[r] : mn;
          rm = lt ? r : rm;
        }
        B = fma((double)(2 * k - M + 1), (double)value_of(mn), B);
        int pm = pos[0];
#pragma unroll
        for (int r = 1; r < K; ++r) pm = rm == r ? pos[r] : pm;
        const int at = (pm < ENS_RUN ? pm : ENS_RUN - 1) - 1;                     // 0 .. 30
        const int nk = runs[(rm * (ENS_RUN - 1) + at) * 64 + lane];
        const int nv = pm < ENS_RUN ? nk : INT_MAX;
#pragma unroll
        for (int r = 0; r < K; ++r) {
          const bool hit = rm == r;
          head[r] = hit ? nv : head[r];
          pos[r] = hit ? (pm < ENS_RUN ? pm + 1 : pm) : pos[r];
        }
      }
    }
    // 1 / M is one more float64 rounding than a division (exact where M is a power of two): far inside the float64 allowance
    const double e = sum * inv_m - yd;
    const double var0 = (sdd - sd * sd * inv_m) * inv_m;
    const double A = sa * inv_m;
    const bool ok = active && !bad;
    if (ok) {
      s_e2 = fma(e, e, s_e2);
      s_e1 += fabs(e);
      s_var += var0;
      s_a += A;
      s_b += B;
      s_n += 1.0;
      atomicAdd(&hist[rank], 1u);
    }
    if (p.crps && active) p.crps[yo] = ok ? (float)(A - B * inv_m2) : __builtin_nanf("");
  }
  s_e2 = wave_sum_f64(s_e2);
  s_e1 = wave_sum_f64(s_e1);
  s_var = wave_sum_f64(s_var);
  s_a = wave_sum_f64(s_a);
  s_b = wave_sum_f64(s_b);
  s_n = wave_sum_f64(s_n);
  if (lane == 0) {
    double* o = psums + 6ll * blockIdx.x;
    o[0] = s_e2, o[1] = s_e1, o[2] = s_var, o[3] = s_a, o[4] = s_b, o[5] = s_n;
  }
  __syncthreads();
  unsigned long long* oh = phist + (long long)blockIdx.x * (M + 1);
  for (int b = lane; b <= M; b += 64) oh[b] = hist[b];
}

// stage 2: one block per cell.  Wave 0 is the cell stage of verify_common.h; every thread adds the partial histograms of its bins
// in index order.
__global__ __launch_bounds__(ENS_THREADS) void ens_score_final_kernel(const double* __restrict__ psums,
                                                                      const unsigned long long* __restrict__ phist, int bpc,
                                                                      int members, double* __restrict__ sums,
                                                                      long long* __restrict__ hist) {
  const long long cell = blockIdx.x;
  const int bins = members + 1;
  for (int b = threadIdx.x; b < bins; b += ENS_THREADS) {
    const unsigned long long* src = phist + cell * bpc * bins + b;
    unsigned long long acc = 0;
    for (int i = 0; i < bpc; ++i) acc += src[(long long)i * bins];
    hist[cell * bins + b] = (long long)acc;
  }
  if (threadIdx.x < 64) cell_final<6>(psums, bpc, cell, true, threadIdx.x, sums);
}

inline int ens_runs(int members) { return (members + ENS_RUN - 1) / ENS_RUN; }

// one-wave blocks a CU holds: four times the waves per SIMD that the instance's registers allow (the compiler's resource report:
// 66, 99, 163 registers at 8, 16, 32 keys), fewer where the runs in LDS are the limit (2 at 8 runs)
inline int ens_blocks_per_cu(int members) {
  if (members <= 8) return 28;
  if (members <= 16) return 16;
  if (members <= ENS_RUN) return 12;
  const int by_lds = ENS_LDS_PER_CU / ens_lds_bytes(ens_runs(members));
  return by_lds < 12 ? by_lds : 12;
}

inline size_t ens_partial_bytes(int members) { return 6 * sizeof(double) + (size_t)(members + 1) * sizeof(unsigned long long); }

template <int MP, int K>
void ens_score_launch(const ScoreArgs& p, unsigned grid, double* psums, unsigned long long* phist, hipStream_t s) {
  ens_score_kernel<MP, K><<<grid, 64, 0, s>>>(p, psums, phist);
}

}  // namespace

extern "C" {

int dlwp_ens_mean_spread(dlwp_handle_t h, const void* x, int leads, int samples, int members, long long lead_stride,
                         long long sample_stride, long long member_stride, long long row, int ddof, void* mean, void* spread,
                         void* stream) {
  DLWP_UNTAPED(dlwp_ens_mean_spread);
  DLWP_CHECK_ARG(leads >= 1 && samples >= 1 && row >= 1, "dlwp_ens_mean_spread: leads %d, samples %d, row %lld must all be >= 1", leads,
                 samples, row);
  DLWP_CHECK_ARG(members >= 2, "dlwp_ens_mean_spread: members %d, expected >= 2", members);
  DLWP_CHECK_ARG(ddof == 0 || ddof == 1, "dlwp_ens_mean_spread: ddof %d, expected 0 or 1", ddof);
  DLWP_CHECK_ARG(lead_stride >= 0 && sample_stride >= 0 && member_stride >= 0, "dlwp_ens_mean_spread: negative stride");
  DLWP_CHECK_ARG(x && (mean || spread), "dlwp_ens_mean_spread: null pointer");
  const bool vec = mult4(row) && mult4(lead_stride) && mult4(sample_stride) && mult4(member_stride) && aligned16(x) &&
                   aligned16(mean) && aligned16(spread);
  const long long units = vec ? row / 4 : row;
  const long long tiles = (units + ENS_THREADS - 1) / ENS_THREADS;
  const long long rows = (long long)leads * samples;
  DLWP_CHECK_ARG(tiles < (1ll << 31) && rows * tiles < (1ll << 31), "dlwp_ens_mean_spread: %lld rows of %lld floats are too many for one grid",
                 rows, row);
  DLWP_CHECK_ARG(h, "dlwp_ens_mean_spread: null handle");
  MomentArgs p;
  p.x = (const float*)x, p.mean = (float*)mean, p.spread = (float*)spread;
  p.ls = lead_stride, p.ss = sample_stride, p.ms = member_stride, p.row = row;
  p.samples = samples, p.members = members, p.ddof = ddof, p.tiles = (int)tiles;
  const unsigned grid = (unsigned)(rows * tiles);
  if (vec)
    ens_mean_spread_kernel<true><<<grid, ENS_THREADS, 0, (hipStream_t)stream>>>(p);
  else
    ens_mean_spread_kernel<false><<<grid, ENS_THREADS, 0, (hipStream_t)stream>>>(p);
  DLWP_LAUNCH_CHECK("ens_mean_spread kernel");
  return DLWP_OK;
}

size_t dlwp_ens_score_workspace(dlwp_handle_t h, int leads, int groups, int members) {
  if (leads < 1 || groups < 1 || members < 2 || members > ENS_MAX_MEMBERS) return 0;
  const long long cells = (long long)leads * groups;
  return (size_t)cells * (size_t)cell_bpc_cap(h, cells, ens_blocks_per_cu(members)) * ens_partial_bytes(members);
}

int dlwp_ens_score_sums(dlwp_handle_t h, const void* x, long long lead_stride, long long sample_stride, long long member_stride,
                        const void* y, int leads, int samples, int members, int groups, long long run, void* sums, void* hist,
                        void* crps_out, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_ens_score_sums);
  DLWP_CHECK_ARG(leads >= 1 && samples >= 1 && groups >= 1 && run >= 1,
                 "dlwp_ens_score_sums: leads %d, samples %d, groups %d, run %lld must all be >= 1", leads, samples, groups, run);
  DLWP_CHECK_ARG(members >= 2 && members <= ENS_MAX_MEMBERS, "dlwp_ens_score_sums: members %d, expected 2 .. %d", members,
                 ENS_MAX_MEMBERS);
  DLWP_CHECK_ARG(lead_stride >= 0 && sample_stride >= 0 && member_stride >= 0, "dlwp_ens_score_sums: negative stride");
  DLWP_CHECK_ARG(x && y && sums && hist && ws, "dlwp_ens_score_sums: null pointer");
  const long long cells = (long long)leads * groups;
  DLWP_CHECK_ARG(cells < (1ll << 20), "dlwp_ens_score_sums: %lld (lead, group) cells, at most 2^20", cells);
  const long long tiles_per_row = (run + 63) / 64;
  DLWP_CHECK_ARG(tiles_per_row < (1ll << 31) / samples, "dlwp_ens_score_sums: %d samples of %lld floats are too many tiles", samples, run);
  const long long tiles = (long long)samples * tiles_per_row;
  const long long cap = cell_bpc_cap(h, cells, ens_blocks_per_cu(members));
  const int bpc = (int)(tiles < cap ? tiles : cap);
  const size_t ws_need = (size_t)cells * (size_t)bpc * ens_partial_bytes(members);
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_ens_score_sums: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dlwp_ens_score_sums: workspace must be 8-byte aligned");
  DLWP_CHECK_ARG(h, "dlwp_ens_score_sums: null handle");
  ScoreArgs p;
  p.x = (const float*)x, p.y = (const float*)y, p.crps = (float*)crps_out;
  p.ls = lead_stride, p.ss = sample_stride, p.ms = member_stride, p.run = run;
  p.samples = samples, p.members = members, p.groups = groups, p.bpc = bpc;
  p.tiles_per_row = (unsigned)tiles_per_row;
  p.inv_m = 1.0 / (double)members;
  double* psums = (double*)ws;
  unsigned long long* phist = (unsigned long long*)(psums + 6ll * cells * bpc);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)(cells * bpc);      // <= max(cells, 28 blocks per CU)
  if (members <= 2) ens_score_launch<2, 1>(p, grid, psums, phist, s);
  else if (members <= 4) ens_score_launch<4, 1>(p, grid, psums, phist, s);
  else if (members <= 8) ens_score_launch<8, 1>(p, grid, psums, phist, s);
  else if (members <= 16) ens_score_launch<16, 1>(p, grid, psums, phist, s);
  else if (members <= ENS_RUN) ens_score_launch<32, 1>(p, grid, psums, phist, s);
  else {
    switch (ens_runs(members)) {
      case 2: ens_score_launch<32, 2>(p, grid, psums, phist, s); break;
      case 3: ens_score_launch<32, 3>(p, grid, psums, phist, s); break;
      case 4: ens_score_launch<32, 4>(p, grid, psums, phist, s); break;
      case 5: ens_score_launch<32, 5>(p, grid, psums, phist, s); break;
      case 6: ens_score_launch<32, 6>(p, grid, psums, phist, s); break;
      case 7: ens_score_launch<32, 7>(p, grid, psums, phist, s); break;
      default: ens_score_launch<32, 8>(p, grid, psums, phist, s); break;
    }
  }
  ens_score_final_kernel<<<(unsigned)cells, ENS_THREADS, 0, s>>>(psums, phist, bpc, members, (double*)sums, (long long*)hist);
  DLWP_LAUNCH_CHECK("ens_score_sums kernels");
  return DLWP_OK;
}

}  // extern "C"
