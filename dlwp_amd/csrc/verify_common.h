// verify_common.h -- what the device verification files share (verify, skill, skill_map, spectrum, ensemble, events, quantile .hip;
// series.hip and halo.hip take the two route predicates).  DESIGN.md 5.43.  Only what at least two translation units use lives here:
//   * the small helpers: f32x4, mult4, aligned16, the lane tree wave_sum_f64, dlwp_cu (a handle's CU count, an MI355X without one);
//   * the WINDOW: one operand of a per-lead comparison -- base, lead stride, sample stride and shift per lead -- with the pair count
//     count0 - f * count_dec of lead f, the leads that have pairs, the argument check and the 16-byte route predicate;
//   * the PLAN of a launch over (lead, group) cells: blocks per cell and the workspace bound that covers it;
//   * the TREE behind "repeated calls give identical bits": per-thread float64 sums, 64 lanes (wave_sum_f64), the four waves of a
//     256-thread block through LDS in wave order (block_sums), one partial of N doubles per block, and a second launch in which one
//     wave adds a cell's partials in index order and finishes with the lane tree (cell_final).  No atomics, no "last block" scheme, no
//     size read from the device; the order of every addition is fixed by the launch shape alone;
//   * the UNIT WALK of a block-strided loop over a (rows x units-per-row) grid: divided once, then advanced with one carry.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {      // every translation unit has its own copy: nothing here is exported

constexpr int DLWP_DEFAULT_CU = 256;       // the workspace queries without a handle: an MI355X

inline int dlwp_cu(dlwp_handle_t h) { return h ? h->cu_count : DLWP_DEFAULT_CU; }
inline bool mult4(long long v) { return (v & 3) == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }      // null counts as aligned

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// ---- the window ------------------------------------------------------------------------------------------------------------------- //
// Lead f of an operand starts f lead strides and f * shift sample rows behind the base (the table in include/dlwp_hip.h); group g
// of a sample row starts g runs further.
struct Window {
  const float* base;
  long long ls, ss;                        // lead / sample strides in elements
  int shift;

  __device__ __forceinline__ const float* lead(unsigned f) const { return base + (long long)f * ls + (long long)f * shift * ss; }
  __device__ __forceinline__ const float* lead(unsigned f, unsigned g, long long run) const { return lead(f) + (long long)g * run; }
};

inline Window window_of(const void* base, long long lead_stride, long long sample_stride, int shift) {
  Window w;
  w.base = (const float*)base, w.ls = lead_stride, w.ss = sample_stride, w.shift = shift;
  return w;
}

// pairs of lead f; <= 0: none
__host__ __device__ __forceinline__ long long window_pairs(int count0, int count_dec, unsigned f) {
  return (long long)count0 - (long long)f * count_dec;
}

// leads with pairs: count0 - f * count_dec > 0
inline long long window_active_leads(int leads, int count0, int count_dec) {
  const long long active = count0 <= 0 ? 0 : (count_dec == 0 ? leads : ((long long)count0 + count_dec - 1) / count_dec);
  return active > leads ? leads : active;
}

// "negative stride, shift or count_dec" is refused when one of these (or count_dec >= 0) fails
inline bool window_nonneg(const Window& w) { return w.ls >= 0 && w.ss >= 0 && w.shift >= 0; }

// every row base of the operand is 16-byte aligned (the run length is the caller's to test)
inline bool window_vec(const Window& w) { return mult4(w.ls) && mult4(w.ss) && aligned16(w.base); }

// ---- the plan of a launch over (lead, group) cells ---------------------------------------------------------------------------------- //
// blocks per cell the handle's CU count allows for this many cells: the whole launch aims at blocks_per_cu blocks per CU; at least 1
inline long long cell_bpc_cap(dlwp_handle_t h, long long cells, int blocks_per_cu) {
  const long long want = (long long)dlwp_cu(h) * blocks_per_cu / (cells > 0 ? cells : 1);
  return want < 1 ? 1 : want;
}

// blocks per cell of a launch over the active leads: no more than `need` (what lead 0, the longest, can use); 0 without an active lead
inline int cell_plan_bpc(dlwp_handle_t h, long long active, int groups, long long need, int blocks_per_cu) {
  if (active <= 0) return 0;
  const long long cap = cell_bpc_cap(h, active * groups, blocks_per_cu);
  return (int)(need < cap ? need : cap);
}

// the workspace bound: cells x blocks per cell rounded UP x bytes per partial.  Rounded up, cells * per_cell covers blocks_per_cu
// blocks per CU, which is what a launch over fewer (active) leads may spread over its cells
inline size_t cell_workspace_bytes(dlwp_handle_t h, long long cells, int blocks_per_cu, size_t partial_bytes) {
  const long long per_cell = ((long long)dlwp_cu(h) * blocks_per_cu + cells - 1) / cells;
  return (size_t)cells * (size_t)per_cell * partial_bytes;
}

// ---- the tree --------------------------------------------------------------------------------------------------------------------- //
// Block stage, 256 threads: out[k] = the block's sum of v[k], k < N -- 64 lanes, then the four waves in wave order; lane k of wave 0
// stores sum k.  `wave` is the caller's, made with wave_number() IN FRONT of its loop: the number then lives in a scalar register and
// the lane is recomputed here, so no thread index is kept across the loop (skill_partial_kernel holds 64 registers that way, and no
// other user's count rose with it -- one form for all).
__device__ __forceinline__ int wave_number() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

template <int N>
__device__ __forceinline__ void block_sums(double (&v)[N], int wave, double* __restrict__ out) {
  __shared__ double sm[N][4];
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = wave_sum_f64(v[k]);
    if (lane == 0) sm[k][wave] = v[k];
  }
  __syncthreads();
  if (wave == 0 && lane < N) {
    const int k = lane;
    out[k] = ((sm[k][0] + sm[k][1]) + sm[k][2]) + sm[k][3];
  }
}

// Cell stage, one wave: lane l sums partials l, l + 64, ... of the cell in index order, then the lane tree; lane 0 stores.  A cell
// without pairs (!live) reads nothing and stores zeros.
template <int N>
__device__ __forceinline__ void cell_final(const double* __restrict__ partial, int bpc, long long cell, bool live, int lane,
                                           double* __restrict__ sums) {
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  if (live) {
    const double* src = partial + (long long)N * cell * bpc;
    for (int i = lane; i < bpc; i += 64) {
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] += src[(long long)N * i + k];
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum_f64(v[k]);
  if (lane == 0) {
    double* o = sums + (long long)N * cell;
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = v[k];
  }
}

// one 64-thread block per cell; cells of leads without pairs (cell >= active_cells) store zeros
template <int N>
__global__ __launch_bounds__(64) void cell_final_kernel(const double* __restrict__ partial, int bpc, int active_cells,
                                                        double* __restrict__ sums) {
  cell_final<N>(partial, bpc, blockIdx.x, (int)blockIdx.x < active_cells, threadIdx.x, sums);
}

// ---- the unit walk ------------------------------------------------------------------------------------------------------------------ //
// A thread's position in a grid of `units` per row: divided once, then advanced by the host's step with one carry.
struct UnitStep {
  long long row, col;                      // a step of (blocks x threads) units as whole rows and the rest
};

inline UnitStep unit_step(long long step, long long units) {
  UnitStep s;
  s.row = step / units, s.col = step % units;
  return s;
}

struct UnitWalk {
  long long row, col;

  __device__ __forceinline__ UnitWalk(long long q, long long units) : row(q / units), col(q - row * units) {}
  __device__ __forceinline__ void advance(const UnitStep& s, long long units) {
    row += s.row;
    col += s.col;
    if (col >= units) {
      col -= units;
      ++row;
    }
  }
};

}  // namespace
