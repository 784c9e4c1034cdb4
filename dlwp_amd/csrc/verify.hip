// verify.hip -- forecast verification where the series is (gfx950): per-lead sums of squared and absolute differences between
// two strided float32 operands, and the NaN-skipping mean over samples that climo_error subtracts.
//
// Reference: DLWP/model/verify.py:17-102 (forecast_error, persistence_error, climo_error; numpy nanmean of diff ** 2 / |diff| per
// forecast step), called by examples/validate.py on the output of predict_timeseries.  dlwp_amd/model/verify.py maps its five
// uses onto dlwp_verify_error_sums (the table in include/dlwp_hip.h) and finishes the few hundred doubles on the host.
// d = a - b is rounded once in float32, as numpy rounds it, and everything behind it is float64.  Every sum is two-stage with a
// fixed tree -- lanes, waves through LDS, one partial per block, a second kernel over the partials of a cell -- without atomics
// and without a "last block" scheme: repeated launches give identical bits.  No launch kernel reads a size from the device and
// the entry points never synchronise.  Every offset is 64-bit: one lead of a 256-member series is 16 M floats, the series 3.6 GB.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int VERIFY_THREADS = 256;
constexpr int VERIFY_BLOCKS_PER_CU = 8;
constexpr int VERIFY_DEFAULT_CU = 256;    // dlwp_verify_error_workspace without a handle: an MI355X

struct VerifyArgs {
  const float* a;
  const float* b;
  long long a_ls, a_ss, b_ls, b_ss;      // lead / sample strides in elements
  int a_shift, b_shift;
  int count0, count_dec;
  int groups, bpc;                       // blocks per (lead, group) cell
  long long run;                         // floats of one group in one sample row
  long long step_row, step_col;          // bpc * 256 units as (rows, columns) of a cell
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// block-wide sums of three doubles; valid in thread 0.  256 threads: 64 lanes, then the four waves in wave order
__device__ __forceinline__ void block_sum3(double& x, double& y, double& z) {
  __shared__ double sm[3][VERIFY_THREADS / 64];
  x = wave_sum_f64(x);
  y = wave_sum_f64(y);
  z = wave_sum_f64(z);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sm[0][wave] = x;
    sm[1][wave] = y;
    sm[2][wave] = z;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    x = ((sm[0][0] + sm[0][1]) + sm[0][2]) + sm[0][3];
    y = ((sm[1][0] + sm[1][1]) + sm[1][2]) + sm[1][3];
    z = ((sm[2][0] + sm[2][1]) + sm[2][2]) + sm[2][3];
  }
}

// one pair: d rounded once in float32 and widened; a NaN d is skipped and not counted (inf - inf too: IEEE)
__device__ __forceinline__ void pair_add(float x, float y, double& s2, double& s1, unsigned long long& n) {
  const float d = x - y;
  const bool ok = d == d;
  const double dd = ok ? (double)d : 0.0;
  s2 = fma(dd, dd, s2);                  // dd * dd is exact in float64 (24 x 24 bits): the same bits as a product and a sum
  s1 += fabs(dd);
  n += ok ? 1ull : 0ull;
}

// stage 1.  Block blk of cell (lead f, group g) takes units blk * 256 + t, + bpc * 256, ... of the cell's count_f x units-per-row
// grid; a unit is four floats (VEC: run % 4 == 0 and every row base 16-byte aligned, checked by the host) or one.  The position
// is divided into (row, column) once and then advanced by the host's (step_row, step_col) with one carry.
template <bool VEC>
__global__ __launch_bounds__(VERIFY_THREADS) void verify_partial_kernel(VerifyArgs p, double* __restrict__ partial) {
  const unsigned cell = blockIdx.x / (unsigned)p.bpc;
  const unsigned blk = blockIdx.x - cell * (unsigned)p.bpc;
  const unsigned f = cell / (unsigned)p.groups, g = cell - f * (unsigned)p.groups;
  const long long cnt = (long long)p.count0 - (long long)f * p.count_dec;      // > 0: the host launches active leads only
  const long long units = VEC ? p.run / 4 : p.run;
  const long long total = cnt * units;
  const long long step = (long long)p.bpc * VERIFY_THREADS;
  const float* pa = p.a + (long long)f * p.a_ls + (long long)f * p.a_shift * p.a_ss + (long long)g * p.run;
  const float* pb = p.b + (long long)f * p.b_ls + (long long)f * p.b_shift * p.b_ss + (long long)g * p.run;
  double s2 = 0.0, s1 = 0.0;
  unsigned long long n = 0;
  long long q = (long long)blk * VERIFY_THREADS + threadIdx.x;
  long long row = q / units, col = q - row * units;
  for (; q < total; q += step) {
    if (VEC) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(pa + row * p.a_ss + 4 * col);
      const f32x4 y = *reinterpret_cast<const f32x4*>(pb + row * p.b_ss + 4 * col);
#pragma unroll
      for (int k = 0; k < 4; ++k) pair_add(x[k], y[k], s2, s1, n);
    } else {
      pair_add(pa[row * p.a_ss + col], pb[row * p.b_ss + col], s2, s1, n);
    }
    row += p.step_row;
    col += p.step_col;
    if (col >= units) {
      col -= units;
      ++row;
    }
  }
  double nd = (double)n;                 // exact below 2^53 pairs
  block_sum3(s2, s1, nd);
  if (threadIdx.x == 0) {
    double* o = partial + 3ll * blockIdx.x;
    o[0] = s2;
    o[1] = s1;
    o[2] = nd;
  }
}

// stage 2: one wave per cell.  Lane l sums partials l, l + 64, ... of its cell in index order, then the lane tree.  Cells of leads
// without pairs (cell >= active_cells) read nothing and store zeros.
__global__ __launch_bounds__(64) void verify_final_kernel(const double* __restrict__ partial, int bpc, int active_cells,
                                                          double* __restrict__ sums) {
  const int cell = blockIdx.x;
  double s2 = 0.0, s1 = 0.0, nd = 0.0;
  if (cell < active_cells) {
    const double* src = partial + 3ll * cell * bpc;
    for (int i = threadIdx.x; i < bpc; i += 64) {
      s2 += src[3 * i + 0];
      s1 += src[3 * i + 1];
      nd += src[3 * i + 2];
    }
  }
  s2 = wave_sum_f64(s2);
  s1 = wave_sum_f64(s1);
  nd = wave_sum_f64(nd);
  if (threadIdx.x == 0) {
    double* o = sums + 3ll * cell;
    o[0] = s2;
    o[1] = s1;
    o[2] = nd;
  }
}

// mean[c] = float32(sum of the non-NaN x[i][c] in float64, i ascending, over their number); NaN where there is none
__global__ __launch_bounds__(VERIFY_THREADS) void verify_nanmean_kernel(const float* __restrict__ x, int count, long long row,
                                                                        float* __restrict__ mean) {
  const long long c = (long long)blockIdx.x * VERIFY_THREADS + threadIdx.x;
  if (c >= row) return;
  double s = 0.0;
  long long n = 0;
  const float* px = x + c;
#pragma unroll 8
  for (int i = 0; i < count; ++i) {
    const float v = px[(long long)i * row];
    const bool ok = v == v;
    s += ok ? (double)v : 0.0;
    n += ok ? 1 : 0;
  }
  mean[c] = n > 0 ? (float)(s / (double)n) : __builtin_nanf("");
}

inline int verify_cu(dlwp_handle_t h) { return h ? h->cu_count : VERIFY_DEFAULT_CU; }

// blocks per cell the handle's CU count allows for this many cells: the whole launch aims at 8 blocks per CU
inline int verify_bpc_cap(dlwp_handle_t h, long long cells) {
  const long long want = (long long)verify_cu(h) * VERIFY_BLOCKS_PER_CU / (cells > 0 ? cells : 1);
  return (int)(want < 1 ? 1 : want);
}

inline bool mult4(long long v) { return (v & 3) == 0; }

}  // namespace

extern "C" {

size_t dlwp_verify_error_workspace(dlwp_handle_t h, int leads, int groups) {
  if (leads < 1 || groups < 1) return 0;
  const long long cells = (long long)leads * groups;
  // B rounded UP: cells * B covers 8 blocks per CU, which is what a launch over fewer (active) leads may spread over its cells
  const long long per_cell = ((long long)verify_cu(h) * VERIFY_BLOCKS_PER_CU + cells - 1) / cells;
  return (size_t)cells * (size_t)per_cell * 3 * sizeof(double);
}

int dlwp_verify_error_sums(dlwp_handle_t h, const void* a, long long a_lead_stride, long long a_sample_stride, int a_shift,
                           const void* b, long long b_lead_stride, long long b_sample_stride, int b_shift, int leads, int count0,
                           int count_dec, int groups, long long run, void* sums, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_error_sums);
  DLWP_CHECK_ARG(leads >= 1 && groups >= 1 && run >= 1, "dlwp_verify_error_sums: leads %d, groups %d, run %lld must all be >= 1",
                 leads, groups, run);
  DLWP_CHECK_ARG(count_dec >= 0 && a_shift >= 0 && b_shift >= 0 && a_lead_stride >= 0 && a_sample_stride >= 0 &&
                     b_lead_stride >= 0 && b_sample_stride >= 0,
                 "dlwp_verify_error_sums: negative stride, shift or count_dec");
  DLWP_CHECK_ARG(a && b && sums && ws, "dlwp_verify_error_sums: null pointer");
  const long long cells = (long long)leads * groups;
  DLWP_CHECK_ARG(cells < (1ll << 20), "dlwp_verify_error_sums: %lld (lead, group) cells, at most 2^20", cells);
  // leads with pairs: count0 - f * count_dec > 0
  long long active = count0 <= 0 ? 0 : (count_dec == 0 ? leads : ((long long)count0 + count_dec - 1) / count_dec);
  if (active > leads) active = leads;
  const bool vec = mult4(run) && mult4(a_lead_stride) && mult4(a_sample_stride) && mult4(b_lead_stride) &&
                   mult4(b_sample_stride) && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
  const long long units = vec ? run / 4 : run;
  int bpc = 0;
  if (active > 0) {
    // no more blocks in a cell than lead 0 (the longest) has 256-unit slices
    const long long need = ((long long)count0 * units + VERIFY_THREADS - 1) / VERIFY_THREADS;
    const long long cap = verify_bpc_cap(h, active * groups);
    bpc = (int)(need < cap ? need : cap);
  }
  const size_t ws_need = (size_t)active * groups * bpc * 3 * sizeof(double);
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_verify_error_sums: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(h, "dlwp_verify_error_sums: null handle");
  hipStream_t s = (hipStream_t)stream;
  if (active > 0) {
    VerifyArgs p;
    p.a = (const float*)a;
    p.b = (const float*)b;
    p.a_ls = a_lead_stride, p.a_ss = a_sample_stride, p.b_ls = b_lead_stride, p.b_ss = b_sample_stride;
    p.a_shift = a_shift, p.b_shift = b_shift;
    p.count0 = count0, p.count_dec = count_dec;
    p.groups = groups, p.bpc = bpc;
    p.run = run;
    const long long step = (long long)bpc * VERIFY_THREADS;
    p.step_row = step / units, p.step_col = step % units;
    const unsigned grid = (unsigned)(active * groups * bpc);      // <= max(cells, 8 blocks per CU)
    if (vec)
      verify_partial_kernel<true><<<grid, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
    else
      verify_partial_kernel<false><<<grid, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
  }
  verify_final_kernel<<<(unsigned)cells, 64, 0, s>>>((const double*)ws, bpc, (int)(active * groups), (double*)sums);
  DLWP_LAUNCH_CHECK("verify_error_sums kernels");
  return DLWP_OK;
}

int dlwp_verify_nanmean_samples(dlwp_handle_t h, const void* x, int count, long long row, void* mean, void* stream) {
  DLWP_UNTAPED(dlwp_verify_nanmean_samples);
  DLWP_CHECK_ARG(count >= 1 && row >= 1, "dlwp_verify_nanmean_samples: count %d and row %lld must be >= 1", count, row);
  DLWP_CHECK_ARG(row <= (long long)0x7fffffff * VERIFY_THREADS, "dlwp_verify_nanmean_samples: row %lld too long", row);
  DLWP_CHECK_ARG(x && mean, "dlwp_verify_nanmean_samples: null pointer");
  DLWP_CHECK_ARG(h, "dlwp_verify_nanmean_samples: null handle");
  const unsigned grid = (unsigned)((row + VERIFY_THREADS - 1) / VERIFY_THREADS);
  verify_nanmean_kernel<<<grid, VERIFY_THREADS, 0, (hipStream_t)stream>>>((const float*)x, count, row, (float*)mean);
  DLWP_LAUNCH_CHECK("verify_nanmean_samples kernel");
  return DLWP_OK;
}

}  // extern "C"
