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
//
// The second half of the reference module (DLWP/model/verify.py:105-273) adds three entry points with the same conventions:
// dlwp_verify_label_nanmean (the mean per calendar month over the whole predictor record: a block owns a label, a chunk of that
// label's sample list and a column tile, a second launch adds the chunks in order), dlwp_verify_label_error_sums (the error of
// selected rows against that table: one cell of the tree above, with an optional anomaly output) and dlwp_gather_rows_fill (the
// verification windows: rows copied by index, NaN rows where the record has no state).
#include "common.h"

#include <type_traits>

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

// ---- means per label (calendar month) over a long record, and the error of selected rows against such a table -------------------- //
constexpr int VERIFY_MAX_LABELS = 64;

struct LabelMeanArgs {
  const float* x;
  const int* index;                      // sample indices grouped by label, ascending inside a label
  long long row;
  int count, split, tiles;
  int off[VERIFY_MAX_LABELS + 1];        // list of label l: index[off[l] .. off[l + 1])
};

__device__ __forceinline__ void nan_add(float v, double& s, int& n) {
  const bool ok = v == v;
  s += ok ? (double)v : 0.0;
  n += ok ? 1 : 0;
}

// stage 1.  A block owns (label, chunk k of that label's list, column tile): list positions [len * k / split, len * (k + 1) / split),
// 256 threads x (VEC: four adjacent columns, one 16-byte load per sample; else one).  The sample index is the same in every lane;
// four rows are in flight per thread and are added in list order.  An index outside the record is skipped, never read.
template <bool VEC>
__global__ __launch_bounds__(VERIFY_THREADS) void verify_label_partial_kernel(LabelMeanArgs p, double* __restrict__ psum,
                                                                              int* __restrict__ pcnt) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned cell = blockIdx.x / (unsigned)p.tiles;
  const unsigned tile = blockIdx.x - cell * (unsigned)p.tiles;
  const unsigned label = cell / (unsigned)p.split, chunk = cell - label * (unsigned)p.split;
  const long long c = ((long long)tile * VERIFY_THREADS + threadIdx.x) * W;
  if (c >= p.row) return;
  const long long lo = p.off[label], len = p.off[label + 1] - lo;
  long long i = lo + len * chunk / p.split;
  const long long end = lo + len * (chunk + 1) / p.split;
  const float* px = p.x + c;
  double s[W];
  int n[W];
#pragma unroll
  for (int k = 0; k < W; ++k) s[k] = 0.0, n[k] = 0;
  const float qnan = __builtin_nanf("");
  for (; i + 4 <= end; i += 4) {
    float v[4][W];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = p.index[i + u];
      const bool in = (unsigned)r < (unsigned)p.count;
      const float* q = px + (long long)(in ? r : 0) * p.row;
      if (VEC) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
        for (int k = 0; k < W; ++k) v[u][k] = in ? t[k] : qnan;
      } else {
        v[u][0] = in ? q[0] : qnan;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) nan_add(v[u][k], s[k], n[k]);
  }
  for (; i < end; ++i) {
    const int r = p.index[i];
    if ((unsigned)r >= (unsigned)p.count) continue;
    const float* q = px + (long long)r * p.row;
    if (VEC) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
      for (int k = 0; k < W; ++k) nan_add(t[k], s[k], n[k]);
    } else {
      nan_add(q[0], s[0], n[0]);
    }
  }
  const long long o = (long long)cell * p.row + c;
#pragma unroll
  for (int k = 0; k < W; ++k) psum[o + k] = s[k], pcnt[o + k] = n[k];
}

// stage 2: one thread per (label, column) adds the chunks in chunk order, divides once and rounds once
__global__ __launch_bounds__(VERIFY_THREADS) void verify_label_final_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                                            long long row, int split, int tiles,
                                                                            float* __restrict__ mean) {
  const unsigned label = blockIdx.x / (unsigned)tiles;
  const long long c = (long long)(blockIdx.x - label * (unsigned)tiles) * VERIFY_THREADS + threadIdx.x;
  if (c >= row) return;
  double s = 0.0;
  long long n = 0;
  for (int k = 0; k < split; ++k) {
    const long long o = ((long long)label * split + k) * row + c;
    s += psum[o];
    n += pcnt[o];
  }
  mean[(long long)label * row + c] = n > 0 ? (float)(s / (double)n) : __builtin_nanf("");
}

struct LabelErrorArgs {
  const float* x;
  const int* rows;
  const int* labels;
  const float* table;
  float* anomaly;                        // may be null
  long long row;                         // floats of a row
  int count_x, m, n_labels, bpc;
  long long step_row, step_col;
};

// d = x[rows[i]] - table[labels[i]] over i < m as ONE cell of verify_partial_kernel's tree: units, steps and partials as there.  A row
// index or label outside its range makes the whole row NaN (skipped, not counted, NaN in `anomaly`) and is never used as an address.
template <bool VEC>
__global__ __launch_bounds__(VERIFY_THREADS) void verify_label_error_kernel(LabelErrorArgs p, double* __restrict__ partial) {
  const long long units = VEC ? p.row / 4 : p.row;
  const long long total = (long long)p.m * units;
  const long long step = (long long)p.bpc * VERIFY_THREADS;
  const float qnan = __builtin_nanf("");
  double s2 = 0.0, s1 = 0.0;
  unsigned long long n = 0;
  long long q = (long long)blockIdx.x * VERIFY_THREADS + threadIdx.x;
  long long i = q / units, col = q - i * units;
  for (; q < total; q += step) {
    const int r = p.rows[i], l = p.labels[i];
    const bool in = (unsigned)r < (unsigned)p.count_x && (unsigned)l < (unsigned)p.n_labels;
    const float* px = p.x + (long long)(in ? r : 0) * p.row;
    const float* pt = p.table + (long long)(in ? l : 0) * p.row;
    if (VEC) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(px + 4 * col);
      const f32x4 y = *reinterpret_cast<const f32x4*>(pt + 4 * col);
      f32x4 d;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xv = in ? x[k] : qnan;
        d[k] = xv - y[k];
        pair_add(xv, y[k], s2, s1, n);
      }
      if (p.anomaly) *reinterpret_cast<f32x4*>(p.anomaly + i * p.row + 4 * col) = d;
    } else {
      const float xv = in ? px[col] : qnan, yv = pt[col];
      pair_add(xv, yv, s2, s1, n);
      if (p.anomaly) p.anomaly[i * p.row + col] = xv - yv;
    }
    i += p.step_row;
    col += p.step_col;
    if (col >= units) {
      col -= units;
      ++i;
    }
  }
  double nd = (double)n;
  block_sum3(s2, s1, nd);
  if (threadIdx.x == 0) {
    double* o = partial + 3ll * blockIdx.x;
    o[0] = s2;
    o[1] = s1;
    o[2] = nd;
  }
}

// ---- dst[j] = src[rows[j]], a quiet NaN row where rows[j] is no row of src -------------------------------------------------------- //
struct GatherArgs {
  const unsigned* src;
  const long long* rows;
  unsigned* dst;
  long long src_rows, row, total;        // total: n * units
  long long step, step_row, step_col;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// bits are moved as unsigned words, so NaN payloads survive.  A thread carries four units (one 16-byte word or one float each) per
// turn: the four loads are issued before the four stores.
template <bool VEC>
__global__ __launch_bounds__(VERIFY_THREADS) void gather_rows_fill_kernel(GatherArgs p) {
  typedef typename std::conditional<VEC, u32x4, unsigned>::type word_t;
  constexpr int W = VEC ? 4 : 1;
  const long long units = p.row / W;
  const unsigned qnan = 0x7fc00000u;
  long long q = (long long)blockIdx.x * VERIFY_THREADS + threadIdx.x;
  long long j = q / units, col = q - j * units;
  while (q < p.total) {
    word_t v[4];
    long long at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      at[u] = -1;
      if (q < p.total) {
        const long long r = p.rows[j];
        const bool in = r >= 0 && r < p.src_rows;
        const word_t t = *reinterpret_cast<const word_t*>(p.src + (in ? r : 0) * p.row + col * W);
        v[u] = in ? t : (word_t)qnan;
        at[u] = j * p.row + col * W;
      }
      q += p.step;
      j += p.step_row;
      col += p.step_col;
      if (col >= units) {
        col -= units;
        ++j;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (at[u] >= 0) *reinterpret_cast<word_t*>(p.dst + at[u]) = v[u];
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline long long label_tiles(long long row, bool vec) { return ((vec ? row / 4 : row) + VERIFY_THREADS - 1) / VERIFY_THREADS; }

// chunks per label: 8 blocks per CU over the (label, column tile) cells, and never more chunks than samples
inline int label_split(dlwp_handle_t h, int count, long long row, int n_labels, bool vec) {
  const long long cap = verify_bpc_cap(h, (long long)n_labels * label_tiles(row, vec));
  return (int)(cap < count ? cap : count);
}

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

size_t dlwp_verify_label_nanmean_workspace(dlwp_handle_t h, int count, long long row, int n_labels) {
  if (count < 1 || row < 1 || n_labels < 1 || n_labels > VERIFY_MAX_LABELS) return 0;
  // the 16-byte route has the fewer cells and therefore the larger split: enough for either route
  const int split = label_split(h, count, row, n_labels, mult4(row));
  return (size_t)n_labels * (size_t)split * (size_t)row * (sizeof(double) + sizeof(int));
}

int dlwp_verify_label_nanmean(dlwp_handle_t h, const void* x, int count, long long row, const int* offsets, const void* index,
                              int n_labels, void* mean, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_label_nanmean);
  DLWP_CHECK_ARG(count >= 1 && row >= 1, "dlwp_verify_label_nanmean: count %d and row %lld must be >= 1", count, row);
  DLWP_CHECK_ARG(n_labels >= 1 && n_labels <= VERIFY_MAX_LABELS, "dlwp_verify_label_nanmean: n_labels %d, expected 1 .. %d", n_labels,
                 VERIFY_MAX_LABELS);
  DLWP_CHECK_ARG(x && offsets && index && mean && ws, "dlwp_verify_label_nanmean: null pointer");
  DLWP_CHECK_ARG(offsets[0] == 0 && offsets[n_labels] == count,
                 "dlwp_verify_label_nanmean: offsets must run from 0 to count %d, got %d .. %d", count, offsets[0], offsets[n_labels]);
  for (int l = 0; l < n_labels; ++l)
    DLWP_CHECK_ARG(offsets[l] <= offsets[l + 1], "dlwp_verify_label_nanmean: offsets decrease at label %d", l);
  const bool vec = mult4(row) && aligned16(x);
  const long long tiles = label_tiles(row, vec);
  const int split = label_split(h, count, row, n_labels, vec);
  const long long ftiles = label_tiles(row, false);
  DLWP_CHECK_ARG((long long)n_labels * split * tiles < (1ll << 31) && n_labels * ftiles < (1ll << 31),
                 "dlwp_verify_label_nanmean: row %lld too long", row);
  const size_t cells = (size_t)n_labels * (size_t)split * (size_t)row;
  const size_t ws_need = cells * (sizeof(double) + sizeof(int));
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_verify_label_nanmean: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dlwp_verify_label_nanmean: workspace must be 8-byte aligned");
  DLWP_CHECK_ARG(h, "dlwp_verify_label_nanmean: null handle");
  LabelMeanArgs p;
  p.x = (const float*)x;
  p.index = (const int*)index;
  p.row = row;
  p.count = count, p.split = split, p.tiles = (int)tiles;
  for (int l = 0; l <= VERIFY_MAX_LABELS; ++l) p.off[l] = offsets[l < n_labels ? l : n_labels];
  double* psum = (double*)ws;
  int* pcnt = (int*)(psum + cells);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)((long long)n_labels * split * tiles);
  if (vec)
    verify_label_partial_kernel<true><<<grid, VERIFY_THREADS, 0, s>>>(p, psum, pcnt);
  else
    verify_label_partial_kernel<false><<<grid, VERIFY_THREADS, 0, s>>>(p, psum, pcnt);
  verify_label_final_kernel<<<(unsigned)(n_labels * ftiles), VERIFY_THREADS, 0, s>>>(psum, pcnt, row, split, (int)ftiles, (float*)mean);
  DLWP_LAUNCH_CHECK("verify_label_nanmean kernels");
  return DLWP_OK;
}

int dlwp_verify_label_error_sums(dlwp_handle_t h, const void* x, int count_x, long long row, const void* rows, const void* labels, int m,
                                 const void* table, int n_labels, void* anomaly, void* sums, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_label_error_sums);
  DLWP_CHECK_ARG(count_x >= 1 && m >= 1 && row >= 1, "dlwp_verify_label_error_sums: count_x %d, m %d, row %lld must all be >= 1", count_x,
                 m, row);
  DLWP_CHECK_ARG(n_labels >= 1 && n_labels <= VERIFY_MAX_LABELS, "dlwp_verify_label_error_sums: n_labels %d, expected 1 .. %d", n_labels,
                 VERIFY_MAX_LABELS);
  DLWP_CHECK_ARG(x && rows && labels && table && sums && ws, "dlwp_verify_label_error_sums: null pointer");
  const bool vec = mult4(row) && aligned16(x) && aligned16(table) && aligned16(anomaly);
  const long long units = vec ? row / 4 : row;
  const long long need = ((long long)m * units + VERIFY_THREADS - 1) / VERIFY_THREADS;
  const long long cap = verify_bpc_cap(h, 1);
  const int bpc = (int)(need < cap ? need : cap);
  const size_t ws_need = (size_t)bpc * 3 * sizeof(double);
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_verify_label_error_sums: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(h, "dlwp_verify_label_error_sums: null handle");
  LabelErrorArgs p;
  p.x = (const float*)x, p.rows = (const int*)rows, p.labels = (const int*)labels, p.table = (const float*)table;
  p.anomaly = (float*)anomaly;
  p.row = row;
  p.count_x = count_x, p.m = m, p.n_labels = n_labels, p.bpc = bpc;
  const long long step = (long long)bpc * VERIFY_THREADS;
  p.step_row = step / units, p.step_col = step % units;
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    verify_label_error_kernel<true><<<(unsigned)bpc, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
  else
    verify_label_error_kernel<false><<<(unsigned)bpc, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
  verify_final_kernel<<<1, 64, 0, s>>>((const double*)ws, bpc, 1, (double*)sums);
  DLWP_LAUNCH_CHECK("verify_label_error_sums kernels");
  return DLWP_OK;
}

int dlwp_gather_rows_fill(dlwp_handle_t h, const void* src, long long src_rows, long long row, const void* rows, long long n, void* dst,
                          void* stream) {
  DLWP_UNTAPED(dlwp_gather_rows_fill);
  DLWP_CHECK_ARG(src_rows >= 1 && row >= 1 && n >= 0, "dlwp_gather_rows_fill: src_rows %lld, row %lld must be >= 1 and n %lld >= 0",
                 src_rows, row, n);
  DLWP_CHECK_ARG(n <= 0x7fffffffffffffffll / row / 4, "dlwp_gather_rows_fill: n %lld rows of %lld floats overflow", n, row);
  if (n == 0) return DLWP_OK;
  DLWP_CHECK_ARG(src && rows && dst, "dlwp_gather_rows_fill: null pointer");
  DLWP_CHECK_ARG(h, "dlwp_gather_rows_fill: null handle");
  const bool vec = mult4(row) && aligned16(src) && aligned16(dst);
  const long long units = vec ? row / 4 : row;
  GatherArgs p;
  p.src = (const unsigned*)src, p.rows = (const long long*)rows, p.dst = (unsigned*)dst;
  p.src_rows = src_rows, p.row = row, p.total = n * units;
  // a block moves 4 x 256 units a turn
  const long long need = (p.total + 4 * VERIFY_THREADS - 1) / (4 * VERIFY_THREADS);
  const long long cap = verify_bpc_cap(h, 1);
  const long long grid = need < cap ? need : cap;
  p.step = grid * VERIFY_THREADS;
  p.step_row = p.step / units, p.step_col = p.step % units;
  if (vec)
    gather_rows_fill_kernel<true><<<(unsigned)grid, VERIFY_THREADS, 0, (hipStream_t)stream>>>(p);
  else
    gather_rows_fill_kernel<false><<<(unsigned)grid, VERIFY_THREADS, 0, (hipStream_t)stream>>>(p);
  DLWP_LAUNCH_CHECK("gather_rows_fill kernel");
  return DLWP_OK;
}

}  // extern "C"
