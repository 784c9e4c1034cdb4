// verify.hip -- forecast verification where the series is (gfx950): per-lead sums of squared and absolute differences between
// two strided float32 operands, and the NaN-skipping mean over samples that climo_error subtracts.
//
// Reference: DLWP/model/verify.py:17-102 (forecast_error, persistence_error, climo_error; numpy nanmean of diff ** 2 / |diff| per
// forecast step), called by examples/validate.py on the output of predict_timeseries.  dlwp_amd/model/verify.py maps its five
// uses onto dlwp_verify_error_sums (the table in include/dlwp_hip.h) and finishes the few hundred doubles on the host.
// d = a - b is rounded once in float32, as numpy rounds it, and everything behind it is float64.  Every sum is two-stage on the
// fixed tree of verify_common.h: repeated launches give identical bits.  No launch kernel reads a size from the device and
// the entry points never synchronise.  Every offset is 64-bit: one lead of a 256-member series is 16 M floats, the series 3.6 GB.
//
// The second half of the reference module (DLWP/model/verify.py:105-273) adds three entry points with the same conventions:
// dlwp_verify_label_nanmean (the mean per calendar month over the whole predictor record: a block owns a label, a chunk of that
// label's sample list and a column tile, a second launch adds the chunks in order), dlwp_verify_label_error_sums (the error of
// selected rows against that table: one cell of the tree above, with an optional anomaly output) and dlwp_gather_rows_fill (the
// verification windows: rows copied by index, NaN rows where the record has no state).
#include "verify_common.h"

#include <type_traits>

namespace {

constexpr int VERIFY_THREADS = 256;
constexpr int VERIFY_BLOCKS_PER_CU = 8;

struct VerifyArgs {
  Window a, b;
  int count0, count_dec;
  int groups, bpc;                       // blocks per (lead, group) cell
  long long run;                         // floats of one group in one sample row
  UnitStep step;                         // bpc * 256 units as (rows, columns) of a cell
};

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
// is divided into (row, column) once and then advanced by the host's step with one carry (UnitWalk).
template <bool VEC>
__global__ __launch_bounds__(VERIFY_THREADS) void verify_partial_kernel(VerifyArgs p, double* __restrict__ partial) {
  const unsigned cell = blockIdx.x / (unsigned)p.bpc;
  const unsigned blk = blockIdx.x - cell * (unsigned)p.bpc;
  const unsigned f = cell / (unsigned)p.groups, g = cell - f * (unsigned)p.groups;
  const long long cnt = window_pairs(p.count0, p.count_dec, f);      // > 0: the host launches active leads only
  const long long units = VEC ? p.run / 4 : p.run;
  const long long total = cnt * units;
  const long long step = (long long)p.bpc * VERIFY_THREADS;
  const float* pa = p.a.lead(f, g, p.run);
  const float* pb = p.b.lead(f, g, p.run);
  const int wave = wave_number();
  double s2 = 0.0, s1 = 0.0;
  unsigned long long n = 0;
  long long q = (long long)blk * VERIFY_THREADS + threadIdx.x;
  UnitWalk at(q, units);
  for (; q < total; q += step) {
    if (VEC) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(pa + at.row * p.a.ss + 4 * at.col);
      const f32x4 y = *reinterpret_cast<const f32x4*>(pb + at.row * p.b.ss + 4 * at.col);
#pragma unroll
      for (int k = 0; k < 4; ++k) pair_add(x[k], y[k], s2, s1, n);
    } else {
      pair_add(pa[at.row * p.a.ss + at.col], pb[at.row * p.b.ss + at.col], s2, s1, n);
    }
    at.advance(p.step, units);
  }
  double v[3] = {s2, s1, (double)n};     // the count is exact below 2^53 pairs
  block_sums<3>(v, wave, partial + 3ll * blockIdx.x);
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
  UnitStep step;
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
  const int wave = wave_number();
  long long q = (long long)blockIdx.x * VERIFY_THREADS + threadIdx.x;
  UnitWalk at(q, units);
  for (; q < total; q += step) {
    const long long i = at.row, col = at.col;
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
    at.advance(p.step, units);
  }
  double v[3] = {s2, s1, (double)n};
  block_sums<3>(v, wave, partial + 3ll * blockIdx.x);
}

// ---- dst[j] = src[rows[j]], a quiet NaN row where rows[j] is no row of src -------------------------------------------------------- //
struct GatherArgs {
  const unsigned* src;
  const long long* rows;
  unsigned* dst;
  long long src_rows, row, total;        // total: n * units
  long long step;
  UnitStep step2;                        // `step` units as (rows, columns)
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
  UnitWalk w(q, units);
  while (q < p.total) {
    word_t v[4];
    long long at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      at[u] = -1;
      if (q < p.total) {
        const long long r = p.rows[w.row];
        const bool in = r >= 0 && r < p.src_rows;
        const word_t t = *reinterpret_cast<const word_t*>(p.src + (in ? r : 0) * p.row + w.col * W);
        v[u] = in ? t : (word_t)qnan;
        at[u] = w.row * p.row + w.col * W;
      }
      q += p.step;
      w.advance(p.step2, units);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (at[u] >= 0) *reinterpret_cast<word_t*>(p.dst + at[u]) = v[u];
  }
}

inline long long label_tiles(long long row, bool vec) { return ((vec ? row / 4 : row) + VERIFY_THREADS - 1) / VERIFY_THREADS; }

// chunks per label: 8 blocks per CU over the (label, column tile) cells, and never more chunks than samples
inline int label_split(dlwp_handle_t h, int count, long long row, int n_labels, bool vec) {
  const long long cap = cell_bpc_cap(h, (long long)n_labels * label_tiles(row, vec), VERIFY_BLOCKS_PER_CU);
  return (int)(cap < count ? cap : count);
}

}  // namespace

extern "C" {

size_t dlwp_verify_error_workspace(dlwp_handle_t h, int leads, int groups) {
  if (leads < 1 || groups < 1) return 0;
  return cell_workspace_bytes(h, (long long)leads * groups, VERIFY_BLOCKS_PER_CU, 3 * sizeof(double));
}

int dlwp_verify_error_sums(dlwp_handle_t h, const void* a, long long a_lead_stride, long long a_sample_stride, int a_shift,
                           const void* b, long long b_lead_stride, long long b_sample_stride, int b_shift, int leads, int count0,
                           int count_dec, int groups, long long run, void* sums, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_error_sums);
  DLWP_CHECK_ARG(leads >= 1 && groups >= 1 && run >= 1, "dlwp_verify_error_sums: leads %d, groups %d, run %lld must all be >= 1",
                 leads, groups, run);
  VerifyArgs p;
  p.a = window_of(a, a_lead_stride, a_sample_stride, a_shift);
  p.b = window_of(b, b_lead_stride, b_sample_stride, b_shift);
  DLWP_CHECK_ARG(count_dec >= 0 && window_nonneg(p.a) && window_nonneg(p.b),
                 "dlwp_verify_error_sums: negative stride, shift or count_dec");
  // inherited: this entry point wants a workspace pointer even where no partial is written (skill and spectrum do not)
  DLWP_CHECK_ARG(a && b && sums && ws, "dlwp_verify_error_sums: null pointer");
  const long long cells = (long long)leads * groups;
  // inherited: fewer than 2^20 cells here, at most 2^20 in skill.hip and spectrum.hip
  DLWP_CHECK_ARG(cells < (1ll << 20), "dlwp_verify_error_sums: %lld (lead, group) cells, at most 2^20", cells);
  const long long active = window_active_leads(leads, count0, count_dec);
  const bool vec = mult4(run) && window_vec(p.a) && window_vec(p.b);
  const long long units = vec ? run / 4 : run;
  // no more blocks in a cell than lead 0 (the longest) has 256-unit slices
  const int bpc = cell_plan_bpc(h, active, groups, ((long long)count0 * units + VERIFY_THREADS - 1) / VERIFY_THREADS,
                                VERIFY_BLOCKS_PER_CU);
  const size_t ws_need = (size_t)active * groups * bpc * 3 * sizeof(double);
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_verify_error_sums: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(h, "dlwp_verify_error_sums: null handle");
  hipStream_t s = (hipStream_t)stream;
  if (active > 0) {
    p.count0 = count0, p.count_dec = count_dec;
    p.groups = groups, p.bpc = bpc;
    p.run = run;
    p.step = unit_step((long long)bpc * VERIFY_THREADS, units);
    const unsigned grid = (unsigned)(active * groups * bpc);      // <= max(cells, 8 blocks per CU)
    if (vec)
      verify_partial_kernel<true><<<grid, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
    else
      verify_partial_kernel<false><<<grid, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
  }
  cell_final_kernel<3><<<(unsigned)cells, 64, 0, s>>>((const double*)ws, bpc, (int)(active * groups), (double*)sums);
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
  const long long cap = cell_bpc_cap(h, 1, VERIFY_BLOCKS_PER_CU);
  const int bpc = (int)(need < cap ? need : cap);
  const size_t ws_need = (size_t)bpc * 3 * sizeof(double);
  DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_verify_label_error_sums: workspace too small (%zu < %zu)", ws_bytes, ws_need);
  DLWP_CHECK_ARG(h, "dlwp_verify_label_error_sums: null handle");
  LabelErrorArgs p;
  p.x = (const float*)x, p.rows = (const int*)rows, p.labels = (const int*)labels, p.table = (const float*)table;
  p.anomaly = (float*)anomaly;
  p.row = row;
  p.count_x = count_x, p.m = m, p.n_labels = n_labels, p.bpc = bpc;
  p.step = unit_step((long long)bpc * VERIFY_THREADS, units);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    verify_label_error_kernel<true><<<(unsigned)bpc, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
  else
    verify_label_error_kernel<false><<<(unsigned)bpc, VERIFY_THREADS, 0, s>>>(p, (double*)ws);
  cell_final_kernel<3><<<1, 64, 0, s>>>((const double*)ws, bpc, 1, (double*)sums);
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
  const long long cap = cell_bpc_cap(h, 1, VERIFY_BLOCKS_PER_CU);
  const long long grid = need < cap ? need : cap;
  p.step = grid * VERIFY_THREADS;
  p.step2 = unit_step(p.step, units);
  if (vec)
    gather_rows_fill_kernel<true><<<(unsigned)grid, VERIFY_THREADS, 0, (hipStream_t)stream>>>(p);
  else
    gather_rows_fill_kernel<false><<<(unsigned)grid, VERIFY_THREADS, 0, (hipStream_t)stream>>>(p);
  DLWP_LAUNCH_CHECK("gather_rows_fill kernel");
  return DLWP_OK;
}

}  // extern "C"
