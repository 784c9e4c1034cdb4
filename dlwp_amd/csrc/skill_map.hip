// skill_map.hip -- forecast skill per grid point where the series is (gfx950): the sums of skill.hip reduced over the SAMPLES of a
// lead at every point of the sample row instead of over the row, and the scores made from them on the device.
//
// dlwp_verify_skill_map addresses its operands, the climatology table and the labels exactly as dlwp_verify_skill_sums does with
// groups = 1 and run = row (include/dlwp_hip.h); there are no weights -- a weight is constant per point and cancels.  Per pair
// d = fc - ob, fa = fc - c, oa = ob - c are rounded once in float32; a pair with a NaN among them, or with a label outside
// [0, n_labels), is skipped for that point; everything behind that is float64.  The reduction runs along the strided sample axis and
// keeps the contiguous one, so there is no tree: a thread owns one unit (four adjacent points with 16-byte loads, or one point) of
// one lead and walks that lead's samples -- or one of `split` chunks of them -- in sample order with its sums in registers.  With one
// chunk the same launch makes the scores; with several, the chunks' planes go to the workspace and a second launch adds them in chunk
// order.  No atomics, no "last block" scheme, no size read from the device, no synchronisation: repeated calls give identical bits.
#include "verify_common.h"

namespace {

constexpr int MAP_THREADS = 256;
constexpr int MAP_BLOCKS_PER_CU = 8;     // the split rule of dlwp_verify_label_nanmean: chunks until 8 blocks per CU exist
constexpr int MAP_SUMS = 9;
constexpr int MAP_SCORES = 6;
constexpr int MAP_MAX_LABELS = 64;

struct MapArgs {
  Window fc, ob;
  const float* climo;                    // (n_labels, row) or null
  const int* labels;                     // may be null: label 0
  long long lab_ls;
  int lab_shift;
  int count0, count_dec;
  int n_labels, split, tiles;
  long long row;
  double* partial;                       // split > 1: (leads, split, 9, row)
  double* sums;                          // split == 1: the outputs, each may be null
  float* scores;
  int* counts;
};

// finish_skill's formulas with S0 = count, in float64, cast once.  Nothing here may be contracted into a fused multiply-add: every
// single operation then rounds as the host's does
__device__ __forceinline__ void map_scores(const double (&v)[MAP_SUMS], float (&out)[MAP_SCORES]) {
#pragma clang fp contract(off)
  const double qnan = __builtin_nan("");
  const bool some = v[8] > 0.0;
  const double s0 = some ? v[8] : qnan;
  const double mse = v[1] / s0;
  const double m_f = v[3] / s0, m_o = v[4] / s0;
  const double raw = sqrt(v[6] * v[7]);
  const double var_f = v[6] / s0 - m_f * m_f, var_o = v[7] / s0 - m_o * m_o;
  const double cen = sqrt(var_f * var_o);
  const double cov = v[5] / s0 - m_f * m_o;
  out[0] = (float)mse;
  out[1] = (float)sqrt(mse);
  out[2] = (float)(v[2] / s0);
  out[3] = (float)(v[0] / s0);
  out[4] = (float)(some && raw > 0.0 ? v[5] / raw : qnan);
  out[5] = (float)(some && cen > 0.0 ? cov / cen : qnan);
}

// W adjacent values of one plane: one store of 16 bytes (two for float64) where a unit is four points.  The types promise only the
// alignment of an element; row % 4 == 0 and c % 4 == 0 make the address as aligned as the plane's base
typedef double f64x2u __attribute__((ext_vector_type(2), aligned(8)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));

template <int W>
__device__ __forceinline__ void put(double* o, const double (&v)[W]) {
  if constexpr (W == 4) {
    const f64x2u a = {v[0], v[1]}, b = {v[2], v[3]};
    *reinterpret_cast<f64x2u*>(o) = a;
    *reinterpret_cast<f64x2u*>(o + 2) = b;
  } else {
    o[0] = v[0];
  }
}
template <int W>
__device__ __forceinline__ void put(float* o, const float (&v)[W]) {
  if constexpr (W == 4) {
    const f32x4u a = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4u*>(o) = a;
  } else {
    o[0] = v[0];
  }
}
template <int W>
__device__ __forceinline__ void put(int* o, const int (&v)[W]) {
  if constexpr (W == 4) {
    const i32x4u a = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<i32x4u*>(o) = a;
  } else {
    o[0] = v[0];
  }
}

// the planes of points c .. c + W - 1 of lead f: whichever of the three outputs exist
template <int W>
__device__ __forceinline__ void map_store(const double (&v)[MAP_SUMS][W], long long f, long long row, long long c, double* sums,
                                          float* scores, int* counts) {
  if (sums) {
    double* o = sums + f * MAP_SUMS * row + c;
#pragma unroll
    for (int j = 0; j < MAP_SUMS; ++j) put<W>(o + j * row, v[j]);
  }
  if (scores) {
    float r[MAP_SCORES][W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      double p[MAP_SUMS];
      float q[MAP_SCORES];
#pragma unroll
      for (int j = 0; j < MAP_SUMS; ++j) p[j] = v[j][k];
      map_scores(p, q);
#pragma unroll
      for (int j = 0; j < MAP_SCORES; ++j) r[j][k] = q[j];
    }
    float* o = scores + f * MAP_SCORES * row + c;
#pragma unroll
    for (int j = 0; j < MAP_SCORES; ++j) put<W>(o + j * row, r[j]);
  }
  if (counts) {
    int n[W];
#pragma unroll
    for (int k = 0; k < W; ++k) n[k] = (int)v[MAP_SUMS - 1][k];      // at most 2^31 - 1 samples
    put<W>(counts + f * row + c, n);
  }
}

// stage 1.  A block owns (lead f, chunk k of its samples, column tile): samples [cnt_f k / split, cnt_f (k + 1) / split), 256 threads x
// (VEC: four adjacent points, one 16-byte load per operand and sample; else one point).  U samples are in flight per thread and are
// added in sample order; the sample index and the label are the same in every lane (scalar loads), and the labels of the NEXT U
// samples are fetched while the data of these are in flight, because the table address needs them.  A sample past the chunk's end
// re-reads the chunk's last row and is not counted; a label out of range reads table row 0 and is not counted.  Leads without pairs
// run an empty loop and store zeros (and NaN scores): no launch depends on how many leads are active.
template <bool VEC, bool CLIMO, int U>
__global__ __launch_bounds__(MAP_THREADS, 2) void skill_map_kernel(MapArgs p) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned cell = blockIdx.x / (unsigned)p.tiles;
  const unsigned tile = blockIdx.x - cell * (unsigned)p.tiles;
  const unsigned f = cell / (unsigned)p.split, chunk = cell - f * (unsigned)p.split;
  const long long c = ((long long)tile * MAP_THREADS + threadIdx.x) * W;
  if (c >= p.row) return;
  long long cnt = window_pairs(p.count0, p.count_dec, f);
  if (cnt < 0) cnt = 0;
  const long long lo = cnt * chunk / p.split, end = cnt * (chunk + 1) / p.split;
  const float* pf = p.fc.lead(f) + c;
  const float* po = p.ob.lead(f) + c;
  const float* pc = CLIMO ? p.climo + c : nullptr;
  const int* pl = CLIMO && p.labels ? p.labels + (long long)f * p.lab_ls + (long long)f * p.lab_shift : nullptr;
  double s[MAP_SUMS - 1][W];
  unsigned n[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    n[k] = 0;
#pragma unroll
    for (int j = 0; j < MAP_SUMS - 1; ++j) s[j][k] = 0.0;
  }
  int label[U];
#pragma unroll
  for (int u = 0; u < U; ++u) label[u] = pl && lo + u < end ? pl[lo + u] : 0;
  for (long long i = lo; i < end; i += U) {
    float x[U][W], y[U][W], t[U][W];
    bool use[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = i + u < end;
      const long long r = live ? i + u : end - 1;      // lo <= r < end: a row of this chunk
      const bool in = !CLIMO || (unsigned)label[u] < (unsigned)p.n_labels;      // a label out of range is never an address
      use[u] = live && in;
      const float* qf = pf + r * p.fc.ss;
      const float* qo = po + r * p.ob.ss;
      const float* qc = CLIMO ? pc + (long long)(in ? label[u] : 0) * p.row : nullptr;
      if (VEC) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(qf);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(qo);
        f32x4 tv = {0.f, 0.f, 0.f, 0.f};
        if (CLIMO) tv = *reinterpret_cast<const f32x4*>(qc);
#pragma unroll
        for (int k = 0; k < W; ++k) x[u][k] = xv[k], y[u][k] = yv[k], t[u][k] = tv[k];
      } else {
        x[u][0] = qf[0], y[u][0] = qo[0];
        t[u][0] = CLIMO ? qc[0] : 0.f;
      }
    }
    int next[U];
#pragma unroll
    for (int u = 0; u < U; ++u) next[u] = pl && i + U + u < end ? pl[i + U + u] : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float df = x[u][k] - y[u][k];
        const float faf = CLIMO ? x[u][k] - t[u][k] : x[u][k];
        const float oaf = CLIMO ? y[u][k] - t[u][k] : y[u][k];
        const bool ok = use[u] && df == df && faf == faf && oaf == oaf;
        // zeroed in float32 (one select per value), then widened; products of two floats are exact in float64
        const double d = (double)(ok ? df : 0.f), fa = (double)(ok ? faf : 0.f), oa = (double)(ok ? oaf : 0.f);
        n[k] += ok ? 1u : 0u;
        s[0][k] += d;
        s[1][k] = fma(d, d, s[1][k]);
        s[2][k] += fabs(d);
        s[3][k] += fa;
        s[4][k] += oa;
        s[5][k] = fma(fa, oa, s[5][k]);
        s[6][k] = fma(fa, fa, s[6][k]);
        s[7][k] = fma(oa, oa, s[7][k]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) label[u] = next[u];
  }
  double v[MAP_SUMS][W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
#pragma unroll
    for (int j = 0; j < MAP_SUMS - 1; ++j) v[j][k] = s[j][k];
    v[MAP_SUMS - 1][k] = (double)n[k];
  }
  if (p.partial) {
    double* o = p.partial + ((long long)cell * MAP_SUMS) * p.row + c;
#pragma unroll
    for (int j = 0; j < MAP_SUMS; ++j) put<W>(o + j * p.row, v[j]);
  } else {
    map_store<W>(v, f, p.row, c, p.sums, p.scores, p.counts);
  }
}

// stage 2 (and dlwp_verify_skill_map_finish with split = 1 on a finished table): one thread per (lead, point) adds the planes of the
// chunks in chunk order and stores what map_store stores
__global__ __launch_bounds__(MAP_THREADS) void skill_map_final_kernel(const double* __restrict__ partial, int split, int tiles,
                                                                      long long row, double* sums, float* scores, int* counts) {
  const unsigned f = blockIdx.x / (unsigned)tiles;
  const long long c = (long long)(blockIdx.x - f * (unsigned)tiles) * MAP_THREADS + threadIdx.x;
  if (c >= row) return;
  double v[MAP_SUMS][1];
#pragma unroll
  for (int j = 0; j < MAP_SUMS; ++j) v[j][0] = 0.0;
  for (int k = 0; k < split; ++k) {
    const double* src = partial + (((long long)f * split + k) * MAP_SUMS) * row + c;
#pragma unroll
    for (int j = 0; j < MAP_SUMS; ++j) v[j][0] += src[j * row];
  }
  map_store<1>(v, f, row, c, sums, scores, counts);
}

inline long long map_tiles(long long row, bool vec) { return ((vec ? row / 4 : row) + MAP_THREADS - 1) / MAP_THREADS; }

// chunks of the sample axis.  split = 0: only as many as leads x column tiles leave the chip unfilled; a positive split as given;
// never more chunks than lead 0 has samples, never fewer than one
inline int map_split(dlwp_handle_t h, int leads, int count0, long long row, int split, bool vec) {
  long long want = split;
  if (split == 0) {
    want = cell_bpc_cap(h, (long long)leads * map_tiles(row, vec), MAP_BLOCKS_PER_CU);
  }
  if (want > count0) want = count0;
  return (int)(want < 1 ? 1 : want);
}

inline size_t map_ws_bytes(int leads, int split, long long row) {
  return split > 1 ? (size_t)leads * (size_t)split * MAP_SUMS * (size_t)row * sizeof(double) : 0;
}

template <bool VEC, bool CLIMO, int U>
void map_launch(const MapArgs& p, unsigned grid, hipStream_t s) {
  skill_map_kernel<VEC, CLIMO, U><<<grid, MAP_THREADS, 0, s>>>(p);
}

}  // namespace

extern "C" {

size_t dlwp_verify_skill_map_workspace(dlwp_handle_t h, int leads, int count0, long long row, int split) {
  if (leads < 1 || row < 1 || split < 0) return 0;
  // the 16-byte route has the fewer tiles and therefore the larger automatic split: enough for either route
  return map_ws_bytes(leads, map_split(h, leads, count0, row, split, mult4(row)), row);
}

int dlwp_verify_skill_map(dlwp_handle_t h, const void* fc, long long fc_lead_stride, long long fc_sample_stride, int fc_shift,
                          const void* ob, long long ob_lead_stride, long long ob_sample_stride, int ob_shift, int leads, int count0,
                          int count_dec, long long row, const void* climo, int n_labels, const void* labels,
                          long long label_lead_stride, int label_shift, int split, void* sums, void* scores, void* counts, void* ws,
                          size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_skill_map);
  DLWP_CHECK_ARG(leads >= 1 && row >= 1, "dlwp_verify_skill_map: leads %d and row %lld must be >= 1", leads, row);
  MapArgs p;
  p.fc = window_of(fc, fc_lead_stride, fc_sample_stride, fc_shift);
  p.ob = window_of(ob, ob_lead_stride, ob_sample_stride, ob_shift);
  DLWP_CHECK_ARG(count_dec >= 0 && window_nonneg(p.fc) && window_nonneg(p.ob) && label_lead_stride >= 0 && label_shift >= 0,
                 "dlwp_verify_skill_map: negative stride, shift or count_dec");
  DLWP_CHECK_ARG(!climo || (n_labels >= 1 && n_labels <= MAP_MAX_LABELS), "dlwp_verify_skill_map: n_labels %d, expected 1 .. %d",
                 n_labels, MAP_MAX_LABELS);
  DLWP_CHECK_ARG(climo || !labels, "dlwp_verify_skill_map: labels without a climatology table");
  DLWP_CHECK_ARG(fc && ob && (sums || scores || counts), "dlwp_verify_skill_map: null operand, or no output at all");
  DLWP_CHECK_ARG(split >= 0, "dlwp_verify_skill_map: split %d must be >= 0", split);
  const bool vec = mult4(row) && window_vec(p.fc) && window_vec(p.ob) && aligned16(climo);
  const int chunks = map_split(h, leads, count0, row, split, vec);
  const long long tiles = map_tiles(row, vec), ftiles = map_tiles(row, false);
  DLWP_CHECK_ARG((long long)leads * chunks * tiles < (1ll << 31) && (long long)leads * ftiles < (1ll << 31),
                 "dlwp_verify_skill_map: row %lld too long for %d leads in %d chunks", row, leads, chunks);
  const size_t ws_need = map_ws_bytes(leads, chunks, row);
  DLWP_CHECK_ARG(ws_bytes >= ws_need && (ws || ws_need == 0), "dlwp_verify_skill_map: workspace too small (%zu < %zu)", ws_bytes,
                 ws_need);
  DLWP_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dlwp_verify_skill_map: workspace must be 8-byte aligned");
  DLWP_CHECK_ARG(h, "dlwp_verify_skill_map: null handle");
  hipStream_t s = (hipStream_t)stream;
  p.climo = (const float*)climo, p.labels = (const int*)labels;
  p.lab_ls = label_lead_stride;
  p.lab_shift = label_shift;
  p.count0 = count0, p.count_dec = count_dec;
  p.n_labels = climo ? n_labels : 1, p.split = chunks, p.tiles = (int)tiles;
  p.row = row;
  p.partial = chunks > 1 ? (double*)ws : nullptr;
  p.sums = (double*)sums, p.scores = (float*)scores, p.counts = (int*)counts;
  const unsigned grid = (unsigned)((long long)leads * chunks * tiles);
  // samples in flight per thread: what 128 registers hold beside the 32 float64 sums of a 16-byte unit
  if (climo) {
    if (vec)
      map_launch<true, true, 2>(p, grid, s);
    else
      map_launch<false, true, 4>(p, grid, s);
  } else {
    if (vec)
      map_launch<true, false, 4>(p, grid, s);
    else
      map_launch<false, false, 4>(p, grid, s);
  }
  if (chunks > 1)
    skill_map_final_kernel<<<(unsigned)(leads * ftiles), MAP_THREADS, 0, s>>>((const double*)ws, chunks, (int)ftiles, row, (double*)sums,
                                                                              (float*)scores, (int*)counts);
  DLWP_LAUNCH_CHECK("verify_skill_map kernels");
  return DLWP_OK;
}

int dlwp_verify_skill_map_finish(dlwp_handle_t h, const void* sums, long long cells, void* scores, void* counts, void* stream) {
  DLWP_UNTAPED(dlwp_verify_skill_map_finish);
  DLWP_CHECK_ARG(cells >= 1, "dlwp_verify_skill_map_finish: cells %lld must be >= 1", cells);
  DLWP_CHECK_ARG(sums && (scores || counts), "dlwp_verify_skill_map_finish: null table, or no output at all");
  const long long tiles = map_tiles(cells, false);
  DLWP_CHECK_ARG(tiles < (1ll << 31), "dlwp_verify_skill_map_finish: %lld cells too long for one grid", cells);
  DLWP_CHECK_ARG(h, "dlwp_verify_skill_map_finish: null handle");
  skill_map_final_kernel<<<(unsigned)tiles, MAP_THREADS, 0, (hipStream_t)stream>>>((const double*)sums, 1, (int)tiles, cells, nullptr,
                                                                                  (float*)scores, (int*)counts);
  DLWP_LAUNCH_CHECK("verify_skill_map_finish kernel");
  return DLWP_OK;
}

}  // extern "C"
