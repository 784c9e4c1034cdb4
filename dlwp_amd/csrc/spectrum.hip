// spectrum.hip -- zonal power spectra of a forecast and its verification where the series is (gfx950): per lead and group the sums
// behind the power of the truth, the power of the error, and their cross spectrum at every zonal wavenumber.
//
// dlwp_verify_spectrum_sums addresses its operands exactly as dlwp_verify_skill_sums does (include/dlwp_hip.h) and reads a group's run
// as longitude rows of `width` floats.  Per row it transforms ob and d = fc - ob (rounded once in float32): a real DFT of length
// width, done as a product of 32 rows against a twiddle matrix on v_mfma_f32_32x32x2_f32 (exact float32, a j-ordered fmaf chain).
//   * the row's mean comes out first: y_j = fl32(x_j - m), m = fl32(float64 row sum / width); wavenumber 0 is taken from the float64
//     row sum itself, so a field with a large mean keeps its small scales;
//   * the real input is folded: e_j = y_j + y_{W-j} meets the cosines, o_j = y_j - y_{W-j} the sines, j <= W / 2, in place in LDS
//     (e_j where y_j was, o_j where y_{W-j} was): K = W / 2 + 1 products per coefficient and part, padded to an even number with zeros;
//   * the twiddles are gathered per step from ONE table of W cosines and W sines in LDS by the running index (j k) mod W; the table is
//     made on the host in float64 and rounded once.  One kernel serves every 4 <= W <= 512 of either parity.
// A wave owns 32-wavenumber tiles (mw, mw + nw, ...) of the block's 32 rows and keeps the four products (O cos, O sin, D cos,
// D sin) of a tile in 64 accumulator registers; behind the product everything is float64 and stays in registers: re, im widened, the
// four terms weighted and added over the lane's 16 rows into per-thread sums that live across the block's row tiles.  One partial
// (4 K + 2 doubles) per block in ws; a second launch adds a cell's partials in index order (the window, the plan and the lane tree are
// verify_common.h's; the partial's length varies with the width, so the cell stage is this file's own).  No atomics, no
// synchronisation with the host, identical bits on repeated calls.  A row with a non-finite fc, ob or d is zeroed in LDS and has weight 0 and no count.
#include "verify_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int SPEC_ROWS = 32;             // longitude rows of a tile: M of the matrix instruction
constexpr int SPEC_MAX_WIDTH = 512;
constexpr int SPEC_MIN_WIDTH = 4;
constexpr int SPEC_BLOCKS_PER_CU = 8;
constexpr int SPEC_TPW = 3;               // wavenumber tiles a wave may own: ceil(9 / 3) at width 512
constexpr int SPEC_FINAL_THREADS = 256;
constexpr int SPEC_THREADS = 256;         // four waves stage a tile; nw of them own wavenumber tiles
constexpr int SPEC_BATCH = 8;             // units a thread has in flight in stage 1

struct SpecArgs {
  Window fc, ob;
  const float* weights;                  // w_len floats or null
  const float* tw;                       // width cosines, then width sines
  long long run;                         // floats of one group in one sample row
  int count0, count_dec;
  int groups, bpc;                       // blocks per (lead, group) cell
  int width, rpr;                        // W; longitude rows of a run
  int w_len;
  int K, pitch, nT, nw;                  // wavenumbers; floats of a row in LDS; 32-wavenumber tiles; waves that own tiles
};

// the LDS of a block: doubles in front
struct SpecLds {
  double* wl;          // [32] weight of a row of the tile; 0 for a row past the end or skipped
  double* rso;         // [32] float64 row sums of ob
  double* rsd;         // [32] and of d
  long long* off_f;    // [32] element offset of the row in fc
  long long* off_o;    // [32] and in ob
  int* okf;            // [32] the row exists (stage 0), and is finite (stage 2)
  float* tw;           // [2 W]
  float* buf_o;        // [32][pitch]
  float* buf_d;        // [32][pitch]
};

inline size_t spec_lds_bytes(int width, int pitch) {
  return (size_t)SPEC_ROWS * (3 * 8 + 2 * 8 + 4) + (size_t)2 * width * 4 + (size_t)2 * SPEC_ROWS * pitch * 4;
}

// Stage 0 .. 3 per row tile; see the head of the file.  Four waves; wave (mw = (wave + block) % 4) < nw owns wavenumber tiles mw,
// mw + nw, ...: with three owners (widths 180 and 360) the wave that only stages is a different one from block to block
template <bool VEC>
__global__ __launch_bounds__(SPEC_THREADS, 2) void spectrum_partial_kernel(SpecArgs p, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char spec_lds_raw[];
  SpecLds L;
  L.wl = reinterpret_cast<double*>(spec_lds_raw);
  L.rso = L.wl + SPEC_ROWS;
  L.rsd = L.rso + SPEC_ROWS;
  L.off_f = reinterpret_cast<long long*>(L.rsd + SPEC_ROWS);
  L.off_o = L.off_f + SPEC_ROWS;
  L.okf = reinterpret_cast<int*>(L.off_o + SPEC_ROWS);
  L.tw = reinterpret_cast<float*>(L.okf + SPEC_ROWS);
  L.buf_o = L.tw + 2 * p.width;
  L.buf_d = L.buf_o + SPEC_ROWS * p.pitch;

  const int W = p.width, K = p.K, pitch = p.pitch;
  const int T = (int)blockDim.x, t = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int mw = __builtin_amdgcn_readfirstlane((wave + (int)blockIdx.x) & 3);
  const int lane = t & 63, h = lane >> 5, c = lane & 31;
  const unsigned cell = blockIdx.x / (unsigned)p.bpc;
  const unsigned blk = blockIdx.x - cell * (unsigned)p.bpc;
  const unsigned f = cell / (unsigned)p.groups, g = cell - f * (unsigned)p.groups;
  const unsigned cnt = (unsigned)window_pairs(p.count0, p.count_dec, f);      // > 0: the host launches active leads only
  const unsigned rows_total = cnt * (unsigned)p.rpr;                                     // < 2^31: checked by the host
  const unsigned n_tiles = (rows_total + SPEC_ROWS - 1) / SPEC_ROWS;
  const float* pf = p.fc.lead(f, g, p.run);
  const float* po = p.ob.lead(f, g, p.run);

  for (int i = t; i < 2 * W; i += T) L.tw[i] = p.tw[i];

  double acc[SPEC_TPW][4];               // per thread: wavenumber 32 * tile + c over this lane's rows of every tile of the block
#pragma unroll
  for (int tt = 0; tt < SPEC_TPW; ++tt)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[tt][q] = 0.0;
  double sw = 0.0;                       // threads 0 .. 31: sum of weights and rows counted of row t of every tile
  unsigned long long nrows = 0;

  const int ns = (K + 1) >> 1;           // matrix steps: two j each
  constexpr int U = VEC ? 4 : 1;
  const int upr = W / U;                 // units of a row
  const int units = SPEC_ROWS * upr;

  for (unsigned tile = blk; tile < n_tiles; tile += (unsigned)p.bpc) {
    // stage 0: where the rows of the tile are, and their weights
    if (t < SPEC_ROWS) {
      const unsigned R = tile * SPEC_ROWS + (unsigned)t;
      const bool valid = R < rows_total;
      const unsigned i = valid ? R / (unsigned)p.rpr : 0u;
      const unsigned r = valid ? R - i * (unsigned)p.rpr : 0u;
      L.off_f[t] = (long long)i * p.fc.ss + (long long)r * W;
      L.off_o[t] = (long long)i * p.ob.ss + (long long)r * W;
      L.okf[t] = valid ? 1 : 0;
      L.wl[t] = valid ? (p.weights ? (double)p.weights[r % (unsigned)p.w_len] : 1.0) : 0.0;
    }
    __syncthreads();
    // stage 1: ob and d = fc - ob of the tile into LDS, coalesced over the tile (its rows are adjacent inside a sample row).  The loads
    // of eight units are issued before the first is stored: one trip to memory per eight, not eight.  A unit of a row that does not
    // exist loads the cell's first element (it exists: the lead has pairs) and stores zeros
    {
      int row = t / upr, col = t - row * upr;
      const int srow = T / upr, scol = T - srow * upr;
      for (int base = 0; base < units; base += SPEC_BATCH * T) {
        float x[SPEC_BATCH][U], y[SPEC_BATCH][U];
        int at[SPEC_BATCH];              // where the unit goes in a buffer; -1: past the end of the tile
#pragma unroll
        for (int i = 0; i < SPEC_BATCH; ++i) {
          const bool in = base + i * T + t < units;
          const int rr = in ? row : 0;
          const bool ld = in && L.okf[rr] != 0;
          const long long of = ld ? L.off_f[rr] + U * col : 0, oo = ld ? L.off_o[rr] + U * col : 0;
          at[i] = in ? row * pitch + U * col : -1;
          if (VEC) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(pf + of);
            const f32x4 yv = *reinterpret_cast<const f32x4*>(po + oo);
#pragma unroll
            for (int k = 0; k < U; ++k) x[i][k] = ld ? xv[k] : 0.f, y[i][k] = ld ? yv[k] : 0.f;
          } else {
            x[i][0] = ld ? pf[of] : 0.f, y[i][0] = ld ? po[oo] : 0.f;
          }
          row += srow, col += scol;
          if (col >= upr) col -= upr, ++row;
        }
#pragma unroll
        for (int i = 0; i < SPEC_BATCH; ++i) {
          if (at[i] >= 0) {
#pragma unroll
            for (int k = 0; k < U; ++k) {
              L.buf_o[at[i] + k] = y[i][k];
              L.buf_d[at[i] + k] = x[i][k] - y[i][k];
            }
          }
        }
      }
    }
    __syncthreads();
    // stage 2: eight lanes per row.  Float64 row sums, the finite test (a non-finite fc makes d non-finite), the mean out, the fold
    // in place.  The fold's stores depend on the mean, and the mean on every load of the row: no store overtakes a load
    for (int row = wave * 8 + (lane >> 3); row < SPEC_ROWS; row += (T >> 6) * 8) {
      const int sub = lane & 7;
      float* bo = L.buf_o + row * pitch;
      float* bd = L.buf_d + row * pitch;
      double so = 0.0, sd = 0.0;
      int bad = 0;
#pragma unroll 4
      for (int j = sub; j < W; j += 8) {
        const float a = bo[j], b = bd[j];
        bad |= (__builtin_isfinite(a) && __builtin_isfinite(b)) ? 0 : 1;
        so += (double)a, sd += (double)b;
      }
#pragma unroll
      for (int m = 1; m < 8; m <<= 1) {
        so += __shfl_xor(so, m, 64), sd += __shfl_xor(sd, m, 64);
        bad |= __shfl_xor(bad, m, 64);
      }
      const bool ok = L.okf[row] != 0 && bad == 0;
      if (ok) {
        const float mo = (float)(so / (double)W), md = (float)(sd / (double)W);
        const int half = (W - 1) >> 1;
        for (int j = 1 + sub; j <= half; j += 8) {
          const float a = bo[j] - mo, b = bo[W - j] - mo;
          bo[j] = a + b, bo[W - j] = a - b;
          const float a2 = bd[j] - md, b2 = bd[W - j] - md;
          bd[j] = a2 + b2, bd[W - j] = a2 - b2;
        }
        if (sub == 0) bo[0] -= mo, bd[0] -= md;
        if (sub == 1 && (W & 1) == 0) bo[W >> 1] -= mo, bd[W >> 1] -= md;
      } else {
        for (int j = sub; j < W; j += 8) bo[j] = 0.f, bd[j] = 0.f;
      }
      if (sub == 0) {
        L.rso[row] = ok ? so : 0.0;
        L.rsd[row] = ok ? sd : 0.0;
        if (!ok) L.wl[row] = 0.0, L.okf[row] = 0;
      }
    }
    __syncthreads();
    if (t < SPEC_ROWS) {
      sw += L.wl[t];
      nrows += (unsigned long long)L.okf[t];
    }
    // stage 3: the products of this wave's wavenumber tiles, and the float64 sums behind them
#pragma unroll
    for (int tt = 0; tt < SPEC_TPW; ++tt) {
      const int wt = mw + tt * p.nw;
      if (mw < p.nw && wt < p.nT) {
        const int kw = 32 * wt + c;
        const unsigned kwc = kw < K ? (unsigned)kw : 0u;      // columns past K are computed on wavenumber 0 and never stored
        const unsigned step = (2u * kwc) % (unsigned)W;
        unsigned idx = ((unsigned)h * kwc) % (unsigned)W;     // (j k) mod W of this lane's j = 2 s + h
        f32x16 a_oc, a_os, a_dc, a_ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) a_oc[r] = 0.f, a_os[r] = 0.f, a_dc[r] = 0.f, a_ds[r] = 0.f;
        const float* ro = L.buf_o + c * pitch;
        const float* rd = L.buf_d + c * pitch;

        // the operands of step s + 1 are fetched in front of the products of step s (the last step fetches its own again)
        float cb = L.tw[idx], sb = L.tw[W + idx];
        // lane half 0 reads index W here (j = 0): the pad column, never written -- whatever it holds, the select on j > 0 drops it
        float eo = ro[h], oo = ro[W - h], ed = rd[h], od = rd[W - h];
        for (int s = 0; s < ns; ++s) {
          const int j = 2 * s + h;
          const bool je = j < K, jo = j > 0 && 2 * j < W;     // e_j exists for j <= W / 2; o_0 and o_{W/2} are zero
          if (s + 1 < ns) {
            idx += step;
            if (idx >= (unsigned)W) idx -= (unsigned)W;
          }
          const int jn = s + 1 < ns ? j + 2 : j;
          const float n_cb = L.tw[idx], n_sb = L.tw[W + idx];
          const float n_eo = ro[jn], n_oo = ro[W - jn], n_ed = rd[jn], n_od = rd[W - jn];
          a_oc = __builtin_amdgcn_mfma_f32_32x32x2f32(je ? eo : 0.f, cb, a_oc, 0, 0, 0);
          a_os = __builtin_amdgcn_mfma_f32_32x32x2f32(jo ? oo : 0.f, sb, a_os, 0, 0, 0);
          a_dc = __builtin_amdgcn_mfma_f32_32x32x2f32(je ? ed : 0.f, cb, a_dc, 0, 0, 0);
          a_ds = __builtin_amdgcn_mfma_f32_32x32x2f32(jo ? od : 0.f, sb, a_ds, 0, 0, 0);
          cb = n_cb, sb = n_sb, eo = n_eo, oo = n_oo, ed = n_ed, od = n_od;
        }
        // lane (c, h) holds wavenumber kw of rows (r & 3) + 8 (r >> 2) + 4 h.  X = re - i * (sine sum)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          const double w = L.wl[row];
          double o_re = (double)a_oc[r], o_im = -(double)a_os[r], d_re = (double)a_dc[r], d_im = -(double)a_ds[r];
          if (kw == 0) o_re = L.rso[row], o_im = 0.0, d_re = L.rsd[row], d_im = 0.0;
          s0 = fma(w, o_re * o_re + o_im * o_im, s0);
          s1 = fma(w, d_re * d_re + d_im * d_im, s1);
          s2 = fma(w, d_re * o_re + d_im * o_im, s2);
          s3 = fma(w, d_im * o_re - d_re * o_im, s3);
        }
        acc[tt][0] += s0, acc[tt][1] += s1, acc[tt][2] += s2, acc[tt][3] += s3;
      }
    }
    __syncthreads();
  }

  // the block's partial: [4][K] sums with the one-sided Parseval factor c_k / W^2, then (sum w, rows counted)
  double* out = partial + (long long)(4 * K + 2) * blockIdx.x;
#pragma unroll
  for (int tt = 0; tt < SPEC_TPW; ++tt) {
    const int wt = mw + tt * p.nw;
    if (mw < p.nw && wt < p.nT) {
      const int kw = 32 * wt + c;
      const double scale = ((kw == 0 || 2 * kw == W) ? 1.0 : 2.0) / ((double)W * (double)W);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double v = acc[tt][q];
        v += __shfl_down(v, 32, 64);     // the two row halves of a wavenumber
        if (h == 0 && kw < K) out[q * K + kw] = v * scale;
      }
    }
  }
  if (wave == 0) {
    const double a = wave_sum_f64(sw), b = wave_sum_f64((double)nrows);
    if (lane == 0) out[4 * K] = a, out[4 * K + 1] = b;
  }
}

// stage 2: one block per cell.  Thread e adds entry e of the cell's partials in index order.  Cells of leads without pairs (cell >=
// active_cells) read nothing and store zeros.
__global__ __launch_bounds__(SPEC_FINAL_THREADS) void spectrum_final_kernel(const double* __restrict__ partial, int bpc, int active_cells,
                                                                            int K, double* __restrict__ sums, double* __restrict__ norm) {
  const int cell = blockIdx.x;
  const int P = 4 * K + 2;
  for (int e = threadIdx.x; e < P; e += SPEC_FINAL_THREADS) {
    double v = 0.0;
    if (cell < active_cells) {
      const double* src = partial + (long long)P * cell * bpc + e;
      for (int i = 0; i < bpc; ++i) v += src[(long long)P * i];
    }
    if (e < 4 * K)
      sums[(long long)4 * K * cell + e] = v;
    else
      norm[2ll * cell + (e - 4 * K)] = v;
  }
}

}  // namespace

extern "C" {

size_t dlwp_verify_spectrum_workspace(dlwp_handle_t h, int leads, int groups, int width) {
  if (leads < 1 || groups < 1 || width < SPEC_MIN_WIDTH || width > SPEC_MAX_WIDTH) return 0;
  return cell_workspace_bytes(h, (long long)leads * groups, SPEC_BLOCKS_PER_CU, (size_t)(4 * (width / 2 + 1) + 2) * sizeof(double));
}

int dlwp_verify_spectrum_sums(dlwp_handle_t h, const void* fc, long long fc_lead_stride, long long fc_sample_stride, int fc_shift,
                              const void* ob, long long ob_lead_stride, long long ob_sample_stride, int ob_shift, int leads, int count0,
                              int count_dec, int groups, long long run, int width, const void* weights, int w_len,
                              const void* twiddles, void* sums, void* norm, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_spectrum_sums);
  DLWP_CHECK_ARG(leads >= 1 && groups >= 1 && run >= 1, "dlwp_verify_spectrum_sums: leads %d, groups %d, run %lld must all be >= 1",
                 leads, groups, run);
  SpecArgs p;
  p.fc = window_of(fc, fc_lead_stride, fc_sample_stride, fc_shift);
  p.ob = window_of(ob, ob_lead_stride, ob_sample_stride, ob_shift);
  DLWP_CHECK_ARG(count_dec >= 0 && window_nonneg(p.fc) && window_nonneg(p.ob),
                 "dlwp_verify_spectrum_sums: negative stride, shift or count_dec");
  DLWP_CHECK_ARG(width >= SPEC_MIN_WIDTH && width <= SPEC_MAX_WIDTH && run % width == 0,
                 "dlwp_verify_spectrum_sums: width %d must lie in %d .. %d and divide a run of %lld", width, SPEC_MIN_WIDTH,
                 SPEC_MAX_WIDTH, run);
  const long long rpr = run / width;
  DLWP_CHECK_ARG(!weights || (w_len >= 1 && w_len <= rpr && rpr % w_len == 0),
                 "dlwp_verify_spectrum_sums: %d weights do not divide the %lld longitude rows of a run", w_len, rpr);
  DLWP_CHECK_ARG(fc && ob && sums && norm && twiddles, "dlwp_verify_spectrum_sums: null pointer");
  const long long cells = (long long)leads * groups;
  // inherited: at most 2^20 cells here and in skill.hip, fewer than 2^20 in verify.hip
  DLWP_CHECK_ARG(cells <= (1ll << 20), "dlwp_verify_spectrum_sums: %lld (lead, group) cells, at most 2^20", cells);
  DLWP_CHECK_ARG(count0 <= 0 || (long long)count0 * rpr < (1ll << 31) - SPEC_ROWS,
                 "dlwp_verify_spectrum_sums: %lld longitude rows in a cell, fewer than 2^31 expected", (long long)count0 * rpr);
  const long long active = window_active_leads(leads, count0, count_dec);
  const int K = width / 2 + 1;
  // no more blocks in a cell than lead 0 (the longest) has row tiles
  const int bpc = cell_plan_bpc(h, active, groups, ((long long)count0 * rpr + SPEC_ROWS - 1) / SPEC_ROWS, SPEC_BLOCKS_PER_CU);
  const size_t ws_need = (size_t)active * groups * bpc * (size_t)(4 * K + 2) * sizeof(double);
  // inherited: a null workspace is accepted where no partial is written (verify.hip wants one regardless)
  DLWP_CHECK_ARG(ws_bytes >= ws_need && (ws || ws_need == 0), "dlwp_verify_spectrum_sums: workspace too small (%zu < %zu)", ws_bytes,
                 ws_need);
  DLWP_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dlwp_verify_spectrum_sums: workspace must be 8-byte aligned");
  DLWP_CHECK_ARG(h, "dlwp_verify_spectrum_sums: null handle");
  hipStream_t s = (hipStream_t)stream;
  if (active > 0) {
    p.weights = (const float*)weights, p.tw = (const float*)twiddles;
    p.run = run;
    p.count0 = count0, p.count_dec = count_dec;
    p.groups = groups, p.bpc = bpc;
    p.width = width, p.rpr = (int)rpr;
    p.w_len = weights ? w_len : 1;
    p.K = K;
    p.pitch = (width + 1) | 1;           // odd: the 32 rows of an A operand sit on 32 banks; index W exists
    p.nT = (K + 31) / 32;                // 1 .. 9
    const int per = (p.nT + 3) / 4;      // tiles per wave with at most four waves: 1 .. 3
    p.nw = (p.nT + per - 1) / per;       // waves that own tiles: 3 at width 180 (3 tiles) and 360 (6 tiles)
    const size_t lds = spec_lds_bytes(width, p.pitch);
    const bool vec = mult4(width) && window_vec(p.fc) && window_vec(p.ob);
    const void* kern = vec ? (const void*)spectrum_partial_kernel<true> : (const void*)spectrum_partial_kernel<false>;
    // the largest image (width 512) is allowed once per instance and device; every width's image fits below it
    static unsigned lds_allowed[2];      // per instance: a bit per device.  Setting the attribute twice is harmless, so no lock
    const unsigned dev_bit = 1u << (h->device & 31);
    if (!(lds_allowed[vec ? 1 : 0] & dev_bit)) {
      const size_t lds_max = spec_lds_bytes(SPEC_MAX_WIDTH, (SPEC_MAX_WIDTH + 1) | 1);
      const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
      if (e != hipSuccess) DLWP_FAIL(DLWP_EHIP, "dlwp_verify_spectrum_sums: hipFuncSetAttribute failed (%d)", (int)e);
      lds_allowed[vec ? 1 : 0] |= dev_bit;
    }
    const unsigned grid = (unsigned)(active * groups * bpc);      // <= max(cells, 8 blocks per CU)
    if (vec)
      spectrum_partial_kernel<true><<<grid, SPEC_THREADS, lds, s>>>(p, (double*)ws);
    else
      spectrum_partial_kernel<false><<<grid, SPEC_THREADS, lds, s>>>(p, (double*)ws);
  }
  spectrum_final_kernel<<<(unsigned)cells, SPEC_FINAL_THREADS, 0, s>>>((const double*)ws, bpc, (int)(active * groups), K, (double*)sums,
                                                                       (double*)norm);
  DLWP_LAUNCH_CHECK("verify_spectrum_sums kernels");
  return DLWP_OK;
}

}  // extern "C"
