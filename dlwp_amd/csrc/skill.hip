// skill.hip -- latitude-weighted forecast skill where the series is (gfx950): one pass over a forecast and its verification yields,
// per lead and group, the ten sums behind the weighted rmse / mse / mae, the bias and the (uncentred and centred) anomaly correlation.
//
// dlwp_verify_skill_sums addresses its two operands exactly as dlwp_verify_error_sums does (csrc/verify.hip; the table in
// include/dlwp_hip.h) and adds what that kernel has no place for: a climatology c looked up per pair of sample rows in a table of at
// most 64 rows (the month-aware table of dlwp_verify_label_nanmean), a weight per latitude row, and the cross products.  Per pair
// d = fc - ob, fa = fc - c, oa = ob - c are rounded once in float32, as numpy rounds float32 operands; a pair with a NaN among them
// is skipped in every sum, the count included; everything behind that is float64.  The tree is verify_common.h's with one partial of
// ten doubles per block in ws: no size read from the device, no synchronisation, repeated calls give identical bits.
#include "verify_common.h"

namespace {

constexpr int SKILL_THREADS = 256;
constexpr int SKILL_BLOCKS_PER_CU = 8;
constexpr int SKILL_SUMS = 10;
constexpr int SKILL_MAX_LABELS = 64;

// how a unit finds its weight: none (all ones), one weight per unit (a scalar unit, or four floats that cannot straddle a latitude row:
// w_inner % 4 == 0), or one per element
enum { W_NONE = 0, W_UNIT = 1, W_ELEM = 2 };

struct SkillArgs {
  Window fc, ob;
  const float* climo;                    // (n_labels, groups * run) or null
  const int* labels;                     // may be null: label 0
  const float* weights;                  // w_len floats or null
  long long lab_ls;
  int lab_shift;
  int count0, count_dec;
  int groups, bpc;                       // blocks per (lead, group) cell
  int n_labels, w_len;
  long long run;                         // floats of one group in one sample row
  long long w_inner;
  long long step_row, step_col;          // bpc * 256 units as (rows, columns) of a cell
  long long step_wcol;                   // the same step inside the weight period w_len x w_inner, as (latitude rows, columns)
  int step_wrow;
};

struct SkillAcc {
  double s[SKILL_SUMS - 1];              // S0 .. S8
  unsigned long long n;
};

// one pair.  d, fa, oa were rounded in float32 by the caller; a NaN among them drops the pair from every sum.  The pair is zeroed in
// float32 (one select per value), then widened
template <bool WEIGHTED>
__device__ __forceinline__ void pair_add(float df, float faf, float oaf, float wf, SkillAcc& a, unsigned& counted) {
  const bool ok = df == df && faf == faf && oaf == oaf;
  const double d = (double)(ok ? df : 0.f), fa = (double)(ok ? faf : 0.f), oa = (double)(ok ? oaf : 0.f);
  counted += ok ? 1u : 0u;
  if (WEIGHTED) {
    const double w = (double)(ok ? wf : 0.f);
    const double wd = w * d, wfa = w * fa, woa = w * oa;
    a.s[0] += w;
    a.s[1] += wd;
    a.s[2] = fma(wd, d, a.s[2]);
    a.s[3] = fma(w, fabs(d), a.s[3]);
    a.s[4] += wfa;
    a.s[5] += woa;
    a.s[6] = fma(wfa, oa, a.s[6]);
    a.s[7] = fma(wfa, fa, a.s[7]);
    a.s[8] = fma(woa, oa, a.s[8]);
  } else {                               // w = 1: S0 is the count (filled in after the loop), products of two floats are exact
    a.s[1] += d;
    a.s[2] = fma(d, d, a.s[2]);
    a.s[3] += fabs(d);
    a.s[4] += fa;
    a.s[5] += oa;
    a.s[6] = fma(fa, oa, a.s[6]);
    a.s[7] = fma(fa, fa, a.s[7]);
    a.s[8] = fma(oa, oa, a.s[8]);
  }
}

// the weights of a unit whose first element sits at (wrow, wcol) of the weight period
template <bool VEC, int WMODE>
__device__ __forceinline__ void unit_weights(const SkillArgs& p, int wrow, long long wcol, float (&w)[VEC ? 4 : 1]) {
  constexpr int W = VEC ? 4 : 1;
  if (WMODE == W_NONE) {
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = 1.f;
  } else if (WMODE == W_UNIT) {
    const float v = p.weights[wrow];
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = v;
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      w[k] = p.weights[wrow];
      if (++wcol == p.w_inner) {
        wcol = 0;
        wrow = wrow + 1 == p.w_len ? 0 : wrow + 1;
      }
    }
  }
}

// stage 1.  Block blk of cell (lead f, group g) takes units blk * 256 + t, + bpc * 256, ... of the cell's count_f x units-per-row grid,
// as verify_partial_kernel does; a unit is four floats (VEC) or one.  Beside (row, col) a thread carries the element offset of its
// unit in either operand and the position of the unit's first element inside the weight period, (wrow, wcol) with wcol < w_inner and
// wrow < w_len; run is a multiple of the period, so the carry from col into row does not touch it, and the host's (step_wrow,
// step_wcol) advances it with two carries and no division.  The label of the NEXT unit is fetched while this one's data are in
// flight (the table address needs it), so no load waits for another.  Eight waves per SIMD (64 registers) keep the launch's eight
// blocks per CU resident.  The walk is this kernel's own and not verify_common.h's UnitWalk: its row is unsigned and clamped to cnt
// (the loop's only test) and the operand offsets are carried beside it; on UnitWalk the weighted 16-byte instances spill at 64.
template <bool VEC, int WMODE, bool CLIMO>
__global__ __launch_bounds__(SKILL_THREADS, SKILL_BLOCKS_PER_CU) void skill_partial_kernel(SkillArgs p, double* __restrict__ partial) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned cell = blockIdx.x / (unsigned)p.bpc;
  const unsigned blk = blockIdx.x - cell * (unsigned)p.bpc;
  const unsigned f = cell / (unsigned)p.groups, g = cell - f * (unsigned)p.groups;
  const unsigned cnt = (unsigned)window_pairs(p.count0, p.count_dec, f);      // > 0: the host launches active leads only
  const long long units = p.run / W;
  const unsigned step_row = (unsigned)p.step_row;     // <= bpc * 256 <= 8 CUs * 256
  const float* pf = p.fc.lead(f, g, p.run);
  const float* po = p.ob.lead(f, g, p.run);
  const float* pc = CLIMO ? p.climo + (long long)g * p.run : nullptr;
  const int* pl = CLIMO && p.labels ? p.labels + (long long)f * p.lab_ls + (long long)f * p.lab_shift : nullptr;
  const long long trow = (long long)p.groups * p.run;
  // a step moves an operand by step_row rows and step_col units; a carry of col by one more row less a run
  const long long f_step = (long long)step_row * p.fc.ss + W * p.step_col, f_carry = p.fc.ss - p.run;
  const long long o_step = (long long)step_row * p.ob.ss + W * p.step_col, o_carry = p.ob.ss - p.run;
  const float qnan = __builtin_nanf("");
  SkillAcc acc;
#pragma unroll
  for (int k = 0; k < SKILL_SUMS - 1; ++k) acc.s[k] = 0.0;
  acc.n = 0;
  // the wave's number lives in a scalar register and the lane is recomputed behind the loop: no thread index is kept across it
  const int wave = wave_number();
  const long long q = (long long)blk * SKILL_THREADS + threadIdx.x;
  const long long row0 = q / units;
  long long col = q - row0 * units;
  // row < cnt <=> the unit exists (col < units always); unsigned: row + step_row + 1 < 2^31 + 8 CUs * 256 does not wrap
  unsigned row = row0 < cnt ? (unsigned)row0 : cnt;
  long long f_at = row0 * p.fc.ss + W * col, o_at = row0 * p.ob.ss + W * col;
  long long wcol = 0;
  int wrow = 0;
  if (WMODE != W_NONE) {
    const long long at = (W * col) % (p.w_inner * p.w_len);
    wrow = (int)(at / p.w_inner);
    wcol = at - wrow * p.w_inner;
  }
  int label = 0;
  if (CLIMO && pl && row < cnt) label = pl[row];
  while (row < cnt) {
    float w[W];
    unit_weights<VEC, WMODE>(p, wrow, wcol, w);      // their addresses depend on no load: issued ahead of the data
    const bool in = !CLIMO || (unsigned)label < (unsigned)p.n_labels;      // a label out of range is never an address
    float x[W], y[W], c[W];
    if (VEC) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(pf + f_at);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(po + o_at);
      f32x4 cv = {0.f, 0.f, 0.f, 0.f};
      if (CLIMO) cv = *reinterpret_cast<const f32x4*>(pc + (in ? label : 0) * trow + W * col);
#pragma unroll
      for (int k = 0; k < W; ++k) x[k] = xv[k], y[k] = yv[k], c[k] = cv[k];
    } else {
      x[0] = pf[f_at], y[0] = po[o_at];
      c[0] = CLIMO ? pc[(in ? label : 0) * trow + col] : 0.f;
    }
    row += step_row;
    col += p.step_col;
    f_at += f_step;
    o_at += o_step;
    if (col >= units) {
      col -= units;
      ++row;
      f_at += f_carry;
      o_at += o_carry;
    }
    if (WMODE != W_NONE) {
      wcol += p.step_wcol;
      wrow += p.step_wrow;
      if (wcol >= p.w_inner) {
        wcol -= p.w_inner;
        ++wrow;
      }
      if (wrow >= p.w_len) wrow -= p.w_len;
    }
    int next_label = 0;
    if (CLIMO && pl && row < cnt) next_label = pl[row];
    unsigned counted = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float ck = in ? c[k] : qnan;
      pair_add<WMODE != W_NONE>(x[k] - y[k], CLIMO ? x[k] - ck : x[k], CLIMO ? y[k] - ck : y[k], w[k], acc, counted);
    }
    acc.n += counted;
    label = next_label;
  }
  double v[SKILL_SUMS];
  v[SKILL_SUMS - 1] = (double)acc.n;     // exact below 2^53 pairs
  v[0] = WMODE == W_NONE ? v[SKILL_SUMS - 1] : acc.s[0];
#pragma unroll
  for (int k = 1; k < SKILL_SUMS - 1; ++k) v[k] = acc.s[k];
  block_sums<SKILL_SUMS>(v, wave, partial + (long long)SKILL_SUMS * blockIdx.x);
}

template <bool VEC, int WMODE>
void skill_launch(const SkillArgs& p, unsigned grid, double* ws, hipStream_t s) {
  if (p.climo)
    skill_partial_kernel<VEC, WMODE, true><<<grid, SKILL_THREADS, 0, s>>>(p, ws);
  else
    skill_partial_kernel<VEC, WMODE, false><<<grid, SKILL_THREADS, 0, s>>>(p, ws);
}

}  // namespace

extern "C" {

size_t dlwp_verify_skill_workspace(dlwp_handle_t h, int leads, int groups) {
  if (leads < 1 || groups < 1) return 0;
  return cell_workspace_bytes(h, (long long)leads * groups, SKILL_BLOCKS_PER_CU, SKILL_SUMS * sizeof(double));
}

int dlwp_verify_skill_sums(dlwp_handle_t h, const void* fc, long long fc_lead_stride, long long fc_sample_stride, int fc_shift,
                           const void* ob, long long ob_lead_stride, long long ob_sample_stride, int ob_shift, int leads, int count0,
                           int count_dec, int groups, long long run, const void* climo, int n_labels, const void* labels,
                           long long label_lead_stride, int label_shift, const void* weights, int w_len, long long w_inner,
                           void* sums, void* ws, size_t ws_bytes, void* stream) {
  DLWP_UNTAPED(dlwp_verify_skill_sums);
  DLWP_CHECK_ARG(leads >= 1 && groups >= 1 && run >= 1, "dlwp_verify_skill_sums: leads %d, groups %d, run %lld must all be >= 1",
                 leads, groups, run);
  SkillArgs p;
  p.fc = window_of(fc, fc_lead_stride, fc_sample_stride, fc_shift);
  p.ob = window_of(ob, ob_lead_stride, ob_sample_stride, ob_shift);
  DLWP_CHECK_ARG(count_dec >= 0 && window_nonneg(p.fc) && window_nonneg(p.ob) && label_lead_stride >= 0 && label_shift >= 0,
                 "dlwp_verify_skill_sums: negative stride, shift or count_dec");
  DLWP_CHECK_ARG(!climo || (n_labels >= 1 && n_labels <= SKILL_MAX_LABELS), "dlwp_verify_skill_sums: n_labels %d, expected 1 .. %d",
                 n_labels, SKILL_MAX_LABELS);
  DLWP_CHECK_ARG(climo || !labels, "dlwp_verify_skill_sums: labels without a climatology table");
  DLWP_CHECK_ARG(!weights || (w_len >= 1 && w_inner >= 1 && w_len <= run && w_inner <= run / w_len && run % (w_inner * w_len) == 0),
                 "dlwp_verify_skill_sums: %d weights of %lld elements each do not divide a run of %lld", w_len, w_inner, run);
  DLWP_CHECK_ARG(fc && ob && sums, "dlwp_verify_skill_sums: null pointer");
  const long long cells = (long long)leads * groups;
  // inherited: at most 2^20 cells here and in spectrum.hip, fewer than 2^20 in verify.hip
  DLWP_CHECK_ARG(cells <= (1ll << 20), "dlwp_verify_skill_sums: %lld (lead, group) cells, at most 2^20", cells);
  const long long active = window_active_leads(leads, count0, count_dec);
  const bool vec = mult4(run) && window_vec(p.fc) && window_vec(p.ob) && aligned16(climo);
  const long long units = vec ? run / 4 : run;
  // no more blocks in a cell than lead 0 (the longest) has 256-unit slices
  const int bpc = cell_plan_bpc(h, active, groups, ((long long)count0 * units + SKILL_THREADS - 1) / SKILL_THREADS,
                                SKILL_BLOCKS_PER_CU);
  const size_t ws_need = (size_t)active * groups * bpc * SKILL_SUMS * sizeof(double);
  // inherited: a null workspace is accepted where no partial is written (verify.hip wants one regardless)
  DLWP_CHECK_ARG(ws_bytes >= ws_need && (ws || ws_need == 0), "dlwp_verify_skill_sums: workspace too small (%zu < %zu)", ws_bytes,
                 ws_need);
  DLWP_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dlwp_verify_skill_sums: workspace must be 8-byte aligned");
  DLWP_CHECK_ARG(h, "dlwp_verify_skill_sums: null handle");
  hipStream_t s = (hipStream_t)stream;
  if (active > 0) {
    p.climo = (const float*)climo;
    p.labels = (const int*)labels, p.weights = (const float*)weights;
    p.lab_ls = label_lead_stride;
    p.lab_shift = label_shift;
    p.count0 = count0, p.count_dec = count_dec;
    p.groups = groups, p.bpc = bpc;
    p.n_labels = climo ? n_labels : 1;
    p.w_len = weights ? w_len : 1;
    p.run = run;
    p.w_inner = weights ? w_inner : run;
    const long long step = (long long)bpc * SKILL_THREADS;
    p.step_row = step / units, p.step_col = step % units;
    // the step in elements, reduced to the weight period; the carry of col into row moves a whole run = whole periods
    const long long wstep = (p.step_col * (vec ? 4 : 1)) % (p.w_inner * p.w_len);
    p.step_wrow = (int)(wstep / p.w_inner), p.step_wcol = wstep % p.w_inner;
    const unsigned grid = (unsigned)(active * groups * bpc);      // <= max(cells, 8 blocks per CU)
    double* part = (double*)ws;
    if (!weights) {
      if (vec)
        skill_launch<true, W_NONE>(p, grid, part, s);
      else
        skill_launch<false, W_NONE>(p, grid, part, s);
    } else if (!vec) {
      skill_launch<false, W_UNIT>(p, grid, part, s);
    } else if (mult4(w_inner)) {
      skill_launch<true, W_UNIT>(p, grid, part, s);
    } else {
      skill_launch<true, W_ELEM>(p, grid, part, s);
    }
  }
  cell_final_kernel<SKILL_SUMS><<<(unsigned)cells, 64, 0, s>>>((const double*)ws, bpc, (int)(active * groups), (double*)sums);
  DLWP_LAUNCH_CHECK("verify_skill_sums kernels");
  return DLWP_OK;
}

}  // extern "C"
