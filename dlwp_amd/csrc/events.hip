// events.hip -- ensemble EVENT verification where the series is (gfx950): for up to 8 thresholds, how many members of a column show
// the event (x > thr, or x < thr) and whether it verified (y > thr / y < thr).  dlwp_ens_event_counts reduces that, per (lead, group)
// cell and threshold, to the joint count table[n][o] -- everything model/ensemble.py derives (Brier score and its decomposition,
// reliability diagram, ROC, ranked probability score) follows from it in float64 on the host -- and writes the probability field
// float32(n / M).  DESIGN.md 5.37 has the definitions and the measurements; include/dlwp_hip.h has the contract.
//
// One pass over the members: a lane owns four adjacent columns (16-byte loads, as ens_mean_spread_kernel) or one, keeps KP
// counters per column in registers (KP = 1, 2, 4, 8 >= K; the pad thresholds are NaN and never count) and compares the float32
// values themselves.  The per-group thresholds are wave-uniform and live in scalar registers.
//
// The table update.  A block of four waves keeps its table in LDS as `copies` interleaved replicas, table[bin * copies + c]: a lane
// adds to replica (lane & (copies - 1)), so the adds of a wave instruction spread over min(copies, 32) banks whatever the data
// are, and at most 64 / copies lanes meet on one address.  `copies` is the largest power of two <= 32 that keeps bins * copies
// within EV_TABLE_INTS.  Where that leaves fewer than 16 replicas (bins > 640: M >= 40 at K = 8) a tail threshold would put
// most of a wave on one address, so the wave aggregates first: up to EV_MATCH_ROUNDS times, take the first remaining lane's bin,
// ballot the lanes with the same bin, add their number once, remove them; the lanes still left hold other bins and use plain LDS
// adds.  Integer adds commute: the order of arrival changes no bit.
//
// Conventions of ensemble.hip / verify.hip: 64-bit offsets, no synchronisation, no size read from the device, no global atomics and
// no "last block" scheme.  Each block writes its partial table (32-bit: the host checks that a block counts fewer than 2^31
// columns) to the workspace and a second kernel adds a cell's partials in index order: repeated calls give identical bits.
#include "verify_common.h"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_MEMBERS = 256;
constexpr int EV_MAX_THRESHOLDS = 8;
constexpr int EV_TABLE_INTS = 10240;       // at most 40 KB of (dynamic) LDS for the replicas: four blocks share a CU, K = 8, M = 32 gets 16
constexpr int EV_MAX_COPIES = 32;          // one replica per LDS bank
constexpr int EV_MATCH_ROUNDS = 4;
constexpr int EV_BLOCKS_PER_CU = 10;       // grid cap: twice the blocks a CU holds

struct EventArgs {
  const float* x;
  const float* y;                          // null: no table
  const float* thr;
  float* prob;                             // may be null
  unsigned* partial;                       // (blocks, bins); null: no table
  long long ls, ss, ms, run;
  int leads, samples, members, groups, thresholds, bpc;
  unsigned tiles_per_row;                  // tiles of EV_THREADS * W points of one group in one sample row
  int copies, rounds;                      // replicas of the LDS table; match rounds (0: none)
};

template <bool BELOW>
__device__ __forceinline__ bool event_of(float v, float t) {
  return BELOW ? v < t : v > t;
}

// one column's update of bin `bin` (counted where ok); uniform control flow: every lane of the wave calls it
__device__ __forceinline__ void table_add(unsigned* tab, int bin, bool ok, int copies, int rounds, int lane) {
  const int c = lane & (copies - 1);
  if (rounds) {                            // uniform
    unsigned long long live = __ballot(ok);
    for (int r = 0; r < rounds && live; ++r) {
      const int leader = __ffsll((long long)live) - 1;
      const int b = __builtin_amdgcn_readlane(bin, leader);
      const unsigned long long same = __ballot(ok && bin == b);
      if (lane == leader) atomicAdd(&tab[b * copies + c], (unsigned)__popcll(same));
      ok = ok && bin != b;
      live &= ~same;
    }
  }
  if (ok) atomicAdd(&tab[bin * copies + c], 1u);
}

// Block blk of cell (lead f, group g) takes the tiles blk, blk + bpc, ... of the cell's samples x tiles_per_row grid; a lane owns
// the W points from (tile * EV_THREADS + thread) * W of the group.  Lanes past the end of the run read point 0 (in bounds) and
// neither count nor store.  PP: a threshold per point.
template <int W, int KP, bool BELOW, bool PP>
__global__ __launch_bounds__(EV_THREADS) void ens_event_kernel(EventArgs p) {
  extern __shared__ unsigned ev_lds[];     // the table's replicas, then float32(n / M) for n = 0 .. M
  const int M = p.members, K = p.thresholds;
  const int bins = K * (M + 1) * 2;
  unsigned* tab = ev_lds;
  float* pof = reinterpret_cast<float*>(ev_lds + bins * p.copies);
  const int lane = threadIdx.x & 63;
  const unsigned cell = blockIdx.x / (unsigned)p.bpc, blk = blockIdx.x - cell * (unsigned)p.bpc;
  const unsigned f = cell / (unsigned)p.groups, g = cell - f * (unsigned)p.groups;
  const bool tabled = p.partial != nullptr;
  if (tabled)
    for (int b = threadIdx.x; b < bins * p.copies; b += EV_THREADS) tab[b] = 0u;
  if (p.prob)
    for (int n = threadIdx.x; n <= M; n += EV_THREADS) pof[n] = (float)((double)n / (double)M);
  __syncthreads();
  const long long row = (long long)p.groups * p.run;
  const float nan = __builtin_nanf("");
  float thr[KP][W];
  if (!PP) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float t = k < K ? p.thr[(long long)k * p.groups + g] : nan;
#pragma unroll
      for (int c = 0; c < W; ++c) thr[k][c] = t;
    }
  }
  const unsigned tiles = (unsigned)p.samples * p.tiles_per_row;          // < 2^31: checked by the host
  for (unsigned tile = blk; tile < tiles; tile += (unsigned)p.bpc) {
    const unsigned s = tile / p.tiles_per_row, tp = tile - s * p.tiles_per_row;
    const long long col = ((long long)tp * EV_THREADS + threadIdx.x) * W;
    const bool active = col < p.run;
    const long long pc = (long long)g * p.run + (active ? col : 0);
    const float* px = p.x + (long long)f * p.ls + (long long)s * p.ss + pc;
    const long long yo = ((long long)f * p.samples + s) * row + pc;
    if (PP) {
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < K) {                       // uniform
          const float* pt = p.thr + (long long)k * row + pc;
          if (W == 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(pt);
#pragma unroll
            for (int c = 0; c < W; ++c) thr[k][c] = q[c];
          } else {
            thr[k][0] = pt[0];
          }
        } else {
#pragma unroll
          for (int c = 0; c < W; ++c) thr[k][c] = nan;
        }
      }
    }
    float yv[W];
#pragma unroll
    for (int c = 0; c < W; ++c) yv[c] = 0.0f;
    if (tabled) {
      if (W == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p.y + yo);
#pragma unroll
        for (int c = 0; c < W; ++c) yv[c] = q[c];
      } else {
        yv[0] = p.y[yo];
      }
    }
    int n[KP][W];
    bool bad[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
      bad[c] = false;
#pragma unroll
      for (int k = 0; k < KP; ++k) n[k][c] = 0;
    }
#pragma unroll 8
    for (int i = 0; i < M; ++i) {
      float v[W];
      if (W == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(px + (long long)i * p.ms);
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = q[c];
      } else {
        v[0] = px[(long long)i * p.ms];
      }
#pragma unroll
      for (int c = 0; c < W; ++c) {
        bad[c] = bad[c] || v[c] != v[c];
#pragma unroll
        for (int k = 0; k < KP; ++k) n[k][c] += event_of<BELOW>(v[c], thr[k][c]) ? 1 : 0;
      }
    }
    if (tabled) {
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < K) {                       // uniform
#pragma unroll
          for (int c = 0; c < W; ++c) {
            const bool ok = active && !bad[c] && yv[c] == yv[c] && thr[k][c] == thr[k][c];
            const int o = event_of<BELOW>(yv[c], thr[k][c]) ? 1 : 0;
            table_add(tab, (k * (M + 1) + n[k][c]) * 2 + o, ok, p.copies, p.rounds, lane);
          }
        }
      }
    }
    if (p.prob && active) {
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < K) {                       // uniform
          float o[W];
#pragma unroll
          for (int c = 0; c < W; ++c) o[c] = (bad[c] || thr[k][c] != thr[k][c]) ? nan : pof[n[k][c]];
          float* po = p.prob + ((long long)k * p.leads * p.samples) * row + yo;
          if (W == 4)
            *reinterpret_cast<f32x4*>(po) = f32x4{o[0], o[W > 1 ? 1 : 0], o[W > 2 ? 2 : 0], o[W > 3 ? 3 : 0]};
          else
            po[0] = o[0];
        }
      }
    }
  }
  if (tabled) {
    __syncthreads();
    unsigned* out = p.partial + (long long)blockIdx.x * bins;
    for (int b = threadIdx.x; b < bins; b += EV_THREADS) {
      unsigned acc = 0u;
      for (int c = 0; c < p.copies; ++c) acc += tab[b * p.copies + c];
      out[b] = acc;
    }
  }
}

// stage 2: one block per cell; a thread adds the partials of its bins in index order
__global__ __launch_bounds__(EV_THREADS) void ens_event_final_kernel(const unsigned* __restrict__ partial, int bpc, int bins,
                                                                     long long* __restrict__ table) {
  const long long cell = blockIdx.x;
  for (int b = threadIdx.x; b < bins; b += EV_THREADS) {
    const unsigned* src = partial + cell * bpc * bins + b;
    long long acc = 0;
    for (int i = 0; i < bpc; ++i) acc += (long long)src[(long long)i * bins];
    table[cell * bins + b] = acc;
  }
}

inline bool ev_sizes_ok(int leads, int groups, int members, int thresholds) {
  return leads >= 1 && groups >= 1 && members >= 2 && members <= EV_MAX_MEMBERS && thresholds >= 1 && thresholds <= EV_MAX_THRESHOLDS;
}

inline size_t ev_partial_bytes(int members, int thresholds) { return (size_t)thresholds * (members + 1) * 2 * sizeof(unsigned); }

inline size_t ev_lds_bytes(const EventArgs& p) {
  return ((size_t)p.thresholds * (p.members + 1) * 2 * p.copies + p.members + 1) * sizeof(unsigned);
}

template <int W, int KP, bool BELOW>
void ev_launch_pp(const EventArgs& p, bool pp, unsigned grid, hipStream_t s) {
  if (pp)
    ens_event_kernel<W, KP, BELOW, true><<<grid, EV_THREADS, ev_lds_bytes(p), s>>>(p);
  else
    ens_event_kernel<W, KP, BELOW, false><<<grid, EV_THREADS, ev_lds_bytes(p), s>>>(p);
}

template <int W, int KP>
void ev_launch_kp(const EventArgs& p, bool below, bool pp, unsigned grid, hipStream_t s) {
  if (below)
    ev_launch_pp<W, KP, true>(p, pp, grid, s);
  else
    ev_launch_pp<W, KP, false>(p, pp, grid, s);
}

template <int W>
void ev_launch(const EventArgs& p, bool below, bool pp, unsigned grid, hipStream_t s) {
  if (p.thresholds <= 1) ev_launch_kp<W, 1>(p, below, pp, grid, s);
  else if (p.thresholds <= 2) ev_launch_kp<W, 2>(p, below, pp, grid, s);
  else if (p.thresholds <= 4) ev_launch_kp<W, 4>(p, below, pp, grid, s);
  else ev_launch_kp<W, 8>(p, below, pp, grid, s);
}

}  // namespace

extern "C" {

size_t dlwp_ens_event_workspace(dlwp_handle_t h, int leads, int groups, int members, int thresholds) {
  if (!ev_sizes_ok(leads, groups, members, thresholds)) return 0;
  const long long cells = (long long)leads * groups;
  return (size_t)cells * (size_t)cell_bpc_cap(h, cells, EV_BLOCKS_PER_CU) * ev_partial_bytes(members, thresholds);
}

int dlwp_ens_event_counts(dlwp_handle_t h, const void* x, long long lead_stride, long long sample_stride, long long member_stride,
                          const void* y, const void* thr, int thr_per_point, int below, int leads, int samples, int members,
                          int groups, long long run, int thresholds, void* table, void* prob_out, void* ws, size_t ws_bytes,
                          void* stream) {
  DLWP_UNTAPED(dlwp_ens_event_counts);
  DLWP_CHECK_ARG(leads >= 1 && samples >= 1 && groups >= 1 && run >= 1,
                 "dlwp_ens_event_counts: leads %d, samples %d, groups %d, run %lld must all be >= 1", leads, samples, groups, run);
  DLWP_CHECK_ARG(members >= 2 && members <= EV_MAX_MEMBERS, "dlwp_ens_event_counts: members %d, expected 2 .. %d", members,
                 EV_MAX_MEMBERS);
  DLWP_CHECK_ARG(thresholds >= 1 && thresholds <= EV_MAX_THRESHOLDS, "dlwp_ens_event_counts: thresholds %d, expected 1 .. %d",
                 thresholds, EV_MAX_THRESHOLDS);
  DLWP_CHECK_ARG((thr_per_point == 0 || thr_per_point == 1) && (below == 0 || below == 1),
                 "dlwp_ens_event_counts: flags thr_per_point %d, below %d, expected 0 or 1", thr_per_point, below);
  DLWP_CHECK_ARG(lead_stride >= 0 && sample_stride >= 0 && member_stride >= 0, "dlwp_ens_event_counts: negative stride");
  DLWP_CHECK_ARG(x && thr && (table || prob_out) && (y != nullptr) == (table != nullptr) && (!table || ws),
                 "dlwp_ens_event_counts: null pointer (y and table go together, table needs ws, one of table / prob_out is needed)");
  const long long cells = (long long)leads * groups;
  DLWP_CHECK_ARG(cells < (1ll << 20), "dlwp_ens_event_counts: %lld (lead, group) cells, at most 2^20", cells);
  const bool vec = mult4(run) && mult4(lead_stride) && mult4(sample_stride) && mult4(member_stride) && aligned16(x) && aligned16(y) &&
                   aligned16(prob_out) && (!thr_per_point || aligned16(thr));
  const long long tile_points = (long long)EV_THREADS * (vec ? 4 : 1);
  const long long tiles_per_row = (run + tile_points - 1) / tile_points;
  DLWP_CHECK_ARG(tiles_per_row < (1ll << 31) / samples, "dlwp_ens_event_counts: %d samples of %lld floats are too many tiles", samples,
                 run);
  const long long tiles = (long long)samples * tiles_per_row;
  const long long cap = cell_bpc_cap(h, cells, EV_BLOCKS_PER_CU);
  const int bpc = (int)(tiles < cap ? tiles : cap);
  // the partial tables are 32-bit: a block counts (tiles / bpc rounded up) * tile_points columns at most
  DLWP_CHECK_ARG((tiles + bpc - 1) / bpc < (1ll << 31) / tile_points,
                 "dlwp_ens_event_counts: %lld tiles over %d blocks per cell are too many columns for a 32-bit partial count", tiles, bpc);
  const int bins = thresholds * (members + 1) * 2;
  if (table) {
    const size_t ws_need = (size_t)cells * (size_t)bpc * ev_partial_bytes(members, thresholds);
    DLWP_CHECK_ARG(ws_bytes >= ws_need, "dlwp_ens_event_counts: workspace too small (%zu < %zu)", ws_bytes, ws_need);
    DLWP_CHECK_ARG(((uintptr_t)ws & 3) == 0, "dlwp_ens_event_counts: workspace must be 4-byte aligned");
  }
  DLWP_CHECK_ARG(h, "dlwp_ens_event_counts: null handle");
  EventArgs p;
  p.x = (const float*)x, p.y = (const float*)y, p.thr = (const float*)thr, p.prob = (float*)prob_out;
  p.partial = table ? (unsigned*)ws : nullptr;
  p.ls = lead_stride, p.ss = sample_stride, p.ms = member_stride, p.run = run;
  p.leads = leads, p.samples = samples, p.members = members, p.groups = groups, p.thresholds = thresholds, p.bpc = bpc;
  p.tiles_per_row = (unsigned)tiles_per_row;
  int copies = 1;
  while (copies < EV_MAX_COPIES && bins * copies * 2 <= EV_TABLE_INTS) copies *= 2;
  p.copies = copies;
  p.rounds = copies < 16 ? EV_MATCH_ROUNDS : 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)(cells * bpc);      // <= max(cells, EV_BLOCKS_PER_CU blocks per CU)
  if (vec)
    ev_launch<4>(p, below != 0, thr_per_point != 0, grid, s);
  else
    ev_launch<1>(p, below != 0, thr_per_point != 0, grid, s);
  if (table) ens_event_final_kernel<<<(unsigned)cells, EV_THREADS, 0, s>>>(p.partial, bpc, bins, (long long*)table);
  DLWP_LAUNCH_CHECK("ens_event_counts kernels");
  return DLWP_OK;
}

}  // extern "C"
