// series.hip -- batches of SeriesDataGenerator cut out of a series that lives in HBM (gfx950): one launch copies every window of a
// batch -- the input steps, the insolation planes behind them, every target block -- from up to four (rows, row) float32 sources
// into X and the target arrays.
//
// Reference: DLWP/model/generators.py:323-629 (SeriesDataGenerator.generate: one fancy-index copy per time step, a stack, an
// insolation concatenate and a reshape per target block, all on the host).  dlwp_amd/model/generators.py turns the same windows into
// a table of segments (window_plan); a segment is a run of floats that is contiguous in its source and in its destination:
//   dst[g.dst][i * row_d + g.dst_at + e] = src[g.src][(samples[i] + g.shift) * row_s + g.src_at + e],   e < g.len, i < n
// A run may continue over the end of its source row into the following times (that is what merging the consecutive states of a
// window into one segment means); it is one unit for the bounds: when the first or the last time it touches is no row of the
// source, the whole run is stored as quiet NaNs and nothing is read.
// Work: a sample's segments are cut into chunks of SERIES_CHUNK units (a unit is a 16-byte word on the vector path, a float on the
// scalar one); a 256-thread block takes one chunk per turn, four units per thread with the four loads in front of the four
// stores, and walks the (sample, chunk) list with the stride of the grid.  Everything that selects the segment is the same in
// every lane of a block: the chunk index comes from blockIdx, the segment from one ballot over the chunk prefix, its
// descriptors from the kernel arguments.  No atomics, no LDS, no synchronisation, 64-bit offsets.
#include "verify_common.h"      // mult4, aligned16

#include <type_traits>

namespace {

constexpr int SERIES_THREADS = 256;
constexpr int SERIES_UNROLL = 4;
constexpr int SERIES_CHUNK = SERIES_THREADS * SERIES_UNROLL;      // units a block moves per turn
constexpr int SERIES_BLOCKS_PER_CU = 8;                           // the cap of the other copy kernels (verify.hip)

static_assert(DLWP_SERIES_MAX_SEGS <= 64, "the segment of a chunk is found by one 64-lane ballot");

// a segment as the kernel reads it: the host has divided already
struct SeriesSeg {
  int src_dst;                               // src | dst << 8
  int span;                                  // times behind the first one that the run touches: (src_at + len - 1) / row_s
  long long shift, src_at, dst_at, units;
};

struct SeriesArgs {
  dlwp_series_src src[DLWP_SERIES_MAX_SRCS];
  dlwp_series_dst dst[DLWP_SERIES_MAX_DSTS];
  SeriesSeg seg[DLWP_SERIES_MAX_SEGS];
  int cstart[DLWP_SERIES_MAX_SEGS + 1];      // chunks of a sample in front of segment g; entries past n_seg repeat the total
  int step_i, step_c;                        // the grid's stride over (sample, chunk), divided on the host
  const long long* samples;
  long long n;
};
// the kernel-argument space holds 4 KiB, of which the compiler's hidden arguments take 256 bytes
static_assert(sizeof(SeriesArgs) + 256 <= 4096, "the descriptor tables must fit the kernel-argument space");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__global__ __launch_bounds__(SERIES_THREADS) void series_window_gather_kernel(const SeriesArgs p) {
  typedef typename std::conditional<VEC, u32x4, unsigned>::type word_t;
  constexpr int W = VEC ? 4 : 1;
  const unsigned qnan = 0x7fc00000u;
  const int chunks = p.cstart[DLWP_SERIES_MAX_SEGS];               // of one sample
  const int lane = threadIdx.x & 63;
  const int my_end = p.cstart[lane + 1 < DLWP_SERIES_MAX_SEGS ? lane + 1 : DLWP_SERIES_MAX_SEGS];      // lane g: where segment g ends
  long long i = blockIdx.x / (unsigned)chunks;
  int c = (int)(blockIdx.x - (unsigned)i * (unsigned)chunks);
  while (i < p.n) {
    // segments in front of chunk c: those that end at or before it (empty trailing entries end at `chunks` > c)
    const int g = __builtin_amdgcn_readfirstlane(__popcll(__ballot(my_end <= c)));
    const SeriesSeg sg = p.seg[g];
    const dlwp_series_src ss = p.src[sg.src_dst & 255];
    const dlwp_series_dst dd = p.dst[sg.src_dst >> 8];
    const long long units = sg.units;
    // the first time of the run (wrapping add: |shift| < 2^40 cannot wrap a start position into the source) and the last one
    const long long t = (long long)((unsigned long long)p.samples[i] + (unsigned long long)sg.shift);
    const bool in = t >= 0 && t <= ss.rows - 1 - sg.span;
    const unsigned* sp = (const unsigned*)ss.base + (in ? t : 0) * ss.row + sg.src_at;
    unsigned* dp = (unsigned*)dd.base + i * dd.row + sg.dst_at;
    const long long u0 = (long long)(c - p.cstart[g]) * SERIES_CHUNK + threadIdx.x;
    word_t v[SERIES_UNROLL];
#pragma unroll
    for (int u = 0; u < SERIES_UNROLL; ++u) {
      const long long q = u0 + u * SERIES_THREADS;
      v[u] = (word_t)qnan;
      if (in && q < units) v[u] = *reinterpret_cast<const word_t*>(sp + q * W);
    }
#pragma unroll
    for (int u = 0; u < SERIES_UNROLL; ++u) {
      const long long q = u0 + u * SERIES_THREADS;
      if (q < units) *reinterpret_cast<word_t*>(dp + q * W) = v[u];
    }
    i += p.step_i;
    c += p.step_c;
    if (c >= chunks) {
      c -= chunks;
      ++i;
    }
  }
}

constexpr long long SERIES_MAX_FLOATS = 0x7fffffffffffffffll / 4;

}  // namespace

extern "C" {

int dlwp_series_gather_grid_cap(dlwp_handle_t h) { return h ? h->cu_count * SERIES_BLOCKS_PER_CU : 0; }

int dlwp_series_window_gather(dlwp_handle_t h, const dlwp_series_src* srcs, int n_src, const dlwp_series_dst* dsts, int n_dst,
                              const dlwp_series_seg* segs, int n_seg, const void* samples, long long n, void* stream) {
  DLWP_UNTAPED(dlwp_series_window_gather);
  DLWP_CHECK_ARG(n_src >= 1 && n_src <= DLWP_SERIES_MAX_SRCS, "dlwp_series_window_gather: n_src %d, expected 1 .. %d", n_src,
                 DLWP_SERIES_MAX_SRCS);
  DLWP_CHECK_ARG(n_dst >= 1 && n_dst <= DLWP_SERIES_MAX_DSTS, "dlwp_series_window_gather: n_dst %d, expected 1 .. %d", n_dst,
                 DLWP_SERIES_MAX_DSTS);
  DLWP_CHECK_ARG(n_seg >= 1 && n_seg <= DLWP_SERIES_MAX_SEGS, "dlwp_series_window_gather: n_seg %d, expected 1 .. %d", n_seg,
                 DLWP_SERIES_MAX_SEGS);
  DLWP_CHECK_ARG(n >= 0, "dlwp_series_window_gather: n %lld must be >= 0", n);
  DLWP_CHECK_ARG(srcs && dsts && segs, "dlwp_series_window_gather: null pointer");
  bool vec = true;
  for (int s = 0; s < n_src; ++s) {
    DLWP_CHECK_ARG(srcs[s].base, "dlwp_series_window_gather: null pointer (source %d)", s);
    DLWP_CHECK_ARG(srcs[s].rows >= 1 && srcs[s].row >= 1, "dlwp_series_window_gather: source %d: rows %lld, row %lld must be >= 1", s,
                   srcs[s].rows, srcs[s].row);
    DLWP_CHECK_ARG(srcs[s].rows <= SERIES_MAX_FLOATS / srcs[s].row, "dlwp_series_window_gather: source %d: %lld rows of %lld floats overflow",
                   s, srcs[s].rows, srcs[s].row);
    vec = vec && mult4(srcs[s].row) && aligned16(srcs[s].base);
  }
  for (int d = 0; d < n_dst; ++d) {
    DLWP_CHECK_ARG(dsts[d].base, "dlwp_series_window_gather: null pointer (destination %d)", d);
    DLWP_CHECK_ARG(dsts[d].row >= 1, "dlwp_series_window_gather: destination %d: row %lld must be >= 1", d, dsts[d].row);
    DLWP_CHECK_ARG(n <= SERIES_MAX_FLOATS / dsts[d].row, "dlwp_series_window_gather: destination %d: n %lld rows of %lld floats overflow", d,
                   n, dsts[d].row);
    vec = vec && mult4(dsts[d].row) && aligned16(dsts[d].base);
  }
  for (int g = 0; g < n_seg; ++g) {
    const dlwp_series_seg& sg = segs[g];
    DLWP_CHECK_ARG(sg.src >= 0 && sg.src < n_src && sg.dst >= 0 && sg.dst < n_dst,
                   "dlwp_series_window_gather: segment %d: source %d of %d, destination %d of %d", g, sg.src, n_src, sg.dst, n_dst);
    DLWP_CHECK_ARG(sg.len >= 1, "dlwp_series_window_gather: segment %d: len %lld must be >= 1", g, sg.len);
    DLWP_CHECK_ARG(sg.src_at >= 0 && sg.src_at < srcs[sg.src].row,
                   "dlwp_series_window_gather: segment %d: src_at %lld leaves the source row of %lld floats", g, sg.src_at, srcs[sg.src].row);
    DLWP_CHECK_ARG(sg.dst_at >= 0 && sg.dst_at <= dsts[sg.dst].row && sg.len <= dsts[sg.dst].row - sg.dst_at,
                   "dlwp_series_window_gather: segment %d: dst_at %lld + len %lld leaves the destination row of %lld floats", g, sg.dst_at,
                   sg.len, dsts[sg.dst].row);
    // a run over consecutive times ends inside the source: (rows - 1) * row + src_at + len must not overflow, nor the shifted time
    DLWP_CHECK_ARG(sg.len <= SERIES_MAX_FLOATS - srcs[sg.src].row && sg.shift > -(1ll << 40) && sg.shift < (1ll << 40),
                   "dlwp_series_window_gather: segment %d: len %lld or shift %lld overflow", g, sg.len, sg.shift);
    vec = vec && mult4(sg.src_at) && mult4(sg.dst_at) && mult4(sg.len);
  }
  SeriesArgs p;
  memset(&p, 0, sizeof(p));
  long long chunks = 0;
  for (int g = 0; g < n_seg; ++g) {
    const dlwp_series_seg& sg = segs[g];
    const long long span = (sg.src_at + sg.len - 1) / srcs[sg.src].row;
    DLWP_CHECK_ARG(span < (1ll << 31), "dlwp_series_window_gather: segment %d: a run over %lld source rows overflows", g, span + 1);
    p.seg[g].src_dst = sg.src | sg.dst << 8;
    p.seg[g].span = (int)span;
    p.seg[g].shift = sg.shift, p.seg[g].src_at = sg.src_at, p.seg[g].dst_at = sg.dst_at;
    p.seg[g].units = sg.len / (vec ? 4 : 1);
    p.cstart[g] = (int)chunks;
    chunks += (p.seg[g].units + SERIES_CHUNK - 1) / SERIES_CHUNK;
    DLWP_CHECK_ARG(chunks < (1ll << 30), "dlwp_series_window_gather: a sample of more than 2^30 chunks of %d units overflows", SERIES_CHUNK);
  }
  for (int g = n_seg; g <= DLWP_SERIES_MAX_SEGS; ++g) p.cstart[g] = (int)chunks;
  DLWP_CHECK_ARG(n <= 0x7fffffffffffffffll / chunks, "dlwp_series_window_gather: n %lld samples of %lld chunks overflow", n, chunks);
  if (n == 0) return DLWP_OK;
  DLWP_CHECK_ARG(samples, "dlwp_series_window_gather: null pointer (samples)");
  DLWP_CHECK_ARG(h, "dlwp_series_window_gather: null handle");
  for (int s = 0; s < n_src; ++s) p.src[s] = srcs[s];
  for (int d = 0; d < n_dst; ++d) p.dst[d] = dsts[d];
  p.samples = (const long long*)samples;
  p.n = n;
  const long long turns = n * chunks;
  const long long cap = (long long)h->cu_count * SERIES_BLOCKS_PER_CU;
  const long long grid = turns < cap ? turns : cap;
  p.step_i = (int)(grid / chunks), p.step_c = (int)(grid % chunks);
  if (vec)
    series_window_gather_kernel<true><<<(unsigned)grid, SERIES_THREADS, 0, (hipStream_t)stream>>>(p);
  else
    series_window_gather_kernel<false><<<(unsigned)grid, SERIES_THREADS, 0, (hipStream_t)stream>>>(p);
  DLWP_LAUNCH_CHECK("series_window_gather kernel");
  return DLWP_OK;
}

}  // extern "C"
