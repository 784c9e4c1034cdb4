// perturb.hip -- the ensemble member generator (gfx950): out[s, m] = x[s] + sign * sigma[k] * zeta(d, s, k), a perturbed-initial-
// condition ensemble made where the rollout reads it.  DESIGN.md 5.36 and include/dlwp_hip.h have the definition; the numpy
// statement in dlwp_amd/model/ensemble.py is the contract.  The reference has no counterpart (its examples/plot_ensemble.py
// averages differently trained models on the host).
//
// White noise z(d, s, k, i, j): Philox-4x32-10 (philox.h) with key (seed lo, seed hi) and counter (j >> 2, (i + 32768) + 65536 k, d, s);
// words (w0, w1) and (w2, w3) each give a Box-Muller pair.  The row i is VIRTUAL: rows beyond the poles and the columns across the
// date line exist in counter space, so the smoothing has no boundary rule and reads no memory for its halo.
//
//   white path (both radii 0)   no LDS.  A lane owns a column quad of one (s, k, i): one Philox block and four normals per draw.  It
//                               loads its quad of x once and stores it for every member of its member chunk (the chunk is the whole
//                               call where the rows alone fill the chip), so input traffic is 1 / chunk of the output's.
//   smoothed path               a workgroup of 256 owns a 32 x 64 tile of one (draw, sample, channel): the white tile with its halo
//                               goes to LDS, then the longitude pass, then the latitude pass, then the store -- for both members of an
//                               antithetic pair.  LDS (tile + 2 R)^2-ish floats: 40 KB at R = 16 (4 workgroups per CU of 160 KB),
//                               24.6 KB at R = 6 (6 workgroups = 24 waves per CU); the halo costs 1.63 x the Philox blocks at R = 6.
//
// Every float32 operation that the definition rounds is written as __fmul_rn / __fadd_rn, which the compiler never contracts: the
// 16-byte and the element path, every tile and every split of the members over calls give the same bits.  No atomics, no
// allocation, no synchronisation; every output element is written by exactly one lane.
#include "common.h"
#include "philox.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_TH = 32;                  // tile of the smoothed path: rows
constexpr int PT_TW = 64;                  //                            columns (one wave per row of the passes)
constexpr int PT_MAX_R = DLWP_ENS_MAX_RADIUS;
constexpr int PT_WHITE_LANES = 256 * 2048; // lanes that fill an MI355X: the white path splits the members until it has them

struct PerturbArgs {
  const float* x;
  const float* sigma;
  float* out;
  long long oss, oms;                      // output strides of the sample and the member axis, elements
  long long units;                         // white path: quads of the input
  int S, K, H, W;
  int members, first;
  unsigned k0, k1;
  int control, anti;
  int Ry, Rx;
  int qw;                                  // column quads per row
  int chunk;                               // white path: members per lane
  int d_lo, draws;                         // smoothed path: first draw and draws of the call
  int p_lo, p_hi;                          // draw-index range [p_lo, p_hi) of the call's members
  int tiles_y, tiles_x;
  float gy[2 * PT_MAX_R + 1], gx[2 * PT_MAX_R + 1];
};

// u1 = (2 (wa >> 9) + 1) 2^-24 in (0, 1) and 2 u2 = (wb >> 8) 2^-23 in [0, 2) are exact in float32
__device__ __forceinline__ void normal_pair(unsigned wa, unsigned wb, float& ze, float& zo) {
  const float u1 = (float)(2u * (wa >> 9) + 1u) * 0x1p-24f;
  const float a = (float)(wb >> 8) * 0x1p-23f;
  const float r = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincospif(a, &sn, &cs);
  ze = __fmul_rn(r, cs);
  zo = __fmul_rn(r, sn);
}

// the four normals of column quad q of virtual row i
__device__ __forceinline__ void white_quad(const PerturbArgs& p, int q, int i, int k, int d, int s, float (&z)[4]) {
  unsigned w[4];
  philox4x32_10((unsigned)q, (unsigned)(i + 32768) + 65536u * (unsigned)k, (unsigned)d, (unsigned)s, p.k0, p.k1, w);
  normal_pair(w[0], w[1], z[0], z[1]);
  normal_pair(w[2], w[3], z[2], z[3]);
}

__device__ __forceinline__ float perturbed(float x, float sigma, float zeta, bool neg) {
  const float t = __fmul_rn(sigma, zeta);
  return __fadd_rn(x, neg ? -t : t);
}

// ---- white path ---------------------------------------------------------------------------------------------------------------------- //
template <bool VEC>
__global__ __launch_bounds__(PT_THREADS) void ens_perturb_white_kernel(PerturbArgs p) {
  const long long u = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (u >= p.units) return;
  const int q = (int)(u % p.qw);
  const long long rr = u / p.qw;
  const int i = (int)(rr % p.H);
  const long long sk = rr / p.H;
  const int k = (int)(sk % p.K), s = (int)(sk / p.K);
  const int j0 = 4 * q;
  const int nv = p.W - j0 < 4 ? p.W - j0 : 4;            // VEC: always 4
  const long long at = rr * p.W + j0;                    // offset in x; rr = (s K + k) H + i
  const long long orow = at - (long long)s * p.K * p.H * p.W;
  float xv[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p.x + at);
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] = v[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) xv[e] = p.x[at + e];
  }
  const float sg = p.sigma[k];
  const int m0 = blockIdx.y * p.chunk;
  const int m1 = m0 + p.chunk < p.members ? m0 + p.chunk : p.members;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  int d_have = -1;
  for (int m = m0; m < m1; ++m) {
    const int g = p.first + m;
    float o[4];
    if (p.control && g == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = xv[e];
    } else {
      const int pi = g - p.control;
      const int d = p.anti ? pi >> 1 : pi;
      const bool neg = p.anti && (pi & 1);
      if (d != d_have) {
        white_quad(p, q, i, k, d, s, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = __fadd_rn(0.f, z[e]);    // the one-tap pass of the definition (-0 becomes +0)
        d_have = d;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = perturbed(xv[e], sg, z[e], neg);
    }
    float* po = p.out + (long long)s * p.oss + (long long)m * p.oms + orow;
    if (VEC) {
      *reinterpret_cast<f32x4*>(po) = f32x4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nv) po[e] = o[e];
    }
  }
}

// ---- smoothed path ------------------------------------------------------------------------------------------------------------------- //
// the control member of a smoothed call: out[s, 0] = x[s]
__global__ __launch_bounds__(PT_THREADS) void ens_perturb_control_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                         long long row, long long total, long long oss) {
  const long long e = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long s = e / row;
  out[s * oss + (e - s * row)] = x[e];
}

__global__ __launch_bounds__(PT_THREADS) void ens_perturb_smooth_kernel(PerturbArgs p) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int Ry = p.Ry, Rx = p.Rx;
  const int PW = PT_TW + 2 * Rx;                          // pitch of the white tile
  float* white = lds;                                     // (PT_TH + 2 Ry) x PW
  float* rowp = lds + (PT_TH + 2 * Ry) * PW;              // (PT_TH + 2 Ry) x PT_TW
  unsigned b = blockIdx.x;
  const int tiles = p.tiles_y * p.tiles_x;
  const int tile = (int)(b % (unsigned)tiles);
  b /= (unsigned)tiles;
  const int k = (int)(b % (unsigned)p.K);
  b /= (unsigned)p.K;
  const int s = (int)(b % (unsigned)p.S);
  const int d = p.d_lo + (int)(b / (unsigned)p.S);
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int i0 = ty * PT_TH, j0 = tx * PT_TW;
  const int th = p.H - i0 < PT_TH ? p.H - i0 : PT_TH;
  const int tw = p.W - j0 < PT_TW ? p.W - j0 : PT_TW;
  const int nr = th + 2 * Ry, nc = tw + 2 * Rx;           // nr <= PT_TH + 2 Ry, nc <= PW

  // 1. white noise.  Tile column c is the unwrapped column ulo + c (shifted by W, so never negative: Rx <= W); unwrapped column
  //    u = kk W + j belongs to Philox quad j >> 2 of period kk.  An item is one quad of one row; a quad cut by the tile's edge or by
  //    the date line writes only its columns inside [0, nc).
  const int ulo = j0 - Rx + p.W;
  const int pid_lo = (ulo / p.W) * p.qw + ((ulo % p.W) >> 2);
  const int uhi = ulo + nc - 1;
  const int np = (uhi / p.W) * p.qw + ((uhi % p.W) >> 2) - pid_lo + 1;
  for (int it = tid; it < nr * np; it += PT_THREADS) {
    const int r = it / np;
    const int pid = pid_lo + (it - r * np);
    const int kk = pid / p.qw, q = pid - kk * p.qw;
    float z[4];
    white_quad(p, q, i0 - Ry + r, k, d, s, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * q + e;
      const int c = kk * p.W + j - ulo;
      if (j < p.W && c >= 0 && c < nc) white[r * PW + c] = z[e];
    }
  }
  __syncthreads();

  // 2. longitude pass: taps in ascending order, a float32 accumulator from 0
  const int c = tid & (PT_TW - 1), r0 = tid >> 6;
  if (c < tw) {
    for (int r = r0; r < nr; r += PT_THREADS / PT_TW) {
      float acc = 0.f;
      const float* w = white + r * PW + c;
      for (int t = 0; t <= 2 * Rx; ++t) acc = __fadd_rn(acc, __fmul_rn(p.gx[t], w[t]));
      rowp[r * PT_TW + c] = acc;
    }
  }
  __syncthreads();

  // 3. latitude pass and the stores: one zeta serves both members of an antithetic pair
  if (c < tw) {
    const float sg = p.sigma[k];
    const long long row_elems = (long long)p.K * p.H * p.W;
    for (int i = r0; i < th; i += PT_THREADS / PT_TW) {
      float acc = 0.f;
      for (int t = 0; t <= 2 * Ry; ++t) acc = __fadd_rn(acc, __fmul_rn(p.gy[t], rowp[(i + t) * PT_TW + c]));
      const long long orow = ((long long)k * p.H + (i0 + i)) * p.W + (j0 + c);
      const float xv = p.x[(long long)s * row_elems + orow];
      const int pa = p.anti ? 2 * d : d, pb = p.anti ? 2 * d + 1 : d;
      for (int pi = pa; pi <= pb; ++pi) {
        if (pi < p.p_lo || pi >= p.p_hi) continue;
        const int m = pi + p.control - p.first;
        p.out[(long long)s * p.oss + (long long)m * p.oms + orow] = perturbed(xv, sg, acc, p.anti && (pi & 1));
      }
    }
  }
}

inline bool pt_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int dlwp_ens_perturb(dlwp_handle_t h, const void* x, const void* sigma, void* out, dlwp_ens_perturb_desc d, void* stream) {
  DLWP_UNTAPED(dlwp_ens_perturb);
  DLWP_CHECK_ARG(d.samples >= 1 && d.channels >= 1 && d.height >= 1 && d.width >= 1,
                 "dlwp_ens_perturb: samples %d, channels %d, height %d, width %d must all be >= 1", d.samples, d.channels, d.height,
                 d.width);
  DLWP_CHECK_ARG(d.members >= 1, "dlwp_ens_perturb: members %d, expected >= 1", d.members);
  DLWP_CHECK_ARG(d.first_member >= 0 && (long long)d.first_member + d.members < (1ll << 31),
                 "dlwp_ens_perturb: first_member %d with %d members, expected 0 <= first_member and first_member + members < 2^31",
                 d.first_member, d.members);
  DLWP_CHECK_ARG(d.radius_y >= 0 && d.radius_y <= PT_MAX_R && d.radius_x >= 0 && d.radius_x <= PT_MAX_R,
                 "dlwp_ens_perturb: radii (%d, %d), expected 0 .. %d", d.radius_y, d.radius_x, PT_MAX_R);
  DLWP_CHECK_ARG(d.radius_x <= d.width, "dlwp_ens_perturb: radius_x %d wraps a row of %d columns more than once", d.radius_x, d.width);
  DLWP_CHECK_ARG(d.channels < 65536, "dlwp_ens_perturb: %d channels, at most 65535", d.channels);
  DLWP_CHECK_ARG(d.height + d.radius_y < 32768, "dlwp_ens_perturb: height %d + radius_y %d, expected < 32768", d.height, d.radius_y);
  DLWP_CHECK_ARG((d.control == 0 || d.control == 1) && (d.antithetic == 0 || d.antithetic == 1),
                 "dlwp_ens_perturb: control %d and antithetic %d must be 0 or 1", d.control, d.antithetic);
  const long long row = (long long)d.channels * d.height * d.width;
  DLWP_CHECK_ARG(row < (1ll << 31) && (long long)d.samples * row < (1ll << 38), "dlwp_ens_perturb: %d samples of %lld floats are too many",
                 d.samples, row);
  // the two layouts, possibly padded: members inside a sample or samples inside a member; either way no two elements meet
  const bool members_inner = (d.members == 1 || d.member_stride >= row) &&
                             (d.samples == 1 || d.sample_stride >= (long long)(d.members - 1) * d.member_stride + row);
  const bool samples_inner = (d.samples == 1 || d.sample_stride >= row) &&
                             (d.members == 1 || d.member_stride >= (long long)(d.samples - 1) * d.sample_stride + row);
  DLWP_CHECK_ARG(d.sample_stride >= 0 && d.member_stride >= 0, "dlwp_ens_perturb: negative stride");
  DLWP_CHECK_ARG(members_inner || samples_inner,
                 "dlwp_ens_perturb: output strides (sample %lld, member %lld) overlap for %d samples, %d members of %lld floats",
                 d.sample_stride, d.member_stride, d.samples, d.members, row);
  DLWP_CHECK_ARG(x && sigma && out, "dlwp_ens_perturb: null pointer");
  DLWP_CHECK_ARG((((uintptr_t)x | (uintptr_t)sigma | (uintptr_t)out) & 3) == 0, "dlwp_ens_perturb: tensors must be float aligned");
  PerturbArgs p;
  p.x = (const float*)x, p.sigma = (const float*)sigma, p.out = (float*)out;
  p.oss = d.sample_stride, p.oms = d.member_stride;
  p.S = d.samples, p.K = d.channels, p.H = d.height, p.W = d.width;
  p.members = d.members, p.first = d.first_member;
  p.k0 = (unsigned)(d.seed & 0xffffffffull), p.k1 = (unsigned)(d.seed >> 32);
  p.control = d.control, p.anti = d.antithetic;
  p.Ry = d.radius_y, p.Rx = d.radius_x;
  p.qw = (d.width + 3) / 4;
  p.units = (long long)d.samples * d.channels * d.height * p.qw;
  // draw indices of the call: member g is draw index g - control; with control, member 0 is x itself
  const bool has_control = d.control && d.first_member == 0;
  p.p_lo = has_control ? 0 : d.first_member - d.control;
  p.p_hi = d.first_member + d.members - d.control;
  p.d_lo = d.antithetic ? p.p_lo >> 1 : p.p_lo;
  p.draws = p.p_hi > p.p_lo ? (d.antithetic ? ((p.p_hi - 1) >> 1) + 1 : p.p_hi) - p.d_lo : 0;
  p.tiles_y = (d.height + PT_TH - 1) / PT_TH, p.tiles_x = (d.width + PT_TW - 1) / PT_TW;
  p.chunk = d.members;
  for (int t = 0; t <= 2 * PT_MAX_R; ++t) p.gy[t] = d.taps_y[t], p.gx[t] = d.taps_x[t];
  const bool white = d.radius_y == 0 && d.radius_x == 0;
  long long blocks;
  int chunks = 1;
  if (white) {
    // halve the members a lane owns (never below 8, an even count so that antithetic pairs stay together) until the launch has
    // the lanes of the chip; which lane writes a member does not change its bits
    while (p.chunk >= 16 && p.units * ((d.members + p.chunk - 1) / p.chunk) < PT_WHITE_LANES) p.chunk = ((p.chunk + 3) / 4) * 2;
    chunks = (d.members + p.chunk - 1) / p.chunk;
    blocks = (p.units + PT_THREADS - 1) / PT_THREADS;
    DLWP_CHECK_ARG(chunks <= 65535, "dlwp_ens_perturb: %d member chunks", chunks);
  } else {
    blocks = (long long)p.draws * d.samples * d.channels * p.tiles_y * p.tiles_x;
  }
  DLWP_CHECK_ARG(blocks < (1ll << 31), "dlwp_ens_perturb: %lld workgroups are too many for one grid", blocks);
  DLWP_CHECK_ARG(h, "dlwp_ens_perturb: null handle");
  hipStream_t st = (hipStream_t)stream;
  if (white) {
    const bool vec = (d.width & 3) == 0 && (d.sample_stride & 3) == 0 && (d.member_stride & 3) == 0 && pt_aligned16(x) &&
                     pt_aligned16(out);
    const dim3 grid((unsigned)blocks, (unsigned)chunks);
    if (vec)
      ens_perturb_white_kernel<true><<<grid, PT_THREADS, 0, st>>>(p);
    else
      ens_perturb_white_kernel<false><<<grid, PT_THREADS, 0, st>>>(p);
  } else {
    if (has_control) {
      const long long total = (long long)d.samples * row;
      ens_perturb_control_kernel<<<(unsigned)((total + PT_THREADS - 1) / PT_THREADS), PT_THREADS, 0, st>>>(
          (const float*)x, (float*)out, row, total, d.sample_stride);
    }
    if (blocks > 0) {
      const size_t lds = (size_t)(PT_TH + 2 * d.radius_y) * (PT_TW + 2 * d.radius_x + PT_TW) * sizeof(float);
      ens_perturb_smooth_kernel<<<(unsigned)blocks, PT_THREADS, lds, st>>>(p);
    }
  }
  DLWP_LAUNCH_CHECK("ens_perturb kernels");
  return DLWP_OK;
}

}  // extern "C"
