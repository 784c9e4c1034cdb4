// sepconv.hip -- keras DepthwiseConv2D and SeparableConv2D (stride 1, channels_first): a depthwise stencil and a pointwise (1 x 1)
// product on the matrix cores, each with its two adjoints.  gfx950 only; float32 storage and arithmetic.
//
// Depthwise (kernel K (kh, kw, cin, dm), output channel c dm + m):
//   y[n][c dm + m][i][j] = act(b[c dm + m] + sum_{u,v} xpad[n][c][i + u dh][j + v dw] K[u][v][c][m])
// xpad = the input under the halo (the padding layers in front and the layer's own 'same' zeros, composed; the five DLWP_PAD_* modes
// per axis through the index map of dlwp_pad2d_fwd).  One workgroup owns a TH x 64 tile of outputs of one (sample, input channel), TH =
// 32, 16 or 8 by the map's height: the haloed input tile ((TH + (kh-1) dh) x (64 + (kw-1) dw) floats) and the channel's kh kw dm taps are staged in LDS once and serve
// all dm output channels.  Every output element is ONE fmaf chain that starts from the bias (or +0) and runs over the taps in
// ascending (u, v).
//   bwd_data: gather form, no atomics, no workspace.  One lane per source pixel (n, c, y, x): the sum over the padded positions (r, s)
//     that map to it (its own, then -- only for a pixel within a summing halo's reach of a border -- the halo rows / columns in
//     ascending order: wrap adds the periodic images, edge adds to the border, the mirrors add their reflections, zero drops) of
//     G(r, s) = sum_{m,u,v} dz[n][c dm + m][r - u dh][s - v dw] K[u][v][c][m].  It OVERWRITES its channel window.
//   bwd_weight: a fixed two-launch tree.  Launch 1: workgroup (split, c) sums its DW_SPAN consecutive positions of the flattened
//     (n, i, j) range for every (m, u, v) (a fixed per-lane order, then a fixed shuffle / LDS tree) into ws[split][u][v][c][m]; launch 2
//     adds the splits in ascending order (and the old value behind them where accumulate).  The split depends on the shape alone.
//
// Pointwise (kernel P (q, o), pixels contiguous):  y[n][o][p] = act(b[o] + sum_q x[n][q][p] P[q][o])
//   v_mfma_f32_32x32x2_f32 with M = output channels (A = the weights, from LDS), N = 32 consecutive pixels of ONE sample (B = two
//   coalesced 128-byte rows of x per instruction, straight from global memory: the operand is (channels x pixels), the transpose of
//   what dense.hip reads), K = the input channels in ascending order: every output element is one q-ordered chain that starts from
//   the bias, so a sample's bits never depend on the batch.  A workgroup (4 waves) owns 128 pixels of one sample and up to 128 output
//   channels; the weights are staged in LDS in chunks of 64 input channels, zero-filled where ragged.  Loads are 4-byte (a channel
//   window's rows are only 4-byte aligned; a wave's 32 lanes read 128 contiguous bytes either way).
//   bwd_data: dx[n][q][p] = sum_o dz[n][o][p] P[q][o] -- the same kernel, the weights staged through the other index.
//   bwd_weight: dw[q][o] (+)= sum_{n,p} x[n][q][p] dz[n][o][p].  M = q, N = o, K = pixels: a workgroup owns a 64 x 64 block of dw and
//     PW_UNITS consecutive units (a unit = 32 pixels of one sample) of the flattened (n, pixel chunk) range, stages both operands in
//     LDS (coalesced rows) and writes ws[split][q][o]; the second launch adds the splits in ascending order.
#include "common.h"
#include "tape.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int DW_TW = 64;                  // columns of the depthwise forward's output tile; its rows: 32, 16 or 8 (dw_tile_rows)
constexpr int DW_SPAN = 4096;              // positions of (n, i, j) per first-stage partial of the depthwise weight gradient
constexpr int DW_PT = DW_SPAN / 256;
constexpr int PW_QC = 64;                  // summed channels per staged weight chunk
constexpr int PW_UNITS = 16;               // 32-pixel units per first-stage partial of the pointwise weight gradient
constexpr int PW_PITCH = 33;

__device__ __forceinline__ float sep_act(float v, int act) {
  return act == DLWP_ACT_TANH ? tanhf(v) : (act == DLWP_ACT_RELU ? dlwp_nmax(v, 0.f) : v);
}

// dlwp_map_coord on the range a validated halo reaches (one period / one reflection): no division
__device__ __forceinline__ int smap(int p, int n, int mode) {
  if ((unsigned)p < (unsigned)n) return p;
  if (mode == DLWP_PAD_ZERO) return -1;
  if (mode == DLWP_PAD_EDGE) return p < 0 ? 0 : n - 1;
  if (mode == DLWP_PAD_REFLECT) return p < 0 ? -p : 2 * n - 2 - p;
  if (mode == DLWP_PAD_SYMMETRIC) return p < 0 ? -p - 1 : 2 * n - 1 - p;
  return p < 0 ? p + n : p - n;   // DLWP_PAD_WRAP
}

struct DwGeom {
  int N, C, H, W, Ho, Wo, PH, PW;          // PH x PW: the padded image
  int kh, kw, dh, dw, dm, top, left, mode_h, mode_w, act;
  int in_c_off, in_c_total, out_c_off, out_c_total;
  int tiles_h, tiles_w;
};

// TH: rows of the output tile (32, 16 or 8, by the map's height); KS = 3: 3 x 3 taps, the weights of a channel in registers and the
// tap loops unrolled; KS = 0: any kernel.  Staging walks the haloed tile row by row (no division; the row map once per row).
template <int TH, int KS>
__global__ __launch_bounds__(256) void dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ y, DwGeom g) {
  extern __shared__ float lds[];
  const int t = threadIdx.x;
  long long b = blockIdx.x;
  const int tj = (int)(b % g.tiles_w);
  b /= g.tiles_w;
  const int ti = (int)(b % g.tiles_h);
  b /= g.tiles_h;
  const int c = (int)(b % g.C);
  const long long n = b / g.C;
  const int i0 = ti * TH, j0 = tj * DW_TW;
  const int ih = TH + (g.kh - 1) * g.dh, iw = DW_TW + (g.kw - 1) * g.dw;
  float* xt = lds;
  float* kt = lds + ih * iw;
  const float* xs = x + (n * g.in_c_total + g.in_c_off + c) * (long long)g.H * g.W;
  const int tx = t & 63, ty = t >> 6;
  for (int r = ty; r < ih; r += 4) {
    const int pr = i0 + r;                  // (beyond the padded image: read by outputs that are never stored)
    const int yy = pr < g.PH ? smap(pr - g.top, g.H, g.mode_h) : -1;
    const float* rowp = xs + (long long)(yy < 0 ? 0 : yy) * g.W;
    for (int s = tx; s < iw; s += 64) {
      const int ps = j0 + s;
      float v = 0.f;
      if (yy >= 0 && ps < g.PW) {
        const int xx = smap(ps - g.left, g.W, g.mode_w);
        if (xx >= 0) v = rowp[xx];
      }
      xt[r * iw + s] = v;
    }
  }
  const int taps = g.kh * g.kw;
  for (int e = t; e < taps * g.dm; e += 256) {          // kt[m][tap]
    const int m = e / taps, tap = e - m * taps;
    kt[e] = w[((long long)tap * g.C + c) * g.dm + m];
  }
  __syncthreads();
  const int j = j0 + tx;
  for (int m = 0; m < g.dm; ++m) {
    const int oc = c * g.dm + m;
    const float bv = bias ? bias[oc] : 0.f;
    const float* km = kt + m * taps;
    float* yo = y + (n * g.out_c_total + g.out_c_off + oc) * (long long)g.Ho * g.Wo;
    float k9[9];
    if (KS == 3) {
#pragma unroll
      for (int q = 0; q < 9; ++q) k9[q] = km[q];
    }
#pragma unroll
    for (int rr = 0; rr < TH / 4; ++rr) {
      const int li = ty + 4 * rr, i = i0 + li;
      if (i >= g.Ho) break;                 // (uniform over the wave: ty is the wave's)
      float acc = bv;
      if (KS == 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const float* row = xt + (li + u * g.dh) * iw + tx;
#pragma unroll
          for (int v = 0; v < 3; ++v) acc = fmaf(row[v * g.dw], k9[3 * u + v], acc);
        }
      } else {
        for (int u = 0; u < g.kh; ++u) {
          const float* row = xt + (li + u * g.dh) * iw + tx;
          for (int v = 0; v < g.kw; ++v) acc = fmaf(row[v * g.dw], km[u * g.kw + v], acc);
        }
      }
      if (j < g.Wo) yo[(long long)i * g.Wo + j] = sep_act(acc, g.act);
    }
  }
}

// G(r, s) of the header: the gradient of padded position (r, s) of channel c
__device__ __forceinline__ float dw_padded_grad(const float* __restrict__ dzc, const float* __restrict__ wc, int r, int s,
                                                const DwGeom& g) {
  const long long plane = (long long)g.Ho * g.Wo;
  float acc = 0.f;
  for (int m = 0; m < g.dm; ++m) {
    const float* dzm = dzc + m * plane;
    for (int u = 0; u < g.kh; ++u) {
      const int i = r - u * g.dh;
      if ((unsigned)i >= (unsigned)g.Ho) continue;
      for (int v = 0; v < g.kw; ++v) {
        const int j = s - v * g.dw;
        if ((unsigned)j >= (unsigned)g.Wo) continue;
        acc = fmaf(dzm[(long long)i * g.Wo + j], wc[(long long)(u * g.kw + v) * g.C * g.dm + m], acc);
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(256) void dw_bwd_data_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                          float* __restrict__ dx, long long total, int reach_h, int reach_w,
                                                          DwGeom g) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int xx = (int)(e % g.W);
    long long q = e / g.W;
    const int yy = (int)(q % g.H);
    q /= g.H;
    const int c = (int)(q % g.C);
    const long long n = q / g.C;
    const float* dzc = dz + (n * g.out_c_total + g.out_c_off + (long long)c * g.dm) * g.Ho * g.Wo;
    const float* wc = w + (long long)c * g.dm;
    const int r0 = yy + g.top, s0 = xx + g.left;
    const bool near_h = yy < reach_h || yy >= g.H - reach_h, near_w = xx < reach_w || xx >= g.W - reach_w;
    float acc = 0.f;
    auto row_terms = [&](int r) {
      if (near_w)
        for (int s = 0; s < g.left; ++s)
          if (smap(s - g.left, g.W, g.mode_w) == xx) acc += dw_padded_grad(dzc, wc, r, s, g);
      acc += dw_padded_grad(dzc, wc, r, s0, g);
      if (near_w)
        for (int s = g.left + g.W; s < g.PW; ++s)
          if (smap(s - g.left, g.W, g.mode_w) == xx) acc += dw_padded_grad(dzc, wc, r, s, g);
    };
    if (near_h)
      for (int r = 0; r < g.top; ++r)
        if (smap(r - g.top, g.H, g.mode_h) == yy) row_terms(r);
    row_terms(r0);
    if (near_h)
      for (int r = g.top + g.H; r < g.PH; ++r)
        if (smap(r - g.top, g.H, g.mode_h) == yy) row_terms(r);
    dx[((n * g.in_c_total + g.in_c_off + c) * g.H + yy) * (long long)g.W + xx] = acc;
  }
}

// sum of v over the workgroup's 256 lanes, in a fixed order (lane tree, then the four waves in turn); valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void dw_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                            float* __restrict__ part, long long total, DwGeom g) {
  __shared__ float red[4];
  const int t = threadIdx.x, c = blockIdx.y;
  const long long lo = (long long)blockIdx.x * DW_SPAN;
  const long long plane = (long long)g.Ho * g.Wo;
  int pi[DW_PT], pj[DW_PT];
  long long pn[DW_PT];
#pragma unroll
  for (int k = 0; k < DW_PT; ++k) {
    const long long e = lo + t + 256 * k;
    if (e < total) {
      pn[k] = e / plane;
      const int rem = (int)(e - pn[k] * plane);
      pi[k] = rem / g.Wo;
      pj[k] = rem - pi[k] * g.Wo;
    } else {
      pn[k] = -1;
      pi[k] = pj[k] = 0;
    }
  }
  const long long wcount = (long long)g.kh * g.kw * g.C * g.dm;
  float* out = part + (long long)blockIdx.x * wcount;
  for (int u = 0; u < g.kh; ++u)
    for (int v = 0; v < g.kw; ++v) {
      float xv[DW_PT];                      // this lane's inputs under tap (u, v): read once, used by every m
#pragma unroll
      for (int k = 0; k < DW_PT; ++k) {
        xv[k] = 0.f;
        if (pn[k] >= 0) {
          const int yy = smap(pi[k] + u * g.dh - g.top, g.H, g.mode_h), xx = smap(pj[k] + v * g.dw - g.left, g.W, g.mode_w);
          if (yy >= 0 && xx >= 0) xv[k] = x[((pn[k] * g.in_c_total + g.in_c_off + c) * g.H + yy) * (long long)g.W + xx];
        }
      }
      for (int m = 0; m < g.dm; ++m) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < DW_PT; ++k)
          if (pn[k] >= 0)
            acc = fmaf(xv[k], dz[(pn[k] * g.out_c_total + g.out_c_off + (long long)c * g.dm + m) * plane +
                                 (long long)pi[k] * g.Wo + pj[k]], acc);
        const float sum = block_sum(acc, red);
        if (t == 0) out[((long long)(u * g.kw + v) * g.C + c) * g.dm + m] = sum;
      }
    }
}

// dst[e] (+)= part[0][e] + part[1][e] + ... in ascending order (the old value is added behind the sum)
__global__ __launch_bounds__(256) void sep_sum_parts_kernel(const float* __restrict__ part, float* __restrict__ dst, long long count,
                                                            int S, int accumulate) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float v = part[e];
  for (int s = 1; s < S; ++s) v += part[(long long)s * count + e];
  dst[e] = accumulate ? dst[e] + v : v;
}

struct PwGeom {
  int n, hw, Kd, Md, ldw, act;             // Kd: summed channels, Md: produced channels, ldw: row length of w (= o)
  int in_c_off, in_c_total, out_c_off, out_c_total;
  int pblocks;                             // 128-pixel groups of a sample: one workgroup each
};

// out[n][out_c_off + i][p] = act(bias[i] + sum_k in[n][in_c_off + k][p] * W(k, i)),  W(k, i) = TRANS ? w[i ldw + k] : w[k ldw + i]
// Per chunk of PW_QC summed channels: the chunk's weights go to LDS (zero-filled where ragged) while the wave's own operand loads of
// the chunk are already in flight, then PW_QC / 2 matrix instructions per 32 produced channels.
template <int OT, bool TRANS>
__global__ __launch_bounds__(256) void pw_mm_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ out, PwGeom g) {
  constexpr int MW = OT * 32;
  __shared__ float wl[PW_QC * MW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j = lane & 31, hh = lane >> 5;
  const long long n = blockIdx.x / g.pblocks;
  const int pb = blockIdx.x - (int)n * g.pblocks;
  const int p = pb * 128 + wave * 32 + j;
  const bool p_ok = p < g.hw;
  const int m0 = blockIdx.y * MW;
  f32x16 acc[OT];
#pragma unroll
  for (int ot = 0; ot < OT; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ch = m0 + ot * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      acc[ot][r] = (bias && ch < g.Md) ? bias[ch] : 0.f;
    }
  const float* xin = in + (n * g.in_c_total + g.in_c_off) * (long long)g.hw + (p_ok ? p : 0);
  for (int kc = 0; kc < g.Kd; kc += PW_QC) {
    float xv[PW_QC / 2];
#pragma unroll
    for (int s = 0; s < PW_QC / 2; ++s) {
      const int k = kc + 2 * s + hh;
      xv[s] = (p_ok && k < g.Kd) ? xin[(long long)k * g.hw] : 0.f;
    }
    __syncthreads();
    for (int e = t; e < PW_QC * MW; e += 256) {
      const int k = e / MW, i = e - k * MW;
      const int gk = kc + k, gi = m0 + i;
      float v = 0.f;
      if (gk < g.Kd && gi < g.Md) v = TRANS ? w[(long long)gi * g.ldw + gk] : w[(long long)gk * g.ldw + gi];
      wl[e] = v;
    }
    __syncthreads();
    const int steps = min(PW_QC, g.Kd - kc + 1) >> 1;
#pragma unroll
    for (int s = 0; s < PW_QC / 2; ++s) {
      if (s < steps) {
#pragma unroll
        for (int ot = 0; ot < OT; ++ot)
          acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(2 * s + hh) * MW + ot * 32 + j], xv[s], acc[ot], 0, 0, 0);
      }
    }
  }
  if (!p_ok) return;
  float* yo = out + (n * g.out_c_total + g.out_c_off) * (long long)g.hw + p;
#pragma unroll
  for (int ot = 0; ot < OT; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ch = m0 + ot * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (ch < g.Md) yo[(long long)ch * g.hw] = sep_act(acc[ot][r], g.act);
    }
}

struct PwwGeom {
  int n, hw, q, o, chunks;                 // chunks = ceil(hw / 32); units = n * chunks
  int x_c_off, x_c_total, z_c_off, z_c_total;
};

__global__ __launch_bounds__(256) void pw_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                            float* __restrict__ part, PwwGeom g) {
  __shared__ float xs[64 * PW_PITCH], gs[64 * PW_PITCH];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j = lane & 31, hh = lane >> 5;
  const int q0 = blockIdx.y * 64, o0 = blockIdx.z * 64;
  const int qt = wave >> 1, ot = wave & 1;
  const int scol = t & 31, srow = t >> 5;
  const long long units = (long long)g.n * g.chunks;
  const long long u_lo = (long long)blockIdx.x * PW_UNITS;
  const long long u_hi = u_lo + PW_UNITS < units ? u_lo + PW_UNITS : units;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (long long un = u_lo; un < u_hi; ++un) {
    const long long n = un / g.chunks;
    const int p = (int)(un - n * g.chunks) * 32 + scol;
    float xr[8], gr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = srow + 8 * i;
      xr[i] = (p < g.hw && q0 + row < g.q) ? x[(n * g.x_c_total + g.x_c_off + q0 + row) * (long long)g.hw + p] : 0.f;
      gr[i] = (p < g.hw && o0 + row < g.o) ? dz[(n * g.z_c_total + g.z_c_off + o0 + row) * (long long)g.hw + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      xs[(srow + 8 * i) * PW_PITCH + scol] = xr[i];
      gs[(srow + 8 * i) * PW_PITCH + scol] = gr[i];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(qt * 32 + j) * PW_PITCH + 2 * s + hh], gs[(ot * 32 + j) * PW_PITCH + 2 * s + hh],
                                                 acc, 0, 0, 0);
  }
  float* outp = part + (long long)blockIdx.x * g.q * g.o;
  const int oc = o0 + ot * 32 + j;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qq = q0 + qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
    if (qq < g.q && oc < g.o) outp[(long long)qq * g.o + oc] = acc[r];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

int dw_shape(const char* who, dlwp_shape4 xs, const dlwp_depthwise2d& d, int* ho, int* wo) {
  DLWP_CHECK_ARG(xs.n >= 0 && xs.c >= 1 && xs.h >= 1 && xs.w >= 1, "%s: bad input shape (%d, %d, %d, %d)", who, xs.n, xs.c, xs.h,
                 xs.w);
  DLWP_CHECK_ARG(d.kh >= 1 && d.kh <= 7 && d.kw >= 1 && d.kw <= 7, "%s: kernel size %d x %d (1 .. 7 per axis)", who, d.kh, d.kw);
  DLWP_CHECK_ARG(d.dil_h >= 1 && d.dil_h <= 4 && d.dil_w >= 1 && d.dil_w <= 4, "%s: dilation %d x %d (1 .. 4)", who, d.dil_h, d.dil_w);
  DLWP_CHECK_ARG(d.depth_multiplier >= 1 && d.depth_multiplier <= 8, "%s: depth_multiplier %d (1 .. 8)", who, d.depth_multiplier);
  DLWP_CHECK_ARG((unsigned)d.act <= 2u, "%s: unknown activation %d", who, d.act);
  const dlwp_pad2d& p = d.halo;
  DLWP_CHECK_ARG(p.top >= 0 && p.bottom >= 0 && p.left >= 0 && p.right >= 0, "%s: negative padding", who);
  DLWP_CHECK_ARG((unsigned)p.mode_h <= 4u && (unsigned)p.mode_w <= 4u, "%s: unknown pad mode", who);
  DLWP_CHECK_ARG(p.top < (1 << 20) && p.bottom < (1 << 20) && p.left < (1 << 20) && p.right < (1 << 20) && xs.h < (1 << 24) &&
                     xs.w < (1 << 24) && xs.c < (1 << 24), "%s: sizes beyond the 32-bit coordinate range", who);
  DLWP_CHECK_ARG(dlwp_pad_fits(p.top, p.bottom, xs.h, p.mode_h), "%s: the row halo (%d, %d) of mode %d exceeds what an axis of %d serves",
                 who, p.top, p.bottom, p.mode_h, xs.h);
  DLWP_CHECK_ARG(dlwp_pad_fits(p.left, p.right, xs.w, p.mode_w),
                 "%s: the column halo (%d, %d) of mode %d exceeds what an axis of %d serves", who, p.left, p.right, p.mode_w, xs.w);
  const int oh = xs.h + p.top + p.bottom - d.dil_h * (d.kh - 1), ow = xs.w + p.left + p.right - d.dil_w * (d.kw - 1);
  DLWP_CHECK_ARG(oh >= 1 && ow >= 1, "%s: kernel %d x %d (dilation %d x %d) larger than the padded input %d x %d", who, d.kh, d.kw,
                 d.dil_h, d.dil_w, xs.h + p.top + p.bottom, xs.w + p.left + p.right);
  *ho = oh;
  *wo = ow;
  return DLWP_OK;
}

int dw_windows(const char* who, dlwp_shape4 xs, dlwp_depthwise2d& d) {
  if (d.in_c_total <= 0) d.in_c_total = xs.c;
  if (d.out_c_total <= 0) d.out_c_total = xs.c * d.depth_multiplier;
  DLWP_CHECK_ARG(d.in_c_off >= 0 && (long long)d.in_c_off + xs.c <= d.in_c_total,
                 "%s: the input channel window [%d, +%d) lies outside the %d channels of the tensor", who, d.in_c_off, xs.c,
                 d.in_c_total);
  DLWP_CHECK_ARG(d.out_c_off >= 0 && (long long)d.out_c_off + (long long)xs.c * d.depth_multiplier <= d.out_c_total,
                 "%s: the output channel window [%d, +%d) lies outside the %d channels of the tensor", who, d.out_c_off,
                 xs.c * d.depth_multiplier, d.out_c_total);
  return DLWP_OK;
}

int dw_tile_rows(int ho) { return ho > 16 ? 32 : (ho > 8 ? 16 : 8); }

DwGeom dw_geom(dlwp_shape4 xs, const dlwp_depthwise2d& d, int ho, int wo) {
  DwGeom g;
  g.N = xs.n, g.C = xs.c, g.H = xs.h, g.W = xs.w, g.Ho = ho, g.Wo = wo;
  g.PH = xs.h + d.halo.top + d.halo.bottom, g.PW = xs.w + d.halo.left + d.halo.right;
  g.kh = d.kh, g.kw = d.kw, g.dh = d.dil_h, g.dw = d.dil_w, g.dm = d.depth_multiplier;
  g.top = d.halo.top, g.left = d.halo.left, g.mode_h = d.halo.mode_h, g.mode_w = d.halo.mode_w, g.act = d.act;
  g.in_c_off = d.in_c_off, g.in_c_total = d.in_c_total, g.out_c_off = d.out_c_off, g.out_c_total = d.out_c_total;
  const int th = dw_tile_rows(ho);
  g.tiles_h = (ho + th - 1) / th, g.tiles_w = (wo + DW_TW - 1) / DW_TW;
  return g;
}

int grid_of(dlwp_handle_t h, long long total) {
  const long long blocks = (total + 255) / 256, cap = (long long)h->cu_count * 16;
  return (int)(blocks < cap ? blocks : cap);
}

long long dw_splits(dlwp_shape4 xs, int ho, int wo) {
  const long long total = (long long)xs.n * ho * wo;
  return total > 0 ? (total + DW_SPAN - 1) / DW_SPAN : 1;
}

int pw_check(const char* who, int n, int hw, dlwp_pointwise2d& d) {
  DLWP_CHECK_ARG(n >= 0 && hw >= 1 && d.q >= 1 && d.o >= 1 && d.q < (1 << 20) && d.o < (1 << 20),
                 "%s: bad sizes (n %d, hw %d, q %d, o %d): every size must be at least 1", who, n, hw, d.q, d.o);
  DLWP_CHECK_ARG((unsigned)d.act <= 2u, "%s: unknown activation %d", who, d.act);
  if (d.in_c_total <= 0) d.in_c_total = d.q;
  if (d.out_c_total <= 0) d.out_c_total = d.o;
  DLWP_CHECK_ARG(d.in_c_off >= 0 && (long long)d.in_c_off + d.q <= d.in_c_total,
                 "%s: the input channel window [%d, +%d) lies outside the %d channels of the tensor", who, d.in_c_off, d.q,
                 d.in_c_total);
  DLWP_CHECK_ARG(d.out_c_off >= 0 && (long long)d.out_c_off + d.o <= d.out_c_total,
                 "%s: the output channel window [%d, +%d) lies outside the %d channels of the tensor", who, d.out_c_off, d.o,
                 d.out_c_total);
  DLWP_CHECK_ARG((long long)n * ((hw + 127) / 128) < (1ll << 31), "%s: n x hw beyond the grid range", who);
  return DLWP_OK;
}

// (measured at 256 members on 32 x 88 x 180 / 64 x 44 x 90 / 128 x 22 x 45: 362 / 262 / 297 us as built; 468 / 432 / 302 us with the
// weights resident and a workgroup walking up to 8 pixel groups, 616 / 489 / 304 us with resident weights and one group -- the kernel
// waits on its operand loads: more waves in flight, and loads issued in front of the weight staging, hide more of that)
template <bool TRANS>
void pw_launch(const float* in, const float* w, const float* bias, float* out, const PwGeom& g, hipStream_t s) {
  const int groups = g.Md <= 32 ? 1 : (g.Md <= 64 ? 2 : 4);
  const dim3 grid((unsigned)((long long)g.n * g.pblocks), (unsigned)((g.Md + groups * 32 - 1) / (groups * 32)));
  if (groups == 1)
    pw_mm_kernel<1, TRANS><<<grid, 256, 0, s>>>(in, w, bias, out, g);
  else if (groups == 2)
    pw_mm_kernel<2, TRANS><<<grid, 256, 0, s>>>(in, w, bias, out, g);
  else
    pw_mm_kernel<4, TRANS><<<grid, 256, 0, s>>>(in, w, bias, out, g);
}

}  // namespace

extern "C" {

int dlwp_depthwise2d_out_shape(dlwp_shape4 xs, dlwp_depthwise2d d, dlwp_shape4* ys) {
  DLWP_CHECK_ARG(ys != nullptr, "dlwp_depthwise2d_out_shape: null pointer");
  int ho, wo;
  int rc = dw_shape("dlwp_depthwise2d_out_shape", xs, d, &ho, &wo);
  if (rc != DLWP_OK) return rc;
  rc = dw_windows("dlwp_depthwise2d_out_shape", xs, d);
  if (rc != DLWP_OK) return rc;
  ys->n = xs.n, ys->c = xs.c * d.depth_multiplier, ys->h = ho, ys->w = wo;
  return DLWP_OK;
}

int dlwp_depthwise2d_fwd(dlwp_handle_t h, const void* x, const void* w, const void* bias, void* y, dlwp_shape4 xs, dlwp_depthwise2d d,
                         int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_depthwise2d_fwd, h, x, w, bias, y, xs, d, dtype);
  const char* who = "dlwp_depthwise2d_fwd";
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  int ho, wo;
  int rc = dw_shape(who, xs, d, &ho, &wo);
  if (rc != DLWP_OK) return rc;
  rc = dw_windows(who, xs, d);
  if (rc != DLWP_OK) return rc;
  const DwGeom g = dw_geom(xs, d, ho, wo);
  const long long blocks = (long long)xs.n * xs.c * g.tiles_h * g.tiles_w;
  DLWP_CHECK_ARG(blocks < (1ll << 31), "%s: sizes beyond the grid range", who);
  DLWP_CHECK_ARG(xs.n == 0 || (x && w && y), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  if (xs.n == 0) return DLWP_OK;
  const int th = dw_tile_rows(ho);
  const int ih = th + (d.kh - 1) * d.dil_h, iw = DW_TW + (d.kw - 1) * d.dil_w;
  const size_t lds = (size_t)(ih * iw + d.kh * d.kw * d.depth_multiplier) * sizeof(float);
  const bool k3 = d.kh == 3 && d.kw == 3;
#define DW_FWD(TH, KS)                                                                                                     \
  dw_fwd_kernel<TH, KS><<<(unsigned)blocks, 256, lds, (hipStream_t)stream>>>((const float*)x, (const float*)w, (const float*)bias, \
                                                                              (float*)y, g)
  if (th == 32) {
    if (k3) DW_FWD(32, 3); else DW_FWD(32, 0);
  } else if (th == 16) {
    if (k3) DW_FWD(16, 3); else DW_FWD(16, 0);
  } else {
    if (k3) DW_FWD(8, 3); else DW_FWD(8, 0);
  }
#undef DW_FWD
  DLWP_LAUNCH_CHECK("dw_fwd_kernel");
  return DLWP_OK;
}

int dlwp_depthwise2d_bwd_data(dlwp_handle_t h, const void* dz, const void* w, void* dx, dlwp_shape4 xs, dlwp_depthwise2d d, int dtype,
                              void* stream) {
  DLWP_TAPE(h, stream, dlwp_depthwise2d_bwd_data, h, dz, w, dx, xs, d, dtype);
  const char* who = "dlwp_depthwise2d_bwd_data";
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  int ho, wo;
  int rc = dw_shape(who, xs, d, &ho, &wo);
  if (rc != DLWP_OK) return rc;
  rc = dw_windows(who, xs, d);
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(xs.n == 0 || (dz && w && dx), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  if (xs.n == 0) return DLWP_OK;
  const DwGeom g = dw_geom(xs, d, ho, wo);
  const dlwp_pad2d& p = d.halo;
  const int far_h = p.top > p.bottom ? p.top : p.bottom, far_w = p.left > p.right ? p.left : p.right;
  const int reach_h = (p.mode_h == DLWP_PAD_ZERO || far_h == 0) ? 0 : far_h + 1;      // (a zero halo folds nothing back)
  const int reach_w = (p.mode_w == DLWP_PAD_ZERO || far_w == 0) ? 0 : far_w + 1;
  const long long total = (long long)xs.n * xs.c * xs.h * xs.w;
  dw_bwd_data_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)dz, (const float*)w, (float*)dx, total, reach_h,
                                                                         reach_w, g);
  DLWP_LAUNCH_CHECK("dw_bwd_data_kernel");
  return DLWP_OK;
}

size_t dlwp_depthwise2d_bwd_workspace(dlwp_shape4 xs, dlwp_depthwise2d d) {
  int ho, wo;
  if (dw_shape("dlwp_depthwise2d_bwd_workspace", xs, d, &ho, &wo) != DLWP_OK) return 0;
  return (size_t)dw_splits(xs, ho, wo) * d.kh * d.kw * xs.c * d.depth_multiplier * sizeof(float);
}

int dlwp_depthwise2d_bwd_weight(dlwp_handle_t h, const void* x, const void* dz, void* dw, dlwp_shape4 xs, dlwp_depthwise2d d, void* ws,
                                int accumulate, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_depthwise2d_bwd_weight, h, x, dz, dw, xs, d, ws, accumulate, dtype);
  const char* who = "dlwp_depthwise2d_bwd_weight";
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  int ho, wo;
  int rc = dw_shape(who, xs, d, &ho, &wo);
  if (rc != DLWP_OK) return rc;
  rc = dw_windows(who, xs, d);
  if (rc != DLWP_OK) return rc;
  const long long splits = dw_splits(xs, ho, wo);
  DLWP_CHECK_ARG(splits < (1ll << 31) && xs.c <= 65535, "%s: sizes beyond the grid range", who);
  DLWP_CHECK_ARG(dw && ws && (xs.n == 0 || (x && dz)), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  const DwGeom g = dw_geom(xs, d, ho, wo);
  const long long count = (long long)d.kh * d.kw * xs.c * d.depth_multiplier;
  const long long total = (long long)xs.n * ho * wo;
  dw_bwd_weight_kernel<<<dim3((unsigned)splits, (unsigned)xs.c), 256, 0, (hipStream_t)stream>>>((const float*)x, (const float*)dz,
                                                                                                (float*)ws, total, g);
  DLWP_LAUNCH_CHECK("dw_bwd_weight_kernel");
  sep_sum_parts_kernel<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>((const float*)ws, (float*)dw, count,
                                                                                         (int)splits, accumulate ? 1 : 0);
  DLWP_LAUNCH_CHECK("sep_sum_parts_kernel");
  return DLWP_OK;
}

int dlwp_pointwise2d_fwd(dlwp_handle_t h, const void* x, const void* w, const void* bias, void* y, int n, int hw, dlwp_pointwise2d d,
                         int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_pointwise2d_fwd, h, x, w, bias, y, n, hw, d, dtype);
  const char* who = "dlwp_pointwise2d_fwd";
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  const int rc = pw_check(who, n, hw, d);
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(n == 0 || (x && w && y), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  if (n == 0) return DLWP_OK;
  const PwGeom g{n, hw, d.q, d.o, d.o, d.act, d.in_c_off, d.in_c_total, d.out_c_off, d.out_c_total, (hw + 127) / 128};
  pw_launch<false>((const float*)x, (const float*)w, (const float*)bias, (float*)y, g, (hipStream_t)stream);
  DLWP_LAUNCH_CHECK("pw_mm_kernel");
  return DLWP_OK;
}

int dlwp_pointwise2d_bwd_data(dlwp_handle_t h, const void* dz, const void* w, void* dx, int n, int hw, dlwp_pointwise2d d, int dtype,
                              void* stream) {
  DLWP_TAPE(h, stream, dlwp_pointwise2d_bwd_data, h, dz, w, dx, n, hw, d, dtype);
  const char* who = "dlwp_pointwise2d_bwd_data";
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  const int rc = pw_check(who, n, hw, d);
  if (rc != DLWP_OK) return rc;
  DLWP_CHECK_ARG(n == 0 || (dz && w && dx), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  if (n == 0) return DLWP_OK;
  // dz lies in the OUTPUT window of the descriptor, dx in its input window
  const PwGeom g{n, hw, d.o, d.q, d.o, DLWP_ACT_LINEAR, d.out_c_off, d.out_c_total, d.in_c_off, d.in_c_total, (hw + 127) / 128};
  pw_launch<true>((const float*)dz, (const float*)w, nullptr, (float*)dx, g, (hipStream_t)stream);
  DLWP_LAUNCH_CHECK("pw_mm_kernel");
  return DLWP_OK;
}

size_t dlwp_pointwise2d_bwd_workspace(int n, int hw, dlwp_pointwise2d d) {
  if (n < 0 || hw < 1 || d.q < 1 || d.o < 1) return 0;
  const long long units = (long long)n * ((hw + 31) / 32);
  const long long splits = units > 0 ? (units + PW_UNITS - 1) / PW_UNITS : 1;
  return (size_t)splits * d.q * d.o * sizeof(float);
}

int dlwp_pointwise2d_bwd_weight(dlwp_handle_t h, const void* x, const void* dz, void* dw, int n, int hw, dlwp_pointwise2d d, void* ws,
                                int accumulate, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_pointwise2d_bwd_weight, h, x, dz, dw, n, hw, d, ws, accumulate, dtype);
  const char* who = "dlwp_pointwise2d_bwd_weight";
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  const int rc = pw_check(who, n, hw, d);
  if (rc != DLWP_OK) return rc;
  const long long units = (long long)n * ((hw + 31) / 32);
  const long long splits = units > 0 ? (units + PW_UNITS - 1) / PW_UNITS : 1;
  DLWP_CHECK_ARG(splits < (1ll << 31) && (d.q + 63) / 64 <= 65535 && (d.o + 63) / 64 <= 65535, "%s: sizes beyond the grid range", who);
  DLWP_CHECK_ARG(dw && ws && (n == 0 || (x && dz)), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  const PwwGeom g{n, hw, d.q, d.o, (hw + 31) / 32, d.in_c_off, d.in_c_total, d.out_c_off, d.out_c_total};
  pw_bwd_weight_kernel<<<dim3((unsigned)splits, (unsigned)((d.q + 63) / 64), (unsigned)((d.o + 63) / 64)), 256, 0,
                         (hipStream_t)stream>>>((const float*)x, (const float*)dz, (float*)ws, g);
  DLWP_LAUNCH_CHECK("pw_bwd_weight_kernel");
  const long long count = (long long)d.q * d.o;
  sep_sum_parts_kernel<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>((const float*)ws, (float*)dw, count,
                                                                                         (int)splits, accumulate ? 1 : 0);
  DLWP_LAUNCH_CHECK("sep_sum_parts_kernel");
  return DLWP_OK;
}

}  // extern "C"
