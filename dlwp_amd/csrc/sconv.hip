// sconv.hip -- keras Conv2D(filters, k, strides=2), restated as a stride-1 convolution on the space-to-depth image of its input.
//
// Definition (channels_first, kernel K (kh, kw, cin, F)):  y[n][o][i][j] = b[o] + sum_{u,v,c} xpad[n][c][2i+u][2j+v] * K[u][v][c][o],
// xpad = the input under the layer's padding -- 'valid': none, out = (len - k) / 2 + 1;  'same' (TensorFlow's rule for stride 2):
// out = ceil(len / 2), max((out - 1) 2 + k - len, 0) zeros in all, the smaller half first.  With u = 2 ti + a, v = 2 tj + b and
// T = ceil(k / 2) per axis, and P the space-to-depth image of xpad,
//   P[n][(2a+b)*cin + c][i][j] = xpad[n][c][2i+a][2j+b]                       (phase-major, +0 outside the padded image)
// y is the stride-1 'valid' cross-correlation of P (4 cin channels, (out_h + Th - 1) x (out_w + Tw - 1)) with
//   w2[ti][tj][(2a+b)*cin + c][o] = K[2ti+a][2tj+b][c][o]                      (zero where that index is >= kh / kw)
// -- a permutation with zero fill, no sums; bias and activation stay in the convolution's epilogue (the bias is NOT replicated).
//   dlwp_sconv_weights:             K -> w2 (sh, sw, 4 cin, F)
//   dlwp_sconv_weights_bwd:         dw2 -> dK: every element of K sits in exactly one element of w2, a pure gather
//   dlwp_space_to_depth2_pad:       (n, c_total, H, W)[c_off:+c] -> P (n, 4c, hp, wp), taking the halo in front of the layer with it:
//                                   P[..][i][j] = src[map(2i+a - top)][map(2j+b - left)] under the five DLWP_PAD_* modes per axis
//   dlwp_space_to_depth2_pad_bwd:   its adjoint in gather form (no atomics): EVERY element of the source window is written
// The first three move and zero-fill only: bit-exact by construction.  The adjoint sums where a halo folds back (wrap: the periodic
// images, edge: onto the border, the mirrors: their reflections): the pixel's own position first, then the halo positions in
// ascending (row, column) order.
//
// The derived kernel may be stored with MORE taps than T: (sh, sw, 4 cin, F), sh >= Th, sw >= Tw, the Th x Tw block at offset (0, 0)
// and zeros below / right of it -- the matrix-core forward and weight-gradient kernels exist for 3 x 3 and 5 x 5 taps.  The block
// sits at the origin so that NOTHING shifts: the convolution stays 'valid' with no halo, and P just grows by sh - Th rows and
// sw - Tw columns at the bottom / right (hp = out_h + sh - 1, wp = out_w + sw - 1), which hold the next real pixels or +0 beyond the
// padded image and meet zero taps only.
//
// Access pattern of dlwp_space_to_depth2_pad (HBM-bound, float32).  16-byte route: one lane moves 8 consecutive padded columns of
// one padded row = 4 phase pixels of each of the two column phases, as two 16-byte loads of one source row and one 16-byte store to
// each of the two column-phase planes.  Its conditions, exactly:
//   wp % 4 == 0, pad.left % 4 == 0, in_w % 4 == 0, src and dst 16-byte aligned
// (then every quad of padded columns is wholly inside the source row, aligned, or wholly in the halo / beyond the padded image; a
// halo quad is fetched per element through the mode's map).  Element route otherwise: one lane per phase pixel, its 2 x 2 padded
// pixels (two neighbouring columns of two rows) to the 4 phase planes (coalesced stores).
// dlwp_space_to_depth2_pad_bwd: where both modes are DLWP_PAD_ZERO (one term per source pixel) and the conditions above hold, one
// lane takes a quad of each column-phase plane and writes 8 source pixels of one row; otherwise one lane per phase cell gathers the
// up to 2 x 2 source pixels whose own padded position lies in it (the index arithmetic of the forward's element route): four loads
// up front and four stores, as d2s_crop_kernel, and in between only a pixel within a summing halo's reach of a border adds the halo
// rows and columns that map to it.  The halo maps are division-free: a validated halo (dlwp_pad_fits) never reaches further
// than one period / one reflection.
#include "common.h"
#include "tape.h"

namespace {

__global__ __launch_bounds__(256) void sconv_weights_kernel(const float* __restrict__ w, float* __restrict__ w2, int kh, int kw,
                                                            int cin, int F, int Sh, int Sw) {
  const long long total = (long long)Sh * Sw * 4 * cin * F;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int o = (int)(e % F);
    long long q = e / F;
    const int pc = (int)(q % (4 * cin));
    q /= 4 * cin;
    const int tj = (int)(q % Sw), ti = (int)(q / Sw);
    const int ph = pc / cin, c = pc - ph * cin;
    const int u = 2 * ti + (ph >> 1), v = 2 * tj + (ph & 1);
    w2[e] = (u < kh && v < kw) ? w[((long long)(u * kw + v) * cin + c) * F + o] : 0.f;
  }
}

// dK[u][v][c][o] (+)= dw2[u>>1][v>>1][(2(u&1) + (v&1))*cin + c][o]
__global__ __launch_bounds__(256) void sconv_weights_bwd_kernel(const float* __restrict__ dw2, float* __restrict__ dw, int kh,
                                                                int kw, int cin, int F, int Sw, int accumulate) {
  const long long total = (long long)kh * kw * cin * F;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int o = (int)(e % F);
    long long q = e / F;
    const int c = (int)(q % cin);
    q /= cin;
    const int v = (int)(q % kw), u = (int)(q / kw);
    const float g = dw2[(((long long)(u >> 1) * Sw + (v >> 1)) * (4 * cin) + (2 * (u & 1) + (v & 1)) * cin + c) * F + o];
    dw[e] = accumulate ? dw[e] + g : g;
  }
}

struct S2dGeom {
  int C, H, W, hp, wp, top, left, PH, PW, mode_h, mode_w, c_off, c_total;    // PH x PW: the padded image
};

// dlwp_map_coord on the range a validated halo reaches (p in [-n, 2n) for wrap, one reflection for the mirrors): no division
__device__ __forceinline__ int smap(int p, int n, int mode) {
  if ((unsigned)p < (unsigned)n) return p;
  if (mode == DLWP_PAD_ZERO) return -1;
  if (mode == DLWP_PAD_EDGE) return p < 0 ? 0 : n - 1;
  if (mode == DLWP_PAD_REFLECT) return p < 0 ? -p : 2 * n - 2 - p;
  if (mode == DLWP_PAD_SYMMETRIC) return p < 0 ? -p - 1 : 2 * n - 1 - p;
  return p < 0 ? p + n : p - n;   // DLWP_PAD_WRAP
}

// one lane per PHASE pixel (n, ch, i, j): the 2 x 2 padded pixels at (2i, 2j), through the halo maps, to the 4 phase planes
__global__ __launch_bounds__(256) void s2d_pad_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total,
                                                      S2dGeom g) {
  const long long plane = (long long)g.hp * g.wp, cp = (long long)g.C * plane;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int j = (int)(e % g.wp);
    long long q = e / g.wp;
    const int i = (int)(q % g.hp);
    q /= g.hp;
    const int ch = (int)(q % g.C);
    const long long n = q / g.C;
    const int r0 = 2 * i, s0 = 2 * j;
    const int ya = r0 < g.PH ? smap(r0 - g.top, g.H, g.mode_h) : -1, yb = r0 + 1 < g.PH ? smap(r0 + 1 - g.top, g.H, g.mode_h) : -1;
    const int xa = s0 < g.PW ? smap(s0 - g.left, g.W, g.mode_w) : -1, xb = s0 + 1 < g.PW ? smap(s0 + 1 - g.left, g.W, g.mode_w) : -1;
    const float* s = src + (n * g.c_total + g.c_off + ch) * (long long)g.H * g.W;
    const float* ra = s + (long long)(ya < 0 ? 0 : ya) * g.W;
    const float* rb = s + (long long)(yb < 0 ? 0 : yb) * g.W;
    const float v00 = (ya >= 0 && xa >= 0) ? ra[xa] : 0.f, v01 = (ya >= 0 && xb >= 0) ? ra[xb] : 0.f;
    const float v10 = (yb >= 0 && xa >= 0) ? rb[xa] : 0.f, v11 = (yb >= 0 && xb >= 0) ? rb[xb] : 0.f;
    float* d = dst + (n * 4 * g.C + ch) * plane + (long long)i * g.wp + j;
    d[0] = v00;
    d[cp] = v01;
    d[2 * cp] = v10;
    d[3 * cp] = v11;
  }
}

// 4 padded columns s .. s+3 (s a multiple of 4) of the source row `row` (nullptr: a zero row): one 16-byte load in the interior
__device__ __forceinline__ float4 s2d_quad(const float* row, int s, const S2dGeom& g) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!row) return v;
  const int x0 = s - g.left;
  if (x0 >= 0 && x0 + 4 <= g.W) return *reinterpret_cast<const float4*>(row + x0);
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = s + k < g.PW ? smap(x0 + k, g.W, g.mode_w) : -1;
    t[k] = x >= 0 ? row[x] : 0.f;
  }
  return make_float4(t[0], t[1], t[2], t[3]);
}

// one lane per 8 padded columns of one padded row (a, i): 4 phase pixels of both column phases (see the header for the conditions)
__global__ __launch_bounds__(256) void s2d_pad_vec_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total,
                                                          S2dGeom g) {
  const long long plane = (long long)g.hp * g.wp;
  const int quads = g.wp >> 2;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int qd = (int)(e % quads);
    long long q = e / quads;
    const int i = (int)(q % g.hp);
    q /= g.hp;
    const int a = (int)(q & 1);
    q >>= 1;
    const int ch = (int)(q % g.C);
    const long long n = q / g.C;
    const int r = 2 * i + a;
    const int y = r < g.PH ? smap(r - g.top, g.H, g.mode_h) : -1;
    const float* row = y >= 0 ? src + ((n * g.c_total + g.c_off + ch) * g.H + y) * (long long)g.W : nullptr;
    const float4 lo = s2d_quad(row, 8 * qd, g), hi = s2d_quad(row, 8 * qd + 4, g);
    float* d = dst + (n * 4 * g.C + (long long)(2 * a) * g.C + ch) * plane + (long long)i * g.wp + 4 * qd;
    *reinterpret_cast<float4*>(d) = make_float4(lo.x, lo.z, hi.x, hi.z);
    *reinterpret_cast<float4*>(d + (long long)g.C * plane) = make_float4(lo.y, lo.w, hi.y, hi.w);
  }
}

// adjoint, gather form: one lane per PHASE cell (n, ch, i, j) of the cells that hold the source's own padded positions (rows
// top .. top + H - 1, columns left .. left + W - 1): the up to 2 x 2 source pixels whose own position lies in the cell.  Their own
// terms come from the 4 phase planes at (i, j), four loads up front (coalesced, the mirror of s2d_pad_kernel; as d2s_crop_kernel takes
// them); only a pixel within a summing halo's reach of a border (reach 0: a zero halo folds nothing back) then adds the halo positions
// that map to it, in ascending (r, s) inside [0, 2hp) x [0, 2wp) and the padded image; then the stores.  A lone term is stored as it is
// (-0 stays -0), a pixel with no term is +0.
__global__ __launch_bounds__(256) void s2d_pad_bwd_kernel(const float* __restrict__ ddst, float* __restrict__ dsrc, long long total,
                                                          int cells_h, int cells_w, int reach_h, int reach_w, S2dGeom g) {
  const long long plane = (long long)g.hp * g.wp, cp = (long long)g.C * plane;
  const int r_end = min(g.PH, 2 * g.hp), s_end = min(g.PW, 2 * g.wp);
  const int t_end = min(g.top, r_end), l_end = min(g.left, s_end);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int jc = (int)(e % cells_w);
    long long q = e / cells_w;
    const int ic = (int)(q % cells_h);
    q /= cells_h;
    const int ch = (int)(q % g.C);
    const long long n = q / g.C;
    const int i = (g.top >> 1) + ic, j = (g.left >> 1) + jc;
    const float* base = ddst + (n * 4 * g.C + ch) * plane;
    const int ya = 2 * i - g.top, xa = 2 * j - g.left;
    const bool rok[2] = {ya >= 0 && ya < g.H, ya + 1 >= 0 && ya + 1 < g.H};
    const bool cok[2] = {xa >= 0 && xa < g.W, xa + 1 >= 0 && xa + 1 < g.W};
    const bool in = i < g.hp && j < g.wp;                  // (the cell lies inside the phase tensor: the own terms exist)
    const float* d = base + (long long)i * g.wp + j;
    float v[2][2];
    v[0][0] = (in && rok[0] && cok[0]) ? d[0] : 0.f;
    v[0][1] = (in && rok[0] && cok[1]) ? d[cp] : 0.f;
    v[1][0] = (in && rok[1] && cok[0]) ? d[2 * cp] : 0.f;
    v[1][1] = (in && rok[1] && cok[1]) ? d[3 * cp] : 0.f;
    if (reach_h | reach_w) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int y = ya + a, x = xa + b;
          if (!(rok[a] && cok[b])) continue;
          const bool near_h = y < reach_h || y >= g.H - reach_h, near_w = x < reach_w || x >= g.W - reach_w;
          if (!(near_h || near_w)) continue;
          const int r0 = y + g.top, s0 = x + g.left;
          float acc = v[a][b];
          bool any = in;
          auto row_terms = [&](int r, bool own_too) {      // the halo columns of padded row r that map to x (+ column s0 itself)
            const float* prow = base + (long long)(2 * (r & 1)) * cp + (long long)(r >> 1) * g.wp;
            auto add = [&](int s) {
              const float t = prow[(long long)(s & 1) * cp + (s >> 1)];
              acc = any ? acc + t : t;
              any = true;
            };
            if (near_w)
              for (int s = 0; s < l_end; ++s)
                if (smap(s - g.left, g.W, g.mode_w) == x) add(s);
            if (own_too && s0 < s_end) add(s0);
            if (near_w)
              for (int s = g.left + g.W; s < s_end; ++s)
                if (smap(s - g.left, g.W, g.mode_w) == x) add(s);
          };
          if (near_h)
            for (int r = 0; r < t_end; ++r)
              if (smap(r - g.top, g.H, g.mode_h) == y) row_terms(r, true);
          if (r0 < r_end) row_terms(r0, false);            // (its own position is in acc already)
          if (near_h)
            for (int r = g.top + g.H; r < r_end; ++r)
              if (smap(r - g.top, g.H, g.mode_h) == y) row_terms(r, true);
          v[a][b] = acc;
        }
      }
    }
    float* o = dsrc + ((n * g.c_total + g.c_off + ch) * g.H + ya) * (long long)g.W + xa;     // (used only where in range)
    if (rok[0] && cok[0]) o[0] = v[0][0];
    if (rok[0] && cok[1]) o[1] = v[0][1];
    if (rok[1] && cok[0]) o[g.W] = v[1][0];
    if (rok[1] && cok[1]) o[g.W + 1] = v[1][1];
  }
}

// adjoint under zero / zero modes, 16-byte route: one lane per 8 padded columns of one source row: a quad of each column-phase plane
// (or zeros beyond the phase tensor) -> the two source quads that lie inside the row
__global__ __launch_bounds__(256) void s2d_pad_bwd_vec_kernel(const float* __restrict__ ddst, float* __restrict__ dsrc,
                                                              long long total, int groups, S2dGeom g) {
  const long long plane = (long long)g.hp * g.wp;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int qd = (int)(e % groups);
    long long q = e / groups;
    const int y = (int)(q % g.H);
    q /= g.H;
    const int ch = (int)(q % g.C);
    const long long n = q / g.C;
    const int c0 = 8 * qd - g.left;                 // first of the 8 source columns (a multiple of 4)
    if (c0 + 8 <= 0 || c0 >= g.W) continue;
    const int r = y + g.top;
    float4 e0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = e0;
    if (r < 2 * g.hp && 4 * qd < g.wp) {
      const float* s0 = ddst + (n * 4 * g.C + (long long)(2 * (r & 1)) * g.C + ch) * plane + (long long)(r >> 1) * g.wp + 4 * qd;
      e0 = *reinterpret_cast<const float4*>(s0);                             // column phase 0
      e1 = *reinterpret_cast<const float4*>(s0 + (long long)g.C * plane);    // column phase 1
    }
    float* d = dsrc + ((n * g.c_total + g.c_off + ch) * g.H + y) * (long long)g.W + c0;
    if (c0 >= 0) *reinterpret_cast<float4*>(d) = make_float4(e0.x, e1.x, e0.y, e1.y);
    if (c0 + 8 <= g.W) *reinterpret_cast<float4*>(d + 4) = make_float4(e0.z, e1.z, e0.w, e1.w);
  }
}

bool vec_ok(const void* a, const void* b, const S2dGeom& g) {
  return g.wp % 4 == 0 && g.left % 4 == 0 && g.W % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

// (shape checks first: they need no device, and a wrong halo must never reach a launch)
int check_s2d(const char* who, dlwp_handle_t h, const void* a, const void* b, int n, int c, int H, int W, const dlwp_pad2d& p,
              int hp, int wp, int c_off, int c_total, int dtype) {
  DLWP_CHECK_ARG(dtype == DLWP_F32, "%s: dtype %d not supported", who, dtype);
  DLWP_CHECK_ARG(n >= 0 && c >= 1 && H >= 1 && W >= 1 && hp >= 1 && wp >= 1,
                 "%s: bad shape (n %d, c %d, %d x %d -> %d x %d): every size must be at least 1", who, n, c, H, W, hp, wp);
  DLWP_CHECK_ARG(c_off >= 0 && c_total >= 1 && (long long)c_off + c <= c_total,
                 "%s: the channel window [%d, +%d) lies outside the %d channels of the tensor", who, c_off, c, c_total);
  DLWP_CHECK_ARG(p.top >= 0 && p.bottom >= 0 && p.left >= 0 && p.right >= 0, "%s: negative padding", who);
  DLWP_CHECK_ARG((unsigned)p.mode_h <= 4u && (unsigned)p.mode_w <= 4u, "%s: unknown pad mode", who);
  DLWP_CHECK_ARG(dlwp_pad_fits(p.top, p.bottom, H, p.mode_h), "%s: the row halo (%d, %d) of mode %d exceeds what an axis of %d serves",
                 who, p.top, p.bottom, p.mode_h, H);
  DLWP_CHECK_ARG(dlwp_pad_fits(p.left, p.right, W, p.mode_w),
                 "%s: the column halo (%d, %d) of mode %d exceeds what an axis of %d serves", who, p.left, p.right, p.mode_w, W);
  DLWP_CHECK_ARG((long long)H + p.top + p.bottom < (1ll << 30) && (long long)W + p.left + p.right < (1ll << 30) &&
                     hp < (1 << 29) && wp < (1 << 29) && (long long)c * 4 < (1ll << 31),
                 "%s: sizes beyond the 32-bit coordinate range", who);
  DLWP_CHECK_ARG(n == 0 || (a && b), "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  return DLWP_OK;
}

int grid_of(dlwp_handle_t h, long long total) {
  const long long blocks = (total + 255) / 256, cap = (long long)h->cu_count * 16;
  return (int)(blocks < cap ? blocks : cap);
}

int check_weights(const char* who, dlwp_handle_t h, const void* a, const void* b, int kh, int kw, int cin, int f, int sh, int sw,
                  int dtype) {
  DLWP_CHECK_ARG(dtype == DLWP_F32 && kh > 0 && kw > 0 && cin > 0 && f > 0, "%s: bad arguments", who);
  DLWP_CHECK_ARG(sh >= (kh + 1) / 2 && sw >= (kw + 1) / 2 && sh <= 64 && sw <= 64,
                 "%s: %d x %d stored taps do not hold the %d x %d taps of a %d x %d kernel", who, sh, sw, (kh + 1) / 2, (kw + 1) / 2,
                 kh, kw);
  DLWP_CHECK_ARG(a && b, "%s: null pointer", who);
  DLWP_CHECK_ARG(h != nullptr, "%s: null handle", who);
  return DLWP_OK;
}

}  // namespace

extern "C" {

// per axis: T = ceil(k / 2) taps on the space-to-depth image, the layer's own zero padding and the output length
int dlwp_sconv_geometry(int k, int same, int len, int* t, int* pad_lo, int* pad_hi, int* out_len) {
  DLWP_CHECK_ARG(k > 0 && len > 0 && t && pad_lo && pad_hi && out_len, "dlwp_sconv_geometry: bad arguments");
  DLWP_CHECK_ARG(same || len >= k, "dlwp_sconv_geometry: a 'valid' kernel of %d does not fit an axis of %d", k, len);
  *t = (k + 1) / 2;
  if (same) {
    const int out = (len + 1) / 2;
    const long long tot = (long long)(out - 1) * 2 + k - len;
    const int pad = tot > 0 ? (int)tot : 0;
    *pad_lo = pad / 2;
    *pad_hi = pad - pad / 2;
    *out_len = out;
  } else {
    *pad_lo = *pad_hi = 0;
    *out_len = (len - k) / 2 + 1;
  }
  return DLWP_OK;
}

int dlwp_sconv_weights(dlwp_handle_t h, const void* w, void* w2, int kh, int kw, int cin, int f, int sh, int sw, int dtype,
                       void* stream) {
  DLWP_TAPE(h, stream, dlwp_sconv_weights, h, w, w2, kh, kw, cin, f, sh, sw, dtype);
  const int rc = check_weights("dlwp_sconv_weights", h, w, w2, kh, kw, cin, f, sh, sw, dtype);
  if (rc != DLWP_OK) return rc;
  const long long total = (long long)sh * sw * 4 * cin * f;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  sconv_weights_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>((const float*)w, (float*)w2, kh, kw, cin, f, sh, sw);
  DLWP_LAUNCH_CHECK("sconv_weights_kernel");
  return DLWP_OK;
}

int dlwp_sconv_weights_bwd(dlwp_handle_t h, const void* dw2, void* dw, int kh, int kw, int cin, int f, int sh, int sw,
                           int accumulate, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_sconv_weights_bwd, h, dw2, dw, kh, kw, cin, f, sh, sw, accumulate, dtype);
  const int rc = check_weights("dlwp_sconv_weights_bwd", h, dw2, dw, kh, kw, cin, f, sh, sw, dtype);
  if (rc != DLWP_OK) return rc;
  const long long total = (long long)kh * kw * cin * f;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  sconv_weights_bwd_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>((const float*)dw2, (float*)dw, kh, kw, cin, f, sw,
                                                                          accumulate ? 1 : 0);
  DLWP_LAUNCH_CHECK("sconv_weights_bwd_kernel");
  return DLWP_OK;
}

int dlwp_space_to_depth2_pad(dlwp_handle_t h, const void* src, void* dst, int n, int c, int in_h, int in_w, dlwp_pad2d pad, int hp,
                             int wp, int c_off, int c_total, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_space_to_depth2_pad, h, src, dst, n, c, in_h, in_w, pad, hp, wp, c_off, c_total, dtype);
  const int rc = check_s2d("dlwp_space_to_depth2_pad", h, src, dst, n, c, in_h, in_w, pad, hp, wp, c_off, c_total, dtype);
  if (rc != DLWP_OK) return rc;
  if (n == 0) return DLWP_OK;
  const S2dGeom g{c, in_h, in_w, hp, wp, pad.top, pad.left, in_h + pad.top + pad.bottom, in_w + pad.left + pad.right,
                  pad.mode_h, pad.mode_w, c_off, c_total};
  if (vec_ok(src, dst, g)) {
    const long long total = (long long)n * c * 2 * hp * (wp / 4);
    s2d_pad_vec_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)src, (float*)dst, total, g);
  } else {
    const long long total = (long long)n * c * hp * wp;
    s2d_pad_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)src, (float*)dst, total, g);
  }
  DLWP_LAUNCH_CHECK("s2d_pad_kernel");
  return DLWP_OK;
}

int dlwp_space_to_depth2_pad_bwd(dlwp_handle_t h, const void* ddst, void* dsrc, int n, int c, int in_h, int in_w, dlwp_pad2d pad,
                                 int hp, int wp, int c_off, int c_total, int dtype, void* stream) {
  DLWP_TAPE(h, stream, dlwp_space_to_depth2_pad_bwd, h, ddst, dsrc, n, c, in_h, in_w, pad, hp, wp, c_off, c_total, dtype);
  const int rc = check_s2d("dlwp_space_to_depth2_pad_bwd", h, ddst, dsrc, n, c, in_h, in_w, pad, hp, wp, c_off, c_total, dtype);
  if (rc != DLWP_OK) return rc;
  if (n == 0) return DLWP_OK;
  const S2dGeom g{c, in_h, in_w, hp, wp, pad.top, pad.left, in_h + pad.top + pad.bottom, in_w + pad.left + pad.right,
                  pad.mode_h, pad.mode_w, c_off, c_total};
  if (pad.mode_h == DLWP_PAD_ZERO && pad.mode_w == DLWP_PAD_ZERO && vec_ok(ddst, dsrc, g)) {
    const int groups = (pad.left + in_w + 7) / 8;
    const long long total = (long long)n * c * in_h * groups;
    s2d_pad_bwd_vec_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)ddst, (float*)dsrc, total, groups, g);
  } else {
    // the cells of the source's own padded positions; a halo of (lo, hi) reaches pixels within max(lo, hi) + 1 of a border at most
    // (wrap: the opposite max(lo, hi) rows, the mirrors: rows 0 ... lo / the last hi + 1, edge: the border row itself)
    const int cells_h = ((pad.top + in_h - 1) >> 1) - (pad.top >> 1) + 1, cells_w = ((pad.left + in_w - 1) >> 1) - (pad.left >> 1) + 1;
    const int far_h = pad.top > pad.bottom ? pad.top : pad.bottom, far_w = pad.left > pad.right ? pad.left : pad.right;
    const int reach_h = (pad.mode_h == DLWP_PAD_ZERO || far_h == 0) ? 0 : far_h + 1;      // (a zero halo folds nothing back)
    const int reach_w = (pad.mode_w == DLWP_PAD_ZERO || far_w == 0) ? 0 : far_w + 1;
    const long long total = (long long)n * c * cells_h * cells_w;
    s2d_pad_bwd_kernel<<<grid_of(h, total), 256, 0, (hipStream_t)stream>>>((const float*)ddst, (float*)dsrc, total, cells_h, cells_w,
                                                                           reach_h, reach_w, g);
  }
  DLWP_LAUNCH_CHECK("s2d_pad_bwd_kernel");
  return DLWP_OK;
}

}  // extern "C"
