// conv_fwd_few_wino.hip -- the first layer of a large ensemble on Winograd multiplies: 3x3, DILATION 2, at most FOUR input
// channels, MaxPooling2D(2) epilogue, pooled image only, float32 -- the streaming structure of conv_fwd_few.hip (workgroups own
// equal contiguous shares of (tile position, sample) items, the halo resolved once per position, the sample as the scalar base of
// the buffer descriptor, two LDS input buffers, one barrier per item, compiler-scheduled) with F(2x2, 3x3) instead of the direct
// sum: 16 multiplies per output and input channel instead of 36 (DLWP_OPT_FEW_WINO).
//
// * Sub-lattices.  A dilation-2 convolution is four independent dilation-1 problems on the (row parity, column parity)
//   sub-lattices of the image, all with the same filters; a pooling window holds ONE pixel of each sub-lattice, at the same
//   sub-lattice index.  An 8 x 32 tile is 2 x 8 Winograd tiles (2x2 outputs each) on each of the four sub-lattices.
// * One MFMA step per Winograd position.  K = 4 of v_mfma_f32_16x16x4_f32 is exactly the four input channels.  M row 4 t + p =
//   (tile t of the wave's four tiles, parity class p = 2 pi + pj); wave w owns sub-lattice tile row w >> 1, tile columns
//   4 (w & 1) + t.  Lane l supplies A for row l & 15, channel l >> 4: it reads its 4 x 4 patch from the LDS tile -- staged
//   DE-INTERLEAVED, [channel][pi][pj][6][20], so that a patch row is four adjacent floats -- and applies B^T d B in packed fp32.
// * Pooling in registers.  The C fragment is col = lane & 15 (channel), row = 4 (lane >> 4) + reg: registers 0-3 of every
//   accumulator of a lane are the four parity classes of ONE tile and channel.  The lane applies A^T M A per parity (packed over
//   the register pairs), takes the maximum over the four parities -- the pooled 2 x 2 block of the tile --, adds the bias and
//   activates once per pooled value: no LDS exchange, no second barrier.
// * Weights.  U = G g G^T, 16 positions x 2 channel tiles per lane, stay in registers for the whole launch; derived in the
//   prologue from the HWIO weights with wino_filter_transform_f32's expressions.
// * Order of operations = conv_fwd_wino_kernel.h's: d B before B^T (d B), the channel group of 4 in one matrix step from 0,
//   A^T M summed (0 + 1) + 2 and (1 - 2) - 3, then the same over columns: the bits of the general Winograd family on this geometry
//   (whose padded channels 4-7 add exact zeros).  The maximum is taken BEFORE bias and activation (monotonic: the same value).
// * Stores.  The lane's pooled 2 x 2 block leaves from registers as two 8-byte pairs per channel tile; the four lanes of a channel
//   cover 32 consecutive bytes of a row.  (16-byte row segments -- the lanes of neighbouring tiles exchanging a row each -- timed
//   the same, 72-75 us at 256 members either way, DESIGN 5.26: the shorter form is kept.)
#include "conv_fwd_kernel.h"

namespace {

template <bool QUAD_>
struct FewWinoCfg {
  static constexpr int DIL = 2, TH = 8, TW = 32, WAVES = 4, NT = 256;
  static constexpr bool QUAD = QUAD_;                 // (conv_fwd_few.hip: the window as 10 aligned 16-byte quads per row)
  static constexpr int LR = TH + 2 * DIL, LC = QUAD ? 40 : TW + 2 * DIL;
  static constexpr int PS_RAW = LR * LC;
  static constexpr int EPL = QUAD ? 4 : 1;            // floats per staged element
  static constexpr int NQ = (PS_RAW / EPL + 63) / 64;  // elements a lane stages (a wave = one channel plane)
  // LDS: [channel][pi][pj][LR / 2][LCP].  Sub-plane stride 120 = 24 (mod 32) and an ODD channel stride: the 32 lanes of half a
  // patch read (tiles 2 floats apart, 4 parities, 2 channels) fall on 32 different banks
  static constexpr int LCP = 20, SP = (LR / 2) * LCP, PS = 4 * SP + 1;
  static constexpr int X_FLOATS = 4 * PS;
  static constexpr int LDS_BYTES = 2 * X_FLOATS * 4;
};

template <int ACT, bool QUAD>
__global__ __launch_bounds__(256, QUAD ? 3 : 2) void conv2d_fwd_few_wino_f32(const ConvArgs a, const int group) {
  using C = FewWinoCfg<QUAD>;
  constexpr unsigned DROP = 0x7ffffff0u;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- items and shares: conv_fwd_few.hip's arithmetic
  const int npos = a.tiles_h * a.tiles_w * a.cout_tiles;
  const long long T = (long long)npos * a.N;
  int L;
  {
    const int b = blockIdx.x, nb = gridDim.x;
    const int xcd = b & 7, idx = b >> 3, q = nb >> 3, r = nb & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int it = (int)(T * L / gridDim.x);
  int left = (int)(T * (L + 1) / gridDim.x) - it;
  if (left <= 0) return;
  int g0, gs, pos, sn;
  {
    const int per = npos * group;
    const int sg = it / per, rem = it - sg * per;
    g0 = sg * group;
    gs = min(group, a.N - g0);
    pos = rem / gs;
    sn = rem - pos * gs;
  }
  auto advance = [&](int& g0_, int& gs_, int& pos_, int& sn_) {
    if (++sn_ == gs_) {
      sn_ = 0;
      if (++pos_ == npos) {
        pos_ = 0;
        g0_ += gs_;
        gs_ = min(group, a.N - g0_);
      }
    }
  };

  const unsigned plane_bytes = (unsigned)(a.Hs * a.Ws) * 4u;
  const unsigned oplane_bytes = (unsigned)(a.Hp * a.Wp) * 4u;
  const long long x_sample = (long long)a.in_c_total * plane_bytes;
  const long long y_sample = (long long)a.out_c_total * oplane_bytes;
  const char* x0 = (const char*)a.x + (long long)a.in_c_off * plane_bytes;
  char* y0 = (char*)a.y + (long long)a.out_c_off * oplane_bytes;

  // ---- per-position state
  unsigned goff[C::NQ];          // byte offset of this lane's window elements in a channel plane (DROP: reads 0.0)
  unsigned voff[2];              // byte offset of this lane's pooled pixels, channel tile g (DROP: dropped)
  bool second_ok = true;         // this lane's second pooled row is inside the map
  float bw[16][2];               // B operands: U[xy][ci = lane >> 4][co = n0 + 16 g + (lane & 15)]
  float bv[2];
  int ct_loaded = -1;
  auto setup_loads = [&](int p) {
    const int tw = p % a.tiles_w;
    const int th = (p / a.tiles_w) % a.tiles_h;
    const int i0 = th * C::TH, j0 = tw * C::TW;
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) {
      const int s = (lane + 64 * q) * C::EPL;
      const int lr = s / C::LC, lc = s - lr * C::LC;
      const int rs = dlwp_map_coord_tile(i0 + lr - a.pad_top, a.H, a.mode_h);
      const int cs = dlwp_map_coord_tile(j0 + lc - (C::QUAD ? 4 : a.pad_left), a.W, a.mode_w);
      const bool ok = (q < C::NQ - 1 || s < C::PS_RAW) && rs >= 0 && cs >= 0 && wave < a.Cin;
      goff[q] = ok ? (unsigned)(rs * a.Ws + cs) * 4u : DROP;
    }
  };
  // the lane's pooled pixels.  Its C rows are tile t = lane >> 4 of the wave: sub-lattice tile (wave >> 1, 4 (wave & 1) + t) =
  // pooled rows 2 (wave >> 1) + {0, 1}, pooled columns 8 (wave & 1) + 2 t + {0, 1} of the item (Wp is even: a pair is in or out).
  auto setup_outputs = [&](int p) {
    const int tw = p % a.tiles_w;
    const int r = p / a.tiles_w;
    const int th = r % a.tiles_h, ct = r / a.tiles_h;
    const int n0 = ct * 32;
    const int pr = th * (C::TH / 2) + 2 * (wave >> 1);
    const int pc = tw * (C::TW / 2) + 8 * (wave & 1) + 2 * (lane >> 4);
    second_ok = pr + 1 < a.Hp;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int co = n0 + g * 16 + (lane & 15);
      const bool c_ok = co < a.Cout;
      const int cc = c_ok ? co : 0;
      if (ct != ct_loaded) {   // (uniform) U = G g G^T: the expressions of wino_filter_transform_f32 (conv_fwd.hip)
        const int ci = lane >> 4;
        float gt[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) gt[tap] = (c_ok && ci < a.Cin) ? a.w[((long long)tap * a.Cin + ci) * a.Cout + cc] : 0.f;
        float tm[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float w0 = gt[c], w1 = gt[3 + c], w2 = gt[6 + c];
          tm[0][c] = w0;
          tm[1][c] = 0.5f * (w0 + w1 + w2);
          tm[2][c] = 0.5f * (w0 - w1 + w2);
          tm[3][c] = w2;
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float t0 = tm[rr][0], t1 = tm[rr][1], t2 = tm[rr][2];
          bw[rr * 4 + 0][g] = t0;
          bw[rr * 4 + 1][g] = 0.5f * (t0 + t1 + t2);
          bw[rr * 4 + 2][g] = 0.5f * (t0 - t1 + t2);
          bw[rr * 4 + 3][g] = t2;
        }
        bv[g] = (a.bias && c_ok) ? a.bias[cc] : 0.f;
      }
      voff[g] = (c_ok && pr < a.Hp && pc < a.Wp) ? (unsigned)((co * a.Hp + pr) * a.Wp + pc) * 4u : DROP;
    }
    ct_loaded = ct;
  };

  // this lane's A-operand patch: M row m = lane & 15 = (tile m >> 2, parity m & 3), channel lane >> 4.  Window rows
  // 4 ti + pi + 2 k, window columns 4 tj + pj + 2 k' (+ the quad window's left margin): parity plane, then ADJACENT slots
  int abase;
  {
    const int m = lane & 15, pi = (m >> 1) & 1, pj = m & 1;
    const int ti = wave >> 1, tj = 4 * (wave & 1) + (m >> 2);
    const int c0 = 4 * tj + pj + (C::QUAD ? 4 - a.pad_left : 0);
    abase = (lane >> 4) * C::PS + (2 * pi + (c0 & 1)) * C::SP + 2 * ti * C::LCP + (c0 >> 1);
  }
  // LDS slots of the staged elements: channel plane `wave`, window element lane + 64 q -> (row parity, column parity, row / 2,
  // column / 2); a quad = two column pairs, one per column parity
  int sdst[C::NQ];
#pragma unroll
  for (int q = 0; q < C::NQ; ++q) {
    const int s = (lane + 64 * q) * C::EPL;
    const int lr = s / C::LC, lc = s - lr * C::LC;
    sdst[q] = wave * C::PS + (2 * (lr & 1) + (lc & 1)) * C::SP + (lr >> 1) * C::LCP + (lc >> 1);
  }
  const bool last_ok = (lane + 64 * (C::NQ - 1)) * C::EPL < C::PS_RAW;

  using elem_t = std::conditional_t<C::QUAD, f32x4, float>;
  elem_t xr[C::NQ];
  auto load_item = [&](int nn) {
    const __amdgpu_buffer_rsrc_t x_rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)(x0 + (long long)nn * x_sample), 0, (unsigned)a.Cin * plane_bytes, 0x00020000);
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) {
      if constexpr (C::QUAD)
        xr[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, goff[q], wave * plane_bytes, 0));
      else
        xr[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rsrc, goff[q], wave * plane_bytes, 0));
    }
  };
  auto stage = [&](int buf) {
    float* pl = lds + buf * C::X_FLOATS;
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) {
      if (q == C::NQ - 1 && !last_ok) continue;
      if constexpr (C::QUAD) {
        pl[sdst[q]] = xr[q].x;
        pl[sdst[q] + 1] = xr[q].z;
        pl[sdst[q] + C::SP] = xr[q].y;
        pl[sdst[q] + C::SP + 1] = xr[q].w;
      } else {
        pl[sdst[q]] = xr[q];
      }
    }
  };

  // ---- the pipeline (conv_fwd_few.hip):
  //        body k:  transform + MFMAs(k) from LDS buffer k & 1 | tile k + 1: registers -> the other buffer | epilogue + stores(k) |
  //                 loads(k + 2) -> registers | barrier
  int g1 = g0, gs1 = gs, p1 = pos, sn1 = sn;
  advance(g1, gs1, p1, sn1);
  setup_loads(pos);
  load_item(g0 + sn);
  setup_outputs(pos);
  stage(0);
  if (left > 1) {
    if (p1 != pos) setup_loads(p1);
    load_item(g1 + sn1);
  }
  __syncthreads();

  for (;;) {
#pragma unroll
    for (int buf = 0; buf < 2; ++buf) {
      const float* xs = lds + buf * C::X_FLOATS + abase;
      // ---- V = B^T d B on column pairs (conv_fwd_wino_kernel.h: vt_rows / vt_cols)
      f32x2 v2[8];               // V[r][2 h], V[r][2 h + 1] at [2 r + h]
      {
        f32x2 d2[4][2], t2[4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          d2[r][0] = (f32x2){xs[r * C::LCP], xs[r * C::LCP + 1]};
          d2[r][1] = (f32x2){xs[r * C::LCP + 2], xs[r * C::LCP + 3]};
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          t2[r][0] = pk_wino_t01(d2[r][0], d2[r][1]);
          t2[r][1] = pk_wino_t23(d2[r][0], d2[r][1]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          v2[0 + h] = pk_sub(t2[0][h], t2[2][h]);
          v2[2 + h] = pk_add(t2[1][h], t2[2][h]);
          v2[4 + h] = pk_sub(t2[2][h], t2[1][h]);
          v2[6 + h] = pk_sub(t2[1][h], t2[3][h]);
        }
      }
      const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(y0 + (long long)(g0 + sn) * y_sample), 0, (unsigned)a.Cout * oplane_bytes, 0x00020000);
      // ---- one channel tile at a time: 64 accumulator registers live, not 128 -- three waves per SIMD with 16-byte loads (155
      //      VGPRs; the element loader holds 174: two), so that a launch of up to three workgroups per CU is one
      //      round (8 members of the 88 x 180 grid: 528 items)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        __builtin_amdgcn_sched_barrier(0);   // (the second tile's matrix steps stay behind the first tile's epilogue)
        // ---- 16 positions: one matrix step each, from 0
        f32x4 acc[16];
#pragma unroll
        for (int xy = 0; xy < 16; ++xy)
          acc[xy] = __builtin_amdgcn_mfma_f32_16x16x4f32(v2[(xy >> 2) * 2 + ((xy >> 1) & 1)][xy & 1], bw[xy][g],
                                                         (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        // ---- the next item's tile: registers -> the other buffer (its readers passed the last barrier)
        if (g == 0 && left > 1) stage(buf ^ 1);
        // The output transform reads the accumulators through inline asm (pk_add / pk_sub), where the compiler places no wait
        // states behind a matrix instruction: nothing may move across this point, and the last step's 8 passes drain first
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15");
        __builtin_amdgcn_sched_barrier(0);

        // ---- epilogue: Y = A^T M A per parity class (register pairs), maximum over the four, bias, activation
        f32x2 y[2][2][2];          // [register pair][output row aa][output column]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          auto m = [&](int xy) -> f32x2 { return h == 0 ? acc[xy].xy : acc[xy].zw; };
          f32x2 s[2][4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            s[0][c] = pk_add(pk_add(m(0 * 4 + c), m(1 * 4 + c)), m(2 * 4 + c));
            s[1][c] = pk_sub(pk_sub(m(1 * 4 + c), m(2 * 4 + c)), m(3 * 4 + c));
          }
#pragma unroll
          for (int aa = 0; aa < 2; ++aa) {
            y[h][aa][0] = pk_add(pk_add(s[aa][0], s[aa][1]), s[aa][2]);
            y[h][aa][1] = pk_sub(pk_sub(s[aa][1], s[aa][2]), s[aa][3]);
          }
        }
        f32x2 o[2];                // pooled row aa: columns 0, 1 of the tile's 2 x 2 block
#pragma unroll
        for (int aa = 0; aa < 2; ++aa) {
          const f32x2 mx = (f32x2){dlwp_nmax(dlwp_nmax(y[0][aa][0].x, y[0][aa][0].y), dlwp_nmax(y[1][aa][0].x, y[1][aa][0].y)),
                                   dlwp_nmax(dlwp_nmax(y[0][aa][1].x, y[0][aa][1].y), dlwp_nmax(y[1][aa][1].x, y[1][aa][1].y))};
          o[aa] = act_apply2_c<ACT>(mx + (f32x2){bv[g], bv[g]});
        }
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o[0]), y_rsrc, voff[g], 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o[1]), y_rsrc,
                                              (second_ok && voff[g] != DROP) ? voff[g] + (unsigned)a.Wp * 4u : DROP, 0, 0);
      }
      if (left == 1) return;

      // ---- the loads of the item after the next go out behind the stores
      int g2 = g1, gs2 = gs1, p2 = p1, sn2 = sn1;
      advance(g2, gs2, p2, sn2);
      if (left > 2) {
        if (p2 != p1) setup_loads(p2);
        load_item(g2 + sn2);
      }
      if (p1 != pos) setup_outputs(p1);
      g0 = g1, gs = gs1, pos = p1, sn = sn1;
      g1 = g2, gs1 = gs2, p1 = p2, sn1 = sn2;
      --left;
      __syncthreads();   // one barrier per item
    }
  }
}

template <bool QUAD>
void launch_few_wino(const ConvArgs& a, int grid, hipStream_t s) {
  using C = FewWinoCfg<QUAD>;
  // samples per group = the length of a workgroup's share (conv_fwd_few.hip)
  const long long items = (long long)a.tiles_h * a.tiles_w * a.cout_tiles * a.N;
  int group = (int)((items + grid / 2) / grid);
  group = group < 4 ? 4 : (group > a.N ? a.N : group);
  if (a.act == DLWP_ACT_TANH)
    hipLaunchKernelGGL((conv2d_fwd_few_wino_f32<DLWP_ACT_TANH, QUAD>), dim3(grid), dim3(C::NT), C::LDS_BYTES, s, a, group);
  else if (a.act == DLWP_ACT_RELU)
    hipLaunchKernelGGL((conv2d_fwd_few_wino_f32<DLWP_ACT_RELU, QUAD>), dim3(grid), dim3(C::NT), C::LDS_BYTES, s, a, group);
  else
    hipLaunchKernelGGL((conv2d_fwd_few_wino_f32<DLWP_ACT_LINEAR, QUAD>), dim3(grid), dim3(C::NT), C::LDS_BYTES, s, a, group);
}

}  // namespace

// Host logic only: does the kernel cover this launch?  (a.tiles_* need not be set.)  What conv_fwd_few.hip takes, narrowed to
// dilation 2, at most four input channels, whole 32-channel tiles and the pooled image alone.
bool dlwp_conv_few_wino_covers(const ConvArgs& a, int ks, int dil_h, int dil_w) {
  return dlwp_conv_few_covers(a, ks, dil_h, dil_w) && dil_h == 2 && a.Cin <= 4 && a.Cout % 32 == 0 && a.out_pool == 1 && !a.y2;
}

// a.tiles_h / tiles_w / cout_tiles = the 8 x 32 / 32-channel tiling; `grid` workgroups share tiles x N items
void dlwp_conv_few_wino_launch(const ConvArgs& a, int grid, hipStream_t s) {
  const bool quad = a.W % 4 == 0 && a.Ws == a.W && ((long long)a.Hs * a.Ws) % 4 == 0 && ((long long)a.in_c_off * a.Hs * a.Ws) % 4 == 0 &&
                    ((size_t)a.x & 15) == 0 && a.pad_left >= 0 && a.pad_left <= 4 &&
                    (a.mode_w == DLWP_PAD_ZERO || a.mode_w == DLWP_PAD_WRAP);
  if (quad) launch_few_wino<true>(a, grid, s);
  else launch_few_wino<false>(a, grid, s);
}
