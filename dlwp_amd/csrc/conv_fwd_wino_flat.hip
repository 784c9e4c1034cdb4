// conv_fwd_wino_flat.hip -- the Winograd F(2x2, 3x3) forward of conv_fwd_wino_kernel.h on FLAT RUNS of tiles, gfx950.
//
// The 8 x 32 instances cover a map with whole 8 x 32 rectangles.  On the 22 x 45 maps of the U-Net that multiplies padding:
//   layer 4 (128 -> 64 on the up-sampled 22 x 45 source, 44 x 90 out): 48 x 96 covered, 1152 tiles per image for 990 real ones;
//   layer 3 (64 -> 128 on 22 x 45, two samples side by side): 288 tiles per image for 253 real ones (11 x 23).
// No rectangle of 64 tiles divides those grids; a run does.  A workgroup here takes the 64 tiles g = 64 run ... 64 run + 63 of one
// image, numbered row-major over the tile grid (tile rows of a.tiles_w tiles), a.tiles_h = ceil(tiles per image / 64) runs per
// image: 1024 tile slots for layer 4 (3 % padding), 256 for layer 3 (1 %).
//
// The kernel is conv2d_fwd_wino_body<C> with C = WinoFlatCfg: the same pipeline, filter staging, MFMA order, input transform and
// output transform (WinoCfg::FLAT selects the differences, which are all per-lane offsets):
//   * the loader stages the WHOLE rows the run's patches touch -- up to FR tile rows: 2 FR + 2 image rows, columns -1 ... 46 of a
//     plain source; FR + 2 SOURCE rows of an up-sampled one, each source element written to the two column slots it replicates
//     into (the patch's rows 1 and 2 are then one LDS row: vt_read) -- for every chunk of 8 channels;
//   * a lane's patch origin is its tile's place in those rows;
//   * the outputs are staged [co][tile row][tile][tile column] and leave as the run's row segments.
// Same values in the same patch positions, the same multiplies in the same order: the bits of the 8 x 32 instances (and so of
// every batch size and schedule that picks either).
#include "conv_fwd_wino_kernel.h"

namespace {

template <bool UPS_, int BNF_>
struct WinoFlatCfg : WinoCfg<1, 8, 32, 4, BNF_, 8, false, UPS_> {
  using Base = WinoCfg<1, 8, 32, 4, BNF_, 8, false, UPS_>;
  static constexpr bool FLAT = true;
  static constexpr int FR = UPS_ ? 3 : 4;        // tile rows a run may touch (host: wino_flat_runs)
  static constexpr int NCOL = 48;                // columns staged per row: -1 ... 46 (host: at most 46 tile / source columns + halo)
  static constexpr int LR = UPS_ ? FR + 2 : 2 * FR + 2;
  static constexpr int LCP = UPS_ ? 2 * NCOL + 2 : NCOL;   // (up-sampled: source column c in slots 2 c + 3, 2 c + 4)
  static constexpr int PS_RAW = LR * LCP;
  static constexpr int PS = PS_RAW + (((16 - PS_RAW % 32) % 32) + 32) % 32;
  static constexpr int X_FLOATS = Base::CK * PS;
  static constexpr int L_FLOATS =
      (2 * X_FLOATS + 2 * Base::U_FLOATS) > Base::O2_FLOATS ? (2 * X_FLOATS + 2 * Base::U_FLOATS) : Base::O2_FLOATS;
  static constexpr int LDS_BYTES = L_FLOATS * 4;
  static constexpr int NPOS = (LR * NCOL + Base::NT - 1) / Base::NT;
  static constexpr int XRW = NPOS;
  static constexpr int NXI = Base::CK * NPOS;
  static_assert(Base::T == 64 && Base::TPAD == 64 && Base::RTW == 16, "a run is the 64 tiles of the four waves");
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

template <class C>
__global__ __launch_bounds__(C::NT, C::WAVES_PER_SIMD) void conv2d_fwd_wino_flat_f32(const ConvArgs a) {
  conv2d_fwd_wino_body<C>(a, blockIdx.x, gridDim.x);
}

template <class C>
int launch_flat(const ConvArgs& a, int grid, hipStream_t s) {
  static int prepared = -1;
  if (prepared < 0 && C::LDS_BYTES > 64 * 1024)
    prepared = (int)hipFuncSetAttribute((const void*)conv2d_fwd_wino_flat_f32<C>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        C::LDS_BYTES);
  if (prepared > 0) return prepared;
  prepared = 0;
  hipLaunchKernelGGL((conv2d_fwd_wino_flat_f32<C>), dim3(grid), dim3(C::NT), C::LDS_BYTES, s, wino_derive(a));
  return 0;
}

}  // namespace

// Host logic only: runs per image when the flat kernel covers this launch of a 32- (bnf 2) or 64-channel (bnf 4) Winograd
// instance, else 0.  3 x 3 'same' convolution (odd halo of 1), dilation 1 (caller), float32 in and out, a plain source or a 2x
// up-sampled one, zero / periodic / edge halos (they commute with the up-sampling), whole chunks of 8 input channels, whole
// 32 / 64-channel output tiles, no fused epilogue.  The staged rows hold 48 columns and FR tile rows: the tile grid is at most
// 23 (plain) / 46 (up-sampled: one tile per source pixel) wide and no run of 64 tiles touches more than FR of its rows.
int dlwp_conv_wino_flat_runs(const ConvArgs& a, int bnf) {
  const auto commutes = [](int m) { return m == DLWP_PAD_ZERO || m == DLWP_PAD_WRAP || m == DLWP_PAD_EDGE; };
  if (bnf != 2 && bnf != 4) return 0;
  if (a.in_bf16 || a.out_bf16 || a.compute_bf16 || a.in_oct || a.out_oct || a.out_pool || a.y2 || a.yact || a.lstm_f || a.out_d2s ||
      a.ksplit > 1 || a.col0 != 0)
    return 0;
  if (a.pad_top != 1 || a.pad_left != 1 || !commutes(a.mode_h) || !commutes(a.mode_w) || a.Ho != a.H || a.Wo != a.W) return 0;
  if (a.Cin % 8 != 0 || a.Cout % (16 * bnf) != 0) return 0;
  const bool ups = a.src_mode == DLWP_SRC_UPSAMPLE2;
  if (ups ? (a.H != 2 * a.Hs || a.W != 2 * a.Ws) : (a.src_mode != DLWP_SRC_DIRECT || a.H != a.Hs || a.W != a.Ws)) return 0;
  if (!ups && bnf != 2) return 0;
  const int tw = (a.Wo + 1) / 2, th = (a.Ho + 1) / 2, fr = ups ? 3 : 4;
  if ((ups ? tw : 2 * tw) + 2 > 48) return 0;
  const long long tiles = (long long)tw * th;
  if ((long long)a.Hs * a.Ws * a.in_c_total >= (1ll << 28) || (long long)a.Ho * a.Wo * a.out_c_total >= (1ll << 28)) return 0;
  const long long runs = (tiles + 63) / 64;
  for (long long r = 0; r < runs; ++r) {
    const long long last = (r * 64 + 63 < tiles ? r * 64 + 63 : tiles - 1);
    if (last / tw - (r * 64) / tw + 1 > fr) return 0;
  }
  return (int)runs;
}

// a.tiles_w = (Wo + 1) / 2, a.tiles_h = runs per image, a.cout_tiles = Cout / (16 bnf), a.w = the transformed filters; grid =
// N x runs x cout_tiles.  Returns 0 or the HIP error of the attribute call.
int dlwp_conv_wino_flat_launch(const ConvArgs& a, int bnf, int grid, hipStream_t s) {
  if (a.src_mode == DLWP_SRC_UPSAMPLE2)
    return bnf == 4 ? launch_flat<WinoFlatCfg<true, 4>>(a, grid, s) : launch_flat<WinoFlatCfg<true, 2>>(a, grid, s);
  return launch_flat<WinoFlatCfg<false, 2>>(a, grid, s);
}
