// wino_phase_timing.hip -- where does a block of the Winograd forward kernel spend its life?  s_memtime stamps of wave 0
// (DLWP_STAMP in conv_fwd_wino_kernel.h; 16 slots per block), in the order they are taken:
//   0 entry | 7 every global load of chunk 0 issued | 8 chunk 0 written to LDS (its data has landed) | 1 in front of the first MFMA |
//   2 behind the last MFMA | 3 barrier | 4 output transform + activation written to LDS | 5 barrier | 6 last store issued
// Shapes = the four launches of the cfg2 U-Net's 256-member forward that run conv2d_fwd_wino_body, on the instances the library
// takes for them: layers 2 and 5 (44 x 90) on the column-pair + edge-pair 8 x 32 instance, layer 3 (22 x 45) and layer 4 (up-sampled
// 22 x 45 -> 44 x 90) on flat runs.  Random data; only the timing is meaningful.
// Build: hipcc -O3 -std=c++17 -fno-slp-vectorize -mllvm -pragma-unroll-threshold=1000000 --offload-arch=gfx950 -DDLWP_PHASE_TIMING
//        -o wino_phase_timing.bin wino_phase_timing.hip
#include "../../dlwp_amd/csrc/conv_fwd_wino_flat.hip"
#include <algorithm>
#include <cstdio>
#include <vector>

void dlwp_set_error(const char*, ...) {}

template <class C>
__global__ __launch_bounds__(C::NT, C::WAVES_PER_SIMD) void timed_kernel(const ConvArgs a) {
  conv2d_fwd_wino_body<C>(a, blockIdx.x, gridDim.x);
}

template <class C>
static void run(const char* what, int N, int Cin, int Cout, int H, int W, int out_pool, int src_mode) {
  ConvArgs a{};
  const int Hs = src_mode == 1 ? H / 2 : H, Ws = src_mode == 1 ? W / 2 : W;
  size_t xe = (size_t)N * Cin * Hs * Ws, ue = (size_t)Cin * Cout * 16;
  const int Ho = H, Wo = W, Hp = out_pool ? H / 2 : H, Wp = out_pool ? W / 2 : W;
  size_t ye = (size_t)N * Cout * Hp * Wp;
  float *x, *u, *y, *b;
  hipMalloc(&x, xe * 4); hipMalloc(&u, ue * 4); hipMalloc(&y, ye * 4); hipMalloc(&b, Cout * 4);
  std::vector<float> hx(xe), hu(ue);
  unsigned s = 12345;
  for (auto& v : hx) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xffff) / 32768.f - 1.f; }
  for (auto& v : hu) { s = s * 1664525u + 1013904223u; v = (((s >> 8) & 0xffff) / 32768.f - 1.f) * 0.05f; }
  hipMemcpy(x, hx.data(), xe * 4, hipMemcpyHostToDevice);
  hipMemcpy(u, hu.data(), ue * 4, hipMemcpyHostToDevice);
  hipMemset(b, 0, Cout * 4);
  a.x = x; a.w = u; a.bias = b; a.y = y;
  a.N = N; a.Cin = Cin; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
  a.in_c_off = 0; a.in_c_total = Cin; a.out_c_off = 0; a.out_c_total = Cout;
  a.pad_top = 1; a.pad_left = 1; a.mode_h = DLWP_PAD_ZERO; a.mode_w = DLWP_PAD_WRAP;
  a.src_mode = src_mode; a.act = DLWP_ACT_TANH;
  a.out_pool = out_pool; a.Hp = Hp; a.Wp = Wp; a.in_bf16 = 0; a.out_bf16 = 0; a.compute_bf16 = 0; a.col0 = 0;
  a.cout_tiles = Cout / C::BN;
  int grid;
  if constexpr (C::FLAT) {            // as conv_fwd.hip fills a flat launch
    a.tiles_w = (Wo + 1) / 2;
    a.tiles_h = (a.tiles_w * ((Ho + 1) / 2) + 63) / 64;
    grid = N * a.tiles_h * a.cout_tiles;
  } else {                            // ... and an edge-pair launch
    a.tiles_h = (Ho + C::TH - 1) / C::TH; a.tiles_w = (Wo + C::TW - 1) / C::TW;
    a.edge_pairs = C::EP ? 1 : 0;
    grid = (C::EP ? a.tiles_w * (a.tiles_h - 1) + (a.tiles_w + 1) / 2 : a.tiles_h * a.tiles_w) * a.cout_tiles * N;
  }
  a = wino_derive(a);
  long long* dbg;
  hipMalloc(&dbg, sizeof(long long) * 16 * grid);
  hipMemset(dbg, 0, sizeof(long long) * 16 * grid);
  if (C::LDS_BYTES > 64 * 1024)
    hipFuncSetAttribute((const void*)timed_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
  a.dbg = nullptr;
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL((timed_kernel<C>), dim3(grid), dim3(C::NT), C::LDS_BYTES, 0, a);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0);
  for (int i = 0; i < 10; ++i) hipLaunchKernelGGL((timed_kernel<C>), dim3(grid), dim3(C::NT), C::LDS_BYTES, 0, a);
  hipEventRecord(e1);
  hipDeviceSynchronize();
  float ms = 0; hipEventElapsedTime(&ms, e0, e1); ms /= 10;
  a.dbg = dbg;
  hipLaunchKernelGGL((timed_kernel<C>), dim3(grid), dim3(C::NT), C::LDS_BYTES, 0, a);
  if (hipDeviceSynchronize() != hipSuccess) { printf("%s: the launch failed\n", what); exit(1); }
  std::vector<long long> h(16 * (size_t)grid);
  hipMemcpy(h.data(), dbg, sizeof(long long) * h.size(), hipMemcpyDeviceToHost);
  static const int order[9] = {0, 7, 8, 1, 2, 3, 4, 5, 6};
  double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int bI = 0; bI < grid; ++bI) {
    for (int k = 0; k < 8; ++k) ph[k] += (double)(h[bI * 16 + order[k + 1]] - h[bI * 16 + order[k]]);
  }
  double life = 0;
  for (int k = 0; k < 8; ++k) { ph[k] /= grid; life += ph[k]; }
  const int chunks = (Cin + 7) / 8;
  printf("%s: grid %d, %d chunks, %.4f ms per launch (unstamped runs); mean block life %.0f cycles\n", what, grid, chunks, ms, life);
  printf("   entry -> chunk-0 loads issued %.0f | -> chunk 0 in LDS %.0f | -> first MFMA %.0f | loop %.0f (%.0f per chunk) | barrier %.0f | "
         "transform+act %.0f | barrier %.0f | stores %.0f   [in front of the first MFMA %.0f, behind the last %.0f]\n",
         ph[0], ph[1], ph[2], ph[3], ph[3] / chunks, ph[4], ph[5], ph[6], ph[7], ph[0] + ph[1] + ph[2], ph[4] + ph[5] + ph[6] + ph[7]);
  hipFree(x); hipFree(u); hipFree(y); hipFree(b); hipFree(dbg);
}

int main() {
  typedef WinoCfg<1, 8, 32, 4, 2, 8, false, false, false, false, false, true, false, true> PairEdge;
  run<PairEdge>("layer 2  32->64 @44x90, pooled epilogue (column pairs + edge pairs)", 256, 32, 64, 44, 90, 1, 0);
  run<WinoFlatCfg<false, 2>>("layer 3  64->128 @22x45 (flat runs)", 256, 64, 128, 22, 45, 0, 0);
  run<WinoFlatCfg<true, 4>>("layer 4  128->64 @44x90 up-sampled source (flat runs, 64 channels / block)", 256, 128, 64, 44, 90, 0, 1);
  run<PairEdge>("layer 5  64->32 @44x90 (column pairs + edge pairs)", 256, 64, 32, 44, 90, 0, 0);
  return 0;
}
