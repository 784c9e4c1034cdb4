// philox.h -- Philox-4x32-10 (Salmon et al., SC'11), the library's counter-based generator: ten rounds on a 128-bit counter under a
// 64-bit key, no state.  Used by Dropout (csrc/dense.hip: counter (q lo, q hi, step, layer)) and by the ensemble member generator
// (csrc/perturb.hip: counter (column quad, row + channel, draw, sample)); tests/test_dense_cpu.py and tests/test_perturb_cpu.py pin
// the Python restatements to Random123's known answers.
#pragma once

__device__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* o) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
