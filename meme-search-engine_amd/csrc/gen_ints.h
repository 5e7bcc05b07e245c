// The project's own generator (gen.hip, oracle/mse_oracle.c::orc_gen_row_ints): Philox-4x32-10 keyed by (seed, row); call c of a row gives
// components 2c and 2c + 1, each a centred Irwin-Hall sum of four 16-bit uniforms (an integer in [-131070, 131070], variance 65536^2 / 3).
#pragma once
#include <stdint.h>

namespace mse {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void pair_of(uint32_t seed, uint64_t row, uint32_t call, int& a, int& b) {
    uint32_t r[4];
    philox4x32_10(call, 0u, (uint32_t)row, (uint32_t)(row >> 32), seed, 0x5EEDu, r);
    a = (int)((r[0] & 0xffffu) + (r[0] >> 16) + (r[1] & 0xffffu) + (r[1] >> 16)) - 131070;
    b = (int)((r[2] & 0xffffu) + (r[2] >> 16) + (r[3] & 0xffffu) + (r[3] >> 16)) - 131070;
}

}  // namespace mse
