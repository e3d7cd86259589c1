// Philox4x32-10 and the open-unit uniform of the device variates: the Gibbs draws (abi_gibbs.hip) and the PRS-CS variates
// (abi_cs.hip) take their random words from here, one block per (SNP, column).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace viprs {

// Philox4x32-10 (Salmon et al. 2011), the published constants
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// (2 (x >> 9) + 1) 2^-24: an odd multiple of 2^-24 below 1, exact in float32
__device__ __forceinline__ float open_unit(uint32_t x) { return (float)(2u * (x >> 9) + 1u) * 0x1p-24f; }

}  // namespace viprs
