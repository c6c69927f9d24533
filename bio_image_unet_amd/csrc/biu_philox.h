// Philox4x32-10 (Salmon et al., Random123) and the 24-bit uniform the augmentation kernels draw from it: shared by biu_augment.hip (uint8
// batches), biu_augment_f32.hip (float fields) and biu_augment_vol.hip (float volumes), so all read the one stream tests/augment_oracle.py restates.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace biu_philox {
struct U4 {
    uint32_t x, y, z, w;
};

// ten rounds, the key bumped between rounds
__host__ __device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ uint32_t word_of(const U4& r, int i) { return i == 0 ? r.x : i == 1 ? r.y : i == 2 ? r.z : r.w; }
__device__ __forceinline__ float uniform24(uint32_t u) { return (float)(u >> 8) * 5.9604644775390625e-08f; }     // (u >> 8) * 2^-24, exact
}  // namespace biu_philox
