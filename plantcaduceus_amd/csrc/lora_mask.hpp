// The dropout mask of a LoRA branch: a pure function of (seed, stream, row, column), so that the backward regenerates
// it instead of reading a stored one.  Plain C++: host and device compile the same text.
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants)
//   counter = (k >> 3, m, stream_lo, stream_hi), key = (seed_lo, seed_hi)  ->  w0..w3: 8 x 16 bits, one call per 8 consecutive columns
//   h(m, k) = (w[(k & 7) >> 1] >> 16 (k & 1)) & 0xffff        keep(m, k) = h >= T        T = floor(p 65536 + 0.5)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCAD_HD __host__ __device__ __forceinline__
#else
#define PCAD_HD inline
#endif

namespace pcad {

PCAD_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;  c[1] = (uint32_t)p1;  c[2] = n2;  c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;  k1 += 0xBB67AE85u;
    }
}

// bit i of the result: keep(m, 8 k8 + i)
PCAD_HD uint32_t lora_keep8(uint32_t T, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_lo, uint32_t stream_hi, uint32_t m, uint32_t k8) {
    uint32_t c[4] = {k8, m, stream_lo, stream_hi};
    philox4x32_10(c, seed_lo, seed_hi);
    uint32_t keep = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t h = (c[i >> 1] >> (16 * (i & 1))) & 0xffffu;
        keep |= (uint32_t)(h >= T) << i;
    }
    return keep;
}

}  // namespace pcad
