// Philox4x32-10 counter-based generator shared by the sampler's draws, dropout (sampler_kernels.hip) and the row-list
// dropout of full-batch training (spmm_large.hip, loss_kernels.hip): uniform i of a stream (seed, offset) is word i & 3 of
// philox4x32_10(offset + i / 4, seed), mapped to [0, 1) with 24 bits.
#pragma once
#include "common.h"

struct Philox4 { uint32_t v[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint64_t ctr, uint64_t seed) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 r; r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}
// The same generator over the whole 128-bit counter: ctr = the low 64 bits (c0, c1), hi = the high 64 bits (c2, c3).  With hi = 0 it
// is philox4x32_10(ctr, seed) word for word; the ego-net sampler (shadow_kernels.hip) keeps the node in the low half and the
// (call, root, hop) in the high half, so that no two of its draws share a counter.
__device__ __forceinline__ Philox4 philox4x32_10_wide(uint64_t ctr, uint64_t hi, uint64_t seed) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = (uint32_t)hi, c3 = (uint32_t)(hi >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 r; r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}
// raw 32-bit word i of the stream (seed, offset)
__device__ __forceinline__ uint32_t philox_word_at(uint64_t seed, uint64_t offset, long long i) {
    const Philox4 p = philox4x32_10(offset + (uint64_t)(i >> 2), seed);
    const int q = (int)(i & 3);                                  // (selects: a dynamic index would put the four words in LDS)
    return q == 0 ? p.v[0] : (q == 1 ? p.v[1] : (q == 2 ? p.v[2] : p.v[3]));
}
// (the same word by a dynamic index, kept: on philox_word_at's selects the kernels of the captured step that call this change their
// registers, LDS and scratch — profiles/row_list_resources.txt)
__device__ __forceinline__ float philox_uniform_at(uint64_t seed, uint64_t offset, long long i) {
    const Philox4 p = philox4x32_10(offset + (uint64_t)(i >> 2), seed);
    return (float)(p.v[i & 3] >> 8) * 5.9604644775390625e-08f;   // 2^-24
}

