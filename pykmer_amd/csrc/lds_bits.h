// lds_bits.h -- placing a lane's bits in a bit array in LDS: how the structure pass (kmer_count.hip) and the squeeze pass
// (kmer_pack.hip) put a piece's codes and restart bits into the chunk's slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pk {

// OR `n_bits` bits of (lo, hi) into the LDS bit array `dst` at bit offset `at`
__device__ __forceinline__ void lds_or_bits(uint32_t *dst, uint32_t at, unsigned long long lo, unsigned long long hi, uint32_t n_bits) {
    if (n_bits == 0) return;
    const uint32_t w0 = at >> 5, sh = at & 31u;
    const uint32_t x[5] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0u};
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint32_t v = sh ? ((x[i] << sh) | carry) : x[i];
        carry = sh ? (x[i] >> (32u - sh)) : 0u;
        if (v) atomicOr(&dst[w0 + i], v);                    // words past the lane's bits are all zero and skipped
    }
}

}  // namespace pk
