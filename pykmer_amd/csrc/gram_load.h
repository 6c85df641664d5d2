// gram_load.h -- how the merger kernels (gram_scan.hip, gram_spectrum.hip) read the staged table slices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pk {

constexpr uint32_t H4 = 0x80808080u, L4 = 0x7f7f7f7fu;

// The 32 addresses of "word" w.  Words are numbered so that the 64 lanes of a wave (64 consecutive words)
// cover one 2 KiB block with two fully contiguous 1 KiB load instructions: lane l of block B takes bytes
// [B*2048 + l*16, +16) and [B*2048 + 1024 + l*16, +16).  Which 32 addresses share a word does not matter to
// the tallies as long as every table uses the same grouping.  Bytes at or beyond n read as 0 (never valid).
__device__ __forceinline__ uint64_t n_words_for(uint64_t n) { return ((n + 2047u) / 2048u) * 64u; }

__device__ __forceinline__ uint4 load_half(const uint8_t *t, uint64_t off, uint64_t n) {
    if (off + 16u <= n) {
        // every byte is read exactly once: stream it past the caches (nontemporal)
        // (the table pointers come out of a pointer array, so the compiler cannot tell their address space and would emit
        // FLAT loads, which count on the LDS counter as well and complete out of order: every LDS wait then also drains the
        // loads in flight.  They are global memory: say so.)
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) u32x4 *gptr;
        const u32x4 x = __builtin_nontemporal_load((gptr)(t + off));
        return make_uint4(x.x, x.y, x.z, x.w);
    }
    uint32_t v[4] = {0, 0, 0, 0};
    const __attribute__((address_space(1))) uint8_t *tg = (const __attribute__((address_space(1))) uint8_t *)t;
    for (uint64_t i = off; i < n; i++) v[(i - off) >> 2] |= (uint32_t)tg[i] << (8u * ((i - off) & 3u));
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void load_word(const uint8_t *t, uint64_t w, uint64_t n, uint4 &a, uint4 &b) {
    const uint64_t off = (w >> 6) * 2048u + (w & 63u) * 16u;
    a = load_half(t, off, n);
    b = load_half(t, off + 1024u, n);
}

}  // namespace pk
