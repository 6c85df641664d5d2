// kmer_window.h -- which bases of the packed stream end a valid window (indexer.py:144), stated once.
//
// The packed stream (kmer_pack.hip) holds valid bases only, one restart bit per base: the run of valid bases begins anew
// there.  The window of k bases that ends at base j is valid iff no restart lies among the k-1 positions behind its first
// base, i.e. at j-k+2 .. j: a shift-or smear of the restart bits over k-1 positions, for a word of bases at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pk {

// OR of x << s for s = 0 .. n-1: n = 0 .. 16 on 32-bit words, 0 .. 20 on 64-bit ones (k = 1 gives n = 0).  N_EVEN: the
// caller knows n to be even (deep windows, k = 19 and 21) and is spared the last term.
template <bool N_EVEN, typename T>
__device__ __forceinline__ T smear(T x, uint32_t n) {
    const T y1 = x | (x << 1), y2 = y1 | (y1 << 2), y3 = y2 | (y2 << 4), y4 = y3 | (y3 << 8);
    if (sizeof(T) == 4 && n >= 16u) return y4;                            // a 32-bit word: 16 is all there is
    T acc = 0;
    uint32_t off = 0;                                                     // n = 16 + 4 at most
    if (n & 16u) { acc |= y4; off = 16; }
    if (n & 8u) { acc |= y3 << off; off += 8; }
    if (n & 4u) { acc |= y2 << off; off += 4; }
    if (n & 2u) { acc |= y1 << off; off += 2; }
    if (!N_EVEN && (n & 1u)) { acc |= x << off; }
    return acc;
}

// The valid windows that END at each of a piece's nv pushed-together bases (bit j: one ends at base j), given the bases'
// restart bits as the piece alone knows them (F; base 0's is completed here: the run was already broken when the piece
// began) and the length of the run carried in: no restart among the k-1 positions behind the window's first base, and --
// where no restart precedes -- enough bases carried in.
__device__ __forceinline__ unsigned long long window_ends(unsigned long long &F, uint32_t nv, uint32_t run, uint32_t km1) {
    if (run == 0u && nv) F |= 1ull;
    const unsigned long long keep = nv >= 64u ? ~0ull : ((1ull << nv) - 1ull);
    const unsigned long long X = smear<false>(F, km1);
    const uint32_t short_by = run >= km1 ? 0u : km1 - run;                // leading positions the carried run cannot complete
    const unsigned long long lead = short_by >= 64u ? ~0ull : ((1ull << short_by) - 1ull);
    // a restart inside the piece takes over from the carried run: positions at or above the first restart obey X only
    const unsigned long long below_first = F ? ((F & (0ull - F)) - 1ull) : ~0ull;
    return ~X & ~(lead & below_first) & keep;
}

}  // namespace pk
