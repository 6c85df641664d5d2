// kmer_qlane.h -- what one thread of a slot of the packed stream works on, for the kernels that look its windows up
// (kmer_query.hip, kmer_cover.hip): its 16 bases, the 16 before them, which of its bases end a valid window, and the
// canonical k-mers of those windows.  k <= 17: the 16 bases before a thread's own 16 are all the history a window needs.
#pragma once
#include "kmer_window.h"
#include "pk_kernels.h"

namespace pk {

constexpr int QNT = 1024;                 // threads per slot, 16 bases each

// What thread t of a slot works on: its 16 bases, the 16 before them, and which of its bases end a valid window.
struct QLane { uint32_t cur, prev, ok; };
__device__ __forceinline__ QLane q_lane(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ restarts, uint32_t nb,
                                        const L2 *__restrict__ chunk_l2_state, uint32_t c, uint32_t t, uint32_t k) {
    QLane q; q.cur = 0; q.prev = 0; q.ok = 0;
    if (16u * t >= nb) return q;                             // words past the base count hold an earlier feed's bits
    const uint32_t cnt = min(16u, nb - 16u * t), km1 = k - 1u;
    const uint32_t *cw = codes + (uint64_t)c * SLOT_CODE_WORDS;
    const uint32_t *rw = restarts + (uint64_t)c * SLOT_RST_WORDS;
    q.cur = cw[t];
    const uint32_t rword = rw[t >> 1];
    uint32_t r;                                              // restart bits: the 16 bases before (low half), the own 16 (high half)
    if (t == 0u) {
        // in front of the slot: the chunk's start state, newest base lowest -> stream order; of its bases only the
        // last `len` belong to the open run
        const L2 st = chunk_l2_state[c];
        const uint32_t len = l2_len(st);
        q.prev = revpairs32(st.bits);
        r = rword << 16;
        if (len < km1) r |= 1u << (16u - len);
    } else {
        q.prev = cw[t - 1u];
        r = (t & 1u) ? rword : ((rword << 16) | (rw[(t >> 1) - 1u] >> 16));
    }
    q.ok = ~(smear<false>(r, km1) >> 16) & ((1u << cnt) - 1u);
    return q;
}

// The canonical k-mers of the thread's 16 windows (indexer.py:149-150, 341): a[j] for the window that ends at its base j.
template <typename KT>
__device__ __forceinline__ void q_kmers(const QLane &q, uint32_t k, KT (&a)[16]) {
    const KT mask = (KT)((2u * k >= sizeof(KT) * 8u) ? ~(KT)0 : (((KT)1 << (2u * k)) - 1));
    const unsigned long long fwd64 = ((unsigned long long)revpairs32(q.prev) << 32) | revpairs32(q.cur);          // first base highest
    const unsigned long long rev64 = (~(((unsigned long long)q.cur << 32) | q.prev)) >> (2u * (17u - k));       // complemented, first base lowest
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const KT f = (KT)(fwd64 >> (2u * (15u - j))) & mask, rv = (KT)(rev64 >> (2u * j)) & mask;
        a[j] = f < rv ? f : rv;
    }
}

}  // namespace pk
