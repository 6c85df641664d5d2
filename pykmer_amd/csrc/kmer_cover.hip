// kmer_cover.hip -- which bases of a query text the tables cover, and the text with those bases marked.
//
// The valid bases of the stream -- ACGTacgt in sequence lines of a record, exactly the bases of the packed stream -- are
// numbered g = 0, 1, .. in text order over all feeds.  A base is COVERED iff it lies in a valid window whose canonical
// k-mer has min <= T_t[a] <= max in at least one table t.  Phase 1 (pk_query_set_cover) leaves one bit per valid base in
// HBM; phase 2 (pk_query_set_mask) takes such bits back and patches them into the text.  Two phases because a base at the
// end of a feed may be covered only by a window that ends in the next one.
//   k_cover_scan    one workgroup: base_first[c] = the valid bases of the stream before slot c, from the squeeze's n_bases[]
//                   and the count at the end of the feed before (nb[in]); leaves the count behind this feed in nb[out].  The
//                   host makes `out` the next feed's `in` only once the feed has settled, as for the positions of
//                   kmer_coords.hip, so that a repeated feed (flags[0] = 2) starts from the same count.
//   k_query_cover   one workgroup per slot, 16 windows per thread (q_lane and q_kmers of the lookup): one 16-bit plane "window
//                   j is valid and matches", OR-ed over the tables of the launch.  A matching window that ends at base g of
//                   the stream covers the bases g-k+1 .. g -- all of them in the stream and in one run, or the window would
//                   not be valid -- so in base ordinals the cover is pure arithmetic: the plane smeared back over k-1
//                   positions (32 bits at most), OR-ed into an LDS bitmap of the slot that begins one word in front of it, and
//                   the non-zero words flushed with atomicOr at base_first[c].  Slot starts, slots with fewer than k-1 bases
//                   and feed seams need no case of their own; neighbouring slots and later launches meet in the edge words.
//   k_mask_apply    text geometry (256 lanes per 16 KiB chunk, 64 bytes per lane, lane_start): the mask of a lane's valid
//                   bases of live records (clean pieces from piece_scan, the others by the rolled byte loop in the waves that
//                   hold one), prefix-summed behind base_first[c]; the lane's <= 64 cover bits from that bit offset,
//                   deposited onto the set bits of the mask, patched into the lane's bytes in LDS; the chunk leaves through
//                   a buffer of its own, so that a repeated feed parses the text it parsed before.
// Like the kernels of kmer_query.hip all return at once, writing nothing, when flags[0] is raised; OR is idempotent.
#include "kmer_pieces.h"
#include "kmer_qlane.h"
#include "wg_scan.h"

namespace pk {

constexpr uint32_t COVER_LDS_WORDS = 516;   // 16384 bits of the slot, 32 in front (the reach of its first windows), 31 of alignment

__global__ __launch_bounds__(QNT) void k_cover_scan(const uint32_t *__restrict__ n_bases, uint32_t n_chunks,
                                                    const unsigned long long *__restrict__ nb_in, unsigned long long *__restrict__ nb_out,
                                                    unsigned long long *__restrict__ base_first, const uint32_t *__restrict__ flags) {
    __shared__ unsigned long long wsum[QNT / 64];
    if (flags[0]) return;
    unsigned long long run = *nb_in;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += QNT) {
        const uint32_t c = c0 + threadIdx.x;
        const unsigned long long v = c < n_chunks ? n_bases[c] : 0ull;
        unsigned long long total;
        const unsigned long long ex = wg_excl_sum<QNT / 64, true>(v, wsum, total);   // wsum may still be read by the round before
        if (c < n_chunks) base_first[c] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) *nb_out = run;
}

template <typename KT>
__global__ __launch_bounds__(QNT) void k_query_cover(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ restarts,
                                                     const uint32_t *__restrict__ n_bases, const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                     const unsigned long long *__restrict__ base_first, QueryTables tabs, uint32_t n_tab,
                                                     uint32_t min_count, uint32_t max_count, uint32_t *__restrict__ bitmap,
                                                     unsigned long long n_words, const uint32_t *__restrict__ flags) {
    __shared__ uint32_t bm[COVER_LDS_WORDS];
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const uint32_t nb = n_bases[c];
    if (nb == 0u) return;
    for (uint32_t i = threadIdx.x; i < COVER_LDS_WORDS; i += QNT) bm[i] = 0u;
    __syncthreads();
    const QLane q = q_lane(codes, restarts, nb, chunk_l2_state, c, threadIdx.x, k);
    uint32_t m = 0u;                                         // bit j: window j is valid and matches in a table of the launch
    if (__any(q.ok != 0u)) {
        KT a[16];
        q_kmers<KT>(q, k, a);
        for (uint32_t tt = 0; tt < n_tab; tt++) {
            if (__all(m == q.ok)) break;                     // every valid window of the wave matches already
            const uint8_t *__restrict__ T = tabs.t[tt];
            uint32_t cv[16];                                 // all gathers of a table in flight before the first is used
#pragma unroll
            for (int j = 0; j < 16; j++) cv[j] = ((q.ok >> j) & 1u) ? (uint32_t)T[a[j]] : 0u;   // a count of 0 lies in no window (min >= 1)
#pragma unroll
            for (int j = 0; j < 16; j++) m |= (cv[j] >= min_count && cv[j] <= max_count) ? 1u << j : 0u;
        }
    }
    // the window that ends at the thread's base j covers j-k+1 .. j: with the 16 positions before the thread's own in the
    // low half of a word, the plane smeared towards bit 0 over k positions (mirrored: smear runs towards the top)
    const unsigned long long first = base_first[c];
    if (m) {
        const uint32_t mirrored = __builtin_bitreverse32(m << 16);
        const uint32_t y = __builtin_bitreverse32((uint32_t)smear<false>((unsigned long long)mirrored, k));
        // LDS bit s + 32 + p holds position p of the slot (s: the bit of the slot's first base in its HBM word); y's bit 0
        // is position 16 t - 16
        const uint32_t at = (uint32_t)(first & 31ull) + 16u + 16u * threadIdx.x, w = at >> 5, sh = at & 31u;
        const uint32_t lo = y << sh, hi = sh ? y >> (32u - sh) : 0u;
        if (lo) atomicOr(&bm[w], lo);
        if (hi) atomicOr(&bm[w + 1u], hi);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < COVER_LDS_WORDS; i += QNT) {
        const uint32_t v = bm[i];
        const unsigned long long gw = (first >> 5) + i;      // LDS word i is HBM word first / 32 - 1 + i
        if (v && gw >= 1ull && gw - 1ull < n_words) atomicOr(&bitmap[gw - 1ull], v);
    }
}

// One piece walked byte by byte from its exact start state, as SeqWalker::step walks it (byte i <-> bit i): the valid bases
// of live records and the bytes that open a record.
struct MaskPiece { unsigned long long valid, hdrm; };
__device__ __forceinline__ MaskPiece mask_walk(const uint8_t *mine, uint32_t nb, uint32_t ls_in, const L2 &st) {
    MaskPiece mp; mp.valid = 0; mp.hdrm = 0;
    uint32_t ls = ls_in;
    bool live = st.rec != 0u;                                // text before the first header is dropped
    for_each_byte_of(mine, nb, [&](uint32_t i, uint32_t c, bool act) {
        const bool term = is_term(c), ws = is_ws(c), gt = c == '>';
        const bool at_start = ls == LS_START, in_seq = ls == LS_SEQ;
        const bool hdr_start = act && at_start && !ws && gt;
        const bool seqchar = act && !ws && (in_seq || (at_start && !gt));
        const bool t = act && term;
        const unsigned long long bit = 1ull << i;
        if (hdr_start) { live = true; mp.hdrm |= bit; }
        ls = t ? (uint32_t)LS_START : hdr_start ? (uint32_t)LS_HEADER : seqchar ? (uint32_t)LS_SEQ : ls;
        mp.valid |= (seqchar && base_code(c) < 4u && live) ? bit : 0ull;
    });
    return mp;
}

// 4 flag bits -> 0xff in every flagged byte of a dword, byte 0 lowest
__device__ __forceinline__ uint32_t byte_mask4(uint32_t four) { return (((four & 15u) * 0x00204081u) & 0x01010101u) * 0xffu; }

__global__ __launch_bounds__(WG) void k_mask_apply(const uint8_t *__restrict__ fasta, uint64_t n_bytes, const LaneState *__restrict__ lane_state,
                                                   const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                   const unsigned long long *__restrict__ base_first, const uint32_t *__restrict__ bits,
                                                   unsigned long long n_words, uint32_t mode, uint8_t *__restrict__ out,
                                                   unsigned long long *__restrict__ masked, unsigned long long recs_cap,
                                                   const uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint8_t text[WG * LDS_STRIDE];
    __shared__ uint32_t sh32[WG / 64];
    __shared__ unsigned long long wave_sum[WG / 64];
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const uint64_t base = (uint64_t)c * CHUNK;
    const L2 chunk_st = chunk_l2_state[c];
    const LaneStart ln = lane_start(lane_state[(uint64_t)c * WG + threadIdx.x], chunk_st, k - 1u);
    const L2 &st = ln.st;
    const uint32_t rec0 = chunk_st.rec;                      // the record open at the chunk's first byte (1-based; 0: none)
    stage_chunk(fasta, base, n_bytes, text);
    __syncthreads();
    uint8_t *mine = text + threadIdx.x * LDS_STRIDE;
    const uint32_t nb = piece_len(base, n_bytes);
    // a clean piece (plain sequence text) by masks: its valid bases are the letters piece_scan finds, and no record opens
    PieceMasks pm;
    uint32_t cw[4];
    piece_scan(mine, nb, pm, cw);
    MaskPiece mp;
    mp.valid = st.rec != 0u ? pm.valid : 0ull;
    mp.hdrm = 0ull;
    if (__any(!ln.clean)) {
        const MaskPiece walked = mask_walk(mine, nb, ln.ls_in, st);
        if (!ln.clean) mp = walked;
    }
    const uint32_t nv = (uint32_t)__popcll(mp.valid);
    uint32_t total;
    const uint32_t off = wg_excl_sum<WG / 64, false>(nv, sh32, total);   // sh32: first use
    // the lane's cover bits: nv bits from bit g0 of the bitmap, on the bytes of its valid bases
    const unsigned long long sel = nv ? cover_select(mp.valid, base_first[c] + off, bits, n_words, (mode & MASK_INVERT) != 0u) : 0ull;
    // the lane's own bytes, in LDS; only dwords that change are written
    if (sel) {
        uint32_t *dw = reinterpret_cast<uint32_t *>(mine);
#pragma unroll
        for (uint32_t d = 0; d < (uint32_t)PIECE / 4u; d++) {
            const uint32_t bm = byte_mask4((uint32_t)(sel >> (4u * d)));
            if (bm) dw[d] = (mode & MASK_HARD) ? ((dw[d] & ~bm) | (bm & 0x4e4e4e4eu)) : (dw[d] | (bm & 0x20202020u));
        }
    }
    // masked[rec], by the walker's own record number (1-based): where one record holds the whole chunk (the genome case)
    // the chunk's sum takes one atomic, behind the barrier below; otherwise one per wave that lies in one record, and in the
    // other waves one per lane and record (a header ends the one before)
    const bool chunk_one = (bool)__syncthreads_and(mp.hdrm == 0ull && st.rec == rec0);
    const bool wave_one = chunk_one || (__all(mp.hdrm == 0ull) && __all(st.rec == (uint32_t)__builtin_amdgcn_readfirstlane((int)st.rec)));
    if (wave_one) {
        unsigned long long n = (unsigned long long)__popcll(sel);
        for (int s = 32; s; s >>= 1) n += __shfl_down(n, s, 64);
        if ((threadIdx.x & 63u) == 0u) {
            if (chunk_one) wave_sum[threadIdx.x >> 6] = n;
            else if (n && st.rec && st.rec <= recs_cap) atomicAdd(&masked[st.rec - 1u], n);
        }
    } else {
        unsigned long long left = sel, hdrs = mp.hdrm, rec = st.rec;
        for (;;) {
            const unsigned long long seg = hdrs ? ((hdrs & (0ull - hdrs)) - 1ull) : ~0ull;   // the bytes below the next header
            const unsigned long long n = (unsigned long long)__popcll(left & seg);
            if (n && rec && rec <= recs_cap) atomicAdd(&masked[rec - 1ull], n);
            if (!hdrs) break;
            left &= ~seg;
            hdrs &= hdrs - 1ull;
            rec++;
        }
    }
    __syncthreads();
    if (chunk_one && threadIdx.x == 0) {
        unsigned long long n = 0ull;
        for (int w = 0; w < WG / 64; w++) n += wave_sum[w];
        if (n && rec0 && rec0 <= recs_cap) atomicAdd(&masked[rec0 - 1u], n);
    }
    // the chunk out, coalesced 16 B per lane as it came in (out holds n_bytes + 64 bytes)
#pragma unroll
    for (int i = 0; i < CHUNK / (WG * 16); i++) {
        const uint32_t p = i * WG + threadIdx.x, bo = p * 16u;
        const uint64_t g = base + (uint64_t)bo;
        if (g < n_bytes) *reinterpret_cast<uint4 *>(out + g) = *reinterpret_cast<const uint4 *>(text + (bo / PIECE) * LDS_STRIDE + (bo % PIECE));
    }
}

// ------------------------------------------------------------------ host side -------------------
void launch_cover_scan(const PartPlan &pl, const PartBuffers &b, const unsigned long long *nb_in, unsigned long long *nb_out,
                       unsigned long long *base_first, hipStream_t s) {
    hipLaunchKernelGGL(k_cover_scan, dim3(1), dim3(QNT), 0, s, (const uint32_t *)b.n_bases, pl.n_chunks, nb_in, nb_out, base_first,
                       (const uint32_t *)b.flags);
}

void launch_query_cover(const PartPlan &pl, const PartBuffers &b, const L2 *st2, const unsigned long long *base_first, const uint8_t *const *tables,
                        uint32_t n_tab, uint32_t min_count, uint32_t max_count, uint32_t *bitmap, uint64_t n_words, hipStream_t s) {
    const QueryTables tabs = query_tables(tables, n_tab);
#define PK_QUERY_COVER(KT) hipLaunchKernelGGL(k_query_cover<KT>, dim3(pl.n_chunks), dim3(QNT), 0, s, (const uint32_t *)b.codes, (const uint32_t *)b.restarts, \
                                              (const uint32_t *)b.n_bases, st2, pl.k, base_first, tabs, n_tab, min_count, max_count, bitmap,                 \
                                              (unsigned long long)n_words, (const uint32_t *)b.flags)
    if (pl.k <= 15) PK_QUERY_COVER(uint32_t); else PK_QUERY_COVER(uint64_t);
#undef PK_QUERY_COVER
}

void launch_mask_apply(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state, const L2 *st2,
                       const unsigned long long *base_first, const uint32_t *bits, uint64_t n_words, uint32_t mode, uint8_t *out,
                       unsigned long long *masked, uint64_t recs_cap, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_apply, dim3(pl.n_chunks), dim3(WG), 0, s, fasta, n, lane_state, st2, pl.k, base_first, bits, (unsigned long long)n_words, mode,
                       out, masked, (unsigned long long)recs_cap, (const uint32_t *)b.flags);
}

}  // namespace pk
