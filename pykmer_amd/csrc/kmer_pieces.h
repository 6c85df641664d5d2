// kmer_pieces.h -- what the kernels that walk a feed's text again behind the squeeze share (kmer_coords.hip, kmer_cover.hip,
// kmer_intervals.hip): the position pair of a stretch of text with its scans, the byte-wise walk that finds a piece's
// positions, and the cover bits of a piece's valid bases.  Positions are counted as DevRec.seq_len counts them
// (SeqWalker::step, kmer_walk.h); see kmer_coords.hip.
#pragma once
#include "pk_kernels.h"

namespace pk {

constexpr unsigned long long CP_HDR = 1ull << 63;        // a pair in one word: bit 63 = a record opens, the rest = positions

__device__ __forceinline__ unsigned long long cp_compose(unsigned long long a, unsigned long long b) {   // a first, then b
    return (b & CP_HDR) ? b : a + b;
}

// inclusive scan of pairs over a wave
__device__ __forceinline__ unsigned long long cp_wave_incl(unsigned long long v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v = cp_compose(o, v);
    }
    return v;
}

// Exclusive scan of pairs over the workgroup's NW waves (sh: NW words); total = all of them composed.  The pair before
// lane 0 is the identity (0).
template <int NW>
__device__ __forceinline__ unsigned long long cp_block_excl(unsigned long long v, unsigned long long *sh, unsigned long long &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long inc = cp_wave_incl(v, lane);
    __syncthreads();                                         // sh may still be read from an earlier call
    if (lane == 63u) sh[w] = inc;
    __syncthreads();
    unsigned long long pre = 0ull, tot = 0ull;
    for (uint32_t i = 0; i < (uint32_t)NW; i++) { if (i < w) pre = cp_compose(pre, sh[i]); tot = cp_compose(tot, sh[i]); }
    total = tot;
    const unsigned long long up = __shfl_up(inc, 1, 64);
    return lane == 0u ? pre : cp_compose(pre, up);
}

// One piece walked byte by byte from its exact start state, as SeqWalker::step walks it (byte i <-> bit i).
struct CoordPiece {
    unsigned long long wend;      // a valid window of a live record ends at this byte (the kmer_acc rule)
    unsigned long long posm;      // the byte holds a position: a sequence character, or a blank that turned out interior
    unsigned long long hdrm;      // the byte opens a record
    unsigned long long carried;   // pending blanks carried into the piece that turned out interior in it
    __device__ __forceinline__ unsigned long long pair() const {
        if (!hdrm) return carried + (unsigned long long)__popcll(posm);
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(hdrm);
        return CP_HDR | (unsigned long long)__popcll(posm & ~((2ull << last) - 1ull));
    }
};

__device__ __forceinline__ CoordPiece coords_walk(const uint8_t *mine, uint32_t nb, uint32_t ls_in, const L2 &st, uint32_t k) {
    CoordPiece cp; cp.wend = 0; cp.posm = 0; cp.hdrm = 0; cp.carried = 0;
    uint32_t ls = ls_in, run = l2_len(st);
    bool live = st.rec != 0u;                                // text before the first header is dropped
    unsigned long long pend_in = st.p_tail, pendm = 0;       // pending blanks: carried in / of this piece
    for_each_byte_of(mine, nb, [&](uint32_t i, uint32_t c, bool act) {
        const bool term = is_term(c), ws = is_ws(c), gt = c == '>';
        const bool at_start = ls == LS_START, in_seq = ls == LS_SEQ;
        const bool hdr_start = act && at_start && !ws && gt;
        const bool seqchar = act && !ws && (in_seq || (at_start && !gt));
        const bool t = act && term;
        const unsigned long long bit = 1ull << i;
        if (hdr_start) { live = true; run = 0u; cp.hdrm |= bit; }
        if (seqchar && (pend_in | pendm)) {                  // blanks were interior: each holds a position and maps to None
            cp.posm |= pendm; cp.carried += pend_in; run = 0u; pend_in = 0ull; pendm = 0ull;
        }
        if (t) { pend_in = 0ull; pendm = 0ull; }
        else if (act && ws && in_seq) pendm |= bit;
        ls = t ? (uint32_t)LS_START : hdr_start ? (uint32_t)LS_HEADER : seqchar ? (uint32_t)LS_SEQ : ls;
        cp.posm |= seqchar ? bit : 0ull;
        const bool valid = seqchar && base_code(c) < 4u;
        run = valid ? (run < k ? run + 1u : run) : (seqchar ? 0u : run);
        cp.wend |= (valid && run == k && live) ? bit : 0ull;
    });
    return cp;
}

constexpr uint32_t MASK_HARD = 1u, MASK_INVERT = 2u;       // the mode bits of a mask (pk_query_set_mask)

// The cover bits of a piece's valid bases on the bytes that hold them: popcount(valid) bits from bit g0 of the bitmap
// (n_words u32; words past its end read as zero), with `invert` their complement, deposited onto the set bits of `valid`,
// lowest first, a run of set bits at a time (plain sequence text: one or two).  valid != 0.
__device__ __forceinline__ unsigned long long cover_select(unsigned long long valid, unsigned long long g0, const uint32_t *__restrict__ bits,
                                                           unsigned long long n_words, bool invert) {
    const unsigned long long w0 = g0 >> 5;
    const uint32_t sh = (uint32_t)(g0 & 31ull);
    const auto word = [&](unsigned long long w) -> unsigned long long { return w < n_words ? (unsigned long long)bits[w] : 0ull; };
    unsigned long long got = (word(w0) | (word(w0 + 1ull) << 32)) >> sh;
    if (sh) got |= word(w0 + 2ull) << (64u - sh);
    if (invert) got = ~got;
    unsigned long long sel = 0ull, rest = valid;
    while (rest) {
        const uint32_t at = (uint32_t)__builtin_ctzll(rest);
        const unsigned long long from = ~(rest >> at);       // the run begins at bit 0 and ends below the first set bit
        const uint32_t len = from ? (uint32_t)__builtin_ctzll(from) : 64u;
        const unsigned long long run = len >= 64u ? ~0ull : ((1ull << len) - 1ull);
        sel |= (got & run) << at;
        got = len >= 64u ? 0ull : got >> len;
        rest &= ~(run << at);
    }
    return sel;
}

}  // namespace pk
