// kmer_coords.hip -- base coordinates of the rows of a binned query (pk_query_set_coords, DESIGN.md 4.10 "Coordinates").
//
// The packed stream the lookups read carries no positions, so the text of the feed is walked once more, from the exact
// parser state the structure pass left for every 64-byte piece (lane_state behind chunk_l2_state, as k_squeeze takes it).
// Positions are counted as DevRec.seq_len counts them (SeqWalker::step, kmer_walk.h): within a record every sequence
// character gets the next position, valid base or not; blanks inside a sequence line get theirs once a sequence character
// follows them on the same line; terminators, stripped blanks and header text get none.  A valid window is k consecutive
// positions: the one whose last base has position e begins at e - k + 1.  For the window of ordinal o (kmer_query.hip) in
// record r, with j = o - P[r] and row = Bf[r] + j / W:
//     j % W == 0                             bin_start[row] = e - k + 1
//     (j + 1) % W == 0 or j + 1 == n_valid   bin_end[row]   = e + 1      (n_valid as this feed's squeeze left it)
// The second rule gives a record still open at the end of the feed a provisional end; a later feed that adds windows to
// that row overwrites it, in stream order.  Every address is written by one lane per feed: plain stores, no atomics, and
// the arrays are not zeroed between feeds.
//
// What a stretch of text does to the position is the pair (opens a record, positions since the last header or since the
// stretch began); because the state a piece is entered with is exact the pair is concrete (it includes the pending blanks
// carried in that turn out interior in the piece), and pairs compose associatively: b.hdr ? b : (a.hdr, a.cnt + b.cnt).
//   k_coords_sum    one workgroup per chunk: the chunk's pair.  Clean pieces (plain sequence text) take their count from
//                   the structure pass's PiecePack; the text is read only for chunks that hold other pieces
//   k_coords_scan   one workgroup: the position at every chunk's first byte, from the position at the end of the feed
//                   before (pos[in]); leaves the position at the end of this feed in pos[out].  The host makes `out` the
//                   next feed's `in` only once the feed has settled, so that a repeated feed (flags[0] = 2) starts from
//                   the same position.
//   k_coords_write  one workgroup per chunk: positions, runs and records of its pieces again, the windows that end in each
//                   piece prefix-summed behind slot_first[c] (their ordinals), and the two rules above.  Clean pieces by
//                   masks (piece_scan and the pack's restart bits), the others by the rolled byte loop
// Like the kernels of kmer_query.hip all three return at once, writing nothing, when flags[0] is raised.  The pair, its
// scans and the byte-wise walk (coords_walk) are in kmer_pieces.h, which kmer_intervals.hip shares.
#include "kmer_pieces.h"
#include "kmer_window.h"
#include "wg_scan.h"

namespace pk {

__global__ __launch_bounds__(WG) void k_coords_sum(const uint8_t *__restrict__ fasta, uint64_t n_bytes, const LaneState *__restrict__ lane_state,
                                                   const PiecePack *__restrict__ packs, const L2 *__restrict__ chunk_l2_state,
                                                   const uint32_t *__restrict__ chunk_odd, uint32_t k, unsigned long long *__restrict__ chunk_pos,
                                                   const uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint8_t text[WG * LDS_STRIDE];
    __shared__ unsigned long long sh[WG / 64];
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const uint64_t base = (uint64_t)c * CHUNK;
    const LaneStart ln = lane_start(lane_state[(uint64_t)c * WG + threadIdx.x], chunk_l2_state[c], k - 1u);
    const L2 &st = ln.st;
    const uint32_t ls_in = ln.ls_in;
    const bool clean = ln.clean;
    const uint32_t nb = piece_len(base, n_bytes);
    // a clean piece (plain sequence text): the structure pass counted its sequence characters; blanks pending from the
    // piece before are interior if a sequence character comes first (squeeze_apply).  Only a chunk that holds other
    // pieces (uniform) is read, and only the waves that hold one walk (the walk costs a wave the same for one lane as for 64)
    const uint32_t meta = packs[(uint64_t)c * WG + threadIdx.x].meta;
    unsigned long long mine = nb ? ((meta >> 8) & 0xffu) + ((st.p_tail && ((meta >> 16) & 1u)) ? st.p_tail : 0ull) : 0ull;
    if (chunk_odd[c] != 0u) {
        stage_chunk(fasta, base, n_bytes, text);
        __syncthreads();
        if (__any(!clean)) {
            const unsigned long long walked = coords_walk(text + threadIdx.x * LDS_STRIDE, nb, ls_in, st, k).pair();
            if (!clean) mine = walked;
        }
    }
    unsigned long long total;
    cp_block_excl<WG / 64>(mine, sh, total);
    if (threadIdx.x == 0) chunk_pos[c] = total;
}

// One workgroup, in place: chunk_pos[c] = the chunk's pair  ->  the position at the chunk's first byte.
constexpr int CSNT = 1024;
__global__ __launch_bounds__(CSNT) void k_coords_scan(unsigned long long *__restrict__ chunk_pos, uint32_t n_chunks,
                                                      const unsigned long long *__restrict__ pos_in, unsigned long long *__restrict__ pos_out,
                                                      const uint32_t *__restrict__ flags) {
    __shared__ unsigned long long sh[CSNT / 64];
    if (flags[0]) return;
    unsigned long long run = *pos_in & ~CP_HDR;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += CSNT) {
        const uint32_t c = c0 + threadIdx.x;
        const unsigned long long v = c < n_chunks ? chunk_pos[c] : 0ull;
        unsigned long long total;
        const unsigned long long ex = cp_block_excl<CSNT / 64>(v, sh, total);
        if (c < n_chunks) chunk_pos[c] = cp_compose(run, ex) & ~CP_HDR;
        run = cp_compose(run, total) & ~CP_HDR;
    }
    if (threadIdx.x == 0) *pos_out = run;
}

// the byte of the n-th set bit of x, n counted from 0 (n < popcount(x))
__device__ __forceinline__ uint32_t nth_set(unsigned long long x, uint32_t n) {
    uint32_t at = 0;
#pragma unroll
    for (uint32_t w = 32u; w; w >>= 1) {
        const uint32_t below = (uint32_t)__popcll(x & ((1ull << w) - 1ull));
        if (n >= below) { n -= below; x >>= w; at += w; }
    }
    return at;
}

__global__ __launch_bounds__(WG) void k_coords_write(const uint8_t *__restrict__ fasta, uint64_t n_bytes, const LaneState *__restrict__ lane_state,
                                                     const PiecePack *__restrict__ packs, const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                     const unsigned long long *__restrict__ chunk_pos,
                                                     const unsigned long long *__restrict__ slot_first, const unsigned long long *__restrict__ P,
                                                     const unsigned long long *__restrict__ Bf, unsigned long long W,
                                                     const DevRec *__restrict__ recs, unsigned long long *__restrict__ bin_start,
                                                     unsigned long long *__restrict__ bin_end, unsigned long long rows_cap,
                                                     const uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint8_t text[WG * LDS_STRIDE];
    __shared__ unsigned long long sh[WG / 64];
    __shared__ uint32_t sh32[WG / 64];
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const uint64_t base = (uint64_t)c * CHUNK;
    const LaneStart ln = lane_start(lane_state[(uint64_t)c * WG + threadIdx.x], chunk_l2_state[c], k - 1u);
    const L2 &st = ln.st;
    const uint32_t ls_in = ln.ls_in;
    const bool clean = ln.clean;
    unsigned long long restart = packs[(uint64_t)c * WG + threadIdx.x].restart;   // a copy: window_ends completes base 0's bit in place
    stage_chunk(fasta, base, n_bytes, text);
    __syncthreads();
    const uint8_t *mine = text + threadIdx.x * LDS_STRIDE;
    const uint32_t nb = piece_len(base, n_bytes);
    // A clean piece (plain sequence text, the usual one) by masks: every byte that is no terminator holds a position, no
    // record opens, blanks carried in resolve at byte 0 or not at all, and the windows follow from the pack's restart bits
    // as in squeeze_apply -- over the piece's valid bases pushed together, so cp.wend counts BASES there (valid: which bytes
    // they are).  The other pieces byte by byte, in the waves that hold one.
    PieceMasks pm;
    uint32_t cw[4];
    piece_scan(mine, nb, pm, cw);
    const unsigned long long valid = pm.valid;
    CoordPiece cp;
    cp.posm = ~pm.term; cp.hdrm = 0ull;
    cp.carried = (st.p_tail && (cp.posm & 1ull)) ? st.p_tail : 0ull;
    cp.wend = st.rec != 0u ? window_ends(restart, (uint32_t)__popcll(valid), cp.carried ? 0u : l2_len(st), k - 1u) : 0ull;
    if (__any(!clean)) {
        const CoordPiece walked = coords_walk(mine, nb, ls_in, st, k);
        if (!clean) cp = walked;
    }
    // the byte of the n-th window of the mask w of this piece
    const auto byte_of = [&](unsigned long long w, uint32_t n) -> uint32_t {
        const uint32_t at = nth_set(w, n);
        return clean ? nth_set(valid, at) : at;
    };
    uint32_t n_win;
    const uint32_t off = wg_excl_sum<WG / 64, false>((uint32_t)__popcll(cp.wend), sh32, n_win);   // sh32: first use
    if (n_win == 0u) return;                                 // uniform: no window ends in the chunk
    unsigned long long unused;
    const unsigned long long ex = cp_block_excl<WG / 64>(cp.pair(), sh, unused);
    if (!cp.wend) return;
    // positions counted in the record open at the piece's first byte, before that byte (pending blanks not among them)
    const unsigned long long pos0 = cp_compose(chunk_pos[c], ex) & ~CP_HDR;
    // the position of the sequence character at byte i
    const auto pos_of = [&](uint32_t i) -> unsigned long long {
        const unsigned long long below = (1ull << i) - 1ull, h = cp.hdrm & below;
        if (!h) return pos0 + cp.carried + (unsigned long long)__popcll(cp.posm & below);   // carried blanks resolve at the piece's first sequence character
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(h);
        return (unsigned long long)__popcll(cp.posm & below & ~((2ull << last) - 1ull));
    };
    // record by record (a header ends the one before): the windows of ordinals [o, o + nw) end at the bytes `w`
    unsigned long long o = slot_first[c] + off, left = cp.wend, hdrs = cp.hdrm;
    unsigned long long rec = st.rec;                         // 1-based
    for (;;) {
        const unsigned long long seg = hdrs ? ((hdrs & (0ull - hdrs)) - 1ull) : ~0ull;   // the bytes below the next header
        const unsigned long long w = left & seg;
        const uint32_t nw = (uint32_t)__popcll(w);
        if (nw) {                                            // rec >= 1: a window lies in a record
            const unsigned long long r = rec - 1ull, j0 = o - P[r], row0 = Bf[r], m = recs[r].n_valid;
            const unsigned long long q = j0 / W, rem = j0 - q * W;
            // windows that begin a bin: j % W == 0
            {
                const unsigned long long d = rem ? W - rem : 0ull;
                unsigned long long row = row0 + q + (rem ? 1ull : 0ull);
                for (unsigned long long idx = d; idx < nw; row++) {
                    if (row < rows_cap) bin_start[row] = pos_of(byte_of(w, (uint32_t)idx)) + 1ull - k;
                    if (W >= nw - idx) break;
                    idx += W;
                }
            }
            // windows that end a bin: (j + 1) % W == 0, and the record's last window so far
            {
                unsigned long long row = row0 + q;
                for (unsigned long long idx = W - 1ull - rem; idx < nw; row++) {
                    if (row < rows_cap) bin_end[row] = pos_of(byte_of(w, (uint32_t)idx)) + 1ull;
                    if (W >= nw - idx) break;
                    idx += W;
                }
                if (m > j0 && m - j0 <= nw) {
                    const unsigned long long last_row = row0 + (m - 1ull) / W;
                    if (last_row < rows_cap) bin_end[last_row] = pos_of(byte_of(w, (uint32_t)(m - j0 - 1ull))) + 1ull;
                }
            }
        }
        if (!hdrs) break;
        o += nw;
        left &= ~seg;
        hdrs &= hdrs - 1ull;
        rec++;
    }
}

// ------------------------------------------------------------------ host side -------------------
void launch_coords_positions(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state,
                             const PiecePack *packs, const L2 *st2, const uint32_t *chunk_odd, unsigned long long *chunk_pos,
                             const unsigned long long *pos_in, unsigned long long *pos_out, hipStream_t s) {
    hipLaunchKernelGGL(k_coords_sum, dim3(pl.n_chunks), dim3(WG), 0, s, fasta, n, lane_state, packs, st2, chunk_odd, pl.k, chunk_pos,
                       (const uint32_t *)b.flags);
    hipLaunchKernelGGL(k_coords_scan, dim3(1), dim3(CSNT), 0, s, chunk_pos, pl.n_chunks, pos_in, pos_out, (const uint32_t *)b.flags);
}

void launch_query_coords(const PartPlan &pl, const PartBuffers &b, const QueryBuffers &qb, const uint8_t *fasta, uint64_t n, const LaneState *lane_state,
                         const PiecePack *packs, const L2 *st2, const uint32_t *chunk_odd, const DevRec *recs, const unsigned long long *P,
                         const unsigned long long *Bf, uint64_t bin_windows, unsigned long long *chunk_pos, const unsigned long long *pos_in,
                         unsigned long long *pos_out, unsigned long long *bin_start, unsigned long long *bin_end, uint64_t rows_cap, hipStream_t s) {
    launch_coords_positions(pl, b, fasta, n, lane_state, packs, st2, chunk_odd, chunk_pos, pos_in, pos_out, s);
    hipLaunchKernelGGL(k_coords_write, dim3(pl.n_chunks), dim3(WG), 0, s, fasta, n, lane_state, packs, st2, pl.k, (const unsigned long long *)chunk_pos,
                       (const unsigned long long *)qb.slot_first, P, Bf, (unsigned long long)bin_windows, recs, bin_start, bin_end,
                       (unsigned long long)rows_cap, (const uint32_t *)b.flags);
}

}  // namespace pk
