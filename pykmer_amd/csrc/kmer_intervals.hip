// kmer_intervals.hip -- the selected bases of a mask feed as intervals (record, start, end) in position coordinates
// (pk_query_set_intervals, DESIGN.md 4.14 "Intervals").
//
// An interval is a maximal run of consecutive positions of one record that all hold selected bases; positions are those of
// kmer_coords.hip.  The EVENT bytes of the text are the bytes that hold a position and the bytes that open a record; one bit
// of state, OPEN, says that the last event of the stream was a selected base.  A START is a selected byte met while not
// open; an END is an event that is not selected (an invalid character, an interior blank, a valid base that is not
// selected, a header) met while open, and its value is the running position at that byte -- for a header that of the
// record it closes.  Pending blanks carried into a piece that resolve in it (CoordPiece::carried) are one more event, not
// selected, in front of the piece's first byte; its value is the position before them.  Both lists are in stream order, the
// j-th start pairs with the j-th end, and starts - ends = open at every point of the stream, so the two running counts
// carry the open bit from feed to feed.
//
// What a stretch of text does to OPEN is: nothing (no event), or set it to what its last event says; that composes as
// "the later one, unless it is nothing".  What it adds to the two counts depends on the state it is entered with only
// through its first event, so a chunk is summed as if entered closed, with the kind of its first event beside the sums.
//   k_iv_count   one workgroup per chunk, text geometry of k_mask_apply: the selected bytes as k_mask_apply derives them,
//                the events as k_coords_write derives them; the chunk's starts, ends, first event and what it does to OPEN
//   k_iv_scan    one workgroup over the chunks, a tile at a time: OPEN at every chunk's first byte from the counts at the
//                end of the feed before (ns_in - ne_in), the sums corrected for it, and the rows of the chunk's first start
//                and first end; leaves the counts behind the feed in ns_out / ne_out.  The host makes them the next feed's
//                only once the feed has settled
//   k_iv_write   one workgroup per chunk that holds a start or an end: iv_record / iv_start at the row of each start,
//                iv_end at the row of each end.  One writer per address, plain stores; rows at or past `cap` are not written
// Behind k_cover_scan (base_first) and k_coords_sum / k_coords_scan (chunk_pos) of the same feed.  All return at once,
// writing nothing, when flags[0] is raised.
#include "kmer_pieces.h"
#include "wg_scan.h"

namespace pk {

// what a stretch of text does to OPEN: 0 nothing, 2 | v: sets it to v
struct OpenCompose { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return b ? b : a; } };   // a first, then b
struct OpenShflUp { __device__ __forceinline__ uint32_t operator()(uint32_t v, int d) const { return __shfl_up(v, d, 64); } };

// a chunk's summary in one word, as if the chunk were entered closed
constexpr uint32_t IV_ENDS_SHIFT = 16, IV_KIND_SHIFT = 32, IV_OPEN_SHIFT = 34;
constexpr unsigned long long IV_FIRST_SELECTED = 1ull, IV_FIRST_OTHER = 2ull;   // the kind of the first event; 0: no event
// ... and behind the scan: the row of its first start, OPEN at its first byte, and whether it holds a start or an end
constexpr unsigned long long IV_ENTERED_OPEN = 1ull << 63, IV_ANY = 1ull << 62;

// The events of the lane's piece and which of them are selected.  text: the staged chunk.  Clean pieces (plain sequence
// text) by masks, as in k_mask_apply and k_coords_write; the others by the rolled byte loop in the waves that hold one.
struct IvPiece {
    CoordPiece cp;                // posm, hdrm, carried (wend is not used)
    unsigned long long sel;       // the selected bytes, all of them in posm
    __device__ __forceinline__ unsigned long long events() const { return cp.posm | cp.hdrm; }
    // what the piece does to OPEN
    __device__ __forceinline__ uint32_t open_change() const {
        const unsigned long long e = events();
        return e ? 2u | (uint32_t)((sel >> (63u - (uint32_t)__builtin_clzll(e))) & 1ull) : 0u;
    }
};

// chunk_first: the stream ordinal of the chunk's first valid base; those in front of the lane are counted here (sh32: first use)
__device__ __forceinline__ IvPiece iv_piece(const uint8_t *text, uint32_t nb, const LaneStart &ln, uint32_t k, unsigned long long chunk_first,
                                            const uint32_t *__restrict__ bits, unsigned long long n_words, uint32_t mode, uint32_t *sh32) {
    const uint8_t *mine = text + threadIdx.x * LDS_STRIDE;
    const L2 &st = ln.st;
    PieceMasks pm;
    uint32_t cw[4];
    piece_scan(mine, nb, pm, cw);
    IvPiece p;
    p.cp.wend = 0ull;
    p.cp.posm = ~pm.term; p.cp.hdrm = 0ull;
    p.cp.carried = (st.p_tail && (p.cp.posm & 1ull)) ? st.p_tail : 0ull;
    if (__any(!ln.clean)) {
        const CoordPiece walked = coords_walk(mine, nb, ln.ls_in, st, k);
        if (!ln.clean) p.cp = walked;
    }
    // the valid bases of live records: letters that are sequence characters, behind the first header of the stream
    const unsigned long long live = st.rec != 0u ? ~0ull : p.cp.hdrm ? ~((p.cp.hdrm & (0ull - p.cp.hdrm)) - 1ull) : 0ull;
    const unsigned long long valid = pm.valid & p.cp.posm & live;
    const uint32_t nv = (uint32_t)__popcll(valid);
    uint32_t total;
    const uint32_t off = wg_excl_sum<WG / 64, false>(nv, sh32, total);
    p.sel = nv ? cover_select(valid, chunk_first + off, bits, n_words, (mode & MASK_INVERT) != 0u) : 0ull;
    return p;
}

// The starts and ends among the piece's bytes, entered with `open`: adding the selected bytes to (no event | selected) lets
// a carry run from every selected byte through the bytes without an event and through further selected ones, up to the
// next event that is not selected.  That event is an end; a selected byte that no carry reaches is a start.  Resolving
// carried blanks close the run in front of byte 0 (carried_end), and the bytes are then entered closed.
struct IvEdges { unsigned long long starts, ends; bool carried_end; };
__device__ __forceinline__ IvEdges iv_edges(const IvPiece &p, bool open) {
    IvEdges e;
    e.carried_end = open && p.cp.carried != 0ull;
    const unsigned long long ev = p.events();
    const unsigned long long r = (~ev | p.sel) + p.sel + ((open && p.cp.carried == 0ull) ? 1ull : 0ull);
    e.ends = r & ev & ~p.sel;
    e.starts = p.sel & ~r;
    return e;
}

__global__ __launch_bounds__(WG) void k_iv_count(const uint8_t *__restrict__ fasta, uint64_t n_bytes, const LaneState *__restrict__ lane_state,
                                                 const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                 const unsigned long long *__restrict__ base_first, const uint32_t *__restrict__ bits,
                                                 unsigned long long n_words, uint32_t mode, unsigned long long *__restrict__ chunk_iv,
                                                 const uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint8_t text[WG * LDS_STRIDE];
    __shared__ uint32_t sh32[WG / 64], sh_open[WG / 64], sh_sum[WG / 64];
    __shared__ uint32_t first_kind;
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const uint64_t base = (uint64_t)c * CHUNK;
    const LaneStart ln = lane_start(lane_state[(uint64_t)c * WG + threadIdx.x], chunk_l2_state[c], k - 1u);
    if (threadIdx.x == 0) first_kind = 0u;
    stage_chunk(fasta, base, n_bytes, text);
    __syncthreads();
    const IvPiece p = iv_piece(text, piece_len(base, n_bytes), ln, k, base_first[c], bits, n_words, mode, sh32);
    uint32_t change;
    const uint32_t before = wg_excl_scan<WG / 64, false>(p.open_change(), 0u, sh_open, change, OpenCompose(), OpenShflUp());
    const IvEdges e = iv_edges(p, (before & 1u) != 0u);     // no event before: entered closed
    const unsigned long long ev = p.events();
    if (before == 0u && ev)                                  // the chunk's first event: one lane
        first_kind = (p.cp.carried == 0ull && ((ev & (0ull - ev)) & p.sel)) ? (uint32_t)IV_FIRST_SELECTED : (uint32_t)IV_FIRST_OTHER;
    uint32_t sums;
    wg_excl_sum<WG / 64, false>((uint32_t)__popcll(e.starts) | (((uint32_t)__popcll(e.ends) + (e.carried_end ? 1u : 0u)) << IV_ENDS_SHIFT), sh_sum, sums);
    // (the barrier of the sum lies behind the store of first_kind)
    if (threadIdx.x == 0)
        chunk_iv[2ull * c] = (unsigned long long)sums | ((unsigned long long)first_kind << IV_KIND_SHIFT) | ((unsigned long long)change << IV_OPEN_SHIFT);
}

// One workgroup, in place: chunk_iv[2c] = the chunk's summary  ->  the row of its first start with IV_ENTERED_OPEN and IV_ANY,
// chunk_iv[2c + 1] = the row of its first end.
constexpr int IVNT = 1024;
__global__ __launch_bounds__(IVNT) void k_iv_scan(unsigned long long *__restrict__ chunk_iv, uint32_t n_chunks,
                                                  const unsigned long long *__restrict__ ns_in, const unsigned long long *__restrict__ ne_in,
                                                  unsigned long long *__restrict__ ns_out, unsigned long long *__restrict__ ne_out,
                                                  const uint32_t *__restrict__ flags) {
    __shared__ uint32_t sh_open[IVNT / 64];
    __shared__ unsigned long long sh_sum[IVNT / 64];
    if (flags[0]) return;
    unsigned long long ns = *ns_in, ne = *ne_in;
    uint32_t open = 2u | (uint32_t)((ns - ne) & 1ull);       // starts - ends is the open bit
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += IVNT) {
        const uint32_t c = c0 + threadIdx.x;
        const unsigned long long w = c < n_chunks ? chunk_iv[2ull * c] : 0ull;
        uint32_t open_behind;
        const uint32_t entered = wg_excl_scan<IVNT / 64, true>((uint32_t)(w >> IV_OPEN_SHIFT) & 3u, open, sh_open, open_behind, OpenCompose(), OpenShflUp()) & 1u;
        const unsigned long long kind = (w >> IV_KIND_SHIFT) & 3ull;
        unsigned long long s = w & 0xffffull, e = (w >> IV_ENDS_SHIFT) & 0xffffull;
        if (entered && kind == IV_FIRST_SELECTED) s--;       // the run goes on: its first selected byte starts nothing
        if (entered && kind == IV_FIRST_OTHER) e++;          // the run ends at the chunk's first event
        unsigned long long tot;
        const unsigned long long ex = wg_excl_sum<IVNT / 64, true>(s | (e << 32), sh_sum, tot);   // a tile holds < 2^32 of either
        if (c < n_chunks) {
            chunk_iv[2ull * c] = (ns + (ex & 0xffffffffull)) | (entered ? IV_ENTERED_OPEN : 0ull) | ((s | e) ? IV_ANY : 0ull);
            chunk_iv[2ull * c + 1ull] = ne + (ex >> 32);
        }
        ns += tot & 0xffffffffull;
        ne += tot >> 32;
        open = open_behind;
    }
    if (threadIdx.x == 0) { *ns_out = ns; *ne_out = ne; }
}

__global__ __launch_bounds__(WG) void k_iv_write(const uint8_t *__restrict__ fasta, uint64_t n_bytes, const LaneState *__restrict__ lane_state,
                                                 const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                 const unsigned long long *__restrict__ base_first, const uint32_t *__restrict__ bits,
                                                 unsigned long long n_words, uint32_t mode, const unsigned long long *__restrict__ chunk_pos,
                                                 const unsigned long long *__restrict__ chunk_iv, unsigned long long *__restrict__ iv_record,
                                                 unsigned long long *__restrict__ iv_start, unsigned long long *__restrict__ iv_end,
                                                 unsigned long long cap, const uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint8_t text[WG * LDS_STRIDE];
    __shared__ uint32_t sh32[WG / 64], sh_open[WG / 64], sh_sum[WG / 64];
    __shared__ unsigned long long sh_pos[WG / 64];
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const unsigned long long w0 = chunk_iv[2ull * c];
    if (!(w0 & IV_ANY)) return;                              // uniform: the chunk holds no start and no end
    const uint64_t base = (uint64_t)c * CHUNK;
    const LaneStart ln = lane_start(lane_state[(uint64_t)c * WG + threadIdx.x], chunk_l2_state[c], k - 1u);
    stage_chunk(fasta, base, n_bytes, text);
    __syncthreads();
    const IvPiece p = iv_piece(text, piece_len(base, n_bytes), ln, k, base_first[c], bits, n_words, mode, sh32);
    uint32_t unused32;
    const uint32_t before = wg_excl_scan<WG / 64, false>(p.open_change(), (w0 & IV_ENTERED_OPEN) ? 3u : 2u, sh_open, unused32, OpenCompose(), OpenShflUp());
    const IvEdges e = iv_edges(p, (before & 1u) != 0u);
    uint32_t sums;
    const uint32_t off = wg_excl_sum<WG / 64, false>((uint32_t)__popcll(e.starts) | (((uint32_t)__popcll(e.ends) + (e.carried_end ? 1u : 0u)) << IV_ENDS_SHIFT),
                                                     sh_sum, sums);
    unsigned long long unused;
    const unsigned long long ex = cp_block_excl<WG / 64>(p.cp.pair(), sh_pos, unused);
    if (!(e.starts | e.ends) && !e.carried_end) return;
    // positions counted in the record open at the piece's first byte, before that byte (pending blanks not among them)
    const unsigned long long pos0 = cp_compose(chunk_pos[c], ex) & ~CP_HDR;
    // the positions of its record in front of byte i (those of carried blanks that resolve in the piece among them)
    const auto pos_of = [&](uint32_t i) -> unsigned long long {
        const unsigned long long below = (1ull << i) - 1ull, h = p.cp.hdrm & below;
        if (!h) return pos0 + p.cp.carried + (unsigned long long)__popcll(p.cp.posm & below);
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(h);
        return (unsigned long long)__popcll(p.cp.posm & below & ~((2ull << last) - 1ull));
    };
    unsigned long long row = (w0 & ~(IV_ENTERED_OPEN | IV_ANY)) + (off & 0xffffu);
    for (unsigned long long m = e.starts; m; m &= m - 1ull, row++) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        if (row >= cap) break;
        // a selected base lies in a record: the walker's number is 1-based
        iv_record[row] = (unsigned long long)ln.st.rec + (unsigned long long)__popcll(p.cp.hdrm & ((1ull << i) - 1ull)) - 1ull;
        iv_start[row] = pos_of(i);
    }
    row = chunk_iv[2ull * c + 1ull] + (off >> IV_ENDS_SHIFT);
    if (e.carried_end) {
        if (row < cap) iv_end[row] = pos0;
        row++;
    }
    for (unsigned long long m = e.ends; m; m &= m - 1ull, row++) {
        if (row >= cap) break;
        iv_end[row] = pos_of((uint32_t)__builtin_ctzll(m));
    }
}

// ------------------------------------------------------------------ host side -------------------
void launch_iv_count(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state, const L2 *st2,
                     const unsigned long long *base_first, const uint32_t *bits, uint64_t n_words, uint32_t mode, unsigned long long *chunk_iv,
                     const unsigned long long *ns_in, const unsigned long long *ne_in, unsigned long long *ns_out, unsigned long long *ne_out,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_iv_count, dim3(pl.n_chunks), dim3(WG), 0, s, fasta, n, lane_state, st2, pl.k, base_first, bits, (unsigned long long)n_words, mode,
                       chunk_iv, (const uint32_t *)b.flags);
    hipLaunchKernelGGL(k_iv_scan, dim3(1), dim3(IVNT), 0, s, chunk_iv, pl.n_chunks, ns_in, ne_in, ns_out, ne_out, (const uint32_t *)b.flags);
}

void launch_iv_write(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state, const L2 *st2,
                     const unsigned long long *base_first, const uint32_t *bits, uint64_t n_words, uint32_t mode, const unsigned long long *chunk_pos,
                     const unsigned long long *chunk_iv, unsigned long long *iv_record, unsigned long long *iv_start, unsigned long long *iv_end,
                     uint64_t cap, hipStream_t s) {
    hipLaunchKernelGGL(k_iv_write, dim3(pl.n_chunks), dim3(WG), 0, s, fasta, n, lane_state, st2, pl.k, base_first, bits, (unsigned long long)n_words, mode,
                       chunk_pos, chunk_iv, iv_record, iv_start, iv_end, (unsigned long long)cap, (const uint32_t *)b.flags);
}

}  // namespace pk
