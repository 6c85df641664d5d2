// kmer_pack.hip -- the squeeze pass: FASTA text -> packed stream of valid bases.
//
// The reference turns every record into a tuple of codes (0-3, None) and slides a k-window over it
// (parse_fasta indexer.py:45-99, gen_kmers :130-160).  Here the text is read once more after the
// structure pass (kmer_count.hip) has given every 64-byte piece its exact parser state, and what is kept
// of it is just what the k-mer windows need:
//
//   codes    2 bits per VALID base of a record (A 0, C 1, G 2, T 3; CONV, indexer.py:36-41), 16 per dword
//            from bit 0 up, in text order.  Line terminators, headers, blanks and characters that map to
//            None are gone;
//   restart  1 bit per base: the run of valid bases starts anew here (first base of a record, or
//            something that maps to None lay between it and the base before: indexer.py:144 voids every
//            window that would span it).
//
// Each 16 KiB chunk of text owns a fixed slot (4 KiB of codes, 2 KiB of restart bits, a base count), so no
// stream-wide compaction is needed: the k-1 bases in front of a slot come from the chunk's start state.
// Per-record tallies (seq_len, number of valid windows, header extent: indexer.py:75-95,349-351) are
// taken here too, where the text is in hand.  0.38 bytes written per base instead of one 4-byte record;
// kmer_fuse.hip assembles the k-mers from the slots with no dependence between its threads.
#include "fasta_fsm.h"
#include "kmer_walk.h"
#include "kmer_window.h"
#include "lds_bits.h"
#include "pk_kernels.h"
#include "wg_scan.h"

namespace pk {

constexpr int SQUEEZE_WAVES = 4;   // waves per SIMD the squeeze kernel is compiled for (3, 5, 6 and 8 all give 0.31 ms instead of 0.21)

// ------------------------------------------------------------------ clean pieces ----
// A CLEAN piece holds nothing but sequence characters and line terminators and does not start inside a header line
// (the structure pass flags everything else): no record opens, nothing is stripped.  The structure pass has already
// classified its bytes and pushed its bases together (PiecePack, fasta_fsm.h); what is added here is what depends on
// the state the piece is entered with:
//   restart bit of base 0   the run was already broken when the piece began;
//   window count            positions with no restart among the k-1 before them (shift-or smear), minus those the
//                           incoming run is too short for (indexer.py:144);
//   tallies                 sequence characters (valid or not, indexer.py:77), pending blanks that turn out interior.
// `mine`: this lane's piece is a clean one; other lanes run along and leave no trace.
__device__ __forceinline__ void squeeze_apply(const PiecePack &pk, SeqWalker &wk, PieceBases &pb, bool mine) {
    const uint32_t nv = pack_n_valid(pk);
    if (mine) wk.seq_acc += pack_n_seq(pk);                               // indexer.py:77: valid or not
    // blanks pending from the piece before (that piece was not a clean one; this one is): interior if sequence text
    // follows -- each maps to None and the run breaks -- and stripped if the line ends here (indexer.py:56)
    if (mine && wk.pend) {
        if (pack_first_is_seq(pk)) { wk.seq_acc += wk.pend; wk.run = 0u; }
        wk.pend = 0;
    }
    const bool live = mine && wk.rec != 0;                                // text before the first header is dropped
    unsigned long long F = pk.restart;
    const unsigned long long has = window_ends(F, nv, wk.run, wk.k - 1u);
    wk.kmer_acc += live ? (uint64_t)__popcll(has) : 0ull;
    pb.code_lo = live ? pk.c_lo : 0ull; pb.code_hi = live ? pk.c_hi : 0ull;
    pb.restart = live ? F : 0ull;
    pb.n = live ? nv : 0u;
}

// ------------------------------------------------------------------ header pieces ----
// A HEADER PIECE (the structure pass's term, k_chunk_l2): a full piece that holds header text -- it opens records, or is
// entered inside a header line -- whose lines do not begin with a blank and that has no blank or control byte outside the
// header text.  Its header lines are found by masks (header_text, fasta_fsm.h): everything that is neither a terminator
// nor header text is a sequence character.  A read set has such a piece every kilobase; walking them byte by byte (64
// steps of ~100 instructions for the wave, whatever the number of lanes at work) was 86 % of this kernel's time there.
//
// Index one past the last byte of the header line `run` that str.strip() keeps (indexer.py:56,66), 0 if there is none:
// bytes from 0x21 up are kept; blanks and control bytes above the last of those are looked at one by one, from the top
// (a header rarely ends in one: zero rounds).
__device__ __forceinline__ uint32_t header_text_end(const uint8_t *text, unsigned long long run, unsigned long long blank) {
    const unsigned long long solid = run & ~blank;
    uint32_t end = solid ? 64u - (uint32_t)__builtin_clzll(solid) : 0u;
    unsigned long long todo = run & blank & (end >= 64u ? 0ull : ~0ull << end);
    while (todo) {
        const uint32_t p = 63u - (uint32_t)__builtin_clzll(todo);
        if (!is_ws(text[p])) { end = p + 1u; break; }
        todo ^= 1ull << p;
    }
    return end;
}

// All lanes of the wave; `mine`: this lane holds a header piece of a live record (wq.rec != 0) in `text`, with wq at the
// exact state of its first byte.  Leaves the piece's bases in rb and the tallies of the piece's LAST record in wq (the
// caller flushes them); the records that end inside the piece are flushed here.
__device__ __forceinline__ void squeeze_header_piece(const uint8_t *text, SeqWalker &wq, PieceBases &rb, bool mine) {
    PieceMasks pm;
    uint32_t cw[4];
    piece_scan(text, (uint32_t)PIECE, pm, cw);
    const uint32_t ls_in = wq.ls;
    const unsigned long long H = header_text(pm, ls_in), S = header_starts(pm, ls_in);
    const unsigned long long seq = ~pm.term & ~H, valid = pm.valid & seq;
    PiecePack hk;
    piece_compact(mine ? valid : 0ull, mine ? ((seq & ~valid) | H) : 0ull, cw, true, 0u, false, hk);     // loops as a wave
    if (!mine) return;
    // blanks pending from the piece before: interior if a sequence character comes first (indexer.py:56; step())
    if (wq.pend && ls_in == LS_SEQ && (seq & 1ull)) { wq.seq_acc += wq.pend; wq.run = 0u; }
    wq.pend = 0;
    unsigned long long F = hk.restart;
    const uint32_t nv = pack_n_valid(hk);
    const unsigned long long has = window_ends(F, nv, wq.run, wq.k - 1u);
    if (ls_in == LS_HEADER) {                                             // the line the piece is entered in goes on
        const uint32_t e = header_text_end(text, H & ~(H + 1ull), pm.blank);
        if (e) wq.name_end = wq.pos0 + e;
    }
    // one round per record opened: what lies below its '>' belongs to the record before
    unsigned long long below_prev = 0, cmp_prev = 0, todo = S;
    while (todo) {
        const uint32_t s = (uint32_t)__builtin_ctzll(todo);
        const unsigned long long bit = 1ull << s, below = bit - 1ull;
        const unsigned long long cmp_below = (1ull << (uint32_t)__popcll(valid & below)) - 1ull;     // <= 63 bases below a byte
        wq.seq_acc += (uint64_t)__popcll(seq & below & ~below_prev);
        wq.kmer_acc += (uint64_t)__popcll(has & cmp_below & ~cmp_prev);
        wq.flush_rec();
        wq.rec++;                                                         // indexer.py:66-82
        if (wq.rec <= wq.recs_cap) wq.recs[wq.rec - 1].name_off = wq.pos0 + s + 1u;
        wq.name_end = wq.pos0 + header_text_end(text, H & ~(H + bit), pm.blank);      // at least the '>' itself
        below_prev = below; cmp_prev = cmp_below;
        todo &= todo - 1ull;
    }
    wq.seq_acc += (uint64_t)__popcll(seq & ~below_prev);
    wq.kmer_acc += (uint64_t)__popcll(has & ~cmp_prev);
    rb.code_lo = hk.c_lo; rb.code_hi = hk.c_hi; rb.restart = F; rb.n = nv;
}

// ---- staging: the chunk's 16 KiB as a plain image in LDS (the lane's piece = 64 contiguous bytes; the 4-way bank
// conflict on its four 16-byte reads is noise here).  Full chunks arrive by LDS-DMA (global_load_lds: no registers,
// asynchronous -- the NEXT chunk's image is requested before the current one is squeezed and lands meanwhile); a chunk
// that reaches the end of the stream goes through registers so that bytes past the end are never read and arrive as 0.
__device__ __forceinline__ void stage_image_async(const uint8_t *__restrict__ fasta, uint64_t chunk_base, uint8_t *buf) {
    // the lane index is made opaque here: as loop invariants of the chunk loop the four lane addresses lived in registers,
    // were spilled, and each re-load from scratch waited for the DMA issued just before it (a memory round trip apiece)
    uint32_t lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int i = 0; i < CHUNK / (WG * 16); i++) {
        const uint32_t p = i * WG + lane;                                    // 16-byte piece of the chunk; one wave-instruction = 1 KiB
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(fasta + chunk_base + p * 16u),
                                         (__attribute__((address_space(3))) void *)(buf + (p & ~63u) * 16u), 16, 0, 0);
    }
}
__device__ __forceinline__ void stage_image_tail(const uint8_t *__restrict__ fasta, uint64_t chunk_base, uint64_t n_bytes, uint8_t *buf) {
#pragma unroll
    for (int i = 0; i < CHUNK / (WG * 16); i++) {
        const uint32_t p = i * WG + threadIdx.x;
        const uint64_t g = chunk_base + (uint64_t)p * 16u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g + 16u <= n_bytes) {
            v = *reinterpret_cast<const uint4 *>(fasta + g);
        } else if (g < n_bytes) {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < (uint32_t)(n_bytes - g); j++) w[j >> 2] |= (uint32_t)fasta[g + j] << (8u * (j & 3u));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(buf + p * 16u) = v;
    }
}
__device__ __forceinline__ void stage_image(const uint8_t *__restrict__ fasta, uint64_t chunk_base, uint64_t n_bytes, uint8_t *buf) {
    if (chunk_base + CHUNK <= n_bytes) stage_image_async(fasta, chunk_base, buf);     // uniform
    else stage_image_tail(fasta, chunk_base, n_bytes, buf);
}

template <uint32_t KC>                   // k as a literal (0: the argument)
__global__ __launch_bounds__(WG, SQUEEZE_WAVES) void k_squeeze(const uint8_t *__restrict__ fasta, uint64_t n_bytes, uint64_t stream_off,
                                                const LaneState *__restrict__ lane_state, const PiecePack *__restrict__ packs,
                                                const L2 *__restrict__ chunk_l2_state,
                                                const uint32_t *__restrict__ chunk_odd, const ChunkFix *__restrict__ chunk_fix, uint32_t k_arg,
                                                uint32_t n_chunks, uint32_t chunks_per_wg,
                                                uint32_t *__restrict__ codes,
                                                uint32_t *__restrict__ restarts, uint32_t *__restrict__ n_bases,
                                                DevRec *__restrict__ recs, uint64_t recs_cap, Carry *carry, uint32_t *__restrict__ flags) {
    // The record array was sized before this feed's records were counted (no host round trip between the structure pass and
    // this kernel).  The count is known here -- the structure pass's scan left it in `carry` -- so if the array is too
    // small every workgroup returns before touching anything, flags[0] = 2 keeps the later kernels of the feed away (each
    // of them returns at once on a raised flag and none overwrites it: the workspace still holds an earlier feed's text),
    // and the host grows the array and repeats from here.
    if (carry->n_recs > recs_cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) flags[0] = 2u;
        return;
    }
    __shared__ __attribute__((aligned(16))) uint8_t image[2][CHUNK];   // text of chunks that hold queued pieces (header pieces, pieces for the byte-wise machine)
    __shared__ __attribute__((aligned(16))) uint32_t slot_codes[SLOT_CODE_WORDS + 8];   // + slack: lds_or_bits touches up to 5 words
    __shared__ __attribute__((aligned(16))) uint32_t slot_rst[SLOT_RST_WORDS + 8];
    __shared__ uint32_t scan_sh[WG / 64];
    __shared__ uint16_t queue[WG];                         // pieces that need their text
    __shared__ uint32_t n_queued;
    __shared__ RecAcc racc;
    __shared__ uint32_t todo[SQUEEZE_G_MAX / 32];          // of the workgroup's chunks: the ones that are not settled
    const uint32_t k = KC ? KC : k_arg, km1 = k - 1;
    if (threadIdx.x == 0) n_queued = 0;
    for (uint32_t i = threadIdx.x; i < SLOT_CODE_WORDS + 8; i += WG) slot_codes[i] = 0;
    for (uint32_t i = threadIdx.x; i < SLOT_RST_WORDS + 8; i += WG) slot_rst[i] = 0;
    recacc_init(racc);
    SeqWalker wk;
    wk.setup(k, recs, recs_cap, &racc);
    const uint32_t c_lo = blockIdx.x * chunks_per_wg, c_hi = min(c_lo + chunks_per_wg, n_chunks);
    // Per chunk a lane needs its state (8 bytes) and its pack (32 bytes).  Both are requested one chunk AHEAD and taken
    // delivery of right before the current chunk's slot is stored (settle, as in the sort kernels: loads and stores
    // share one in-order counter, and a load waited for after the stores would also wait for the stores).  The text
    // itself is only fetched -- by LDS-DMA, also one chunk ahead -- for chunks with queued pieces.
    struct Fetched { uint32_t ls_flags, ls_rec_tail; uint4 p0, p1; };
    auto fetch = [&](uint32_t c, Fetched &f) {
        const LaneState l = lane_state[(uint64_t)c * WG + threadIdx.x];
        f.ls_flags = l.flags; f.ls_rec_tail = l.rec_tail;
        const uint4 *src = reinterpret_cast<const uint4 *>(packs + (uint64_t)c * WG + threadIdx.x);
        f.p0 = src[0]; f.p1 = src[1];
    };
    Fetched nxt;
    auto settle = [&]() {
        __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): also the next chunk's image, if one was requested
        asm volatile("" : "+v"(nxt.ls_flags), "+v"(nxt.ls_rec_tail), "+v"(nxt.p0.x), "+v"(nxt.p0.y), "+v"(nxt.p0.z), "+v"(nxt.p0.w),
                          "+v"(nxt.p1.x), "+v"(nxt.p1.y), "+v"(nxt.p1.z), "+v"(nxt.p1.w));
    };
    // the first chunk at or behind c that is not settled (c_hi: none).  Uniform.
    auto next_todo = [&](uint32_t c) -> uint32_t {
        for (uint32_t i = c - c_lo; i < SQUEEZE_G_MAX; i = (i | 31u) + 1u) {
            const uint32_t m = todo[i >> 5] & (~0u << (i & 31u));
            if (m) return min(c_lo + (i & ~31u) + (uint32_t)__builtin_ctz(m), c_hi);
        }
        return c_hi;
    };
    __syncthreads();                                       // racc is set up
    // ---- settled chunks (ChunkFix, fasta_fsm.h): the structure pass has placed their bases and counted their windows as if
    // they were entered in a live record behind a run of k-1 bases.  What is left depends on the state the chunk is really
    // entered with, and only the leading lanes see it: they go through lane_start + squeeze_apply like every clean piece, in
    // order, and give the base-0 restart bit, the windows the carried run is too short for and the pending blanks that turn
    // out interior.  What goes to the slots (a restart bit OR-ed in, a base count of 0) is the same however often this runs.
    // One thread per chunk (the plan gives a workgroup at most SQUEEZE_G_MAX); the chunks that are not settled are marked in
    // `todo` and take the loop below.
    static_assert(SQUEEZE_G_MAX <= WG && SQUEEZE_G_MAX % 32 == 0, "one thread per chunk of the workgroup");
    if (threadIdx.x < SQUEEZE_G_MAX / 32) todo[threadIdx.x] = 0u;
    if (threadIdx.x == 0 && c_lo < c_hi) racc.rec0 = chunk_l2_state[c_lo].rec;   // nothing is gathered yet: the record window starts where the chunks do
    __syncthreads();
    {
        const uint32_t c = c_lo + threadIdx.x;
        const bool have = c < c_hi;
        ChunkFix fx; fx.n_lead = 0u; fx.n_seq = 0u; fx.n_win = 0u; fx.pad_ = 0u;
        L2 chunk_st = l2_identity();
        LaneState lst; lst.flags = 0u; lst.rec_tail = 0u;
        uint4 p1 = make_uint4(0, 0, 0, 0);
        if (have) {
            if (chunk_fix) fx = chunk_fix[c];
            chunk_st = chunk_l2_state[c];
            lst = lane_state[(uint64_t)c * WG];            // lane 0 leads every settled chunk: asked for along with the record
            p1 = reinterpret_cast<const uint4 *>(packs + (uint64_t)c * WG)[1];
        }
        const bool is_settled = fx.n_lead != 0u;
        if (have && !is_settled) atomicOr(&todo[threadIdx.x >> 5], 1u << (threadIdx.x & 31u));
        wk.begin(LS_SEQ, chunk_st, 0ull);
        // lanes without a chunk go along in the record of the wave's first chunk, so that the wave's sums can be taken as one
        if (!have) wk.rec = (uint32_t)__builtin_amdgcn_readfirstlane((int)wk.rec);
        if (is_settled && chunk_st.rec == 0u) {            // text in front of the first header is dropped
            n_bases[c] = 0u;
        } else if (is_settled) {
            uint64_t seq = fx.n_seq, win = fx.n_win;               // less the leading lanes' share, which is added as it really is
            for (uint32_t j = 0; j < fx.n_lead; j++) {
                if (j) {
                    lst = lane_state[(uint64_t)c * WG + j];
                    p1 = reinterpret_cast<const uint4 *>(packs + (uint64_t)c * WG + j)[1];
                }
                PiecePack pk;
                pk.c_lo = 0ull; pk.c_hi = 0ull; pk.restart = ((unsigned long long)p1.y << 32) | p1.x; pk.meta = p1.z; pk.pad_ = 0u;
                const LaneStart ln = lane_start(lst, chunk_st, km1);
                unsigned long long assumed_F = pk.restart;
                const unsigned long long assumed = window_ends(assumed_F, pack_n_valid(pk), settled_run(lane_state_l2(lst), km1), km1);
                seq -= pack_n_seq(pk);
                win -= (uint64_t)__popcll(assumed);
                wk.ls = ln.ls_in; wk.pend = ln.st.p_tail; wk.run = l2_len(ln.st);
                PieceBases pb;
                squeeze_apply(pk, wk, pb, true);                 // adds the lane's exact tallies to wk's
                // base 0 of the lane restarts the run after all: it lies l2_len(prefix) bases into the slot
                if (pb.restart & ~assumed_F & 1ull) {
                    const uint32_t at = l2_len(lane_state_l2(lst));
                    atomicOr(&restarts[(uint64_t)c * SLOT_RST_WORDS + (at >> 5)], 1u << (at & 31u));
                }
            }
            wk.seq_acc += seq; wk.kmer_acc += win;
        }
        wk.flush_rec_wave();
    }
    __syncthreads();
    uint32_t c = next_todo(c_lo), c_next = c_hi;
    if (c < c_hi) {
        if (chunk_odd[c]) stage_image(fasta, (uint64_t)c * CHUNK, n_bytes, image[0]);
        fetch(c, nxt);
        c_next = next_todo(c + 1u);
    }
    settle();
    __syncthreads();
    for (uint32_t n_done = 0; c < c_hi; c = c_next, c_next = next_todo(min(c_next + 1u, c_hi)), n_done++) {
        const uint64_t base = (uint64_t)c * CHUNK;
        uint8_t *buf = image[n_done & 1u];
        const bool all_clean = chunk_odd[c] == 0u;         // uniform over the workgroup; the usual chunk
        if (!all_clean) __syncthreads();                   // every wave's share of the image has landed (each waited for its own in settle)
        // the record tallies of a chunk count up from the record it starts in; when that moves on, what was gathered
        // is written out (a genome keeps one window for thousands of chunks, a read set moves it with every chunk)
        const uint32_t first_rec = chunk_l2_state[c].rec;
        if (first_rec != racc.rec0) {                      // uniform: rec0 has not changed since the barrier
            recacc_spill(racc, racc.rec0, recs, recs_cap);
            __syncthreads();
            if (threadIdx.x == 0) racc.rec0 = first_rec;
            __syncthreads();
        }
        const Fetched me = nxt;
        if (c_next < c_hi) {
            // the other image is free: its readers passed the barriers of the chunk before this one
            if (chunk_odd[c_next]) stage_image(fasta, (uint64_t)c_next * CHUNK, n_bytes, image[(n_done + 1u) & 1u]);
            fetch(c_next, nxt);
        }
        // exact parser state at this lane's first byte: chunk state . lane prefix (both from the structure pass)
        const L2 chunk_st = chunk_l2_state[c];
        LaneState lst; lst.flags = me.ls_flags; lst.rec_tail = me.ls_rec_tail;
        const LaneStart ln = lane_start(lst, chunk_st, km1);
        wk.begin(ln.ls_in, ln.st, stream_off + base + (uint64_t)threadIdx.x * PIECE);
        uint8_t *piece = buf + threadIdx.x * PIECE;
        PieceBases pb;
        pb.clear();
        // Plain sequence text: the structure pass's pack plus this lane's state.  Every other piece needs the chunk's
        // text: header pieces take it by masks (squeeze_header_piece), pieces with a blank or control byte outside header
        // text byte by byte, which costs the same for one lane as for 64.  They are queued, and the queue is worked off 64
        // pieces per wave pass -- with a header every kilobase (read sets) that is one pass per workgroup instead of one
        // per wave.  A queued piece's result is left in the piece's own 64 bytes of the image.
        const bool clean = ln.clean;                       // chunk_odd counts the rest
        {
            PiecePack pk;
            pk.c_lo = ((unsigned long long)me.p0.y << 32) | me.p0.x; pk.c_hi = ((unsigned long long)me.p0.w << 32) | me.p0.z;
            pk.restart = ((unsigned long long)me.p1.y << 32) | me.p1.x; pk.meta = me.p1.z; pk.pad_ = 0;
            if (all_clean || __any(clean)) squeeze_apply(pk, wk, pb, clean);
        }
        if (!all_clean) {
            if (!clean) queue[atomicAdd(&n_queued, 1u)] = (uint16_t)threadIdx.x;
            __syncthreads();
            const uint32_t n_q = n_queued;
            for (uint32_t q0 = (threadIdx.x >> 6) * 64u; q0 < n_q; q0 += WG) {        // wave-uniform
                const uint32_t qi = q0 + (threadIdx.x & 63u);
                const bool work = qi < n_q;
                const uint32_t pc = work ? queue[qi] : 0u;
                const LaneState l2s = lane_state[(uint64_t)c * WG + pc];
                SeqWalker wq;
                wq.setup(k, recs, recs_cap, &racc);
                const LaneStart lq = lane_start(l2s, chunk_st, km1);
                wq.begin(lq.ls_in, lq.st, stream_off + base + (uint64_t)pc * PIECE);
                // header pieces by masks (text in front of the first record is dropped: that piece takes the byte-wise walk)
                const bool by_masks = work && lane_state_header_piece(l2s) && wq.rec != 0u;
                const uint32_t nbq = (work && !by_masks) ? piece_len_of(pc, base, n_bytes) : 0u;
                uint8_t *pq = buf + pc * PIECE;
                PieceBases rb;
                rb.clear();
                if (__any(by_masks)) squeeze_header_piece(pq, wq, rb, by_masks);
                if (__any(nbq != 0u))
                    for_each_byte_of(pq, nbq, [&](uint32_t i, uint32_t ch, bool act) {
                        uint32_t code;
                        bool rst;
                        const bool take = wq.step(i, ch, act, code, rst);
                        rb.push(take, code, rst);
                    });
                wq.flush_rec_wave();
                wk.seq_tot += wq.seq_tot; wk.kmer_tot += wq.kmer_tot;                  // stream totals travel with the lane that did the work
                if (work) {
                    unsigned long long *res = reinterpret_cast<unsigned long long *>(pq);
                    res[0] = rb.code_lo; res[1] = rb.code_hi; res[2] = rb.restart; res[3] = rb.n;
                }
            }
            __syncthreads();
            if (!clean) {
                const unsigned long long *res = reinterpret_cast<const unsigned long long *>(piece);
                pb.code_lo = res[0]; pb.code_hi = res[1]; pb.restart = res[2]; pb.n = (uint32_t)res[3];
            }
            if (threadIdx.x == 0) n_queued = 0;                                       // read again only after the next barrier
        }
        wk.flush_rec_wave();
        // where the lane's bases go in the chunk's slot: exclusive prefix of the counts over the workgroup
        uint32_t total;
        const uint32_t at = wg_excl_sum<WG / 64, false>(pb.n, scan_sh, total);   // scan_sh: last read before the barriers of the chunk before
        lds_or_bits(slot_codes, 2u * at, pb.code_lo, pb.code_hi, 2u * pb.n);
        lds_or_bits(slot_rst, at, pb.restart, 0ull, pb.n);
        __syncthreads();
        settle();
        // slot -> HBM, 16 bytes per lane, only the words that hold bases; the LDS copy is cleared for the next chunk
        const uint32_t code_q = (total + 63u) / 64u, rst_q = (total + 127u) / 128u;      // uint4 groups in use
        // (the lane's byte offset is formed here, opaque to the compiler: as a loop invariant the two lane addresses were
        // kept in registers, spilled once the header-piece code raised the pressure, and re-loaded from scratch right in
        // front of the stores -- a memory round trip per chunk, 0.204 -> 0.245 ms on the 800 Mbp genome)
        uint32_t lane_off = threadIdx.x * 16u;
        asm volatile("" : "+v"(lane_off));
        uint8_t *gc = reinterpret_cast<uint8_t *>(codes + (uint64_t)c * SLOT_CODE_WORDS);
        uint8_t *gr = reinterpret_cast<uint8_t *>(restarts + (uint64_t)c * SLOT_RST_WORDS);
        if (threadIdx.x < code_q) {
            *reinterpret_cast<uint4 *>(gc + lane_off) = reinterpret_cast<uint4 *>(slot_codes)[threadIdx.x];
            reinterpret_cast<uint4 *>(slot_codes)[threadIdx.x] = make_uint4(0, 0, 0, 0);
        }
        if (threadIdx.x < rst_q) {
            *reinterpret_cast<uint4 *>(gr + lane_off) = reinterpret_cast<uint4 *>(slot_rst)[threadIdx.x];
            reinterpret_cast<uint4 *>(slot_rst)[threadIdx.x] = make_uint4(0, 0, 0, 0);
        }
        if (threadIdx.x == 0) n_bases[c] = total;
    }
    wk.finish();
    recacc_finish(racc, recs, recs_cap, carry);
}

// chunk_fix: what launch_chunk_l2 was given for this feed
void launch_squeeze(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, uint64_t stream_off, const LaneState *lane_state,
                    const PiecePack *packs, const L2 *st2, const uint32_t *chunk_odd, const ChunkFix *chunk_fix, DevRec *recs, uint64_t recs_cap, Carry *carry,
                    hipStream_t s) {
#define PK_SQUEEZE(KC) hipLaunchKernelGGL(k_squeeze<KC>, dim3(pl.n_wg0), dim3(WG), 0, s, fasta, n, stream_off, lane_state, packs, st2, chunk_odd, chunk_fix, pl.k, \
                                          pl.n_chunks, pl.G, b.codes, b.restarts, b.n_bases, recs, recs_cap, carry, b.flags)
    if (pl.k == 15) PK_SQUEEZE(15);
    else if (pl.k == 17) PK_SQUEEZE(17);
    else PK_SQUEEZE(0);
#undef PK_SQUEEZE
}

}  // namespace pk
