// kmer_query.hip -- per-record k-mer hits of a query text against N device-resident 4^k-byte tables.
//
// The query path runs the structure pass and the squeeze of the indexer unchanged; where the indexer sorts the packed stream
// into its own table (kmer_fuse.hip, kmer_part.hip), the kernels here look every canonical k-mer up in the staged tables and
// tally, per record r and table t,
//     hits[r][t]  = #{ windows j of r : min <= T_t[a_j] <= max }        depth[r][t] = sum of T_t[a_j] over the same j.
// Input is the packed stream of kmer_pack.hip: per 16 KiB text chunk a slot of 2-bit codes (base b of the slot in dword
// b / 16, bits 2 (b % 16)), one restart bit per base and the base count; the k-1 bases in front of a slot are the chunk's
// start state.  The stream holds only valid bases of live records, so the window ending at base j is a fixed bit field of two
// dwords, and it is valid iff no restart bit lies among the k-1 positions behind its first base.  k <= 17: the 16 bases
// before a thread's own 16 are all the history a window needs.
//
// The packed stream carries no record identity.  Windows are attributed by ORDINAL: the valid windows of the stream,
// numbered in text order, belong to record r for ordinals in [P[r], P[r+1]), P[r] = sum of n_valid over the records before
// r.  The squeeze has written this feed's DevRec.n_valid when these kernels start, and P[r] depends on records before r
// only, so it is final once r has opened: k_query_scan extends P by the records this feed opened.  A slot's first ordinal
// is the stream's window count before the feed (the host knows it from the previous feed's read-back) plus the prefix sum
// of the per-slot window counts (k_query_count, then the same k_query_scan).  Empty records, many records in one 64-byte
// piece and records that span feeds need nothing else.
//
// Three launches per feed and group of <= QUERY_MAX_TABLES tables (count and scan once per feed):
//   k_query_count   one workgroup per slot: its number of valid windows
//   k_query_scan    one workgroup: slot_first[] and the new entries of P[]
//   k_query_lookup  one workgroup per slot, 16 windows per thread: assemble, gather T_t[a] for every table of the group,
//                   tally.  A wave that lies in one record sums across the wave first; the tallies of a slot meet in an
//                   LDS accumulator (the slot's first QACC_RECS records, in the spirit of RecAcc, kmer_walk.h) and reach
//                   HBM as one atomic per record, table and slot.
// Binned tallies (pk_query_set_bins, W valid windows per bin): the accumulators hold one row per bin instead of one per
// record, record after record and bin after bin; record r's first row is Bf[r] = sum of ceil(n_valid / W) over the records
// before r, final once r has opened exactly as P[r] is, and extended by the same k_query_scan.  The window of ordinal o in
// record r falls in row Bf[r] + (o - P[r]) / W.  From one valid window to the next the row stays or grows by one, so the
// rows of a slot are as dense as its records are in the per-record case and the tally below serves both.
// Count spectra (pk_query_set_spectrum): the lookup also tallies every gathered byte, the zeros included, per row and table:
// spectrum[row][t][c] = #{ j : T_t[a_j] == c }, u64 in HBM.  The tables of a launch are taken one after the other; a
// slot's first QSPEC_ROWS rows meet in one LDS histogram that is flushed (non-zero entries, one HBM atomic each) and zeroed
// between two tables, later rows go to HBM directly.  One count usually dominates a table, so equal counts are joined
// before they reach a counter: a wave that lies in one row first sums the windows that hold the count of its first window
// across the wave (one LDS atomic for all of them), and every thread joins equal consecutive counts of a row.
// Shared windows (pk_query_set_pairs; all tables in one launch): the lookup also keeps, per thread and table, which of the
// thread's 16 windows passed the count window -- one 16-bit plane per table, two planes to a register -- and after the
// table loop tallies, per row and pair of tables i < j,  shared[row][p] = #{ j : V_i(j) and V_j(j) }  as popcount(v_i & v_j):
// the merger's and + bit count (gram_occ.hip) over windows instead of addresses.  The levels are those of hits: a wave in
// one row sums across the wave, a thread masks its planes by row segment, a slot's first QPAIR_ROWS rows meet in LDS.
// Every kernel returns at once, writing nothing, when it finds flags[0] raised (the squeeze backed out: the slots still
// hold an earlier text); the host grows the record and accumulator arrays and repeats the feed's squeeze and these kernels.
#include <type_traits>

#include "kmer_qlane.h"
#include "wg_scan.h"

namespace pk {

constexpr uint32_t QACC_RECS = 128;       // rows (records or bins) of a slot tallied in LDS; later ones (reads below ~128 bytes of
                                          // text, bins of fewer than 128 windows) go to HBM directly
constexpr uint32_t QSPEC_ROWS = 32;       // rows of a slot whose count spectrum of one table is tallied in LDS (256 u32 each)
constexpr uint32_t QPAIR_ROWS = 64;       // rows of a slot whose shared windows are tallied in LDS (one u32 per pair of tables)
constexpr uint32_t QPAIR_MAX = QUERY_MAX_TABLES * (QUERY_MAX_TABLES - 1u) / 2u;   // pairs of one launch

__global__ __launch_bounds__(QNT) void k_query_count(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ restarts,
                                                     const uint32_t *__restrict__ n_bases, const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                     uint32_t *__restrict__ slot_count, const uint32_t *__restrict__ flags) {
    __shared__ uint32_t wsum[QNT / 64];
    if (flags[0]) return;
    const uint32_t c = blockIdx.x;
    const QLane q = q_lane(codes, restarts, n_bases[c], chunk_l2_state, c, threadIdx.x, k);
    uint32_t total;
    wg_excl_sum<QNT / 64, true>((uint32_t)__builtin_popcount(q.ok), wsum, total);   // SH_BUSY only to keep the generated code: wsum is free here, the barrier in front is not needed
    if (threadIdx.x == 0) slot_count[c] = total;
}

// One workgroup.  slot_first[c] = windows_before + the window counts of the slots before c.  P[r] for the records this feed
// opened: p_done entries are final already (the records the stream held before this feed; P[0] = 0), the stream now holds
// carry->n_recs records.  BINS: Bf[r], the bins of the records before r at W windows per bin, over the same r.
template <bool BINS>
__global__ __launch_bounds__(QNT) void k_query_scan(const uint32_t *__restrict__ slot_count, uint32_t n_chunks, unsigned long long windows_before,
                                                    unsigned long long *__restrict__ slot_first, const DevRec *__restrict__ recs,
                                                    const Carry *__restrict__ carry, unsigned long long p_done, unsigned long long *__restrict__ P,
                                                    unsigned long long *__restrict__ Bf, unsigned long long W,
                                                    const uint32_t *__restrict__ flags) {
    __shared__ unsigned long long wsum[QNT / 64];
    if (flags[0]) return;
    // exclusive prefix of v over the workgroup; wsum may still be read by the round before
    auto excl_sum = [&](unsigned long long v, unsigned long long &total) { return wg_excl_sum<QNT / 64, true>(v, wsum, total); };
    unsigned long long run = windows_before;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += QNT) {
        const uint32_t c = c0 + threadIdx.x;
        const unsigned long long v = c < n_chunks ? slot_count[c] : 0ull;
        unsigned long long total;
        const unsigned long long ex = excl_sum(v, total);
        if (c < n_chunks) slot_first[c] = run + ex;
        run += total;
    }
    const unsigned long long n_recs = carry->n_recs;
    unsigned long long r0 = p_done;
    if (r0 == 0ull) {
        if (n_recs == 0ull) return;
        if (threadIdx.x == 0) {
            P[0] = 0ull;
            if constexpr (BINS) Bf[0] = 0ull;
        }
        r0 = 1ull;
    }
    run = r0 > 1ull ? P[r0 - 1ull] : 0ull;                   // (P[0] = 0 may have been written by thread 0 just now)
    unsigned long long run_b = 0ull;
    if constexpr (BINS) run_b = r0 > 1ull ? Bf[r0 - 1ull] : 0ull;
    for (unsigned long long b = r0; b < n_recs; b += QNT) {
        const unsigned long long r = b + threadIdx.x;
        const unsigned long long v = r < n_recs ? recs[r - 1ull].n_valid : 0ull;
        unsigned long long total;
        const unsigned long long ex = excl_sum(v, total);
        if (r < n_recs) P[r] = run + ex + v;                 // inclusive: the windows of the records up to and with r - 1
        run += total;
        if constexpr (BINS) {
            const unsigned long long bins = v ? (v - 1ull) / W + 1ull : 0ull;                      // ceil(v / W)
            const unsigned long long ex_b = excl_sum(bins, total);
            if (r < n_recs) Bf[r] = run_b + ex_b + bins;
            run_b += total;
        }
    }
}

// the largest r in [lo, hi] with P[r] <= o (P[lo] <= o is given)
__device__ __forceinline__ unsigned long long q_find(const unsigned long long *__restrict__ P, unsigned long long lo, unsigned long long hi,
                                                     unsigned long long o) {
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo + 1ull) / 2ull;
        if (P[mid] <= o) lo = mid; else hi = mid - 1ull;
    }
    return lo;
}

// BINS: the accumulators' rows are bins of W windows (Bf, W); otherwise records, and Bf and W are not read.
// SPEC: also spectrum[row][table][256], the tally of every valid window's table count; otherwise `spectrum` is not touched.
// PAIRS (never with SPEC, whose table loop has barriers; t0 = 0 and n_tab = N): also shared[row][pair], the windows valid in
// both tables of every pair i < j < N, pairs in row-major order; otherwise `shared` is not touched.
template <typename KT, bool BINS, bool SPEC, bool PAIRS>
__global__ __launch_bounds__(QNT) void k_query_lookup(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ restarts,
                                                      const uint32_t *__restrict__ n_bases, const L2 *__restrict__ chunk_l2_state, uint32_t k,
                                                      const unsigned long long *__restrict__ slot_first, const unsigned long long *__restrict__ P,
                                                      const unsigned long long *__restrict__ Bf, unsigned long long W,
                                                      const Carry *__restrict__ carry, QueryTables tabs, uint32_t n_tab, uint32_t N, uint32_t t0,
                                                      uint32_t min_count, uint32_t max_count, unsigned long long *__restrict__ hits,
                                                      unsigned long long *__restrict__ depth, unsigned long long *__restrict__ spectrum,
                                                      unsigned long long *__restrict__ shared, const uint32_t *__restrict__ flags) {
    static_assert(!(SPEC && PAIRS), "the spectrum's table loop has barriers; pairs are tallied without");
    __shared__ uint32_t wsum[QNT / 64];
    __shared__ uint32_t acc_h[QACC_RECS * QUERY_MAX_TABLES], acc_d[QACC_RECS * QUERY_MAX_TABLES];
    __shared__ uint32_t acc_s[SPEC ? QSPEC_ROWS * 256u : 1u];   // one table at a time; a slot has at most 16384 windows
    __shared__ uint32_t acc_p[PAIRS ? QPAIR_ROWS * QPAIR_MAX : 1u];   // [row][pair]; a slot has at most 16384 windows
    __shared__ unsigned long long rec_range[BINS ? 6 : 2];   // BINS: + the slot's first and last row, P and Bf of its first record
    if (flags[0]) return;
    const uint32_t c = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t nb = n_bases[c];
    if (nb == 0u) return;
    const QLane q = q_lane(codes, restarts, nb, chunk_l2_state, c, threadIdx.x, k);
    uint32_t total;
    const uint32_t off = wg_excl_sum<QNT / 64, true>((uint32_t)__builtin_popcount(q.ok), wsum, total);   // SH_BUSY only to keep the generated code: wsum is free here, the barrier in front is not needed
    if (total == 0u) return;                                 // uniform
    const unsigned long long first = slot_first[c];
    if (threadIdx.x == 0) {
        const unsigned long long n_recs = carry->n_recs;     // >= 1: a window lies in a record
        const unsigned long long lo = q_find(P, 0ull, n_recs - 1ull, first);
        const unsigned long long hi = q_find(P, lo, n_recs - 1ull, first + total - 1ull);
        rec_range[0] = lo;
        rec_range[1] = hi;
        if constexpr (BINS) {
            const unsigned long long p_lo = P[lo], bf_lo = Bf[lo];
            rec_range[2] = bf_lo + (first - p_lo) / W;
            rec_range[3] = Bf[hi] + (first + total - 1ull - P[hi]) / W;
            rec_range[4] = p_lo;
            rec_range[5] = bf_lo;
        }
    }
    for (uint32_t i = threadIdx.x; i < QACC_RECS * n_tab; i += QNT) { acc_h[i] = 0u; acc_d[i] = 0u; }
    if constexpr (SPEC)
        for (uint32_t i = threadIdx.x; i < QSPEC_ROWS * 256u; i += QNT) acc_s[i] = 0u;
    const uint32_t n_pairs = PAIRS ? n_tab * (n_tab - 1u) / 2u : 0u;
    if constexpr (PAIRS)
        for (uint32_t i = threadIdx.x; i < QPAIR_ROWS * n_pairs; i += QNT) acc_p[i] = 0u;
    __syncthreads();
    const unsigned long long r_lo = rec_range[0], r_hi = rec_range[1];
    // the accumulators' rows this slot touches: records, or bins
    const unsigned long long row_lo = BINS ? rec_range[2] : r_lo, row_hi = BINS ? rec_range[3] : r_hi;

    // ---- the canonical k-mers of this thread's windows (indexer.py:149-150, 341)
    KT a[16];
    q_kmers<KT>(q, k, a);
    // ---- the row of every window, relative to the slot's first
    uint32_t rr[16];
    uint32_t rr_first = 0, rr_last = 0;
    if (row_lo == row_hi) {                                  // uniform: the genome case (with bins: a slot inside one bin)
#pragma unroll
        for (int j = 0; j < 16; j++) rr[j] = 0u;
    } else if (BINS && q.ok) {
        // one division for the first window, then (row, rem) steps with the ordinal: rem windows of the row lie before o
        unsigned long long o = first + off, r = r_lo, at = o - rec_range[4], row0 = rec_range[5];
        if (r_lo != r_hi) {                                  // (one record: no thread searches P)
            r = q_find(P, r_lo, r_hi, o);
            at = o - P[r];
            row0 = Bf[r];
        }
        unsigned long long next = r < r_hi ? P[r + 1ull] : ~0ull;
        unsigned long long row = row0 + at / W, rem = at % W;
        bool seen = false;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            rr[j] = 0u;
            if ((q.ok >> j) & 1u) {
                if (o >= next) {
                    do { r++; next = r < r_hi ? P[r + 1ull] : ~0ull; } while (o >= next);
                    row = Bf[r]; rem = 0ull;
                } else if (rem == W) { row++; rem = 0ull; }
                rr[j] = (uint32_t)(row - row_lo);
                if (!seen) { rr_first = rr[j]; seen = true; }
                rr_last = rr[j];
                o++; rem++;
            }
        }
    } else if (q.ok) {
        unsigned long long o = first + off;
        unsigned long long r = q_find(P, r_lo, r_hi, o);
        unsigned long long next = r < r_hi ? P[r + 1ull] : ~0ull;
        bool seen = false;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            rr[j] = 0u;
            if ((q.ok >> j) & 1u) {
                while (o >= next) { r++; next = r < r_hi ? P[r + 1ull] : ~0ull; }
                rr[j] = (uint32_t)(r - r_lo);
                if (!seen) { rr_first = rr[j]; seen = true; }
                rr_last = rr[j];
                o++;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) rr[j] = 0u;
    }
    // does the whole wave lie in one row?
    const bool has = q.ok != 0u;
    const unsigned long long holders = __ballot(has);
    // for a wave with a window (holders != 0): the row of its first window, and whether all its windows lie in that row
    auto wave_ref = [&]() { return (uint32_t)__shfl((int)rr_first, (int)__builtin_ctzll(holders), 64); };
    auto wave_in = [&](uint32_t ref) { return (bool)__all(!has || (rr_first == ref && rr_last == ref)); };
    auto add = [&](uint32_t rel, uint32_t tt, uint32_t h, uint32_t d) {
        if (rel < QACC_RECS) {
            if (h) atomicAdd(&acc_h[rel * n_tab + tt], h);
            if (d) atomicAdd(&acc_d[rel * n_tab + tt], d);
        } else {
            const unsigned long long at = (row_lo + rel) * N + t0 + tt;
            if (h) atomicAdd(&hits[at], (unsigned long long)h);
            if (d) atomicAdd(&depth[at], (unsigned long long)d);
        }
    };
    // n windows of row `rel` (relative to the slot's first) with the count cnt in table tt
    auto add_spec = [&](uint32_t rel, uint32_t tt, uint32_t cnt, uint32_t n) {
        if (rel < QSPEC_ROWS) atomicAdd(&acc_s[rel * 256u + cnt], n);
        else atomicAdd(&spectrum[((row_lo + rel) * N + t0 + tt) * 256ull + cnt], (unsigned long long)n);
    };
    // PAIRS: the planes of this thread, table 2i in the low half of pl[i] and table 2i + 1 in the high half; bit j of a
    // plane: window j is valid and its count lies in the count window
    uint32_t pl[PAIRS ? QUERY_MAX_TABLES / 2u : 1u];
    if constexpr (PAIRS) {
#pragma unroll
        for (uint32_t i = 0; i < QUERY_MAX_TABLES / 2u; i++) pl[i] = 0u;
    }
    // one table for this thread's windows; wave-uniform where it matters, no barrier inside
    auto tally = [&](uint32_t tt, const uint32_t ref, const bool wave_one) {
        const uint8_t *__restrict__ T = tabs.t[tt];
        uint32_t cv[16];                                     // all gathers of a table in flight before the first is used
#pragma unroll
        for (int j = 0; j < 16; j++) cv[j] = ((q.ok >> j) & 1u) ? (uint32_t)T[a[j]] : 0u;   // a count of 0 lies in no window (min >= 1)
        if (wave_one) {
            uint32_t h = 0, d = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const bool in = cv[j] >= min_count && cv[j] <= max_count;
                h += in ? 1u : 0u; d += in ? cv[j] : 0u;
            }
            for (int s = 32; s; s >>= 1) { h += __shfl_down(h, s, 64); d += __shfl_down(d, s, 64); }
            if (lane == 0u) add(ref, tt, h, d);
        } else if (has) {
            uint32_t cur = rr_first, h = 0, d = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if ((q.ok >> j) & 1u) {
                    if (rr[j] != cur) { add(cur, tt, h, d); h = 0; d = 0; cur = rr[j]; }
                    const bool in = cv[j] >= min_count && cv[j] <= max_count;
                    h += in ? 1u : 0u; d += in ? cv[j] : 0u;
                }
            }
            add(cur, tt, h, d);
        }
        if constexpr (PAIRS) {
            uint32_t bits = 0u;
#pragma unroll
            for (int j = 0; j < 16; j++) bits |= (cv[j] >= min_count && cv[j] <= max_count) ? 1u << j : 0u;
            bits <<= 16u * (tt & 1u);
#pragma unroll
            for (uint32_t i = 0; i < QUERY_MAX_TABLES / 2u; i++) pl[i] |= (i == (tt >> 1)) ? bits : 0u;   // (tt is uniform: selects, no indexed register)
        }
        if constexpr (SPEC) {
            // peel: the count of the wave's first window, summed over the wave (the dominant count, more often than not);
            // 256 is no count and peels nothing
            uint32_t peel = 256u;
            if (wave_one) {
                uint32_t mine = 0u, n0 = 0u;
#pragma unroll
                for (int j = 15; j >= 0; j--) mine = ((q.ok >> j) & 1u) ? cv[j] : mine;
                peel = (uint32_t)__shfl((int)mine, (int)__builtin_ctzll(holders), 64);
#pragma unroll
                for (int j = 0; j < 16; j++) n0 += (((q.ok >> j) & 1u) && cv[j] == peel) ? 1u : 0u;
                for (int s = 32; s; s >>= 1) n0 += __shfl_down(n0, s, 64);
                if (lane == 0u) add_spec(ref, tt, peel, n0);
            }
            // the rest: runs of equal (row, count)
            uint32_t cur_r = 0u, cur_c = 0u, n = 0u;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (((q.ok >> j) & 1u) && cv[j] != peel) {
                    if (n && (rr[j] != cur_r || cv[j] != cur_c)) { add_spec(cur_r, tt, cur_c, n); n = 0u; }
                    cur_r = rr[j]; cur_c = cv[j]; n++;
                }
            }
            if (n) add_spec(cur_r, tt, cur_c, n);
        }
    };
    // PAIRS, after the table loop: the pairs of this thread's planes.  The loops over the tables are unrolled over all
    // QUERY_MAX_TABLES and cut short by the uniform n_tab, so that every plane is a fixed half of a fixed register.
    auto plane = [&](uint32_t t) { return (pl[t >> 1] >> (16u * (t & 1u))) & 0xffffu; };
    auto add_pair = [&](uint32_t rel, uint32_t p, uint32_t n) {
        if (rel < QPAIR_ROWS) atomicAdd(&acc_p[rel * n_pairs + p], n);
        else atomicAdd(&shared[(row_lo + rel) * n_pairs + p], (unsigned long long)n);
    };
    auto tally_pairs = [&](const uint32_t ref, const bool wave_one) {
        if (wave_one) {                                      // one add per pair and wave
#pragma unroll
            for (uint32_t i = 0; i + 1u < QUERY_MAX_TABLES; i++) {
                if (i + 1u < n_tab) {
                    const uint32_t vi = plane(i), p0 = i * (2u * n_tab - i - 1u) / 2u;
#pragma unroll
                    for (uint32_t j = i + 1u; j < QUERY_MAX_TABLES; j++) {
                        if (j < n_tab) {
                            uint32_t n = (uint32_t)__builtin_popcount(vi & plane(j));
                            for (int s = 32; s; s >>= 1) n += __shfl_down(n, s, 64);
                            if (lane == 0u && n) add_pair(ref, p0 + j - i - 1u, n);
                        }
                    }
                }
            }
        } else if (has) {
            // row segment after row segment: `m`, the windows of the first row among those left
            uint32_t rest = q.ok;
            while (rest) {
                const uint32_t j0 = (uint32_t)__builtin_ctz(rest);
                uint32_t row = 0u, m = 0u;
#pragma unroll
                for (uint32_t j = 0; j < 16u; j++) row = j == j0 ? rr[j] : row;
#pragma unroll
                for (uint32_t j = 0; j < 16u; j++) m |= rr[j] == row ? 1u << j : 0u;
                m &= rest;
                rest &= ~m;
#pragma unroll
                for (uint32_t i = 0; i + 1u < QUERY_MAX_TABLES; i++) {
                    const uint32_t vi = plane(i) & m, p0 = i * (2u * n_tab - i - 1u) / 2u;
                    if (i + 1u < n_tab && vi) {
#pragma unroll
                        for (uint32_t j = i + 1u; j < QUERY_MAX_TABLES; j++) {
                            if (j < n_tab) {
                                const uint32_t n = (uint32_t)__builtin_popcount(vi & plane(j));
                                if (n) add_pair(row, p0 + j - i - 1u, n);
                            }
                        }
                    }
                }
            }
        }
    };
    if constexpr (SPEC) {
        const unsigned long long span = row_hi - row_lo + 1ull;
        const uint32_t n_spec = (uint32_t)(span < QSPEC_ROWS ? span : QSPEC_ROWS) * 256u;
        const uint32_t ref = holders != 0ull ? wave_ref() : 0u;
        const bool wave_one = holders != 0ull && wave_in(ref);
        for (uint32_t tt = 0; tt < n_tab; tt++) {            // uniform: the barriers are met by every thread
            if (holders != 0ull) tally(tt, ref, wave_one);
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < n_spec; i += QNT) {
                const uint32_t v = acc_s[i];
                if (v) {
                    atomicAdd(&spectrum[((row_lo + i / 256u) * N + t0 + tt) * 256ull + i % 256u], (unsigned long long)v);
                    acc_s[i] = 0u;
                }
            }
            __syncthreads();
        }
    } else if (holders != 0ull) {                            // wave-uniform
        const uint32_t ref = wave_ref();
        const bool wave_one = wave_in(ref);
        for (uint32_t tt = 0; tt < n_tab; tt++) tally(tt, ref, wave_one);
        if constexpr (PAIRS) tally_pairs(ref, wave_one);
    }
    __syncthreads();
    if constexpr (PAIRS) {
        const unsigned long long span = row_hi - row_lo + 1ull;
        const uint32_t n_acc = (uint32_t)(span < QPAIR_ROWS ? span : QPAIR_ROWS) * n_pairs;
        for (uint32_t i = threadIdx.x; i < n_acc; i += QNT) {
            const uint32_t v = acc_p[i];
            if (v) atomicAdd(&shared[row_lo * n_pairs + i], (unsigned long long)v);
        }
    }
    {
        const unsigned long long span = row_hi - row_lo + 1ull;
        const uint32_t n_acc = (uint32_t)(span < QACC_RECS ? span : QACC_RECS) * n_tab;
        for (uint32_t i = threadIdx.x; i < n_acc; i += QNT) {
            const uint32_t h = acc_h[i], d = acc_d[i];
            const unsigned long long at = (row_lo + i / n_tab) * N + t0 + i % n_tab;
            if (h) atomicAdd(&hits[at], (unsigned long long)h);
            if (d) atomicAdd(&depth[at], (unsigned long long)d);
        }
    }
}

// ------------------------------------------------------------------ host side -------------------
size_t query_workspace(uint32_t n_chunks, uint8_t *base, PartBuffers *view, QueryBuffers *qview, PartSignals *signals) {
    PartBuffers unused_p, &b = view ? *view : unused_p;
    QueryBuffers unused_q, &qb = qview ? *qview : unused_q;
    size_t o = 0;
    const auto place = [&](auto *&p, size_t bytes) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(base) + o);
        o = (o + bytes + 255) & ~(size_t)255;
    };
    b = PartBuffers{};
    place(b.codes, (size_t)n_chunks * SLOT_CODE_WORDS * 4);
    place(b.restarts, (size_t)n_chunks * SLOT_RST_WORDS * 4);
    place(b.n_bases, (size_t)n_chunks * 4);
    place(qb.slot_count, (size_t)n_chunks * 4);
    place(qb.slot_first, (size_t)n_chunks * 8);
    b.signals = signals;                                   // outside the workspace: next to the stream totals (pk_host.h: Tail)
    b.side_n = &b.signals->side_n;
    b.flags = b.signals->flags;
    return o;
}

void launch_query_scan(const PartPlan &pl, const PartBuffers &b, const QueryBuffers &qb, const L2 *st2, uint64_t windows_before, const DevRec *recs,
                       const Carry *carry, uint64_t p_done, unsigned long long *P, unsigned long long *Bf, uint64_t bin_windows, hipStream_t s) {
    hipLaunchKernelGGL(k_query_count, dim3(pl.n_chunks), dim3(QNT), 0, s, (const uint32_t *)b.codes, (const uint32_t *)b.restarts,
                       (const uint32_t *)b.n_bases, st2, pl.k, qb.slot_count, (const uint32_t *)b.flags);
#define PK_QUERY_SCAN(BINS) hipLaunchKernelGGL(k_query_scan<BINS>, dim3(1), dim3(QNT), 0, s, (const uint32_t *)qb.slot_count, pl.n_chunks,                 \
                                               (unsigned long long)windows_before, qb.slot_first, recs, carry, (unsigned long long)p_done, P, Bf,         \
                                               (unsigned long long)bin_windows, (const uint32_t *)b.flags)
    if (bin_windows) PK_QUERY_SCAN(true);
    else PK_QUERY_SCAN(false);
#undef PK_QUERY_SCAN
}

void launch_query_lookup(const PartPlan &pl, const PartBuffers &b, const QueryBuffers &qb, const L2 *st2, const unsigned long long *P,
                         const unsigned long long *Bf, uint64_t bin_windows, const Carry *carry, const uint8_t *const *tables, uint32_t n_tab, uint32_t N, uint32_t t0, uint32_t min_count, uint32_t max_count,
                         unsigned long long *hits, unsigned long long *depth, unsigned long long *spectrum, unsigned long long *shared, hipStream_t s) {
    const QueryTables tabs = query_tables(tables, n_tab);
#define PK_QUERY_LOOKUP(KT, BINS, SPEC, PAIRS) hipLaunchKernelGGL((k_query_lookup<KT, BINS, SPEC, PAIRS>), dim3(pl.n_chunks), dim3(QNT), 0, s, (const uint32_t *)b.codes,               \
                                                     (const uint32_t *)b.restarts, (const uint32_t *)b.n_bases, st2, pl.k,                                  \
                                                     (const unsigned long long *)qb.slot_first, P, Bf, (unsigned long long)bin_windows, carry, tabs, n_tab, \
                                                     N, t0, min_count, max_count, hits, depth, spectrum, shared, (const uint32_t *)b.flags)
#define PK_QUERY_LOOKUP_K(BINS, SPEC, PAIRS) do { if (pl.k <= 15) PK_QUERY_LOOKUP(uint32_t, BINS, SPEC, PAIRS); else PK_QUERY_LOOKUP(uint64_t, BINS, SPEC, PAIRS); } while (0)
    if (spectrum) { if (bin_windows) PK_QUERY_LOOKUP_K(true, true, false); else PK_QUERY_LOOKUP_K(false, true, false); }
    else if (shared) { if (bin_windows) PK_QUERY_LOOKUP_K(true, false, true); else PK_QUERY_LOOKUP_K(false, false, true); }
    else { if (bin_windows) PK_QUERY_LOOKUP_K(true, false, false); else PK_QUERY_LOOKUP_K(false, false, false); }
#undef PK_QUERY_LOOKUP_K
#undef PK_QUERY_LOOKUP
}

}  // namespace pk
