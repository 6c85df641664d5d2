// pk_kernels.h -- device-side structs and kernel launchers shared between the kernel files and the host layer (pk_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fasta_fsm.h"

namespace pk {

// One FASTA record while it is being accumulated in HBM (atomics from many lanes).
struct DevRec {
    uint64_t name_off;  // first byte after '>'
    uint64_t name_end;  // one past the last non-blank header byte (atomicMax)
    uint64_t seq_len;   // atomicAdd
    uint64_t n_valid;   // atomicAdd
};

// Parser state carried between feeds + running totals; lives in device memory so that consecutive
// feeds need no host round trip for it.
struct Carry {
    L2 l2;               // state after the last byte fed so far
    L1 l1;
    uint32_t pad;
    uint64_t n_recs;     // = l2.rec, mirrored for the host read-back
    uint64_t total_bp;   // sum of seq_len over all records
    uint64_t num_kmers;  // valid windows counted
    // k = 19, 21: the last 32 valid bases of the stream, newest at the top, at the start of the feed being counted and at
    // its end (k_deep_tail).  The run state above says how many of them a window may use; its 32 bits hold only 16.
    uint64_t deep_in, deep_out;
};

// What a feed's partition passes signal through, zeroed as one span before every attempt (for the first attempt of a feed
// by the scan kernel of the structure pass).  flags[0]: 2 = the squeeze backed out (record array too small), 1 = a bucket
// room or a layout total overflowed; every kernel behind the squeeze returns at once when it finds it raised, so the first
// value raised is the one the host reads.  flags[1]: buckets recounted (statistics).
struct PartSignals {
    unsigned long long side_n;   // entries in the side list
    uint32_t flags[4];
};

void launch_chunk_l1(const uint8_t *fasta, uint64_t n, L1 *chunk_l1, uint32_t n_chunks, hipStream_t s);
void launch_scan_l1(const L1 *in, uint32_t n_chunks, Carry *carry, L1 *out, L1 *tile_ws, PartSignals *zeroed, hipStream_t s);
void launch_scan_l2(const L2 *in, uint32_t n_chunks, Carry *carry, L2 *out, L2 *tile_ws, uint32_t k, hipStream_t s);
void launch_hist8(const uint8_t *table8, uint64_t n, unsigned long long *hist, hipStream_t s);
// the tail (tail_bytes, a multiple of 8) becomes a copy of tail0, the record array (recs_bytes, whole records; may be null) zero
void launch_reset(void *tail, const void *tail0, size_t tail_bytes, DevRec *recs, size_t recs_bytes, hipStream_t s);

// kmer_pack.hip -- the packed stream: one slot per 16 KiB text chunk
constexpr uint32_t SLOT_CODE_WORDS = 1024;   // 16384 bases x 2 bits
constexpr uint32_t SLOT_RST_WORDS = 512;     // 16384 restart bits
constexpr uint32_t SQUEEZE_G_MAX = 256;      // chunks per workgroup of k_squeeze at most (make_part_plan): it looks at them one thread each

// kmer_fuse.hip / kmer_part.hip -- partitioned table update
struct PartPlan {
    uint32_t k, addr_bits;   // addr_bits = 2k - slice_bits: address bits of the table this indexer holds
    uint32_t slice_bits, slice_index;   // k-mers whose top slice_bits address bits differ from slice_index are not this table's
    uint32_t fb_bits;        // address bits inside a final bucket (<= 16)
    uint32_t b1, b2, B1, B2; // level-1 / level-2 digit widths and bucket counts
    uint32_t n_chunks;       // 16 KiB FASTA chunks in this feed
    uint32_t n_wg0, G;       // persistent workgroups of the squeeze kernel and chunks per workgroup
    uint32_t n_wg1, G1;      // the same for the level-1 sort (k_walk_sort)
    uint64_t R2;             // records per level-2 work item
    uint32_t sample_stride;  // every how-manieth slot is tallied to size the buckets (1 = all: exact)
    uint32_t n_tally;        // what the sampling launch tallies: B1 * B2 final buckets (both levels are then laid out from
                             // the estimate), or just the B1 level-1 buckets (one level, or too many final buckets: k = 17)
    uint32_t sample2;        // 1: the final buckets (too many to tally while sampling slots: 2^15 < B1 * B2 <= 2^18) are sized from a
                             // sample of the level-1 RECORDS, after the level-1 sort, and level 2 claims its room like the others
    uint64_t capacity1;      // record slots for all level-1 buckets together (the dump area starts there)
    uint64_t capacity2;      // the same for the final buckets, where they are laid out from the estimate
};
constexpr uint32_t PART_MAX_B1 = 512;   // level-1 buckets at most (part_plan_check): k_level1_finish ranks them in LDS arrays of this size
constexpr uint32_t COUNT_WGS = 256;   // workgroups (= tally rows) of the sampling launch
constexpr uint32_t HIST_REPLICAS = 64;   // copies of the 256-bin histogram change the bucket-count workgroups add into (zeroed by their reader, k_apply_side)
// The workspace of the partition passes: one device allocation, seen through typed pointers.  part_workspace
// (kmer_part.hip) is the one place that lays it out.
struct PartBuffers {
    uint32_t *codes, *restarts, *n_bases;                   // the squeezed text: one slot per chunk
    uint32_t *tally_rows, *tally_tot;                       // the sampling launch's rows and their column sums
    uint32_t *sampled_n, *block_tot;                        // sample2 only (null otherwise): records sampled per level-1 bucket, k_rooms2's block totals
    uint32_t *bucket_base, *bucket_end, *cursor1, *cap_end, *wg2_start;   // level 1, B1 + 1 words each
    uint32_t *l2_order;                                     // B1 words: the level-1 buckets in the order level 2 walks them
    uint32_t *final_start, *cursor2, *cap2_end;             // the final buckets, B1 * B2 + 1 words each
    void *out1, *out2;                                      // level-1 and final records, each with its dump tile
    unsigned long long *side, *side_n;                      // hot-key (address, count) entries; side_n = &signals->side_n
    uint64_t side_cap;
    PartSignals *signals;
    uint32_t *flags;                                        // = signals->flags
};
struct PartEvents { hipEvent_t sort_begin, sort_end, part_end; };   // recorded by launch_partitioned around the level-1 sort and behind level 2
PartPlan make_part_plan(uint32_t k, uint64_t n_bytes, uint32_t slice_bits, uint32_t slice_index);
// The two choices the launchers make on top of the plan, as functions: launch_ws / launch_partitioned switch on them and
// pk_diag_plan_slice reports them (the values are part of that diagnostic: include/pykmer_hip.h).
enum WsVariant : uint32_t { WS_NARROW = 0, WS_NARROW_SLICED = 1, WS_K15 = 2, WS_K17 = 3, WS_WIDE_SLICED = 4, WS_DEEP = 5,
                            WS_WIDE = 6 };   // WS_WIDE: 64-bit k-mers, unsliced, not 9 + 9 -- no k that check_k lets through has it
enum CountKernel : uint32_t { COUNT_WHOLE = 0, COUNT_BYTES = 1, COUNT_HALF = 2 };
WsVariant walk_sort_variant(const PartPlan &pl);                      // kmer_fuse.hip: the k_walk_sort instantiation
uint32_t bucket_split(const PartPlan &pl, uint64_t n_bytes);          // kmer_part.hip: 1 = two count workgroups (or byte counters) per final bucket
CountKernel bucket_count_kernel(const PartPlan &pl, uint64_t n_bytes);   // kmer_part.hip: k_bucket_count, _bytes or _half_lean
// PK_OK, or PK_ERR_HIP and a message naming the limit of the kernels that the plan exceeds
int part_plan_check(const PartPlan &pl, uint64_t n_bytes);
// the bytes of the workspace for the plan; with `view`, also where its regions lie in an allocation starting at `base`.
// `signals`: the feed's PartSignals, which live outside the workspace (the view's signals, side_n and flags point there)
size_t part_workspace(const PartPlan &pl, uint64_t n_bytes, uint8_t *base = nullptr, PartBuffers *view = nullptr, PartSignals *signals = nullptr);
void part_set_attributes();
void fuse_set_attributes();
// The launchers take the plan, the view and what lives outside the workspace.  `carry`: its deep_in / deep_out words are
// touched by k = 19, 21 only.
// chunk_fix (one record per chunk) non-null: a counting feed -- the structure pass squeezes the settled chunks (ChunkFix,
// fasta_fsm.h) into the slots of `b` itself, and the squeeze pass only completes them.  Null: a query feed, nothing is settled.
void launch_chunk_l2(const uint8_t *fasta, uint64_t n, const L1 *st1, L2 *chunk_l2, LaneState *lane_state, PiecePack *packs, uint32_t *chunk_odd,
                     ChunkFix *chunk_fix, const PartBuffers &b, uint32_t n_chunks, uint32_t k, hipStream_t s);
void launch_squeeze(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, uint64_t stream_off, const LaneState *lane_state,
                    const PiecePack *packs, const L2 *st2, const uint32_t *chunk_odd, const ChunkFix *chunk_fix, DevRec *recs, uint64_t recs_cap, Carry *carry,
                    hipStream_t s);
void launch_deep_tail(const PartPlan &pl, const PartBuffers &b, Carry *carry, hipStream_t s);
void launch_provision(const PartPlan &pl, const PartBuffers &b, const L2 *st2, uint32_t stride, const Carry *carry, hipStream_t s);
void launch_walk_sort(const PartPlan &pl, const PartBuffers &b, const L2 *st2, const Carry *carry, hipStream_t s);
// Everything behind the squeeze for one feed, on zeroed signals.  PK_OK, or PK_ERR_HIP and a message naming the stage whose launch failed.
int launch_partitioned(const PartPlan &pl, const PartBuffers &b, const L2 *st2, uint64_t n_bytes, uint32_t stride, const Carry *carry, uint8_t *table8,
                       unsigned long long *hist, unsigned long long *hist_rep, bool fresh, const PartEvents &ev, hipStream_t s);

// kmer_query.hip -- per-record k-mer hits against device-resident tables.  The query path squeezes a feed
// like the indexer and then runs these where the indexer runs launch_partitioned.
constexpr uint32_t QUERY_MAX_TABLES = 16;                   // tables per lookup launch; more are looked up group by group
struct QueryTables { const uint8_t *t[QUERY_MAX_TABLES]; };
// tables[0 .. n_tab) as a launch takes them; the slots behind them repeat the first table, so that every slot can be read
inline QueryTables query_tables(const uint8_t *const *tables, uint32_t n_tab) {
    QueryTables tabs;
    for (uint32_t i = 0; i < QUERY_MAX_TABLES; i++) tabs.t[i] = tables[i < n_tab ? i : 0];
    return tabs;
}
struct QueryBuffers {
    uint32_t *slot_count;                                   // valid windows per slot
    unsigned long long *slot_first;                         // stream ordinal of a slot's first valid window
};
// the workspace of a query feed: the squeezed text (the PartBuffers fields the squeeze uses; the rest stay null) and the
// per-slot window counts; `signals` as for part_workspace
size_t query_workspace(uint32_t n_chunks, uint8_t *base = nullptr, PartBuffers *view = nullptr, QueryBuffers *qview = nullptr,
                       PartSignals *signals = nullptr);
// per-slot window counts -> slot_first; P[p_done .. carry->n_recs) from recs[].n_valid (P[r] = valid windows before record r).
// bin_windows = W > 0: also Bf over the same r (Bf[r] = bins of W windows in the records before r); 0: Bf is not touched.
void launch_query_scan(const PartPlan &pl, const PartBuffers &b, const QueryBuffers &qb, const L2 *st2, uint64_t windows_before, const DevRec *recs,
                       const Carry *carry, uint64_t p_done, unsigned long long *P, unsigned long long *Bf, uint64_t bin_windows, hipStream_t s);
// tables[0 .. n_tab) are columns t0 .. t0 + n_tab of the row-major [row][N] u64 accumulators hits / depth; a row is a record
// (bin_windows = 0) or a bin of bin_windows valid windows: row Bf[r] + (o - P[r]) / W for the window of ordinal o in record r.
// spectrum: null, or the [row][N][256] u64 tally of the table counts of every valid window (the same rows), added to
// shared: null, or (without spectrum; t0 = 0 and n_tab = N) the [row][N (N - 1) / 2] u64 tally of the windows valid in both
// tables of a pair i < j, pairs in row-major order (the same rows), added to
void launch_query_lookup(const PartPlan &pl, const PartBuffers &b, const QueryBuffers &qb, const L2 *st2, const unsigned long long *P,
                         const unsigned long long *Bf, uint64_t bin_windows, const Carry *carry, const uint8_t *const *tables, uint32_t n_tab, uint32_t N, uint32_t t0, uint32_t min_count, uint32_t max_count,
                         unsigned long long *hits, unsigned long long *depth, unsigned long long *spectrum, unsigned long long *shared, hipStream_t s);

// kmer_coords.hip -- base coordinates of a binned query's rows (DESIGN.md 4.10 "Coordinates"), behind launch_query_scan of the
// same feed (slot_first, P, Bf) and its squeeze (recs[].n_valid).  chunk_pos: n_chunks words of scratch.  pos_in: the position
// in the open record at the feed's first byte; pos_out receives the one behind its last.  bin_start / bin_end: rows_cap words
// each; row Bf[r] + j / W takes the first base of its first window and one past the last base of its last.
void launch_query_coords(const PartPlan &pl, const PartBuffers &b, const QueryBuffers &qb, const uint8_t *fasta, uint64_t n, const LaneState *lane_state,
                         const PiecePack *packs, const L2 *st2, const uint32_t *chunk_odd, const DevRec *recs, const unsigned long long *P,
                         const unsigned long long *Bf, uint64_t bin_windows, unsigned long long *chunk_pos, const unsigned long long *pos_in,
                         unsigned long long *pos_out, unsigned long long *bin_start, unsigned long long *bin_end, uint64_t rows_cap, hipStream_t s);

// the first two kernels of launch_query_coords alone: chunk_pos[c] = the position at chunk c's first byte, pos_out as above
void launch_coords_positions(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state,
                             const PiecePack *packs, const L2 *st2, const uint32_t *chunk_odd, unsigned long long *chunk_pos,
                             const unsigned long long *pos_in, unsigned long long *pos_out, hipStream_t s);

// kmer_cover.hip -- the bases of the stream that the tables cover, one bit per valid base, and the text with them marked
// (DESIGN.md 4.14).  All three run behind the squeeze of the same feed (n_bases[]).
// nb_in: the valid bases of the stream before the feed; nb_out receives the number behind it; base_first: n_chunks words.
void launch_cover_scan(const PartPlan &pl, const PartBuffers &b, const unsigned long long *nb_in, unsigned long long *nb_out,
                       unsigned long long *base_first, hipStream_t s);
// ORs into bitmap (n_words u32, bit g at word g / 32, bit g % 32) the bases that lie in a valid window with min <= T[a] <= max
// in one of tables[0 .. n_tab), n_tab <= QUERY_MAX_TABLES
void launch_query_cover(const PartPlan &pl, const PartBuffers &b, const L2 *st2, const unsigned long long *base_first, const uint8_t *const *tables,
                        uint32_t n_tab, uint32_t min_count, uint32_t max_count, uint32_t *bitmap, uint64_t n_words, hipStream_t s);
// out (n + 64 bytes, 16-byte aligned) = the feed's text with the selected valid bases marked: those whose bit in `bits` is set,
// with mode bit 1 (invert) the others; lower case, with mode bit 0 (hard) 'N'.  masked[r] (recs_cap words) += the selected
// bases of record r.
void launch_mask_apply(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state, const L2 *st2,
                       const unsigned long long *base_first, const uint32_t *bits, uint64_t n_words, uint32_t mode, uint8_t *out,
                       unsigned long long *masked, uint64_t recs_cap, hipStream_t s);

// kmer_intervals.hip -- the selected bases of a mask feed as intervals of positions (DESIGN.md 4.14 "Intervals"), behind
// launch_cover_scan (base_first) and launch_coords_positions (chunk_pos) of the same feed; fasta .. mode as launch_mask_apply
// takes them.  chunk_iv: 2 * n_chunks words of scratch.  ns_in / ne_in: the starts and ends of the stream before the feed
// (their difference is the open run); ns_out / ne_out receive those behind it.
void launch_iv_count(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state, const L2 *st2,
                     const unsigned long long *base_first, const uint32_t *bits, uint64_t n_words, uint32_t mode, unsigned long long *chunk_iv,
                     const unsigned long long *ns_in, const unsigned long long *ne_in, unsigned long long *ns_out, unsigned long long *ne_out,
                     hipStream_t s);
// behind launch_iv_count: iv_record / iv_start (row = starts of the stream before) and iv_end (row = ends before); rows at or
// past `cap` are not written
void launch_iv_write(const PartPlan &pl, const PartBuffers &b, const uint8_t *fasta, uint64_t n, const LaneState *lane_state, const L2 *st2,
                     const unsigned long long *base_first, const uint32_t *bits, uint64_t n_words, uint32_t mode, const unsigned long long *chunk_pos,
                     const unsigned long long *chunk_iv, unsigned long long *iv_record, unsigned long long *iv_start, unsigned long long *iv_end,
                     uint64_t cap, hipStream_t s);

// fastq.hip -- the FASTQ front end: FASTQ bytes -> the FASTA text they stand for, checked record by record
struct FqState {             // the stream after some prefix of it
    uint64_t line;           // line terminators seen (the role of the open line is line & 3)
    uint64_t out;            // bytes emitted to the FASTA pipeline
    uint64_t curlen;         // bytes of the open line so far
    uint32_t ws, pad;        // 1: the open line holds nothing but str.strip() whitespace so far
};
struct FqSum {               // what a stretch of bytes does to an FqState
    uint32_t nt;             // terminators
    uint32_t tail;           // bytes behind the last one (or all of them)
    uint32_t kept[4];        // bytes kept when entered in role r
    uint32_t ws, pad;        // 1: the tail holds only whitespace
};
struct FqRec {               // per record number
    uint64_t line1;          // stream offset of line 1
    uint64_t len2, len4;     // raw lengths of lines 2 and 4
};
enum : uint32_t { FQ_RULE_AT = 1, FQ_RULE_GT = 2, FQ_RULE_PLUS = 3, FQ_RULE_LEN = 4, FQ_RULE_END = 5 };
struct FqCarry {
    FqState st;              // after everything fed
    FqState in;              // at the start of the last feed
    uint64_t bytes_fed, in_bytes;
    uint64_t err;            // smallest (record << 3 | rule) that broke a rule, ~0: none
    uint64_t trail;          // the first empty header line (only blank lines may follow it), ~0: none
    uint64_t full;           // 1 + the last line with a byte that is no terminator
    uint64_t need;           // record slots the stream needs
    uint32_t prev4, prev4_in;   // the last 4 bytes of the stream (before the last feed), newest highest
    // base qualities (tq > 0) only
    uint64_t masked, masked_in;   // line-2 bytes turned into 'N' (before the last feed)
    uint64_t settled;        // emitted bytes before this offset belong to records whose whole line 4 has been seen
};
// k_fq_count + k_fq_scan + launch_fq_write.  out: held + n + 64 bytes, 16-byte aligned; record slots at or beyond recs_cap are
// not written (carry->need says how many are needed, and launch_fq_write can be repeated with a larger array).
// tq = 0: base qualities are not looked at, held = 0 and out2 is null.  tq = 1 .. 255: k_fq_write_held stands in for
// k_fq_write and k_fq_mask runs behind k_fq_check; out2 (recs_cap words, a record's slot like recs) receives per record the
// bytes emitted before its line 2; the first `held` bytes of out are emitted text from before this feed that line 4 bytes of
// this feed may still change (the text behind carry->settled of the feed before), and this feed's text goes behind them.
void launch_fq_front(const uint8_t *fastq, uint64_t n, FqSum *sums, FqState *st, uint8_t *out, uint64_t held, FqRec *recs, uint64_t *out2,
                     uint64_t recs_cap, uint32_t tq, FqCarry *carry, hipStream_t s);
void launch_fq_write(const uint8_t *fastq, uint64_t n, const FqState *st, uint8_t *out, uint64_t held, FqRec *recs, uint64_t *out2,
                     uint64_t recs_cap, uint32_t tq, FqCarry *carry, hipStream_t s);

// gram_scan.hip
// tables: device array of N device pointers, each n_slice bytes (16-byte aligned).  pair: device N*N u64,
// zeroed by the launcher when zero_first; [i][i] += total_i, [i][j] (i<j) += shared_ij.
int launch_gram(const uint8_t *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count,
                unsigned long long *dev_pair, bool zero_first, hipStream_t s);

// Several validity windows in one pass over the tables (threshold sweeps): at most gram_windows_per_pass(N) windows
// per launch (0: this N is served by one launch_gram per window), sorted by min_count; window w's tallies are added to
// block out_index[w] (< 256) of dev_pair.
int gram_windows_per_pass(int N);
int launch_gram_windows(const uint8_t *const *dev_tables, int N, uint64_t n_slice, const int *min_counts, const int *max_counts,
                        const int *out_index, int W, unsigned long long *dev_pair, hipStream_t s);

// gram_spectrum.hip -- joint count spectra: ADDS N*256 u64 value histograms, then N(N-1)/2 * 255 * 255 u64 joint bins for
// counts 1..255 (pairs i < j row-major), to dev_accum.  2 <= N <= 128.
// dev_tables is a HOST array of N device pointers; host_gtab / dev_gtab hold spectrum_groups(N) * 16 pointers (the tables of each
// pair group; the host one must stay valid until the stream has copied it).
int spectrum_groups(int N);
int launch_spectrum(const void *const *dev_tables, int N, uint64_t n_slice, unsigned long long *dev_accum, const uint8_t **host_gtab,
                    const uint8_t **dev_gtab, hipStream_t s);

// gram_occ.hip -- occupancy-stratified Gram products (kWIP): ADDS occ_hist[N+1], lin[N][N] ([o-1][i]) and gram[N][N(N+1)/2]
// ([o-1][pair i <= j, row-major]) u64 to dev_accum.  2 <= N <= 128.  dev_tables is a HOST array of N device pointers;
// dev_ptrs holds N device pointers (the occupancy pre-pass's list) and occ_scratch occgram_scratch_bytes(N, n_slice) bytes.
uint64_t occgram_scratch_bytes(int N, uint64_t n_slice);
int launch_occgram(const void *const *dev_tables, int N, uint64_t n_slice, unsigned long long *dev_accum, const uint8_t **dev_ptrs,
                   uint8_t *occ_scratch, hipStream_t s);

// gram_patterns.hip -- presence patterns: ADDS to dev_accum (2^N u64) the number of addresses per N-bit word "which tables
// hold the address with min_count <= count <= max_count" (bit t = table t).  1 <= N <= 16, 1 <= min <= max <= 255.
// dev_tables is a HOST array of N device pointers.
int launch_patterns(const void *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count, unsigned long long *dev_accum,
                    hipStream_t s);

// kmer_extract.hip -- the addresses that satisfy a presence / absence condition over N slices, and their count rows
// (DESIGN.md 4.11).  tables: device array of P present, then A absent table pointers (n_slice bytes each, 16-byte aligned).
// masks: extract_mask_words(n_slice) u16; wg: extract_workgroups(n_slice) + 1 u64, whose last word receives the number
// selected.  addr_out (u64) / counts_out (P bytes per row) are written only when that number is <= cap; cap = 0: count only.
uint32_t extract_workgroups(uint64_t n_slice);
uint64_t extract_mask_words(uint64_t n_slice);
int launch_extract(const uint8_t *const *dev_tables, int P, int A, uint64_t n_slice, uint64_t first_addr, int min_count, int max_count, int min_present,
                   int max_absent, uint16_t *masks, unsigned long long *wg, unsigned long long *addr_out, uint8_t *counts_out, uint64_t cap,
                   hipStream_t s);
// k_extract_scan alone: wg[0 .. n_wg) counts -> their exclusive prefix sums in place, wg[n_wg] = the total (kmer_unitig.hip's scans)
int launch_extract_scan(unsigned long long *wg, uint32_t n_wg, hipStream_t s);
// The same selection as a dense table: out[x] (n_slice bytes, 16-byte aligned, no input) = 0 where x is not selected, else
// the reduction `op` (TABLE_SUM .. TABLE_COUNT) over the present bytes inside the window; nothing at or beyond n_slice is
// written.  One launch, no scratch.
enum TableOp : int { TABLE_SUM = 0, TABLE_MIN = 1, TABLE_MAX = 2, TABLE_COUNT = 3 };
int launch_extract_table(const uint8_t *const *dev_tables, int P, int A, uint64_t n_slice, int min_count, int max_count, int min_present,
                         int max_absent, int op, uint8_t *table_out, hipStream_t s);
// m addresses -> m lines of k letters + '\n' (text 16-byte aligned)
int launch_extract_text(const unsigned long long *addr, uint64_t m, int k, uint8_t *text, hipStream_t s);

// kmer_select.hip -- the bytes of the kept records of a stream.  starts: R + 1 non-decreasing stream offsets,
// keep: R flags (device).  text[0 .. n) (16-byte aligned) is the stream from offset pos on; its bytes that lie in kept records
// go to out[0 .. expected), in order (any alignment) -- if they are exactly `expected` bytes, which the caller derives from the
// same two arrays; otherwise nothing is written.  masks: select_chunks(n) * 256 u64; sums: select_chunks(n) + 1 u64, whose
// last word receives the number of kept bytes, which is also added to *grand.  R = 0 or n = 0: nothing is launched.
uint32_t select_chunks(uint64_t n);
int launch_select(const unsigned long long *starts, const uint8_t *keep, uint64_t R, const uint8_t *text, uint64_t pos, uint64_t n,
                  unsigned long long *masks, unsigned long long *sums, unsigned long long *grand, uint8_t *out, uint64_t expected, hipStream_t s);

// kmer_trim.hip -- the longest covered stretch of every record of a FASTQ feed.  text[0 .. n) (device, any
// alignment) is the stream from offset pos on and holds R whole records, record r the bytes [starts[r], starts[r + 1]) of it
// (starts: R + 1 non-decreasing offsets <= n, device).  bits: n_words u32 of cover bits (bit g at word g / 32, bit g % 32);
// base: the valid bases of the stream before the feed; tq: the quality threshold byte, 0 = off.  cnt: R words, left holding
// every record's first bit; *total receives base + the feed's valid bases; geo: TRIM_FIELDS * R words, field f of record r at
// geo[f * R + r].  R = 0: nothing is launched.
constexpr uint32_t TRIM_FIELDS = 9;   // pos2, pos4, end2, end4, seq_len, trim_start, trim_end, covered, lead
int launch_trim(const uint8_t *text, const unsigned long long *starts, uint64_t R, uint64_t pos, uint32_t tq, const uint32_t *bits,
                uint64_t n_words, unsigned long long base, unsigned long long *cnt, unsigned long long *total, unsigned long long *geo,
                hipStream_t s);
// the first two kernels of launch_trim alone (R > 0): geo fields pos2, pos4, end2, end4, seq_len and lead, cnt and *total
void launch_trim_geometry(const uint8_t *text, const unsigned long long *starts, uint64_t R, uint64_t pos, uint32_t tq, unsigned long long base,
                          unsigned long long *cnt, unsigned long long *total, unsigned long long *geo, hipStream_t s);

// kmer_correct.hip -- single-base corrections of every record of a FASTQ feed.  text .. geo as launch_trim
// takes them (geo: TRIM_FIELDS * R words of scratch, of which the geometry fields are written).  tables[0 .. n_tab), n_tab <=
// QUERY_MAX_TABLES: device tables of 4^k bytes; a window matches iff min_count <= T[a] <= max_count in one of them.
// min_windows: a candidate with fewer windows is not tried.  text_out[0 .. n): a copy of text made by the caller on the same
// stream (it may not overlap text); the corrected bytes are patched into it.  out: CORR_FIELDS * R words, field f of record r
// at out[f * R + r].  R = 0: nothing is launched.
constexpr uint32_t CORR_FIELDS = 6;   // pos2, seq_len, candidates, untried, corrected, ambiguous
int launch_correct(const uint8_t *text, const unsigned long long *starts, uint64_t R, uint64_t pos, uint32_t tq, const uint32_t *bits,
                   uint64_t n_words, unsigned long long base, unsigned long long *cnt, unsigned long long *total, unsigned long long *geo,
                   uint32_t k, const uint8_t *const *tables, uint32_t n_tab, uint32_t min_count, uint32_t max_count, uint32_t min_windows,
                   uint8_t *text_out, unsigned long long *out, hipStream_t s);

// kmer_unitig.hip -- the unitigs of one table of n = 4^k bytes (16-byte aligned), k odd.  link: n bytes of
// scratch that hold one link byte per address from launch_unitig_links on.  totals: UT_WORDS words, zeroed by the caller
// before the links; UT_ERR != 0 afterwards: a walk met its step bound or an impossible link byte (which one: its value).
// A phase (mode UT_ENDS: the linear unitigs, then UT_LOOPS: the circular ones) is
//   launch_unitig_count    wg: unitig_workgroups(n) + 1 words; wg[last] receives the candidates m of the phase
//   launch_unitig_measure  (m > 0) cand, c_n, c_depth (m words) and c_keep (m bytes): the candidates, ascending, and what each
//                          owns; bound: the steps no walk can reach; wgA, wgB: unitig_rank_workgroups(m) + 1 words each, whose
//                          last words receive the phase's rows and the bytes of their records; row_base: the rows before
//   launch_unitig_spell    (rows > 0) the row arrays (rows words each) and the records, text_bytes of them
enum { UT_NODES = 0, UT_BRANCHING = 1, UT_SHORT = 2, UT_NODES_SHORT = 3, UT_LONGEST = 4, UT_ERR = 5, UT_WORDS = 8 };
enum { UT_ENDS = 0, UT_LOOPS = 1 };
uint32_t unitig_workgroups(uint64_t n);
uint32_t unitig_rank_workgroups(uint64_t m);
int launch_unitig_links(const uint8_t *table, uint64_t n, int k, int min_count, int max_count, uint8_t *link, unsigned long long *totals, hipStream_t s);
int launch_unitig_count(int mode, const uint8_t *link, uint64_t n, unsigned long long *wg, hipStream_t s);
int launch_unitig_measure(int mode, const uint8_t *table, uint8_t *link, uint64_t n, int k, int min_count, int max_count, const unsigned long long *wg,
                          unsigned long long *cand, uint64_t m, uint64_t bound, uint64_t min_kmers, unsigned long long *c_n, unsigned long long *c_depth,
                          uint8_t *c_keep, uint64_t row_base, unsigned long long *wgA, unsigned long long *wgB, unsigned long long *totals, hipStream_t s);
int launch_unitig_spell(const uint8_t *link, int k, const unsigned long long *cand, const uint8_t *c_keep, const unsigned long long *c_n,
                        const unsigned long long *c_depth, uint64_t m, const unsigned long long *wgA, const unsigned long long *wgB, uint64_t row_base,
                        uint64_t rows, unsigned long long *r_addr, unsigned long long *r_n, unsigned long long *r_depth, unsigned long long *r_off,
                        uint8_t *text, uint64_t text_bytes, unsigned long long *totals, hipStream_t s);
// The graph pass behind a build (no table): the edges between the written rows, then the GFA text.  UgRows: the row arrays
// and the FASTA text of the two phases as one array of `rows` rows, the first rows0 of them linear.  totals: the builder's;
// its words UG_DROPPED and UG_DEAD are zeroed by the caller before the count, checks 9 to 12 go to UT_ERR.
//   launch_unitig_edges_count  end_row: m words preset to ~0 (m: the ends of the linear phase, cand); wgE:
//                              unitig_rank_workgroups(2 * rows) + 1 words, whose last receives the edges E
//   launch_unitig_edges_fill   (E > 0) from, to (E words) and orient (E bytes)
//   launch_unitig_gfa_sizes    wgS: unitig_rank_workgroups(rows) + 1 words, wgL: unitig_rank_workgroups(E) + 1 words; their last
//                              words receive the bytes of the S-lines and of the L-lines
//   launch_unitig_gfa_write    gfa: UG_HEADER + S + L bytes; the header line is the caller's
enum { UG_DROPPED = 6, UG_DEAD = 7 };
enum { UG_HEADER = 11 };                         // "H\tVN:Z:1.0\n"
struct UgRows {
    const unsigned long long *n[2], *depth[2], *off[2];
    const uint8_t *text[2];
    uint64_t text_bytes[2];
    uint64_t rows0, rows;
};
int launch_unitig_edges_count(const UgRows &R, int k, const uint8_t *link, const unsigned long long *r_addr, const unsigned long long *cand, uint64_t m,
                              unsigned long long *end_row, unsigned long long *wgE, unsigned long long *totals, hipStream_t s);
int launch_unitig_edges_fill(const UgRows &R, int k, const uint8_t *link, const unsigned long long *cand, uint64_t m, const unsigned long long *end_row,
                             const unsigned long long *wgE, uint64_t n_edges, unsigned long long *from, unsigned long long *to, uint8_t *orient,
                             unsigned long long *totals, hipStream_t s);
int launch_unitig_gfa_sizes(const UgRows &R, int k, const unsigned long long *from, const unsigned long long *to, uint64_t n_edges,
                            unsigned long long *wgS, unsigned long long *wgL, hipStream_t s);
int launch_unitig_gfa_write(const UgRows &R, int k, const unsigned long long *from, const unsigned long long *to, const uint8_t *orient, uint64_t n_edges,
                            const unsigned long long *wgS, const unsigned long long *wgL, uint8_t *gfa, uint64_t gfa_bytes, unsigned long long *totals,
                            hipStream_t s);

}  // namespace pk
