/*
 * pykmer_hip.h -- C-ABI of libpykmer_hip.so, the MI355X (gfx950) engine behind pykmer's two hot loops.
 *
 * The reference (sauloal/pykmer) is monolithic Python with no FFI; the boundary sits where it hands
 * work to its hot loops.  Each entry point names the reference code it replaces
 * (file:line into the reference repository).  Plain pointers and sizes only; the caller owns every
 * host buffer; the library owns device memory.  All functions return PK_OK (0) or a negative
 * PK_ERR_* code; pk_last_error() returns the message of the calling thread's last failure.
 * Calls are blocking and may be issued concurrently for different devices.
 */
#ifndef PYKMER_HIP_H
#define PYKMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_ABI_VERSION 3

enum {
    PK_OK = 0,
    PK_ERR_ARG = -1,      /* even / non-positive / unsupported k, bad min/max count, null pointer */
    PK_ERR_HIP = -2,      /* HIP runtime failure (no device, out of memory, launch error)        */
    PK_ERR_RECS_CAP = -3, /* more records than recs_cap; *n_recs_out holds the number needed      */
    PK_ERR_STATE = -4,    /* handle used out of order                                            */
    PK_ERR_FORMAT = -5    /* malformed input (FASTQ); pk_last_error names the record and the rule  */
};

#define PK_FORMAT_FASTA 0
#define PK_FORMAT_FASTQ 1

/* One FASTA record as the reference's parse_fasta yields it (indexer.py:45-99). The caller slices the
 * header text out of its own buffer and drops records with n_valid_kmers == 0 to reproduce the
 * `chromosomes` list (indexer.py:349-351). Offsets are relative to the first byte ever fed. */
typedef struct pk_record {
    uint64_t name_off;      /* first byte after '>'                                             */
    uint64_t name_len;      /* header length after strip() (indexer.py:56,80)                   */
    uint64_t seq_len;       /* stripped sequence characters, valid or not (indexer.py:77,93)    */
    uint64_t n_valid_kmers; /* windows without a None (indexer.py:144)                          */
} pk_record;

int pk_version(void);
int pk_last_error(char *buf, size_t n);
int pk_device_count(void);
/* Optional: brings the HIP runtime up on `device` and loads the kernels, so that a command-line host can do this in a
 * thread while it still parses arguments and maps its input (about 0.2 s that pk_indexer_create / pk_gram* would
 * otherwise spend).  Has no reference counterpart: indexer.py / merger.py start no device. */
int pk_warm(int device);

/* ---- plain device buffers, so a host in any language can stage tables in HBM one at a time (a k=17
 * merge holds N x 16 GiB on the device, never on the host) and hand slices to pk_gram_device_partial. */
int pk_dev_alloc(void **dev_out, uint64_t n_bytes, int device);
int pk_dev_free(void *dev, int device);
int pk_dev_upload(void *dev_dst, const void *host_src, uint64_t n_bytes, int device);
int pk_dev_download(void *host_dst, const void *dev_src, uint64_t n_bytes, int device);
/* Free / total HBM on `device` in bytes: lets the host size how many table slices it stages beside each other. */
int pk_dev_mem_info(uint64_t *free_out, uint64_t *total_out, int device);

/* ---- indexer: replaces gen_kmers + canonical min + process_kmers (indexer.py:130-160, 341, 162-297)
 * and the parser that feeds them (indexer.py:45-99).  k must be odd (tools.py:165-167); 1 <= k <= 17 in one table,
 * k = 19 and 21 through pk_indexer_create_slice.
 *
 * fasta       uncompressed FASTA text (what gzip.open(...,'rt') would hand the reference)
 * table_out   4^k bytes (host); receives table[a] = min(255, #canonical k-mers with value a): the
 *             exact content of the reference's .kin file (tools.py:333-341, indexer.py:262)
 * hist256_out nullable; 256 counters, hist256[v] = #{a : table[a] == v}.  Header.update_stats
 *             (tools.py:246-263) follows from it: hist = hist256[1:], vals_sum = sum v*hist256[v] ...
 */
int pk_count_fasta(const uint8_t *fasta, uint64_t n_bytes, int k, uint8_t *table_out,
                   uint64_t *num_kmers_out, uint64_t *total_bp_out, uint64_t hist256_out[256],
                   pk_record *recs_out, uint64_t recs_cap, uint64_t *n_recs_out, int device);

/* pk_count_fasta keeps its indexer (table + workspace in HBM) for the next call with the same k and device;
 * this frees it. */
int pk_count_release(void);

/* Streaming / device-resident form of the same path (inputs larger than host RAM, inputs that
 * already live in HBM, repeated timing).  One indexer owns one 4^k table in HBM on one device. */
typedef struct pk_indexer pk_indexer;
int pk_indexer_create(pk_indexer **out, int k, int device);
/* Address-range-sharded form (every shard streams the whole text and keeps the canonical k-mers of its own
 * address range; no reduction, the shards' tables concatenate to the 4^k-byte .kin).  n_slices is a power of two; the
 * indexer's table is bytes [slice_index, slice_index + 1) * 4^k / n_slices of the .kin image, and a slice may hold at
 * most 2^34 addresses -- so k = 19 (256 GiB, never run by the reference: README.md:51-52) is 16 slices of 16 GiB,
 * on one GPU after another or spread over several.  num_kmers / total_bp / records describe the whole input whatever the
 * slice; hist256 describes the slice. */
int pk_indexer_create_slice(pk_indexer **out, int k, int device, int slice_index, int n_slices);
int pk_indexer_reset(pk_indexer *ix);                       /* zero the table, forget parser state  */
/* What the feeds hold: PK_FORMAT_FASTA (the default) or PK_FORMAT_FASTQ.  Set after create or reset, before the first
 * feed (PK_ERR_STATE otherwise); it persists across resets.  A FASTQ stream is counted exactly like the FASTA text it
 * stands for (README "FASTQ input": 4-line records, line 1 '@' -> '>', lines 3 and 4 dropped), converted on the device.
 * pk_record.name_off then points into the FASTQ bytes.  A malformed record fails the feed that completes it, or
 * pk_indexer_finish if the stream stops inside a record, with PK_ERR_FORMAT; pk_indexer_reset clears the error. */
int pk_indexer_set_format(pk_indexer *ix, int format);
/* FASTQ indexers: out = { records, lines, FASTQ bytes fed, FASTA bytes emitted to the counting pipeline }. */
int pk_indexer_fastq_stats(pk_indexer *ix, uint64_t out[4]);
/* Base qualities of a FASTQ indexer or query (README "Base quality"): threshold_byte T = Q + offset, 1 .. 255; 0 (the
 * default) is off.  Byte i of a record's line 2 counts as 'N' when byte i of its line 4 is < T as an unsigned byte, unless it
 * is one of the ten str.strip() blanks; nothing else of the stream changes (lengths, names, positions, the malformed-file
 * rules).  After pk_indexer_set_format(FASTQ) and before the first feed (PK_ERR_STATE otherwise; PK_ERR_ARG outside
 * 0 .. 255); it persists across resets, and setting the format back to FASTA turns it off.  The result does not depend on
 * how the stream is cut into feeds: the text of a record is held back on the device until its line 4 has gone by. */
int pk_indexer_set_min_qual(pk_indexer *ix, int threshold_byte);
/* FASTQ indexers: the line-2 bytes replaced so far (a low-quality 'N' counts too); 0 with the threshold off. */
int pk_indexer_fastq_masked(pk_indexer *ix, uint64_t *out);
/* Feed the next n_bytes of the FASTA text.  Chunks may split lines, records and k-mers anywhere.   */
int pk_indexer_feed(pk_indexer *ix, const uint8_t *host_fasta, uint64_t n_bytes);
/* Same, but the bytes already sit in device memory on the indexer's device (16-byte aligned).  Work runs on
 * the indexer's own stream; the call returns when the feed has been counted.  Any size: the library cuts the text into
 * pieces of at most 2 GiB (record positions inside one piece are 32-bit). */
int pk_indexer_feed_device(pk_indexer *ix, const void *dev_fasta, uint64_t n_bytes);
/* Close the last record and report the totals.  hist256_out[v] = number of table entries equal to v
 * (the histogram is kept in HBM while counting, so this makes no pass over the table).              */
int pk_indexer_finish(pk_indexer *ix, uint64_t *num_kmers_out, uint64_t *total_bp_out,
                      uint64_t hist256_out[256], uint64_t *n_recs_out);
int pk_indexer_records(pk_indexer *ix, pk_record *recs_out, uint64_t recs_cap);
int pk_indexer_table_to_host(pk_indexer *ix, uint8_t *table_out);
/* Table bytes [offset, offset + n_bytes) to the host: lets the caller take the .kin image in slices and hash / write
 * slice i while slice i+1 crosses PCIe (tools.py:280,283 hash the whole file afterwards). */
int pk_indexer_table_slice_to_host(pk_indexer *ix, uint8_t *dst, uint64_t offset, uint64_t n_bytes);
/* Device pointer of the finished u8 table (valid until reset/destroy) -- lets a merge run on tables
 * that never left HBM. */
int pk_indexer_table_device(pk_indexer *ix, const void **dev_table_out);
/* Copy table bytes [offset, offset+n_bytes) into another device buffer on the same device (keeps an
 * address-range slice for a sharded merge while the indexer goes on to the next sample). */
int pk_indexer_table_slice_to_device(pk_indexer *ix, void *dev_dst, uint64_t offset, uint64_t n_bytes);
/* Seconds spent since the last reset per stage, measured with HIP events on the indexer's stream:
 * [0] structure scans, [1] squeeze pass (text -> packed bases + record tallies), [2] finish, [3] reset,
 * [4] feeds (as a double), [5] everything between squeeze and bucket count (bucket layout, fused k-mer
 * assembly + level-1 sort, level 2), [6] bucket count + histogram rows + side list, [7] of [5]: the fused
 * k_walk_sort kernel alone, [8] how many feeds had to be laid out a second time with exact bucket sizes, [9] how many final buckets of a
 * sparse table were counted a second time because a byte counter wrapped (k_bucket_count_bytes). */
int pk_indexer_timings(pk_indexer *ix, double out[10]);
void pk_indexer_destroy(pk_indexer *ix);

/* ---- query: per-record k-mer hits of a FASTA / FASTQ text against N tables that lie in HBM (no reference counterpart:
 * README.md stops at the distance matrix).  Let record r, in file order, have the valid windows a_1 .. a_m (m = its
 * n_valid_kmers, canonical values as indexer.py:341 forms them).  For every record and table t
 *   hits[r][t]  = #{ j : min_count <= T_t[a_j] <= max_count }     (every window counts: a k-mer twice in r counts twice)
 *   depth[r][t] = sum of T_t[a_j] over the same j                 (the saturated table counts)
 * Records without a valid window are listed too, with zeros.
 *
 * pk_query_create makes an indexer in query mode: it parses and squeezes the text exactly like pk_indexer_create's, but
 * allocates no 4^k table and looks the k-mers up instead of counting them.  kmer_len odd, 1 <= k <= 17 (PK_ERR_ARG
 * otherwise).  set_format, feed, feed_device, finish, records, fastq_stats, reset and destroy work as for any indexer;
 * finish reports num_kmers, total_bp and the record count and zeroes a non-null hist256_out; the table accessors answer
 * PK_ERR_STATE.  pk_indexer_timings: [0] [1] [4] as above, [5] the seconds of the lookup kernels (window counts, ordinal
 * scan, gathers and tallies), [6] the seconds of the coordinate kernels (0 without pk_query_set_coords), [2] [3] as above,
 * the rest 0.
 * pk_query_set_tables: after create or reset and before the first feed (PK_ERR_STATE otherwise; a feed without tables is
 * PK_ERR_STATE too).  dev_tables are N >= 1 device buffers of 4^k bytes on the indexer's device; the caller owns them and
 * keeps them alive through the feeds.  They stay set across resets.  1 <= min_count <= max_count <= 255.  One lookup
 * launch serves 16 tables; more are looked up group by group inside the feed.
 * pk_query_results: after pk_indexer_finish.  hits_out / depth_out receive n_recs * N u64 each, row-major [r * N + t];
 * PK_ERR_RECS_CAP if the stream holds more than recs_cap records; PK_ERR_STATE when bins are on.
 *
 * Bins: the same tallies along each record, in bins of W valid windows.  Number the m valid windows of record r in text
 * order, j = 0 .. m-1; bin b of r holds the windows b*W <= j < min((b+1)*W, m), so r has ceil(m / W) bins, only its last
 * may hold fewer than W windows, and a record without a valid window has none.  The rows are ordered by record, then by
 * bin: record r's first row is bin_first[r] = sum of ceil(n_valid / W) over the records before r, r = 0 .. R, and
 * bin_first[R] is the number of rows.  hits and depth of a row are defined as above over the windows of that bin only.
 * Bins count valid windows, not bases: in a record without invalid characters window j begins at base j, but the window
 * numbering skips the gap of a run of N.
 * pk_query_set_bins: after pk_query_set_tables and before the first feed (PK_ERR_STATE otherwise).  bin_windows = W >= 1;
 * 0 = one row per record, the default, which a reset restores.  The accumulators are sized before every feed for the rows
 * the stream can hold by then, bytes_fed / W + the record capacity + 1; where they do not fit the device, the feed returns
 * an error whose message names W.
 * pk_query_bin_count: after pk_indexer_finish, the number of rows B.
 * pk_query_bin_results: after pk_indexer_finish.  hits_out / depth_out receive B * N u64 each, row-major [row * N + t];
 * bin_first_out receives R + 1 u64.  PK_ERR_RECS_CAP, with the needed numbers in the message, if B > bins_cap or
 * R > recs_cap; PK_ERR_STATE when bins are off.
 *
 * Coordinates: where a row lies on its record, in bases.  Positions are counted as seq_len counts them: within a record
 * every sequence character gets the next position, 0-based, valid base or not; blanks inside a sequence line get theirs once
 * a non-blank sequence character follows them on the same line; line terminators, the leading and trailing blanks of a line,
 * header text and text before the first header get none.  A record's positions are [0, seq_len); for FASTQ they are those
 * within the read (line 2).  A valid window is k consecutive positions.  For the row of record r and bin b,
 *   bin_start[row] = the position of the first base of window b*W of r
 *   bin_end[row]   = one past the position of the last base of window min((b+1)*W, m) - 1 of r
 * so 0 <= bin_start < bin_end <= seq_len[r], bin_end - bin_start >= (windows of the row) + k - 1 with equality exactly when
 * no invalid character lies inside the span, and bin_start grows strictly along a record.
 * pk_query_set_coords: after pk_query_set_bins with W > 0 and before the first feed (PK_ERR_STATE otherwise); on != 0 keeps
 * the coordinates, 0 (the default) does not.  The setting goes with the bins: a reset clears it with them, and so does a
 * later pk_query_set_bins.  The two arrays are sized with the accumulators (one u64 each per row) and fail the same way.
 * pk_query_bin_coords: after pk_indexer_finish.  start_out / end_out receive B u64 each, in row order.  PK_ERR_STATE when
 * coordinates are off; PK_ERR_RECS_CAP, with the needed number in the message, if B > bins_cap.
 *
 * Count spectra: per row (a record, or a bin when bins are on) and table, how many of the row's valid windows have each
 * table count,  spectrum[row][t][c] = #{ j : T_t[a_j] == c },  c = 0 .. 255, exact u64.  Absent k-mers are c = 0 and the
 * count window plays no part, so spectrum[row][t] sums to the row's windows, and hits and depth of ANY window [A, B] are
 * the sums of spectrum[c] and of c * spectrum[c] over c = A .. B.  The tally rides on the gathers of the lookup.
 * pk_query_set_spectrum: after pk_query_set_tables and before the first feed (PK_ERR_STATE otherwise), before or after
 * pk_query_set_bins; on != 0 keeps the spectra, 0 (the default, which a reset restores) does not.  The array takes
 * rows * N * 2 KiB of device memory beside hits and depth and is sized with them; where it does not fit, the call or the
 * feed returns an error whose message names the size and what reduces it.
 * pk_query_spectrum: after pk_indexer_finish.  out receives rows * N * 256 u64, [row][t][c]; rows are the records, or the
 * B bins in row order when bins are on.  PK_ERR_STATE when spectra are off; PK_ERR_RECS_CAP, with the needed number in the
 * message, if there are more rows than rows_cap.
 *
 * Shared windows: per row (a record, or a bin when bins are on) and pair of tables i < j, how many of the row's valid windows
 * lie in the count window of both,  shared[row][p] = #{ j : min <= T_i[a_j] <= max and min <= T_j[a_j] <= max },  exact u64;
 * p numbers the P = N (N - 1) / 2 pairs in row-major order: (0,1) (0,2) .. (0,N-1) (1,2) ..  The diagonal is hits[row][t].
 * The tally rides on the gathers of the lookup, which needs the tables of a pair in one launch: at most 16 tables.
 * pk_query_set_pairs: after pk_query_set_tables and before the first feed (PK_ERR_STATE otherwise), before or after
 * pk_query_set_bins; on != 0 keeps the shared windows, 0 (the default, which a reset restores) does not.  PK_ERR_ARG with
 * more than 16 tables, or while count spectra are on (the two are tallied in separate streams).  The array takes
 * rows * P * 8 bytes of device memory beside hits and depth and is sized with them; where it does not fit, the call or the
 * feed returns an error whose message names the size and what reduces it.
 * pk_query_pairs: after pk_indexer_finish.  out receives rows * P u64, [row][p]; rows are the records, or the B bins in row
 * order when bins are on.  PK_ERR_STATE when pairs are off; PK_ERR_RECS_CAP, with the needed number in the message, if
 * there are more rows than rows_cap.
 *
 * Covered bases: which bases of the text the tables explain, and the text with those bases marked (the `bbduk kmask` step).
 * A VALID BASE is a byte of ACGTacgt that is a sequence character of a record (text before the first header has none);
 * the valid bases of the stream are numbered g = 0, 1, .. in text order over all records and feeds.  A valid window MATCHES
 * iff min_count <= T_t[a] <= max_count in at least one table t, and a valid base is COVERED iff it lies in at least one
 * matching window.  Two phases, because a base at the end of a feed may be covered only by a window that ends in the next.
 * pk_query_set_cover: after pk_query_set_tables and before the first feed (PK_ERR_STATE otherwise); on != 0 keeps one cover
 * bit per valid base, 0 (the default, which a reset restores) does not.  With the bits on the feeds run the cover kernels
 * where they run the lookup: hits and depth stay zero, and bins, spectra and pairs do not go with it (PK_ERR_ARG).  The
 * bitmap takes one bit per byte fed and is sized before every feed.  pk_indexer_timings [5] holds the cover kernels' seconds.
 * pk_query_cover: after pk_indexer_finish.  *n_bases_out = the valid bases of the stream, B; bits_out receives
 * ceil(B / 8) bytes, bit g at byte g / 8, bit g % 8 (np.unpackbits(bitorder="little")).  PK_ERR_RECS_CAP, with
 * *n_bases_out set, if B > n_bits_cap; PK_ERR_STATE when the bits are off.
 * pk_query_set_mask: after create or reset and before the first feed (PK_ERR_STATE otherwise); it needs no tables.  bits
 * are n_bases cover bits in the layout above, from pk_query_cover or from anywhere; they are copied.  The SELECTED bases
 * are the valid bases whose bit is set, with PK_MASK_INVERT those whose bit is clear.  Every feed (FASTA only; at most one
 * piece, PK_FEED_PIECE bytes from the host and 1 GiB from the device, PK_ERR_ARG beyond) then leaves its text, byte for
 * byte and at the same length, with only the selected bytes changed: byte | 0x20 (lower case), with PK_MASK_HARD 'N'.
 * A reset ends the mode.  pk_indexer_timings [7] holds the apply kernel's seconds.
 * pk_query_mask_text: the last feed's patched bytes; *n_out = their number; PK_ERR_RECS_CAP if it exceeds cap.
 * pk_query_mask_counts: after pk_indexer_finish.  masked_out receives R u64, masked[r] = the selected bases of record r (a
 * base counts whether or not its byte changed); *n_bases_seen_out = the valid bases the stream held.  PK_ERR_STATE if that
 * is not the n_bases the mask was made for (the text changed between the phases); PK_ERR_RECS_CAP if R > recs_cap. */
enum { PK_MASK_HARD = 1, PK_MASK_INVERT = 2 };
/* Intervals of a mask stream.  POSITIONS are those of pk_query_set_coords: within a record every sequence character gets the
 * next position, 0-based, valid base or not; a blank inside a sequence line gets one once a non-blank sequence character
 * follows it on its line; line terminators, leading and trailing blanks, header text and text before the first header get
 * none.  An INTERVAL is a maximal run of consecutive positions of one record that all hold selected bases: (r, start, end),
 * half-open, 0 <= start < end <= seq_len[r].  An invalid character, an interior blank, a header, the end of the stream and
 * a valid base that is not selected end a run; line terminators and leading and trailing blanks do not.  The intervals are
 * in stream order (by record, then by start), those of a record never touch, and their lengths add up to masked[r].
 * pk_query_set_intervals: after pk_query_set_mask and before the first feed (PK_ERR_STATE otherwise); 0 is the default,
 * which a reset restores.  The rows grow with the intervals found; a growth that fails is PK_ERR_HIP naming the size.
 * pk_query_interval_count: after pk_indexer_finish; *n_out = the intervals of the stream, *seconds_out (may be null) = the
 * HIP-event seconds of the interval kernels, which are not part of pk_indexer_timings [7].
 * pk_query_intervals: after pk_indexer_finish; rec_out, start_out and end_out receive one u64 per interval.
 * PK_ERR_RECS_CAP if there are more than cap; PK_ERR_STATE when the intervals are off, or if the stream did not hold the
 * valid bases the mask was made for (as pk_query_mask_counts). */
int pk_query_set_intervals(pk_indexer *q, int on);
int pk_query_interval_count(pk_indexer *q, uint64_t *n_out, double *seconds_out);
int pk_query_intervals(pk_indexer *q, uint64_t *rec_out, uint64_t *start_out, uint64_t *end_out, uint64_t cap);
int pk_query_set_cover(pk_indexer *q, int on);
int pk_query_cover(pk_indexer *q, uint8_t *bits_out, uint64_t n_bits_cap, uint64_t *n_bases_out);
int pk_query_set_mask(pk_indexer *q, const uint8_t *bits, uint64_t n_bases, int mode);
int pk_query_mask_text(pk_indexer *q, uint8_t *host_out, uint64_t cap, uint64_t *n_out);
int pk_query_mask_counts(pk_indexer *q, uint64_t *masked_out, uint64_t recs_cap, uint64_t *n_bases_seen_out);
int pk_query_create(pk_indexer **out, int k, int device);
int pk_query_set_tables(pk_indexer *q, const void *const *dev_tables, int N, int min_count, int max_count);
int pk_query_results(pk_indexer *q, uint64_t *hits_out, uint64_t *depth_out, uint64_t recs_cap);
int pk_query_set_bins(pk_indexer *q, uint64_t bin_windows);
int pk_query_bin_count(pk_indexer *q, uint64_t *n_bins_out);
int pk_query_bin_results(pk_indexer *q, uint64_t *hits_out, uint64_t *depth_out, uint64_t *bin_first_out, uint64_t bins_cap,
                         uint64_t recs_cap);
int pk_query_set_coords(pk_indexer *q, int on);
int pk_query_bin_coords(pk_indexer *q, uint64_t *start_out, uint64_t *end_out, uint64_t bins_cap);
int pk_query_set_spectrum(pk_indexer *q, int on);
int pk_query_spectrum(pk_indexer *q, uint64_t *out, uint64_t rows_cap);
int pk_query_set_pairs(pk_indexer *q, int on);
int pk_query_pairs(pk_indexer *q, uint64_t *out, uint64_t rows_cap);

/* ---- stats: replaces Header.update_stats (tools.py:246-263) on a host table of n bytes. */
int pk_table_stats(const uint8_t *table, uint64_t n, uint64_t hist256_out[256], int device);

/* ---- merger: replaces Header.calculate_distance (tools.py:439-493) for every pair of merger.merge
 * (merger.py:139-176) in ONE pass over the N tables.
 *
 * tables      N host pointers to n-byte tables (n = 4^k, equal sizes: tools.py:444)
 * min/max     validity window, 1 <= min, max <= 255 (merger.py:90-91)
 * matrix_out  N*N*3 u64 row-major: [i][j] = (total_i, total_j, shared_ij) for i != j
 *             (merger.py:175-176); the diagonal, which the reference leaves unassigned
 *             (merger.py:136), is written as (0,0,0).
 * devices     n_devices device ordinals; the address range is split evenly across them and the
 *             partial matrices are summed on the host (single-process form).  The multi-process
 *             RCCL form uses pk_gram_device_partial on each rank's slice.
 */
int pk_gram(const uint8_t *const *tables, int N, uint64_t n, int min_count, int max_count,
            uint64_t *matrix_out, const int *devices, int n_devices);

/* Device-resident slice form: dev_tables[i] points at n_slice bytes of table i in HBM on `device`.
 * pair_out (host) receives N*N u64: [i][i] = total_i over the slice, [i][j] = shared_ij.  Summing
 * pair_out over disjoint slices (ranks) and expanding with pk_gram_expand gives matrix_out.
 * dev_pair_out (nullable, device, N*N u64) receives the same numbers in HBM for an RCCL all-reduce. */
int pk_gram_device_partial(const void *const *dev_tables, int N, uint64_t n_slice, int min_count,
                           int max_count, uint64_t *pair_out, void *dev_pair_out, int device,
                           double *kernel_seconds_out);
/* Same scan, but the tallies are ADDED to dev_pair_accum (device, N*N u64, zeroed by the caller before the
 * first slice): a rank whose share of the address range does not fit HBM beside N tables scans it in
 * sub-slices, and the accumulator is what the RCCL all-reduce sums across ranks (merger.py:163-178). */
int pk_gram_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, int min_count,
                              int max_count, void *dev_pair_accum, int device, double *kernel_seconds_out);
/* The same for n_windows validity windows at once (threshold sweeps: the reference re-runs the whole merge per
 * --min-count / --max-count, README.md:57-61; the compare itself is tools.py:473-475).  dev_pair_accum holds
 * n_windows x N x N u64, block w for (min_counts[w], max_counts[w]); the staged slices are streamed once per group of up
 * to eight windows (N <= 16; five for N <= 24, three for N <= 32, one beyond), not once per window. */
int pk_gram_device_accumulate_windows(const void *const *dev_tables, int N, uint64_t n_slice, const int *min_counts,
                                      const int *max_counts, int n_windows, void *dev_pair_accum, int device,
                                      double *kernel_seconds_out);
int pk_gram_expand(const uint64_t *pair, int N, uint64_t *matrix_out);

/* Joint count spectra of N device-resident slices, ADDED to dev_spec_accum (device, zeroed by the caller):
 * N*256 u64 value histograms, then N(N-1)/2 * 255 * 255 u64 joint bins for counts 1..255 (pairs i<j row-major).
 * hist[i][a] = #{x : c_i(x) = a}; joint bin [p][a-1][b-1] of pair p = (i, j) = #{x : c_i(x) = a, c_j(x) = b}, a, b >= 1.
 * Every --min-count / --max-count window of the pair tally (tools.py:473-482) is a box sum over a pair's spectrum, so one
 * pass answers the sweeps the reference runs as one whole merge per window (README.md:57-61); the row and column of
 * count 0 follow from the histograms.  2 <= N <= 128 (PK_ERR_ARG otherwise); beyond 16 tables the pairs are tallied in
 * groups, each streaming its tables again.  dev_spec_accum holds (N*256 + N(N-1)/2*65025) u64. */
int pk_spectrum_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice,
                                  void *dev_spec_accum, int device, double *kernel_seconds_out);

/* Occupancy-stratified Gram products of N device-resident slices (kWIP, Murray et al. 2017: the entropy weight of a k-mer
 * depends only on how many samples hold it), ADDED to dev_accum (device, zeroed by the caller).  With o(x) = #{i : c_i(x) >= 1}:
 *   occ_hist[N+1]        occ_hist[o] = #{x : o(x) = o}, o = 0..N
 *   lin[N][N]            lin[o-1][i] = sum_{x : o(x) = o} c_i(x)
 *   gram[N][N(N+1)/2]    gram[o-1][p] = sum_{x : o(x) = o} c_i(x) c_j(x), p = (i, j), i <= j, row-major upper triangle with the diagonal
 * all u64, in that order: (N + 1) + N*N + N*N(N+1)/2 words.  Any weighting over occupancy classes, and kWIP's kernel and
 * distance, follow on the host.  2 <= N <= 128 (PK_ERR_ARG otherwise); table pointers 16-byte aligned. */
int pk_occgram_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, void *dev_accum, int device,
                                 double *kernel_seconds_out);

/* Presence patterns of N device-resident slices: with m(x) = sum_t [min_count <= T_t[x] <= max_count] << t (bit t = table t
 * holds address x in the count window), patterns[p] = #{x : m(x) = p} for p = 0 .. 2^N - 1 is ADDED to dev_accum (device,
 * 2^N u64, zeroed by the caller; patterns[0] counts the addresses no table holds, so a pass adds n_slice in all).  Every
 * pair tally, occupancy class, intersection, union and difference of any subset of the tables is a sum over these bins.
 * 1 <= N <= 16, 1 <= min_count <= max_count <= 255, n_slice <= 2^40 (PK_ERR_ARG otherwise: the 2^N bins are a dense array);
 * table pointers 16-byte aligned.  N = 15 and 16 stream the slices 2 and 4 times. */
int pk_patterns_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count,
                                  void *dev_accum, int device, double *kernel_seconds_out);

/* ---- extract: the k-mers behind a condition over N device-resident slices (no reference counterpart: a `jellyfish dump`
 * / `kmc_tools` style answer).  dev_tables lists n_present "present" tables, then n_absent "absent" ones
 * (n_present >= 1, n_present + n_absent <= 128), each n_slice bytes whose first byte is address first_addr of the 4^k-byte
 * table; pointers 16-byte aligned.  With 1 <= min_count <= max_count <= 255, 1 <= min_present <= n_present and
 * 0 <= max_absent <= n_absent, for every address x of the slice
 *   p(x) = #{ i present : min_count <= T_i[x] <= max_count }   (the validity test of the pair tally, tools.py:473-475)
 *   q(x) = #{ j absent  : T_j[x] >= 1 }                        (held at any count: the window does not apply)
 * and x is selected iff p(x) >= min_present and q(x) <= max_absent.  *n_selected_out always receives the exact number of
 * selected addresses M of the slice.  If M <= cap, dev_addr_out (device, cap u64) receives the selected addresses
 * first_addr + offset in ascending order and dev_counts_out (device, cap * n_present bytes) row r = the raw bytes T_i[x_r] of
 * the present tables, in or out of the window; both 16-byte aligned.  If M > cap the call writes nothing to either array
 * and returns PK_ERR_RECS_CAP; cap = 0 with both arrays null asks for the count alone (PK_OK).  Bad arguments are
 * PK_ERR_ARG before anything is queued.  The call keeps one bit per address of the slice (plus 8 bytes per 16384
 * addresses) in HBM while it runs.
 * pk_extract_text: m addresses (device, u64) -> m lines of k letters and '\n' at dev_text_out (device, m * (k + 1) bytes,
 * 16-byte aligned): codes 0,1,2,3 = A,C,G,T, first base in the highest bits, the inverse of
 * the indexer's encoding (indexer.py:131: weight 4^(k-p-1) for base p; AAACC = 5); 1 <= k <= 32. */
int pk_extract_device(const void *const *dev_tables, int n_present, int n_absent, uint64_t n_slice, uint64_t first_addr,
                      int min_count, int max_count, int min_present, int max_absent,
                      void *dev_addr_out, void *dev_counts_out, uint64_t cap, uint64_t *n_selected_out,
                      int device, double *kernel_seconds_out);
int pk_extract_text(const void *dev_addr, uint64_t m, int k, void *dev_text_out, int device);

/* ---- extract, as a table: the same selection over the same slices, handed back dense -- one byte per address, which is
 * what a `.kin` holds, so the result can be fed to every tool that reads one (the `kmc_tools simple` / `jellyfish merge`
 * family: pooled, intersected, united and subtracted samples, occupancy).  Arguments and refusals as pk_extract_device;
 * with V(x) = { i present : min_count <= T_i[x] <= max_count }, so that p(x) = |V(x)|,
 *   out[x] = 0                               if x is not selected
 *   out[x] = min(255, sum_{i in V(x)} T_i[x])   op = PK_TABLE_SUM
 *            min_{i in V(x)} T_i[x]              op = PK_TABLE_MIN
 *            max_{i in V(x)} T_i[x]              op = PK_TABLE_MAX
 *            |V(x)|                              op = PK_TABLE_COUNT   (<= 128)
 * Only bytes inside the window take part (the count rows of pk_extract_device are raw bytes; these are not).  A selected
 * address has p >= min_present >= 1 and every byte of V is >= 1, so out[x] >= 1 exactly on the selected addresses, for
 * every op.  The saturating sum over the window 1-255 with min_present = 1 is the table of the pooled inputs, byte for
 * byte: min(255, sum min(255, c_i)) = min(255, sum c_i).
 * dev_table_out (device, n_slice bytes, 16-byte aligned, overlapping no input) receives out; no byte at or beyond n_slice
 * is written.  dev_hist_accum (device, 256 u64, required, zeroed by the caller before the first slice) has the number of
 * addresses with out[x] = v ADDED to word v for v = 1..255; word 0 is left alone (the zeros are the addresses less the
 * other 255 words, as pk_table_stats derives them), so the slices of a table sum.  A bad op, a null or misaligned output
 * and an output that overlaps an input are PK_ERR_ARG before anything is queued; n_slice = 0 is PK_OK and touches nothing. */
enum { PK_TABLE_SUM = 0, PK_TABLE_MIN = 1, PK_TABLE_MAX = 2, PK_TABLE_COUNT = 3 };
int pk_extract_table_device(const void *const *dev_tables, int n_present, int n_absent, uint64_t n_slice,
                            int min_count, int max_count, int min_present, int max_absent, int op,
                            void *dev_table_out, void *dev_hist_accum, int device, double *kernel_seconds_out);

/* ---- select: the bytes of a chosen subset of the records of a byte stream (no reference counterpart: the `bbduk` /
 * `kat filter seq` step behind a query).  No parser runs: the stream is cut into records by offsets the caller has, for a FASTA
 * or FASTQ file pk_record.name_off - 1 of every record and the length of the stream, so both formats are the same to it.
 * pk_select_create touches no device; the first pk_select_set_records with records brings it up.
 * pk_select_set_records: starts holds n_records + 1 non-decreasing stream offsets, counted from the first byte ever fed; record
 * r is the bytes [starts[r], starts[r + 1]), and keep[r] != 0 keeps it.  Bytes below starts[0] and at or beyond starts[R]
 * belong to no record and are never emitted; equal offsets make an empty record.  A decreasing list, or a null pointer with
 * n_records > 0, is PK_ERR_ARG; n_records = 0 is legal (starts and keep may then be null) and every feed emits nothing.
 * Before the first feed; after one it is PK_ERR_STATE, and so is a feed without records.  Both arrays are copied (to the
 * device, and the offsets with a prefix sum of the kept bytes on the host): the caller may free them.
 * pk_select_feed: the next n_bytes >= 0 of the stream, cut anywhere.  The feed that covers the stream offsets [a, a + n) writes
 * to host_out exactly the bytes at the offsets o of that range whose record is kept, in order, and their number to *n_out: the
 * outputs of the feeds, concatenated, are the kept records however the stream is cut.  out_cap >= n_bytes always suffices.
 * If the feed keeps more than out_cap bytes the call returns PK_ERR_RECS_CAP, *n_out holds the number needed, nothing is
 * written to the output and the stream does not move: the same feed may be sent again.  (The number follows from the
 * offsets alone, so the refusal costs no device work.)
 * pk_select_feed_device: the same with the text in device memory on the selector's device, 16-byte aligned as for
 * pk_indexer_feed_device, and the output in device memory at any alignment, overlapping no input (PK_ERR_ARG otherwise).
 * Both forms cut large feeds into pieces themselves.
 * pk_select_finish: totals_out = { bytes fed, bytes kept, records kept }; a kept record counts, once, when
 * starts[r] < min(bytes fed, starts[R]).  Feeds after it are PK_ERR_STATE.
 * pk_select_timings: out = { seconds of the select kernels so far, measured with HIP events on the selector's stream (the
 * copies of the host form are outside them), feeds (as a double) }. */
typedef struct pk_select pk_select;
int pk_select_create(pk_select **out, int device);
int pk_select_set_records(pk_select *s, const uint64_t *starts, const uint8_t *keep, uint64_t n_records);
int pk_select_feed(pk_select *s, const uint8_t *host_text, uint64_t n_bytes, uint8_t *host_out, uint64_t out_cap, uint64_t *n_out);
int pk_select_feed_device(pk_select *s, const void *dev_text, uint64_t n_bytes, void *dev_out, uint64_t out_cap, uint64_t *n_out);
int pk_select_finish(pk_select *s, uint64_t totals_out[3]);
int pk_select_timings(pk_select *s, double out[2]);
void pk_select_destroy(pk_select *s);

/* ---- trim: the longest covered stretch of every read of a FASTQ stream (no reference counterpart: the khmer `filter-abund` /
 * `bbduk ktrim` step behind a cover lookup).  No parser state and no tables: the trimmer is given the cover bits of the stream
 * (pk_query_cover of the same stream, or bits from anywhere) and the stream a second time, cut into WHOLE records by offsets
 * the caller has (pk_record.name_off - 1 and the length of the stream), and answers per record where lines 2 and 4 lie and
 * which of its positions to keep.  The stream has passed the FASTQ rules in the lookup; whatever the bytes are, no byte
 * outside a record's own range is read for it.
 * Positions, valid bases and covered bases are those of pk_query_set_cover and pk_query_set_coords on the FASTA text the
 * FASTQ stands for: line 2 is the record's one sequence line, position 0 its first non-blank byte, and every byte up to its last
 * non-blank one holds a position.  A valid base is a byte of ACGTacgt at a position, unless min_qual_byte = T > 0 and the
 * byte at the same offset of line 4 is below T as an unsigned byte (pk_indexer_set_min_qual's rule); the valid bases of the
 * stream are numbered in stream order and base g is covered iff bit g of the cover bits is set.  A run is a maximal stretch
 * of consecutive positions of one record that all hold covered bases.
 * pk_trim_create touches no device; pk_trim_set_cover brings it up.
 * pk_trim_set_cover: cover holds ceil(n_bases / 8) bytes, bit g at byte g / 8, bit g % 8 (as pk_query_cover packs them), copied
 * to the device; n_bases = 0 is legal (cover may then be null).  A null pointer with n_bases > 0 and a threshold outside 0 .. 255
 * are PK_ERR_ARG.  Before the first feed; after one it is PK_ERR_STATE, and so is a feed without it.
 * pk_trim_feed: the next n_bytes of the stream, which are n_records whole records: starts holds n_records + 1 non-decreasing
 * offsets relative to the feed, record r the bytes [starts[r], starts[r + 1]), and starts[n_records] = n_bytes.  out receives
 * PK_TRIM_FIELDS * n_records words, field f of record r at out[f * n_records + r]:
 *   PK_TRIM_POS2    the stream offset of the byte that holds position 0 of line 2 (PK_TRIM_END2 when the record has no position)
 *   PK_TRIM_POS4    the stream offset of the byte of line 4 at the same offset within its line
 *   PK_TRIM_END2    the stream offset where line 2's content ends and its terminator begins
 *   PK_TRIM_END4    the same for line 4, whose content is as long as line 2's
 *   PK_TRIM_SEQ_LEN the positions of the record
 *   PK_TRIM_START, PK_TRIM_END   its longest run, half-open and 0-based, among equals the one with the smallest start;
 *                   0 <= start <= end <= seq_len, and 0, 0 for a record without a covered base
 *   PK_TRIM_COVERED the covered bases of the record over all its runs
 *   PK_TRIM_LEAD    the blanks of line 2 in front of position 0: line 2 begins at PK_TRIM_POS2 - lead, line 4 at PK_TRIM_POS4 - lead
 * Non-monotone offsets, a last offset that is not n_bytes and null pointers with records present are PK_ERR_ARG, and then
 * nothing is launched and the stream does not move.  n_records = 0 launches nothing (starts may be null; the bytes, blank
 * lines at most, are counted as fed).
 * pk_trim_feed_device: the same with the text in device memory on the trimmer's device, at any alignment; starts and out stay
 * on the host.
 * pk_trim_finish: totals_out = { records seen, valid bases seen, covered bases }; PK_ERR_STATE, with the totals written, if
 * the valid bases seen are not n_bases -- the stream is not the one the bits were made for (the guard of
 * pk_query_mask_counts, and the check that this walker and the parser agree on what a valid base is).  Feeds after it are
 * PK_ERR_STATE.
 * pk_trim_timings: out = { seconds of the trim kernels so far, measured with HIP events on the trimmer's stream (the copies
 * are outside them), feeds (as a double) }. */
enum { PK_TRIM_POS2 = 0, PK_TRIM_POS4 = 1, PK_TRIM_END2 = 2, PK_TRIM_END4 = 3, PK_TRIM_SEQ_LEN = 4, PK_TRIM_START = 5, PK_TRIM_END = 6,
       PK_TRIM_COVERED = 7, PK_TRIM_LEAD = 8, PK_TRIM_FIELDS = 9 };
typedef struct pk_trim pk_trim;
int pk_trim_create(pk_trim **out, int device);
int pk_trim_set_cover(pk_trim *t, const uint8_t *cover, uint64_t n_bases, int min_qual_byte);
int pk_trim_feed(pk_trim *t, const uint8_t *host_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, uint64_t *out);
int pk_trim_feed_device(pk_trim *t, const void *dev_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, uint64_t *out);
int pk_trim_finish(pk_trim *t, uint64_t totals_out[3]);
int pk_trim_timings(pk_trim *t, double out[2]);
void pk_trim_destroy(pk_trim *t);

/* ---- correct: single-base corrections of the reads of a FASTQ stream (no reference counterpart: the step of Musket, Lighter,
 * BFC and `bbduk` / tadpole `ecc` behind a cover lookup).  Feeds, positions, valid bases, the threshold byte and the cover
 * bits are pk_trim's: the corrector is given the tables, the cover bits of the stream (pk_query_cover of the same stream
 * against the same tables, or bits from anywhere) and the stream a second time, cut into WHOLE records.
 * A valid run is a maximal stretch [lo, hi) of consecutive positions of one record that all hold valid bases.  Window s is
 * the positions [s, s + k); it is valid iff lo <= s and s + k <= hi for one valid run.  A window MATCHES iff at least one
 * table holds min_count <= T[a] <= max_count at its canonical address a.  A CANDIDATE is a position p that holds a valid base,
 * is not covered and lies in a valid run with hi - lo >= k; its windows are W(p) = { s : max(lo, p - k + 1) <= s <=
 * min(p, hi - k) }, w(p) = |W(p)| of them, 1 <= w(p) <= k.  A candidate is TRIED iff w(p) >= min_windows, UNTRIED otherwise.
 * A base b of A C G T other than the base at p (case ignored) PASSES iff every window of W(p) matches when read with b at p
 * and the read's own bases everywhere else.  A tried candidate is CORRECTED iff exactly one base passes, AMBIGUOUS iff two or
 * three pass, UNFIXABLE iff none does.  Every candidate is judged against the uncorrected read: the result depends neither
 * on the order of the positions, nor on how the stream is cut into feeds, nor on other corrections.  A corrected position's
 * byte becomes "ACGT"[b] | (old & 0x20); no other byte of the text changes.
 * pk_correct_create touches no device; k is odd and at most 17 (PK_ERR_ARG otherwise).
 * pk_correct_set_tables: N >= 1 (at most 16: one launch reads them all) device tables of 4^k bytes on the corrector's device,
 * owned by the caller and alive until the last feed, 1 <= min_count <= max_count <= 255; PK_ERR_ARG otherwise.  It brings the
 * device up.
 * pk_correct_set_cover: cover and n_bases as for pk_trim_set_cover (copied), min_qual_byte in 0 .. 255, min_windows in
 * 1 .. k; arguments out of range are PK_ERR_ARG.  It comes after the tables and before the first feed: PK_ERR_STATE out of
 * order, and so is a feed without it.
 * pk_correct_feed: text, starts and n_records as for pk_trim_feed.  host_text_out receives n_bytes bytes: the feed's text with
 * the corrected bytes patched in (it may be host_text itself).  out receives PK_CORR_FIELDS * n_records words, field f of
 * record r at out[f * n_records + r]:
 *   PK_CORR_POS2        the stream offset of the byte that holds position 0 of line 2 (as PK_TRIM_POS2)
 *   PK_CORR_SEQ_LEN     the positions of the record
 *   PK_CORR_CANDIDATES  its candidates; PK_CORR_UNTRIED, PK_CORR_CORRECTED, PK_CORR_AMBIGUOUS: those of each outcome; the
 *                       unfixable ones are the rest: candidates = untried + corrected + ambiguous + unfixable
 * The argument errors of pk_trim_feed, and a null text_out with bytes present, are PK_ERR_ARG; then nothing is launched and
 * the stream does not move.  n_records = 0 launches no kernel (the bytes are copied and counted as fed).
 * pk_correct_feed_device: the same with text and text_out in device memory on the corrector's device, at any alignment and
 * not overlapping (PK_ERR_ARG otherwise); starts and out stay on the host.
 * pk_correct_finish: totals_out = { records seen, valid bases seen, candidates, untried, corrected, ambiguous };
 * PK_ERR_STATE, with the totals written, if the valid bases seen are not n_bases.  Feeds after it are PK_ERR_STATE.
 * pk_correct_timings: out = { seconds of the correct kernels so far, measured with HIP events on the corrector's stream (the
 * copies are outside them), feeds (as a double) }. */
enum { PK_CORR_POS2 = 0, PK_CORR_SEQ_LEN = 1, PK_CORR_CANDIDATES = 2, PK_CORR_UNTRIED = 3, PK_CORR_CORRECTED = 4, PK_CORR_AMBIGUOUS = 5,
       PK_CORR_FIELDS = 6 };
typedef struct pk_correct pk_correct;
int pk_correct_create(pk_correct **out, int k, int device);
int pk_correct_set_tables(pk_correct *c, const void *const *dev_tables, int N, int min_count, int max_count);
int pk_correct_set_cover(pk_correct *c, const uint8_t *cover, uint64_t n_bases, int min_qual_byte, int min_windows);
int pk_correct_feed(pk_correct *c, const uint8_t *host_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records,
                    uint8_t *host_text_out, uint64_t *out);
int pk_correct_feed_device(pk_correct *c, const void *dev_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records,
                           void *dev_text_out, uint64_t *out);
int pk_correct_finish(pk_correct *c, uint64_t totals_out[6]);
int pk_correct_timings(pk_correct *c, double out[2]);
void pk_correct_destroy(pk_correct *c);

/* ---- unitigs: the compacted de Bruijn graph of ONE table, spelled as FASTA on the device (no reference counterpart: the
 * BCALM step behind a k-mer count).  Input: one table T of 4^k bytes, k odd, 1 <= k <= 17, and a count window
 * 1 <= min <= max <= 255.
 * NODE: a canonical address x with min <= T[x] <= max; S is the node set, n_nodes = |S|.
 * ORIENTED K-MER: any value o in [0, 4^k), codes A,C,G,T = 0..3, first base in the highest bits; rc(o) is its reverse
 * complement and canon(o) = min(o, rc(o)); k is odd, so o != rc(o) always.
 * EDGES: out(o) = { t = ((o << 2) | b) & (4^k - 1), b = 0..3 : canon(t) in S } and in(t) = { rc(u) : u in out(rc(t)) }.  Edges
 * are counted as strings: two successors that are each other's reverse complement count as two.
 * COMPACTABLE EDGE: o -> t is compactable iff |out(o)| = 1, |in(t)| = 1 and canon(o) != canon(t).  Self-loops such as poly-A,
 * and hairpins o -> rc(o), count in the degrees but are never compacted.  Compactable edges are symmetric (o -> t iff
 * rc(t) -> rc(o)), so they form a matching on (node, side), and every component is a simple path or a simple cycle that
 * meets each node once.
 * UNITIG: a maximal sequence o_1 -> ... -> o_n of compactable edges, n >= 1; every node lies in exactly one.  Its text is
 * the k letters of o_1 followed by the last letter of each o_i, i >= 2; its length is L = n + k - 1.
 * ORIENTATION AND ORDER: a linear unitig with n >= 2 has two different end nodes; it is spelled starting from the end node
 * with the smaller canonical address, leaving that node towards the rest, and first_addr is that address.  A single node is
 * spelled as its canonical k-mer, first_addr = x.  A cycle (circular = 1) starts at its smallest canonical address x_min,
 * spelled forward from the canonical string of x_min, and stops before returning to it: the text is linear, n + k - 1
 * letters, its last k - 1 letters overlap its start; first_addr = x_min.  The rows are all linear unitigs by ascending
 * first_addr, then all circular ones by ascending first_addr.
 * PER UNITIG: n_kmers = n, depth = the sum of T[x] over its nodes (u64), circular.
 * min_kmers M >= 1: unitigs with n_kmers < M are not written and get no row; n_short counts them and nodes_short their
 * nodes.  Row indices are those of the written rows.  A BRANCHING node has |out(o)| >= 2 for o = x or o = rc(x).
 * The FASTA text is, per row in row order, `>` + the row index in decimal + `\n` + the text + `\n`.
 * pk_unitig_create touches no device; k odd and at most 17, PK_ERR_ARG otherwise.
 * pk_unitig_build: dev_table is 4^k bytes on the builder's device, 16-byte aligned, owned by the caller and not changed; a
 * window or an M out of range is PK_ERR_ARG.  The library owns the link array (4^k bytes), the rows and the text; the rows and
 * the text are sized from what the passes count, and where they do not fit the device the call is PK_ERR_RECS_CAP with a
 * message that names the size.  Every walk carries a step bound that a correct walk cannot reach; PK_ERR_STATE if one is
 * reached.  totals_out = { nodes, branching nodes, linear rows, circular rows, n_short, nodes_short, FASTA bytes, the
 * largest n_kmers of a row }.  A builder may build again; the results are those of the last build.
 * pk_unitig_rows: the four row arrays, U = linear + circular rows each; PK_ERR_RECS_CAP if cap < U, PK_ERR_STATE before a
 * build.  pk_unitig_text: bytes [offset, offset + n_bytes) of the FASTA text; PK_ERR_ARG outside it.
 * pk_unitig_timings: out = { seconds of the link pass, of the linear phase (ends, measure, spell), of the circular phase --
 * HIP events on the builder's stream, the copies and allocations outside them --, builds (as a double) }.
 *
 * THE GRAPH of the last build (pk_unitig_graph; nothing of it is computed or reserved before that call).
 * ORIENTED ROW: let a written row r have the path o_1 -> ... -> o_n.  Its two oriented rows are (r,+) and (r,-).  (r,+) reads
 * the row's text as written: its first k-mer is tail(r,+) = o_1 and its last is head(r,+) = o_n.  (r,-) reads the reverse
 * complement of the text: tail(r,-) = rc(o_n) and head(r,-) = rc(o_1).  All 2U tails are different oriented k-mers.
 * EDGE: (r,s) -> (q,u) is an edge iff tail(q,u) is in out(head(r,s)), with out() as above.  Both rows must be written rows,
 * the overlap is always k - 1 bases, and nothing else is an edge.  What follows: for a linear row no edge out of head(r,s)
 * is compactable; every t in out(head(r,s)) is the tail of exactly one oriented unitig of the graph, which may be one that
 * min_kmers dropped; an edge whose target unitig was dropped is not written, and edges_dropped counts these; a circular row
 * c has exactly the two edges (c,+) -> (c,+) and (c,-) -> (c,-), its closing edge read both ways, and no other edge
 * touches it.
 * MIRROR: (r,s) -> (q,u) is an edge iff (q,~u) -> (r,~s) is, ~ flipping the sign.  Both are written, as BCALM's GFA
 * conversion writes them; an edge that is its own mirror, (r,+) -> (r,-) or (r,-) -> (r,+), a hairpin at a unitig end, is
 * written once.
 * ORDER: edges are ordered by the `from` row ascending, then + before -, then by the base b = 0..3 of the successor
 * ((head << 2) | b) & (4^k - 1).  One (row, sign, b) gives at most one edge, so the order is total; a row has at most 8
 * outgoing edges.
 * COUNT IDENTITY: at M = 1, n_edges = the sum over x in S of (|out(x)| + |out(rc(x))|) - 2 * the sum over the rows of
 * (n_kmers - 1), and edges_dropped = 0.
 * The GFA 1.0 text is `H\tVN:Z:1.0\n`, then per row in row order `S\t<row>\t<text>\tLN:i:<n+k-1>\tKC:i:<depth>\n`, then per
 * edge in edge order `L\t<from>\t<+|->\t<to>\t<+|->\t<k-1>M\n`.
 * pk_unitig_graph: totals_out = { n_edges, edges_dropped, n_dead_ends (the oriented rows without an outgoing written edge),
 * the bytes of the GFA text }.  PK_ERR_STATE before a build, and if a lane of the pass met what cannot be (a record beyond
 * its text, an end that no candidate holds, a line beyond its array); PK_ERR_RECS_CAP, with the size in the message, where
 * the device does not hold the end -> row map (8 bytes per end of a linear unitig), the edge arrays (17 bytes per edge) or
 * the GFA text.  pk_unitig_edges: from, to (E u64 each) and orient (E bytes: bit 0 set: the from side is -, bit 1 set: the
 * to side is -); PK_ERR_RECS_CAP if cap < E.  pk_unitig_gfa_text: bytes [offset, offset + n_bytes) of the GFA text;
 * PK_ERR_ARG outside it.  Both are PK_ERR_STATE before pk_unitig_graph, and again after a later pk_unitig_build until
 * pk_unitig_graph has run anew.  pk_unitig_graph_timings: out = { seconds of the edge passes (end map, count, scan, fill),
 * seconds of the GFA passes (sizes, scans, lines) } of the last pk_unitig_graph, HIP events as above.  Like
 * pk_unitig_timings it needs no build: before one, and before a pk_unitig_graph, it is PK_OK with two zeros. */
typedef struct pk_unitig pk_unitig;
int pk_unitig_create(pk_unitig **out, int k, int device);
int pk_unitig_build(pk_unitig *u, const void *dev_table, int min_count, int max_count, uint64_t min_kmers, uint64_t totals_out[8]);
int pk_unitig_rows(pk_unitig *u, uint64_t *first_addr, uint64_t *n_kmers, uint64_t *depth, uint8_t *circular, uint64_t cap);
int pk_unitig_text(pk_unitig *u, uint8_t *host_out, uint64_t offset, uint64_t n_bytes);
int pk_unitig_timings(pk_unitig *u, double out[4]);
int pk_unitig_graph(pk_unitig *u, uint64_t totals_out[4]);
int pk_unitig_edges(pk_unitig *u, uint64_t *from, uint64_t *to, uint8_t *orient, uint64_t cap);
int pk_unitig_gfa_text(pk_unitig *u, uint8_t *host_out, uint64_t offset, uint64_t n_bytes);
int pk_unitig_graph_timings(pk_unitig *u, double out[2]);
void pk_unitig_destroy(pk_unitig *u);

/* ---- BGZF on the host (no device work): the reference reads `.kin.bgz` tables and `.fa.gz` / `.bgz` inputs through one
 * Python gzip.open stream (tools.py:294-305, indexer.py:112-115); bgzip output (README.md:26) is a series of independent
 * gzip members, inflated here block-parallel on native threads straight into the caller's buffer.
 * pk_bgzf_scan: walks the member headers of `src` (no inflation): offset, size and ISIZE of each; PK_ERR_ARG if the
 * bytes are not BGZF; PK_ERR_RECS_CAP if more than `cap` blocks (*n_blocks_out = the count; call again with room).
 * pk_bgzf_inflate: block i (c_off[i], c_size[i]) -> dst + u_off[i], u_off[i + 1] - u_off[i] bytes (u_off has n_blocks + 1
 * entries); the block list is checked against src_bytes (it may come from a `.gzi` file), CRC32 and ISIZE of every
 * block against its payload (SAM spec 4.1). */
int pk_bgzf_scan(const uint8_t *src, uint64_t n_bytes, uint64_t cap, uint64_t *c_off_out, uint64_t *c_size_out,
                 uint64_t *isize_out, uint64_t *n_blocks_out);
int pk_bgzf_inflate(const uint8_t *src, uint64_t src_bytes, const uint64_t *c_off, const uint64_t *c_size,
                    const uint64_t *u_off, uint64_t n_blocks, uint8_t *dst, int threads);
/* The writer (the README's `bgzip -i -I x.gzi -l 9 -c x > x.bgz` step, README.md:26): every block_input (<= 0xff00) bytes
 * of src become one BGZF block, deflated on native threads; dst needs 65536 bytes per block, the blocks end up back to
 * back in its first *total_out bytes (no end-of-file block), c_sizes_out[i] = size of block i (the `.gzi` follows). */
int pk_bgzf_deflate(const uint8_t *src, uint64_t n_bytes, int level, uint32_t block_input, uint8_t *dst, uint64_t dst_cap,
                    uint64_t *c_sizes_out, uint64_t *total_out, int threads);

/* ---- diagnostics (tools/, tests/): no reference counterpart, no effect on any result.
 * pk_diag_occupancy: workgroups per CU the runtime grants kernel `which` (0 k_bucket_count, 1 k_bucket_count_bytes,
 * 2 k_bucket_count_half_lean, 3 k_scatter2), each at the dynamic LDS size it is launched with; negative = HIP error.
 * pk_diag_plan: the partition plan of ONE feed of n_bytes (0 = the largest piece a feed is cut into) at kmer_len k:
 * out = { largest piece, level-1 record capacity, final-bucket record capacity, level-1 buckets, level-2 digits,
 * address bits per final bucket, 16 KiB chunks, 1 if every record position fits 32 bits }.
 * pk_diag_plan_slice: the same feed into ONE of n_slices address slices (what pk_indexer_create_slice accepts, refused
 * alike), with every choice the launchers make from it; touches no GPU:
 * out = { addr_bits, fb_bits, b1, b2, sample_stride (16: sampled layout, 1: exact), n_tally (buckets tallied while
 * sampling), sample2, n_chunks, walk-sort variant (0 narrow, 1 narrow sliced, 2 k15, 3 k17, 4 wide sliced, 5 deep),
 * bucket-count kernel (0 whole, 1 bytes, 2 half), bucket split, B1, B2, level-1 record capacity, final-bucket record
 * capacity, 1 if every record position fits 32 bits }.
 * pk_diag_settled_chunks: how many 16 KiB chunks of the indexer's last feed the structure pass squeezed itself (full chunks
 * of plain sequence text that are not entered inside a header line; the squeeze pass only completes those); 0 for a query
 * indexer and before the first feed.  Copies one small record per chunk from the device.
 * pk_diag_level2_order: the order in which the level-2 sort walks B1 level-1 buckets of the given sizes (B1 a multiple of
 * 8, 8 .. 512): buckets ranked by size, descending, ties by lower index; rank r is dealt to round r / 8 and to XCD class
 * r % 8 in even rounds, 7 - r % 8 in odd ones; order_out[class * (B1 / 8) + round] = bucket.  The device computes its order
 * with the same code; touches no GPU. */
int pk_diag_occupancy(int which);
int pk_diag_plan(int k, uint64_t n_bytes, uint64_t out[8]);
int pk_diag_settled_chunks(pk_indexer *ix, uint64_t *out);
int pk_diag_plan_slice(int k, int n_slices, uint64_t n_bytes, uint64_t out[16]);
int pk_diag_level2_order(const uint32_t *sizes, uint32_t B1, uint32_t *order_out);

#ifdef __cplusplus
}
#endif
#endif /* PYKMER_HIP_H */
