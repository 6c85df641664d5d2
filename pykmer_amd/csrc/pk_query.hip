// pk_query.hip -- query mode of the host layer: the state a query indexer holds (QueryState, pk_host.h) and the
// pk_query_* entry points.  The feeds themselves go through pk_indexer.hip, which queues the kernels of kmer_query.hip and
// kmer_coords.hip behind the squeeze.
#include "pk_host.h"

using namespace pk;

int QueryState::create() {
    for (hipEvent_t *e : {&lookup_begin, &lookup_end, &coords_begin, &coords_end, &mask_begin, &mask_end}) HIPCHK(hipEventCreate(e));
    return P.reserve(4096 * sizeof(unsigned long long));
}

int QueryState::reset(hipStream_t s) {
    for (DevBuf<unsigned long long> *b : {&P, &Bf, &hits, &depth, &bin_start, &bin_end, &pos, &spec, &shared, &nb, &masked})
        if (b->p) HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, s));
    if (cover_bits.p) HIPCHK(hipMemsetAsync(cover_bits.p, 0, cover_bits.bytes, s));
    windows = p_done = 0;
    bin = n_bins = 0;
    spectrum = false;
    pairs = false;
    coords = false; pos_in = 0; t_coords = 0;
    cover = apply = false; nb_in = 0; t_mask = 0;
    mask_n_bases = mask_out_n = 0; mask_mode = 0;
    return PK_OK;
}

// Covered bases: one bit per valid base, and a stream of `bytes` bytes holds at most as many; one word in front of the
// first base's is never written, one behind the last takes the read of a lane's third word.  Contents kept, the rest zero;
// it grows by half at least, so that a long stream does not move it with every feed.
int QueryState::ensure_cover(uint64_t bytes, hipStream_t s) {
    if (!cover) return PK_OK;
    const size_t need = (bytes / 32 + 2) * sizeof(uint32_t);
    if (need <= cover_bits.bytes) return PK_OK;
    return cover_bits.grow_keep(std::max<size_t>(need, cover_bits.bytes + cover_bits.bytes / 2), s);
}

// the window prefix and the accumulators grow with the record array and keep what they hold; binned, the rows are sized
// again for the `bytes` of the stream, the feed under way included
int QueryState::grow_with_recs(uint64_t cap, uint64_t bytes, hipStream_t s) {
    const size_t row = tables.size() * sizeof(unsigned long long);
    int rc = P.grow_keep(cap * sizeof(unsigned long long), s);
    if (rc) return rc;
    if (bin) {
        if ((rc = Bf.grow_keep(cap * sizeof(unsigned long long), s))) return rc;
        if ((rc = ensure_rows(cap, bytes, s))) return rc;
    } else {
        if ((rc = hits.grow_keep(cap * row, s))) return rc;
        if ((rc = depth.grow_keep(cap * row, s))) return rc;
    }
    if ((rc = ensure_spectrum(cap, bytes, s))) return rc;
    if (apply && (rc = masked.grow_keep(cap * sizeof(unsigned long long), s))) return rc;
    return ensure_pairs(cap, bytes, s);
}

// Shared windows: one u64 per pair of tables for every row hits and depth have (per record: `cap` rows; binned: those of
// ensure_rows), contents kept, the rest zero.  Binned they grow by half at least, as the rows of hits do.  An array that does
// not fit is an error that names its size and what makes it smaller.
int QueryState::ensure_pairs(uint64_t cap, uint64_t bytes, hipStream_t s) {
    if (!pairs || n_pairs() == 0) return PK_OK;
    const uint64_t rows = bin ? bytes / bin + cap + 1 : cap;
    const size_t N = tables.size(), per_row = n_pairs() * sizeof(unsigned long long);
    const char *helps = "take fewer tables per run, larger bins or a smaller query";
    if (rows > SIZE_MAX / 2 / per_row)
        return fail(PK_ERR_ARG, "shared windows of %llu rows and %zu pairs of tables are beyond the address space; %s", (unsigned long long)rows,
                    n_pairs(), helps);
    if (rows * per_row <= shared.bytes) return PK_OK;
    const size_t want = bin ? std::max<size_t>(rows * per_row, shared.bytes + shared.bytes / 2) : rows * per_row;
    const int rc = shared.grow_keep(want, s);
    if (!rc) return PK_OK;
    (void)hipGetLastError();
    const std::string why = g_err;
    return fail(rc, "shared windows need an accumulator of %zu bytes (%llu rows, %zu tables, %zu pairs of 8 bytes each); %s: %s", want,
                (unsigned long long)rows, N, n_pairs(), helps, why.c_str());
}

// Count spectra: 256 u64 per table for every row hits and depth have (per record: `cap` rows; binned: those of ensure_rows),
// contents kept, the rest zero.  They grow to exactly what is needed: 256 times the size of hits, the old and the new array
// side by side are what the device has to hold, and a copy at HBM speed per feed is cheap beside the lookups.  An array that
// does not fit is an error that names its size and what makes it smaller.
int QueryState::ensure_spectrum(uint64_t cap, uint64_t bytes, hipStream_t s) {
    if (!spectrum) return PK_OK;
    const uint64_t rows = bin ? bytes / bin + cap + 1 : cap;
    const size_t N = tables.size(), per_row = N * 256 * sizeof(unsigned long long);
    const char *helps = "take fewer tables per run, larger bins or a smaller query";
    if (rows > SIZE_MAX / 2 / per_row)
        return fail(PK_ERR_ARG, "count spectra of %llu rows and %zu tables (2 KiB each) are beyond the address space; %s", (unsigned long long)rows, N,
                    helps);
    if (rows * per_row <= spec.bytes) return PK_OK;
    const size_t want = rows * per_row;
    const int rc = spec.grow_keep(want, s);
    if (!rc) return PK_OK;
    (void)hipGetLastError();
    const std::string why = g_err;
    return fail(rc, "count spectra need an accumulator of %zu bytes (%llu rows, %zu tables, 2 KiB each); %s: %s", want, (unsigned long long)rows, N, helps,
                why.c_str());
}

// Binned query: the accumulators, and with coordinates their two arrays, hold the rows that `bytes` bytes of stream and
// `cap` records can make (contents kept, the rest zero).  They grow by half at least, so that a long stream does not move
// them with every feed.
int QueryState::ensure_rows(uint64_t cap, uint64_t bytes, hipStream_t s) {
    if (!bin) return PK_OK;
    const uint64_t rows = bytes / bin + cap + 1;
    const size_t word = sizeof(unsigned long long), N = tables.size();
    if (rows > SIZE_MAX / 2 / (N * word))
        return fail(PK_ERR_ARG, "bins of %llu windows: %llu rows of %zu tables are beyond the address space; take larger bins",
                    (unsigned long long)bin, (unsigned long long)rows, N);
    auto grow = [&](DevBuf<unsigned long long> *a, DevBuf<unsigned long long> *b, size_t row, const char *noun, const char *shape) -> int {
        for (DevBuf<unsigned long long> *buf : {a, b}) {
            if (rows * row <= buf->bytes) continue;
            const size_t want = std::max<size_t>(rows * row, buf->bytes + buf->bytes / 2);
            const int rc = buf->grow_keep(want, s);
            if (rc) {
                (void)hipGetLastError();
                const std::string why = g_err;
                return fail(rc, "bins of %llu windows need two %s of %zu bytes (%s); take larger bins: %s", (unsigned long long)bin, noun, want, shape,
                            why.c_str());
            }
        }
        return PK_OK;
    };
    char shape[64];                                          // of the arrays, for the refusal
    snprintf(shape, sizeof shape, "%llu rows, %zu tables", (unsigned long long)rows, N);
    const int rc = grow(&hits, &depth, N * word, "accumulators", shape);
    if (rc || !coords) return rc;
    snprintf(shape, sizeof shape, "%llu rows", (unsigned long long)rows);
    return grow(&bin_start, &bin_end, word, "coordinate arrays", shape);
}

// The opening checks of the pk_query_* entry points, in the order that decides which message a caller sees: a query
// indexer; the entry point's own demand on the tables, bins or coordinates (`met`, null for none; `unmet` says what is
// missing); then either nothing fed yet (`too_late` is the refusal of a setting) or, without one, a finished stream.
static int query_check(pk_indexer *ix, bool (*met)(const QueryState &), const char *unmet, const char *too_late) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->q) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (met && !met(*ix->q)) return fail(PK_ERR_STATE, "%s", unmet);
    if (too_late && (ix->fed || ix->finished)) return fail(PK_ERR_STATE, "%s", too_late);
    if (!too_late && !ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    return PK_OK;
}
static bool has_tables(const QueryState &q) { return !q.tables.empty(); }
static bool binned(const QueryState &q) { return q.bin != 0; }
static bool per_record(const QueryState &q) { return q.bin == 0; }
static bool with_coords(const QueryState &q) { return q.coords; }
static bool with_spectrum(const QueryState &q) { return q.spectrum; }
static bool with_pairs(const QueryState &q) { return q.pairs; }

extern "C" int pk_query_create(pk_indexer **out, int k, int device) {
    if (k > 17) return fail(PK_ERR_ARG, "a query takes kmer_len <= 17 (one unsliced table), got %d", k);
    return create_indexer(out, k, device, 0, 1, true);
}

extern "C" int pk_query_set_tables(pk_indexer *ix, const void *const *dev_tables, int N, int min_count, int max_count) {
    if (int rc = query_check(ix, nullptr, nullptr, "the tables are set before the first feed (reset the indexer first)")) return rc;
    if (N < 1 || !dev_tables) return fail(PK_ERR_ARG, "need at least one table");
    if (min_count < 1 || max_count > 255 || min_count > max_count) return fail(PK_ERR_ARG, "count window must satisfy 1 <= min <= max <= 255, got %d-%d", min_count, max_count);
    for (int i = 0; i < N; i++)
        if (!dev_tables[i]) return fail(PK_ERR_ARG, "table %d is a null pointer", i);
    if (ix->q->pairs && N > (int)QUERY_MAX_TABLES)
        return fail(PK_ERR_ARG, "shared windows (pk_query_set_pairs) take at most %u tables, all in one lookup; got %d", QUERY_MAX_TABLES, N);
    HIPCHK(hipSetDevice(ix->device));
    QueryState &q = *ix->q;
    q.tables.assign((const uint8_t *const *)dev_tables, (const uint8_t *const *)dev_tables + N);
    q.min = min_count; q.max = max_count;
    // the accumulators of an empty stream for this many tables (a reset zeroed them, but N may have changed)
    const size_t need = ix->recs_cap() * (size_t)N * sizeof(unsigned long long);
    for (DevBuf<unsigned long long> *b : {&q.hits, &q.depth}) {
        int rc = b->reserve(need);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, ix->stream));
    }
    if (int rc = q.ensure_spectrum(ix->recs_cap(), 0, ix->stream)) return rc;   // (all zero before the first feed, whatever N was)
    return q.ensure_pairs(ix->recs_cap(), 0, ix->stream);
}

extern "C" int pk_query_set_bins(pk_indexer *ix, uint64_t bin_windows) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_bins", "the bins are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    QueryState &q = *ix->q;
    q.bin = bin_windows;
    q.coords = false;                                        // pk_query_set_coords comes after the bins
    int rc = PK_OK;
    if (bin_windows) {
        // Bf beside P; a reset zeroed what was there, a new array is zeroed here
        rc = q.Bf.grow_keep(ix->recs_cap() * sizeof(unsigned long long), ix->stream);
        if (rc || (rc = q.ensure_rows(ix->recs_cap(), 0, ix->stream))) return rc;
    }
    if ((rc = q.ensure_spectrum(ix->recs_cap(), 0, ix->stream))) return rc;
    return q.ensure_pairs(ix->recs_cap(), 0, ix->stream);
}

extern "C" int pk_query_set_spectrum(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_spectrum", "the spectra are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    QueryState &q = *ix->q;
    if (on && q.pairs) return fail(PK_ERR_ARG, "count spectra and shared windows (pk_query_set_pairs) are tallied in separate streams");
    q.spectrum = on != 0;
    // a reset zeroed what was there, a new array is zeroed here; per record or for the bins set so far
    const int rc = q.ensure_spectrum(ix->recs_cap(), 0, ix->stream);
    if (rc) q.spectrum = false;                              // an array that did not fit: the setting did not take
    return rc;
}

extern "C" int pk_query_set_pairs(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_pairs", "the pairs are set before the first feed (reset the indexer first)")) return rc;
    QueryState &q = *ix->q;
    if (on && q.tables.size() > QUERY_MAX_TABLES)
        return fail(PK_ERR_ARG, "shared windows take at most %u tables, all in one lookup; the indexer has %zu", QUERY_MAX_TABLES, q.tables.size());
    if (on && q.spectrum) return fail(PK_ERR_ARG, "shared windows and count spectra (pk_query_set_spectrum) are tallied in separate streams");
    HIPCHK(hipSetDevice(ix->device));
    q.pairs = on != 0;
    // a reset zeroed what was there, a new array is zeroed here; per record or for the bins set so far
    const int rc = q.ensure_pairs(ix->recs_cap(), 0, ix->stream);
    if (rc) q.pairs = false;                                 // an array that did not fit: the setting did not take
    return rc;
}

extern "C" int pk_query_set_coords(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, binned, "pk_query_set_bins with bins of at least one window comes before pk_query_set_coords", "the coordinates are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    QueryState &q = *ix->q;
    q.coords = on != 0;
    if (!q.coords) return PK_OK;
    // the two position words; a reset zeroed what was there, a new array is zeroed here
    const int rc = q.pos.grow_keep(2 * sizeof(unsigned long long), ix->stream);
    return rc ? rc : q.ensure_rows(ix->recs_cap(), 0, ix->stream);
}

// the two base-count words; a reset zeroed what was there, a new array is zeroed here
static int cover_words_ready(pk_indexer *ix) { return ix->q->nb.grow_keep(2 * sizeof(unsigned long long), ix->stream); }

extern "C" int pk_query_set_cover(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_cover", "the cover bits are set before the first feed (reset the indexer first)")) return rc;
    QueryState &q = *ix->q;
    if (on && (q.bin || q.spectrum || q.pairs))
        return fail(PK_ERR_ARG, "the cover bits take the place of the tallies: bins, count spectra and shared windows belong to a stream of their own");
    if (on && q.apply) return fail(PK_ERR_ARG, "the indexer applies a mask (pk_query_set_mask); the cover bits come from a stream of their own");
    HIPCHK(hipSetDevice(ix->device));
    q.cover = on != 0;
    if (!q.cover) return PK_OK;
    int rc = cover_words_ready(ix);
    if (!rc) rc = q.ensure_cover(0, ix->stream);
    if (rc) q.cover = false;                                 // an array that did not fit: the setting did not take
    return rc;
}

// the valid bases of the stream so far, as the last settled feed left them (after a wait on the stream)
static int bases_seen(pk_indexer *ix, uint64_t *out) {
    *out = 0;
    if (!ix->q->nb.p) return PK_OK;
    unsigned long long n = 0;
    HIPCHK(hipMemcpy(&n, ix->q->nb.p + ix->q->nb_in, sizeof n, hipMemcpyDeviceToHost));
    *out = n;
    return PK_OK;
}

static bool with_cover(const QueryState &q) { return q.cover; }
static bool applying(const QueryState &q) { return q.apply; }

extern "C" int pk_query_cover(pk_indexer *ix, uint8_t *bits_out, uint64_t n_bits_cap, uint64_t *n_bases_out) {
    if (int rc = query_check(ix, with_cover, "the indexer keeps no cover bits (pk_query_set_cover)", nullptr)) return rc;
    if (!n_bases_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    const QueryState &q = *ix->q;
    if (int rc = bases_seen(ix, n_bases_out)) return rc;
    const uint64_t n = *n_bases_out;
    if (n > n_bits_cap) return fail(PK_ERR_RECS_CAP, "%llu valid bases, capacity %llu bits", (unsigned long long)n, (unsigned long long)n_bits_cap);
    if (n == 0) return PK_OK;
    if (!bits_out) return fail(PK_ERR_ARG, "null output pointer");
    if ((n + 7) / 8 > q.cover_bits.bytes) return fail(PK_ERR_HIP, "cover bitmap smaller than the stream (internal error)");
    HIPCHK(hipMemcpy(bits_out, q.cover_bits.p, (n + 7) / 8, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_set_mask(pk_indexer *ix, const uint8_t *bits, uint64_t n_bases, int mode) {
    if (int rc = query_check(ix, nullptr, nullptr, "the mask is set before the first feed (reset the indexer first)")) return rc;
    if (mode < 0 || mode > (PK_MASK_HARD | PK_MASK_INVERT)) return fail(PK_ERR_ARG, "unknown mask mode %d", mode);
    if (n_bases && !bits) return fail(PK_ERR_ARG, "null bitmap for %llu bases", (unsigned long long)n_bases);
    QueryState &q = *ix->q;
    if (q.cover) return fail(PK_ERR_ARG, "the indexer keeps cover bits (pk_query_set_cover); a mask is applied in a stream of its own");
    if (ix->format != PK_FORMAT_FASTA) return fail(PK_ERR_ARG, "a mask is applied to FASTA text only");
    HIPCHK(hipSetDevice(ix->device));
    int rc = cover_words_ready(ix);
    if (rc) return rc;
    // whole words, zero behind the last base; one more for the read of a lane's third word
    const size_t words = n_bases / 32 + 2;
    if ((rc = q.mask_bits.reserve(words * sizeof(uint32_t)))) return rc;
    HIPCHK(hipMemsetAsync(q.mask_bits.p, 0, q.mask_bits.bytes, ix->stream));
    if (n_bases) HIPCHK(hipMemcpyAsync(q.mask_bits.p, bits, (n_bases + 7) / 8, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));                // the caller may free its bits
    if ((rc = q.masked.grow_keep(ix->recs_cap() * sizeof(unsigned long long), ix->stream))) return rc;
    q.mask_n_bases = n_bases;
    q.mask_mode = (uint32_t)mode;
    q.mask_out_n = 0;
    q.apply = true;
    return PK_OK;
}

extern "C" int pk_query_mask_text(pk_indexer *ix, uint8_t *host_out, uint64_t cap, uint64_t *n_out) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->q || !ix->q->apply) return fail(PK_ERR_STATE, "the indexer applies no mask (pk_query_set_mask)");
    if (!n_out) return fail(PK_ERR_ARG, "null output pointer");
    const QueryState &q = *ix->q;
    *n_out = q.mask_out_n;
    if (q.mask_out_n > cap) return fail(PK_ERR_RECS_CAP, "%llu bytes of text, capacity %llu", (unsigned long long)q.mask_out_n, (unsigned long long)cap);
    if (q.mask_out_n == 0) return PK_OK;
    if (!host_out) return fail(PK_ERR_ARG, "null output pointer");
    return bounce_copy(q.mask_out.p, host_out, q.mask_out_n, false, ix->device);   // every feed ends with a wait
}

extern "C" int pk_query_mask_counts(pk_indexer *ix, uint64_t *masked_out, uint64_t recs_cap, uint64_t *n_bases_seen_out) {
    if (int rc = query_check(ix, applying, "the indexer applies no mask (pk_query_set_mask)", nullptr)) return rc;
    if (!n_bases_seen_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    const QueryState &q = *ix->q;
    if (int rc = bases_seen(ix, n_bases_seen_out)) return rc;
    if (*n_bases_seen_out != q.mask_n_bases)
        return fail(PK_ERR_STATE, "the stream holds %llu valid bases and the mask was made for %llu: the text changed between the phases",
                    (unsigned long long)*n_bases_seen_out, (unsigned long long)q.mask_n_bases);
    if (ix->n_recs > recs_cap) return fail(PK_ERR_RECS_CAP, "%llu records, capacity %llu", (unsigned long long)ix->n_recs, (unsigned long long)recs_cap);
    if (ix->n_recs == 0) return PK_OK;
    if (!masked_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipMemcpy(masked_out, q.masked.p, ix->n_recs * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PK_OK;
}

// the rows of a finished binned stream: the last record's bins are not in Bf
int pk::query_count_bins(pk_indexer *ix) {
    QueryState &q = *ix->q;
    q.n_bins = 0;
    if (!q.bin || !ix->n_recs) return PK_OK;
    unsigned long long bf = 0;
    DevRec last;
    HIPCHK(hipMemcpy(&bf, q.Bf.p + (ix->n_recs - 1), sizeof bf, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&last, ix->recs.p + (ix->n_recs - 1), sizeof last, hipMemcpyDeviceToHost));
    q.n_bins = bf + (last.n_valid ? (last.n_valid - 1) / q.bin + 1 : 0);
    return PK_OK;
}

extern "C" int pk_query_bin_count(pk_indexer *ix, uint64_t *n_bins_out) {
    if (!ix || !n_bins_out) return fail(PK_ERR_ARG, "null argument");
    if (int rc = query_check(ix, binned, "the indexer tallies per record (pk_query_set_bins)", nullptr)) return rc;
    *n_bins_out = ix->q->n_bins;
    return PK_OK;
}

extern "C" int pk_query_bin_results(pk_indexer *ix, uint64_t *hits_out, uint64_t *depth_out, uint64_t *bin_first_out, uint64_t bins_cap,
                                    uint64_t recs_cap) {
    if (int rc = query_check(ix, binned, "the indexer tallies per record (pk_query_set_bins); use pk_query_results", nullptr)) return rc;
    const QueryState &q = *ix->q;
    if (ix->n_recs > recs_cap || q.n_bins > bins_cap)
        return fail(PK_ERR_RECS_CAP, "%llu bins and %llu records, capacities %llu and %llu", (unsigned long long)q.n_bins,
                    (unsigned long long)ix->n_recs, (unsigned long long)bins_cap, (unsigned long long)recs_cap);
    if (!bin_first_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    if (ix->n_recs) HIPCHK(hipMemcpy(bin_first_out, q.Bf.p, ix->n_recs * sizeof(uint64_t), hipMemcpyDeviceToHost));
    bin_first_out[ix->n_recs] = q.n_bins;
    if (q.n_bins == 0) return PK_OK;
    if (!hits_out || !depth_out) return fail(PK_ERR_ARG, "null output pointer");
    const size_t n = q.n_bins * q.tables.size() * sizeof(uint64_t);
    HIPCHK(hipMemcpy(hits_out, q.hits.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(depth_out, q.depth.p, n, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_bin_coords(pk_indexer *ix, uint64_t *start_out, uint64_t *end_out, uint64_t bins_cap) {
    if (int rc = query_check(ix, with_coords, "the indexer keeps no coordinates (pk_query_set_coords)", nullptr)) return rc;
    const QueryState &q = *ix->q;
    if (q.n_bins > bins_cap)
        return fail(PK_ERR_RECS_CAP, "%llu bins, capacity %llu", (unsigned long long)q.n_bins, (unsigned long long)bins_cap);
    if (q.n_bins == 0) return PK_OK;
    if (!start_out || !end_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    const size_t n = q.n_bins * sizeof(uint64_t);
    HIPCHK(hipMemcpy(start_out, q.bin_start.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(end_out, q.bin_end.p, n, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_results(pk_indexer *ix, uint64_t *hits_out, uint64_t *depth_out, uint64_t recs_cap) {
    if (int rc = query_check(ix, per_record, "the indexer tallies per bin (pk_query_set_bins); use pk_query_bin_results", nullptr)) return rc;
    if (ix->n_recs > recs_cap) return fail(PK_ERR_RECS_CAP, "%llu records, capacity %llu", (unsigned long long)ix->n_recs, (unsigned long long)recs_cap);
    if (ix->n_recs == 0) return PK_OK;
    if (!hits_out || !depth_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    const size_t n = ix->n_recs * ix->q->tables.size() * sizeof(uint64_t);
    HIPCHK(hipMemcpy(hits_out, ix->q->hits.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(depth_out, ix->q->depth.p, n, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_spectrum(pk_indexer *ix, uint64_t *out, uint64_t rows_cap) {
    if (int rc = query_check(ix, with_spectrum, "the indexer keeps no count spectra (pk_query_set_spectrum)", nullptr)) return rc;
    const QueryState &q = *ix->q;
    const uint64_t rows = q.bin ? q.n_bins : ix->n_recs;
    if (rows > rows_cap) return fail(PK_ERR_RECS_CAP, "%llu rows, capacity %llu", (unsigned long long)rows, (unsigned long long)rows_cap);
    if (rows == 0) return PK_OK;
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(out, q.spec.p, rows * q.tables.size() * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_pairs(pk_indexer *ix, uint64_t *out, uint64_t rows_cap) {
    if (int rc = query_check(ix, with_pairs, "the indexer keeps no shared windows (pk_query_set_pairs)", nullptr)) return rc;
    const QueryState &q = *ix->q;
    const uint64_t rows = q.bin ? q.n_bins : ix->n_recs;
    if (rows > rows_cap) return fail(PK_ERR_RECS_CAP, "%llu rows, capacity %llu", (unsigned long long)rows, (unsigned long long)rows_cap);
    if (rows == 0 || q.n_pairs() == 0) return PK_OK;
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(out, q.shared.p, rows * q.n_pairs() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PK_OK;
}
