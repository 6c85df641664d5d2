// pk_query.hip -- query mode of the host layer: the state a query indexer holds (QueryState, pk_host.h), the one rule that
// sizes its arrays (size_rows) and the pk_query_* entry points, which share their opening checks (query_check), their
// setters' tail (switch_option) and their read-outs (read_rows).  The feeds themselves go through pk_indexer.hip, which
// queues the kernels of kmer_query.hip, kmer_coords.hip, kmer_cover.hip and kmer_intervals.hip behind the squeeze.
#include "pk_host.h"

using namespace pk;

int QueryState::create() {
    for (hipEvent_t *e : {&lookup_begin, &lookup_end, &coords_begin, &coords_end, &mask_begin, &mask_end, &iv_count_begin, &iv_count_end, &iv_write_begin,
                          &iv_write_end})
        HIPCHK(hipEventCreate(e));
    return P.reserve(4096 * sizeof(unsigned long long));
}

int QueryState::reset(hipStream_t s) {
    for (DevBuf<unsigned long long> *b : {&P, &Bf, &hits, &depth, &bin_start, &bin_end, &pos.words, &spec, &shared, &nb.words, &masked, &iv_starts.words, &iv_ends.words})
        if (b->p) HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, s));
    if (cover_bits.p) HIPCHK(hipMemsetAsync(cover_bits.p, 0, cover_bits.bytes, s));
    windows = p_done = 0;
    bin = n_bins = 0;
    spectrum = false;
    pairs = false;
    coords = false; pos.in = 0; t_coords = 0;
    cover = apply = false; nb.in = 0; t_mask = 0;
    mask_n_bases = mask_out_n = 0; mask_mode = 0;
    intervals = false; iv_starts.in = iv_ends.in = 0; n_intervals = 0; t_intervals = 0;   // rows below the counts are always written: not zeroed
    return PK_OK;
}

// One array, or two of a kind, keyed by the records or by the rows of the tallies: what size_rows needs to size it.
struct RowArray {
    DevBuf<unsigned long long> *a, *b;                       // b: null, or a second array of the same shape
    bool on;                                                 // the option that needs it is set
    uint64_t rows;
    size_t per_row;                                          // bytes
    bool by_half;                                            // it grows by half at least, so that a long stream does not move it with
                                                             // every feed; otherwise to exactly what is needed
    // The refusal of an array that does not fit names its size and what makes it smaller.  lead (printf: the bin size), noun
    // and shape (printf: rows, tables, pairs) word the failed growth; lead and beyond (printf: rows, count) the size that is
    // beyond the address space.  No lead: the allocation's own message; no beyond: no such check.
    const char *lead = nullptr, *noun = nullptr, *shape = nullptr, *beyond = nullptr, *advice = nullptr;
    size_t count = 0;
};

// The one place that sizes what grows with the record array (`cap` records) or with the rows of the tallies: per record `cap`
// rows; binned the rows that `bytes` bytes of stream and `cap` records can make, which needs no read-back: every record
// adds at most one partial bin, and n bytes hold at most n windows.  Contents kept, the rest zero.  The growth rules are part
// of the retry and memory behaviour: the record-keyed arrays and the per-record tallies are sized exactly; binned, hits,
// depth, the coordinates and the shared windows grow by half at least; the spectra grow to exactly what is needed, always:
// at 256 times the size of hits the old and the new array side by side are what the device has to hold, and a copy at HBM
// speed per feed is cheap beside the lookups.  Last the cover bits: one bit per valid base, and a stream of `bytes` bytes
// holds at most as many; one word in front of the first base's is never written, one behind the last takes the read of a
// lane's third word.
int QueryState::size_rows(uint64_t cap, uint64_t bytes, hipStream_t s) {
    const size_t word = sizeof(unsigned long long), N = tables.size(), NP = n_pairs();
    const bool binned = bin != 0;
    const uint64_t rows = binned ? bytes / bin + cap + 1 : cap;
    const char *bins = "bins of %llu windows", *larger = "take larger bins", *fewer = "take fewer tables per run, larger bins or a smaller query";
    const RowArray arrays[] = {
        {&P, nullptr, true, cap, word, false},
        {&Bf, nullptr, binned, cap, word, false},
        binned ? RowArray{&hits, &depth, true, rows, N * word, true, bins, "two accumulators", "%llu rows, %zu tables", ": %llu rows of %zu tables", larger, N}
               : RowArray{&hits, &depth, N > 0, rows, N * word, false},
        {&bin_start, &bin_end, binned && coords, rows, word, true, bins, "two coordinate arrays", "%llu rows", nullptr, larger},
        {&spec, nullptr, spectrum, rows, N * 256 * word, false, "count spectra", "an accumulator", "%llu rows, %zu tables, 2 KiB each",
         " of %llu rows and %zu tables (2 KiB each)", fewer, N},
        {&masked, nullptr, apply, cap, word, false},
        {&shared, nullptr, pairs && NP > 0, rows, NP * word, binned, "shared windows", "an accumulator", "%llu rows, %zu tables, %zu pairs of 8 bytes each",
         " of %llu rows and %zu pairs of tables", fewer, NP},
    };
    char lead[64], text[128];                                // of a refusal
    for (const RowArray &r : arrays) {
        if (!r.on) continue;
        if (r.beyond && r.rows > SIZE_MAX / 2 / r.per_row) {
            snprintf(lead, sizeof lead, r.lead, (unsigned long long)bin);
            snprintf(text, sizeof text, r.beyond, (unsigned long long)r.rows, r.count);
            return fail(PK_ERR_ARG, "%s%s are beyond the address space; %s", lead, text, r.advice);
        }
        for (DevBuf<unsigned long long> *buf : {r.a, r.b}) {
            if (!buf || r.rows * r.per_row <= buf->bytes) continue;
            const size_t want = r.by_half ? std::max<size_t>(r.rows * r.per_row, buf->bytes + buf->bytes / 2) : r.rows * r.per_row;
            const int rc = buf->grow_keep(want, s);
            if (!rc) continue;
            if (!r.lead) return rc;
            (void)hipGetLastError();
            const std::string why = g_err;
            snprintf(lead, sizeof lead, r.lead, (unsigned long long)bin);
            snprintf(text, sizeof text, r.shape, (unsigned long long)r.rows, N, NP);
            return fail(rc, "%s need %s of %zu bytes (%s); %s: %s", lead, r.noun, want, text, r.advice, why.c_str());
        }
    }
    const size_t need = (bytes / 32 + 2) * sizeof(uint32_t);
    if (!cover || need <= cover_bits.bytes) return PK_OK;
    return cover_bits.grow_keep(std::max<size_t>(need, cover_bits.bytes + cover_bits.bytes / 2), s);
}

// The interval rows grow with the intervals found, by half at least, never with the bytes fed.
int QueryState::size_intervals(uint64_t rows, hipStream_t s) {
    const size_t need = (size_t)rows * sizeof(unsigned long long);
    for (DevBuf<unsigned long long> *buf : {&iv_record, &iv_start, &iv_end}) {
        if (need <= buf->bytes) continue;
        const size_t want = std::max<size_t>(need, buf->bytes + buf->bytes / 2);
        const int rc = buf->grow_keep(want, s);
        if (!rc) continue;
        (void)hipGetLastError();
        const std::string why = g_err;
        return fail(rc, "the intervals need three arrays of %zu bytes (%llu rows): %s", want, (unsigned long long)rows, why.c_str());
    }
    return PK_OK;
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
    // the tallies of an empty stream for this many tables: all zero before the first feed, whatever N was (a reset zeroed what
    // was there, a new array is zeroed here)
    return q.size_rows(ix->recs_cap(), 0, ix->stream);
}

// What the on/off setters share behind their own checks: the flag, what the option needs besides its rows (`prepare`, null
// for nothing), and the arrays for the settings so far (a reset zeroed what was there, a new array is zeroed here).
static int switch_option(pk_indexer *ix, bool *flag, int on, int (*prepare)(pk_indexer *)) {
    *flag = on != 0;
    int rc = *flag && prepare ? prepare(ix) : PK_OK;
    if (!rc) rc = ix->q->size_rows(ix->recs_cap(), 0, ix->stream);
    if (rc) *flag = false;                                   // an array that did not fit: the setting did not take
    return rc;
}

extern "C" int pk_query_set_bins(pk_indexer *ix, uint64_t bin_windows) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_bins", "the bins are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    QueryState &q = *ix->q;
    q.bin = bin_windows;
    q.coords = false;                                        // pk_query_set_coords comes after the bins
    return q.size_rows(ix->recs_cap(), 0, ix->stream);       // Bf beside P, and the rows of every tally that is on
}

extern "C" int pk_query_set_spectrum(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_spectrum", "the spectra are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    QueryState &q = *ix->q;
    if (on && q.pairs) return fail(PK_ERR_ARG, "count spectra and shared windows (pk_query_set_pairs) are tallied in separate streams");
    return switch_option(ix, &q.spectrum, on, nullptr);      // per record or for the bins set so far
}

extern "C" int pk_query_set_pairs(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_pairs", "the pairs are set before the first feed (reset the indexer first)")) return rc;
    QueryState &q = *ix->q;
    if (on && q.tables.size() > QUERY_MAX_TABLES)
        return fail(PK_ERR_ARG, "shared windows take at most %u tables, all in one lookup; the indexer has %zu", QUERY_MAX_TABLES, q.tables.size());
    if (on && q.spectrum) return fail(PK_ERR_ARG, "shared windows and count spectra (pk_query_set_spectrum) are tallied in separate streams");
    HIPCHK(hipSetDevice(ix->device));
    return switch_option(ix, &q.pairs, on, nullptr);         // per record or for the bins set so far
}

extern "C" int pk_query_set_coords(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, binned, "pk_query_set_bins with bins of at least one window comes before pk_query_set_coords", "the coordinates are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    return switch_option(ix, &ix->q->coords, on, [](pk_indexer *x) { return x->q->pos.ready(x->stream); });   // the position words, then the two arrays
}

static int base_count_ready(pk_indexer *ix) { return ix->q->nb.ready(ix->stream); }

extern "C" int pk_query_set_cover(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, has_tables, "pk_query_set_tables comes before pk_query_set_cover", "the cover bits are set before the first feed (reset the indexer first)")) return rc;
    QueryState &q = *ix->q;
    if (on && (q.bin || q.spectrum || q.pairs))
        return fail(PK_ERR_ARG, "the cover bits take the place of the tallies: bins, count spectra and shared windows belong to a stream of their own");
    if (on && q.apply) return fail(PK_ERR_ARG, "the indexer applies a mask (pk_query_set_mask); the cover bits come from a stream of their own");
    HIPCHK(hipSetDevice(ix->device));
    return switch_option(ix, &q.cover, on, base_count_ready);    // the base-count words, then the bits of an empty stream
}

// the valid bases of the stream so far, as the last settled feed left them (after a wait on the stream)
static int bases_seen(pk_indexer *ix, uint64_t *out) {
    *out = 0;
    if (!ix->q->nb.words.p) return PK_OK;
    unsigned long long n = 0;
    HIPCHK(hipMemcpy(&n, ix->q->nb.start(), sizeof n, hipMemcpyDeviceToHost));
    *out = n;
    return PK_OK;
}

static bool with_cover(const QueryState &q) { return q.cover; }
static bool applying(const QueryState &q) { return q.apply; }

// What the read-outs of a finished stream share behind their own checks: `rows` rows of `per_row` bytes from `a` to `a_out`
// (and from `b` to `b_out`, where there is a second array) -- the capacity, which names the rows by `unit`; nothing to copy;
// the null pointers; the copies.
static int read_rows(pk_indexer *ix, uint64_t rows, uint64_t cap, const char *unit, size_t per_row, const DevBuf<unsigned long long> &a, uint64_t *a_out,
                     const DevBuf<unsigned long long> *b = nullptr, uint64_t *b_out = nullptr) {
    if (rows > cap) return fail(PK_ERR_RECS_CAP, "%llu %s, capacity %llu", (unsigned long long)rows, unit, (unsigned long long)cap);
    if (rows == 0 || per_row == 0) return PK_OK;
    if (!a_out || (b && !b_out)) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(a_out, a.p, rows * per_row, hipMemcpyDeviceToHost));
    if (b) HIPCHK(hipMemcpy(b_out, b->p, rows * per_row, hipMemcpyDeviceToHost));
    return PK_OK;
}

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
    int rc = base_count_ready(ix);
    if (rc) return rc;
    // whole words, zero behind the last base; one more for the read of a lane's third word
    const size_t words = n_bases / 32 + 2;
    if ((rc = q.mask_bits.reserve(words * sizeof(uint32_t)))) return rc;
    HIPCHK(hipMemsetAsync(q.mask_bits.p, 0, q.mask_bits.bytes, ix->stream));
    if (n_bases) HIPCHK(hipMemcpyAsync(q.mask_bits.p, bits, (n_bases + 7) / 8, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));                // the caller may free its bits
    if ((rc = switch_option(ix, &q.apply, 1, nullptr))) return rc;   // masked[], with the record array
    q.mask_n_bases = n_bases;
    q.mask_mode = (uint32_t)mode;
    q.mask_out_n = 0;
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
    return read_rows(ix, ix->n_recs, recs_cap, "records", sizeof(uint64_t), q.masked, masked_out);
}

extern "C" int pk_query_set_intervals(pk_indexer *ix, int on) {
    if (int rc = query_check(ix, applying, "pk_query_set_mask comes before pk_query_set_intervals", "the intervals are set before the first feed (reset the indexer first)")) return rc;
    HIPCHK(hipSetDevice(ix->device));
    // the position word and the two counts, then rows for a first feed
    return switch_option(ix, &ix->q->intervals, on, [](pk_indexer *x) {
        QueryState &q = *x->q;
        for (Carried *c : {&q.pos, &q.iv_starts, &q.iv_ends})
            if (int rc = c->ready(x->stream)) return rc;
        return q.size_intervals(1024, x->stream);
    });
}

static bool with_intervals(const QueryState &q) { return q.intervals; }

extern "C" int pk_query_interval_count(pk_indexer *ix, uint64_t *n_out, double *seconds_out) {
    if (!ix || !n_out) return fail(PK_ERR_ARG, "null argument");
    if (int rc = query_check(ix, with_intervals, "the indexer keeps no intervals (pk_query_set_intervals)", nullptr)) return rc;
    *n_out = ix->q->n_intervals;
    if (seconds_out) *seconds_out = ix->q->t_intervals;
    return PK_OK;
}

extern "C" int pk_query_intervals(pk_indexer *ix, uint64_t *rec_out, uint64_t *start_out, uint64_t *end_out, uint64_t cap) {
    if (int rc = query_check(ix, with_intervals, "the indexer keeps no intervals (pk_query_set_intervals)", nullptr)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    const QueryState &q = *ix->q;
    uint64_t seen = 0;
    if (int rc = bases_seen(ix, &seen)) return rc;
    if (seen != q.mask_n_bases)
        return fail(PK_ERR_STATE, "the stream holds %llu valid bases and the mask was made for %llu: the text changed between the phases",
                    (unsigned long long)seen, (unsigned long long)q.mask_n_bases);
    if (int rc = read_rows(ix, q.n_intervals, cap, "intervals", sizeof(uint64_t), q.iv_record, rec_out)) return rc;
    return read_rows(ix, q.n_intervals, cap, "intervals", sizeof(uint64_t), q.iv_start, start_out, &q.iv_end, end_out);
}

// the intervals of a finished stream: a run still open belongs to the last record and ends with it
int pk::query_close_intervals(pk_indexer *ix) {
    QueryState &q = *ix->q;
    q.n_intervals = 0;
    if (!q.intervals) return PK_OK;
    unsigned long long ns = 0, ne = 0;
    HIPCHK(hipMemcpy(&ns, q.iv_starts.start(), sizeof ns, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ne, q.iv_ends.start(), sizeof ne, hipMemcpyDeviceToHost));
    if (ns < ne || ns - ne > 1 || ns * sizeof(unsigned long long) > q.iv_end.bytes || (ns > ne && !ix->n_recs))
        return fail(PK_ERR_HIP, "%llu interval starts and %llu ends (internal error)", ns, ne);
    if (ns > ne) HIPCHK(hipMemcpy(q.iv_end.p + ne, &ix->recs.p[ix->n_recs - 1].seq_len, sizeof(unsigned long long), hipMemcpyDeviceToDevice));
    q.n_intervals = ns;
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
    return read_rows(ix, q.n_bins, bins_cap, "bins", q.tables.size() * sizeof(uint64_t), q.hits, hits_out, &q.depth, depth_out);
}

extern "C" int pk_query_bin_coords(pk_indexer *ix, uint64_t *start_out, uint64_t *end_out, uint64_t bins_cap) {
    if (int rc = query_check(ix, with_coords, "the indexer keeps no coordinates (pk_query_set_coords)", nullptr)) return rc;
    const QueryState &q = *ix->q;
    return read_rows(ix, q.n_bins, bins_cap, "bins", sizeof(uint64_t), q.bin_start, start_out, &q.bin_end, end_out);
}

extern "C" int pk_query_results(pk_indexer *ix, uint64_t *hits_out, uint64_t *depth_out, uint64_t recs_cap) {
    if (int rc = query_check(ix, per_record, "the indexer tallies per bin (pk_query_set_bins); use pk_query_bin_results", nullptr)) return rc;
    const QueryState &q = *ix->q;
    return read_rows(ix, ix->n_recs, recs_cap, "records", q.tables.size() * sizeof(uint64_t), q.hits, hits_out, &q.depth, depth_out);
}

extern "C" int pk_query_spectrum(pk_indexer *ix, uint64_t *out, uint64_t rows_cap) {
    if (int rc = query_check(ix, with_spectrum, "the indexer keeps no count spectra (pk_query_set_spectrum)", nullptr)) return rc;
    const QueryState &q = *ix->q;
    return read_rows(ix, q.bin ? q.n_bins : ix->n_recs, rows_cap, "rows", q.tables.size() * 256 * sizeof(uint64_t), q.spec, out);
}

extern "C" int pk_query_pairs(pk_indexer *ix, uint64_t *out, uint64_t rows_cap) {
    if (int rc = query_check(ix, with_pairs, "the indexer keeps no shared windows (pk_query_set_pairs)", nullptr)) return rc;
    const QueryState &q = *ix->q;
    return read_rows(ix, q.bin ? q.n_bins : ix->n_recs, rows_cap, "rows", q.n_pairs() * sizeof(uint64_t), q.shared, out);   // one table: no pair, nothing to copy
}
