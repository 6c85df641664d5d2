// pk_correct.hip -- the host layer of the read corrector (pk_correct_*, include/pykmer_hip.h): the caller's tables, the cover
// bits on the device, the position of the stream and the valid bases seen so far, and the feeds through the kernels of
// kmer_correct.hip.  A feed is whole records, as pk_trim's: the one value carried from feed to feed is the stream's valid
// bases.  The corrected text is a copy of the feed's text made on the stream in front of the kernels, which patch it; the
// text that is read is never written.
#include "pk_host.h"

using namespace pk;

static_assert(CORR_FIELDS == PK_CORR_FIELDS, "the kernels' fields are the header's");

struct pk_correct {
    int k = 0, device = 0;
    bool ready = false;                          // the device side exists (made by pk_correct_set_tables)
    bool have_tables = false, have_cover = false, fed = false, finished = false;
    // members are destroyed in reverse order of declaration, behind the destructor's wait: the buffers, then the stream
    Stream stream;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;         // around the kernels of one feed
    DevBuf<const uint8_t *> tables;                          // the caller's table pointers, as the kernel reads them
    DevBuf<uint32_t> bits;
    DevBuf<uint8_t> text, text_out;                          // the device copies of a host-fed feed
    DevBuf<unsigned long long> starts, cnt, geo, out, total;
    uint32_t n_tab = 0, min = 1, max = 255, min_windows = 1;
    uint64_t n_bases = 0, n_words = 0;
    uint32_t tq = 0;
    uint64_t pos = 0, records = 0, valid = 0, feeds = 0;
    uint64_t sums[4] = {0, 0, 0, 0};                         // candidates, untried, corrected, ambiguous
    double t_kernels = 0;

    ~pk_correct() {
        if (!ready) return;
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        for (hipEvent_t e : {ev_begin, ev_end}) if (e) hipEventDestroy(e);
    }
};

static int ensure_device(pk_correct *c) {
    HIPCHK(hipSetDevice(c->device));
    if (c->ready) return PK_OK;
    c->ready = true;                             // from here on the destructor cleans up
    HIPCHK(hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev_begin));
    HIPCHK(hipEventCreate(&c->ev_end));
    return c->total.reserve(sizeof(unsigned long long));
}

extern "C" int pk_correct_create(pk_correct **out, int k, int device) {
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    if (k < 1 || k > 17 || k % 2 == 0) return fail(PK_ERR_ARG, "kmer_len must be odd and at most 17, got %d", k);
    if (device < 0 || device >= MAX_DEVICES) return fail(PK_ERR_ARG, "device ordinal %d out of range", device);
    *out = new pk_correct();
    (*out)->k = k;
    (*out)->device = device;
    return PK_OK;
}

extern "C" void pk_correct_destroy(pk_correct *c) { delete c; }

extern "C" int pk_correct_set_tables(pk_correct *c, const void *const *dev_tables, int N, int min_count, int max_count) {
    if (!c) return fail(PK_ERR_ARG, "null corrector");
    if (c->fed || c->finished) return fail(PK_ERR_STATE, "the tables are set before the first feed");
    if (N < 1 || !dev_tables) return fail(PK_ERR_ARG, "need at least one table");
    if (N > (int)QUERY_MAX_TABLES) return fail(PK_ERR_ARG, "a correction takes at most %u tables, all in one launch; got %d", QUERY_MAX_TABLES, N);
    if (min_count < 1 || max_count > 255 || min_count > max_count) return fail(PK_ERR_ARG, "count window must satisfy 1 <= min <= max <= 255, got %d-%d", min_count, max_count);
    for (int i = 0; i < N; i++)
        if (!dev_tables[i]) return fail(PK_ERR_ARG, "table %d is a null pointer", i);
    c->have_tables = c->have_cover = false;
    if (int rc = ensure_device(c)) return rc;
    if (int rc = c->tables.reserve((size_t)N * sizeof(const uint8_t *))) return rc;
    if (int rc = bounce_copy(c->tables.p, (void *)dev_tables, (size_t)N * sizeof(const uint8_t *), true, c->device)) return rc;
    c->n_tab = (uint32_t)N;
    c->min = (uint32_t)min_count;
    c->max = (uint32_t)max_count;
    c->have_tables = true;
    return PK_OK;
}

extern "C" int pk_correct_set_cover(pk_correct *c, const uint8_t *cover, uint64_t n_bases, int min_qual_byte, int min_windows) {
    if (!c) return fail(PK_ERR_ARG, "null corrector");
    if (!c->have_tables) return fail(PK_ERR_STATE, "pk_correct_set_tables comes before pk_correct_set_cover");
    if (c->fed || c->finished) return fail(PK_ERR_STATE, "the cover bits are set before the first feed");
    if (n_bases && !cover) return fail(PK_ERR_ARG, "null cover bits with %llu bases", (unsigned long long)n_bases);
    if (min_qual_byte < 0 || min_qual_byte > 255) return fail(PK_ERR_ARG, "the quality threshold byte must lie in 0 .. 255, got %d", min_qual_byte);
    if (min_windows < 1 || min_windows > c->k) return fail(PK_ERR_ARG, "min_windows must lie in 1 .. kmer_len = %d, got %d", c->k, min_windows);
    if (n_bases >= (uint64_t)SIZE_MAX / 2u) return fail(PK_ERR_ARG, "%llu bases are beyond the address space", (unsigned long long)n_bases);
    c->have_cover = false;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t n_bytes = (n_bases + 7u) / 8u;
    c->n_words = (n_bases + 31u) / 32u;
    if (c->n_words) {
        std::vector<uint32_t> words(c->n_words, 0u);         // the last word's bytes behind the bits stay zero
        memcpy(words.data(), cover, n_bytes);
        if (n_bases & 7u) reinterpret_cast<uint8_t *>(words.data())[n_bytes - 1u] &= (uint8_t)((1u << (n_bases & 7u)) - 1u);
        if (int rc = c->bits.reserve(c->n_words * sizeof(uint32_t))) return rc;
        if (int rc = bounce_copy(c->bits.p, words.data(), c->n_words * sizeof(uint32_t), true, c->device)) return rc;
    }
    c->n_bases = n_bases;
    c->tq = (uint32_t)min_qual_byte;
    c->min_windows = (uint32_t)min_windows;
    c->have_cover = true;
    return PK_OK;
}

// The opening checks of both feeds; no kernel is launched, and nothing moves, when one of them fails.
static int feed_check(pk_correct *c, const void *text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, const void *text_out,
                      const uint64_t *out) {
    if (!c) return fail(PK_ERR_ARG, "null corrector");
    if (!c->have_cover) return fail(PK_ERR_STATE, "pk_correct_set_tables and pk_correct_set_cover come before the first feed");
    if (c->finished) return fail(PK_ERR_STATE, "the stream is finished");
    if (n_bytes && (!text || !text_out)) return fail(PK_ERR_ARG, "null text pointer");
    if (n_records && (!starts || !out)) return fail(PK_ERR_ARG, "null pointer with %llu records", (unsigned long long)n_records);
    if (n_records >= SIZE_MAX / (16u * TRIM_FIELDS)) return fail(PK_ERR_ARG, "%llu records are beyond the address space", (unsigned long long)n_records);
    if (!starts) return PK_OK;
    for (uint64_t r = 0; r < n_records; r++)
        if (starts[r + 1] < starts[r])
            return fail(PK_ERR_ARG, "the record offsets must not decrease: starts[%llu] = %llu is followed by %llu", (unsigned long long)r,
                        (unsigned long long)starts[r], (unsigned long long)starts[r + 1]);
    if (starts[n_records] != n_bytes)
        return fail(PK_ERR_ARG, "a feed holds whole records: the last offset is %llu, the feed has %llu bytes", (unsigned long long)starts[n_records],
                    (unsigned long long)n_bytes);
    return PK_OK;
}

// The copy of dev_text into dev_out, the kernels over dev_text and the read-back; out: CORR_FIELDS * n_records words on the host.
static int run_feed(pk_correct *c, const uint8_t *dev_text, uint8_t *dev_out, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records,
                    uint64_t *out) {
    if (n_bytes) HIPCHK(hipMemcpyAsync(dev_out, dev_text, n_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (n_records) {
        const uint64_t R = n_records;
        if (int rc = c->starts.reserve((R + 1u) * sizeof(uint64_t))) return rc;
        if (int rc = c->cnt.reserve(R * sizeof(uint64_t))) return rc;
        if (int rc = c->geo.reserve(R * TRIM_FIELDS * sizeof(uint64_t))) return rc;
        if (int rc = c->out.reserve(R * CORR_FIELDS * sizeof(uint64_t))) return rc;
        if (int rc = bounce_copy(c->starts.p, const_cast<uint64_t *>(starts), (R + 1u) * sizeof(uint64_t), true, c->device)) return rc;
        HIPCHK(hipEventRecord(c->ev_begin, c->stream));
        if (launch_correct(dev_text, c->starts.p, R, c->pos, c->tq, c->bits.p, c->n_words, c->valid, c->cnt.p, c->total.p, c->geo.p, (uint32_t)c->k,
                           c->tables.p, c->n_tab, c->min, c->max, c->min_windows, dev_out, c->out.p, c->stream))
            return fail(PK_ERR_HIP, "launching the correct kernels failed: %s", hipGetErrorString(hipGetLastError()));
        HIPCHK(hipEventRecord(c->ev_end, c->stream));
        unsigned long long total = 0;
        HIPCHK(hipMemcpyAsync(&total, c->total.p, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_begin, c->ev_end));
        c->t_kernels += ms * 1e-3;
        if (int rc = bounce_copy(c->out.p, out, R * CORR_FIELDS * sizeof(uint64_t), false, c->device)) return rc;
        c->valid = total;
        for (int f = 0; f < 4; f++)
            for (uint64_t r = 0; r < R; r++) c->sums[f] += out[(uint64_t)(PK_CORR_CANDIDATES + f) * R + r];
        c->records += R;
    } else if (n_bytes) {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    c->pos += n_bytes;
    c->fed = true;
    c->feeds++;
    return PK_OK;
}

extern "C" int pk_correct_feed(pk_correct *c, const uint8_t *host_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records,
                               uint8_t *host_text_out, uint64_t *out) {
    if (int rc = feed_check(c, host_text, n_bytes, starts, n_records, host_text_out, out)) return rc;
    if (n_bytes) {
        HIPCHK(hipSetDevice(c->device));
        if (int rc = c->text.reserve(n_bytes)) return rc;
        if (int rc = c->text_out.reserve(n_bytes)) return rc;
        if (int rc = bounce_copy(c->text.p, const_cast<uint8_t *>(host_text), n_bytes, true, c->device)) return rc;
    }
    if (int rc = run_feed(c, c->text.p, c->text_out.p, n_bytes, starts, n_records, out)) return rc;
    return n_bytes ? bounce_copy(c->text_out.p, host_text_out, n_bytes, false, c->device) : PK_OK;
}

extern "C" int pk_correct_feed_device(pk_correct *c, const void *dev_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records,
                                      void *dev_text_out, uint64_t *out) {
    if (int rc = feed_check(c, dev_text, n_bytes, starts, n_records, dev_text_out, out)) return rc;
    if (n_bytes) {
        const uint8_t *a = (const uint8_t *)dev_text, *b = (const uint8_t *)dev_text_out;
        if (a < b + n_bytes && b < a + n_bytes) return fail(PK_ERR_ARG, "the corrected text may not overlap the text that is read");
        HIPCHK(hipSetDevice(c->device));
    }
    return run_feed(c, (const uint8_t *)dev_text, (uint8_t *)dev_text_out, n_bytes, starts, n_records, out);
}

extern "C" int pk_correct_finish(pk_correct *c, uint64_t totals_out[6]) {
    if (!c || !totals_out) return fail(PK_ERR_ARG, "null argument");
    if (!c->have_cover) return fail(PK_ERR_STATE, "pk_correct_set_cover comes first");
    c->finished = true;
    totals_out[0] = c->records;
    totals_out[1] = c->valid;
    for (int f = 0; f < 4; f++) totals_out[2 + f] = c->sums[f];
    if (c->valid != c->n_bases)
        return fail(PK_ERR_STATE, "the stream holds %llu valid bases, the cover bits were made for %llu", (unsigned long long)c->valid,
                    (unsigned long long)c->n_bases);
    return PK_OK;
}

extern "C" int pk_correct_timings(pk_correct *c, double out[2]) {
    if (!c || !out) return fail(PK_ERR_ARG, "null argument");
    out[0] = c->t_kernels;
    out[1] = (double)c->feeds;
    return PK_OK;
}
