// pk_trim.hip -- the host layer of the read trimmer (pk_trim_*, include/pykmer_hip.h): the cover bits on the device, the
// position of the stream and the valid bases seen so far, and the feeds through the kernels of kmer_trim.hip.  A feed is
// whole records, so nothing of the text is carried from feed to feed: the one value that is, the stream's valid bases, comes
// back with every feed's result and goes into the next feed's scan as an argument.
#include "pk_host.h"

using namespace pk;

static_assert(TRIM_FIELDS == PK_TRIM_FIELDS, "the kernels' fields are the header's");

struct pk_trim {
    int device = 0;
    bool ready = false;                          // the device side exists (made by pk_trim_set_cover)
    bool have_cover = false, fed = false, finished = false;
    // members are destroyed in reverse order of declaration, behind the destructor's wait: the buffers, then the stream
    Stream stream;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;         // around the kernels of one feed
    DevBuf<uint32_t> bits;
    DevBuf<uint8_t> text;                                    // the device copy of a host-fed feed
    DevBuf<unsigned long long> starts, cnt, geo, total;
    uint64_t n_bases = 0, n_words = 0;
    uint32_t tq = 0;
    uint64_t pos = 0, records = 0, valid = 0, covered = 0, feeds = 0;
    double t_kernels = 0;

    ~pk_trim() {
        if (!ready) return;
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        for (hipEvent_t e : {ev_begin, ev_end}) if (e) hipEventDestroy(e);
    }
};

static int ensure_device(pk_trim *t) {
    HIPCHK(hipSetDevice(t->device));
    if (t->ready) return PK_OK;
    t->ready = true;                             // from here on the destructor cleans up
    HIPCHK(hipStreamCreateWithFlags(&t->stream.s, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&t->ev_begin));
    HIPCHK(hipEventCreate(&t->ev_end));
    return t->total.reserve(sizeof(unsigned long long));
}

extern "C" int pk_trim_create(pk_trim **out, int device) {
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    if (device < 0 || device >= MAX_DEVICES) return fail(PK_ERR_ARG, "device ordinal %d out of range", device);
    *out = new pk_trim();
    (*out)->device = device;
    return PK_OK;
}

extern "C" void pk_trim_destroy(pk_trim *t) { delete t; }

extern "C" int pk_trim_set_cover(pk_trim *t, const uint8_t *cover, uint64_t n_bases, int min_qual_byte) {
    if (!t) return fail(PK_ERR_ARG, "null trimmer");
    if (t->fed || t->finished) return fail(PK_ERR_STATE, "the cover bits are set before the first feed");
    if (n_bases && !cover) return fail(PK_ERR_ARG, "null cover bits with %llu bases", (unsigned long long)n_bases);
    if (min_qual_byte < 0 || min_qual_byte > 255) return fail(PK_ERR_ARG, "the quality threshold byte must lie in 0 .. 255, got %d", min_qual_byte);
    if (n_bases >= (uint64_t)SIZE_MAX / 2u) return fail(PK_ERR_ARG, "%llu bases are beyond the address space", (unsigned long long)n_bases);
    t->have_cover = false;
    if (int rc = ensure_device(t)) return rc;
    const uint64_t n_bytes = (n_bases + 7u) / 8u;
    t->n_words = (n_bases + 31u) / 32u;
    if (t->n_words) {
        std::vector<uint32_t> words(t->n_words, 0u);         // the last word's bytes behind the bits stay zero
        memcpy(words.data(), cover, n_bytes);
        if (n_bases & 7u) reinterpret_cast<uint8_t *>(words.data())[n_bytes - 1u] &= (uint8_t)((1u << (n_bases & 7u)) - 1u);
        if (int rc = t->bits.reserve(t->n_words * sizeof(uint32_t))) return rc;
        if (int rc = bounce_copy(t->bits.p, words.data(), t->n_words * sizeof(uint32_t), true, t->device)) return rc;
    }
    t->n_bases = n_bases;
    t->tq = (uint32_t)min_qual_byte;
    t->have_cover = true;
    return PK_OK;
}

// The opening checks of both feeds; no kernel is launched, and nothing moves, when one of them fails.
static int feed_check(pk_trim *t, const void *text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, const uint64_t *out) {
    if (!t) return fail(PK_ERR_ARG, "null trimmer");
    if (!t->have_cover) return fail(PK_ERR_STATE, "pk_trim_set_cover comes before the first feed");
    if (t->finished) return fail(PK_ERR_STATE, "the stream is finished");
    if (n_bytes && !text) return fail(PK_ERR_ARG, "null text pointer");
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

// The kernels over dev_text and the read-back; out: TRIM_FIELDS * n_records words on the host.
static int run_feed(pk_trim *t, const uint8_t *dev_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, uint64_t *out) {
    if (n_records) {
        const uint64_t R = n_records;
        if (int rc = t->starts.reserve((R + 1u) * sizeof(uint64_t))) return rc;
        if (int rc = t->cnt.reserve(R * sizeof(uint64_t))) return rc;
        if (int rc = t->geo.reserve(R * TRIM_FIELDS * sizeof(uint64_t))) return rc;
        if (int rc = bounce_copy(t->starts.p, const_cast<uint64_t *>(starts), (R + 1u) * sizeof(uint64_t), true, t->device)) return rc;
        HIPCHK(hipEventRecord(t->ev_begin, t->stream));
        if (launch_trim(dev_text, t->starts.p, R, t->pos, t->tq, t->bits.p, t->n_words, t->valid, t->cnt.p, t->total.p, t->geo.p, t->stream))
            return fail(PK_ERR_HIP, "launching the trim kernels failed: %s", hipGetErrorString(hipGetLastError()));
        HIPCHK(hipEventRecord(t->ev_end, t->stream));
        unsigned long long total = 0;
        HIPCHK(hipMemcpyAsync(&total, t->total.p, sizeof total, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, t->ev_begin, t->ev_end));
        t->t_kernels += ms * 1e-3;
        if (int rc = bounce_copy(t->geo.p, out, R * TRIM_FIELDS * sizeof(uint64_t), false, t->device)) return rc;
        t->valid = total;
        for (uint64_t r = 0; r < R; r++) t->covered += out[(uint64_t)PK_TRIM_COVERED * R + r];
        t->records += R;
    }
    t->pos += n_bytes;
    t->fed = true;
    t->feeds++;
    return PK_OK;
}

extern "C" int pk_trim_feed(pk_trim *t, const uint8_t *host_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, uint64_t *out) {
    if (int rc = feed_check(t, host_text, n_bytes, starts, n_records, out)) return rc;
    if (n_records) {
        HIPCHK(hipSetDevice(t->device));
        if (int rc = t->text.reserve(n_bytes)) return rc;
        if (int rc = bounce_copy(t->text.p, const_cast<uint8_t *>(host_text), n_bytes, true, t->device)) return rc;
    }
    return run_feed(t, t->text.p, n_bytes, starts, n_records, out);
}

extern "C" int pk_trim_feed_device(pk_trim *t, const void *dev_text, uint64_t n_bytes, const uint64_t *starts, uint64_t n_records, uint64_t *out) {
    if (int rc = feed_check(t, dev_text, n_bytes, starts, n_records, out)) return rc;
    if (n_records) HIPCHK(hipSetDevice(t->device));
    return run_feed(t, (const uint8_t *)dev_text, n_bytes, starts, n_records, out);
}

extern "C" int pk_trim_finish(pk_trim *t, uint64_t totals_out[3]) {
    if (!t || !totals_out) return fail(PK_ERR_ARG, "null argument");
    if (!t->have_cover) return fail(PK_ERR_STATE, "pk_trim_set_cover comes first");
    t->finished = true;
    totals_out[0] = t->records;
    totals_out[1] = t->valid;
    totals_out[2] = t->covered;
    if (t->valid != t->n_bases)
        return fail(PK_ERR_STATE, "the stream holds %llu valid bases, the cover bits were made for %llu", (unsigned long long)t->valid,
                    (unsigned long long)t->n_bases);
    return PK_OK;
}

extern "C" int pk_trim_timings(pk_trim *t, double out[2]) {
    if (!t || !out) return fail(PK_ERR_ARG, "null argument");
    out[0] = t->t_kernels;
    out[1] = (double)t->feeds;
    return PK_OK;
}
