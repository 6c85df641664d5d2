// pk_select.hip -- the host layer of the record selector (pk_select_*, include/pykmer_hip.h): the records and the position of
// the stream, the device arrays of kmer_select.hip and the feeds through them.  The host keeps the offsets and a prefix sum
// of the kept bytes, so it knows the exact output of any stretch of the stream before a kernel runs: the capacity check
// costs no device work, every piece of a feed gets its place in the output in advance, and the device's own count is only
// compared with it.
#include "pk_host.h"

using namespace pk;

namespace {
constexpr uint64_t SEL_PIECE = 64ull << 20;      // a feed is cut into pieces of this many bytes (a multiple of the 16 KiB chunk)
}

struct pk_select {
    int device = 0;
    bool ready = false;                          // the device side exists (made by the first pk_select_set_records that passes its checks)
    bool have_records = false, fed = false, finished = false;
    // members are destroyed in reverse order of declaration, behind the destructor's wait: the buffers, then the stream
    Stream stream;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;         // around the kernels of one piece loop
    DevBuf<unsigned long long> starts, masks, sums, grand;
    DevBuf<uint8_t> keep, text, out;                         // text / out: device copies of host-fed pieces and of their output
    std::vector<uint64_t> h_starts, h_kept;                  // the offsets; h_kept[r] = kept bytes of the records before r (R + 1 each)
    std::vector<uint8_t> h_keep;
    uint64_t R = 0;
    uint64_t pos = 0, bytes_kept = 0, feeds = 0;
    double t_kernels = 0;

    ~pk_select() {
        if (!ready) return;
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        for (hipEvent_t e : {ev_begin, ev_end}) if (e) hipEventDestroy(e);
    }
    // the kept bytes at stream offsets below x
    uint64_t kept_before(uint64_t x) const {
        if (!R || x <= h_starts[0]) return 0;
        if (x >= h_starts[R]) return h_kept[R];
        const uint64_t r = (uint64_t)(std::upper_bound(h_starts.begin(), h_starts.end(), x) - h_starts.begin()) - 1u;   // starts[r] <= x < starts[r + 1]
        return h_kept[r] + (h_kept[r + 1] > h_kept[r] ? x - h_starts[r] : 0u);
    }
    uint64_t kept_in(uint64_t a, uint64_t b) const { return kept_before(b) - kept_before(a); }
};

static int ensure_device(pk_select *s) {
    HIPCHK(hipSetDevice(s->device));
    if (s->ready) return PK_OK;
    s->ready = true;                             // from here on the destructor cleans up
    HIPCHK(hipStreamCreateWithFlags(&s->stream.s, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&s->ev_begin));
    HIPCHK(hipEventCreate(&s->ev_end));
    return s->grand.reserve(sizeof(unsigned long long));
}

extern "C" int pk_select_create(pk_select **out, int device) {
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    if (device < 0 || device >= MAX_DEVICES) return fail(PK_ERR_ARG, "device ordinal %d out of range", device);
    *out = new pk_select();
    (*out)->device = device;
    return PK_OK;
}

extern "C" void pk_select_destroy(pk_select *s) { delete s; }

extern "C" int pk_select_set_records(pk_select *s, const uint64_t *starts, const uint8_t *keep, uint64_t n_records) {
    if (!s) return fail(PK_ERR_ARG, "null selector");
    if (s->fed || s->finished) return fail(PK_ERR_STATE, "the records are set before the first feed");
    if (n_records && (!starts || !keep)) return fail(PK_ERR_ARG, "null pointer with %llu records", (unsigned long long)n_records);
    if (n_records >= SIZE_MAX / 16) return fail(PK_ERR_ARG, "%llu records are beyond the address space", (unsigned long long)n_records);
    for (uint64_t r = 0; r < n_records; r++)
        if (starts[r + 1] < starts[r])
            return fail(PK_ERR_ARG, "the record offsets must not decrease: starts[%llu] = %llu is followed by %llu", (unsigned long long)r,
                        (unsigned long long)starts[r], (unsigned long long)starts[r + 1]);
    s->have_records = false;
    s->R = n_records;
    s->h_starts.assign(n_records + 1, 0);
    if (starts) std::copy(starts, starts + n_records + 1, s->h_starts.begin());
    s->h_keep.assign(keep, keep + n_records);
    s->h_kept.assign(n_records + 1, 0);
    for (uint64_t r = 0; r < n_records; r++) s->h_kept[r + 1] = s->h_kept[r] + (keep[r] ? starts[r + 1] - starts[r] : 0u);
    if (n_records) {
        if (int rc = ensure_device(s)) return rc;
        if (int rc = s->starts.reserve((n_records + 1) * sizeof(uint64_t))) return rc;
        if (int rc = s->keep.reserve(n_records)) return rc;
        if (int rc = bounce_copy(s->starts.p, s->h_starts.data(), (n_records + 1) * sizeof(uint64_t), true, s->device)) return rc;
        if (int rc = bounce_copy(s->keep.p, s->h_keep.data(), n_records, true, s->device)) return rc;
    }
    s->have_records = true;
    return PK_OK;
}

// The opening checks of both feeds.  *need: the bytes the feed emits.  PK_ERR_RECS_CAP leaves everything as it was.
static int feed_check(pk_select *s, const void *text, uint64_t n_bytes, void *out, uint64_t out_cap, uint64_t *n_out, uint64_t *need) {
    if (!s) return fail(PK_ERR_ARG, "null selector");
    if (!s->have_records) return fail(PK_ERR_STATE, "pk_select_set_records comes before the first feed");
    if (s->finished) return fail(PK_ERR_STATE, "the stream is finished");
    if (!n_out) return fail(PK_ERR_ARG, "null output pointer");
    if (n_bytes && !text) return fail(PK_ERR_ARG, "null text pointer");
    *need = s->kept_in(s->pos, s->pos + n_bytes);
    *n_out = *need;
    if (*need > out_cap)
        return fail(PK_ERR_RECS_CAP, "the feed keeps %llu bytes, capacity %llu", (unsigned long long)*need, (unsigned long long)out_cap);
    if (*need && !out) return fail(PK_ERR_ARG, "null output pointer");
    return PK_OK;
}

// One piece on the stream: text[0 .. n) at stream offset `at`, its `expected` kept bytes to dev_out.
static int queue_piece(pk_select *s, const uint8_t *dev_text, uint64_t at, uint64_t n, uint8_t *dev_out, uint64_t expected) {
    if (!expected) return PK_OK;                 // the host knows: no kernel has anything to write
    const uint32_t n_chunks = select_chunks(n);
    if (int rc = s->masks.reserve((size_t)n_chunks * 256u * sizeof(unsigned long long))) return rc;
    if (int rc = s->sums.reserve(((size_t)n_chunks + 1u) * sizeof(unsigned long long))) return rc;
    if (launch_select(s->starts.p, s->keep.p, s->R, dev_text, at, n, s->masks.p, s->sums.p, s->grand.p, dev_out, expected, s->stream))
        return fail(PK_ERR_HIP, "launching the select kernels failed: %s", hipGetErrorString(hipGetLastError()));
    return PK_OK;
}

static int begin_kernels(pk_select *s) {
    HIPCHK(hipMemsetAsync(s->grand.p, 0, sizeof(unsigned long long), s->stream));
    HIPCHK(hipEventRecord(s->ev_begin, s->stream));
    return PK_OK;
}

// waits for the pieces queued since begin_kernels; their kept bytes, as the device counted them, must be `expected`
static int end_kernels(pk_select *s, uint64_t expected) {
    unsigned long long got = 0;
    HIPCHK(hipEventRecord(s->ev_end, s->stream));
    HIPCHK(hipMemcpyAsync(&got, s->grand.p, sizeof got, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s->ev_begin, s->ev_end));
    s->t_kernels += ms * 1e-3;
    if (got != expected)
        return fail(PK_ERR_HIP, "the select kernels kept %llu bytes where the record offsets give %llu: nothing of the piece was written",
                    got, (unsigned long long)expected);
    return PK_OK;
}

static void advance(pk_select *s, uint64_t n_bytes, uint64_t need) {
    s->pos += n_bytes;
    s->bytes_kept += need;
    s->fed = true;
    s->feeds++;
}

extern "C" int pk_select_feed_device(pk_select *s, const void *dev_text, uint64_t n_bytes, void *dev_out, uint64_t out_cap, uint64_t *n_out) {
    uint64_t need = 0;
    if (int rc = feed_check(s, dev_text, n_bytes, dev_out, out_cap, n_out, &need)) return rc;
    if ((uintptr_t)dev_text & 15u) return fail(PK_ERR_ARG, "the device text must be 16-byte aligned");
    const uintptr_t t0 = (uintptr_t)dev_text, o0 = (uintptr_t)dev_out;
    if (need && t0 < o0 + need && o0 < t0 + n_bytes) return fail(PK_ERR_ARG, "the output overlaps the text");
    if (need) {
        HIPCHK(hipSetDevice(s->device));
        if (int rc = begin_kernels(s)) return rc;
        uint64_t emitted = 0;
        for (uint64_t off = 0; off < n_bytes; off += SEL_PIECE) {
            const uint64_t len = std::min(SEL_PIECE, n_bytes - off), k = s->kept_in(s->pos + off, s->pos + off + len);
            if (int rc = queue_piece(s, (const uint8_t *)dev_text + off, s->pos + off, len, (uint8_t *)dev_out + emitted, k)) return rc;
            emitted += k;
        }
        if (int rc = end_kernels(s, need)) return rc;
    }
    advance(s, n_bytes, need);
    return PK_OK;
}

extern "C" int pk_select_feed(pk_select *s, const uint8_t *host_text, uint64_t n_bytes, uint8_t *host_out, uint64_t out_cap, uint64_t *n_out) {
    uint64_t need = 0;
    if (int rc = feed_check(s, host_text, n_bytes, host_out, out_cap, n_out, &need)) return rc;
    if (need) {
        HIPCHK(hipSetDevice(s->device));
        uint64_t emitted = 0;
        for (uint64_t off = 0; off < n_bytes; off += SEL_PIECE) {
            const uint64_t len = std::min(SEL_PIECE, n_bytes - off), k = s->kept_in(s->pos + off, s->pos + off + len);
            if (!k) continue;                    // nothing of this piece is kept: it need not cross to the device
            if (int rc = s->text.reserve(len)) return rc;
            if (int rc = s->out.reserve(k)) return rc;
            if (int rc = bounce_copy(s->text.p, const_cast<uint8_t *>(host_text) + off, len, true, s->device)) return rc;
            if (int rc = begin_kernels(s)) return rc;
            if (int rc = queue_piece(s, s->text.p, s->pos + off, len, s->out.p, k)) return rc;
            if (int rc = end_kernels(s, k)) return rc;
            if (int rc = bounce_copy(s->out.p, host_out + emitted, k, false, s->device)) return rc;
            emitted += k;
        }
    }
    advance(s, n_bytes, need);
    return PK_OK;
}

extern "C" int pk_select_finish(pk_select *s, uint64_t totals_out[3]) {
    if (!s || !totals_out) return fail(PK_ERR_ARG, "null argument");
    if (!s->have_records) return fail(PK_ERR_STATE, "pk_select_set_records comes first");
    s->finished = true;
    uint64_t kept_recs = 0;
    if (s->R) {
        const uint64_t limit = std::min(s->pos, s->h_starts[s->R]);      // a record counts once its first byte has been fed
        const uint64_t upto = (uint64_t)(std::lower_bound(s->h_starts.begin(), s->h_starts.begin() + s->R, limit) - s->h_starts.begin());
        for (uint64_t r = 0; r < upto; r++) kept_recs += s->h_keep[r] != 0;
    }
    totals_out[0] = s->pos;
    totals_out[1] = s->bytes_kept;
    totals_out[2] = kept_recs;
    return PK_OK;
}

extern "C" int pk_select_timings(pk_select *s, double out[2]) {
    if (!s || !out) return fail(PK_ERR_ARG, "null argument");
    out[0] = s->t_kernels;
    out[1] = (double)s->feeds;
    return PK_OK;
}
