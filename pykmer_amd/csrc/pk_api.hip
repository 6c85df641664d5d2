// pk_api.hip -- host side of the C-ABI declared in include/pykmer_hip.h.
// Owns device memory, streams and events (every allocation of the library is made here) and sequences the kernels of the
// indexer (kmer_count.hip, kmer_pack.hip, kmer_fuse.hip, kmer_part.hip, fastq.hip), of the query path (kmer_query.hip, kmer_coords.hip) and of
// the merger (gram_scan.hip, gram_spectrum.hip, gram_occ.hip).  No kernel is defined in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pykmer_hip.h"
#include "pk_kernels.h"

using namespace pk;

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace pk { int set_error(int code, const std::string &msg) { g_err = msg; return code; } }   // for the other translation units

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return fail(PK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

extern "C" int pk_version(void) { return PK_ABI_VERSION; }

extern "C" int pk_last_error(char *buf, size_t n) {
    if (!buf || n == 0) return PK_ERR_ARG;
    snprintf(buf, n, "%s", g_err.c_str());
    return PK_OK;
}

extern "C" int pk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int pk_warm(int device) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(nullptr));                                // the context
    pk::part_set_attributes();                               // the code object (first use of a kernel symbol loads it)
    return PK_OK;
}

// tools.py:165-167: k > 0 and odd.  One indexer holds at most 2^34 addresses (a 16 GiB table): that is all of k <= 17; beyond
// (k = 19: 256 GiB, k = 21: 4 TiB -- README.md:51-52 marks both as never run) the address range is cut into 2^slice_bits
// slices and an indexer counts one of them.
static int check_k(int k, int slice_bits = 0, int slice_index = 0) {
    if (k <= 0 || (k % 2) == 0) return fail(PK_ERR_ARG, "kmer_len must be positive and odd (tools.py:165-167), got %d", k);
    if (k > 21) return fail(PK_ERR_ARG, "kmer_len %d not supported by the device path (max 21)", k);
    if (slice_bits < 0 || slice_bits > 2 * k || slice_bits > 16) return fail(PK_ERR_ARG, "bad number of address slices for kmer_len %d", k);
    if (2 * k - slice_bits > 34)
        return fail(PK_ERR_ARG, "kmer_len %d needs a table of 4^%d bytes; one indexer holds 2^34 (16 GiB): count it in %d address slices "
                                "(pk_indexer_create_slice)", k, k, 1 << (2 * k - 34));
    if (slice_index < 0 || slice_index >= (1 << slice_bits)) return fail(PK_ERR_ARG, "slice index %d outside 0..%d", slice_index, (1 << slice_bits) - 1);
    return PK_OK;
}

// n_slices as a power of two -> slice_bits, then check_k: what pk_indexer_create_slice and pk_diag_plan_slice accept
static int check_slices(int k, int n_slices, int slice_index, int *slice_bits_out) {
    int slice_bits = 0;
    while (slice_bits < 30 && (1 << slice_bits) < n_slices) slice_bits++;
    if (n_slices < 1 || (1 << slice_bits) != n_slices) return fail(PK_ERR_ARG, "the number of address slices must be a power of two, got %d", n_slices);
    *slice_bits_out = slice_bits;
    return check_k(k, slice_bits, slice_index);
}

// ================================================================== owned device memory =========
namespace {
// "Reserve exactly": nothing at all when the capacity suffices (the steady state of the timed path); otherwise the old
// block is freed FIRST and exactly `need` bytes are allocated.  The k = 17 indexer sits next to a 16 GiB table: these
// buffers can afford neither geometric growth nor the old and the new block side by side.  The contents are lost.
int reserve_exact(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return PK_OK;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIPCHK(hipMalloc(p, need));
    *cap = need;
    return PK_OK;
}

// One device allocation of T and its capacity in bytes.  Move-only; the destructor frees, and leaves g_err alone so that
// the message of the call that failed survives the clean-up.  Never a member of an object with static storage: the HIP
// runtime may be gone when static destructors run (Bouncer and GramCtx below keep raw pointers for that reason).
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { swap(o); return *this; }   // o's destructor frees what this held
    ~DevBuf() { if (p) hipFree(p); }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    int reserve(size_t need) { return reserve_exact((void **)&p, &bytes, need); }
    // "Grow and keep": a larger array with the old contents in front and zeros behind, filled on `s`; the host waits for
    // it, then the old array is freed.  The new one is released if a step fails.
    int grow_keep(size_t need, hipStream_t s) {
        if (need <= bytes) return PK_OK;
        DevBuf larger;
        int rc = larger.reserve(need);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(larger.p, 0, need, s));
        if (bytes) HIPCHK(hipMemcpyAsync(larger.p, p, bytes, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        swap(larger);
        return PK_OK;
    }
};
}  // namespace

// ================================================================== host <-> HBM copies =========
// The C-ABI takes plain (pageable) host buffers.  One hipMemcpy from pageable memory is a single thread bouncing
// the bytes through a small pinned buffer; here several host threads each own a pinned bounce buffer (two halves)
// and a stream, so page-touching memcpy and PCIe DMA of different pieces overlap and the link is what limits.
namespace {
constexpr int MAX_DEVICES = 64;
constexpr size_t BOUNCE_HALF = 8u << 20;
constexpr int MAX_COPY_THREADS = 16;
struct Bouncer {
    std::mutex mu;
    int threads = 0;
    uint8_t *pinned[MAX_COPY_THREADS] = {};
    hipStream_t stream[MAX_COPY_THREADS] = {};
    hipEvent_t ev[MAX_COPY_THREADS][2] = {};
};
Bouncer g_bounce[MAX_DEVICES];

int bouncer_for(int device, Bouncer **out) {
    if (device < 0 || device >= MAX_DEVICES) return fail(PK_ERR_ARG, "device ordinal %d out of range", device);
    Bouncer &b = g_bounce[device];
    static std::mutex init_mu;                             // several host threads may make their first copy at once
    std::lock_guard<std::mutex> init_lock(init_mu);
    if (!b.threads) {
        const char *env = getenv("PK_COPY_THREADS");
        int t = env ? atoi(env) : 8;
        t = std::max(1, std::min(t, MAX_COPY_THREADS));
        auto make = [&]() -> int {
            for (int i = 0; i < t; i++) {
                HIPCHK(hipHostMalloc((void **)&b.pinned[i], 2 * BOUNCE_HALF, hipHostMallocDefault));
                HIPCHK(hipStreamCreateWithFlags(&b.stream[i], hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&b.ev[i][0], hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&b.ev[i][1], hipEventDisableTiming));
            }
            return PK_OK;
        };
        if (int rc = make()) {                             // all or nothing: the next call starts from an empty context again
            for (int i = 0; i < t; i++) {
                if (b.pinned[i]) hipHostFree(b.pinned[i]);
                if (b.stream[i]) hipStreamDestroy(b.stream[i]);
                for (auto &e : b.ev[i]) if (e) hipEventDestroy(e);
                b.pinned[i] = nullptr; b.stream[i] = nullptr; b.ev[i][0] = b.ev[i][1] = nullptr;
            }
            return rc;
        }
        b.threads = t;
    }
    *out = &b;
    return PK_OK;
}

// to_device: host -> dev, else dev -> host.  Blocking.
int bounce_copy(void *dev, void *host, size_t n, bool to_device, int device) {
    if (n == 0) return PK_OK;
    HIPCHK(hipSetDevice(device));
    if (n < (4u << 20)) {
        HIPCHK(to_device ? hipMemcpy(dev, host, n, hipMemcpyHostToDevice) : hipMemcpy(host, dev, n, hipMemcpyDeviceToHost));
        return PK_OK;
    }
    Bouncer *b = nullptr;
    int rc = bouncer_for(device, &b);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(b->mu);
    const size_t n_pieces = (n + BOUNCE_HALF - 1) / BOUNCE_HALF;
    const int T = (int)std::min<size_t>((size_t)b->threads, n_pieces);
    std::vector<hipError_t> errs(T, hipSuccess);
    auto work = [&](int t) {
        hipError_t e = hipSetDevice(device);
        size_t pending_off[2] = {0, 0}, pending_len[2] = {0, 0};      // D2H: a half whose DMA is in flight and still has to reach the host buffer
        int h = 0;
        for (size_t p = (size_t)t; p < n_pieces && e == hipSuccess; p += (size_t)T, h ^= 1) {
            const size_t off = p * BOUNCE_HALF, len = std::min(BOUNCE_HALF, n - off);
            uint8_t *half = b->pinned[t] + (size_t)h * BOUNCE_HALF;
            if (to_device) {
                e = hipEventSynchronize(b->ev[t][h]);                  // the DMA that last read this half is done
                if (e != hipSuccess) break;
                memcpy(half, (const uint8_t *)host + off, len);
                e = hipMemcpyAsync((uint8_t *)dev + off, half, len, hipMemcpyHostToDevice, b->stream[t]);
                if (e == hipSuccess) e = hipEventRecord(b->ev[t][h], b->stream[t]);
            } else {
                if (pending_len[h]) {                                  // drain what this half held before reusing it
                    e = hipEventSynchronize(b->ev[t][h]);
                    if (e != hipSuccess) break;
                    memcpy((uint8_t *)host + pending_off[h], half, pending_len[h]);
                }
                e = hipMemcpyAsync(half, (const uint8_t *)dev + off, len, hipMemcpyDeviceToHost, b->stream[t]);
                if (e == hipSuccess) e = hipEventRecord(b->ev[t][h], b->stream[t]);
                pending_off[h] = off; pending_len[h] = len;
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream[t]);
        if (!to_device && e == hipSuccess)
            for (int q = 0; q < 2; q++)
                if (pending_len[q]) memcpy((uint8_t *)host + pending_off[q], b->pinned[t] + (size_t)q * BOUNCE_HALF, pending_len[q]);
        errs[t] = e;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    for (int t = 0; t < T; t++)
        if (errs[t] != hipSuccess) return fail(PK_ERR_HIP, "host <-> device copy failed: %s", hipGetErrorString(errs[t]));
    return PK_OK;
}
}  // namespace

// ================================================================== device buffers =============
extern "C" int pk_dev_alloc(void **dev_out, uint64_t n_bytes, int device) {
    if (!dev_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMalloc(dev_out, n_bytes + 64));            // slack: kernels read whole 16/32-byte words
    return PK_OK;
}
extern "C" int pk_dev_free(void *dev, int device) {
    if (!dev) return PK_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(dev));
    return PK_OK;
}
extern "C" int pk_dev_upload(void *dev_dst, const void *host_src, uint64_t n_bytes, int device) {
    if (n_bytes && (!dev_dst || !host_src)) return fail(PK_ERR_ARG, "null pointer");
    return bounce_copy(dev_dst, const_cast<void *>(host_src), n_bytes, true, device);
}
extern "C" int pk_dev_download(void *host_dst, const void *dev_src, uint64_t n_bytes, int device) {
    if (n_bytes && (!host_dst || !dev_src)) return fail(PK_ERR_ARG, "null pointer");
    return bounce_copy(const_cast<void *>(dev_src), host_dst, n_bytes, false, device);
}

extern "C" int pk_dev_mem_info(uint64_t *free_out, uint64_t *total_out, int device) {
    HIPCHK(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_out) *free_out = f;
    if (total_out) *total_out = t;
    return PK_OK;
}

// ================================================================== indexer ====================
// One counting stream on one device: the .kin image, the scratch of the structure pass (kmer_count.hip), the squeeze
// (kmer_pack.hip), the partition passes (kmer_fuse.hip, kmer_part.hip) and the FASTQ front end (fastq.hip), and the stream
// and events that order and time them.  Everything it holds is released by its destructor.
namespace {
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    ~Stream() { if (s) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

// the device events of a feed, by what they bracket on the stream
struct Events {
    hipEvent_t reset_begin = nullptr, reset_end = nullptr;         // ix_reset
    hipEvent_t scan_begin = nullptr, scan_end = nullptr;           // structure pass: chunk summaries and their scans
    hipEvent_t squeeze_begin = nullptr, squeeze_end = nullptr;
    hipEvent_t sort_begin = nullptr, sort_end = nullptr;           // walk + level-1 sort kernel (inside launch_partitioned)
    hipEvent_t part_end = nullptr;                                 // bucket layout and level 2 end here, the bucket count begins
    hipEvent_t bucket_end = nullptr;
    hipEvent_t final_begin = nullptr, final_end = nullptr;         // pk_indexer_finish
    hipEvent_t lookup_begin = nullptr, lookup_end = nullptr;       // query mode: the kernels of kmer_query.hip
    hipEvent_t coords_begin = nullptr, coords_end = nullptr;       // query mode with coordinates: the kernels of kmer_coords.hip
    Events() = default;
    Events(const Events &) = delete;
    ~Events() { for (hipEvent_t *e : all()) if (*e) hipEventDestroy(*e); }
    std::array<hipEvent_t *, 16> all() {
        return {&reset_begin, &reset_end, &scan_begin, &scan_end, &squeeze_begin, &squeeze_end, &sort_begin, &sort_end, &part_end, &bucket_end,
                &final_begin, &final_end, &lookup_begin, &lookup_end, &coords_begin, &coords_end};
    }
};
}  // namespace

struct pk_indexer {
    int k = 0, device = 0;
    int slice_bits = 0, slice_index = 0;   // the table holds addresses [slice_index, slice_index + 1) * 4^k / 2^slice_bits
    uint64_t n = 0;                  // table bytes: 4^k / 2^slice_bits
    // members are destroyed in reverse order of declaration, behind the destructor's wait: the buffers, then the events,
    // then the stream
    Stream stream;
    Events ev;
    DevBuf<uint8_t> table8;          // the .kin image
    // parser state + running totals, and the value histogram, side by side: one copy brings both to the host, one copy resets both
    struct Tail { Carry carry; unsigned long long hist[256]; FqCarry fq; };
    DevBuf<Tail> tail, tail0;          // tail0: the state of an empty stream (a reset is a device-to-device copy, no host wait)
    struct Pinned { Tail tail; uint32_t flags[4]; } *pin = nullptr;   // pinned landing zone of the small read-backs
    bool tail_on_host = false;         // pin->tail is what the device holds (the last feed brought it along with its flags)
    bool zero_timed = true;            // t_zero of the last reset has been read from its events
    DevBuf<unsigned long long> hist_rep;   // HIST_REPLICAS copies of one feed's histogram change (zero between feeds)
    DevBuf<DevRec> recs;
    DevBuf<L1> c_l1, c_l1s;
    DevBuf<L2> c_l2, c_l2s;
    DevBuf<LaneState> lane_state;      // per 64-byte piece: start state relative to its chunk
    DevBuf<PiecePack> packs;           // per 64-byte piece: its bases, classified and pushed together (structure pass -> squeeze pass)
    DevBuf<uint32_t> chunk_odd;        // per chunk: pieces that are not plain sequence text
    DevBuf<L1> t_l1;                   // scan scratch: one summary per 1024 chunks
    DevBuf<L2> t_l2;
    DevBuf<uint8_t> staging[2];        // device copies of host-fed pieces (one counted while the next uploads)
    uint64_t bytes_fed = 0, n_recs = 0;
    bool finished = false;
    double t_scan = 0, t_squeeze = 0, t_sort = 0, t_final = 0, t_zero = 0, t_part = 0, t_bucket = 0;
    int feeds = 0, relayouts = 0;
    uint64_t recounted = 0;                                // buckets whose byte counters wrapped and were counted again (k_bucket_count_bytes)
    bool table_fresh = true;         // no feed has written the u8 table since the last reset
    DevBuf<uint8_t> ws;              // workspace of the partition passes
    // FASTQ input (fastq.hip): each feed is turned into FASTA text in fq_out[fq_buf]; that text is counted by the next
    // feed (or by finish), whose read-back brings this feed's checks and totals along -- no wait of its own
    int format = PK_FORMAT_FASTA;
    bool fed = false;                  // bytes were fed since the last reset
    DevBuf<FqSum> fq_sums;
    DevBuf<FqState> fq_st;
    DevBuf<uint8_t> fq_out[2];
    int fq_buf = 0;
    uint64_t fq_pending = 0;           // FASTA bytes in fq_out[fq_buf ^ 1] not counted yet
    DevBuf<FqRec> fq_recs;
    uint64_t fq_need = 0;
    bool fq_failed = false;
    std::string fq_err;
    // query mode (pk_query_create): no table of its own; every valid window is looked up in the caller's tables and
    // tallied per record.  q_P, q_hits and q_depth are sized with the record array and grown with it (ensure_recs).
    bool query = false;
    std::vector<const uint8_t *> q_tables;                  // the caller's device tables; they stay across resets
    int q_min = 1, q_max = 255;
    DevBuf<unsigned long long> q_P;                         // P[r]: valid windows of the stream before record r
    DevBuf<unsigned long long> q_hits, q_depth;             // row-major [record][table]; with bins [bin][table]
    uint64_t q_windows = 0, q_p_done = 0;                   // valid windows / final entries of P before the next feed
    // bins (pk_query_set_bins): q_bin valid windows per accumulator row, 0 = one row per record.  q_Bf[r]: the rows before
    // record r, grown with q_P.  The rows a stream of `bytes` bytes and at most `cap` records can hold need no read-back:
    // every record adds at most one partial bin, and n bytes hold at most n windows.
    uint64_t q_bin = 0;
    DevBuf<unsigned long long> q_Bf;
    uint64_t q_n_bins = 0;                                  // after finish
    // coordinates (pk_query_set_coords): per row the position of the first base of its first window and one past the last
    // base of its last, sized and grown with q_hits.  q_pos: the position in the open record at the start of the next feed
    // (word q_pos_in) and where the feed's kernels leave the one at its end (the other word); q_cpos: one word per chunk.
    bool q_coords = false;
    DevBuf<unsigned long long> q_bin_start, q_bin_end, q_pos, q_cpos;
    int q_pos_in = 0;
    double t_coords = 0;
    uint64_t query_rows(uint64_t cap, uint64_t bytes) const { return q_bin ? bytes / q_bin + cap + 1 : cap; }

    uint64_t recs_cap() const { return recs.bytes / sizeof(DevRec); }
    uint64_t fq_recs_cap() const { return fq_recs.bytes / sizeof(FqRec); }
    ~pk_indexer() {
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        if (pin) hipHostFree(pin);
    }
};

static int ix_reset(pk_indexer *ix) {
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipEventRecord(ix->ev.reset_begin, ix->stream));
    // the first feed writes every slice of the u8 table itself (k_bucket_count, fresh); the table is only
    // zeroed if nothing gets fed at all (see pk_indexer_finish).  Nothing here waits for the device: the stream orders
    // the reset behind whatever is still running, and its duration is read at the next point that waits anyway.
    HIPCHK(hipMemcpyAsync(ix->tail.p, ix->tail0.p, sizeof(pk_indexer::Tail), hipMemcpyDeviceToDevice, ix->stream));
    ix->tail_on_host = false;
    if (ix->recs.p) HIPCHK(hipMemsetAsync(ix->recs.p, 0, ix->recs.bytes, ix->stream));
    for (DevBuf<unsigned long long> *b : {&ix->q_P, &ix->q_Bf, &ix->q_hits, &ix->q_depth, &ix->q_bin_start, &ix->q_bin_end, &ix->q_pos})
        if (b->p) HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, ix->stream));
    ix->q_windows = ix->q_p_done = 0;
    ix->q_bin = ix->q_n_bins = 0;
    ix->q_coords = false; ix->q_pos_in = 0; ix->t_coords = 0;
    HIPCHK(hipEventRecord(ix->ev.reset_end, ix->stream));
    ix->zero_timed = false;
    ix->t_zero = 0;
    ix->bytes_fed = ix->n_recs = 0;
    ix->finished = false;
    ix->table_fresh = true;
    ix->t_scan = ix->t_squeeze = ix->t_sort = ix->t_final = ix->t_part = ix->t_bucket = 0;
    ix->feeds = ix->relayouts = 0; ix->recounted = 0;
    ix->fed = false;
    ix->fq_pending = 0; ix->fq_need = 0; ix->fq_failed = false; ix->fq_err.clear();
    return PK_OK;
}

// after a wait on the stream: the duration of the last reset, if it has not been read yet
static void time_reset(pk_indexer *ix) {
    if (ix->zero_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ix->ev.reset_begin, ix->ev.reset_end) == hipSuccess) ix->t_zero = ms * 1e-3;
    ix->zero_timed = true;
}

// The stream totals, the value histogram and the FASTQ state to the host, behind everything queued so far; the host waits
// for it.  This is the wait of a feed: it also surfaces a kernel fault and makes the reset's events readable.
static int read_tail(pk_indexer *ix) {
    HIPCHK(hipMemcpyAsync(&ix->pin->tail, ix->tail.p, sizeof(pk_indexer::Tail), hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    HIPCHK(hipGetLastError());
    time_reset(ix);
    ix->tail_on_host = true;
    return PK_OK;
}

// the device tallies the values 1 .. 255 only: the zeros are the rest of the n addresses
static void hist_with_zeros(const unsigned long long *h, uint64_t n, uint64_t hist256_out[256]) {
    uint64_t nonzero = 0;
    for (int v = 1; v < 256; v++) { hist256_out[v] = h[v]; nonzero += h[v]; }
    hist256_out[0] = n - nonzero;
}

extern "C" void pk_indexer_destroy(pk_indexer *ix) { delete ix; }

static int create_indexer(pk_indexer **out, int k, int device, int slice_index, int n_slices, bool query);

extern "C" int pk_indexer_create(pk_indexer **out, int k, int device) { return create_indexer(out, k, device, 0, 1, false); }

extern "C" int pk_indexer_create_slice(pk_indexer **out, int k, int device, int slice_index, int n_slices) {
    return create_indexer(out, k, device, slice_index, n_slices, false);
}

extern "C" int pk_query_create(pk_indexer **out, int k, int device) {
    if (k > 17) return fail(PK_ERR_ARG, "a query takes kmer_len <= 17 (one unsliced table), got %d", k);
    return create_indexer(out, k, device, 0, 1, true);
}

static int create_indexer(pk_indexer **out, int k, int device, int slice_index, int n_slices, bool query) {
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    *out = nullptr;
    int slice_bits = 0;
    int rc = check_slices(k, n_slices, slice_index, &slice_bits);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<pk_indexer> ix(new pk_indexer());        // a failure below destroys what was built so far
    ix->k = k; ix->device = device; ix->slice_bits = slice_bits; ix->slice_index = slice_index;
    ix->n = 1ULL << (2 * k - slice_bits);
    ix->query = query;
    HIPCHK(hipStreamCreateWithFlags(&ix->stream.s, hipStreamNonBlocking));
    for (hipEvent_t *e : ix->ev.all()) HIPCHK(hipEventCreate(e));
    if (!query && (rc = ix->table8.reserve(std::max<uint64_t>(ix->n, 16)))) return rc;
    if ((rc = ix->tail.reserve(sizeof(pk_indexer::Tail)))) return rc;
    if ((rc = ix->tail0.reserve(sizeof(pk_indexer::Tail)))) return rc;
    HIPCHK(hipHostMalloc(&ix->pin, sizeof(*ix->pin), hipHostMallocDefault));
    {
        Carry c;
        memset(&c, 0, sizeof c);
        c.l1 = 8u | 1u | (LS_START << 1);                    // l1_state(LS_START)
        c.l2.flags = F_NONID | F_PRESET | F_BRK;             // l2_state(0, 0, 0, 0)
        HIPCHK(hipMemset(ix->tail0.p, 0, sizeof(pk_indexer::Tail)));
        HIPCHK(hipMemcpy(&ix->tail0.p->carry, &c, sizeof c, hipMemcpyHostToDevice));
        FqCarry q;
        memset(&q, 0, sizeof q);
        q.st.ws = q.in.ws = 1;                               // the open line (none yet) holds no text
        q.err = q.trail = ~0ull;
        q.prev4 = q.prev4_in = 0x0a0a0a0au;                  // before the stream: line terminators
        HIPCHK(hipMemcpy(&ix->tail0.p->fq, &q, sizeof q, hipMemcpyHostToDevice));
    }
    if ((rc = ix->hist_rep.reserve((size_t)HIST_REPLICAS * 256 * sizeof(unsigned long long)))) return rc;
    HIPCHK(hipMemset(ix->hist_rep.p, 0, ix->hist_rep.bytes));
    // room for the records of small inputs from the start: the squeeze pass checks the capacity itself (see feed_piece)
    if ((rc = ix->recs.reserve(4096 * sizeof(DevRec)))) return rc;
    if (query && (rc = ix->q_P.reserve(4096 * sizeof(unsigned long long)))) return rc;
    part_set_attributes();                               // dynamic-LDS opt-ins, once per process and device
    if ((rc = ix_reset(ix.get()))) return rc;
    *out = ix.release();
    return PK_OK;
}

extern "C" int pk_indexer_reset(pk_indexer *ix) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    return ix_reset(ix);
}

// the scratch of the structure pass for a feed of n_chunks chunks
static int ensure_chunks(pk_indexer *ix, uint32_t n_chunks) {
    const size_t n = n_chunks;
    int rc;
    if ((rc = ix->c_l1.reserve(n * sizeof(L1)))) return rc;
    if ((rc = ix->c_l1s.reserve(n * sizeof(L1)))) return rc;
    if ((rc = ix->c_l2.reserve(n * sizeof(L2)))) return rc;
    if ((rc = ix->c_l2s.reserve(n * sizeof(L2)))) return rc;
    if ((rc = ix->lane_state.reserve(n * WG * sizeof(LaneState)))) return rc;
    if ((rc = ix->packs.reserve(n * WG * sizeof(PiecePack)))) return rc;
    if ((rc = ix->chunk_odd.reserve(n * sizeof(uint32_t)))) return rc;
    if ((rc = ix->t_l1.reserve((n / 1024 + 1) * sizeof(L1)))) return rc;
    return ix->t_l2.reserve((n / 1024 + 1) * sizeof(L2));
}

// Binned query: the accumulators hold the rows that `bytes` bytes of stream and recs_cap() records can make (contents
// kept, the rest zero).  They grow by half at least, so that a long stream does not move them with every feed.
static int ensure_bin_rows(pk_indexer *ix, uint64_t bytes) {
    if (!ix->q_bin) return PK_OK;
    const uint64_t rows = ix->query_rows(ix->recs_cap(), bytes);
    const size_t row = ix->q_tables.size() * sizeof(unsigned long long);
    if (rows > SIZE_MAX / 2 / row)
        return fail(PK_ERR_ARG, "bins of %llu windows: %llu rows of %zu tables are beyond the address space; take larger bins",
                    (unsigned long long)ix->q_bin, (unsigned long long)rows, ix->q_tables.size());
    for (DevBuf<unsigned long long> *b : {&ix->q_hits, &ix->q_depth}) {
        if (rows * row <= b->bytes) continue;
        const size_t want = std::max<size_t>(rows * row, b->bytes + b->bytes / 2);
        const int rc = b->grow_keep(want, ix->stream);
        if (rc) {
            (void)hipGetLastError();
            const std::string why = g_err;
            return fail(rc, "bins of %llu windows need two accumulators of %zu bytes (%llu rows, %zu tables); take larger bins: %s",
                        (unsigned long long)ix->q_bin, want, (unsigned long long)rows, ix->q_tables.size(), why.c_str());
        }
    }
    if (!ix->q_coords) return PK_OK;
    for (DevBuf<unsigned long long> *b : {&ix->q_bin_start, &ix->q_bin_end}) {
        if (rows * sizeof(unsigned long long) <= b->bytes) continue;
        const size_t want = std::max<size_t>(rows * sizeof(unsigned long long), b->bytes + b->bytes / 2);
        const int rc = b->grow_keep(want, ix->stream);
        if (rc) {
            (void)hipGetLastError();
            const std::string why = g_err;
            return fail(rc, "bins of %llu windows need two coordinate arrays of %zu bytes (%llu rows); take larger bins: %s",
                        (unsigned long long)ix->q_bin, want, (unsigned long long)rows, why.c_str());
        }
    }
    return PK_OK;
}

// the sizing rules stay with the callers: the capacities the two record arrays reach are part of the retry behaviour
static int ensure_recs(pk_indexer *ix, uint64_t need) {
    if (need <= ix->recs_cap()) return PK_OK;
    const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(1024, ix->recs_cap() * 2));
    int rc = ix->recs.grow_keep(cap * sizeof(DevRec), ix->stream);
    if (rc || !ix->query) return rc;
    // query mode: the window prefix and the accumulators grow with the record array and keep what they hold
    const size_t row = ix->q_tables.size() * sizeof(unsigned long long);
    if ((rc = ix->q_P.grow_keep(cap * sizeof(unsigned long long), ix->stream))) return rc;
    if (ix->q_bin) return ix->q_Bf.grow_keep(cap * sizeof(unsigned long long), ix->stream);   // the rows: ensure_bin_rows
    if ((rc = ix->q_hits.grow_keep(cap * row, ix->stream))) return rc;
    return ix->q_depth.grow_keep(cap * row, ix->stream);
}

// one feed of at most FEED_MAX bytes: structure pass -> squeeze -> bucket layout -> fused k-mer assembly + level-1
// sort -> level 2 -> bucket count.  Record positions are 32-bit: both bucket areas (their capacity + the dump tile) must
// end below 2^32 records.  The worst plan is k = 17 (2^18 final buckets x 4104 records of fixed slack + 25 % on the
// estimate): 2 GiB of text -> capacity2 = 3.76e9.  feed_piece checks the plan it actually got and refuses otherwise.
// 32-bit k-mers (k <= 15): 1 GiB pieces, record positions below 2^31 -- their sort kernels store through 32-bit byte
// offsets (part_common.h: OFF32).
static const uint64_t FEED_MAX = 2ULL << 30;
static uint64_t feed_max_for(int k) { return k <= 15 ? (1ULL << 30) : FEED_MAX; }

static bool plan_fits_u32(const PartPlan &pl) {
    const uint64_t lim = (pl.k <= 15 ? (1ULL << 31) : (1ULL << 32)) - (16384 + 64);   // the dump tile behind the buckets (part_common.h: TILE)
    return pl.capacity1 < lim && pl.capacity2 < lim;
}

// diagnostics (include/pykmer_hip.h): the partition plan of one feed of n_bytes at kmer_len k
extern "C" int pk_diag_plan(int k, uint64_t n_bytes, uint64_t out[8]) {
    if (!out) return fail(PK_ERR_ARG, "null output");
    int rc = check_k(k, k > 17 ? 2 * k - 34 : 0, 0);
    if (rc) return rc;
    if (n_bytes == 0) n_bytes = feed_max_for(k);
    const PartPlan pl = make_part_plan((uint32_t)k, n_bytes, k > 17 ? (uint32_t)(2 * k - 34) : 0u, 0u);
    out[0] = feed_max_for(k); out[1] = pl.capacity1; out[2] = pl.capacity2; out[3] = pl.B1; out[4] = pl.B2; out[5] = pl.fb_bits;
    out[6] = pl.n_chunks; out[7] = plan_fits_u32(pl) ? 1 : 0;
    return PK_OK;
}

// the same for one of n_slices address slices, with the choices the launchers make on top of the plan
extern "C" int pk_diag_plan_slice(int k, int n_slices, uint64_t n_bytes, uint64_t out[16]) {
    if (!out) return fail(PK_ERR_ARG, "null output");
    int slice_bits = 0;
    int rc = check_slices(k, n_slices, 0, &slice_bits);
    if (rc) return rc;
    if (n_bytes == 0) n_bytes = feed_max_for(k);
    const PartPlan pl = make_part_plan((uint32_t)k, n_bytes, (uint32_t)slice_bits, 0u);
    out[0] = pl.addr_bits; out[1] = pl.fb_bits; out[2] = pl.b1; out[3] = pl.b2; out[4] = pl.sample_stride; out[5] = pl.n_tally;
    out[6] = pl.sample2; out[7] = pl.n_chunks; out[8] = walk_sort_variant(pl); out[9] = bucket_count_kernel(pl, n_bytes);
    out[10] = bucket_split(pl, n_bytes); out[11] = pl.B1; out[12] = pl.B2; out[13] = pl.capacity1; out[14] = pl.capacity2;
    out[15] = plan_fits_u32(pl) ? 1 : 0;
    return PK_OK;
}

static int query_feed_piece(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes);

static int feed_piece(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes) {
    if (ix->query) return query_feed_piece(ix, f, n_bytes);
    const uint32_t n_chunks = (uint32_t)((n_bytes + CHUNK - 1) / CHUNK);
    int rc = ensure_chunks(ix, n_chunks);
    if (rc) return rc;
    PartPlan pl = make_part_plan((uint32_t)ix->k, n_bytes, (uint32_t)ix->slice_bits, (uint32_t)ix->slice_index);
    if (!plan_fits_u32(pl)) return fail(PK_ERR_ARG, "feed of %llu bytes needs record positions beyond 2^32 (internal limit); split it", (unsigned long long)n_bytes);
    if ((rc = part_plan_check(pl, n_bytes))) return rc;
    if ((rc = ix->ws.reserve(part_workspace(pl, n_bytes)))) return rc;
    PartBuffers pb;
    part_workspace(pl, n_bytes, ix->ws.p, &pb);
    Carry *carry = &ix->tail.p->carry;
    const Events &ev = ix->ev;
    // Nothing between here and the last kernel of the feed waits for the device: the record array was sized from what the
    // feeds so far held (ensure_recs below, after the feed), the squeeze pass checks that against the count the structure
    // pass leaves in `carry` and backs out if it does not fit (flags[0] = 2), the sorts back out if a sampled bucket
    // room does not hold (flags[0] = 1), and the host reads flags + record count once, behind the last kernel.  Every
    // kernel behind the squeeze returns at once when it finds flags[0] raised (the workspace then still holds an earlier
    // feed's squeezed text), so a 2 reaches the host as a 2, whatever that text would have done to the sampled layout.
    HIPCHK(hipEventRecord(ev.scan_begin, ix->stream));
    launch_chunk_l1(f, n_bytes, ix->c_l1.p, n_chunks, ix->stream);
    launch_scan_l1(ix->c_l1.p, n_chunks, carry, ix->c_l1s.p, ix->t_l1.p, pb.signals, ix->stream);
    launch_chunk_l2(f, n_bytes, ix->c_l1s.p, ix->c_l2.p, ix->lane_state.p, ix->packs.p, ix->chunk_odd.p, n_chunks, (uint32_t)ix->k, ix->stream);
    launch_scan_l2(ix->c_l2.p, n_chunks, carry, ix->c_l2s.p, ix->t_l2.p, (uint32_t)ix->k, ix->stream);
    HIPCHK(hipEventRecord(ev.scan_end, ix->stream));
    bool squeeze = true;
    uint64_t squeezed_cap = 0;                               // record slots the last squeeze of this feed ran with
    uint32_t stride = pl.sample_stride;
    for (int attempt = 0;; attempt++) {
        if (attempt) HIPCHK(hipMemsetAsync(pb.signals, 0, sizeof(PartSignals), ix->stream));   // the scan kernel zeroed them for the first attempt
        if (squeeze) {
            squeezed_cap = ix->recs_cap();
            HIPCHK(hipEventRecord(ev.squeeze_begin, ix->stream));
            launch_squeeze(pl, pb, f, n_bytes, ix->bytes_fed, ix->lane_state.p, ix->packs.p, ix->c_l2s.p, ix->chunk_odd.p, ix->recs.p, squeezed_cap, carry,
                           ix->stream);
            if (ix->k > 17) launch_deep_tail(pl, pb, carry, ix->stream);
            HIPCHK(hipEventRecord(ev.squeeze_end, ix->stream));
        }
        // the level-1 buckets are laid out from a sample of the slots; if one of them runs out of room every later kernel
        // returns untouched (flags[0] = 1) and the passes behind the squeeze are repeated with exact sizes -- on the text
        // the squeeze of this feed left, so only once that squeeze has run in full (flags[0] = 2 is handled first)
        if ((rc = launch_partitioned(pl, pb, ix->c_l2s.p, n_bytes, stride, carry, ix->table8.p, ix->tail.p->hist, ix->hist_rep.p, ix->table_fresh,
                                     {ev.sort_begin, ev.sort_end, ev.part_end}, ix->stream)))
            return rc;
        HIPCHK(hipEventRecord(ev.bucket_end, ix->stream));
        volatile uint32_t *got = ix->pin->flags;
        // what the host needs of the feed, in two small copies behind the last kernel: the flags, and the stream totals +
        // value histogram (pk_indexer_finish then has nothing left to fetch)
        HIPCHK(hipMemcpyAsync(ix->pin->flags, pb.flags, sizeof ix->pin->flags, hipMemcpyDeviceToHost, ix->stream));
        if ((rc = read_tail(ix))) return rc;
        if (!got[0]) { ix->recounted += got[1]; break; }
        if (attempt >= 3) return fail(PK_ERR_HIP, "the feed's layout did not settle (internal error, flag %u)", got[0]);
        if (got[0] == 2u) {                                  // more records than the array holds: grow it, squeeze again
            rc = ensure_recs(ix, ix->pin->tail.carry.n_recs);
            if (rc) return rc;
            squeeze = true;
        } else {                                             // a bucket outgrew its sampled room: lay out again, exactly
            if (stride == 1) return fail(PK_ERR_HIP, "level-1 buckets overflowed an exact layout (internal error)");
            stride = 1;
            squeeze = false;
            ix->relayouts++;
        }
    }
    // the text counted above is this feed's only if its last squeeze had room for every record (it backs out otherwise)
    if (ix->pin->tail.carry.n_recs > squeezed_cap)
        return fail(PK_ERR_HIP, "feed counted without its squeeze: %llu records, %llu slots (internal error)",
                    (unsigned long long)ix->pin->tail.carry.n_recs, (unsigned long long)squeezed_cap);
    const uint64_t recs_before = ix->n_recs;
    ix->n_recs = ix->pin->tail.carry.n_recs;
    // room for the next feed's records before it arrives: as many again as this feed brought, and then some
    rc = ensure_recs(ix, ix->n_recs + 2 * (ix->n_recs - recs_before) + 1024);
    if (rc) return rc;
    ix->table_fresh = false;
    float scan = 0, squeeze_ms = 0, part = 0, bucket = 0, sort = 0;
    HIPCHK(hipEventElapsedTime(&scan, ev.scan_begin, ev.scan_end));
    HIPCHK(hipEventElapsedTime(&squeeze_ms, ev.squeeze_begin, ev.squeeze_end));
    HIPCHK(hipEventElapsedTime(&part, ev.squeeze_end, ev.part_end));
    HIPCHK(hipEventElapsedTime(&bucket, ev.part_end, ev.bucket_end));
    HIPCHK(hipEventElapsedTime(&sort, ev.sort_begin, ev.sort_end));
    ix->t_scan += scan * 1e-3; ix->t_squeeze += squeeze_ms * 1e-3; ix->t_part += part * 1e-3; ix->t_bucket += bucket * 1e-3; ix->t_sort += sort * 1e-3;
    ix->feeds++;
    ix->bytes_fed += n_bytes;
    return PK_OK;
}

// One feed of a query indexer: the structure pass and the squeeze as above, then the lookup kernels (kmer_query.hip) where
// feed_piece runs launch_partitioned.  There is no sampled layout, so the only flag is 2 (the squeeze backed out): the
// record array, the window prefix and the accumulators grow, and the squeeze and the lookups run again.  With bins the
// accumulators are sized before the kernels run for the rows the stream can hold after this feed (ensure_bin_rows).
static int query_feed_piece(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes) {
    if (ix->q_tables.empty()) return fail(PK_ERR_STATE, "pk_query_set_tables comes before the first feed");
    const uint32_t n_chunks = (uint32_t)((n_bytes + CHUNK - 1) / CHUNK);
    int rc = ensure_chunks(ix, n_chunks);
    if (rc) return rc;
    const PartPlan pl = make_part_plan((uint32_t)ix->k, n_bytes, 0u, 0u);   // the squeeze's launch shape; nothing is partitioned
    if ((rc = ix->ws.reserve(query_workspace(n_chunks)))) return rc;
    PartBuffers pb;
    QueryBuffers qb;
    query_workspace(n_chunks, ix->ws.p, &pb, &qb);
    Carry *carry = &ix->tail.p->carry;
    const Events &ev = ix->ev;
    const uint32_t N = (uint32_t)ix->q_tables.size();
    if ((rc = ensure_bin_rows(ix, ix->bytes_fed + n_bytes))) return rc;
    if (ix->q_coords && (rc = ix->q_cpos.reserve((size_t)n_chunks * sizeof(unsigned long long)))) return rc;
    HIPCHK(hipEventRecord(ev.scan_begin, ix->stream));
    launch_chunk_l1(f, n_bytes, ix->c_l1.p, n_chunks, ix->stream);
    launch_scan_l1(ix->c_l1.p, n_chunks, carry, ix->c_l1s.p, ix->t_l1.p, pb.signals, ix->stream);
    launch_chunk_l2(f, n_bytes, ix->c_l1s.p, ix->c_l2.p, ix->lane_state.p, ix->packs.p, ix->chunk_odd.p, n_chunks, (uint32_t)ix->k, ix->stream);
    launch_scan_l2(ix->c_l2.p, n_chunks, carry, ix->c_l2s.p, ix->t_l2.p, (uint32_t)ix->k, ix->stream);
    HIPCHK(hipEventRecord(ev.scan_end, ix->stream));
    uint64_t squeezed_cap = 0;
    for (int attempt = 0;; attempt++) {
        if (attempt) HIPCHK(hipMemsetAsync(pb.signals, 0, sizeof(PartSignals), ix->stream));
        squeezed_cap = ix->recs_cap();
        HIPCHK(hipEventRecord(ev.squeeze_begin, ix->stream));
        launch_squeeze(pl, pb, f, n_bytes, ix->bytes_fed, ix->lane_state.p, ix->packs.p, ix->c_l2s.p, ix->chunk_odd.p, ix->recs.p, squeezed_cap, carry,
                       ix->stream);
        HIPCHK(hipEventRecord(ev.squeeze_end, ix->stream));
        HIPCHK(hipEventRecord(ev.lookup_begin, ix->stream));
        launch_query_scan(pl, pb, qb, ix->c_l2s.p, ix->q_windows, ix->recs.p, carry, ix->q_p_done, ix->q_P.p, ix->q_Bf.p, ix->q_bin, ix->stream);
        for (uint32_t t0 = 0; t0 < N; t0 += QUERY_MAX_TABLES)
            launch_query_lookup(pl, pb, qb, ix->c_l2s.p, ix->q_P.p, ix->q_Bf.p, ix->q_bin, carry, ix->q_tables.data() + t0, std::min(QUERY_MAX_TABLES, N - t0), N, t0,
                                (uint32_t)ix->q_min, (uint32_t)ix->q_max, ix->q_hits.p, ix->q_depth.p, ix->stream);
        HIPCHK(hipEventRecord(ev.lookup_end, ix->stream));
        if (ix->q_coords) {
            // behind launch_query_scan (slot_first, P, Bf) and on the rows ensure_bin_rows sized; a repeated attempt starts
            // from the same q_pos word: the words change roles only once the feed has settled
            HIPCHK(hipEventRecord(ev.coords_begin, ix->stream));
            launch_query_coords(pl, pb, qb, f, n_bytes, ix->lane_state.p, ix->packs.p, ix->c_l2s.p, ix->chunk_odd.p, ix->recs.p, ix->q_P.p, ix->q_Bf.p,
                                ix->q_bin, ix->q_cpos.p, ix->q_pos.p + ix->q_pos_in, ix->q_pos.p + (ix->q_pos_in ^ 1), ix->q_bin_start.p, ix->q_bin_end.p,
                                ix->q_bin_start.bytes / sizeof(unsigned long long), ix->stream);
            HIPCHK(hipEventRecord(ev.coords_end, ix->stream));
        }
        HIPCHK(hipGetLastError());
        volatile uint32_t *got = ix->pin->flags;
        HIPCHK(hipMemcpyAsync(ix->pin->flags, pb.flags, sizeof ix->pin->flags, hipMemcpyDeviceToHost, ix->stream));
        if ((rc = read_tail(ix))) return rc;
        if (!got[0]) break;
        if (got[0] != 2u || attempt >= 3) return fail(PK_ERR_HIP, "the query feed did not settle (internal error, flag %u)", got[0]);
        if ((rc = ensure_recs(ix, ix->pin->tail.carry.n_recs))) return rc;
        if ((rc = ensure_bin_rows(ix, ix->bytes_fed + n_bytes))) return rc;
    }
    if (ix->pin->tail.carry.n_recs > squeezed_cap)
        return fail(PK_ERR_HIP, "feed looked up without its squeeze: %llu records, %llu slots (internal error)",
                    (unsigned long long)ix->pin->tail.carry.n_recs, (unsigned long long)squeezed_cap);
    const uint64_t recs_before = ix->n_recs;
    ix->n_recs = ix->pin->tail.carry.n_recs;
    ix->q_windows = ix->pin->tail.carry.num_kmers;
    ix->q_p_done = ix->n_recs;
    if ((rc = ensure_recs(ix, ix->n_recs + 2 * (ix->n_recs - recs_before) + 1024))) return rc;
    if ((rc = ensure_bin_rows(ix, ix->bytes_fed + n_bytes))) return rc;
    float scan = 0, squeeze_ms = 0, lookup = 0;
    HIPCHK(hipEventElapsedTime(&scan, ev.scan_begin, ev.scan_end));
    HIPCHK(hipEventElapsedTime(&squeeze_ms, ev.squeeze_begin, ev.squeeze_end));
    HIPCHK(hipEventElapsedTime(&lookup, ev.lookup_begin, ev.lookup_end));
    ix->t_scan += scan * 1e-3; ix->t_squeeze += squeeze_ms * 1e-3; ix->t_part += lookup * 1e-3;
    if (ix->q_coords) {
        float coords = 0;
        HIPCHK(hipEventElapsedTime(&coords, ev.coords_begin, ev.coords_end));
        ix->t_coords += coords * 1e-3;
        ix->q_pos_in ^= 1;                                   // the position behind this feed is the next feed's start
    }
    ix->feeds++;
    ix->bytes_fed += n_bytes;
    return PK_OK;
}

extern "C" int pk_query_set_tables(pk_indexer *ix, const void *const *dev_tables, int N, int min_count, int max_count) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (ix->fed || ix->finished) return fail(PK_ERR_STATE, "the tables are set before the first feed (reset the indexer first)");
    if (N < 1 || !dev_tables) return fail(PK_ERR_ARG, "need at least one table");
    if (min_count < 1 || max_count > 255 || min_count > max_count) return fail(PK_ERR_ARG, "count window must satisfy 1 <= min <= max <= 255, got %d-%d", min_count, max_count);
    for (int i = 0; i < N; i++)
        if (!dev_tables[i]) return fail(PK_ERR_ARG, "table %d is a null pointer", i);
    HIPCHK(hipSetDevice(ix->device));
    ix->q_tables.assign((const uint8_t *const *)dev_tables, (const uint8_t *const *)dev_tables + N);
    ix->q_min = min_count; ix->q_max = max_count;
    // the accumulators of an empty stream for this many tables (a reset zeroed them, but N may have changed)
    const size_t need = ix->recs_cap() * (size_t)N * sizeof(unsigned long long);
    for (DevBuf<unsigned long long> *b : {&ix->q_hits, &ix->q_depth}) {
        int rc = b->reserve(need);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, ix->stream));
    }
    return PK_OK;
}

extern "C" int pk_query_set_bins(pk_indexer *ix, uint64_t bin_windows) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (ix->q_tables.empty()) return fail(PK_ERR_STATE, "pk_query_set_tables comes before pk_query_set_bins");
    if (ix->fed || ix->finished) return fail(PK_ERR_STATE, "the bins are set before the first feed (reset the indexer first)");
    HIPCHK(hipSetDevice(ix->device));
    ix->q_bin = bin_windows;
    ix->q_coords = false;                                    // pk_query_set_coords comes after the bins
    if (!bin_windows) return PK_OK;
    // Bf beside P; a reset zeroed what was there, a new array is zeroed here
    const int rc = ix->q_Bf.grow_keep(ix->recs_cap() * sizeof(unsigned long long), ix->stream);
    return rc ? rc : ensure_bin_rows(ix, 0);
}

extern "C" int pk_query_set_coords(pk_indexer *ix, int on) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (!ix->q_bin) return fail(PK_ERR_STATE, "pk_query_set_bins with bins of at least one window comes before pk_query_set_coords");
    if (ix->fed || ix->finished) return fail(PK_ERR_STATE, "the coordinates are set before the first feed (reset the indexer first)");
    HIPCHK(hipSetDevice(ix->device));
    ix->q_coords = on != 0;
    if (!ix->q_coords) return PK_OK;
    // the two position words; a reset zeroed what was there, a new array is zeroed here
    const int rc = ix->q_pos.grow_keep(2 * sizeof(unsigned long long), ix->stream);
    return rc ? rc : ensure_bin_rows(ix, 0);
}

// the rows of a finished binned stream: the last record's bins are not in Bf
static int query_count_bins(pk_indexer *ix) {
    ix->q_n_bins = 0;
    if (!ix->q_bin || !ix->n_recs) return PK_OK;
    unsigned long long bf = 0;
    DevRec last;
    HIPCHK(hipMemcpy(&bf, ix->q_Bf.p + (ix->n_recs - 1), sizeof bf, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&last, ix->recs.p + (ix->n_recs - 1), sizeof last, hipMemcpyDeviceToHost));
    ix->q_n_bins = bf + (last.n_valid ? (last.n_valid - 1) / ix->q_bin + 1 : 0);
    return PK_OK;
}

extern "C" int pk_query_bin_count(pk_indexer *ix, uint64_t *n_bins_out) {
    if (!ix || !n_bins_out) return fail(PK_ERR_ARG, "null argument");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (!ix->q_bin) return fail(PK_ERR_STATE, "the indexer tallies per record (pk_query_set_bins)");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    *n_bins_out = ix->q_n_bins;
    return PK_OK;
}

extern "C" int pk_query_bin_results(pk_indexer *ix, uint64_t *hits_out, uint64_t *depth_out, uint64_t *bin_first_out, uint64_t bins_cap,
                                    uint64_t recs_cap) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (!ix->q_bin) return fail(PK_ERR_STATE, "the indexer tallies per record (pk_query_set_bins); use pk_query_results");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    if (ix->n_recs > recs_cap || ix->q_n_bins > bins_cap)
        return fail(PK_ERR_RECS_CAP, "%llu bins and %llu records, capacities %llu and %llu", (unsigned long long)ix->q_n_bins,
                    (unsigned long long)ix->n_recs, (unsigned long long)bins_cap, (unsigned long long)recs_cap);
    if (!bin_first_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    if (ix->n_recs) HIPCHK(hipMemcpy(bin_first_out, ix->q_Bf.p, ix->n_recs * sizeof(uint64_t), hipMemcpyDeviceToHost));
    bin_first_out[ix->n_recs] = ix->q_n_bins;
    if (ix->q_n_bins == 0) return PK_OK;
    if (!hits_out || !depth_out) return fail(PK_ERR_ARG, "null output pointer");
    const size_t n = ix->q_n_bins * ix->q_tables.size() * sizeof(uint64_t);
    HIPCHK(hipMemcpy(hits_out, ix->q_hits.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(depth_out, ix->q_depth.p, n, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_bin_coords(pk_indexer *ix, uint64_t *start_out, uint64_t *end_out, uint64_t bins_cap) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (!ix->q_coords) return fail(PK_ERR_STATE, "the indexer keeps no coordinates (pk_query_set_coords)");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    if (ix->q_n_bins > bins_cap)
        return fail(PK_ERR_RECS_CAP, "%llu bins, capacity %llu", (unsigned long long)ix->q_n_bins, (unsigned long long)bins_cap);
    if (ix->q_n_bins == 0) return PK_OK;
    if (!start_out || !end_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    const size_t n = ix->q_n_bins * sizeof(uint64_t);
    HIPCHK(hipMemcpy(start_out, ix->q_bin_start.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(end_out, ix->q_bin_end.p, n, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_query_results(pk_indexer *ix, uint64_t *hits_out, uint64_t *depth_out, uint64_t recs_cap) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (!ix->query) return fail(PK_ERR_STATE, "not a query indexer (pk_query_create)");
    if (ix->q_bin) return fail(PK_ERR_STATE, "the indexer tallies per bin (pk_query_set_bins); use pk_query_bin_results");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    if (ix->n_recs > recs_cap) return fail(PK_ERR_RECS_CAP, "%llu records, capacity %llu", (unsigned long long)ix->n_recs, (unsigned long long)recs_cap);
    if (ix->n_recs == 0) return PK_OK;
    if (!hits_out || !depth_out) return fail(PK_ERR_ARG, "null output pointer");
    HIPCHK(hipSetDevice(ix->device));
    const size_t n = ix->n_recs * ix->q_tables.size() * sizeof(uint64_t);
    HIPCHK(hipMemcpy(hits_out, ix->q_hits.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(depth_out, ix->q_depth.p, n, hipMemcpyDeviceToHost));
    return PK_OK;
}

// ================================================================== FASTQ front end ============
static const char *fq_rule_text(uint32_t rule) {
    switch (rule) {
    case FQ_RULE_AT: return "line 1 must begin with '@' (after an empty line 1 only line terminators may follow)";
    case FQ_RULE_GT: return "line 2 must not begin with '>'";
    case FQ_RULE_PLUS: return "line 3 must begin with '+'";
    case FQ_RULE_LEN: return "line 4 must be as long as line 2";
    default: return "the stream ends inside the record";
    }
}

// the indexer stops at a malformed record until it is reset; rec is 0-based
static int fq_fail(pk_indexer *ix, uint64_t rec, uint32_t rule) {
    uint64_t line1 = 0;
    if (rec < ix->fq_recs_cap()) HIPCHK(hipMemcpy(&line1, &ix->fq_recs.p[rec].line1, sizeof line1, hipMemcpyDeviceToHost));
    fail(PK_ERR_FORMAT, "malformed FASTQ: record %llu (line 1 at byte %llu): %s", (unsigned long long)rec + 1, (unsigned long long)line1,
         fq_rule_text(rule));
    ix->fq_failed = true;
    ix->fq_err = g_err;
    return PK_ERR_FORMAT;
}

// the rules the kernels checked, as the feed's read-back left them in pin
static int fq_verdict(pk_indexer *ix) {
    const FqCarry &q = ix->pin->tail.fq;
    uint64_t rec = ~0ull;
    uint32_t rule = 0;
    if (q.err != ~0ull) { rec = q.err >> 3; rule = (uint32_t)(q.err & 7u); }
    if (q.trail != ~0ull) {                                  // an empty line 1: its record and everything behind it must be blank
        const uint64_t tr = q.trail / 4u;
        if (rec != ~0ull && rec >= tr) rec = ~0ull;          // the blank lines there break the record rules, and that is fine
        if (q.full > q.trail + 1u && tr < rec) { rec = tr; rule = FQ_RULE_AT; }
    }
    return rec == ~0ull ? PK_OK : fq_fail(ix, rec, rule);
}

static int fq_ensure_recs(pk_indexer *ix, uint64_t need) {
    if (need <= ix->fq_recs_cap()) return PK_OK;
    return ix->fq_recs.grow_keep(std::max<uint64_t>(need, 2 * ix->fq_recs_cap()) * sizeof(FqRec), ix->stream);
}

// the FASTA text of the previous FASTQ feed, if any, into the pipeline; ends with the read-back of the carry
static int fq_flush(pk_indexer *ix) {
    if (ix->fq_pending) {
        const uint64_t n = ix->fq_pending;
        ix->fq_pending = 0;
        return feed_piece(ix, ix->fq_out[ix->fq_buf ^ 1].p, n);
    }
    return read_tail(ix);
}

// one FASTQ piece of at most feed_max_for(k) bytes: the front end turns it into FASTA text in fq_out[fq_buf] while the
// text of the piece before goes through the FASTA pipeline
static int fq_feed_piece(pk_indexer *ix, const uint8_t *f, uint64_t n) {
    const uint32_t n_chunks = (uint32_t)((n + CHUNK - 1) / CHUNK);
    const int b = ix->fq_buf;
    int rc;
    if ((rc = ix->fq_sums.reserve((size_t)n_chunks * sizeof(FqSum)))) return rc;
    if ((rc = ix->fq_st.reserve((size_t)n_chunks * sizeof(FqState)))) return rc;
    if ((rc = ix->fq_out[b].reserve(n + 64))) return rc;
    // record slots for what the stream needed so far and one record per 256 bytes of this piece; a piece that needs
    // more writes its text again once the array has grown
    if ((rc = fq_ensure_recs(ix, ix->fq_need + n / 256 + 1024))) return rc;
    FqCarry *carry = &ix->tail.p->fq;
    launch_fq_front(f, n, ix->fq_sums.p, ix->fq_st.p, ix->fq_out[b].p, ix->fq_recs.p, ix->fq_recs_cap(), carry, ix->stream);
    HIPCHK(hipGetLastError());
    if ((rc = fq_flush(ix))) return rc;
    if (ix->pin->tail.fq.need > ix->fq_recs_cap()) {
        if ((rc = fq_ensure_recs(ix, ix->pin->tail.fq.need + n / 256 + 1024))) return rc;
        launch_fq_write(f, n, ix->fq_st.p, ix->fq_out[b].p, ix->fq_recs.p, ix->fq_recs_cap(), carry, ix->stream);
        HIPCHK(hipGetLastError());
        if ((rc = fq_flush(ix))) return rc;
    }
    const FqCarry &q = ix->pin->tail.fq;
    ix->fq_need = q.need;
    if ((rc = fq_verdict(ix))) return rc;
    ix->fq_pending = q.st.out - q.in.out;
    ix->fq_buf = b ^ 1;
    return PK_OK;
}

// end of stream: after the last complete record only line terminators (checked with the feeds), or a last line 4
// without a terminator
static int fq_end_check(pk_indexer *ix) {
    const FqCarry &q = ix->pin->tail.fq;
    if (q.trail != ~0ull) return PK_OK;
    const uint32_t role = (uint32_t)(q.st.line & 3u);
    const uint64_t rec = q.st.line / 4u;
    if (role == 0u && q.st.curlen == 0) return PK_OK;
    if (role == 3u && q.st.curlen > 0) {
        uint64_t len2 = 0;
        if (rec < ix->fq_recs_cap()) HIPCHK(hipMemcpy(&len2, &ix->fq_recs.p[rec].len2, sizeof len2, hipMemcpyDeviceToHost));
        return len2 == q.st.curlen ? PK_OK : fq_fail(ix, rec, FQ_RULE_LEN);
    }
    return fq_fail(ix, rec, FQ_RULE_END);
}

extern "C" int pk_indexer_set_format(pk_indexer *ix, int format) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (format != PK_FORMAT_FASTA && format != PK_FORMAT_FASTQ) return fail(PK_ERR_ARG, "unknown input format %d", format);
    if (ix->fed || ix->finished) return fail(PK_ERR_STATE, "the input format is set before the first feed (reset the indexer first)");
    ix->format = format;
    return PK_OK;
}

extern "C" int pk_indexer_fastq_stats(pk_indexer *ix, uint64_t out[4]) {
    if (!ix || !out) return fail(PK_ERR_ARG, "null argument");
    if (ix->format != PK_FORMAT_FASTQ) return fail(PK_ERR_STATE, "not a FASTQ indexer");
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (!ix->fed) return PK_OK;
    const FqCarry &q = ix->pin->tail.fq;                     // every feed ends with its read-back
    const uint64_t lines = q.st.line + (q.st.curlen > 0 ? 1u : 0u);
    out[0] = q.trail != ~0ull ? q.trail / 4u : (lines + 3u) / 4u;
    out[1] = lines;
    out[2] = q.bytes_fed;
    out[3] = q.st.out;
    return PK_OK;
}

extern "C" int pk_indexer_feed_device(pk_indexer *ix, const void *dev_fasta, uint64_t n_bytes) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (ix->finished) return fail(PK_ERR_STATE, "indexer already finished; reset it first");
    if (n_bytes == 0) return PK_OK;
    if (!dev_fasta || ((uintptr_t)dev_fasta & 15u)) return fail(PK_ERR_ARG, "device FASTA pointer must be non-null and 16-byte aligned");
    if (n_bytes > (1ULL << 40)) return fail(PK_ERR_ARG, "feed of %llu bytes too large; split it", (unsigned long long)n_bytes);
    HIPCHK(hipSetDevice(ix->device));
    const uint8_t *f = (const uint8_t *)dev_fasta;
    const uint64_t piece_max = feed_max_for(ix->k);                 // a multiple of 16: pieces stay aligned
    const bool fastq = ix->format == PK_FORMAT_FASTQ;
    if (fastq && ix->fq_failed) return fail(PK_ERR_FORMAT, "%s", ix->fq_err.c_str());
    ix->fed = true;
    for (uint64_t off = 0; off < n_bytes; off += piece_max) {
        const uint64_t len = std::min(piece_max, n_bytes - off);
        int rc = fastq ? fq_feed_piece(ix, f + off, len) : feed_piece(ix, f + off, len);
        if (rc) return rc;
    }
    return PK_OK;
}

// Host text arrives in pieces of FEED_PIECE bytes through two staging buffers in HBM: while the GPU counts piece i,
// the copy threads already move piece i+1 across PCIe (the upload, ~15 ms per 0.8 GB, is the longer of the two).
extern "C" int pk_indexer_feed(pk_indexer *ix, const uint8_t *host_fasta, uint64_t n_bytes) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (n_bytes == 0) return PK_OK;
    if (!host_fasta) return fail(PK_ERR_ARG, "null FASTA pointer");
    HIPCHK(hipSetDevice(ix->device));
    const char *env = getenv("PK_FEED_PIECE");
    uint64_t piece = env ? strtoull(env, nullptr, 10) : (256ULL << 20);
    piece = std::max<uint64_t>(1 << 20, std::min<uint64_t>(piece, 1ULL << 30)) & ~15ULL;
    const uint64_t n_pieces = (n_bytes + piece - 1) / piece;
    const uint64_t buf_bytes = std::min(piece, n_bytes) + 64;
    const int n_bufs = n_pieces > 1 ? 2 : 1;
    int rc = PK_OK;
    for (int i = 0; i < n_bufs; i++)
        if ((rc = ix->staging[i].reserve(buf_bytes))) return rc;
    auto upload = [&](uint64_t p) -> int {
        const uint64_t off = p * piece, len = std::min(piece, n_bytes - off);
        return bounce_copy(ix->staging[p & 1].p, const_cast<uint8_t *>(host_fasta) + off, len, true, ix->device);
    };
    if ((rc = upload(0))) return rc;
    for (uint64_t p = 0; p < n_pieces; p++) {
        int up_rc = PK_OK;
        std::string up_err;
        std::thread next;
        if (p + 1 < n_pieces) next = std::thread([&]() { up_rc = upload(p + 1); if (up_rc) up_err = g_err; });
        const uint64_t off = p * piece, len = std::min(piece, n_bytes - off);
        rc = pk_indexer_feed_device(ix, ix->staging[p & 1].p, len);
        if (next.joinable()) next.join();
        if (rc) return rc;
        if (up_rc) { g_err = up_err; return up_rc; }
    }
    return PK_OK;
}

extern "C" int pk_indexer_finish(pk_indexer *ix, uint64_t *num_kmers_out, uint64_t *total_bp_out, uint64_t hist256_out[256],
                                 uint64_t *n_recs_out) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    HIPCHK(hipSetDevice(ix->device));
    if (!ix->finished && ix->format == PK_FORMAT_FASTQ) {
        if (ix->fq_failed) return fail(PK_ERR_FORMAT, "%s", ix->fq_err.c_str());
        if (ix->fq_pending) {                                // the last feed's text
            int rc = fq_flush(ix);
            if (rc) return rc;
        }
    }
    if (!ix->finished) {
        if (ix->tail_on_host && (!ix->table_fresh || ix->query)) {
            // the usual case: the last feed's read-back already holds the totals and the histogram (kept up to date by
            // k_bucket_count / k_apply_side: no pass over the table), and every kernel has finished -- nothing to do
            ix->t_final = 0;
        } else {
            HIPCHK(hipEventRecord(ix->ev.final_begin, ix->stream));
            if (ix->table_fresh && !ix->query) {             // nothing was fed: the table is all zero
                HIPCHK(hipMemsetAsync(ix->table8.p, 0, ix->table8.bytes, ix->stream));
                ix->table_fresh = false;
            }
            HIPCHK(hipEventRecord(ix->ev.final_end, ix->stream));
            int rc = read_tail(ix);
            if (rc) return rc;
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, ix->ev.final_begin, ix->ev.final_end));
            ix->t_final = ms * 1e-3;
        }
        if (ix->format == PK_FORMAT_FASTQ) {
            int rc = fq_end_check(ix);
            if (rc) return rc;
        }
        if (ix->query) {
            int rc = query_count_bins(ix);
            if (rc) return rc;
        }
        ix->finished = true;
    }
    const Carry &c = ix->pin->tail.carry;
    if (num_kmers_out) *num_kmers_out = c.num_kmers;
    if (total_bp_out) *total_bp_out = c.total_bp;
    if (n_recs_out) *n_recs_out = c.n_recs;
    if (hist256_out) {
        if (ix->query) memset(hist256_out, 0, 256 * sizeof(uint64_t));   // no table of its own
        else hist_with_zeros(ix->pin->tail.hist, ix->n, hist256_out);
    }
    return PK_OK;
}

extern "C" int pk_indexer_records(pk_indexer *ix, pk_record *recs_out, uint64_t recs_cap) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (ix->n_recs > recs_cap) return fail(PK_ERR_RECS_CAP, "%llu records, capacity %llu", (unsigned long long)ix->n_recs, (unsigned long long)recs_cap);
    if (ix->n_recs == 0) return PK_OK;
    if (!recs_out) return fail(PK_ERR_ARG, "null records pointer");
    HIPCHK(hipSetDevice(ix->device));
    std::vector<DevRec> tmp(ix->n_recs);
    HIPCHK(hipMemcpy(tmp.data(), ix->recs.p, ix->n_recs * sizeof(DevRec), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < ix->n_recs; i++) {
        recs_out[i].name_off = tmp[i].name_off;
        recs_out[i].name_len = tmp[i].name_end > tmp[i].name_off ? tmp[i].name_end - tmp[i].name_off : 0;
        recs_out[i].seq_len = tmp[i].seq_len;
        recs_out[i].n_valid_kmers = tmp[i].n_valid;
    }
    if (ix->format == PK_FORMAT_FASTQ) {                     // FASTQ record i is FASTA record i: names are sliced from the FASTQ
        if (ix->n_recs > ix->fq_recs_cap()) return fail(PK_ERR_HIP, "FASTQ record array too small (internal error)");
        std::vector<FqRec> fq(ix->n_recs);
        HIPCHK(hipMemcpy(fq.data(), ix->fq_recs.p, ix->n_recs * sizeof(FqRec), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < ix->n_recs; i++) recs_out[i].name_off = fq[i].line1 + 1;
    }
    return PK_OK;
}

extern "C" int pk_indexer_table_to_host(pk_indexer *ix, uint8_t *table_out) {
    if (!ix || !table_out) return fail(PK_ERR_ARG, "null argument");
    if (ix->query) return fail(PK_ERR_STATE, "a query indexer holds no table");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    return bounce_copy(ix->table8.p, table_out, ix->n, false, ix->device);
}

extern "C" int pk_indexer_table_slice_to_host(pk_indexer *ix, uint8_t *dst, uint64_t offset, uint64_t n_bytes) {
    if (!ix || !dst) return fail(PK_ERR_ARG, "null argument");
    if (ix->query) return fail(PK_ERR_STATE, "a query indexer holds no table");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    if (offset > ix->n || n_bytes > ix->n - offset) return fail(PK_ERR_ARG, "slice outside the table");
    return bounce_copy(ix->table8.p + offset, dst, n_bytes, false, ix->device);
}

extern "C" int pk_indexer_table_device(pk_indexer *ix, const void **dev_table_out) {
    if (!ix || !dev_table_out) return fail(PK_ERR_ARG, "null argument");
    if (ix->query) return fail(PK_ERR_STATE, "a query indexer holds no table");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    *dev_table_out = ix->table8.p;
    return PK_OK;
}

extern "C" int pk_indexer_table_slice_to_device(pk_indexer *ix, void *dev_dst, uint64_t offset, uint64_t n_bytes) {
    if (!ix || !dev_dst) return fail(PK_ERR_ARG, "null argument");
    if (ix->query) return fail(PK_ERR_STATE, "a query indexer holds no table");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    if (offset > ix->n || n_bytes > ix->n - offset) return fail(PK_ERR_ARG, "slice outside the table");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(dev_dst, ix->table8.p + offset, n_bytes, hipMemcpyDeviceToDevice));
    return PK_OK;
}

extern "C" int pk_indexer_timings(pk_indexer *ix, double out[10]) {
    if (!ix || !out) return fail(PK_ERR_ARG, "null argument");
    for (int i = 0; i < 10; i++) out[i] = 0;
    out[0] = ix->t_scan; out[1] = ix->t_squeeze; out[2] = ix->t_final; out[3] = ix->t_zero; out[4] = (double)ix->feeds;
    out[5] = ix->t_part; out[6] = ix->query ? ix->t_coords : ix->t_bucket; out[7] = ix->t_sort; out[8] = (double)ix->relayouts; out[9] = (double)ix->recounted;
    return PK_OK;
}

static pk_indexer *g_cached_indexer = nullptr;

extern "C" int pk_count_release(void) {
    if (g_cached_indexer) { pk_indexer_destroy(g_cached_indexer); g_cached_indexer = nullptr; }
    return PK_OK;
}

extern "C" int pk_count_fasta(const uint8_t *fasta, uint64_t n_bytes, int k, uint8_t *table_out, uint64_t *num_kmers_out,
                              uint64_t *total_bp_out, uint64_t hist256_out[256], pk_record *recs_out, uint64_t recs_cap,
                              uint64_t *n_recs_out, int device) {
    int rc = check_k(k);
    if (rc) return rc;
    if (!table_out) return fail(PK_ERR_ARG, "null table pointer");
    if (n_bytes && !fasta) return fail(PK_ERR_ARG, "null FASTA pointer");
    // one indexer (1 GiB .. 16 GiB table + workspace in HBM) is kept between calls for the same k and device: a caller
    // that counts sample after sample does not pay hipMalloc / hipFree of ~15 GB each time.  pk_count_release() frees it.
    static std::mutex cache_mu;
    std::lock_guard<std::mutex> cache_lock(cache_mu);
    pk_indexer *&ix = g_cached_indexer;
    if (ix && (ix->k != k || ix->device != device)) { pk_indexer_destroy(ix); ix = nullptr; }
    if (!ix) {
        rc = pk_indexer_create(&ix, k, device);
        if (rc) { ix = nullptr; return rc; }
    } else if ((rc = pk_indexer_reset(ix))) {
        return rc;
    }
    if ((rc = pk_indexer_feed(ix, fasta, n_bytes))) return rc;
    uint64_t n_recs = 0;
    if ((rc = pk_indexer_finish(ix, num_kmers_out, total_bp_out, hist256_out, &n_recs))) return rc;
    if (n_recs_out) *n_recs_out = n_recs;
    if ((rc = pk_indexer_table_to_host(ix, table_out))) return rc;
    if (n_recs > recs_cap) return fail(PK_ERR_RECS_CAP, "%llu records, capacity %llu", (unsigned long long)n_recs, (unsigned long long)recs_cap);
    return pk_indexer_records(ix, recs_out, recs_cap);
}

// ================================================================== stats ======================
extern "C" int pk_table_stats(const uint8_t *table, uint64_t n, uint64_t hist256_out[256], int device) {
    if (!hist256_out || (n && !table)) return fail(PK_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(device));
    DevBuf<unsigned long long> d_hist;
    DevBuf<uint8_t> d_t;
    unsigned long long h[256];
    int rc;
    if ((rc = d_hist.reserve(sizeof h))) return rc;
    if ((rc = d_t.reserve(std::max<uint64_t>(n, 16)))) return rc;
    if (hipMemset(d_hist.p, 0, sizeof h) != hipSuccess || hipMemcpy(d_t.p, table, n, hipMemcpyHostToDevice) != hipSuccess)
        return fail(PK_ERR_HIP, "upload failed");
    launch_hist8(d_t.p, n, d_hist.p, 0);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d_hist.p, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(PK_ERR_HIP, "histogram kernel failed: %s", hipGetErrorString(hipGetLastError()));
    hist_with_zeros(h, n, hist256_out);
    return PK_OK;
}

// ================================================================== merger =====================
static int check_counts(int N, int min_count, int max_count) {
    if (N < 1) return fail(PK_ERR_ARG, "need at least one table");
    if (N > 128) return fail(PK_ERR_ARG, "at most 128 tables per call (got %d)", N);
    if (min_count < 1 || max_count > 255) return fail(PK_ERR_ARG, "min_count must be >= 1 and max_count <= 255 (merger.py:90-91)");
    return PK_OK;
}

extern "C" int pk_gram_expand(const uint64_t *pair, int N, uint64_t *matrix_out) {
    if (!pair || !matrix_out || N < 1) return fail(PK_ERR_ARG, "bad argument");
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            uint64_t *m = matrix_out + ((uint64_t)i * N + j) * 3;
            if (i == j) { m[0] = m[1] = m[2] = 0; continue; }              // merger.py:136: never assigned
            m[0] = pair[(uint64_t)i * N + i];                                // merger.py:175-176
            m[1] = pair[(uint64_t)j * N + j];
            m[2] = i < j ? pair[(uint64_t)i * N + j] : pair[(uint64_t)j * N + i];
        }
    return PK_OK;
}

// Per-device scan context: the table-pointer array in HBM, a stream and two events, created once and reused by
// every scan on that device (a 2 ms kernel should not pay for hipMalloc / hipEventCreate each call).
namespace {
struct GramCtx {
    std::mutex mu;
    const uint8_t **d_ptrs = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    unsigned long long *d_pair = nullptr;      // scratch N x N for callers that only want the host copy
    const uint8_t **d_gtab = nullptr;          // the tables of each pair group of a spectrum pass (spectrum_groups(128) x 16)
    std::vector<const uint8_t *> h_gtab;
    uint8_t *d_occ = nullptr;                  // occupancy bytes of an occgram pass over more than 16 tables (grown on demand)
    size_t occ_cap = 0;
};
GramCtx g_gram[MAX_DEVICES];

int gram_ctx(int device, GramCtx **out) {
    if (device < 0 || device >= MAX_DEVICES) return fail(PK_ERR_ARG, "device ordinal %d out of range", device);
    GramCtx &c = g_gram[device];
    static std::mutex init_mu;
    std::lock_guard<std::mutex> init_lock(init_mu);
    if (!c.d_ptrs) {
        HIPCHK(hipMalloc(&c.d_ptrs, 128 * sizeof(void *)));
        HIPCHK(hipMalloc(&c.d_pair, 128 * 128 * sizeof(unsigned long long)));
        HIPCHK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&c.e0));
        HIPCHK(hipEventCreate(&c.e1));
        HIPCHK(hipMalloc(&c.d_gtab, (size_t)spectrum_groups(128) * 16 * sizeof(void *)));
        c.h_gtab.assign((size_t)spectrum_groups(128) * 16, nullptr);
    }
    *out = &c;
    return PK_OK;
}

// The frame every merge pass over device-resident slices runs in.  The table pointers are checked and the device's
// context is locked; then, on its stream: `before` (what the pass needs in place but does not time: the pointer array,
// scratch), e0, `launch`, e1, `after` (a copy queued behind the pass) and one synchronise.  e0 .. e1 is the pass's kernel
// time.  `before` and `after` return a PK_* code and may be empty; `launch` returns non-zero when a launch failed.
using PassStep = std::function<int(GramCtx &)>;

int timed_pass(const char *what, const void *const *dev_tables, int N, int device, double *kernel_seconds_out,
               const PassStep &before, const PassStep &launch, const PassStep &after = nullptr) {
    if (!dev_tables) return fail(PK_ERR_ARG, "null table list");
    for (int i = 0; i < N; i++)
        if (!dev_tables[i] || ((uintptr_t)dev_tables[i] & 15u)) return fail(PK_ERR_ARG, "table %d: device pointer must be 16-byte aligned", i);
    HIPCHK(hipSetDevice(device));
    GramCtx *c = nullptr;
    int rc = gram_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    if (before && (rc = before(*c))) return rc;
    HIPCHK(hipEventRecord(c->e0, c->stream));
    if (launch(*c)) return fail(PK_ERR_HIP, "%s kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
    HIPCHK(hipEventRecord(c->e1, c->stream));
    if (after && (rc = after(*c))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kernel_seconds_out) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1)); *kernel_seconds_out = ms * 1e-3; }
    return PK_OK;
}

// the pair scans read their table pointers from HBM: uploaded ahead of e0
PassStep upload_pointers(const void *const *dev_tables, int N) {
    return [=](GramCtx &c) -> int {
        HIPCHK(hipMemcpyAsync(c.d_ptrs, dev_tables, N * sizeof(void *), hipMemcpyHostToDevice, c.stream));
        return PK_OK;
    };
}
}  // namespace

// One scan of N device-resident slices.  The tallies overwrite dev_pair_out, or the context's scratch for callers that
// only want the host copy.
extern "C" int pk_gram_device_partial(const void *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count,
                                      uint64_t *pair_out, void *dev_pair_out, int device, double *kernel_seconds_out) {
    int rc = check_counts(N, min_count, max_count);
    if (rc) return rc;
    auto d_pair = [=](GramCtx &c) { return dev_pair_out ? (unsigned long long *)dev_pair_out : c.d_pair; };
    return timed_pass(
        "gram", dev_tables, N, device, kernel_seconds_out, upload_pointers(dev_tables, N),
        [&](GramCtx &c) { return launch_gram(c.d_ptrs, N, n_slice, min_count, max_count, d_pair(c), true, c.stream); },
        [&](GramCtx &c) -> int {
            if (pair_out) HIPCHK(hipMemcpyAsync(pair_out, d_pair(c), (size_t)N * N * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
            return PK_OK;
        });
}

extern "C" int pk_gram_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count,
                                         void *dev_pair_accum, int device, double *kernel_seconds_out) {
    return pk_gram_device_accumulate_windows(dev_tables, N, n_slice, &min_count, &max_count, 1, dev_pair_accum, device, kernel_seconds_out);
}

// Several windows over the same staged slices: one pass per group of windows (k_gram_mw) where the kernel has room for
// them, one single-window scan each otherwise.
extern "C" int pk_gram_device_accumulate_windows(const void *const *dev_tables, int N, uint64_t n_slice, const int *min_counts,
                                                 const int *max_counts, int n_windows, void *dev_pair_accum, int device,
                                                 double *kernel_seconds_out) {
    if (!dev_pair_accum) return fail(PK_ERR_ARG, "null accumulator");
    if (n_windows < 1 || n_windows > 255 || !min_counts || !max_counts) return fail(PK_ERR_ARG, "between 1 and 255 windows per call");
    int rc = PK_OK;
    for (int w = 0; w < n_windows; w++)
        if ((rc = check_counts(N, min_counts[w], max_counts[w]))) return rc;
    const int per_pass = gram_windows_per_pass(N);
    unsigned long long *acc = (unsigned long long *)dev_pair_accum;
    return timed_pass("gram", dev_tables, N, device, kernel_seconds_out, upload_pointers(dev_tables, N), [&](GramCtx &c) {
        std::vector<int> order(n_windows);
        for (int w = 0; w < n_windows; w++) order[w] = w;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return min_counts[a] < min_counts[b]; });
        for (int at = 0; at < n_windows;) {
            const int take = (per_pass >= 2 && n_windows - at >= 2) ? std::min(per_pass, n_windows - at) : 1;
            int lrc;
            if (take == 1) {
                const int w = order[at];
                lrc = launch_gram(c.d_ptrs, N, n_slice, min_counts[w], max_counts[w], acc + (size_t)w * N * N, false, c.stream);
            } else {
                int mn[8], mx[8], out[8];
                for (int i = 0; i < take; i++) { mn[i] = min_counts[order[at + i]]; mx[i] = max_counts[order[at + i]]; out[i] = order[at + i]; }
                lrc = launch_gram_windows(c.d_ptrs, N, n_slice, mn, mx, out, take, acc, c.stream);
            }
            if (lrc) return lrc;
            at += take;
        }
        return 0;
    });
}

// Joint count spectra (gram_spectrum.hip): one pass per pair group over the staged slices, every tally ADDED to the caller's
// accumulator -- the slices of a rank, and the ranks by one all-reduce, sum like pk_gram_device_accumulate's.
extern "C" int pk_spectrum_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, void *dev_spec_accum, int device,
                                             double *kernel_seconds_out) {
    if (N < 2 || N > 128) return fail(PK_ERR_ARG, "a spectrum pass takes 2 to 128 tables (got %d)", N);
    if (!dev_spec_accum) return fail(PK_ERR_ARG, "null accumulator");
    return timed_pass("spectrum", dev_tables, N, device, kernel_seconds_out, nullptr, [&](GramCtx &c) {
        return launch_spectrum(dev_tables, N, n_slice, (unsigned long long *)dev_spec_accum, c.h_gtab.data(), c.d_gtab, c.stream);
    });
}

// Occupancy-stratified Gram products (gram_occ.hip): every tally ADDED to the caller's accumulator, so slices and ranks sum
// like pk_spectrum_device_accumulate's.
extern "C" int pk_occgram_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, void *dev_accum, int device,
                                            double *kernel_seconds_out) {
    if (N < 2 || N > 128) return fail(PK_ERR_ARG, "an occgram pass takes 2 to 128 tables (got %d)", N);
    if (!dev_accum) return fail(PK_ERR_ARG, "null accumulator");
    auto grow_scratch = [&](GramCtx &c) -> int {
        const size_t need = occgram_scratch_bytes(N, n_slice);
        if (need > c.occ_cap) HIPCHK(hipStreamSynchronize(c.stream));
        return reserve_exact((void **)&c.d_occ, &c.occ_cap, need);
    };
    return timed_pass("occgram", dev_tables, N, device, kernel_seconds_out, grow_scratch, [&](GramCtx &c) {
        return launch_occgram(dev_tables, N, n_slice, (unsigned long long *)dev_accum, c.d_ptrs, c.d_occ, c.stream);
    });
}

// The k-mers behind a presence / absence condition (kmer_extract.hip): count, scan and -- when the caller's arrays hold
// the total -- write, all queued behind each other; the host only reads the total back.
extern "C" int pk_extract_device(const void *const *dev_tables, int n_present, int n_absent, uint64_t n_slice, uint64_t first_addr,
                                 int min_count, int max_count, int min_present, int max_absent, void *dev_addr_out, void *dev_counts_out,
                                 uint64_t cap, uint64_t *n_selected_out, int device, double *kernel_seconds_out) {
    if (n_present < 1 || n_absent < 0 || n_present > 128 || n_absent > 128 || n_present + n_absent > 128)
        return fail(PK_ERR_ARG, "an extraction takes 1 to 128 tables, at least one of them present (got %d present, %d absent)", n_present, n_absent);
    if (min_count < 1 || max_count > 255 || min_count > max_count)
        return fail(PK_ERR_ARG, "the count window must satisfy 1 <= min <= max <= 255 (got %d-%d)", min_count, max_count);
    if (min_present < 1 || min_present > n_present) return fail(PK_ERR_ARG, "min_present must lie in 1..%d (got %d)", n_present, min_present);
    if (max_absent < 0 || max_absent > n_absent) return fail(PK_ERR_ARG, "max_absent must lie in 0..%d (got %d)", n_absent, max_absent);
    if (!n_selected_out) return fail(PK_ERR_ARG, "null n_selected_out");
    if (n_slice > (1ull << 40) || first_addr + n_slice < first_addr) return fail(PK_ERR_ARG, "slice of %llu addresses is out of range", (unsigned long long)n_slice);
    if (cap && (!dev_addr_out || !dev_counts_out || ((uintptr_t)dev_addr_out & 15u) || ((uintptr_t)dev_counts_out & 15u)))
        return fail(PK_ERR_ARG, "a capacity needs both output arrays, 16-byte aligned");
    if (cap > (1ull << 40)) return fail(PK_ERR_ARG, "capacity out of range");
    const int N = n_present + n_absent;
    const uint32_t n_wg = extract_workgroups(n_slice);
    DevBuf<uint16_t> d_masks;
    DevBuf<unsigned long long> d_wg;
    unsigned long long total = 0;
    if (n_slice == 0) {
        if (!dev_tables) return fail(PK_ERR_ARG, "null table list");
        *n_selected_out = 0;
        return PK_OK;
    }
    int rc = timed_pass(
        "extract", dev_tables, N, device, kernel_seconds_out,
        [&](GramCtx &c) -> int {
            int r = upload_pointers(dev_tables, N)(c);
            if (!r) r = d_wg.reserve(((size_t)n_wg + 1) * sizeof(unsigned long long));
            if (!r && cap) r = d_masks.reserve(extract_mask_words(n_slice) * sizeof(uint16_t));
            return r;
        },
        [&](GramCtx &c) {
            return launch_extract(c.d_ptrs, n_present, n_absent, n_slice, first_addr, min_count, max_count, min_present, max_absent, d_masks.p, d_wg.p,
                                  (unsigned long long *)dev_addr_out, (uint8_t *)dev_counts_out, cap, c.stream);
        },
        [&](GramCtx &c) -> int {
            HIPCHK(hipMemcpyAsync(&total, d_wg.p + n_wg, sizeof total, hipMemcpyDeviceToHost, c.stream));
            return PK_OK;
        });
    if (rc) return rc;
    *n_selected_out = total;
    if (total > cap && (cap || dev_addr_out || dev_counts_out))
        return fail(PK_ERR_RECS_CAP, "%llu addresses selected, room for %llu", total, (unsigned long long)cap);
    return PK_OK;
}

extern "C" int pk_extract_text(const void *dev_addr, uint64_t m, int k, void *dev_text_out, int device) {
    if (k < 1 || k > 32) return fail(PK_ERR_ARG, "kmer_len must lie in 1..32 (got %d)", k);
    if (m > (1ull << 40)) return fail(PK_ERR_ARG, "too many addresses");
    if (m == 0) return PK_OK;
    if (!dev_addr || !dev_text_out || ((uintptr_t)dev_addr & 7u) || ((uintptr_t)dev_text_out & 15u))
        return fail(PK_ERR_ARG, "address array (8-byte aligned) and text array (16-byte aligned) must not be null");
    HIPCHK(hipSetDevice(device));
    GramCtx *c = nullptr;
    int rc = gram_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    if (launch_extract_text((const unsigned long long *)dev_addr, m, k, (uint8_t *)dev_text_out, c->stream))
        return fail(PK_ERR_HIP, "extract text kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PK_OK;
}

extern "C" int pk_gram(const uint8_t *const *tables, int N, uint64_t n, int min_count, int max_count, uint64_t *matrix_out,
                       const int *devices, int n_devices) {
    int rc = check_counts(N, min_count, max_count);
    if (rc) return rc;
    if (!tables || !matrix_out) return fail(PK_ERR_ARG, "null argument");
    int dev0 = 0;
    if (!devices || n_devices <= 0) { devices = &dev0; n_devices = 1; }
    // address range split into n_devices contiguous slices (multiples of 32 addresses); one host thread per
    // device stages its slice and scans it, all devices at once
    const uint64_t per = ((n + n_devices - 1) / n_devices + 31u) & ~31ULL;
    std::vector<std::vector<uint64_t>> parts(n_devices, std::vector<uint64_t>((size_t)N * N, 0));
    std::vector<int> rcs(n_devices, PK_OK);
    std::vector<std::string> errs(n_devices);
    auto work = [&](int d) {
        const uint64_t lo = std::min<uint64_t>(n, per * d), hi = std::min<uint64_t>(n, lo + per);
        if (hi <= lo) return;
        auto run = [&]() -> int {
            HIPCHK(hipSetDevice(devices[d]));
            // as many tables' slices as fit beside each other in free HBM; the rest in further rounds over
            // sub-slices of the address range (partials add)
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            uint64_t sub = hi - lo;
            const uint64_t budget = (uint64_t)(free_b * 0.8);
            if ((uint64_t)N * (sub + 64) > budget) sub = std::max<uint64_t>(1 << 20, (budget / N - 64) & ~2047ULL);
            std::vector<DevBuf<uint8_t>> slices(N);
            std::vector<const void *> dptr(N, nullptr);
            int r;
            for (int i = 0; i < N; i++) {
                if ((r = slices[i].reserve(std::min(sub, hi - lo) + 64))) return r;
                dptr[i] = slices[i].p;
            }
            std::vector<uint64_t> one((size_t)N * N);
            for (uint64_t a = lo; a < hi; a += sub) {
                const uint64_t b = std::min(hi, a + sub);
                for (int i = 0; i < N; i++)
                    if (hipMemcpy(slices[i].p, tables[i] + a, b - a, hipMemcpyHostToDevice) != hipSuccess) return fail(PK_ERR_HIP, "table upload failed");
                if ((r = pk_gram_device_partial(dptr.data(), N, b - a, min_count, max_count, one.data(), nullptr, devices[d], nullptr))) return r;
                for (size_t i = 0; i < one.size(); i++) parts[d][i] += one[i];
            }
            return PK_OK;
        };
        rcs[d] = run();
        if (rcs[d]) errs[d] = g_err;                       // g_err is thread-local: carry the message back
    };
    if (n_devices == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int d = 0; d < n_devices; d++) th.emplace_back(work, d);
        for (auto &t : th) t.join();
    }
    for (int d = 0; d < n_devices; d++)
        if (rcs[d]) { g_err = errs[d]; return rcs[d]; }
    std::vector<uint64_t> pair((size_t)N * N, 0);
    for (int d = 0; d < n_devices; d++)
        for (size_t i = 0; i < pair.size(); i++) pair[i] += parts[d][i];
    return pk_gram_expand(pair.data(), N, matrix_out);
}
