// pk_common.hip -- the part of the host layer (C-ABI of include/pykmer_hip.h) that belongs to no subsystem: version and
// errors, the caller's device buffers and the host <-> HBM copy.  No kernel is defined in the pk_*.hip files.
#include <cstdarg>

#include "pk_host.h"

using namespace pk;

thread_local std::string pk::g_err;

int pk::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace pk { int set_error(int code, const std::string &msg) { g_err = msg; return code; } }   // for the translation units of the kernels

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

int pk::reserve_exact(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return PK_OK;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIPCHK(hipMalloc(p, need));
    *cap = need;
    return PK_OK;
}

// ================================================================== host <-> HBM copies =========
// The C-ABI takes plain (pageable) host buffers.  One hipMemcpy from pageable memory is a single thread bouncing
// the bytes through a small pinned buffer; here several host threads each own a pinned bounce buffer (two halves)
// and a stream, so page-touching memcpy and PCIe DMA of different pieces overlap and the link is what limits.
namespace {
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
}  // namespace

// to_device: host -> dev, else dev -> host.  Blocking.
int pk::bounce_copy(void *dev, void *host, size_t n, bool to_device, int device) {
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
