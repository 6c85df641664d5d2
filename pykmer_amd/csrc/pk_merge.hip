// pk_merge.hip -- host side of the merger and the extractor: sequences the kernels of gram_scan.hip, gram_spectrum.hip,
// gram_occ.hip, gram_patterns.hip and kmer_extract.hip over device-resident table slices, and pk_table_stats.
#include <functional>

#include "pk_host.h"

using namespace pk;

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

// Presence patterns (gram_patterns.hip): the 2^N tallies of one count window ADDED to the caller's accumulator, so slices
// and ranks sum like pk_occgram_device_accumulate's.
extern "C" int pk_patterns_device_accumulate(const void *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count,
                                             void *dev_accum, int device, double *kernel_seconds_out) {
    if (N < 1 || N > 16) return fail(PK_ERR_ARG, "a pattern pass takes 1 to 16 tables (got %d): its 2^N bins are a dense array", N);
    if (min_count < 1 || max_count > 255 || min_count > max_count)
        return fail(PK_ERR_ARG, "the count window must satisfy 1 <= min <= max <= 255 (got %d-%d)", min_count, max_count);
    if (!dev_accum || ((uintptr_t)dev_accum & 7u)) return fail(PK_ERR_ARG, "null accumulator (or not 8-byte aligned)");
    if (n_slice > (1ull << 40)) return fail(PK_ERR_ARG, "slice of %llu addresses is out of range", (unsigned long long)n_slice);
    return timed_pass("patterns", dev_tables, N, device, kernel_seconds_out, nullptr, [&](GramCtx &c) {
        return launch_patterns(dev_tables, N, n_slice, min_count, max_count, (unsigned long long *)dev_accum, c.stream);
    });
}

// what pk_extract_device and pk_extract_table_device refuse alike
static int check_extract(int n_present, int n_absent, uint64_t n_slice, int min_count, int max_count, int min_present, int max_absent) {
    if (n_present < 1 || n_absent < 0 || n_present > 128 || n_absent > 128 || n_present + n_absent > 128)
        return fail(PK_ERR_ARG, "an extraction takes 1 to 128 tables, at least one of them present (got %d present, %d absent)", n_present, n_absent);
    if (min_count < 1 || max_count > 255 || min_count > max_count)
        return fail(PK_ERR_ARG, "the count window must satisfy 1 <= min <= max <= 255 (got %d-%d)", min_count, max_count);
    if (min_present < 1 || min_present > n_present) return fail(PK_ERR_ARG, "min_present must lie in 1..%d (got %d)", n_present, min_present);
    if (max_absent < 0 || max_absent > n_absent) return fail(PK_ERR_ARG, "max_absent must lie in 0..%d (got %d)", n_absent, max_absent);
    if (n_slice > (1ull << 40)) return fail(PK_ERR_ARG, "slice of %llu addresses is out of range", (unsigned long long)n_slice);
    return PK_OK;
}

// The k-mers behind a presence / absence condition (kmer_extract.hip): count, scan and -- when the caller's arrays hold
// the total -- write, all queued behind each other; the host only reads the total back.
extern "C" int pk_extract_device(const void *const *dev_tables, int n_present, int n_absent, uint64_t n_slice, uint64_t first_addr,
                                 int min_count, int max_count, int min_present, int max_absent, void *dev_addr_out, void *dev_counts_out,
                                 uint64_t cap, uint64_t *n_selected_out, int device, double *kernel_seconds_out) {
    int rc = check_extract(n_present, n_absent, n_slice, min_count, max_count, min_present, max_absent);
    if (rc) return rc;
    if (!n_selected_out) return fail(PK_ERR_ARG, "null n_selected_out");
    if (first_addr + n_slice < first_addr) return fail(PK_ERR_ARG, "slice of %llu addresses is out of range", (unsigned long long)n_slice);
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
    rc = timed_pass(
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

// The same selection as a dense table (k_extract_table), and the table's value histogram behind it on the same stream.
extern "C" int pk_extract_table_device(const void *const *dev_tables, int n_present, int n_absent, uint64_t n_slice, int min_count, int max_count,
                                       int min_present, int max_absent, int op, void *dev_table_out, void *dev_hist_accum, int device,
                                       double *kernel_seconds_out) {
    int rc = check_extract(n_present, n_absent, n_slice, min_count, max_count, min_present, max_absent);
    if (rc) return rc;
    if (op < PK_TABLE_SUM || op > PK_TABLE_COUNT) return fail(PK_ERR_ARG, "op must be 0..3 = sum, min, max, count (got %d)", op);
    if (!dev_table_out || ((uintptr_t)dev_table_out & 15u)) return fail(PK_ERR_ARG, "the output table must not be null and must be 16-byte aligned");
    if (!dev_hist_accum || ((uintptr_t)dev_hist_accum & 7u)) return fail(PK_ERR_ARG, "the histogram accumulator must not be null and must be 8-byte aligned");
    if (!dev_tables) return fail(PK_ERR_ARG, "null table list");
    const int N = n_present + n_absent;
    const uintptr_t o0 = (uintptr_t)dev_table_out, o1 = o0 + n_slice;
    for (int i = 0; i < N; i++)
        if (dev_tables[i] && (uintptr_t)dev_tables[i] < o1 && o0 < (uintptr_t)dev_tables[i] + n_slice)
            return fail(PK_ERR_ARG, "the output table overlaps table %d", i);
    if (n_slice == 0) return PK_OK;
    return timed_pass("extract table", dev_tables, N, device, kernel_seconds_out, upload_pointers(dev_tables, N), [&](GramCtx &c) {
        if (launch_extract_table(c.d_ptrs, n_present, n_absent, n_slice, min_count, max_count, min_present, max_absent, op, (uint8_t *)dev_table_out,
                                 c.stream))
            return 1;
        launch_hist8((const uint8_t *)dev_table_out, n_slice, (unsigned long long *)dev_hist_accum, c.stream);
        return (int)(hipGetLastError() != hipSuccess);
    });
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
