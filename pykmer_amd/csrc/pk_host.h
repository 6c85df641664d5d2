// pk_host.h -- what the files of the host layer share (pk_common.hip, pk_indexer.hip, pk_query.hip, pk_merge.hip, pk_select.hip, pk_trim.hip, pk_correct.hip, pk_unitig.hip): the error
// helper, owned device memory and the host <-> HBM copy for all of them, struct pk_indexer and the state of a query (with
// the value it carries from feed to feed, Carried) for pk_indexer.hip (which feeds both kinds of indexer) and pk_query.hip,
// and the standard headers they use.  Every allocation of
// the library is made in these files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pykmer_hip.h"
#include "pk_kernels.h"

namespace pk {
extern thread_local std::string g_err;                       // what pk_last_error reports (pk_common.hip)
int fail(int code, const char *fmt, ...);                    // formats g_err, returns code

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return pk::fail(PK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

constexpr int MAX_DEVICES = 64;

// ================================================================== owned device memory =========
// "Reserve exactly": nothing at all when the capacity suffices (the steady state of the timed path); otherwise the old
// block is freed FIRST and exactly `need` bytes are allocated.  The k = 17 indexer sits next to a 16 GiB table: these
// buffers can afford neither geometric growth nor the old and the new block side by side.  The contents are lost.
int reserve_exact(void **p, size_t *cap, size_t need);

// One device allocation of T and its capacity in bytes.  Move-only; the destructor frees, and leaves g_err alone so that
// the message of the call that failed survives the clean-up.  Never a member of an object with static storage: the HIP
// runtime may be gone when static destructors run (Bouncer and GramCtx keep raw pointers for that reason).
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

// to_device: host -> dev, else dev -> host.  Blocking.  (pk_common.hip)
int bounce_copy(void *dev, void *host, size_t n, bool to_device, int device);

// the device tallies the values 1 .. 255 only: the zeros are the rest of the n addresses
inline void hist_with_zeros(const unsigned long long *h, uint64_t n, uint64_t hist256_out[256]) {
    uint64_t nonzero = 0;
    for (int v = 1; v < 256; v++) { hist256_out[v] = h[v]; nonzero += h[v]; }
    hist256_out[0] = n - nonzero;
}

// ================================================================== indexer and query state ====
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
    Events() = default;
    Events(const Events &) = delete;
    ~Events() { for (hipEvent_t *e : all()) if (*e) hipEventDestroy(*e); }
    std::array<hipEvent_t *, 12> all() {
        return {&reset_begin, &reset_end, &scan_begin, &scan_end, &squeeze_begin, &squeeze_end, &sort_begin, &sort_end, &part_end, &bucket_end,
                &final_begin, &final_end};
    }
};

// A value carried from one feed to the next in two device words: the feed's kernels read the value at its start from
// start() and leave the one at its end in end().  A repeated attempt of a feed starts from the same word: the two change
// roles only once the feed has settled (settle()).
struct Carried {
    DevBuf<unsigned long long> words;
    int in = 0;                                                 // the word that holds the value at the start of the next feed
    // the two words; a reset zeroed what was there, a new array is zeroed here
    int ready(hipStream_t s) { return words.grow_keep(2 * sizeof(unsigned long long), s); }
    const unsigned long long *start() const { return words.p + in; }
    unsigned long long *end() { return words.p + (in ^ 1); }
    void settle() { in ^= 1; }
};

// What a query indexer (pk_query_create) holds where a counting one holds its table: every valid window is looked up in
// the caller's tables and tallied per record.  Every array keyed by the records or by the rows of the tallies is sized in
// one place (size_rows).  The methods queue their work on the indexer's stream `s`.  (pk_query.hip)
struct QueryState {
    std::vector<const uint8_t *> tables;                    // the caller's device tables; they stay across resets
    int min = 1, max = 255;
    DevBuf<unsigned long long> P;                           // P[r]: valid windows of the stream before record r
    DevBuf<unsigned long long> hits, depth;                 // row-major [record][table]; with bins [bin][table]
    uint64_t windows = 0, p_done = 0;                       // valid windows / final entries of P before the next feed
    // bins (pk_query_set_bins): `bin` valid windows per accumulator row, 0 = one row per record.  Bf[r]: the rows before
    // record r, grown with P.  The rows a stream of `bytes` bytes and at most `cap` records can hold need no read-back:
    // every record adds at most one partial bin, and n bytes hold at most n windows.
    uint64_t bin = 0;
    DevBuf<unsigned long long> Bf;
    uint64_t n_bins = 0;                                    // after finish
    // coordinates (pk_query_set_coords): per row the position of the first base of its first window and one past the last
    // base of its last, sized and grown with hits.  pos: the position in the open record, carried from feed to feed; cpos:
    // one word per chunk.
    bool coords = false;
    DevBuf<unsigned long long> bin_start, bin_end, cpos;
    Carried pos;
    // count spectra (pk_query_set_spectrum): [row][table][256], the tally of the table counts of every valid window of a
    // row, sized, grown and zeroed with hits; 2 KiB per row and table
    bool spectrum = false;
    DevBuf<unsigned long long> spec;
    // shared windows (pk_query_set_pairs; at most QUERY_MAX_TABLES tables): [row][pair], the windows of a row valid in both
    // tables of a pair i < j, sized, grown and zeroed with hits; one table has no pair and no array
    bool pairs = false;
    DevBuf<unsigned long long> shared;
    // covered bases (kmer_cover.hip).  nb: the valid bases of the stream, carried from feed to feed; base_first: one word per
    // chunk.
    // cover (pk_query_set_cover): the feeds run k_query_cover where they run the lookup; cover_bits holds one bit per valid
    // base, sized before every feed for the bytes fed by then.
    // apply (pk_query_set_mask; no tables): the feeds patch the caller's bits (mask_bits, for mask_n_bases bases) into the
    // text; mask_out holds the last feed's patched text (mask_out_n bytes), masked[r] the selected bases of record r, sized
    // and grown with the record array.
    bool cover = false, apply = false;
    DevBuf<unsigned long long> base_first, masked;
    Carried nb;
    DevBuf<uint32_t> cover_bits, mask_bits;
    DevBuf<uint8_t> mask_out;
    uint64_t mask_n_bases = 0, mask_out_n = 0;
    uint32_t mask_mode = 0;
    // intervals (pk_query_set_intervals, with apply; kmer_intervals.hip): the maximal runs of selected bases as (record, start,
    // end) rows in stream order.  iv_starts / iv_ends: the starts and ends of the stream, carried from feed to feed (their
    // difference is the run still open); chunk_iv: two words per chunk; the rows grow with the intervals found (size_intervals),
    // by half at least.  Positions come from pos and cpos, as for the coordinates.
    bool intervals = false;
    DevBuf<unsigned long long> iv_record, iv_start, iv_end, chunk_iv;
    Carried iv_starts, iv_ends;
    uint64_t n_intervals = 0;                               // after finish
    hipEvent_t lookup_begin = nullptr, lookup_end = nullptr;       // the kernels of kmer_query.hip, or k_cover_scan + k_query_cover
    hipEvent_t coords_begin = nullptr, coords_end = nullptr;       // the kernels of kmer_coords.hip
    hipEvent_t mask_begin = nullptr, mask_end = nullptr;           // k_mask_apply
    hipEvent_t iv_count_begin = nullptr, iv_count_end = nullptr;   // the position kernels, k_iv_count and k_iv_scan
    hipEvent_t iv_write_begin = nullptr, iv_write_end = nullptr;   // k_iv_write
    double t_coords = 0, t_mask = 0, t_intervals = 0;

    ~QueryState() {
        for (hipEvent_t e : {lookup_begin, lookup_end, coords_begin, coords_end, mask_begin, mask_end, iv_count_begin, iv_count_end, iv_write_begin, iv_write_end})
            if (e) hipEventDestroy(e);
    }
    uint64_t cover_words() const { return cover_bits.bytes / sizeof(uint32_t); }
    int create();                                                  // the events, and P for the record array's first capacity
    int reset(hipStream_t s);                                      // an empty stream; the tables stay; bins, coordinates, spectra and pairs are off
    // every array of the options that are on, for a record array of `cap` records and a stream of `bytes` bytes (the feed
    // under way included): contents kept, the rest zero; nothing but comparisons where the capacities suffice
    int size_rows(uint64_t cap, uint64_t bytes, hipStream_t s);
    int size_intervals(uint64_t rows, hipStream_t s);              // the three interval arrays for `rows` rows: contents kept
    size_t n_pairs() const { return tables.size() * (tables.size() - 1) / 2; }
};

int create_indexer(pk_indexer **out, int k, int device, int slice_index, int n_slices, bool query);   // pk_indexer.hip
int query_count_bins(pk_indexer *ix);                          // pk_query.hip: the rows of a finished binned stream
int query_close_intervals(pk_indexer *ix);                     // pk_query.hip: the intervals of a finished stream, the open run closed
}  // namespace pk

// One counting stream on one device: the .kin image, the scratch of the structure pass (kmer_count.hip), the squeeze
// (kmer_pack.hip), the partition passes (kmer_fuse.hip, kmer_part.hip) and the FASTQ front end (fastq.hip), and the stream
// and events that order and time them.  Everything it holds is released by its destructor.
struct pk_indexer {
    int k = 0, device = 0;
    int slice_bits = 0, slice_index = 0;   // the table holds addresses [slice_index, slice_index + 1) * 4^k / 2^slice_bits
    uint64_t n = 0;                  // table bytes: 4^k / 2^slice_bits
    // members are destroyed in reverse order of declaration, behind the destructor's wait: the buffers, then the events,
    // then the stream
    pk::Stream stream;
    pk::Events ev;
    std::unique_ptr<pk::QueryState> q;       // query mode: no table, hist_rep or partition of its own
    pk::DevBuf<uint8_t> table8;          // the .kin image
    // parser state + running totals, the value histogram and what the feed's partition passes signal, side by side: one copy
    // brings all of it to the host, one kernel resets it
    struct Tail { pk::Carry carry; unsigned long long hist[256]; pk::FqCarry fq; pk::PartSignals signals; };
    pk::DevBuf<Tail> tail, tail0;          // tail0: the state of an empty stream (the reset kernel copies it, no host wait)
    static_assert(sizeof(Tail) % 8 == 0, "launch_reset copies the tail 8 bytes at a time");
    Tail *pin = nullptr;               // pinned landing zone of the feed's read-back
    bool tail_on_host = false;         // *pin is what the device holds (the last feed's read-back)
    bool zero_timed = true;            // t_zero of the last reset has been read from its events
    pk::DevBuf<unsigned long long> hist_rep;   // HIST_REPLICAS copies of one feed's histogram change (zero between feeds)
    pk::DevBuf<pk::DevRec> recs;
    pk::DevBuf<pk::L1> c_l1, c_l1s;
    pk::DevBuf<pk::L2> c_l2, c_l2s;
    pk::DevBuf<pk::LaneState> lane_state;      // per 64-byte piece: start state relative to its chunk
    pk::DevBuf<pk::PiecePack> packs;           // per 64-byte piece: its bases, classified and pushed together (structure pass -> squeeze pass)
    pk::DevBuf<uint32_t> chunk_odd;        // per chunk: pieces that are not plain sequence text
    pk::DevBuf<pk::ChunkFix> chunk_fix;    // per chunk of a counting feed: what the structure pass leaves of a chunk it squeezed itself
    uint32_t fix_chunks = 0;               // chunks of the last feed that chunk_fix describes (0: a query feed, or none yet)
    pk::DevBuf<pk::L1> t_l1;                   // scan scratch: one summary per 1024 chunks
    pk::DevBuf<pk::L2> t_l2;
    pk::DevBuf<uint8_t> staging[2];        // device copies of host-fed pieces (one counted while the next uploads)
    uint64_t bytes_fed = 0, n_recs = 0;
    bool finished = false;
    double t_scan = 0, t_squeeze = 0, t_sort = 0, t_final = 0, t_zero = 0, t_part = 0, t_bucket = 0;
    int feeds = 0, relayouts = 0;
    uint64_t recounted = 0;                                // buckets whose byte counters wrapped and were counted again (k_bucket_count_bytes)
    bool table_fresh = true;         // no feed has written the u8 table since the last reset
    pk::DevBuf<uint8_t> ws;              // workspace of the partition passes
    // FASTQ input (fastq.hip): each feed is turned into FASTA text in fq_out[fq_buf]; that text is counted by the next
    // feed (or by finish), whose read-back brings this feed's checks and totals along -- no wait of its own
    int format = PK_FORMAT_FASTA;
    bool fed = false;                  // bytes were fed since the last reset
    pk::DevBuf<pk::FqSum> fq_sums;
    pk::DevBuf<pk::FqState> fq_st;
    pk::DevBuf<uint8_t> fq_out[2];
    int fq_buf = 0;
    uint64_t fq_pending = 0;           // FASTA bytes in fq_out[fq_buf ^ 1] not counted yet
    // base qualities (pk_indexer_set_min_qual): line-4 bytes below fq_tq turn their line-2 bytes into 'N'.  The text of a
    // record whose line 4 is still open is held back: fq_tail bytes behind the pending ones, copied to the front of the
    // next feed's buffer, where that feed's line 4 bytes can still reach them.  The threshold stays across resets.
    int fq_tq = 0;
    uint64_t fq_tail = 0;
    pk::DevBuf<uint64_t> fq_out2;      // per record slot of fq_recs: the bytes emitted before its line 2 (allocated with a threshold only)
    pk::DevBuf<pk::FqRec> fq_recs;
    uint64_t fq_need = 0;
    bool fq_failed = false;
    std::string fq_err;

    uint64_t recs_cap() const { return recs.bytes / sizeof(pk::DevRec); }
    uint64_t fq_recs_cap() const { return fq_recs.bytes / sizeof(pk::FqRec); }
    ~pk_indexer() {
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        if (pin) hipHostFree(pin);
    }
};
