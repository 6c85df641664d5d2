// pk_indexer.hip -- the indexer of the host layer: owns an indexer's device memory, stream and events and sequences the
// kernels of a feed (kmer_count.hip, kmer_pack.hip, then kmer_fuse.hip and kmer_part.hip for a counting indexer, kmer_query.hip
// and kmer_coords.hip for a query), with the FASTQ front end (fastq.hip) before them.
#include "pk_host.h"

using namespace pk;

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

// ================================================================== indexer ====================
static int ix_reset(pk_indexer *ix) {
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipEventRecord(ix->ev.reset_begin, ix->stream));
    // the first feed writes every slice of the u8 table itself (k_bucket_count, fresh); the table is only
    // zeroed if nothing gets fed at all (see pk_indexer_finish).  Nothing here waits for the device: the stream orders
    // the reset behind whatever is still running, and its duration is read at the next point that waits anyway.
    // One kernel: the tail becomes tail0, the record array zero (where a copy and a fill of the runtime were two stream
    // operations).
    launch_reset(ix->tail.p, ix->tail0.p, sizeof(pk_indexer::Tail), ix->recs.p, ix->recs.bytes, ix->stream);
    HIPCHK(hipGetLastError());
    ix->tail_on_host = false;
    const int rc = ix->q ? ix->q->reset(ix->stream) : PK_OK;
    if (rc) return rc;
    HIPCHK(hipEventRecord(ix->ev.reset_end, ix->stream));
    ix->zero_timed = false;
    ix->t_zero = 0;
    ix->bytes_fed = ix->n_recs = 0;
    ix->finished = false;
    ix->table_fresh = true;
    ix->t_scan = ix->t_squeeze = ix->t_sort = ix->t_final = ix->t_part = ix->t_bucket = 0;
    ix->feeds = ix->relayouts = 0; ix->recounted = 0;
    ix->fed = false;
    ix->fq_pending = 0; ix->fq_tail = 0; ix->fq_need = 0; ix->fq_failed = false; ix->fq_err.clear();
    ix->fix_chunks = 0;
    return PK_OK;
}

// after a wait on the stream: the duration of the last reset, if it has not been read yet
static void time_reset(pk_indexer *ix) {
    if (ix->zero_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ix->ev.reset_begin, ix->ev.reset_end) == hipSuccess) ix->t_zero = ms * 1e-3;
    ix->zero_timed = true;
}

// The stream totals, the value histogram, the FASTQ state and the feed's signals to the host in one copy, behind everything
// queued so far; the host waits for it.  This is the wait of a feed: it also surfaces a kernel fault and makes the reset's events readable.
static int read_tail(pk_indexer *ix) {
    HIPCHK(hipMemcpyAsync(ix->pin, ix->tail.p, sizeof(pk_indexer::Tail), hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    HIPCHK(hipGetLastError());
    time_reset(ix);
    ix->tail_on_host = true;
    return PK_OK;
}

extern "C" void pk_indexer_destroy(pk_indexer *ix) { delete ix; }

extern "C" int pk_indexer_create(pk_indexer **out, int k, int device) { return create_indexer(out, k, device, 0, 1, false); }

extern "C" int pk_indexer_create_slice(pk_indexer **out, int k, int device, int slice_index, int n_slices) {
    return create_indexer(out, k, device, slice_index, n_slices, false);
}

int pk::create_indexer(pk_indexer **out, int k, int device, int slice_index, int n_slices, bool query) {
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    *out = nullptr;
    int slice_bits = 0;
    int rc = check_slices(k, n_slices, slice_index, &slice_bits);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<pk_indexer> ix(new pk_indexer());        // a failure below destroys what was built so far
    ix->k = k; ix->device = device; ix->slice_bits = slice_bits; ix->slice_index = slice_index;
    ix->n = 1ULL << (2 * k - slice_bits);
    HIPCHK(hipStreamCreateWithFlags(&ix->stream.s, hipStreamNonBlocking));
    for (hipEvent_t *e : ix->ev.all()) HIPCHK(hipEventCreate(e));
    if (query) ix->q.reset(new QueryState());
    if (query && (rc = ix->q->create())) return rc;
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
    // room for the records of small inputs from the start: the squeeze pass checks the capacity itself (see run_feed)
    if ((rc = ix->recs.reserve(4096 * sizeof(DevRec)))) return rc;
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
    if (!ix->q && (rc = ix->chunk_fix.reserve(n * sizeof(ChunkFix)))) return rc;
    if ((rc = ix->t_l1.reserve((n / 1024 + 1) * sizeof(L1)))) return rc;
    return ix->t_l2.reserve((n / 1024 + 1) * sizeof(L2));
}

// after a wait on the stream: the seconds between two of its events, added to *t
static int add_elapsed(double *t, hipEvent_t from, hipEvent_t to) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, from, to));
    *t += ms * 1e-3;
    return PK_OK;
}

// the sizing rules stay with the callers: the capacities the two record arrays reach are part of the retry behaviour.
// `bytes`: the stream with the feed under way, for the rows of a binned query
static int ensure_recs(pk_indexer *ix, uint64_t need, uint64_t bytes) {
    if (need <= ix->recs_cap()) return PK_OK;
    const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(1024, ix->recs_cap() * 2));
    int rc = ix->recs.grow_keep(cap * sizeof(DevRec), ix->stream);
    return rc || !ix->q ? rc : ix->q->size_rows(cap, bytes, ix->stream);   // what a query keys by records or rows follows
}

// one feed of at most FEED_MAX bytes: structure pass -> squeeze -> bucket layout -> fused k-mer assembly + level-1
// sort -> level 2 -> bucket count.  Record positions are 32-bit: both bucket areas (their capacity + the dump tile) must
// end below 2^32 records.  The worst plan is k = 17 (2^18 final buckets x 4104 records of fixed slack + 25 % on the
// estimate): 2 GiB of text -> capacity2 = 3.76e9.  count_feed checks the plan it actually got and refuses otherwise.
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

// diagnostics: the chunks of the last feed that the structure pass squeezed itself, counted from its per-chunk records
extern "C" int pk_diag_settled_chunks(pk_indexer *ix, uint64_t *out) {
    if (!ix || !out) return fail(PK_ERR_ARG, "null argument");
    *out = 0;
    if (!ix->fix_chunks) return PK_OK;
    HIPCHK(hipSetDevice(ix->device));
    std::vector<ChunkFix> fix(ix->fix_chunks);
    HIPCHK(hipMemcpy(fix.data(), ix->chunk_fix.p, fix.size() * sizeof(ChunkFix), hipMemcpyDeviceToHost));   // every feed ends with a wait
    for (const ChunkFix &f : fix) *out += f.n_lead != 0u;
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

// What the two kinds of feed share behind their own preparations: the structure pass, the squeeze, what the caller queues
// behind it, and the read-back of the flags and the stream totals -- at most four times over, while a flag says that the
// feed has not settled.  Flag 2 (the squeeze backed out): the record array grows and the squeeze runs again; after any
// other flag only `queue` does.  `queue(raised)` gets the flag that made it run again, 0 the first time, and answers it as
// the caller sees fit.  `what` and `done` name the feed in the two refusals.
template <class Queue>
static int run_feed(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes, const PartPlan &pl, const PartBuffers &pb, const char *what, const char *done,
                    Queue queue) {
    const uint32_t n_chunks = pl.n_chunks;
    int rc = ensure_chunks(ix, n_chunks);
    if (rc) return rc;
    Carry *carry = &ix->tail.p->carry;
    const Events &ev = ix->ev;
    // a counting feed: the structure pass squeezes the settled chunks into pb's slots itself (ChunkFix, fasta_fsm.h); a query
    // feed keeps every piece's pack and lane state for the coordinate kernels
    ChunkFix *fix = ix->q ? nullptr : ix->chunk_fix.p;
    ix->fix_chunks = 0;
    // Nothing between here and the last kernel of the feed waits for the device: the record array was sized from what the
    // feeds so far held (ensure_recs below, after the feed), the squeeze pass checks that against the count the structure
    // pass leaves in `carry` and backs out if it does not fit (flags[0] = 2), the sorts back out if a sampled bucket
    // room does not hold (flags[0] = 1), and the host reads flags + record count once, behind the last kernel.  Every
    // kernel behind the squeeze returns at once when it finds flags[0] raised (the workspace then still holds an earlier
    // feed's squeezed text), so a 2 reaches the host as a 2, whatever that text would have done to the sampled layout.
    HIPCHK(hipEventRecord(ev.scan_begin, ix->stream));
    launch_chunk_l1(f, n_bytes, ix->c_l1.p, n_chunks, ix->stream);
    launch_scan_l1(ix->c_l1.p, n_chunks, carry, ix->c_l1s.p, ix->t_l1.p, pb.signals, ix->stream);
    launch_chunk_l2(f, n_bytes, ix->c_l1s.p, ix->c_l2.p, ix->lane_state.p, ix->packs.p, ix->chunk_odd.p, fix, pb, n_chunks, (uint32_t)ix->k, ix->stream);
    launch_scan_l2(ix->c_l2.p, n_chunks, carry, ix->c_l2s.p, ix->t_l2.p, (uint32_t)ix->k, ix->stream);
    HIPCHK(hipEventRecord(ev.scan_end, ix->stream));           // where the first squeeze begins, too: one record, not two
    hipEvent_t squeeze_from = ev.scan_end;
    uint32_t raised = 0;
    uint64_t squeezed_cap = 0;                               // record slots the last squeeze of this feed ran with
    for (int attempt = 0;; attempt++) {
        if (attempt) HIPCHK(hipMemsetAsync(pb.signals, 0, sizeof(PartSignals), ix->stream));   // the scan kernel zeroed them for the first attempt
        if (!raised || raised == 2u) {
            squeezed_cap = ix->recs_cap();
            if (attempt) { HIPCHK(hipEventRecord(ev.squeeze_begin, ix->stream)); squeeze_from = ev.squeeze_begin; }
            launch_squeeze(pl, pb, f, n_bytes, ix->bytes_fed, ix->lane_state.p, ix->packs.p, ix->c_l2s.p, ix->chunk_odd.p, fix, ix->recs.p, squeezed_cap,
                           carry, ix->stream);
            if (ix->k > 17) launch_deep_tail(pl, pb, carry, ix->stream);
            HIPCHK(hipEventRecord(ev.squeeze_end, ix->stream));
        }
        if ((rc = queue(raised))) return rc;
        // what the host needs of the feed, in one small copy behind the last kernel: the flags (pb.signals lies in the
        // tail), the stream totals and the value histogram (pk_indexer_finish then has nothing left to fetch)
        if ((rc = read_tail(ix))) return rc;
        raised = ix->pin->signals.flags[0];
        if (!raised) break;
        if (attempt >= 3) return fail(PK_ERR_HIP, "%s did not settle (internal error, flag %u)", what, raised);
        // more records than the array holds: grow it, squeeze again
        if (raised == 2u && (rc = ensure_recs(ix, ix->pin->carry.n_recs, ix->bytes_fed + n_bytes))) return rc;
    }
    // the text behind the squeeze is this feed's only if its last squeeze had room for every record (it backs out otherwise)
    if (ix->pin->carry.n_recs > squeezed_cap)
        return fail(PK_ERR_HIP, "feed %s without its squeeze: %llu records, %llu slots (internal error)", done,
                    (unsigned long long)ix->pin->carry.n_recs, (unsigned long long)squeezed_cap);
    const uint64_t recs_before = ix->n_recs;
    ix->n_recs = ix->pin->carry.n_recs;
    // room for the next feed's records before it arrives: as many again as this feed brought, and then some
    if ((rc = ensure_recs(ix, ix->n_recs + 2 * (ix->n_recs - recs_before) + 1024, ix->bytes_fed + n_bytes))) return rc;
    if ((rc = add_elapsed(&ix->t_scan, ev.scan_begin, ev.scan_end))) return rc;
    if ((rc = add_elapsed(&ix->t_squeeze, squeeze_from, ev.squeeze_end))) return rc;
    ix->feeds++;
    ix->bytes_fed += n_bytes;
    if (fix) ix->fix_chunks = n_chunks;
    return PK_OK;
}

// A counting indexer's feed: the partition passes and the bucket count behind the squeeze.
static int count_feed(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes) {
    const PartPlan pl = make_part_plan((uint32_t)ix->k, n_bytes, (uint32_t)ix->slice_bits, (uint32_t)ix->slice_index);
    if (!plan_fits_u32(pl)) return fail(PK_ERR_ARG, "feed of %llu bytes needs record positions beyond 2^32 (internal limit); split it", (unsigned long long)n_bytes);
    int rc = part_plan_check(pl, n_bytes);
    if (rc) return rc;
    if ((rc = ix->ws.reserve(part_workspace(pl, n_bytes)))) return rc;
    PartBuffers pb;
    part_workspace(pl, n_bytes, ix->ws.p, &pb, &ix->tail.p->signals);
    const Events &ev = ix->ev;
    uint32_t stride = pl.sample_stride;
    // the level-1 buckets are laid out from a sample of the slots; if one of them runs out of room every later kernel
    // returns untouched (flags[0] = 1) and the passes behind the squeeze are repeated with exact sizes -- on the text
    // the squeeze of this feed left, so only once that squeeze has run in full (flags[0] = 2 is handled first)
    auto queue = [&](uint32_t raised) -> int {
        if (raised && raised != 2u) {                        // a bucket outgrew its sampled room: lay out again, exactly
            if (stride == 1) return fail(PK_ERR_HIP, "level-1 buckets overflowed an exact layout (internal error)");
            stride = 1;
            ix->relayouts++;
        }
        const int lrc = launch_partitioned(pl, pb, ix->c_l2s.p, n_bytes, stride, &ix->tail.p->carry, ix->table8.p, ix->tail.p->hist, ix->hist_rep.p,
                                           ix->table_fresh, {ev.sort_begin, ev.sort_end, ev.part_end}, ix->stream);
        if (lrc) return lrc;
        HIPCHK(hipEventRecord(ev.bucket_end, ix->stream));
        return PK_OK;
    };
    if ((rc = run_feed(ix, f, n_bytes, pl, pb, "the feed's layout", "counted", queue))) return rc;
    ix->recounted += ix->pin->signals.flags[1];
    ix->table_fresh = false;
    if ((rc = add_elapsed(&ix->t_part, ev.squeeze_end, ev.part_end))) return rc;
    if ((rc = add_elapsed(&ix->t_bucket, ev.part_end, ev.bucket_end))) return rc;
    return add_elapsed(&ix->t_sort, ev.sort_begin, ev.sort_end);
}

// The feed of a query indexer that applies a mask (pk_query_set_mask): behind the squeeze (for n_bases[]) the base scan and
// k_mask_apply, which leaves the feed's patched text in a buffer of its own -- the squeeze of a repeated attempt (flag 2)
// reads the text it read before.  No tables, no lookups.  With intervals (pk_query_set_intervals) the position kernels of
// kmer_coords.hip and the count and scan of kmer_intervals.hip follow the apply, and the rows are written behind the feed's wait.
static int mask_feed(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes) {
    QueryState &q = *ix->q;
    if (ix->format != PK_FORMAT_FASTA) return fail(PK_ERR_STATE, "a mask is applied to FASTA text only");
    const PartPlan pl = make_part_plan((uint32_t)ix->k, n_bytes, 0u, 0u);   // the squeeze's launch shape; nothing is partitioned
    int rc = ix->ws.reserve(query_workspace(pl.n_chunks));
    if (rc) return rc;
    PartBuffers pb;
    QueryBuffers qb;
    query_workspace(pl.n_chunks, ix->ws.p, &pb, &qb, &ix->tail.p->signals);
    if ((rc = q.base_first.reserve((size_t)pl.n_chunks * sizeof(unsigned long long)))) return rc;
    if ((rc = q.mask_out.reserve(n_bytes + 64))) return rc;
    if (q.intervals && (rc = q.cpos.reserve((size_t)pl.n_chunks * sizeof(unsigned long long)))) return rc;
    if (q.intervals && (rc = q.chunk_iv.reserve((size_t)pl.n_chunks * 2 * sizeof(unsigned long long)))) return rc;
    q.mask_out_n = 0;
    const uint64_t mask_words = q.mask_bits.bytes / sizeof(uint32_t);
    auto queue = [&](uint32_t raised) -> int {
        if (raised && raised != 2u) return fail(PK_ERR_HIP, "the mask feed did not settle (internal error, flag %u)", raised);
        // a repeated attempt starts from the same base count (Carried) and finds masked[] as the feed before left it: the
        // attempt that backed out added nothing
        launch_cover_scan(pl, pb, q.nb.start(), q.nb.end(), q.base_first.p, ix->stream);
        HIPCHK(hipEventRecord(q.mask_begin, ix->stream));
        launch_mask_apply(pl, pb, f, n_bytes, ix->lane_state.p, ix->c_l2s.p, q.base_first.p, q.mask_bits.p, mask_words,
                          q.mask_mode, q.mask_out.p, q.masked.p, q.masked.bytes / sizeof(unsigned long long), ix->stream);
        HIPCHK(hipEventRecord(q.mask_end, ix->stream));
        if (q.intervals) {
            // the positions at the chunk starts, then the starts and ends of every chunk and of the stream behind this feed; a
            // repeated attempt starts from the same position and counts (Carried) and has written no row
            HIPCHK(hipEventRecord(q.iv_count_begin, ix->stream));
            launch_coords_positions(pl, pb, f, n_bytes, ix->lane_state.p, ix->packs.p, ix->c_l2s.p, ix->chunk_odd.p, q.cpos.p, q.pos.start(), q.pos.end(),
                                    ix->stream);
            launch_iv_count(pl, pb, f, n_bytes, ix->lane_state.p, ix->c_l2s.p, q.base_first.p, q.mask_bits.p, mask_words, q.mask_mode, q.chunk_iv.p,
                            q.iv_starts.start(), q.iv_ends.start(), q.iv_starts.end(), q.iv_ends.end(), ix->stream);
            HIPCHK(hipEventRecord(q.iv_count_end, ix->stream));
        }
        HIPCHK(hipGetLastError());
        return PK_OK;
    };
    if ((rc = run_feed(ix, f, n_bytes, pl, pb, "the mask feed", "masked", queue))) return rc;
    q.nb.settle();                                           // the base count behind this feed is the next feed's start
    q.mask_out_n = n_bytes;
    if ((rc = add_elapsed(&q.t_mask, q.mask_begin, q.mask_end))) return rc;
    if (!q.intervals) return PK_OK;
    // the feed has settled and the host has waited for it: the rows the stream needs by now are known (one per start; an end
    // goes to its start's row), the arrays grow to hold them, and the rows are written on the settled state
    unsigned long long ns = 0;
    HIPCHK(hipMemcpy(&ns, q.iv_starts.end(), sizeof ns, hipMemcpyDeviceToHost));
    if ((rc = q.size_intervals(ns, ix->stream))) return rc;
    HIPCHK(hipEventRecord(q.iv_write_begin, ix->stream));
    launch_iv_write(pl, pb, f, n_bytes, ix->lane_state.p, ix->c_l2s.p, q.base_first.p, q.mask_bits.p, mask_words, q.mask_mode, q.cpos.p, q.chunk_iv.p,
                    q.iv_record.p, q.iv_start.p, q.iv_end.p, q.iv_record.bytes / sizeof(unsigned long long), ix->stream);
    HIPCHK(hipEventRecord(q.iv_write_end, ix->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ix->stream));                // the caller may reuse the feed's text
    q.pos.settle();
    q.iv_starts.settle();
    q.iv_ends.settle();
    if ((rc = add_elapsed(&q.t_intervals, q.iv_count_begin, q.iv_count_end))) return rc;
    return add_elapsed(&q.t_intervals, q.iv_write_begin, q.iv_write_end);
}

// A query indexer's feed: the lookup kernels (kmer_query.hip), and with coordinates those of kmer_coords.hip, where
// count_feed runs launch_partitioned.  There is no sampled layout, so the only flag is 2 (the squeeze backed out): the
// record array, the window prefix and the accumulators grow (ensure_recs), and the squeeze and the lookups run again.  The
// arrays of every option are sized before the kernels run, with bins for the rows the stream can hold after this feed, and
// again, for the same stream, whenever the record array grows (QueryState::size_rows both times).
static int query_feed(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes) {
    QueryState &q = *ix->q;
    if (q.apply) return mask_feed(ix, f, n_bytes);
    if (q.tables.empty()) return fail(PK_ERR_STATE, "pk_query_set_tables comes before the first feed");
    const PartPlan pl = make_part_plan((uint32_t)ix->k, n_bytes, 0u, 0u);   // the squeeze's launch shape; nothing is partitioned
    int rc = ix->ws.reserve(query_workspace(pl.n_chunks));
    if (rc) return rc;
    PartBuffers pb;
    QueryBuffers qb;
    query_workspace(pl.n_chunks, ix->ws.p, &pb, &qb, &ix->tail.p->signals);
    Carry *carry = &ix->tail.p->carry;
    const uint32_t N = (uint32_t)q.tables.size();
    if ((rc = q.size_rows(ix->recs_cap(), ix->bytes_fed + n_bytes, ix->stream))) return rc;
    if (q.coords && (rc = q.cpos.reserve((size_t)pl.n_chunks * sizeof(unsigned long long)))) return rc;
    if (q.cover && (rc = q.base_first.reserve((size_t)pl.n_chunks * sizeof(unsigned long long)))) return rc;
    auto queue = [&](uint32_t raised) -> int {
        if (raised && raised != 2u) return fail(PK_ERR_HIP, "the query feed did not settle (internal error, flag %u)", raised);
        HIPCHK(hipEventRecord(q.lookup_begin, ix->stream));
        if (q.cover) {
            // the cover kernels where the lookup runs: no row tallies are needed.  A repeated attempt starts from the same
            // base count (Carried)
            launch_cover_scan(pl, pb, q.nb.start(), q.nb.end(), q.base_first.p, ix->stream);
            for (uint32_t t0 = 0; t0 < N; t0 += QUERY_MAX_TABLES)
                launch_query_cover(pl, pb, ix->c_l2s.p, q.base_first.p, q.tables.data() + t0, std::min(QUERY_MAX_TABLES, N - t0), (uint32_t)q.min,
                                   (uint32_t)q.max, q.cover_bits.p, q.cover_words(), ix->stream);
            HIPCHK(hipEventRecord(q.lookup_end, ix->stream));
            HIPCHK(hipGetLastError());
            return PK_OK;
        }
        launch_query_scan(pl, pb, qb, ix->c_l2s.p, q.windows, ix->recs.p, carry, q.p_done, q.P.p, q.Bf.p, q.bin, ix->stream);
        for (uint32_t t0 = 0; t0 < N; t0 += QUERY_MAX_TABLES)
            launch_query_lookup(pl, pb, qb, ix->c_l2s.p, q.P.p, q.Bf.p, q.bin, carry, q.tables.data() + t0, std::min(QUERY_MAX_TABLES, N - t0), N, t0,
                                (uint32_t)q.min, (uint32_t)q.max, q.hits.p, q.depth.p, q.spectrum ? q.spec.p : nullptr, q.pairs ? q.shared.p : nullptr,
                                ix->stream);
        HIPCHK(hipEventRecord(q.lookup_end, ix->stream));
        if (q.coords) {
            // behind launch_query_scan (slot_first, P, Bf) and on the rows size_rows sized; a repeated attempt starts
            // from the same position (Carried)
            HIPCHK(hipEventRecord(q.coords_begin, ix->stream));
            launch_query_coords(pl, pb, qb, f, n_bytes, ix->lane_state.p, ix->packs.p, ix->c_l2s.p, ix->chunk_odd.p, ix->recs.p, q.P.p, q.Bf.p, q.bin,
                                q.cpos.p, q.pos.start(), q.pos.end(), q.bin_start.p, q.bin_end.p,
                                q.bin_start.bytes / sizeof(unsigned long long), ix->stream);
            HIPCHK(hipEventRecord(q.coords_end, ix->stream));
        }
        HIPCHK(hipGetLastError());
        return PK_OK;
    };
    if ((rc = run_feed(ix, f, n_bytes, pl, pb, "the query feed", "looked up", queue))) return rc;
    q.windows = ix->pin->carry.num_kmers;
    q.p_done = ix->n_recs;
    if ((rc = add_elapsed(&ix->t_part, q.lookup_begin, q.lookup_end))) return rc;
    if (q.cover) q.nb.settle();                              // the base count behind this feed is the next feed's start
    if (!q.coords) return PK_OK;
    if ((rc = add_elapsed(&q.t_coords, q.coords_begin, q.coords_end))) return rc;
    q.pos.settle();                                          // the position behind this feed is the next feed's start
    return PK_OK;
}

static int feed_piece(pk_indexer *ix, const uint8_t *f, uint64_t n_bytes) {
    return ix->q ? query_feed(ix, f, n_bytes) : count_feed(ix, f, n_bytes);
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
    const FqCarry &q = ix->pin->fq;
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
    if (need > ix->fq_recs_cap()) {
        int rc = ix->fq_recs.grow_keep(std::max<uint64_t>(need, 2 * ix->fq_recs_cap()) * sizeof(FqRec), ix->stream);
        if (rc) return rc;
    }
    return ix->fq_tq ? ix->fq_out2.grow_keep(ix->fq_recs_cap() * sizeof(uint64_t), ix->stream) : PK_OK;   // slot for slot
}

// the FASTA text of the previous FASTQ feed, if any, into the pipeline; ends with the read-back of the carry.  With a
// held-back record in front of it the text can be longer than a piece: it goes in pieces (a multiple of 16: they stay aligned).
static int fq_flush(pk_indexer *ix) {
    if (!ix->fq_pending) return read_tail(ix);
    const uint64_t n = ix->fq_pending, piece_max = feed_max_for(ix->k);
    ix->fq_pending = 0;
    for (uint64_t off = 0; off < n; off += piece_max)
        if (int rc = feed_piece(ix, ix->fq_out[ix->fq_buf ^ 1].p + off, std::min(piece_max, n - off))) return rc;
    return PK_OK;
}

// one FASTQ piece of at most feed_max_for(k) bytes: the front end turns it into FASTA text in fq_out[fq_buf] while the
// text of the piece before goes through the FASTA pipeline.  With base qualities the buffer begins with the text held back
// from the piece before (behind its pending bytes), which this piece's line 4 bytes may still change; what is settled
// after this piece becomes the pending text, the rest is held back in turn.
static int fq_feed_piece(pk_indexer *ix, const uint8_t *f, uint64_t n) {
    const uint32_t n_chunks = (uint32_t)((n + CHUNK - 1) / CHUNK);
    const int b = ix->fq_buf;
    const uint32_t tq = (uint32_t)ix->fq_tq;
    const uint64_t held = ix->fq_tail;
    int rc;
    if ((rc = ix->fq_sums.reserve((size_t)n_chunks * sizeof(FqSum)))) return rc;
    if ((rc = ix->fq_st.reserve((size_t)n_chunks * sizeof(FqState)))) return rc;
    if ((rc = ix->fq_out[b].reserve(held + n + 64))) return rc;
    // record slots for what the stream needed so far and one record per 256 bytes of this piece; a piece that needs
    // more writes its text again once the array has grown
    if ((rc = fq_ensure_recs(ix, ix->fq_need + n / 256 + 1024))) return rc;
    FqCarry *carry = &ix->tail.p->fq;
    if (held) HIPCHK(hipMemcpyAsync(ix->fq_out[b].p, ix->fq_out[b ^ 1].p + ix->fq_pending, held, hipMemcpyDeviceToDevice, ix->stream));
    launch_fq_front(f, n, ix->fq_sums.p, ix->fq_st.p, ix->fq_out[b].p, held, ix->fq_recs.p, ix->fq_out2.p, ix->fq_recs_cap(), tq, carry, ix->stream);
    HIPCHK(hipGetLastError());
    if ((rc = fq_flush(ix))) return rc;
    if (ix->pin->fq.need > ix->fq_recs_cap()) {
        if ((rc = fq_ensure_recs(ix, ix->pin->fq.need + n / 256 + 1024))) return rc;
        launch_fq_write(f, n, ix->fq_st.p, ix->fq_out[b].p, held, ix->fq_recs.p, ix->fq_out2.p, ix->fq_recs_cap(), tq, carry, ix->stream);
        HIPCHK(hipGetLastError());
        if ((rc = fq_flush(ix))) return rc;
    }
    const FqCarry &q = ix->pin->fq;
    ix->fq_need = q.need;
    if ((rc = fq_verdict(ix))) return rc;
    const uint64_t out_lo = q.in.out - held;                 // the emitted bytes fq_out[b] begins with
    const uint64_t settled = tq ? std::min(std::max(q.settled, out_lo), q.st.out) : q.st.out;
    ix->fq_pending = settled - out_lo;
    ix->fq_tail = q.st.out - settled;
    ix->fq_buf = b ^ 1;
    return PK_OK;
}

// end of stream: after the last complete record only line terminators (checked with the feeds), or a last line 4
// without a terminator
static int fq_end_check(pk_indexer *ix) {
    const FqCarry &q = ix->pin->fq;
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
    if (format != PK_FORMAT_FASTQ) ix->fq_tq = 0;            // base qualities belong to FASTQ
    return PK_OK;
}

extern "C" int pk_indexer_set_min_qual(pk_indexer *ix, int threshold_byte) {
    if (!ix) return fail(PK_ERR_ARG, "null indexer");
    if (threshold_byte < 0 || threshold_byte > 255) return fail(PK_ERR_ARG, "quality threshold byte %d outside 0..255", threshold_byte);
    if (ix->format != PK_FORMAT_FASTQ) return fail(PK_ERR_STATE, "base qualities need a FASTQ indexer (pk_indexer_set_format first)");
    if (ix->fed || ix->finished) return fail(PK_ERR_STATE, "the quality threshold is set before the first feed (reset the indexer first)");
    ix->fq_tq = threshold_byte;
    return PK_OK;
}

extern "C" int pk_indexer_fastq_masked(pk_indexer *ix, uint64_t *out) {
    if (!ix || !out) return fail(PK_ERR_ARG, "null argument");
    if (ix->format != PK_FORMAT_FASTQ) return fail(PK_ERR_STATE, "not a FASTQ indexer");
    *out = ix->fed && ix->fq_tq ? ix->pin->fq.masked : 0;   // every feed ends with its read-back
    return PK_OK;
}

extern "C" int pk_indexer_fastq_stats(pk_indexer *ix, uint64_t out[4]) {
    if (!ix || !out) return fail(PK_ERR_ARG, "null argument");
    if (ix->format != PK_FORMAT_FASTQ) return fail(PK_ERR_STATE, "not a FASTQ indexer");
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (!ix->fed) return PK_OK;
    const FqCarry &q = ix->pin->fq;                     // every feed ends with its read-back
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
    // pk_query_mask_text hands back one piece: the caller cuts a longer text itself
    if (ix->q && ix->q->apply && n_bytes > piece_max)
        return fail(PK_ERR_ARG, "a mask feed takes at most %llu bytes, got %llu; feed the text in smaller pieces", (unsigned long long)piece_max,
                    (unsigned long long)n_bytes);
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
    if (ix->q && ix->q->apply && n_pieces > 1)               // pk_query_mask_text hands back one piece
        return fail(PK_ERR_ARG, "a mask feed takes at most %llu bytes, got %llu; feed the text in smaller pieces", (unsigned long long)piece,
                    (unsigned long long)n_bytes);
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
        if (ix->fq_pending || ix->fq_tail) {                 // the last feed's text, with what it held back: no line 4 is left to come
            ix->fq_pending += ix->fq_tail;
            ix->fq_tail = 0;
            int rc = fq_flush(ix);
            if (rc) return rc;
        }
    }
    if (!ix->finished) {
        if (ix->tail_on_host && (!ix->table_fresh || ix->q)) {
            // the usual case: the last feed's read-back already holds the totals and the histogram (kept up to date by
            // k_bucket_count / k_apply_side: no pass over the table), and every kernel has finished -- nothing to do
            ix->t_final = 0;
        } else {
            HIPCHK(hipEventRecord(ix->ev.final_begin, ix->stream));
            if (ix->table_fresh && !ix->q) {             // nothing was fed: the table is all zero
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
        if (ix->q) {
            int rc = query_count_bins(ix);
            if (!rc) rc = query_close_intervals(ix);
            if (rc) return rc;
        }
        ix->finished = true;
    }
    const Carry &c = ix->pin->carry;
    if (num_kmers_out) *num_kmers_out = c.num_kmers;
    if (total_bp_out) *total_bp_out = c.total_bp;
    if (n_recs_out) *n_recs_out = c.n_recs;
    if (hist256_out) {
        if (ix->q) memset(hist256_out, 0, 256 * sizeof(uint64_t));   // no table of its own
        else hist_with_zeros(ix->pin->hist, ix->n, hist256_out);
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

// what the table accessors refuse: a query indexer, an unfinished stream, a slice outside the table
static int table_check(pk_indexer *ix, const void *arg, uint64_t offset = 0, uint64_t n_bytes = 0) {
    if (!ix || !arg) return fail(PK_ERR_ARG, "null argument");
    if (ix->q) return fail(PK_ERR_STATE, "a query indexer holds no table");
    if (!ix->finished) return fail(PK_ERR_STATE, "call pk_indexer_finish first");
    if (offset > ix->n || n_bytes > ix->n - offset) return fail(PK_ERR_ARG, "slice outside the table");
    return PK_OK;
}

extern "C" int pk_indexer_table_to_host(pk_indexer *ix, uint8_t *table_out) {
    if (int rc = table_check(ix, table_out)) return rc;
    return bounce_copy(ix->table8.p, table_out, ix->n, false, ix->device);
}

extern "C" int pk_indexer_table_slice_to_host(pk_indexer *ix, uint8_t *dst, uint64_t offset, uint64_t n_bytes) {
    if (int rc = table_check(ix, dst, offset, n_bytes)) return rc;
    return bounce_copy(ix->table8.p + offset, dst, n_bytes, false, ix->device);
}

extern "C" int pk_indexer_table_device(pk_indexer *ix, const void **dev_table_out) {
    if (int rc = table_check(ix, dev_table_out)) return rc;
    *dev_table_out = ix->table8.p;
    return PK_OK;
}

extern "C" int pk_indexer_table_slice_to_device(pk_indexer *ix, void *dev_dst, uint64_t offset, uint64_t n_bytes) {
    if (int rc = table_check(ix, dev_dst, offset, n_bytes)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(dev_dst, ix->table8.p + offset, n_bytes, hipMemcpyDeviceToDevice));
    return PK_OK;
}

extern "C" int pk_indexer_timings(pk_indexer *ix, double out[10]) {
    if (!ix || !out) return fail(PK_ERR_ARG, "null argument");
    for (int i = 0; i < 10; i++) out[i] = 0;
    out[0] = ix->t_scan; out[1] = ix->t_squeeze; out[2] = ix->t_final; out[3] = ix->t_zero; out[4] = (double)ix->feeds;
    out[5] = ix->t_part; out[6] = ix->q ? ix->q->t_coords : ix->t_bucket; out[7] = ix->q ? ix->q->t_mask : ix->t_sort; out[8] = (double)ix->relayouts; out[9] = (double)ix->recounted;
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
