// pk_unitig.hip -- the host layer of the unitig builder (pk_unitig_*, include/pykmer_hip.h): the link array, the candidates
// and rows of the two phases (linear unitigs, then circular ones) and their FASTA text on the device, sized from what the
// passes of kmer_unitig.hip count, and the copies back.  The table is the caller's.  pk_unitig_graph adds, behind a build
// and only when it is called, the end -> row map, the edge arrays and the GFA text.
#include "pk_host.h"

using namespace pk;

namespace {
// what one phase keeps: its candidates (ends, or nodes that may lie on cycles) and, once they are measured, its rows and text
struct Phase {
    DevBuf<unsigned long long> cand, c_n, c_depth, wgA, wgB, r_addr, r_n, r_depth, r_off;
    DevBuf<uint8_t> c_keep, text;
    uint64_t m = 0, rows = 0, bytes = 0;
};
}  // namespace

struct pk_unitig {
    int k = 0, device = 0;
    uint64_t n = 0;                              // 4^k
    bool ready = false, built = false;
    // members are destroyed in reverse order of declaration, behind the destructor's wait: the buffers, then the stream
    Stream stream;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    DevBuf<uint8_t> link;
    DevBuf<unsigned long long> wg, totals;
    Phase ph[2];
    unsigned long long tot[UT_WORDS] = {};
    double t_links = 0, t_paths = 0, t_cycles = 0;
    uint64_t builds = 0;
    // the graph of the last build (pk_unitig_graph): nothing of it is reserved before that call
    bool graphed = false;
    DevBuf<unsigned long long> end_row, wgE, wgS, wgL, e_from, e_to;
    DevBuf<uint8_t> e_orient, gfa;
    uint64_t n_edges = 0, edges_dropped = 0, n_dead_ends = 0, gfa_bytes = 0;
    double t_edges = 0, t_gfa = 0;

    ~pk_unitig() {
        if (!ready) return;
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        for (hipEvent_t e : {ev_begin, ev_end}) if (e) hipEventDestroy(e);
    }
};

static int ensure_device(pk_unitig *u) {
    HIPCHK(hipSetDevice(u->device));
    if (u->ready) return PK_OK;
    u->ready = true;                             // from here on the destructor cleans up
    HIPCHK(hipStreamCreateWithFlags(&u->stream.s, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&u->ev_begin));
    HIPCHK(hipEventCreate(&u->ev_end));
    return u->totals.reserve(UT_WORDS * sizeof(unsigned long long));
}

extern "C" int pk_unitig_create(pk_unitig **out, int k, int device) {
    if (!out) return fail(PK_ERR_ARG, "null output pointer");
    if (k < 1 || k > 17 || k % 2 == 0) return fail(PK_ERR_ARG, "unitigs need an odd kmer_len of at most 17 (one unsliced table), got %d", k);
    if (device < 0 || device >= MAX_DEVICES) return fail(PK_ERR_ARG, "device ordinal %d out of range", device);
    *out = new pk_unitig();
    (*out)->k = k;
    (*out)->device = device;
    (*out)->n = 1ull << (2 * k);
    return PK_OK;
}

extern "C" void pk_unitig_destroy(pk_unitig *u) { delete u; }

// Arrays sized by what a pass has counted: refused with the size when the device does not hold them.
template <class T> static int reserve_counted(DevBuf<T> &b, uint64_t need, const char *what) {
    if (need <= b.bytes) return PK_OK;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (need > (uint64_t)free_b + b.bytes)
        return fail(PK_ERR_RECS_CAP, "%s take %llu bytes and the device has %llu free: a narrower count window or a larger --min-kmers makes them smaller", what,
                    (unsigned long long)need, (unsigned long long)free_b);
    return b.reserve(need);
}

// ends the timed stretch that began at ev_begin, waits for it, adds its seconds to acc and brings the totals to the host
static int settle(pk_unitig *u, double &acc) {
    HIPCHK(hipEventRecord(u->ev_end, u->stream));
    HIPCHK(hipMemcpyAsync(u->tot, u->totals.p, sizeof u->tot, hipMemcpyDeviceToHost, u->stream));
    HIPCHK(hipStreamSynchronize(u->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, u->ev_begin, u->ev_end));
    acc += ms * 1e-3;
    if (u->tot[UT_ERR])
        return fail(PK_ERR_STATE, "a unitig walk stopped at its step bound or at an impossible link byte (check %llu): the link array is not what the table gives",
                    u->tot[UT_ERR]);
    return PK_OK;
}

static int read_word(pk_unitig *u, const unsigned long long *dev, uint64_t *out) {
    unsigned long long v = 0;
    HIPCHK(hipMemcpyAsync(&v, dev, sizeof v, hipMemcpyDeviceToHost, u->stream));
    HIPCHK(hipStreamSynchronize(u->stream));
    *out = v;
    return PK_OK;
}

static int run_phase(pk_unitig *u, int mode, const uint8_t *table, int min_count, int max_count, uint64_t min_kmers, uint64_t row_base, double &acc) {
    Phase &f = u->ph[mode];
    const uint32_t n_wg = unitig_workgroups(u->n);
    f.m = f.rows = f.bytes = 0;
    HIPCHK(hipEventRecord(u->ev_begin, u->stream));
    if (launch_unitig_count(mode, u->link.p, u->n, u->wg.p, u->stream))
        return fail(PK_ERR_HIP, "launching the unitig count kernels failed: %s", hipGetErrorString(hipGetLastError()));
    if (int rc = settle(u, acc)) return rc;
    if (int rc = read_word(u, u->wg.p + n_wg, &f.m)) return rc;
    if (f.m == 0) return PK_OK;
    const uint64_t m = f.m, rank_wg = unitig_rank_workgroups(m);
    const char *what = mode == UT_ENDS ? "the ends of the linear unitigs" : "the nodes that may lie on cycles";
    if (int rc = reserve_counted(f.cand, m * 8u, what)) return rc;
    if (int rc = reserve_counted(f.c_n, m * 8u, what)) return rc;
    if (int rc = reserve_counted(f.c_depth, m * 8u, what)) return rc;
    if (int rc = reserve_counted(f.c_keep, m, what)) return rc;
    if (int rc = reserve_counted(f.wgA, (rank_wg + 1u) * 8u, what)) return rc;
    if (int rc = reserve_counted(f.wgB, (rank_wg + 1u) * 8u, what)) return rc;
    const uint64_t bound = mode == UT_ENDS ? u->tot[UT_NODES] : m;
    HIPCHK(hipEventRecord(u->ev_begin, u->stream));
    if (launch_unitig_measure(mode, table, u->link.p, u->n, u->k, min_count, max_count, u->wg.p, f.cand.p, m, bound, min_kmers, f.c_n.p, f.c_depth.p,
                              f.c_keep.p, row_base, f.wgA.p, f.wgB.p, u->totals.p, u->stream))
        return fail(PK_ERR_HIP, "launching the unitig measure kernels failed: %s", hipGetErrorString(hipGetLastError()));
    if (int rc = settle(u, acc)) return rc;
    if (int rc = read_word(u, f.wgA.p + rank_wg, &f.rows)) return rc;
    if (int rc = read_word(u, f.wgB.p + rank_wg, &f.bytes)) return rc;
    if (f.rows == 0) return PK_OK;
    what = mode == UT_ENDS ? "the rows and the text of the linear unitigs" : "the rows and the text of the circular unitigs";
    if (int rc = reserve_counted(f.r_addr, f.rows * 8u, what)) return rc;
    if (int rc = reserve_counted(f.r_n, f.rows * 8u, what)) return rc;
    if (int rc = reserve_counted(f.r_depth, f.rows * 8u, what)) return rc;
    if (int rc = reserve_counted(f.r_off, f.rows * 8u, what)) return rc;
    if (int rc = reserve_counted(f.text, f.bytes, what)) return rc;
    HIPCHK(hipEventRecord(u->ev_begin, u->stream));
    if (launch_unitig_spell(u->link.p, u->k, f.cand.p, f.c_keep.p, f.c_n.p, f.c_depth.p, m, f.wgA.p, f.wgB.p, row_base, f.rows, f.r_addr.p, f.r_n.p,
                            f.r_depth.p, f.r_off.p, f.text.p, f.bytes, u->totals.p, u->stream))
        return fail(PK_ERR_HIP, "launching the unitig spell kernels failed: %s", hipGetErrorString(hipGetLastError()));
    return settle(u, acc);
}

extern "C" int pk_unitig_build(pk_unitig *u, const void *dev_table, int min_count, int max_count, uint64_t min_kmers, uint64_t totals_out[8]) {
    if (!u || !totals_out) return fail(PK_ERR_ARG, "null argument");
    if (!dev_table || ((uintptr_t)dev_table & 15u)) return fail(PK_ERR_ARG, "the table must be a 16-byte aligned device pointer");
    if (!(1 <= min_count && min_count <= max_count && max_count <= 255))
        return fail(PK_ERR_ARG, "the count window must satisfy 1 <= min <= max <= 255, got %d-%d", min_count, max_count);
    if (min_kmers < 1) return fail(PK_ERR_ARG, "min_kmers must be at least 1");
    u->built = u->graphed = false;
    if (int rc = ensure_device(u)) return rc;
    const uint8_t *table = (const uint8_t *)dev_table;
    if (int rc = reserve_counted(u->link, (u->n + 15u) & ~15ull, "the link bytes")) return rc;
    if (int rc = u->wg.reserve(((size_t)unitig_workgroups(u->n) + 1u) * sizeof(unsigned long long))) return rc;
    HIPCHK(hipMemsetAsync(u->totals.p, 0, UT_WORDS * sizeof(unsigned long long), u->stream));
    HIPCHK(hipEventRecord(u->ev_begin, u->stream));
    if (launch_unitig_links(table, u->n, u->k, min_count, max_count, u->link.p, u->totals.p, u->stream))
        return fail(PK_ERR_HIP, "launching the unitig link kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (int rc = settle(u, u->t_links)) return rc;
    if (int rc = run_phase(u, UT_ENDS, table, min_count, max_count, min_kmers, 0, u->t_paths)) return rc;
    if (int rc = run_phase(u, UT_LOOPS, table, min_count, max_count, min_kmers, u->ph[0].rows, u->t_cycles)) return rc;
    u->builds++;
    u->built = true;
    totals_out[0] = u->tot[UT_NODES];
    totals_out[1] = u->tot[UT_BRANCHING];
    totals_out[2] = u->ph[0].rows;
    totals_out[3] = u->ph[1].rows;
    totals_out[4] = u->tot[UT_SHORT];
    totals_out[5] = u->tot[UT_NODES_SHORT];
    totals_out[6] = u->ph[0].bytes + u->ph[1].bytes;
    totals_out[7] = u->tot[UT_LONGEST];
    return PK_OK;
}

extern "C" int pk_unitig_rows(pk_unitig *u, uint64_t *first_addr, uint64_t *n_kmers, uint64_t *depth, uint8_t *circular, uint64_t cap) {
    if (!u) return fail(PK_ERR_ARG, "null unitig builder");
    if (!u->built) return fail(PK_ERR_STATE, "pk_unitig_build comes first");
    const uint64_t rows = u->ph[0].rows + u->ph[1].rows;
    if (rows > cap) return fail(PK_ERR_RECS_CAP, "%llu rows do not fit arrays of %llu", (unsigned long long)rows, (unsigned long long)cap);
    if (rows && (!first_addr || !n_kmers || !depth || !circular)) return fail(PK_ERR_ARG, "null pointer with %llu rows", (unsigned long long)rows);
    uint64_t at = 0;
    for (int mode = 0; mode < 2; mode++) {
        Phase &f = u->ph[mode];
        if (!f.rows) continue;
        if (int rc = bounce_copy(f.r_addr.p, first_addr + at, f.rows * 8u, false, u->device)) return rc;
        if (int rc = bounce_copy(f.r_n.p, n_kmers + at, f.rows * 8u, false, u->device)) return rc;
        if (int rc = bounce_copy(f.r_depth.p, depth + at, f.rows * 8u, false, u->device)) return rc;
        memset(circular + at, mode, f.rows);
        at += f.rows;
    }
    return PK_OK;
}

extern "C" int pk_unitig_text(pk_unitig *u, uint8_t *host_out, uint64_t offset, uint64_t n_bytes) {
    if (!u) return fail(PK_ERR_ARG, "null unitig builder");
    if (!u->built) return fail(PK_ERR_STATE, "pk_unitig_build comes first");
    const uint64_t lin = u->ph[0].bytes, all = lin + u->ph[1].bytes;
    if (offset > all || n_bytes > all - offset)
        return fail(PK_ERR_ARG, "bytes %llu + %llu lie outside the %llu bytes of text", (unsigned long long)offset, (unsigned long long)n_bytes,
                    (unsigned long long)all);
    if (n_bytes && !host_out) return fail(PK_ERR_ARG, "null output pointer");
    uint64_t done = 0;
    if (offset < lin && n_bytes) {
        done = std::min(n_bytes, lin - offset);
        if (int rc = bounce_copy(u->ph[0].text.p + offset, host_out, done, false, u->device)) return rc;
    }
    if (done < n_bytes)
        return bounce_copy(u->ph[1].text.p + (offset + done - lin), host_out + done, n_bytes - done, false, u->device);
    return PK_OK;
}

extern "C" int pk_unitig_timings(pk_unitig *u, double out[4]) {
    if (!u || !out) return fail(PK_ERR_ARG, "null argument");
    out[0] = u->t_links;
    out[1] = u->t_paths;
    out[2] = u->t_cycles;
    out[3] = (double)u->builds;
    return PK_OK;
}

// settle() for the graph pass: its checks are 9 and above
static int settle_graph(pk_unitig *u, double &acc) {
    const int rc = settle(u, acc);
    if (rc == PK_ERR_STATE && u->tot[UT_ERR] >= 9)
        return fail(PK_ERR_STATE, "the graph pass met a record beyond its text, an end that no candidate holds or a line beyond its array (check %llu): "
                    "the rows are not what the link array gives", u->tot[UT_ERR]);
    return rc;
}

extern "C" int pk_unitig_graph(pk_unitig *u, uint64_t totals_out[4]) {
    if (!u || !totals_out) return fail(PK_ERR_ARG, "null argument");
    if (!u->built) return fail(PK_ERR_STATE, "pk_unitig_build comes first");
    u->graphed = false;
    HIPCHK(hipSetDevice(u->device));
    u->n_edges = u->edges_dropped = u->n_dead_ends = 0;
    u->gfa_bytes = UG_HEADER;
    u->t_edges = u->t_gfa = 0;
    UgRows R;
    for (int mode = 0; mode < 2; mode++) {
        const Phase &f = u->ph[mode];
        R.n[mode] = f.r_n.p; R.depth[mode] = f.r_depth.p; R.off[mode] = f.r_off.p; R.text[mode] = f.text.p; R.text_bytes[mode] = f.bytes;
    }
    R.rows0 = u->ph[0].rows;
    R.rows = R.rows0 + u->ph[1].rows;
    const uint64_t m = u->ph[0].m;
    if (R.rows) {
        const uint32_t n_wgE = unitig_rank_workgroups(2u * R.rows), n_wgS = unitig_rank_workgroups(R.rows);
        if (int rc = reserve_counted(u->end_row, m * 8u, "the rows of the unitig ends")) return rc;
        if (int rc = reserve_counted(u->wgE, (n_wgE + 1ull) * 8u, "the edge counts")) return rc;
        HIPCHK(hipMemsetAsync(u->totals.p + UG_DROPPED, 0, 2 * sizeof(unsigned long long), u->stream));
        if (m) HIPCHK(hipMemsetAsync(u->end_row.p, 0xff, m * 8u, u->stream));
        HIPCHK(hipEventRecord(u->ev_begin, u->stream));
        if (launch_unitig_edges_count(R, u->k, u->link.p, u->ph[0].r_addr.p, u->ph[0].cand.p, m, u->end_row.p, u->wgE.p, u->totals.p, u->stream))
            return fail(PK_ERR_HIP, "launching the unitig edge count kernels failed: %s", hipGetErrorString(hipGetLastError()));
        if (int rc = settle_graph(u, u->t_edges)) return rc;
        if (int rc = read_word(u, u->wgE.p + n_wgE, &u->n_edges)) return rc;
        u->edges_dropped = u->tot[UG_DROPPED];
        u->n_dead_ends = u->tot[UG_DEAD];
        const uint64_t E = u->n_edges;
        if (E) {
            const char *what = "the edges between the unitigs";
            if (int rc = reserve_counted(u->e_from, E * 8u, what)) return rc;
            if (int rc = reserve_counted(u->e_to, E * 8u, what)) return rc;
            if (int rc = reserve_counted(u->e_orient, E, what)) return rc;
            HIPCHK(hipEventRecord(u->ev_begin, u->stream));
            if (launch_unitig_edges_fill(R, u->k, u->link.p, u->ph[0].cand.p, m, u->end_row.p, u->wgE.p, E, u->e_from.p, u->e_to.p, u->e_orient.p,
                                         u->totals.p, u->stream))
                return fail(PK_ERR_HIP, "launching the unitig edge fill kernel failed: %s", hipGetErrorString(hipGetLastError()));
            if (int rc = settle_graph(u, u->t_edges)) return rc;
        }
        const uint32_t n_wgL = unitig_rank_workgroups(E);
        if (int rc = reserve_counted(u->wgS, (n_wgS + 1ull) * 8u, "the sizes of the GFA lines")) return rc;
        if (int rc = reserve_counted(u->wgL, (n_wgL + 1ull) * 8u, "the sizes of the GFA lines")) return rc;
        HIPCHK(hipEventRecord(u->ev_begin, u->stream));
        if (launch_unitig_gfa_sizes(R, u->k, u->e_from.p, u->e_to.p, E, u->wgS.p, u->wgL.p, u->stream))
            return fail(PK_ERR_HIP, "launching the GFA size kernels failed: %s", hipGetErrorString(hipGetLastError()));
        if (int rc = settle_graph(u, u->t_gfa)) return rc;
        uint64_t s_bytes = 0, l_bytes = 0;
        if (int rc = read_word(u, u->wgS.p + n_wgS, &s_bytes)) return rc;
        if (int rc = read_word(u, u->wgL.p + n_wgL, &l_bytes)) return rc;
        u->gfa_bytes = UG_HEADER + s_bytes + l_bytes;
        if (int rc = reserve_counted(u->gfa, u->gfa_bytes, "the GFA text")) return rc;
        HIPCHK(hipEventRecord(u->ev_begin, u->stream));
        if (launch_unitig_gfa_write(R, u->k, u->e_from.p, u->e_to.p, u->e_orient.p, E, u->wgS.p, u->wgL.p, u->gfa.p, u->gfa_bytes, u->totals.p, u->stream))
            return fail(PK_ERR_HIP, "launching the GFA line kernels failed: %s", hipGetErrorString(hipGetLastError()));
        if (int rc = settle_graph(u, u->t_gfa)) return rc;
    } else if (int rc = reserve_counted(u->gfa, UG_HEADER, "the GFA text")) {
        return rc;
    }
    static const char header[UG_HEADER + 1] = "H\tVN:Z:1.0\n";
    HIPCHK(hipMemcpyAsync(u->gfa.p, header, UG_HEADER, hipMemcpyHostToDevice, u->stream));
    HIPCHK(hipStreamSynchronize(u->stream));
    u->graphed = true;
    totals_out[0] = u->n_edges;
    totals_out[1] = u->edges_dropped;
    totals_out[2] = u->n_dead_ends;
    totals_out[3] = u->gfa_bytes;
    return PK_OK;
}

extern "C" int pk_unitig_edges(pk_unitig *u, uint64_t *from, uint64_t *to, uint8_t *orient, uint64_t cap) {
    if (!u) return fail(PK_ERR_ARG, "null unitig builder");
    if (!u->built) return fail(PK_ERR_STATE, "pk_unitig_build comes first");
    if (!u->graphed) return fail(PK_ERR_STATE, "pk_unitig_graph comes first, after the last pk_unitig_build");
    const uint64_t E = u->n_edges;
    if (E > cap) return fail(PK_ERR_RECS_CAP, "%llu edges do not fit arrays of %llu", (unsigned long long)E, (unsigned long long)cap);
    if (!E) return PK_OK;
    if (!from || !to || !orient) return fail(PK_ERR_ARG, "null pointer with %llu edges", (unsigned long long)E);
    if (int rc = bounce_copy(u->e_from.p, from, E * 8u, false, u->device)) return rc;
    if (int rc = bounce_copy(u->e_to.p, to, E * 8u, false, u->device)) return rc;
    return bounce_copy(u->e_orient.p, orient, E, false, u->device);
}

extern "C" int pk_unitig_gfa_text(pk_unitig *u, uint8_t *host_out, uint64_t offset, uint64_t n_bytes) {
    if (!u) return fail(PK_ERR_ARG, "null unitig builder");
    if (!u->built) return fail(PK_ERR_STATE, "pk_unitig_build comes first");
    if (!u->graphed) return fail(PK_ERR_STATE, "pk_unitig_graph comes first, after the last pk_unitig_build");
    if (offset > u->gfa_bytes || n_bytes > u->gfa_bytes - offset)
        return fail(PK_ERR_ARG, "bytes %llu + %llu lie outside the %llu bytes of GFA text", (unsigned long long)offset, (unsigned long long)n_bytes,
                    (unsigned long long)u->gfa_bytes);
    if (!n_bytes) return PK_OK;
    if (!host_out) return fail(PK_ERR_ARG, "null output pointer");
    return bounce_copy(u->gfa.p + offset, host_out, n_bytes, false, u->device);
}

extern "C" int pk_unitig_graph_timings(pk_unitig *u, double out[2]) {
    if (!u || !out) return fail(PK_ERR_ARG, "null argument");
    out[0] = u->t_edges;
    out[1] = u->t_gfa;
    return PK_OK;
}
