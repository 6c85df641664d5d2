// kmer_unitig.hip -- the unitigs of one table: the compacted de Bruijn graph of the nodes
//   S = { canonical x : min <= T[x] <= max },
// spelled as FASTA on the device.  No reference counterpart (the BCALM step behind a k-mer count).
//
// With out(o) = { t = ((o << 2) | b) & (4^k - 1), b = 0..3 : canon(t) in S } and in(t) = { p : t in out(p) }, the edge o -> t
// is compactable iff |out(o)| = 1, |in(t)| = 1 and canon(o) != canon(t).  Compactable edges are symmetric (o -> t iff
// rc(t) -> rc(o)), so they are a matching on (node, side): every component is a simple path or a simple cycle.
//
// The link byte of a canonical address x (0 where x is no node):
//   bit 0      x is a node
//   bit 1      a compactable edge leaves x itself (its RIGHT side); bits 2-3: the base b of that edge
//   bit 4      a compactable edge leaves rc(x) (its LEFT side);     bits 5-6: the base b of that edge
//   bit 7      seen: the node lies on a path that a walk has measured
// A walk holds an oriented k-mer o; at node y = canon(o) it leaves by the right side iff o == y, and the next oriented
// k-mer is ((o << 2) | b) & (4^k - 1) with that side's base.
//
//   k_ut_links     a dense pass: a thread takes 16 consecutive addresses, and for every node among them up to 8 loads per side
//                  for the two degrees; one link byte per address, and the tallies of nodes and branching nodes
//   k_ut_count     per workgroup, the link bytes that are ENDS (a node with a side without link) or LOOPS (a node with both
//   k_ut_compact   sides linked and not seen); their addresses, ascending (the tile compaction of kmer_extract.hip)
//   k_ut_measure   one lane per end walks to the other end, marks every node seen, sums n and depth; the end OWNS its path
//                  iff n = 1 or its address is below the other end's.  One lane per loop candidate walks forward from the
//                  canonical string and stops at the first node with a smaller address: only a cycle's minimum completes it.
//   k_ut_rank_*    the rows (owners with n >= min_kmers, in candidate order = ascending first_addr) and the offsets of their
//                  records, `>` row `\n` text `\n`: two workgroup-sum + scan rounds
//   k_ut_rows      the row arrays
//   k_ut_spell     one lane per row walks again and writes its record
// Every walk carries a step bound that a correct walk cannot reach (the nodes for paths, the candidates for cycles); a lane
// that reaches it, or meets a link byte that cannot be, raises the error word and returns.
//
// The graph pass (pk_unitig_graph, after a build; no table): the edges between the written rows and the GFA text.  With
// tail(r,+) = o_1, head(r,+) = o_n, tail(r,-) = rc(o_n), head(r,-) = rc(o_1), (r,s) -> (q,u) is an edge iff
// tail(q,u) in out(head(r,s)); membership of t is link[canon(t)] & LK_NODE.  Heads and tails are read off the FASTA records.
//   k_ug_ends      one lane per linear row: end_row[i] = row << 1 | s for the candidate i (an index into the ends of the linear
//                  phase, ascending) of each of its two end nodes y, where a successor t with canon(t) = y is the tail
//                  (row, s ^ (t != y)); UG_NONE stays where the end belongs to a unitig that min_kmers dropped
//   k_ug_count     one lane per (row, sign): the head, its four successors, four link bytes, and per member a binary search
//                  of canon(t) in the ends; the edges per workgroup, and the tallies of dropped edges and dead ends
//   k_ug_fill      the same again behind the scan: from, to, orient at the scanned offsets, in (row, sign, base) order.  A
//                  circular row emits (c,s) -> (c,s) without a lookup.
//   k_ug_sizes_*   the bytes of the S-lines per 256 rows and of the L-lines per 256 edges, for the two scans
//   k_ug_slines    a workgroup writes the S-lines of its 256 rows, k_ug_llines the L-lines of its 256 edges: one thread per
//                  output byte, which finds its line in the workgroup's scanned sizes in LDS and its place in the line; the
//                  sequence is copied out of the FASTA text
// No loop here depends on the data beyond its length: the searches take at most 64 steps.  Checks 9 to 12 of the error word:
// a record that passes its text, an end or a member that no candidate holds, an edge or a line beyond its array.
#include "pk_kernels.h"
#include "wg_scan.h"

namespace pk {

constexpr int UT = 256;                          // threads per workgroup of the dense and the rank passes
constexpr uint32_t U_ADDR = 16;                  // addresses per thread and step
constexpr uint32_t U_TILE = UT * U_ADDR;         // addresses per step of a workgroup
constexpr uint32_t U_STEPS = 4;
constexpr uint64_t U_WG = (uint64_t)U_TILE * U_STEPS;
constexpr int UW = 64;                           // threads per workgroup of the walks: one wave, so that long walks spread over the CUs

constexpr uint32_t LK_NODE = 0x01u, LK_R = 0x02u, LK_L = 0x10u, LK_SEEN = 0x80u;
constexpr uint32_t LK_BOTH = LK_NODE | LK_R | LK_L;

struct UtParams {
    uint32_t k, lo, hi;
    uint64_t mask;                               // 4^k - 1
};

__device__ __forceinline__ uint64_t ut_rc(uint64_t o, uint32_t k) {
    uint64_t x = ~o;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(x) >> (64u - 2u * k);
}
__device__ __forceinline__ uint64_t ut_canon(uint64_t o, uint32_t k) { const uint64_t r = ut_rc(o, k); return o < r ? o : r; }
__device__ __forceinline__ bool ut_member(const uint8_t *__restrict__ T, uint64_t o, const UtParams &p) {
    const uint32_t v = T[ut_canon(o, p.k)];
    return v >= p.lo && v <= p.hi;
}

// The side of node x that the oriented k-mer o (x or rc(x)) leaves by: 1 | b << 1 if the one edge o -> t is compactable,
// else 0.  many: |out(o)| >= 2.
__device__ __forceinline__ uint32_t ut_side(const uint8_t *__restrict__ T, uint64_t o, uint64_t x, const UtParams &p, bool &many) {
    uint32_t cnt = 0, b1 = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; b++)
        if (ut_member(T, ((o << 2) | b) & p.mask, p)) { cnt++; b1 = b; }
    many = cnt >= 2u;
    if (cnt != 1u) return 0u;
    const uint64_t t = ((o << 2) | b1) & p.mask;
    if (ut_canon(t, p.k) == x) return 0u;        // a self-loop or a hairpin: counted, never compacted
    uint32_t in = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) in += ut_member(T, (t >> 2) | ((uint64_t)c << (2u * (p.k - 1u))), p);
    return in == 1u ? (1u | (b1 << 1)) : 0u;
}

// 16 bytes at a + off, cut at n (the bytes at or beyond n read as 0)
__device__ __forceinline__ void ut_load16(const uint8_t *__restrict__ a, uint64_t off, uint64_t n, uint32_t (&w)[4]) {
    if (off + U_ADDR <= n) {
        const uint4 x = *(const uint4 *)(a + off);
        w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
        for (uint64_t i = off; i < n; i++) w[(i - off) >> 2] |= (uint32_t)a[i] << (8u * ((i - off) & 3u));
    }
}

// totals: UT_NODES .. UT_ERR words, zeroed by the caller
__global__ __launch_bounds__(UT) void k_ut_links(const uint8_t *__restrict__ T, uint64_t n, UtParams p, uint8_t *__restrict__ link,
                                                 unsigned long long *__restrict__ totals) {
    __shared__ uint32_t wsum[2][UT / 64];
    uint32_t nodes = 0, branching = 0;
    for (uint32_t s = 0; s < U_STEPS; s++) {
        const uint64_t off = (uint64_t)blockIdx.x * U_WG + (uint64_t)s * U_TILE + (uint64_t)threadIdx.x * U_ADDR;
        if (off >= n) break;
        uint32_t w[4], r[4] = {0, 0, 0, 0};
        ut_load16(T, off, n, w);
        if (w[0] | w[1] | w[2] | w[3]) {
            for (uint32_t j = 0; j < U_ADDR; j++) {
                const uint32_t v = (w[j >> 2] >> (8u * (j & 3u))) & 0xffu;
                if (v < p.lo || v > p.hi) continue;
                const uint64_t x = off + j, xr = ut_rc(x, p.k);
                if (x > xr) continue;            // not a canonical address: no node
                bool many_r, many_l;
                const uint32_t right = ut_side(T, x, x, p, many_r), left = ut_side(T, xr, x, p, many_l);
                r[j >> 2] |= (LK_NODE | (right << 1) | (left << 4)) << (8u * (j & 3u));
                nodes++;
                branching += many_r || many_l;
            }
        }
        if (off + U_ADDR <= n) *(uint4 *)(link + off) = make_uint4(r[0], r[1], r[2], r[3]);
        else for (uint64_t i = off; i < n; i++) link[i] = (uint8_t)(r[(i - off) >> 2] >> (8u * ((i - off) & 3u)));
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { nodes += __shfl_down(nodes, d, 64); branching += __shfl_down(branching, d, 64); }
    if ((threadIdx.x & 63u) == 0u) { wsum[0][threadIdx.x >> 6] = nodes; wsum[1][threadIdx.x >> 6] = branching; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (int i = 0; i < UT / 64; i++) { a += wsum[0][i]; b += wsum[1][i]; }
        if (a) atomicAdd(totals + UT_NODES, (unsigned long long)a);
        if (b) atomicAdd(totals + UT_BRANCHING, (unsigned long long)b);
    }
}

// bit j: link byte off + j is selected.  ENDS: a node with a side without link; LOOPS: a node with both sides linked, not seen
template <int MODE> __device__ __forceinline__ uint32_t ut_mask16(const uint8_t *__restrict__ link, uint64_t off, uint64_t n) {
    uint32_t w[4], mask = 0;
    ut_load16(link, off, n, w);
    if (!(w[0] | w[1] | w[2] | w[3])) return 0u;
#pragma unroll
    for (uint32_t j = 0; j < U_ADDR; j++) {
        const uint32_t b = (w[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        const bool sel = MODE == UT_ENDS ? ((b & LK_NODE) && (b & LK_BOTH) != LK_BOTH) : ((b & (LK_BOTH | LK_SEEN)) == LK_BOTH);
        mask |= (uint32_t)sel << j;
    }
    return mask;
}

template <int MODE> __global__ __launch_bounds__(UT) void k_ut_count(const uint8_t *__restrict__ link, uint64_t n, unsigned long long *__restrict__ wg_count) {
    __shared__ uint32_t wsum[UT / 64];
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < U_STEPS; s++) {
        const uint64_t off = (uint64_t)blockIdx.x * U_WG + (uint64_t)s * U_TILE + (uint64_t)threadIdx.x * U_ADDR;
        if (off >= n) break;
        cnt += __popc(ut_mask16<MODE>(link, off, n));
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < UT / 64; w++) tot += wsum[w];
        wg_count[blockIdx.x] = tot;
    }
}

// wg: the scanned workgroup counts, wg[n_wg] the total; nothing is written when the total exceeds cap
template <int MODE> __global__ __launch_bounds__(UT) void k_ut_compact(const uint8_t *__restrict__ link, uint64_t n, const unsigned long long *__restrict__ wg,
                                                                      uint32_t n_wg, uint64_t cap, unsigned long long *__restrict__ addr_out) {
    __shared__ uint16_t sel[U_TILE];
    __shared__ uint32_t wsum[UT / 64];
    if (wg[n_wg] > cap) return;
    unsigned long long rank = wg[blockIdx.x];
    if (wg[blockIdx.x + 1u] == rank) return;
    for (uint32_t s = 0; s < U_STEPS; s++) {
        const uint64_t tile = (uint64_t)blockIdx.x * U_WG + (uint64_t)s * U_TILE;
        if (tile >= n) break;
        const uint64_t off = tile + (uint64_t)threadIdx.x * U_ADDR;
        uint32_t mask = off < n ? ut_mask16<MODE>(link, off, n) : 0u;
        uint32_t S;                              // the barrier in front: the previous step's readers of sel and wsum are done
        uint32_t r = wg_excl_sum<UT / 64, true>((uint32_t)__popc(mask), wsum, S);
        if (S == 0u) continue;                   // uniform
        while (mask) {
            const uint32_t j = __ffs(mask) - 1u;
            mask &= mask - 1u;
            sel[r++] = (uint16_t)(threadIdx.x * U_ADDR + j);
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < S; i += UT) addr_out[rank + i] = tile + sel[i];
        rank += S;
    }
}

__device__ __forceinline__ void ut_raise(unsigned long long *totals, unsigned long long what) { atomicMax(totals + UT_ERR, what); }

// the oriented k-mer a row is spelled from: the node itself unless only its left side is linked
__device__ __forceinline__ uint64_t ut_first(uint64_t x, uint32_t lk, uint32_t k) { return ((lk & LK_R) || !(lk & LK_L)) ? x : ut_rc(x, k); }
// the link bits (1 | b << 1, or 0) of the side by which the oriented k-mer o leaves its node y, link byte lk
__device__ __forceinline__ uint32_t ut_leave(uint64_t o, uint64_t y, uint32_t lk) { return (o == y ? lk >> 1 : lk >> 4) & 7u; }

// c_n, c_depth, c_keep [m]: per candidate the k-mers and the depth of what it owns, and whether that is a row
template <int MODE> __global__ __launch_bounds__(UW) void k_ut_measure(const uint8_t *__restrict__ T, uint8_t *link, UtParams p,
                                                                      const unsigned long long *__restrict__ cand, uint64_t m, uint64_t bound,
                                                                      uint64_t min_kmers, unsigned long long *__restrict__ c_n,
                                                                      unsigned long long *__restrict__ c_depth, uint8_t *__restrict__ c_keep,
                                                                      unsigned long long *__restrict__ totals) {
    const uint64_t i = (uint64_t)blockIdx.x * UW + threadIdx.x;
    if (i >= m) return;
    c_n[i] = 0; c_depth[i] = 0; c_keep[i] = 0;
    const uint64_t x = cand[i];
    uint32_t lk = link[x];
    if (!(lk & LK_NODE)) { ut_raise(totals, 1); return; }
    uint64_t o = MODE == UT_ENDS ? ut_first(x, lk, p.k) : x, y = x, n = 1, depth = T[x];
    bool owner = false;
    if (MODE == UT_ENDS) {
        link[x] = (uint8_t)(lk | LK_SEEN);       // both ends of a path write the same byte into every node of it
        for (;;) {
            const uint32_t side = ut_leave(o, y, lk);
            if (!(side & 1u)) break;
            if (n >= bound) { ut_raise(totals, 2); return; }
            o = ((o << 2) | (side >> 1)) & p.mask;
            y = ut_canon(o, p.k);
            lk = link[y];
            if (!(lk & LK_NODE)) { ut_raise(totals, 3); return; }
            link[y] = (uint8_t)(lk | LK_SEEN);
            n++;
            depth += T[y];
        }
        owner = n == 1u || x < y;
    } else {
        for (;;) {
            const uint32_t side = ut_leave(o, y, lk);
            if (!(side & 1u)) { ut_raise(totals, 4); return; }     // a node of a cycle has both sides linked
            o = ((o << 2) | (side >> 1)) & p.mask;
            y = ut_canon(o, p.k);
            if (y == x) { owner = true; break; }
            if (y < x) break;                    // not the cycle's smallest address
            if (n >= bound) { ut_raise(totals, 5); return; }
            lk = link[y];
            n++;
            depth += T[y];
        }
    }
    if (!owner) return;
    if (n >= min_kmers) {
        c_n[i] = n; c_depth[i] = depth; c_keep[i] = 1;
        atomicMax(totals + UT_LONGEST, (unsigned long long)n);
    } else {
        atomicAdd(totals + UT_SHORT, 1ull);
        atomicAdd(totals + UT_NODES_SHORT, (unsigned long long)n);
    }
}

__device__ __forceinline__ uint32_t ut_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10ull) { v /= 10ull; d++; }
    return d;
}
// the bytes of row `row` (its index among all rows) with n k-mers: '>' digits '\n' n + k - 1 letters '\n'
__device__ __forceinline__ uint64_t ut_record(uint64_t row, uint64_t n, uint32_t k) { return n + k - 1u + 3u + ut_digits(row); }

// wgA[b] = the rows of workgroup b's candidates
__global__ __launch_bounds__(UT) void k_ut_rank_rows(const uint8_t *__restrict__ c_keep, uint64_t m, unsigned long long *__restrict__ wgA) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x;
    unsigned long long total;
    wg_excl_sum<UT / 64, false>((unsigned long long)(i < m ? c_keep[i] : 0), sh, total);
    if (threadIdx.x == 0) wgA[blockIdx.x] = total;
}
// wgA scanned; wgB[b] = the record bytes of workgroup b's rows
__global__ __launch_bounds__(UT) void k_ut_rank_bytes(const uint8_t *__restrict__ c_keep, const unsigned long long *__restrict__ c_n, uint64_t m,
                                                      const unsigned long long *__restrict__ wgA, uint64_t row_base, uint32_t k,
                                                      unsigned long long *__restrict__ wgB) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x;
    const unsigned long long keep = i < m ? c_keep[i] : 0;
    unsigned long long total;
    const unsigned long long row = wgA[blockIdx.x] + wg_excl_sum<UT / 64, false>(keep, sh, total);
    const unsigned long long size = keep ? ut_record(row_base + row, c_n[i], k) : 0ull;
    wg_excl_sum<UT / 64, true>(size, sh, total);
    if (threadIdx.x == 0) wgB[blockIdx.x] = total;
}
// wgA and wgB scanned: the row arrays, r_off the offset of the row's record in the phase's text
__global__ __launch_bounds__(UT) void k_ut_rows(const unsigned long long *__restrict__ cand, const uint8_t *__restrict__ c_keep,
                                                const unsigned long long *__restrict__ c_n, const unsigned long long *__restrict__ c_depth, uint64_t m,
                                                const unsigned long long *__restrict__ wgA, const unsigned long long *__restrict__ wgB, uint64_t row_base,
                                                uint32_t k, uint64_t rows, unsigned long long *__restrict__ r_addr, unsigned long long *__restrict__ r_n,
                                                unsigned long long *__restrict__ r_depth, unsigned long long *__restrict__ r_off,
                                                unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x;
    const unsigned long long keep = i < m ? c_keep[i] : 0;
    unsigned long long total;
    const unsigned long long row = wgA[blockIdx.x] + wg_excl_sum<UT / 64, false>(keep, sh, total);
    const unsigned long long size = keep ? ut_record(row_base + row, c_n[i], k) : 0ull;
    const unsigned long long off = wgB[blockIdx.x] + wg_excl_sum<UT / 64, true>(size, sh, total);
    if (!keep) return;
    if (row >= rows) { ut_raise(totals, 6); return; }
    r_addr[row] = cand[i]; r_n[row] = c_n[i]; r_depth[row] = c_depth[i]; r_off[row] = off;
}

// one lane per row: its record at text + r_off[row]
__global__ __launch_bounds__(UW) void k_ut_spell(const uint8_t *__restrict__ link, UtParams p, const unsigned long long *__restrict__ r_addr,
                                                 const unsigned long long *__restrict__ r_n, const unsigned long long *__restrict__ r_off, uint64_t rows,
                                                 uint64_t row_base, uint8_t *__restrict__ text, uint64_t text_bytes,
                                                 unsigned long long *__restrict__ totals) {
    const uint64_t row = (uint64_t)blockIdx.x * UW + threadIdx.x;
    if (row >= rows) return;
    const uint64_t x = r_addr[row], n = r_n[row], off = r_off[row];
    const uint32_t nd = ut_digits(row_base + row);
    if (n == 0u || off > text_bytes || ut_record(row_base + row, n, p.k) > text_bytes - off) { ut_raise(totals, 7); return; }
    uint8_t *w = text + off;
    *w = (uint8_t)'>';
    uint64_t v = row_base + row;
    for (uint32_t d = nd; d >= 1u; d--) { w[d] = (uint8_t)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
    w += nd + 1u;
    *w++ = (uint8_t)'\n';
    uint32_t lk = link[x];
    uint64_t o = ut_first(x, lk, p.k), y = x;
    for (uint32_t c = 0; c < p.k; c++) *w++ = (uint8_t)((0x54474341u >> (8u * (uint32_t)((o >> (2u * (p.k - 1u - c))) & 3ull))) & 0xffu);   // "ACGT"
    for (uint64_t s = 1; s < n; s++) {
        const uint32_t side = ut_leave(o, y, lk);
        if (!(side & 1u)) { ut_raise(totals, 8); return; }
        o = ((o << 2) | (side >> 1)) & p.mask;
        y = ut_canon(o, p.k);
        lk = link[y];
        *w++ = (uint8_t)((0x54474341u >> (8u * (uint32_t)(o & 3ull))) & 0xffu);
    }
    *w = (uint8_t)'\n';
}

// ------------------------------------------------------------------ the graph pass: edges and GFA text ----------------
constexpr unsigned long long UG_NONE = ~0ull;

__device__ __forceinline__ uint64_t ug_kmer(const uint8_t *__restrict__ s, uint32_t k) {
    uint64_t o = 0;
    for (uint32_t c = 0; c < k; c++) { const uint32_t a = s[c]; o = (o << 2) | (((a >> 1) & 3u) ^ ((a >> 2) & 1u)); }      // A, C, G, T -> 0 .. 3
    return o;
}

// the index of x in cand[0, m), ascending; m where it is absent
__device__ __forceinline__ uint64_t ug_find(const unsigned long long *__restrict__ cand, uint64_t m, uint64_t x) {
    uint64_t lo = 0, hi = m;
    for (uint32_t step = 0; step < 64u && lo < hi; step++) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (cand[mid] < x) lo = mid + 1u; else hi = mid;
    }
    return lo < m && cand[lo] == x ? lo : m;
}

// row g of all rows: its k-mers, its depth and the first letter of its sequence in its phase's FASTA text; false where the
// record passes the end of that text
__device__ __forceinline__ bool ug_row(const UgRows &R, uint32_t k, uint64_t g, uint64_t &n, uint64_t &depth, const uint8_t *&seq) {
    const uint32_t ph = g >= R.rows0;
    const uint64_t i = g - (ph ? R.rows0 : 0ull), off = R.off[ph][i];
    n = R.n[ph][i];
    depth = R.depth[ph][i];
    if (n == 0u || off > R.text_bytes[ph] || ut_record(g, n, k) > R.text_bytes[ph] - off) return false;
    seq = R.text[ph] + off + 2u + ut_digits(g);
    return true;
}

__global__ __launch_bounds__(UT) void k_ug_ends(UgRows R, uint32_t k, const unsigned long long *__restrict__ r_addr,
                                                const unsigned long long *__restrict__ cand, uint64_t m, unsigned long long *__restrict__ end_row,
                                                unsigned long long *__restrict__ totals) {
    const uint64_t g = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (g >= R.rows0) return;
    uint64_t n, depth;
    const uint8_t *seq;
    if (!ug_row(R, k, g, n, depth, seq)) { ut_raise(totals, 9); return; }
    const uint64_t o1 = ug_kmer(seq, k), y1 = ut_canon(o1, k), i = ug_find(cand, m, y1);
    if (y1 != r_addr[g] || i == m) { ut_raise(totals, 10); return; }
    end_row[i] = (g << 1) | (unsigned long long)(o1 != y1);              // tail(g,+) = o_1
    if (n == 1u) return;
    const uint64_t t = ut_rc(ug_kmer(seq + (n - 1u), k), k), y2 = ut_canon(t, k), j = ug_find(cand, m, y2);
    if (j == m || j == i) { ut_raise(totals, 10); return; }
    end_row[j] = (g << 1) | (unsigned long long)(t == y2);               // tail(g,-) = rc(o_n)
}

// What leaves the oriented row `lane` = row << 1 | sign.  bit b of mask: the successor with base b is the tail of the written
// row to[b], read as sign[b]; dropped: the members whose unitig has no row.  false (the error word is raised): nothing to use.
__device__ __forceinline__ bool ug_out(const UgRows &R, const UtParams &p, const uint8_t *__restrict__ link, const unsigned long long *__restrict__ cand,
                                       uint64_t m, const unsigned long long *__restrict__ end_row, uint64_t lane, uint32_t &mask, uint64_t (&to)[4],
                                       uint32_t (&sign)[4], uint32_t &dropped, unsigned long long *__restrict__ totals) {
    const uint64_t g = lane >> 1;
    const uint32_t s = (uint32_t)(lane & 1u);
    mask = 0; dropped = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; b++) { to[b] = 0; sign[b] = 0; }
    if (g >= R.rows0) { mask = 1u; to[0] = g; sign[0] = s; return true; }       // a cycle's closing edge, read this way round
    uint64_t n, depth;
    const uint8_t *seq;
    if (!ug_row(R, p.k, g, n, depth, seq)) { ut_raise(totals, 9); return false; }
    const uint64_t head = s ? ut_rc(ug_kmer(seq, p.k), p.k) : ug_kmer(seq + (n - 1u), p.k);
#pragma unroll
    for (uint32_t b = 0; b < 4u; b++) {
        const uint64_t t = ((head << 2) | b) & p.mask, y = ut_canon(t, p.k);
        if (!(link[y] & LK_NODE)) continue;
        const uint64_t j = ug_find(cand, m, y);
        if (j == m) { ut_raise(totals, 10); mask = 0; return false; }
        const unsigned long long e = end_row[j];
        if (e == UG_NONE) { dropped++; continue; }
        mask |= 1u << b;
        to[b] = e >> 1;
        sign[b] = (uint32_t)(e & 1u) ^ (uint32_t)(t != y);
    }
    return true;
}

// a lane's tallies in one word for one workgroup sum: edges (at most 4 * 256), dropped edges, dead ends
constexpr uint32_t UG_F = 16;
constexpr unsigned long long UG_FMASK = (1ull << UG_F) - 1ull;

__global__ __launch_bounds__(UT) void k_ug_count(UgRows R, UtParams p, const uint8_t *__restrict__ link, const unsigned long long *__restrict__ cand,
                                                 uint64_t m, const unsigned long long *__restrict__ end_row, unsigned long long *__restrict__ wgE,
                                                 unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t lane = (uint64_t)blockIdx.x * UT + threadIdx.x;
    unsigned long long v = 0;
    if (lane < 2u * R.rows) {
        uint32_t mask, dropped, sign[4];
        uint64_t to[4];
        if (ug_out(R, p, link, cand, m, end_row, lane, mask, to, sign, dropped, totals))
            v = (unsigned long long)__popc(mask) | ((unsigned long long)dropped << UG_F) | ((unsigned long long)(mask == 0u) << (2u * UG_F));
    }
    unsigned long long total;
    wg_excl_sum<UT / 64, false>(v, sh, total);
    if (threadIdx.x == 0) {
        wgE[blockIdx.x] = total & UG_FMASK;
        if ((total >> UG_F) & UG_FMASK) atomicAdd(totals + UG_DROPPED, (total >> UG_F) & UG_FMASK);
        if (total >> (2u * UG_F)) atomicAdd(totals + UG_DEAD, total >> (2u * UG_F));
    }
}

// wgE scanned
__global__ __launch_bounds__(UT) void k_ug_fill(UgRows R, UtParams p, const uint8_t *__restrict__ link, const unsigned long long *__restrict__ cand,
                                                uint64_t m, const unsigned long long *__restrict__ end_row, const unsigned long long *__restrict__ wgE,
                                                uint64_t n_edges, unsigned long long *__restrict__ from, unsigned long long *__restrict__ to_out,
                                                uint8_t *__restrict__ orient, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t lane = (uint64_t)blockIdx.x * UT + threadIdx.x;
    uint32_t mask = 0, dropped, sign[4];
    uint64_t to[4];
    if (lane < 2u * R.rows && !ug_out(R, p, link, cand, m, end_row, lane, mask, to, sign, dropped, totals)) mask = 0;
    unsigned long long total;
    const uint32_t cnt = __popc(mask);
    uint64_t at = wgE[blockIdx.x] + wg_excl_sum<UT / 64, false>((unsigned long long)cnt, sh, total);
    if (!cnt) return;
    if (at > n_edges || cnt > n_edges - at) { ut_raise(totals, 11); return; }
#pragma unroll
    for (uint32_t b = 0; b < 4u; b++) {
        if (!((mask >> b) & 1u)) continue;
        from[at] = lane >> 1;
        to_out[at] = to[b];
        orient[at] = (uint8_t)((uint32_t)(lane & 1u) | (sign[b] << 1));
        at++;
    }
}

// little-endian: byte i of the word is s[i]
constexpr uint64_t ug_word(const char *s) {
    uint64_t v = 0;
    for (int i = 0; i < 8 && s[i]; i++) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
    return v;
}
__device__ __forceinline__ uint8_t ug_at(uint64_t word, uint64_t i) { return (uint8_t)(word >> (8u * (uint32_t)i)); }
// digit j, from the left, of the d digits of v
__device__ __forceinline__ uint8_t ug_digit(uint64_t v, uint32_t d, uint64_t j) {
    for (uint32_t i = (uint32_t)j + 1u; i < d; i++) v /= 10ull;
    return (uint8_t)('0' + (uint32_t)(v % 10ull));
}

// S <row> <text> LN:i:<L> KC:i:<depth>, tab separated
__device__ __forceinline__ uint64_t ug_s_size(uint64_t g, uint64_t n, uint64_t depth, uint32_t k) {
    const uint64_t L = n + k - 1u;
    return L + 16u + ut_digits(g) + ut_digits(L) + ut_digits(depth);
}
__device__ __forceinline__ uint8_t ug_s_byte(uint64_t g, uint64_t n, uint64_t depth, const uint8_t *__restrict__ seq, uint32_t k, uint64_t q) {
    const uint64_t L = n + k - 1u;
    const uint32_t dg = ut_digits(g), dl = ut_digits(L), dd = ut_digits(depth);
    if (q < 2u) return ug_at(ug_word("S\t"), q);
    q -= 2u;
    if (q < dg) return ug_digit(g, dg, q);
    q -= dg;
    if (q == 0u) return (uint8_t)'\t';
    q -= 1u;
    if (q < L) return seq[q];
    q -= L;
    if (q < 6u) return ug_at(ug_word("\tLN:i:"), q);
    q -= 6u;
    if (q < dl) return ug_digit(L, dl, q);
    q -= dl;
    if (q < 6u) return ug_at(ug_word("\tKC:i:"), q);
    q -= 6u;
    return q < dd ? ug_digit(depth, dd, q) : (uint8_t)'\n';
}

// L <from> <sign> <to> <sign> <k-1>M, tab separated
__device__ __forceinline__ uint64_t ug_l_size(uint64_t from, uint64_t to, uint32_t k) { return 10u + ut_digits(from) + ut_digits(to) + ut_digits(k - 1u); }
__device__ __forceinline__ uint8_t ug_l_byte(uint64_t from, uint64_t to, uint32_t orient, uint32_t k, uint64_t q) {
    const uint32_t df = ut_digits(from), dt = ut_digits(to), dk = ut_digits(k - 1u);
    if (q < 2u) return ug_at(ug_word("L\t"), q);
    q -= 2u;
    if (q < df) return ug_digit(from, df, q);
    q -= df;
    if (q < 3u) return q == 1u ? (uint8_t)((orient & 1u) ? '-' : '+') : (uint8_t)'\t';
    q -= 3u;
    if (q < dt) return ug_digit(to, dt, q);
    q -= dt;
    if (q < 3u) return q == 1u ? (uint8_t)((orient & 2u) ? '-' : '+') : (uint8_t)'\t';
    q -= 3u;
    if (q < dk) return ug_digit(k - 1u, dk, q);
    return q == dk ? (uint8_t)'M' : (uint8_t)'\n';
}

__global__ __launch_bounds__(UT) void k_ug_sizes_s(UgRows R, uint32_t k, unsigned long long *__restrict__ wgS) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t g = (uint64_t)blockIdx.x * UT + threadIdx.x;
    uint64_t n, depth;
    const uint8_t *seq;
    unsigned long long total;
    wg_excl_sum<UT / 64, false>((unsigned long long)(g < R.rows && ug_row(R, k, g, n, depth, seq) ? ug_s_size(g, n, depth, k) : 0ull), sh, total);
    if (threadIdx.x == 0) wgS[blockIdx.x] = total;
}
__global__ __launch_bounds__(UT) void k_ug_sizes_l(const unsigned long long *__restrict__ from, const unsigned long long *__restrict__ to, uint64_t n_edges,
                                                   uint32_t k, unsigned long long *__restrict__ wgL) {
    __shared__ unsigned long long sh[UT / 64];
    const uint64_t e = (uint64_t)blockIdx.x * UT + threadIdx.x;
    unsigned long long total;
    wg_excl_sum<UT / 64, false>((unsigned long long)(e < n_edges ? ug_l_size(from[e], to[e], k) : 0ull), sh, total);
    if (threadIdx.x == 0) wgL[blockIdx.x] = total;
}

// the line that holds byte q of a workgroup's lines: the last r with off[r] <= q (lines of no bytes lie on the next one)
__device__ __forceinline__ uint32_t ug_line(const unsigned long long *off, uint64_t q) {
    uint32_t lo = 0, hi = UT - 1;
    for (uint32_t step = 0; step < 8u && lo < hi; step++) {              // 2^8 = UT
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (off[mid] <= q) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// wgS scanned; the S-lines begin behind the header line
__global__ __launch_bounds__(UT) void k_ug_slines(UgRows R, uint32_t k, const unsigned long long *__restrict__ wgS, uint8_t *__restrict__ gfa,
                                                  uint64_t gfa_bytes, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long sh[UT / 64], off[UT], s_n[UT], s_depth[UT];
    __shared__ const uint8_t *s_seq[UT];
    const uint64_t g = (uint64_t)blockIdx.x * UT + threadIdx.x;
    uint64_t n = 0, depth = 0;
    const uint8_t *seq = nullptr;
    unsigned long long size = 0, total;
    if (g < R.rows) {
        if (ug_row(R, k, g, n, depth, seq)) size = ug_s_size(g, n, depth, k);
        else ut_raise(totals, 9);
    }
    off[threadIdx.x] = wg_excl_sum<UT / 64, false>(size, sh, total);
    s_n[threadIdx.x] = n; s_depth[threadIdx.x] = depth; s_seq[threadIdx.x] = seq;
    __syncthreads();
    const uint64_t base = (uint64_t)UG_HEADER + wgS[blockIdx.x];
    if (base > gfa_bytes || total > gfa_bytes - base) { if (threadIdx.x == 0) ut_raise(totals, 12); return; }      // uniform
    for (uint64_t q = threadIdx.x; q < total; q += UT) {
        const uint32_t r = ug_line(off, q);
        gfa[base + q] = ug_s_byte((uint64_t)blockIdx.x * UT + r, s_n[r], s_depth[r], s_seq[r], k, q - off[r]);
    }
}

// wgS and wgL scanned; the L-lines begin behind the last S-line
__global__ __launch_bounds__(UT) void k_ug_llines(const unsigned long long *__restrict__ from, const unsigned long long *__restrict__ to,
                                                  const uint8_t *__restrict__ orient, uint64_t n_edges, uint32_t k,
                                                  const unsigned long long *__restrict__ wgS, uint32_t n_wgS, const unsigned long long *__restrict__ wgL,
                                                  uint8_t *__restrict__ gfa, uint64_t gfa_bytes, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long sh[UT / 64], off[UT], s_from[UT], s_to[UT];
    __shared__ uint8_t s_orient[UT];
    const uint64_t e = (uint64_t)blockIdx.x * UT + threadIdx.x;
    const uint64_t f = e < n_edges ? from[e] : 0ull, t = e < n_edges ? to[e] : 0ull;
    unsigned long long total;
    off[threadIdx.x] = wg_excl_sum<UT / 64, false>((unsigned long long)(e < n_edges ? ug_l_size(f, t, k) : 0ull), sh, total);
    s_from[threadIdx.x] = f; s_to[threadIdx.x] = t; s_orient[threadIdx.x] = e < n_edges ? orient[e] : (uint8_t)0;
    __syncthreads();
    const uint64_t lines = (uint64_t)UG_HEADER + wgS[n_wgS];
    if (lines > gfa_bytes || wgL[blockIdx.x] > gfa_bytes - lines || total > gfa_bytes - lines - wgL[blockIdx.x]) {       // uniform
        if (threadIdx.x == 0) ut_raise(totals, 12);
        return;
    }
    const uint64_t base = lines + wgL[blockIdx.x];
    for (uint64_t q = threadIdx.x; q < total; q += UT) {
        const uint32_t r = ug_line(off, q);
        gfa[base + q] = ug_l_byte(s_from[r], s_to[r], s_orient[r], k, q - off[r]);
    }
}

static UtParams ut_params(int k, int min_count, int max_count) {
    UtParams p;
    p.k = (uint32_t)k; p.lo = (uint32_t)min_count; p.hi = (uint32_t)max_count;
    p.mask = (1ull << (2 * k)) - 1ull;
    return p;
}

uint32_t unitig_workgroups(uint64_t n) { return (uint32_t)((n + U_WG - 1) / U_WG); }
uint32_t unitig_rank_workgroups(uint64_t m) { return (uint32_t)((m + UT - 1) / UT); }

int launch_unitig_links(const uint8_t *table, uint64_t n, int k, int min_count, int max_count, uint8_t *link, unsigned long long *totals, hipStream_t s) {
    hipLaunchKernelGGL(k_ut_links, dim3(unitig_workgroups(n)), dim3(UT), 0, s, table, n, ut_params(k, min_count, max_count), link, totals);
    return hipGetLastError() != hipSuccess;
}

int launch_unitig_count(int mode, const uint8_t *link, uint64_t n, unsigned long long *wg, hipStream_t s) {
    const uint32_t n_wg = unitig_workgroups(n);
    if (mode == UT_ENDS) hipLaunchKernelGGL(k_ut_count<UT_ENDS>, dim3(n_wg), dim3(UT), 0, s, link, n, wg);
    else hipLaunchKernelGGL(k_ut_count<UT_LOOPS>, dim3(n_wg), dim3(UT), 0, s, link, n, wg);
    if (hipGetLastError() != hipSuccess) return 1;
    return launch_extract_scan(wg, n_wg, s);
}

int launch_unitig_measure(int mode, const uint8_t *table, uint8_t *link, uint64_t n, int k, int min_count, int max_count, const unsigned long long *wg,
                          unsigned long long *cand, uint64_t m, uint64_t bound, uint64_t min_kmers, unsigned long long *c_n, unsigned long long *c_depth,
                          uint8_t *c_keep, uint64_t row_base, unsigned long long *wgA, unsigned long long *wgB, unsigned long long *totals, hipStream_t s) {
    const uint32_t n_wg = unitig_workgroups(n), walk_wg = (uint32_t)((m + UW - 1) / UW), rank_wg = unitig_rank_workgroups(m);
    const UtParams p = ut_params(k, min_count, max_count);
    if (mode == UT_ENDS) {
        hipLaunchKernelGGL(k_ut_compact<UT_ENDS>, dim3(n_wg), dim3(UT), 0, s, (const uint8_t *)link, n, wg, n_wg, m, cand);
        hipLaunchKernelGGL(k_ut_measure<UT_ENDS>, dim3(walk_wg), dim3(UW), 0, s, table, link, p, (const unsigned long long *)cand, m, bound, min_kmers, c_n,
                           c_depth, c_keep, totals);
    } else {
        hipLaunchKernelGGL(k_ut_compact<UT_LOOPS>, dim3(n_wg), dim3(UT), 0, s, (const uint8_t *)link, n, wg, n_wg, m, cand);
        hipLaunchKernelGGL(k_ut_measure<UT_LOOPS>, dim3(walk_wg), dim3(UW), 0, s, table, link, p, (const unsigned long long *)cand, m, bound, min_kmers, c_n,
                           c_depth, c_keep, totals);
    }
    hipLaunchKernelGGL(k_ut_rank_rows, dim3(rank_wg), dim3(UT), 0, s, (const uint8_t *)c_keep, m, wgA);
    if (hipGetLastError() != hipSuccess || launch_extract_scan(wgA, rank_wg, s)) return 1;
    hipLaunchKernelGGL(k_ut_rank_bytes, dim3(rank_wg), dim3(UT), 0, s, (const uint8_t *)c_keep, (const unsigned long long *)c_n, m,
                       (const unsigned long long *)wgA, row_base, (uint32_t)k, wgB);
    if (hipGetLastError() != hipSuccess) return 1;
    return launch_extract_scan(wgB, rank_wg, s);
}

int launch_unitig_spell(const uint8_t *link, int k, const unsigned long long *cand, const uint8_t *c_keep, const unsigned long long *c_n,
                        const unsigned long long *c_depth, uint64_t m, const unsigned long long *wgA, const unsigned long long *wgB, uint64_t row_base,
                        uint64_t rows, unsigned long long *r_addr, unsigned long long *r_n, unsigned long long *r_depth, unsigned long long *r_off,
                        uint8_t *text, uint64_t text_bytes, unsigned long long *totals, hipStream_t s) {
    hipLaunchKernelGGL(k_ut_rows, dim3(unitig_rank_workgroups(m)), dim3(UT), 0, s, cand, c_keep, c_n, c_depth, m, wgA, wgB, row_base, (uint32_t)k, rows,
                       r_addr, r_n, r_depth, r_off, totals);
    hipLaunchKernelGGL(k_ut_spell, dim3((uint32_t)((rows + UW - 1) / UW)), dim3(UW), 0, s, link, ut_params(k, 1, 255), (const unsigned long long *)r_addr,
                       (const unsigned long long *)r_n, (const unsigned long long *)r_off, rows, row_base, text, text_bytes, totals);
    return hipGetLastError() != hipSuccess;
}

int launch_unitig_edges_count(const UgRows &R, int k, const uint8_t *link, const unsigned long long *r_addr, const unsigned long long *cand, uint64_t m,
                              unsigned long long *end_row, unsigned long long *wgE, unsigned long long *totals, hipStream_t s) {
    const uint32_t n_wg = unitig_rank_workgroups(2u * R.rows);
    if (R.rows0) hipLaunchKernelGGL(k_ug_ends, dim3(unitig_rank_workgroups(R.rows0)), dim3(UT), 0, s, R, (uint32_t)k, r_addr, cand, m, end_row, totals);
    hipLaunchKernelGGL(k_ug_count, dim3(n_wg), dim3(UT), 0, s, R, ut_params(k, 1, 255), link, cand, m, (const unsigned long long *)end_row, wgE, totals);
    if (hipGetLastError() != hipSuccess) return 1;
    return launch_extract_scan(wgE, n_wg, s);
}

int launch_unitig_edges_fill(const UgRows &R, int k, const uint8_t *link, const unsigned long long *cand, uint64_t m, const unsigned long long *end_row,
                             const unsigned long long *wgE, uint64_t n_edges, unsigned long long *from, unsigned long long *to, uint8_t *orient,
                             unsigned long long *totals, hipStream_t s) {
    hipLaunchKernelGGL(k_ug_fill, dim3(unitig_rank_workgroups(2u * R.rows)), dim3(UT), 0, s, R, ut_params(k, 1, 255), link, cand, m, end_row, wgE, n_edges,
                       from, to, orient, totals);
    return hipGetLastError() != hipSuccess;
}

int launch_unitig_gfa_sizes(const UgRows &R, int k, const unsigned long long *from, const unsigned long long *to, uint64_t n_edges,
                            unsigned long long *wgS, unsigned long long *wgL, hipStream_t s) {
    const uint32_t n_wgS = unitig_rank_workgroups(R.rows), n_wgL = unitig_rank_workgroups(n_edges);
    hipLaunchKernelGGL(k_ug_sizes_s, dim3(n_wgS), dim3(UT), 0, s, R, (uint32_t)k, wgS);
    if (hipGetLastError() != hipSuccess || launch_extract_scan(wgS, n_wgS, s)) return 1;
    if (n_edges) hipLaunchKernelGGL(k_ug_sizes_l, dim3(n_wgL), dim3(UT), 0, s, from, to, n_edges, (uint32_t)k, wgL);
    if (hipGetLastError() != hipSuccess) return 1;
    return launch_extract_scan(wgL, n_wgL, s);
}

int launch_unitig_gfa_write(const UgRows &R, int k, const unsigned long long *from, const unsigned long long *to, const uint8_t *orient, uint64_t n_edges,
                            const unsigned long long *wgS, const unsigned long long *wgL, uint8_t *gfa, uint64_t gfa_bytes, unsigned long long *totals,
                            hipStream_t s) {
    const uint32_t n_wgS = unitig_rank_workgroups(R.rows);
    hipLaunchKernelGGL(k_ug_slines, dim3(n_wgS), dim3(UT), 0, s, R, (uint32_t)k, wgS, gfa, gfa_bytes, totals);
    if (n_edges)
        hipLaunchKernelGGL(k_ug_llines, dim3(unitig_rank_workgroups(n_edges)), dim3(UT), 0, s, from, to, orient, n_edges, (uint32_t)k, wgS, n_wgS, wgL, gfa,
                           gfa_bytes, totals);
    return hipGetLastError() != hipSuccess;
}

}  // namespace pk
