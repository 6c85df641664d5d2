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

}  // namespace pk
