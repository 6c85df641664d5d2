// kmer_extract.hip -- the k-mers behind a condition over N tables: which addresses x of a staged slice have
//   p(x) = #{ present tables i : min <= T_i[x] <= max } >= min_present   and   q(x) = #{ absent tables j : T_j[x] >= 1 } <= max_absent,
// handed back as the ascending list of those addresses and, per address, the raw bytes T_i[x] of the P present tables.
// No reference counterpart (its README stops at the distance matrix).
//
// A three-launch stream compaction; no workgroup ever waits for another:
//   k_extract_count  streams every table once (the pair scan's traffic): a thread takes 16 consecutive addresses of every
//                    table, counts p and q per address in byte lanes of 4 + 4 dwords, reduces them to a 16-bit selection
//                    mask, keeps the mask (1 bit per address) and adds its population to the workgroup's count
//   k_extract_scan   one workgroup: the exclusive prefix of the workgroup counts, and the total
//   k_extract_write  returns at once when the total exceeds the capacity.  Otherwise it reads the masks back, ranks the
//                    selected addresses of a 4096-address tile in LDS, writes addr_out[rank] (one u64 per lane, consecutive
//                    ranks) and then the tile's count rows as one contiguous byte range of counts_out: a thread produces one
//                    aligned dword of it, gathering its four bytes T_i[x] from the tables, so the rows leave as dword
//                    stores whatever P is (the range's unaligned ends, at most 3 bytes each, are byte stores)
//   k_extract_text   m addresses -> m lines of k letters + '\n', 16 output bytes per thread
// And the same selection as a dense table, one byte per address (a `.kin` made from `.kin`s):
//   k_extract_table  a streaming map with k_extract_count's geometry: beside p and q a thread reduces the present bytes that
//                    lie in the window (sum, min, max; the count is p itself) in 16-bit lanes, blanks the addresses that
//                    are not selected and stores its 16 result bytes at once
#include "pk_kernels.h"
#include "gram_load.h"
#include "wg_scan.h"

namespace pk {

constexpr int XT = 256;                          // threads per workgroup
constexpr uint32_t X_ADDR = 16;                  // addresses per thread and step: one 16-byte load per table, in address order
constexpr uint32_t X_TILE = XT * X_ADDR;         // addresses per step of a workgroup
constexpr uint32_t X_STEPS = 4;                  // steps per workgroup
constexpr uint64_t X_WG = (uint64_t)X_TILE * X_STEPS;   // addresses per workgroup
constexpr int XS = 1024;                         // threads of the scan

struct ExtractParams {
    uint32_t lo_rep, lo_hi;      // min_count: its low 7 bits in every byte, and whether it is >= 128
    uint32_t up_rep, up_hi;      // the same for max_count + 1 (used when has_up)
    uint32_t has_up;             // max_count < 255
    uint32_t min_present, max_absent;
};

// bit 7 of every byte of x whose value is >= c, 1 <= c <= 255 given as (c & 0x7f) in every byte and c >= 128.  The
// subtraction never borrows across bytes: (low 7 bits | 0x80) - (at most 0x7f) >= 1 in every byte.
__device__ __forceinline__ uint32_t x_ge(uint32_t x, uint32_t c_rep, uint32_t c_hi) {
    const uint32_t gl = (((x & L4) | H4) - c_rep) & H4;          // low 7 bits of x >= low 7 bits of c
    return (c_hi ? (x & gl) : (x | gl)) & H4;
}
// 1 in every byte of x that lies in the count window (the validity test of the pair tally, tools.py:473-475)
__device__ __forceinline__ uint32_t x_valid(uint32_t x, const ExtractParams &p) {
    uint32_t v = x_ge(x, p.lo_rep, p.lo_hi);
    if (p.has_up) v &= ~x_ge(x, p.up_rep, p.up_hi);
    return v >> 7;
}
// 1 in every byte of x that is not zero
__device__ __forceinline__ uint32_t x_held(uint32_t x) { return ((((x & L4) + L4) | x) & H4) >> 7; }

// The threshold test on the byte counters p and q of 16 addresses: bit j for address j.  With up to 128 tables a counter
// reaches 0x80, so the thresholds are compared on the extracted byte, not on a byte's high bit.
__device__ __forceinline__ uint32_t x_select16(const uint32_t (&p)[4], const uint32_t (&q)[4], const ExtractParams &ep) {
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t j = 0; j < X_ADDR; j++) {
        const uint32_t pj = (p[j >> 2] >> (8u * (j & 3u))) & 0xffu, qj = (q[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        mask |= (uint32_t)(pj >= ep.min_present && qj <= ep.max_absent) << j;
    }
    return mask;
}
// q of addresses [off, off + 16) over the absent tables, added to the byte counters
__device__ __forceinline__ void x_count_absent(const uint8_t *const *__restrict__ tables, uint32_t P, uint32_t A, uint64_t off, uint64_t n,
                                               uint32_t (&q)[4]) {
#pragma unroll 4
    for (uint32_t t = P; t < P + A; t++) {
        const uint4 x = load_half(tables[t], off, n);
        q[0] += x_held(x.x); q[1] += x_held(x.y); q[2] += x_held(x.z); q[3] += x_held(x.w);
    }
}

// The selection mask of addresses [off, off + 16): bit j for address off + j.  p and q are byte counters.  Bytes at or
// beyond n read as 0: p = 0 < min_present, never selected.
__device__ __forceinline__ uint32_t x_mask16(const uint8_t *const *__restrict__ tables, uint32_t P, uint32_t A, uint64_t off, uint64_t n,
                                             const ExtractParams &ep) {
    uint32_t p[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t t = 0; t < P; t++) {
        const uint4 x = load_half(tables[t], off, n);
        p[0] += x_valid(x.x, ep); p[1] += x_valid(x.y, ep); p[2] += x_valid(x.z, ep); p[3] += x_valid(x.w, ep);
    }
    x_count_absent(tables, P, A, off, n, q);
    return x_select16(p, q, ep);
}

// masks (nullable: the caller wants the count alone): one u16 per 16 addresses; wg_count[b] = selected addresses of workgroup b
__global__ __launch_bounds__(XT) void k_extract_count(const uint8_t *const *__restrict__ tables, uint32_t P, uint32_t A, uint64_t n, ExtractParams ep,
                                                      uint16_t *__restrict__ masks, unsigned long long *__restrict__ wg_count) {
    __shared__ uint32_t wsum[XT / 64];
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < X_STEPS; s++) {
        const uint64_t off = (uint64_t)blockIdx.x * X_WG + (uint64_t)s * X_TILE + (uint64_t)threadIdx.x * X_ADDR;
        if (off >= n) break;
        const uint32_t mask = x_mask16(tables, P, A, off, n, ep);
        if (masks) masks[off / X_ADDR] = (uint16_t)mask;
        cnt += __popc(mask);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < XT / 64; w++) tot += wsum[w];
        wg_count[blockIdx.x] = tot;
    }
}

// wg[0 .. n_wg): counts -> exclusive prefix sums, in place; wg[n_wg] = the total
__global__ __launch_bounds__(XS) void k_extract_scan(unsigned long long *__restrict__ wg, uint32_t n_wg) {
    __shared__ unsigned long long wsum[XS / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long run = 0;
    for (uint32_t b0 = 0; b0 < n_wg; b0 += XS) {
        const uint32_t b = b0 + threadIdx.x;
        const unsigned long long v = b < n_wg ? wg[b] : 0ull;
        unsigned long long inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
        __syncthreads();
        if (lane == 63u) wsum[w] = inc;
        __syncthreads();
        unsigned long long pre = 0, total = 0;
        for (uint32_t i = 0; i < XS / 64; i++) { if (i < w) pre += wsum[i]; total += wsum[i]; }
        if (b < n_wg) wg[b] = run + pre + inc - v;
        run += total;
    }
    if (threadIdx.x == 0) wg[n_wg] = run;
}

__global__ __launch_bounds__(XT) void k_extract_write(const uint8_t *const *__restrict__ tables, uint32_t P, uint64_t n, uint64_t first_addr,
                                                      const uint16_t *__restrict__ masks, const unsigned long long *__restrict__ wg, uint32_t n_wg,
                                                      uint64_t cap, unsigned long long *__restrict__ addr_out, uint8_t *__restrict__ counts_out) {
    __shared__ const uint8_t *tp[128];
    __shared__ uint16_t sel[X_TILE];             // the tile's selected addresses, relative to the tile, ascending
    __shared__ uint32_t wsum[XT / 64];
    if (wg[n_wg] > cap) return;                  // too many for the caller's arrays: nothing is written
    unsigned long long rank = wg[blockIdx.x];    // of the workgroup's first selected address
    if (wg[blockIdx.x + 1u] == rank) return; // nothing selected here (wg[n_wg] is the total, so the last workgroup reads it)
    if (threadIdx.x < P) tp[threadIdx.x] = tables[threadIdx.x];
    for (uint32_t s = 0; s < X_STEPS; s++) {
        const uint64_t tile = (uint64_t)blockIdx.x * X_WG + (uint64_t)s * X_TILE;
        if (tile >= n) break;
        const uint64_t off = tile + (uint64_t)threadIdx.x * X_ADDR;
        uint32_t mask = off < n ? masks[off / X_ADDR] : 0u;
        uint32_t S;                              // the barrier in front: the previous step's readers of sel and wsum are done (and tp is written)
        uint32_t r = wg_excl_sum<XT / 64, true>((uint32_t)__popc(mask), wsum, S);
        if (S == 0u) continue;                   // uniform
        while (mask) {
            const uint32_t j = __ffs(mask) - 1u;
            mask &= mask - 1u;
            sel[r++] = (uint16_t)(threadIdx.x * X_ADDR + j);
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < S; i += XT) addr_out[rank + i] = first_addr + tile + sel[i];
        // the tile's rows are bytes [g0, g1) of counts_out; a thread builds the aligned dword at gd
        const uint64_t g0 = rank * P, g1 = g0 + (uint64_t)S * P;
        for (uint64_t gd = (g0 & ~3ull) + 4ull * threadIdx.x; gd < g1; gd += 4ull * XT) {
            const uint64_t gf = gd < g0 ? g0 : gd;             // the first byte of the dword that belongs to the tile
            const uint32_t jf = (uint32_t)(gf - g0);
            uint32_t row = jf / P, col = jf - row * P, word = 0, have = 0;
            for (uint64_t g = gf; g < gd + 4u && g < g1; g++) {
                const uint32_t v = tp[col][tile + sel[row]];
                word |= v << (8u * (uint32_t)(g - gd));
                have++;
                if (++col == P) { col = 0; row++; }
            }
            if (have == 4u) *(uint32_t *)(counts_out + gd) = word;
            else for (uint64_t g = gf; g < gf + have; g++) counts_out[g] = (uint8_t)(word >> (8u * (uint32_t)(g - gd)));
        }
        rank += S;
    }
}

// ---- the selection as a table ----
// Two 16-bit lanes per dword: the even bytes of a table dword in one accumulator, the odd bytes in another.  A sum over 128
// tables reaches 128 * 255 = 32 640 < 2^16, so a lane never carries into its neighbour; min and max are the packed u16
// instructions on the same lanes, and so is the clamp of the sum to 255.
constexpr uint32_t LANES = 0x00ff00ffu;
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// one table dword x, v = x_valid(x), into the accumulators of its even and odd bytes.  Bytes outside the window take no
// part: they enter as the operation's identity, 0 for sum and max, 255 for min.
template <int OP> __device__ __forceinline__ void x_reduce(uint32_t x, uint32_t v, uint32_t &even, uint32_t &odd) {
    const uint32_t in = v * 0xffu;               // 0xff in every byte inside the window (v holds 0 or 1 per byte: no carries)
    if (OP == TABLE_SUM) { x &= in; even += x & LANES; odd += (x >> 8) & LANES; }
    if (OP == TABLE_MIN) { x |= ~in; even = pk_min_u16(even, x & LANES); odd = pk_min_u16(odd, (x >> 8) & LANES); }
    if (OP == TABLE_MAX) { x &= in; even = pk_max_u16(even, x & LANES); odd = pk_max_u16(odd, (x >> 8) & LANES); }
}

// out[off .. off + 16) for off < n, cut at n.  Bytes at or beyond n read as 0 and are not stored.
template <int OP> __global__ __launch_bounds__(XT) void k_extract_table(const uint8_t *const *__restrict__ tables, uint32_t P, uint32_t A, uint64_t n,
                                                                        ExtractParams ep, uint8_t *__restrict__ out) {
    constexpr uint32_t ID = OP == TABLE_MIN ? LANES : 0u;
    for (uint32_t s = 0; s < X_STEPS; s++) {
        const uint64_t off = (uint64_t)blockIdx.x * X_WG + (uint64_t)s * X_TILE + (uint64_t)threadIdx.x * X_ADDR;
        if (off >= n) break;
        uint32_t p[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        uint32_t even[4] = {ID, ID, ID, ID}, odd[4] = {ID, ID, ID, ID};
#pragma unroll 4
        for (uint32_t t = 0; t < P; t++) {
            const uint4 x = load_half(tables[t], off, n);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const uint32_t v = x_valid(xs[d], ep);
                p[d] += v;
                x_reduce<OP>(xs[d], v, even[d], odd[d]);
            }
        }
        x_count_absent(tables, P, A, off, n, q);
        const uint32_t mask = x_select16(p, q, ep);
        uint32_t r[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t m4 = (mask >> (4 * d)) & 0xfu;                                        // the dword's four selection bits ...
            const uint32_t sel = ((m4 & 1u) | ((m4 & 2u) << 7) | ((m4 & 4u) << 14) | ((m4 & 8u) << 21)) * 0xffu;   // ... as 0xff bytes
            if (OP == TABLE_COUNT) r[d] = p[d] & sel;                                             // p <= 128 fits its byte
            else if (OP == TABLE_SUM) r[d] = (pk_min_u16(even[d], LANES) | (pk_min_u16(odd[d], LANES) << 8)) & sel;
            else r[d] = (even[d] | (odd[d] << 8)) & sel;   // a selected address has a byte in the window: no identity is left
        }
        if (off + X_ADDR <= n) *(uint4 *)(out + off) = make_uint4(r[0], r[1], r[2], r[3]);
        else for (uint64_t i = off; i < n; i++) out[i] = (uint8_t)(r[(i - off) >> 2] >> (8u * ((i - off) & 3u)));
    }
}

// text bytes [0, m * (k + 1)): line r holds the k letters of addr[r], first base in the highest bits, then '\n'
__global__ __launch_bounds__(XT) void k_extract_text(const unsigned long long *__restrict__ addr, uint64_t m, uint32_t k, uint8_t *__restrict__ text) {
    const uint64_t total = m * (k + 1u);
    const uint64_t g0 = ((uint64_t)blockIdx.x * XT + threadIdx.x) * 16u;
    if (g0 >= total) return;
    uint64_t row = g0 / (k + 1u);
    uint32_t col = (uint32_t)(g0 - row * (k + 1u));
    unsigned long long a = addr[row];
    uint32_t word[4] = {0, 0, 0, 0};
    const uint32_t have = total - g0 < 16u ? (uint32_t)(total - g0) : 16u;
    for (uint32_t b = 0; b < have; b++) {
        const uint32_t ch = col == k ? (uint32_t)'\n' : (0x54474341u >> (8u * (uint32_t)((a >> (2u * (k - 1u - col))) & 3ull))) & 0xffu;   // "ACGT"
        word[b >> 2] |= ch << (8u * (b & 3u));
        if (++col > k) { col = 0; if (++row < m) a = addr[row]; }
    }
    if (have == 16u) *(uint4 *)(text + g0) = make_uint4(word[0], word[1], word[2], word[3]);
    else for (uint32_t b = 0; b < have; b++) text[g0 + b] = (uint8_t)(word[b >> 2] >> (8u * (b & 3u)));
}

uint32_t extract_workgroups(uint64_t n_slice) { return (uint32_t)((n_slice + X_WG - 1) / X_WG); }
uint64_t extract_mask_words(uint64_t n_slice) { return (n_slice + X_ADDR - 1) / X_ADDR; }

int launch_extract_scan(unsigned long long *wg, uint32_t n_wg, hipStream_t s) {
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(XS), 0, s, wg, n_wg);
    return hipGetLastError() != hipSuccess;
}

static ExtractParams extract_params(int min_count, int max_count, int min_present, int max_absent) {
    ExtractParams ep;
    ep.lo_rep = (uint32_t)(min_count & 0x7f) * 0x01010101u;
    ep.lo_hi = min_count >= 128;
    ep.up_rep = (uint32_t)((max_count + 1) & 0x7f) * 0x01010101u;
    ep.up_hi = max_count + 1 >= 128;
    ep.has_up = max_count < 255;
    ep.min_present = (uint32_t)min_present;
    ep.max_absent = (uint32_t)max_absent;
    return ep;
}

int launch_extract(const uint8_t *const *dev_tables, int P, int A, uint64_t n_slice, uint64_t first_addr, int min_count, int max_count, int min_present,
                   int max_absent, uint16_t *masks, unsigned long long *wg, unsigned long long *addr_out, uint8_t *counts_out, uint64_t cap,
                   hipStream_t s) {
    const ExtractParams ep = extract_params(min_count, max_count, min_present, max_absent);
    const uint32_t n_wg = extract_workgroups(n_slice);
    const bool write = cap > 0;
    hipLaunchKernelGGL(k_extract_count, dim3(n_wg), dim3(XT), 0, s, dev_tables, (uint32_t)P, (uint32_t)A, n_slice, ep, write ? masks : nullptr, wg);
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(XS), 0, s, wg, n_wg);
    if (write)
        hipLaunchKernelGGL(k_extract_write, dim3(n_wg), dim3(XT), 0, s, dev_tables, (uint32_t)P, n_slice, first_addr, (const uint16_t *)masks,
                           (const unsigned long long *)wg, n_wg, cap, addr_out, counts_out);
    return hipGetLastError() != hipSuccess;
}

template <int OP> static void launch_table_op(const uint8_t *const *dev_tables, int P, int A, uint64_t n_slice, const ExtractParams &ep, uint8_t *out,
                                              hipStream_t s) {
    hipLaunchKernelGGL(k_extract_table<OP>, dim3(extract_workgroups(n_slice)), dim3(XT), 0, s, dev_tables, (uint32_t)P, (uint32_t)A, n_slice, ep, out);
}

int launch_extract_table(const uint8_t *const *dev_tables, int P, int A, uint64_t n_slice, int min_count, int max_count, int min_present,
                         int max_absent, int op, uint8_t *table_out, hipStream_t s) {
    const ExtractParams ep = extract_params(min_count, max_count, min_present, max_absent);
    switch (op) {
    case TABLE_SUM: launch_table_op<TABLE_SUM>(dev_tables, P, A, n_slice, ep, table_out, s); break;
    case TABLE_MIN: launch_table_op<TABLE_MIN>(dev_tables, P, A, n_slice, ep, table_out, s); break;
    case TABLE_MAX: launch_table_op<TABLE_MAX>(dev_tables, P, A, n_slice, ep, table_out, s); break;
    case TABLE_COUNT: launch_table_op<TABLE_COUNT>(dev_tables, P, A, n_slice, ep, table_out, s); break;
    default: return 1;
    }
    return hipGetLastError() != hipSuccess;
}

int launch_extract_text(const unsigned long long *addr, uint64_t m, int k, uint8_t *text, hipStream_t s) {
    const uint64_t threads = (m * (uint64_t)(k + 1) + 15u) / 16u;
    hipLaunchKernelGGL(k_extract_text, dim3((uint32_t)((threads + XT - 1) / XT)), dim3(XT), 0, s, addr, m, (uint32_t)k, text);
    return hipGetLastError() != hipSuccess;
}

}  // namespace pk
