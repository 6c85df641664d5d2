// gram_patterns.hip -- presence patterns of N <= 16 dense tables: how many addresses each subset of the tables holds.
//
// For every address x the N-bit word m(x) = sum_t [min <= T_t[x] <= max] << t says which tables hold x in the count window;
// k_patterns ADDS the histogram of m over a slice to a flat accumulator of 2^N u64 in HBM.  Every pair tally, occupancy
// class, intersection, union and difference of any subset of the tables is a sum over that histogram (pykmer_amd/patterns.py).
//
// Layout of the work.  A lane takes one 32-address word of every table (gram_load.h: a wave covers a 2 KiB block with two
// contiguous 1 KiB loads per table).  Per dword of 4 addresses and table t the window test leaves bit 7 of every valid byte
// (the H4 / L4 form of gram_scan.hip); shifted right by 7 - t it is ORed into a `lo` dword for t < 8 and by 15 - t into a
// `hi` dword for t >= 8, so the pattern of address b of the dword is byte b of lo | byte b of hi << 8.  The tables are loaded
// eight at a time -- the eight of `lo`, then the eight of `hi` -- which keeps 16 sixteen-byte loads per lane in flight.
//
// Tallies.  The workgroup keeps 2^min(N, 14) u32 bins in LDS (64 KiB at most: two workgroups per CU) and every address with
// a non-zero pattern is one LDS atomic add (after one round of a wave-level pre-sum of the first lane's pattern: see the
// kernel; measured in DESIGN.md 4.15).  Pattern 0 -- the bulk of sparse tables -- is never added: the first launch adds
// n to accum[0] once and every workgroup subtracts what it tallied (u64 wrap-around, exact at the end), the way k_occgram
// treats class 0.  The non-zero bins go to HBM with one atomicAdd each, once per workgroup.  For N = 15 and 16 the pass is
// 2^(N - 14) launches over the slice; launch `top` keeps the patterns whose bits 14.. equal `top` and bins their low 14 bits.
//
// No bin wraps: an address adds at most 1 to one bin, a workgroup takes PT_THREADS * 32 = 8192 addresses per iteration, and
// the launcher sizes the grid so that no workgroup runs more than PT_MAX_ITERS = 2^19 - 1 iterations: < 2^32 adds per
// workgroup in all, so even one bin that took every one of them holds.
#include "pk_kernels.h"
#include "gram_load.h"
#include <algorithm>

namespace pk {

constexpr int PT_THREADS = 256;                     // 4 waves
constexpr int PT_MAXT = 16;
constexpr int PT_BIN_BITS = 14;                     // 2^14 u32 bins = 64 KiB of LDS
constexpr uint64_t PT_MAX_ITERS = (1u << 19) - 1;   // iterations of one workgroup: (2^19 - 1) * 8192 < 2^32 adds
static_assert(PT_MAX_ITERS * PT_THREADS * 32 < (1ull << 32), "a u32 bin could wrap");

struct PatTables { const uint8_t *t[PT_MAXT]; };
struct PatWindow {     // the window test's constants (gram_scan.hip: ValidParams)
    uint32_t lo_rep;   // (min & 0x7f) replicated to 4 bytes
    uint32_t lo_hi;    // min >= 128
    uint32_t up_rep;   // ((max + 1) & 0x7f) replicated
    uint32_t up_hi;    // max + 1 >= 128
    uint32_t has_up;   // max < 255
};

// bit 7 of each byte set iff min <= byte <= max
template <bool FAST>
__device__ __forceinline__ uint32_t pt_valid(uint32_t x, const PatWindow &p) {
    if (FAST) return (((x & L4) + L4) | x) & H4;               // min = 1, max = 255: byte != 0
    const uint32_t xl = x & L4, xh = x & H4;
    const uint32_t gl = ((xl | H4) - p.lo_rep) & H4;            // low 7 bits >= low 7 bits of min
    uint32_t ge = p.lo_hi ? (xh & gl) : (xh | gl);
    if (p.has_up) {
        const uint32_t ul = ((xl | H4) - p.up_rep) & H4;
        const uint32_t gu = p.up_hi ? (xh & ul) : (xh | ul);    // byte >= max + 1
        ge &= ~gu;
    }
    return ge;
}

// ORs the validity of tables T0 .. T0 + 7 (those below N) at the lane's word into bits 0..7 of every byte of m[0..8)
template <bool FAST, int T0>
__device__ __forceinline__ void pt_eight(const PatTables &T, int N, uint64_t word, uint64_t n, const PatWindow &w, uint32_t (&m)[8]) {
    uint4 a[8], b[8];
#pragma unroll
    for (int x = 0; x < 8; x++)
        if (T0 + x < N) load_word(T.t[T0 + x], word, n, a[x], b[x]);   // uniform
#pragma unroll
    for (int x = 0; x < 8; x++) {
        if (T0 + x >= N) continue;
        m[0] |= pt_valid<FAST>(a[x].x, w) >> (7 - x);
        m[1] |= pt_valid<FAST>(a[x].y, w) >> (7 - x);
        m[2] |= pt_valid<FAST>(a[x].z, w) >> (7 - x);
        m[3] |= pt_valid<FAST>(a[x].w, w) >> (7 - x);
        m[4] |= pt_valid<FAST>(b[x].x, w) >> (7 - x);
        m[5] |= pt_valid<FAST>(b[x].y, w) >> (7 - x);
        m[6] |= pt_valid<FAST>(b[x].z, w) >> (7 - x);
        m[7] |= pt_valid<FAST>(b[x].w, w) >> (7 - x);
    }
}

template <bool FAST>
__global__ __launch_bounds__(PT_THREADS) void k_patterns(const PatTables T, int N, uint64_t n, const PatWindow w, uint32_t top, int bin_bits,
                                                        unsigned long long *__restrict__ accum) {
    extern __shared__ uint32_t pt_bins[];               // 1 << bin_bits
    const uint32_t n_bins = 1u << bin_bits, bin_mask = n_bins - 1u;
    for (uint32_t i = threadIdx.x; i < n_bins; i += PT_THREADS) pt_bins[i] = 0;
    __syncthreads();
    if (top == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&accum[0], (unsigned long long)n);

    const int lane = threadIdx.x & 63;
    const uint64_t n_words = n_words_for(n);
    for (uint64_t w0 = (uint64_t)blockIdx.x * PT_THREADS; w0 < n_words; w0 += (uint64_t)gridDim.x * PT_THREADS) {
        const uint64_t word = w0 + threadIdx.x;
        if (word >= n_words) continue;
        uint32_t lo[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int nt = N;                                             // opaque per iteration: otherwise its 16 tests are hoisted
        asm volatile("" : "+s"(nt));                            // out of the loop as scalar masks, which spill
        pt_eight<FAST, 0>(T, nt, word, n, w, lo);
        if (nt > 8) pt_eight<FAST, 8>(T, nt, word, n, w, hi);
        // Tallies, in wave-uniform control flow.  Genome families share a core, so one pattern takes a large share of the
        // held addresses and 64 lanes adding to one LDS word serialise: the lanes whose pattern equals the first active
        // lane's are counted by ballot and that lane adds their number (one round); the others add on their own.
#pragma unroll
        for (int d = 0; d < 8; d++) {
            if (__ballot((lo[d] | hi[d]) != 0u) == 0ull) continue;   // four addresses per lane that no table holds
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t p = ((lo[d] >> (8 * b)) & 0xffu) | (((hi[d] >> (8 * b)) & 0xffu) << 8);
                const bool act = p != 0u && (p >> bin_bits) == top;
                const unsigned long long any = __ballot(act);
                if (any == 0ull) continue;
                const int first = __ffsll((long long)any) - 1;
                const uint32_t pf = (uint32_t)__shfl((int)p, first, 64);
                const unsigned long long same = __ballot(act && p == pf);
                if (lane == first) atomicAdd(&pt_bins[pf & bin_mask], (uint32_t)__popcll(same));
                if (act && p != pf) atomicAdd(&pt_bins[p & bin_mask], 1u);
            }
        }
    }
    __syncthreads();
    // workgroup bins -> HBM, and their sum off accum[0]
    unsigned long long mine = 0;
    unsigned long long *out = accum + ((size_t)top << bin_bits);
    for (uint32_t i = threadIdx.x; i < n_bins; i += PT_THREADS) {
        const uint32_t v = pt_bins[i];
        if (!v) continue;
        atomicAdd(&out[i], (unsigned long long)v);
        mine += v;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += (unsigned long long)__shfl_xor((long long)mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&accum[0], 0ull - mine);
}

// dev_tables: HOST array of N device pointers.  One launch for N <= 14, 2^(N - 14) beyond.
int launch_patterns(const void *const *dev_tables, int N, uint64_t n_slice, int min_count, int max_count, unsigned long long *dev_accum,
                    hipStream_t s) {
    if (N < 1 || N > PT_MAXT || min_count < 1 || max_count > 255 || min_count > max_count) return -1;
    if (n_slice == 0) return 0;
    PatTables T;
    for (int t = 0; t < PT_MAXT; t++) T.t[t] = (const uint8_t *)dev_tables[t < N ? t : 0];
    PatWindow w;
    w.lo_rep = (uint32_t)(min_count & 0x7f) * 0x01010101u;
    w.lo_hi = min_count >= 128;
    w.has_up = max_count < 255;
    w.up_rep = (uint32_t)((max_count + 1) & 0x7f) * 0x01010101u;
    w.up_hi = (max_count + 1) >= 128;
    const bool fast = min_count == 1 && max_count == 255;
    int dev = 0, n_cu = 256;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    const int bin_bits = std::min(N, PT_BIN_BITS);
    const size_t lds = sizeof(uint32_t) << bin_bits;
    const uint64_t n_words = ((n_slice + 2047u) / 2048u) * 64u;          // n_words_for(n_slice)
    const uint64_t n_iters = (n_words + PT_THREADS - 1) / PT_THREADS;
    uint64_t grid = std::min<uint64_t>(n_iters, (uint64_t)n_cu * 2);     // two workgroups per CU
    grid = std::max<uint64_t>(grid, (n_iters + PT_MAX_ITERS - 1) / PT_MAX_ITERS);
    for (uint32_t top = 0; top < (1u << (N - bin_bits)); top++) {
        if (fast) hipLaunchKernelGGL(k_patterns<true>, dim3((uint32_t)grid), dim3(PT_THREADS), lds, s, T, N, n_slice, w, top, bin_bits, dev_accum);
        else hipLaunchKernelGGL(k_patterns<false>, dim3((uint32_t)grid), dim3(PT_THREADS), lds, s, T, N, n_slice, w, top, bin_bits, dev_accum);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

}  // namespace pk
