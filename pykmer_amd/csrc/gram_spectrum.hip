// gram_spectrum.hip -- joint count spectra of N dense tables in one streaming pass.
//
// Every validity window of the reference's pair tally (Header.calculate_distance, tools.py:473-482) is a box sum over the
// pair's joint count spectrum J_ij[a][b] = #{x : c_i(x) = a, c_j(x) = b}:  shared_ij(lo, hi) = sum_{a,b in [lo,hi]} J_ij[a][b],
// total_i(lo, hi) = sum_{a in [lo,hi]} hist_i[a].  k_spectrum ADDS to a u64 accumulator in HBM
//   hist[N][256]            per table, the addresses holding each count 0..255
//   core[P][255][255]       P = N(N-1)/2 pairs i < j, row-major upper triangle: addresses with c_i = a >= 1 and c_j = b >= 1
// (row / column 0 of J follow from the marginals on the host), so that ONE pass over the tables answers every
// --min-count / --max-count question the reference answers with one whole merge each (README.md:57-61).
//
// Layout of the work: a lane holds 16 consecutive bytes of every table of its pair group (up to 16 tables: all of them for
// N <= 16, otherwise two blocks of 8, or one block of 8 with itself) and turns each table's 16 bytes into one register of
// flags: bit 8k + d = "byte k of dword d is non-zero", bit 8k + 4 + d = "... is 1" (SWAR, the non-zero test of
// valid_bits<true>).  Per pair, AND-ing two flag registers gives
//   (1,1) events  -> a per-lane register tally (16-bit halves; the launcher bounds a lane's chunks so they cannot carry),
//                    the hot bin of genome tables, never touching memory until the end;
//   other events  -> a lane walks its own (usually none): counts a, b <= L go to a u32 tally of the pair's low-count
//                    corner [1, L]^2 in LDS, the rest to the HBM accumulator with wave-aggregated u64 atomics (the lanes that
//                    share the leader's bin add once, the others add their own);
// and per table the non-zero / ones counts (registers) and counts >= 2 (LDS histogram) give hist.  Zeros are counted as
// n - non-zero: the first workgroup adds n, every wave subtracts its non-zero count (u64 wrap-around, exact at the end).
// LDS and register tallies are bounded by the bytes one workgroup covers (< 2^26), so no u32 counter can wrap.
#include "pk_kernels.h"
#include "gram_load.h"
#include <algorithm>
#include <vector>

namespace pk {

constexpr int SPEC_MAXT = 16;                       // tables of one pair group
constexpr int SPEC_SLOTS = SPEC_MAXT * (SPEC_MAXT - 1) / 2;
constexpr int SPEC_THREADS = 512;
constexpr uint32_t SPEC_MAX_CHUNKS = 4095;          // 16-byte chunks per lane: 16-bit tallies of <= 16 per chunk stay < 2^16
constexpr size_t SPEC_LDS = 160 * 1024 - 1024;      // dynamic LDS of a workgroup (one per CU); the rest is static
constexpr uint32_t LO4 = 0x0f0f0f0fu;

struct SpecGroup {
    int nt;                   // tables in the group
    int split;                // 0: every pair x < y of the group; else the pairs x < split <= y (two blocks)
    int hist;                 // 1: this group also takes the value histograms of its tables
    int L;                    // edge of the low-count corner kept in LDS: counts 1..L
    int npairs;               // pairs of the group (LDS corners)
    uint32_t slots[4];        // bit s: slot s (x < y, row-major over SPEC_MAXT) is a pair of the group
    int16_t t[SPEC_MAXT];     // table index of group slot x (ascending)
};

__device__ __forceinline__ uint32_t nz_bits(uint32_t v) { return (((v & L4) + L4) | v) & H4; }
__device__ __forceinline__ uint32_t one_bits(uint32_t v) {
    const uint32_t y = v ^ 0x01010101u;
    return ~(((y & L4) + L4) | y) & H4;
}
// byte k of dword d -> bit 8k + d (non-zero), bit 8k + 4 + d (equal to 1)
__device__ __forceinline__ uint32_t flags16(const uint4 &v) {
    return (nz_bits(v.x) >> 7) | (nz_bits(v.y) >> 6) | (nz_bits(v.z) >> 5) | (nz_bits(v.w) >> 4) |
           (one_bits(v.x) >> 3) | (one_bits(v.y) >> 2) | (one_bits(v.z) >> 1) | one_bits(v.w);
}
// the count behind flag bit p (p & 4 == 0)
__device__ __forceinline__ uint32_t byte_at(const uint4 &v, uint32_t p) {
    // masks, not an indexed pick: written as v[p & 3], the compiler moves the lane's loaded bytes to scratch to index them
    const uint32_t m1 = 0u - (p & 1u), m2 = 0u - ((p >> 1) & 1u);
    const uint32_t lo = (v.x & ~m1) | (v.y & m1), hi = (v.z & ~m1) | (v.w & m1);
    return __builtin_amdgcn_ubfe((lo & ~m2) | (hi & m2), p & 24u, 8u);
}
__device__ __forceinline__ uint32_t spec_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(SPEC_THREADS) void k_spectrum(const uint8_t *const *__restrict__ gtab, int N, uint64_t n, SpecGroup g,
                                                           unsigned long long *__restrict__ accum) {
    extern __shared__ uint32_t lds[];               // [hist tables][256] then [npairs][L][L]
    __shared__ int pair_of[SPEC_SLOTS];             // corner q -> global pair index
    __shared__ int tab_of[SPEC_MAXT];               // group slot x -> table index (read after the loop from here, not kept)
    __shared__ int meta[4];                         // L, nt, histogram words, LDS words (the same)
    unsigned long long *const hist = accum, *const core = accum + (size_t)N * 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = g.L, LL = g.L * g.L, nt = g.nt;
    uint32_t *hl = lds;
    uint32_t *corner = lds + (g.hist ? nt * 256 : 0);
    for (int i = threadIdx.x; i < (g.hist ? nt * 256 : 0) + g.npairs * LL; i += blockDim.x) lds[i] = 0;
    if (threadIdx.x < SPEC_MAXT) tab_of[threadIdx.x] = g.t[threadIdx.x];
    if (threadIdx.x == 0) {
        meta[0] = L; meta[1] = nt; meta[2] = g.hist ? nt * 256 : 0; meta[3] = meta[2] + g.npairs * LL;
    }
    if (threadIdx.x == 0) {
        int q = 0;
        for (int x = 0; x < nt; x++)
            for (int y = x + 1; y < nt; y++)
                if (g.split == 0 || (x < g.split && y >= g.split)) {
                    const int i = g.t[x], j = g.t[y];
                    pair_of[q++] = i * N - i * (i + 1) / 2 + (j - i - 1);
                }
    }
    if (g.hist && blockIdx.x == 0 && threadIdx.x < nt) atomicAdd(&hist[g.t[threadIdx.x] * 256], (unsigned long long)n);
    __syncthreads();

    uint32_t acc11[SPEC_SLOTS / 2];                 // (1,1) events per pair slot, two 16-bit tallies per register
    uint32_t cnt[SPEC_MAXT];                        // per table: non-zero bytes (low half), bytes equal to 1 (high half)
#pragma unroll
    for (int s = 0; s < SPEC_SLOTS / 2; s++) acc11[s] = 0;
#pragma unroll
    for (int x = 0; x < SPEC_MAXT; x++) cnt[x] = 0;

    const uint64_t n_chunks = (n + 15u) / 16u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + wave * 64; base < n_chunks; base += stride) {   // wave-uniform
        const uint64_t c = base + lane;
        const bool live = c < n_chunks;
        uint4 v[SPEC_MAXT];
        uint32_t f[SPEC_MAXT];
        // the group's table pointers (gtab[x] = table g.t[x]) and size are fetched per chunk: held across the loop, they
        // and the per-table tests derived from them spill scalar registers
        const uint8_t *const *tp = gtab;
        int ntc = nt, hc = g.hist;
        asm volatile("" : "+s"(tp), "+s"(ntc), "+s"(hc));
#pragma unroll
        for (int x = 0; x < SPEC_MAXT; x++) {
            v[x] = make_uint4(0, 0, 0, 0);
            if (x < ntc && live) v[x] = load_half(tp[x], c * 16u, n);
        }
#pragma unroll
        for (int x = 0; x < SPEC_MAXT; x++) {
            if (x >= ntc) { f[x] = 0; continue; }
            f[x] = flags16(v[x]);
            if (hc) {
                cnt[x] += __builtin_popcount(f[x] & LO4) + (__builtin_popcount(f[x] & ~LO4) << 16);
                uint32_t ge2 = f[x] & ~(f[x] >> 4) & LO4;               // counts >= 2: the histogram's LDS rows
                while (ge2) {
                    const uint32_t p = __builtin_ctz(ge2);
                    ge2 &= ge2 - 1;
                    atomicAdd(&hl[x * 256 + byte_at(v[x], p)], 1u);
                }
            }
        }
        // the group's slot mask, opaque per chunk: otherwise the 120 slot tests are hoisted out of the loop as scalar
        // booleans, which spill
        uint32_t sm0 = g.slots[0], sm1 = g.slots[1], sm2 = g.slots[2], sm3 = g.slots[3];
        asm volatile("" : "+s"(sm0), "+s"(sm1), "+s"(sm2), "+s"(sm3));
        int q = 0;                                  // corner of the pair (x, y) in LDS
#pragma unroll
        for (int x = 0; x < SPEC_MAXT; x++)
#pragma unroll
            for (int y = x + 1; y < SPEC_MAXT; y++) {
                const int s = x * SPEC_MAXT - x * (x + 1) / 2 + (y - x - 1);   // compile-time slot
                const uint32_t sm = s < 32 ? sm0 : s < 64 ? sm1 : s < 96 ? sm2 : sm3;
                if (!((sm >> (s & 31)) & 1u)) continue;                        // uniform
                const uint32_t both = f[x] & f[y];
                const uint32_t j11 = (both >> 4) & LO4;
                acc11[s >> 1] += (uint32_t)__builtin_popcount(j11) << (16 * (s & 1));
                uint32_t rest = both & ~j11 & LO4;
                const int qq = q++;
                if (__builtin_amdgcn_ballot_w64(rest != 0) == 0) continue;
                uint32_t *cq = corner + qq * LL;
                const int pg = pair_of[qq];
                unsigned long long *cg = core + (size_t)pg * (255 * 255);
                do {
                    const bool act = rest != 0;
                    uint32_t a = 0, b = 0;
                    if (act) {
                        const uint32_t p = __builtin_ctz(rest);
                        rest &= rest - 1;
                        a = byte_at(v[x], p);
                        b = byte_at(v[y], p);
                    }
                    const bool in = act && a <= (uint32_t)L && b <= (uint32_t)L;
                    if (in) atomicAdd(&cq[(a - 1) * L + (b - 1)], 1u);
                    const bool out = act && !in;
                    const uint64_t om = __builtin_amdgcn_ballot_w64(out);
                    if (om) {
                        const uint32_t key = (a - 1) * 255u + (b - 1);
                        const int leader = __builtin_ctzll(om);
                        const uint32_t lk = __builtin_amdgcn_readlane(key, leader);
                        const uint64_t same = __builtin_amdgcn_ballot_w64(out && key == lk);
                        if (out) {
                            if (key != lk) atomicAdd(&cg[key], 1ull);
                            else if (lane == leader) atomicAdd(&cg[key], (unsigned long long)__builtin_popcountll(same));
                        }
                    }
                } while (__builtin_amdgcn_ballot_w64(rest != 0));
            }
    }

    // register tallies -> LDS ((1,1) is bin 0 of each corner, ones are row 1 of the histogram) and the zero counts.  The
    // group's sizes are read back from LDS here: kept in scalar registers across the loop, they spill.
    const int L2 = meta[0], LL2 = meta[0] * meta[0], nt2 = meta[1], hist_words = meta[2], words = meta[3];
    uint32_t *corner2 = lds + hist_words;
    {
        int q = 0;
#pragma unroll
        for (int x = 0; x < SPEC_MAXT; x++)
#pragma unroll
            for (int y = x + 1; y < SPEC_MAXT; y++) {
                const int s = x * SPEC_MAXT - x * (x + 1) / 2 + (y - x - 1);
                if (!((g.slots[s >> 5] >> (s & 31)) & 1u)) continue;
                const uint32_t t = spec_wave_sum((acc11[s >> 1] >> (16 * (s & 1))) & 0xffffu);
                if (lane == 0 && t) atomicAdd(&corner2[q * LL2], t);
                q++;
            }
    }
    if (hist_words) {
#pragma unroll
        for (int x = 0; x < SPEC_MAXT; x++) {
            if (x >= nt2) continue;
            const uint32_t nzs = spec_wave_sum(cnt[x] & 0xffffu), ones = spec_wave_sum(cnt[x] >> 16);
            if (lane == 0) {
                if (ones) atomicAdd(&hl[x * 256 + 1], ones);
                if (nzs) atomicAdd(&hist[tab_of[x] * 256], 0ull - (unsigned long long)nzs);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += blockDim.x) {
        const uint32_t val = lds[i];
        if (!val) continue;
        if (i < hist_words) {
            atomicAdd(&hist[tab_of[i >> 8] * 256 + (i & 255)], (unsigned long long)val);
        } else {
            const int k = i - hist_words, qq = k / LL2, r = k % LL2;
            atomicAdd(&core[(size_t)pair_of[qq] * (255 * 255) + (r / L2) * 255 + (r % L2)], (unsigned long long)val);
        }
    }
}

// Pair groups: N <= 16 one group holding every table (the tables are streamed once); beyond that blocks of 8 tables, a
// group per block (its inner pairs and its tables' histograms) and per pair of blocks (their cross pairs), each group
// streaming its tables again.  The corner edge L is the largest that fits the group's pairs in LDS.
int spectrum_groups(int N) {
    const int NB = (N + 7) / 8;
    return N <= SPEC_MAXT ? 1 : NB * (NB + 1) / 2;
}

int launch_spectrum(const void *const *dev_tables, int N, uint64_t n_slice, unsigned long long *dev_accum, const uint8_t **host_gtab,
                    const uint8_t **dev_gtab, hipStream_t s) {
    if (N < 2 || N > 128) return -1;
    if (n_slice == 0) return 0;
    static bool opted = false;
    if (!opted) {
        opted = true;
        hipFuncSetAttribute((const void *)k_spectrum, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_LDS);
    }
    int dev = 0, n_cu = 256;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    const uint64_t n_chunks = (n_slice + 15u) / 16u;
    const uint64_t wg_cap = (uint64_t)SPEC_THREADS * SPEC_MAX_CHUNKS;         // chunks one workgroup may take
    uint64_t grid = (n_chunks + SPEC_THREADS - 1) / SPEC_THREADS;
    if (grid > (uint64_t)n_cu) grid = (uint64_t)n_cu;                          // one workgroup per CU (LDS), persistent
    if (grid < (n_chunks + wg_cap - 1) / wg_cap) grid = (n_chunks + wg_cap - 1) / wg_cap;

    std::vector<SpecGroup> groups;
    auto add = [&](SpecGroup g) {
        const int hist_words = g.hist ? g.nt * 256 : 0;
        g.npairs = 0;
        for (int x = 0; x < SPEC_MAXT; x++)
            for (int y = x + 1; y < SPEC_MAXT; y++) {
                const int sl = x * SPEC_MAXT - x * (x + 1) / 2 + (y - x - 1);
                if (y < g.nt && (g.split == 0 || (x < g.split && y >= g.split))) {
                    g.slots[sl >> 5] |= 1u << (sl & 31);
                    g.npairs++;
                }
            }
        int L = 1;
        while (L < 255 && (size_t)(hist_words + (size_t)g.npairs * (L + 1) * (L + 1)) * 4u <= SPEC_LDS) L++;
        g.L = L;
        const size_t gi = groups.size();
        for (int x = 0; x < SPEC_MAXT; x++) host_gtab[gi * SPEC_MAXT + x] = x < g.nt ? (const uint8_t *)dev_tables[g.t[x]] : nullptr;
        groups.push_back(g);
    };
    if (N <= SPEC_MAXT) {
        SpecGroup g{};
        g.nt = N; g.split = 0; g.hist = 1;
        for (int x = 0; x < N; x++) g.t[x] = (int16_t)x;
        add(g);
    } else {
        constexpr int B = 8;
        const int NB = (N + B - 1) / B;
        for (int a = 0; a < NB; a++)
            for (int b = a; b < NB; b++) {
                SpecGroup g{};
                for (int i = a * B; i < std::min(N, a * B + B); i++) g.t[g.nt++] = (int16_t)i;
                g.split = 0; g.hist = 1;
                if (b != a) {
                    g.split = g.nt; g.hist = 0;
                    for (int i = b * B; i < std::min(N, b * B + B); i++) g.t[g.nt++] = (int16_t)i;
                }
                add(g);
            }
    }
    if (hipMemcpyAsync(dev_gtab, host_gtab, groups.size() * SPEC_MAXT * sizeof(void *), hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const SpecGroup &g = groups[gi];
        const size_t lds = (size_t)((g.hist ? g.nt * 256 : 0) + (size_t)g.npairs * g.L * g.L) * 4u;
        hipLaunchKernelGGL(k_spectrum, dim3((uint32_t)grid), dim3(SPEC_THREADS), lds, s, dev_gtab + gi * SPEC_MAXT, N, n_slice, g, dev_accum);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

}  // namespace pk
