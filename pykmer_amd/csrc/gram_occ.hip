// gram_occ.hip -- occupancy-stratified Gram products of N dense tables: the integers behind kWIP's entropy-weighted kernel.
//
// kWIP (Murray et al. 2017) weights each k-mer by the entropy of its sample occupancy o(x) = #{i : c_i(x) >= 1}.  The weight
// depends on x only through o(x), so every weighting is a sum over occupancy classes of class-stratified integer products.
// k_occgram ADDS to a flat u64 accumulator in HBM
//   occ_hist[N + 1]     #{x : o(x) = o}, o = 0..N
//   lin[N][N]           [o-1][i] = sum_{x : o(x) = o} c_i(x)
//   gram[N][T]          [o-1][p] = sum_{x : o(x) = o} c_i(x) * c_j(x), p = (i, j), i <= j, row-major upper triangle with the
//                       diagonal (T = N(N+1)/2)
// and the host does all the float64 weighting (pykmer_amd/kwip.py).
//
// Layout of the work.  A workgroup stages a tile of `tg` groups of 1024 addresses of the pass's tables (<= 16) in LDS, with
// one occupancy byte per address (summed from the staged tables for N <= 16, read from the k_occupancy scratch otherwise)
// and a class-present bitmask per group and per tile.  The pass's pairs come in items of 8 x 8 tables (a block with itself:
// the upper triangle, or two blocks); a wave's unit of work is (class o, item), for every class present in the tile.  It
// holds the item's 64 tallies in registers, one lane per 16 addresses: per group that holds class o it masks its rows to
// the addresses of class o (SWAR byte mask "occupancy == o") and adds v_dot4_u32_u8(row & mask, col) for 4 addresses at a
// time.  Diagonal items also tally lin (a dot4 with 0x01010101) and, in the pass that owns them, occ_hist[o], in the slots
// of the lower triangle the item leaves free.  After the tile the 64 tallies are summed over the wave by a transposing
// butterfly (lane l ends with slot l) and added to the workgroup's u64 tallies in LDS; those go to HBM once, at the end.
//
// No counter wraps: per tile a lane adds <= 4 * TG_MAX = 32 dot4 results (each <= 4 * 255^2) to a u32 tally, so a wave's
// sum is <= 64 * 32 * 260100 < 2^31; everything beyond the tile is u64.  Class 0 is never tallied: the pass that owns
// occ_hist adds n to occ_hist[0] once and every workgroup subtracts its classes 1..N (u64 wrap-around, exact at the end).
#include "pk_kernels.h"
#include "gram_load.h"
#include <algorithm>
#include <vector>

namespace pk {

constexpr int OG_THREADS = 256;                     // 4 waves
constexpr int OG_WAVES = OG_THREADS / 64;
constexpr int OG_MAXT = 16;                         // tables staged by one pass
constexpr int OG_TG_MAX = 8;                        // groups of 1024 addresses per tile
constexpr int OG_MW = 5;                            // class bitmask words: classes 0..128
constexpr int OG_LDS = 160 * 1024;

struct OccItem {
    int r0, c0;               // first staged slot of the row block and of the column block
    int nc;                   // tables of the column block (a row block is full, or, on the diagonal, the column block)
    int diag;                 // 1: a block with itself, pairs r <= c; also tallies lin of its tables
    int cnt;                  // 1: also tallies occ_hist
};

struct OccPass {
    const uint8_t *tab[OG_MAXT];
    const uint8_t *occ;       // occupancy bytes of the slice (N > 16), or null: the sum over the staged tables
    int nt, nitems, tg, words, hist;
    int16_t t[OG_MAXT];       // table index of staged slot x
    OccItem item[3];
};

__device__ __forceinline__ uint32_t og_nz(uint32_t v) { return ((((v & L4) + L4) | v) & H4) >> 7; }   // 1 per non-zero byte
__device__ __forceinline__ uint32_t og_eq(uint32_t v, uint32_t ob) {                                  // 0xff per byte == o
    const uint32_t y = v ^ ob;
    const uint32_t h = ~(((y & L4) + L4) | y) & H4;
    return (h - (h >> 7)) | h;
}
__device__ __forceinline__ uint32_t og_dot(const uint4 &a, const uint4 &b, uint32_t acc) {
    acc = __builtin_amdgcn_udot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_udot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_udot4(a.z, b.z, acc, false);
    return __builtin_amdgcn_udot4(a.w, b.w, acc, false);
}
__device__ __forceinline__ uint4 og_and(const uint4 &a, const uint4 &m) { return make_uint4(a.x & m.x, a.y & m.y, a.z & m.z, a.w & m.w); }

// the lower-triangle slots a diagonal item uses for lin[r] and occ_hist
__host__ __device__ constexpr int og_lin_slot(int r) { return r < 7 ? 7 * 8 + r : 6 * 8; }
constexpr int OG_CNT_SLOT = 6 * 8 + 1;

// One (class o, item) over the staged tile; lane l returns the wave's total of slot l.
template <bool DIAG>
__device__ uint32_t og_item(const uint4 *tabl, const uint4 *occl, const uint32_t *gm, int tg, int words, int o, const OccItem &it,
                            int lane) {
    uint32_t acc[64];
#pragma unroll
    for (int s = 0; s < 64; s++) acc[s] = 0;
    const uint32_t ob = (uint32_t)o * 0x01010101u;
    for (int g = 0; g < tg; g++) {
        const uint32_t bits = __builtin_amdgcn_readfirstlane(gm[g * OG_MW + (o >> 5)]);
        if (!((bits >> (o & 31)) & 1u)) continue;
        // the column count, opaque per group: otherwise its 16 tests are hoisted out of the loop as scalar masks
        int nc = it.nc;
        asm volatile("" : "+s"(nc));
        // rows and columns as lane addresses: their 16 scalar offsets would otherwise be live at once
        int rowi = (it.r0 * tg + g) * 64 + lane, coli = (it.c0 * tg + g) * 64 + lane, stride = tg * 64;
        asm volatile("" : "+v"(rowi), "+v"(coli), "+v"(stride));
        const uint4 oc = occl[g * 64 + lane];
        const uint4 m = make_uint4(og_eq(oc.x, ob), og_eq(oc.y, ob), og_eq(oc.z, ob), og_eq(oc.w, ob));
        uint4 a[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            a[r] = make_uint4(0, 0, 0, 0);
            if (!DIAG || r < nc) a[r] = og_and(tabl[rowi + r * stride], m);
        }
#pragma unroll
        for (int c = 0; c < 8; c++) {
            if (c >= nc) continue;                                  // uniform
            const uint4 b = DIAG ? a[c] : tabl[coli + c * stride];   // (c_i & m)(c_j & m) = (c_i & m) c_j
#pragma unroll
            for (int r = 0; r < 8; r++)
                if (!DIAG || r <= c) acc[r * 8 + c] = og_dot(a[r], b, acc[r * 8 + c]);
        }
        if (DIAG) {
            const uint4 ones = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
#pragma unroll
            for (int r = 0; r < 8; r++)
                if (r < nc) acc[og_lin_slot(r)] = og_dot(a[r], ones, acc[og_lin_slot(r)]);
            if (it.cnt) acc[OG_CNT_SLOT] = og_dot(og_and(m, ones), ones, acc[OG_CNT_SLOT]);
        }
    }
    // transposing butterfly: after the step of width s a lane keeps the half of its slots selected by lane bit s and adds
    // its partner's copy of that half; after six steps lane l holds the wave's sum of slot l
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const bool up = (lane & s) != 0;
#pragma unroll
        for (int k = 0; k < s; k++) {
            const uint32_t keep = up ? acc[k + s] : acc[k];
            const uint32_t send = up ? acc[k] : acc[k + s];
            acc[k] = keep + (uint32_t)__shfl_xor((int)send, s, 64);
        }
    }
    return acc[0];
}

__global__ __launch_bounds__(OG_THREADS) void k_occgram(const OccPass P, int N, uint64_t n, unsigned long long *__restrict__ accum) {
    extern __shared__ uint4 og_lds[];                 // u64 tallies [N classes][nitems * 64], tables [nt][tg][64], occupancy [tg][64]
    __shared__ uint32_t gm[OG_TG_MAX * OG_MW];        // classes present per group
    __shared__ uint32_t tu[OG_MW];                    // ... and in the tile
    __shared__ int tt[OG_MAXT];                       // table index of staged slot x
    __shared__ const uint8_t *tp[OG_MAXT];            // its pointer
    __shared__ OccItem items[3];                      // (pointers and items are read where used, not held in scalar
                                                      // registers across the loops: see DESIGN 4.8 on scalar pressure)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tg = P.tg, words = P.words, nslots = P.nitems * 64;
    unsigned long long *tl = (unsigned long long *)og_lds;
    uint4 *tabl = og_lds + (size_t)N * nslots / 2;
    uint4 *occl = tabl + (size_t)P.nt * tg * 64;
    for (int i = threadIdx.x; i < N * nslots; i += OG_THREADS) tl[i] = 0;
    if (threadIdx.x < OG_MAXT) {
        tt[threadIdx.x] = P.t[threadIdx.x];
        tp[threadIdx.x] = P.tab[threadIdx.x];
    }
    if (threadIdx.x < 3) items[threadIdx.x] = P.item[threadIdx.x];
    __syncthreads();
    if (P.hist && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&accum[0], (unsigned long long)n);

    const uint64_t tile_bytes = (uint64_t)tg * 1024u;
    const uint32_t n_tiles = (uint32_t)((n + tile_bytes - 1) / tile_bytes);    // < 2^32 for any table of k <= 20
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();                                            // the previous tile's items are done
        if (threadIdx.x < tg * OG_MW) gm[threadIdx.x] = 0;
        if (threadIdx.x < OG_MW) tu[threadIdx.x] = 0;
        __syncthreads();
        for (int g = wave; g < tg; g += OG_WAVES) {
            const uint64_t off = (uint64_t)tile * tile_bytes + (uint64_t)g * 1024u + (uint64_t)lane * 16u;
            int nt = P.nt, words = P.words;                         // opaque per group: the 16 + 5 tests on them are
            asm volatile("" : "+s"(nt), "+s"(words));               // hoisted out of the loop as scalar masks otherwise
            uint4 v[OG_MAXT];
#pragma unroll
            for (int x = 0; x < OG_MAXT; x++)
                if (x < nt) v[x] = load_half(tp[x], off, n);
            uint4 oc;
            if (P.occ) {
                oc = load_half(P.occ, off, n);
            } else {
                oc = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int x = 0; x < OG_MAXT; x++)
                    if (x < nt) oc = make_uint4(oc.x + og_nz(v[x].x), oc.y + og_nz(v[x].y), oc.z + og_nz(v[x].z), oc.w + og_nz(v[x].w));
            }
#pragma unroll
            for (int x = 0; x < OG_MAXT; x++)
                if (x < nt) tabl[(x * tg + g) * 64 + lane] = v[x];
            occl[g * 64 + lane] = oc;
            const uint32_t ow[4] = {oc.x, oc.y, oc.z, oc.w};
            uint32_t cm[OG_MW] = {0, 0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const uint32_t o = (ow[b >> 2] >> (8 * (b & 3))) & 0xffu;
#pragma unroll
                for (int k = 0; k < OG_MW; k++)
                    if (k < words) cm[k] |= (o >> 5) == (uint32_t)k ? 1u << (o & 31) : 0u;
            }
#pragma unroll
            for (int k = 0; k < OG_MW; k++) {
                if (k >= words) continue;
                uint32_t x = cm[k] & (k == 0 ? ~1u : ~0u);          // class 0 is not tallied
#pragma unroll
                for (int d = 32; d; d >>= 1) x |= (uint32_t)__shfl_xor((int)x, d, 64);
                if (lane == 0 && x) {
                    gm[g * OG_MW + k] = x;
                    atomicOr(&tu[k], x);
                }
            }
        }
        __syncthreads();
        int q = 0;                                                  // (class, item) units in order; wave q % 4 takes unit q
        for (int k = 0; k < words; k++) {
            uint32_t bits = __builtin_amdgcn_readfirstlane(tu[k]);
            while (bits) {
                const int o = k * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                for (int i = 0; i < P.nitems; i++) {
                    OccItem it;
                    it.r0 = __builtin_amdgcn_readfirstlane(items[i].r0);
                    it.c0 = __builtin_amdgcn_readfirstlane(items[i].c0);
                    it.nc = __builtin_amdgcn_readfirstlane(items[i].nc);
                    it.diag = __builtin_amdgcn_readfirstlane(items[i].diag);
                    it.cnt = __builtin_amdgcn_readfirstlane(items[i].cnt);
                    if (!it.diag && o == 1) continue;               // one table holds the k-mer: no cross products
                    if (q++ % OG_WAVES != wave) continue;
                    const uint32_t s = it.diag ? og_item<true>(tabl, occl, gm, tg, words, o, it, lane)
                                               : og_item<false>(tabl, occl, gm, tg, words, o, it, lane);
                    if (s) atomicAdd(&tl[(size_t)(o - 1) * nslots + i * 64 + lane], (unsigned long long)s);
                }
            }
        }
    }
    __syncthreads();
    // workgroup tallies -> HBM: occ_hist [N + 1], lin [N][N], gram [N][T]
    unsigned long long *hist = accum, *lin = accum + (N + 1), *gram = lin + (size_t)N * N;
    const int T = N * (N + 1) / 2;
    for (int ii = 0; ii < P.nitems; ii++) {
        const OccItem it = P.item[ii];
        for (int i = threadIdx.x; i < N * 64; i += OG_THREADS) {
            const int o = i / 64 + 1, s = i % 64, r = s >> 3, c = s & 7;
            const unsigned long long v = tl[(size_t)(o - 1) * nslots + ii * 64 + s];
            if (!v) continue;
            if (!it.diag || r <= c) {
                const int a = tt[it.r0 + r], b = tt[it.c0 + c];
                atomicAdd(&gram[(size_t)(o - 1) * T + a * N - a * (a - 1) / 2 + (b - a)], v);
            } else if (s == OG_CNT_SLOT) {
                atomicAdd(&hist[o], v);
                atomicAdd(&hist[0], 0ull - v);
            } else {
                atomicAdd(&lin[(size_t)(o - 1) * N + tt[it.r0 + (s == og_lin_slot(7) ? 7 : c)]], v);
            }
        }
    }
}

// Occupancy bytes of N > 16 tables (one byte per address, <= 128) for the passes that stage only some of them.
__global__ __launch_bounds__(256) void k_occupancy(const uint8_t *const *__restrict__ tabs, int N, uint64_t n, uint8_t *__restrict__ occ) {
    const uint64_t n_chunks = (n + 15u) / 16u;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * blockDim.x) {
        uint4 s = make_uint4(0, 0, 0, 0);
        for (int t = 0; t < N; t++) {
            const uint4 v = load_half(tabs[t], c * 16u, n);
            s = make_uint4(s.x + og_nz(v.x), s.y + og_nz(v.y), s.z + og_nz(v.z), s.w + og_nz(v.w));
        }
        *(uint4 *)(occ + c * 16u) = s;                          // the scratch holds occgram_scratch_bytes(n) >= 16 * n_chunks
    }
}

uint64_t occgram_scratch_bytes(int N, uint64_t n_slice) { return N > OG_MAXT ? (n_slice + 15u) / 16u * 16u : 0; }

// Passes: N <= 16 one pass staging every table, items (block 0, block 0), (0, 1), (1, 1) of 8 tables; beyond that one pass
// per block of 8 (its upper triangle, its lin, occ_hist in the first) and per pair of blocks (their cross pairs), each
// reading the occupancy scratch.  tg is the largest tile that lets two workgroups share a CU, else one.
int launch_occgram(const void *const *dev_tables, int N, uint64_t n_slice, unsigned long long *dev_accum, const uint8_t **dev_ptrs,
                   uint8_t *occ_scratch, hipStream_t s) {
    if (N < 2 || N > 128) return -1;
    if (n_slice == 0) return 0;
    static bool opted = false;
    if (!opted) {
        opted = true;
        hipFuncSetAttribute((const void *)k_occgram, hipFuncAttributeMaxDynamicSharedMemorySize, OG_LDS - 1024);
    }
    int dev = 0, n_cu = 256;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);

    std::vector<OccPass> passes;
    auto block = [&](int b) { return std::make_pair(b * 8, std::min(N, b * 8 + 8)); };
    if (N <= OG_MAXT) {
        OccPass p{};
        p.nt = N; p.hist = 1; p.occ = nullptr;
        for (int x = 0; x < N; x++) p.t[x] = (int16_t)x;
        p.item[p.nitems++] = OccItem{0, 0, std::min(N, 8), 1, 1};
        if (N > 8) {
            p.item[p.nitems++] = OccItem{0, 8, N - 8, 0, 0};
            p.item[p.nitems++] = OccItem{8, 8, N - 8, 1, 0};
        }
        passes.push_back(p);
    } else {
        const int NB = (N + 7) / 8;
        for (int a = 0; a < NB; a++)
            for (int b = a; b < NB; b++) {
                OccPass p{};
                p.occ = occ_scratch;
                const auto A = block(a), B = block(b);
                for (int i = A.first; i < A.second; i++) p.t[p.nt++] = (int16_t)i;
                if (a == b) {
                    p.hist = a == 0;
                    p.item[p.nitems++] = OccItem{0, 0, p.nt, 1, p.hist};
                } else {
                    for (int i = B.first; i < B.second; i++) p.t[p.nt++] = (int16_t)i;
                    p.item[p.nitems++] = OccItem{0, 8, B.second - B.first, 0, 0};
                }
                passes.push_back(p);
            }
        if (hipMemcpyAsync(dev_ptrs, dev_tables, N * sizeof(void *), hipMemcpyHostToDevice, s) != hipSuccess) return -2;
        const uint64_t n_chunks = (n_slice + 15u) / 16u;
        const uint64_t grid = std::min<uint64_t>((n_chunks + 255) / 256, (uint64_t)n_cu * 8);
        hipLaunchKernelGGL(k_occupancy, dim3((uint32_t)grid), dim3(256), 0, s, dev_ptrs, N, n_slice, occ_scratch);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    const int words = (N + 1 + 31) / 32;
    for (OccPass &p : passes) {
        for (int x = 0; x < p.nt; x++) p.tab[x] = (const uint8_t *)dev_tables[p.t[x]];
        p.words = words;
        const size_t tl_bytes = (size_t)N * p.nitems * 64 * 8;
        const size_t per_group = (size_t)1024 * (p.nt + 1);
        int per_cu = 2;
        size_t avail = OG_LDS / 2 - 1024;
        if (tl_bytes + 2 * per_group > avail) { per_cu = 1; avail = OG_LDS - 1024; }
        p.tg = (int)std::min<size_t>(OG_TG_MAX, (avail - tl_bytes) / per_group);
        if (p.tg < 1) return -1;
        const size_t lds = tl_bytes + per_group * p.tg;
        const uint64_t n_tiles = (n_slice + (uint64_t)p.tg * 1024 - 1) / ((uint64_t)p.tg * 1024);
        const uint64_t grid = std::min<uint64_t>(n_tiles, (uint64_t)n_cu * per_cu);
        hipLaunchKernelGGL(k_occgram, dim3((uint32_t)grid), dim3(OG_THREADS), lds, s, p, N, n_slice, dev_accum);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

}  // namespace pk
