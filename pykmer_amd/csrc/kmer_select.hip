// kmer_select.hip -- the bytes of a chosen subset of records of a byte stream.  The stream is cut into R
// records by R + 1 non-decreasing offsets: record r is the bytes [starts[r], starts[r + 1]), bytes below starts[0] and at or
// beyond starts[R] belong to no record, and keep[r] != 0 keeps record r.  A piece of the stream, text[0 .. n) at stream offset
// `pos`, goes in; the bytes of it that lie in kept records come out, in order, back to back.  No parser runs: the offsets
// come from an earlier parse (pk_record.name_off), so FASTA, FASTQ and anything else cut this way are the same to it.
// No reference counterpart (its README stops at the distance matrix).
//
// A three-launch stream compaction with the geometry of the text kernels (one workgroup per 16 KiB chunk, one 64-byte piece
// per lane); no workgroup ever waits for another:
//   k_sel_count  the workgroup finds the records of the chunk's first and last record byte over all of starts, 256 probes a
//                round (sel_record_of_wg); every lane then finds the record of its piece's first byte between those two by
//                binary search (a handful of steps on lines its neighbours read as well), walks the record boundaries inside
//                its piece into a 64-bit keep mask, leaves the mask in HBM (8 bytes per 64 of text) and adds its population
//                to the chunk's count
//   k_sel_scan   one workgroup, in place: the exclusive prefix of the chunk counts, and the piece's total
//   k_sel_write  returns at once when the total is not the one the host expects (it knows the number exactly and has sized
//                the output for it: nothing is ever written beyond it).  Otherwise a chunk with kept bytes stages its text in LDS, ranks its lanes' kept bytes,
//                compacts them in LDS at the byte alignment of their place in the output and writes that contiguous range:
//                full dwords as dwords, the unaligned head and tail byte by byte (k_fq_write's way out)
#include "pk_kernels.h"
#include "wg_scan.h"

namespace pk {

constexpr int SEL_SCAN_T = 1024;                 // threads of the scan

// the largest r in [a, b] with starts[r] <= x; starts[a] <= x.  Among equal offsets (empty records) it is the last one,
// so with x < starts[b + 1] record r is the one that holds byte x.
__device__ __forceinline__ uint64_t sel_record_of(const unsigned long long *__restrict__ starts, uint64_t a, uint64_t b, uint64_t x) {
    while (a < b) {
        const uint64_t m = a + (b - a + 1u) / 2u;
        if (starts[m] <= x) a = m; else b = m - 1u;
    }
    return a;
}

// The same by the whole workgroup (a, b and x the same in every thread; every thread gets the answer): every round the WG
// threads probe WG evenly spaced offsets at once and count those at or below x -- the offsets do not decrease, so they
// are the leading ones -- which cuts the range by WG + 1: three rounds of one load for a million records, where one
// thread halving the range would wait for twenty loads one after the other.
__device__ __forceinline__ uint64_t sel_record_of_wg(const unsigned long long *__restrict__ starts, uint64_t a, uint64_t b, uint64_t x) {
    while (a < b) {                              // uniform
        const uint64_t step = (b - a) / WG + 1u; // a + WG * step > b: the probes reach past the range
        const uint64_t p = a + ((uint64_t)threadIdx.x + 1u) * step;
        const uint32_t c = (uint32_t)__syncthreads_count(p <= b && starts[p] <= x);
        a += (uint64_t)c * step;                 // starts[a] <= x still; the next probe, if it lies in the range, is above x
        if (a + step - 1u < b) b = a + step - 1u;
    }
    return a;
}

// bits [a, b) of a 64-bit word, 0 <= a < b <= 64
__device__ __forceinline__ unsigned long long sel_bits(uint32_t a, uint32_t b) {
    return (b >= 64u ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
}

// masks[chunk * WG + lane]: bit i = byte i of the lane's piece lies in a kept record; sums[chunk] = kept bytes of the chunk.
// R >= 1 (the host launches nothing for a stream without records).
__global__ __launch_bounds__(WG) void k_sel_count(const unsigned long long *__restrict__ starts, const uint8_t *__restrict__ keep, uint64_t R,
                                                  uint64_t pos, uint64_t n, unsigned long long *__restrict__ masks,
                                                  unsigned long long *__restrict__ sums) {
    __shared__ uint32_t wsum[WG / 64];
    const uint64_t base = (uint64_t)blockIdx.x * CHUNK;
    const uint64_t c0 = pos + base, c1 = pos + (n - base < (uint64_t)CHUNK ? n : base + CHUNK);   // the chunk's stream offsets
    const uint64_t first = starts[0], last = starts[R];
    const uint64_t lo = c0 > first ? c0 : first, hi = c1 < last ? c1 : last;   // its bytes that belong to a record: [lo, hi)
    unsigned long long mask = 0;
    if (lo < hi) {                               // uniform
        const uint64_t e0 = sel_record_of_wg(starts, 0, R - 1u, lo), e1 = sel_record_of_wg(starts, e0, R - 1u, hi - 1u);
        const uint64_t g0 = c0 + (uint64_t)threadIdx.x * PIECE;
        const uint64_t g1 = g0 + PIECE < c1 ? g0 + PIECE : c1;
        uint64_t o = g0 > lo ? g0 : lo;
        const uint64_t end = g1 < hi ? g1 : hi;
        if (o < end) {
            // starts[r] <= o < starts[r + 1] going in; behind a boundary o = starts[r], and an empty record moves nothing.
            // o < end <= starts[R], so the walk ends at r = R - 1 at the latest.
            uint64_t r = sel_record_of(starts, e0, e1, o);
            while (o < end) {
                uint64_t e = starts[r + 1u];
                if (e > end) e = end;
                if (e > o && keep[r]) mask |= sel_bits((uint32_t)(o - g0), (uint32_t)(e - g0));
                o = e;
                r++;
            }
        }
    }
    masks[(uint64_t)blockIdx.x * WG + threadIdx.x] = mask;
    uint32_t total;
    wg_excl_sum<WG / 64, false>((uint32_t)__popcll(mask), wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. n_chunks): counts -> exclusive prefix sums, in place; sums[n_chunks] = the total, also added to *grand
__global__ __launch_bounds__(SEL_SCAN_T) void k_sel_scan(unsigned long long *__restrict__ sums, uint32_t n_chunks, unsigned long long *__restrict__ grand) {
    __shared__ unsigned long long wsum[SEL_SCAN_T / 64];
    unsigned long long run = 0;
    for (uint32_t b0 = 0; b0 < n_chunks; b0 += SEL_SCAN_T) {
        const uint32_t b = b0 + threadIdx.x;
        const unsigned long long v = b < n_chunks ? sums[b] : 0ull;
        unsigned long long total;
        const unsigned long long pre = wg_excl_sum<SEL_SCAN_T / 64, true>(v, wsum, total);
        if (b < n_chunks) sums[b] = run + pre;
        run += total;
    }
    if (threadIdx.x == 0) {
        sums[n_chunks] = run;
        *grand += run;                           // one workgroup on an in-order stream: no other writer
    }
}

// out[sums[chunk] .. sums[chunk + 1]) = the chunk's kept bytes.  text is 16-byte aligned; out has any alignment.
__global__ __launch_bounds__(WG) void k_sel_write(const uint8_t *__restrict__ text, uint64_t n, const unsigned long long *__restrict__ masks,
                                                  const unsigned long long *__restrict__ sums, uint32_t n_chunks, uint8_t *__restrict__ out,
                                                  uint64_t expected) {
    __shared__ __align__(16) uint8_t lds[WG * LDS_STRIDE];
    __shared__ __align__(16) uint8_t obuf[CHUNK + 16];
    __shared__ uint32_t wsum[WG / 64];
    if (sums[n_chunks] != expected) return;      // not what the host sized the output for: nothing is written (the host reports it)
    const unsigned long long off = sums[blockIdx.x];
    if (sums[blockIdx.x + 1u] == off) return;    // nothing kept here (sums[n_chunks] is the total, so the last chunk reads it)
    const uint64_t base = (uint64_t)blockIdx.x * CHUNK;
    stage_chunk(text, base, n, lds);
    const unsigned long long mask = masks[(uint64_t)blockIdx.x * WG + threadIdx.x];
    uint32_t S;                                  // the barrier inside also puts the staged text in front of its readers
    const uint32_t rank = wg_excl_sum<WG / 64, false>((uint32_t)__popcll(mask), wsum, S);
    const uintptr_t a_lo = (uintptr_t)(out + off), a_hi = a_lo + S, w_lo = a_lo & ~(uintptr_t)3;
    const uint8_t *mine = lds + threadIdx.x * LDS_STRIDE;
    uint8_t *dst = obuf + (uint32_t)(a_lo - w_lo) + rank;
    if (mask) {
        // every lane starts 4 bytes further into its piece than the lane before it: side by side the lanes' targets lie
        // 64 bytes apart (when most bytes are kept), which in step would be two LDS banks for the whole wave
        const uint32_t rot = (threadIdx.x * 4u) & 63u;
        for (uint32_t i = 0; i < (uint32_t)PIECE; i++) {
            const uint32_t p = (i + rot) & 63u;
            if ((mask >> p) & 1ull) dst[__popcll(mask & ((1ull << p) - 1ull))] = mine[p];
        }
    }
    __syncthreads();
    for (uintptr_t w = w_lo + 4u * threadIdx.x; w < a_hi; w += 4u * WG) {
        const uint32_t li = (uint32_t)(w - w_lo);
        if (w >= a_lo && w + 4u <= a_hi) {
            *reinterpret_cast<uint32_t *>(w) = *reinterpret_cast<const uint32_t *>(obuf + li);
        } else {
            for (uint32_t j = 0; j < 4u; j++)
                if (w + j >= a_lo && w + j < a_hi) *reinterpret_cast<uint8_t *>(w + j) = obuf[li + j];
        }
    }
}

uint32_t select_chunks(uint64_t n) { return (uint32_t)((n + CHUNK - 1) / CHUNK); }

int launch_select(const unsigned long long *starts, const uint8_t *keep, uint64_t R, const uint8_t *text, uint64_t pos, uint64_t n,
                  unsigned long long *masks, unsigned long long *sums, unsigned long long *grand, uint8_t *out, uint64_t expected, hipStream_t s) {
    const uint32_t n_chunks = select_chunks(n);
    if (!n_chunks || !R) return 0;
    hipLaunchKernelGGL(k_sel_count, dim3(n_chunks), dim3(WG), 0, s, starts, keep, R, pos, n, masks, sums);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(SEL_SCAN_T), 0, s, sums, n_chunks, grand);
    hipLaunchKernelGGL(k_sel_write, dim3(n_chunks), dim3(WG), 0, s, text, n, (const unsigned long long *)masks, (const unsigned long long *)sums,
                       n_chunks, out, expected);
    return hipGetLastError() != hipSuccess;
}

}  // namespace pk
