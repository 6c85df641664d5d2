// kmer_correct.hip -- single-base corrections of the reads of a FASTQ feed (README "Correcting reads").  A
// feed is kmer_trim.hip's: whole records cut by R + 1 offsets, no parser state; k_trim_count and k_trim_scan run as they are
// (launch_trim_geometry) and leave every record's line geometry, its valid bases and its first cover bit.  No reference
// counterpart (its README stops at the distance matrix).
//
//   k_correct_runs<KT>  one wavefront per record.  It walks line 2 in 64-position steps (the loads of TRIM_STEPS steps in
//                 flight): the step's valid bases V as a ballot, their cover bits C (cover_select) and the 2-bit codes of its
//                 bases, 16 to a word, into a ring of four steps in LDS.  A CANDIDATE is a valid base that is not covered
//                 and lies in a run of at least k valid bases; its windows are the k-mers of the run that hold it, w of
//                 them.  A candidate of step m is judged one step late, when V of step m + 1 is known: k <= 17 < 64, so by
//                 then the run's end is known or known to lie at or beyond p + k, and the same holds for its start and step
//                 m - 1.  Candidates are taken one at a time with lanes = (base, window), 3 w <= 51 of them: each lane cuts
//                 its window out of the ring, puts its base at p, forms the canonical k-mer (forward word: first base
//                 highest; reverse: complemented, as q_kmers) and gathers table after table until one matches -- first one
//                 window of every base, then the other windows of the bases whose first one matched.  One ballot
//                 says per base whether all its windows matched: exactly one base -> the lane that holds p writes the byte
//                 into text_out, keeping its case.  Every candidate is judged against the text as it was read: text_out is
//                 never read.
// Positions, valid bases and cover bits are kmer_trim.hip's; every load is guarded by the record's own end.
#include "kmer_trim.h"

namespace pk {

constexpr uint32_t CORR_RING = 16;               // words of a wave's ring: four steps of 64 codes, 16 to a word

// bit i of x -> bit 2 i
__device__ __forceinline__ unsigned long long corr_spread(uint32_t x32) {
    unsigned long long x = x32;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// 2-bit field i of the low k fields -> field k - 1 - i
__device__ __forceinline__ uint32_t corr_reverse(uint32_t x, uint32_t k) {
    const uint32_t r = __builtin_bitreverse32(x);
    return (((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u)) >> (32u - 2u * k);
}
__device__ __forceinline__ unsigned long long corr_reverse(unsigned long long x, uint32_t k) {
    const unsigned long long r = __builtin_bitreverse64(x);
    return (((r & 0x5555555555555555ull) << 1) | ((r >> 1) & 0x5555555555555555ull)) >> (64u - 2u * k);
}

// the lanes of a wave see each other's LDS words on either side of this
__device__ __forceinline__ void corr_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// What a record's walk carries from step to step: the valid bases of the step before the one being judged, and of that
// step its valid bases, cover bits, the two bit planes of its codes and every lane's byte; the record's counts.
struct CorrWalk {
    unsigned long long Vp, Vc, Cc, Lc, Hc;
    uint32_t byte_c;
    uint32_t candidates, untried, corrected, ambiguous;
};

// Step m of the walk (its first position: q = 64 m; c, qv: its bytes of lines 2 and 4, blanks behind the sequence): its
// codes go into the ring, and the candidates of step m - 1 are judged.  g: the ordinal of the step's first cover bit.
template <typename KT>
__device__ __forceinline__ void corr_step(CorrWalk &w, uint32_t *ring, uint32_t lane, uint64_t q, uint32_t c, uint32_t qv, uint32_t tq,
                                          unsigned long long &g, const uint32_t *__restrict__ bits, unsigned long long n_words, uint32_t k,
                                          const uint8_t *const *__restrict__ tables, uint32_t n_tab, uint32_t mn, uint32_t mx, uint32_t min_windows,
                                          uint64_t p2, uint64_t n, uint8_t *__restrict__ text_out) {
    const uint32_t code = base_code(c);
    const unsigned long long Vn = trim_valid(c, qv, tq);
    const unsigned long long Cn = Vn ? cover_select(Vn, g, bits, n_words, false) : 0ull;
    g += (unsigned long long)__popcll(Vn);
    const unsigned long long Ln = __ballot((code & 1u) != 0u), Hn = __ballot((code & 2u) != 0u);
    const unsigned long long W0 = corr_spread((uint32_t)Ln) | (corr_spread((uint32_t)Hn) << 1);
    const unsigned long long W1 = corr_spread((uint32_t)(Ln >> 32)) | (corr_spread((uint32_t)(Hn >> 32)) << 1);
    corr_wave_sync();                                        // the step before has read what it needed of the ring
    if (lane < 4u) {
        const unsigned long long W = lane < 2u ? W0 : W1;
        ring[(((uint32_t)q >> 4) + lane) & (CORR_RING - 1u)] = (uint32_t)(W >> (32u * (lane & 1u)));
    }
    corr_wave_sync();
    const KT mask = (KT)((2u * k >= sizeof(KT) * 8u) ? ~(KT)0 : (((KT)1 << (2u * k)) - 1));
    const uint64_t qc = q - 64u;                             // the first position of the step being judged (no candidate at q = 0)
    unsigned long long cand = w.Vc & ~w.Cc;
    while (cand) {
        const uint32_t i = (uint32_t)__builtin_ctzll(cand);
        cand &= cand - 1ull;
        // the valid bases below and above p, nearest first, k - 1 of them at most
        const unsigned long long below = ~(i ? (w.Vp >> i) | (w.Vc << (64u - i)) : w.Vp);
        const unsigned long long above = ~(i == 63u ? Vn : (w.Vc >> (i + 1u)) | (Vn << (63u - i)));
        const uint32_t nl = min(below ? (uint32_t)__builtin_clzll(below) : 64u, k - 1u);
        const uint32_t nr = min(above ? (uint32_t)__builtin_ctzll(above) : 64u, k - 1u);
        if (nl + nr + 1u < k) continue;                      // its run is shorter than k: no window, no candidate
        w.candidates++;
        const uint32_t nw = nl + nr + 2u - k;                // its windows begin at p - nl .. p + nr - (k - 1)
        if (nw < min_windows) { w.untried++; continue; }
        const uint32_t old = (uint32_t)((w.Lc >> i) & 1ull) | ((uint32_t)((w.Hc >> i) & 1ull) << 1);
        const uint32_t bi = (lane >= nw ? 1u : 0u) + (lane >= 2u * nw ? 1u : 0u), wi = lane - bi * nw;
        const bool active = lane < 3u * nw;
        const uint32_t b = bi + (bi >= old ? 1u : 0u);       // the three bases other than the read's own
        const uint32_t s = (uint32_t)qc + i - nl + wi;       // the window's first position, modulo 2^32: the ring takes its low bits
        const uint32_t wd = (s >> 4) & (CORR_RING - 1u), sh = 2u * (s & 15u);
        const unsigned long long two = ((unsigned long long)ring[(wd + 1u) & (CORR_RING - 1u)] << 32) | ring[wd];
        const uint32_t at = 2u * ((nl - wi) & (uint32_t)(sizeof(KT) * 4u - 1u));   // p's field in the window, first base lowest (an idle lane's: any)
        KT P = (KT)(two >> sh);
        P = (KT)(((P & ~((KT)3 << at)) | ((KT)b << at)) & mask);
        const KT fwd = (KT)corr_reverse(P, k), rev = (KT)(~P & mask);
        const uint64_t a = (uint64_t)(fwd < rev ? fwd : rev);
        // the lanes with `mine` gather table after table until one matches; the loop ends when no lane wants a table
        const auto gather = [&](bool mine) -> bool {
            bool hit = false;
            for (uint32_t t = 0; t < n_tab; t++) {
                const bool want = mine && !hit;
                if (!__ballot(want)) break;
                if (want) {
                    const uint32_t v = tables[t][a];
                    hit = v >= mn && v <= mx;
                }
            }
            return hit;
        };
        // First one window of every base, the one that begins at p - nl: a base whose first window matches nowhere has
        // failed, and its other windows are not looked up.  Most candidates end here: three lanes' gathers, not 3 w.
        const bool lead = active && wi == 0u;
        const unsigned long long H0 = __ballot(lead && gather(lead));
        const bool alive = active && ((H0 >> (bi * nw)) & 1ull) != 0ull;
        const bool rest = alive && wi != 0u;
        const bool hit = gather(rest);
        const unsigned long long H = __ballot(alive && (wi == 0u || hit)), all = (1ull << nw) - 1ull;
        const bool p0 = (H & all) == all, p1 = ((H >> nw) & all) == all, p2b = ((H >> (2u * nw)) & all) == all;
        const uint32_t passing = (p0 ? 1u : 0u) + (p1 ? 1u : 0u) + (p2b ? 1u : 0u);
        if (passing == 1u) {
            w.corrected++;
            const uint32_t pb = p0 ? 0u : (p1 ? 1u : 2u), nb = pb + (pb >= old ? 1u : 0u);
            const uint64_t pos = qc + i;
            if (lane == i && pos < n) text_out[p2 + pos] = (uint8_t)(((0x54474341u >> (8u * nb)) & 0xffu) | (w.byte_c & 0x20u));
        } else if (passing > 1u) {
            w.ambiguous++;
        }
    }
    w.Vp = w.Vc; w.Vc = Vn; w.Cc = Cn; w.Lc = Ln; w.Hc = Hn; w.byte_c = c;
}

// Per record r: out + f * R + r for the fields pos2, seq_len (geo's), candidates, untried, corrected, ambiguous, and the
// corrected bytes in text_out.  first[r]: the stream's valid bases before the record.
template <typename KT>
__global__ __launch_bounds__(WG) void k_correct_runs(const uint8_t *__restrict__ text, uint64_t R, uint64_t pos, uint32_t tq,
                                                     const unsigned long long *__restrict__ first, const uint32_t *__restrict__ bits,
                                                     unsigned long long n_words, const unsigned long long *__restrict__ geo, uint32_t k,
                                                     const uint8_t *const *__restrict__ tables, uint32_t n_tab, uint32_t mn, uint32_t mx,
                                                     uint32_t min_windows, uint8_t *__restrict__ text_out, unsigned long long *__restrict__ out) {
    __shared__ uint32_t rings[TRIM_WAVES][CORR_RING];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform: the record's offsets are scalar loads
    uint32_t *ring = rings[wave];
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_WAVES + wave; r < R; r += (uint64_t)gridDim.x * TRIM_WAVES) {
        const uint64_t p2 = geo[r] - pos, p4 = geo[R + r] - pos, e4 = geo[3u * R + r] - pos, n = geo[4u * R + r];
        unsigned long long g = first[r];
        CorrWalk w;
        w.Vp = w.Vc = w.Cc = w.Lc = w.Hc = 0ull;
        w.byte_c = 32u;
        w.candidates = w.untried = w.corrected = w.ambiguous = 0u;
        // a record shorter than k has no run of k bases; the step behind the last one judges the last one's candidates
        for (uint64_t q0 = 0; n >= k && q0 < n + 64u; q0 += TRIM_ROUND) {
            uint32_t c[TRIM_STEPS], qv[TRIM_STEPS];
            trim_load(text, p2 + q0, p2 + n, lane, 32u, c);
            trim_load_qual(text, p2 + q0, p2 + n, p4 + q0, e4, lane, tq, qv);
#pragma unroll
            for (int j = 0; j < TRIM_STEPS; j++) {
                const uint64_t q = q0 + 64u * (uint32_t)j;
                if (q >= n + 64u) break;
                corr_step<KT>(w, ring, lane, q, c[j], qv[j], tq, g, bits, n_words, k, tables, n_tab, mn, mx, min_windows, p2, n, text_out);
            }
        }
        if (lane == 0u) {
            out[r] = geo[r];
            out[R + r] = n;
            out[2u * R + r] = w.candidates;
            out[3u * R + r] = w.untried;
            out[4u * R + r] = w.corrected;
            out[5u * R + r] = w.ambiguous;
        }
    }
}

int launch_correct(const uint8_t *text, const unsigned long long *starts, uint64_t R, uint64_t pos, uint32_t tq, const uint32_t *bits,
                   uint64_t n_words, unsigned long long base, unsigned long long *cnt, unsigned long long *total, unsigned long long *geo,
                   uint32_t k, const uint8_t *const *tables, uint32_t n_tab, uint32_t min_count, uint32_t max_count, uint32_t min_windows,
                   uint8_t *text_out, unsigned long long *out, hipStream_t s) {
    if (!R) return 0;
    launch_trim_geometry(text, starts, R, pos, tq, base, cnt, total, geo, s);
    const uint64_t want = (R + TRIM_WAVES - 1u) / TRIM_WAVES;
    const uint32_t wgs = (uint32_t)(want < TRIM_MAX_WGS ? want : TRIM_MAX_WGS);
    if (k <= 15u)
        hipLaunchKernelGGL(k_correct_runs<uint32_t>, dim3(wgs), dim3(WG), 0, s, text, R, pos, tq, (const unsigned long long *)cnt, bits,
                           (unsigned long long)n_words, (const unsigned long long *)geo, k, tables, n_tab, min_count, max_count, min_windows, text_out, out);
    else
        hipLaunchKernelGGL(k_correct_runs<unsigned long long>, dim3(wgs), dim3(WG), 0, s, text, R, pos, tq, (const unsigned long long *)cnt, bits,
                           (unsigned long long)n_words, (const unsigned long long *)geo, k, tables, n_tab, min_count, max_count, min_windows, text_out, out);
    return hipGetLastError() != hipSuccess;
}

}  // namespace pk
