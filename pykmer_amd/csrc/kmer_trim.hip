// kmer_trim.hip -- the longest covered stretch of every read of a FASTQ feed.  A feed holds WHOLE records,
// cut by R + 1 non-decreasing offsets: record r is the bytes [starts[r], starts[r + 1]) of the feed's text.  No parser state
// runs here: the file has passed the FASTQ front end (fastq.hip) in the lookup pass, so a record is four lines, and a
// record that is not is still read inside its own bytes only -- every load below is guarded by the record's end.
// No reference counterpart (its README stops at the distance matrix).
//
// Two kernels around a scan, one wavefront per record in both (records grid-strided, WG / 64 per workgroup):
//   k_trim_count  finds the ends of lines 1-3 with ballots over 64-byte steps (the loads of four steps in flight at a time,
//                 here and below), walks line 2 for its leading blanks, its last non-blank byte and its valid bases -- a
//                 letter of ACGTacgt, unless a threshold is set and the byte at the same offset of line 4 lies below it
//                 (README "Base quality") -- and leaves the record's geometry
//   k_trim_scan   one workgroup, in place: the valid bases of the stream before every record (its first cover bit)
//   k_trim_runs   walks the positions of line 2 again, 64 a step: the cover bits of the step's valid bases (cover_select,
//                 kmer_pieces.h: the word seams are its business) deposited on their positions, and the longest run of set
//                 positions with a carry from step to step -- the run open at the step's end and the best so far, which a
//                 later run replaces only when it is strictly longer, so the smallest start wins a tie
// Positions are those of query.py --coords on the FASTA text the FASTQ stands for: a record's line 2 is its one sequence
// line, position 0 is its first non-blank byte, and every byte up to its last non-blank one holds a position.
// The guarded loads, the line search and the ballot of valid bases live in kmer_trim.h, which kmer_correct.hip shares; its
// walker runs behind k_trim_count and k_trim_scan (launch_trim_geometry).
#include "kmer_trim.h"
#include "wg_scan.h"

namespace pk {

constexpr int TRIM_SCAN_T = 1024;                // threads of the scan
constexpr int TRIM_SCAN_PER = 4;                 // consecutive records per thread and round

// Per record r of the feed (text[0 .. n) at stream offset pos): geo + f * R + r for the fields f below, and cnt[r] = its
// valid bases.  Stream offsets throughout.
//   0 pos2     the byte that holds position 0 of line 2 (the end of line 2's content when the line holds no position)
//   1 pos4     the byte at the same offset of line 4
//   2 end2     the end of line 2's content (where its terminator begins)
//   3 end4     the end of line 4's content: as long as line 2's, and inside the record
//   4 seq_len  the positions of the record
//   8 lead     the blanks of line 2 in front of position 0 (fields 5-7 are k_trim_runs')
__global__ __launch_bounds__(WG) void k_trim_count(const uint8_t *__restrict__ text, const unsigned long long *__restrict__ starts, uint64_t R,
                                                   uint64_t pos, uint32_t tq, unsigned long long *__restrict__ geo,
                                                   unsigned long long *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform: the record's offsets are scalar loads
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_WAVES + wave; r < R; r += (uint64_t)gridDim.x * TRIM_WAVES) {
        const uint64_t s = starts[r], e = starts[r + 1u];
        const uint64_t e1 = trim_line_end(text, s, e, lane), l2 = trim_next_line(text, e1, e);
        const uint64_t e2 = trim_line_end(text, l2, e, lane), l3 = trim_next_line(text, e2, e);
        const uint64_t e3 = trim_line_end(text, l3, e, lane), l4 = trim_next_line(text, e3, e);
        const uint64_t e4 = e - l4 < e2 - l2 ? e : l4 + (e2 - l2);
        uint64_t first = e2, last = e2, n_valid = 0;             // the first and the last non-blank byte of line 2
        for (uint64_t q = l2; q < e2; q += TRIM_ROUND) {
            uint32_t c[TRIM_STEPS], qv[TRIM_STEPS];
            trim_load(text, q, e2, lane, 32u, c);                // behind the line: blanks, which are neither ink nor bases
            trim_load_qual(text, q, e2, l4 + (q - l2), e4, lane, tq, qv);
#pragma unroll
            for (int j = 0; j < TRIM_STEPS; j++) {
                const uint64_t at = q + 64u * (uint32_t)j;
                const unsigned long long ink = __ballot(!is_ws(c[j]));
                if (ink) {
                    if (first == e2) first = at + (uint64_t)__builtin_ctzll(ink);
                    last = at + 63u - (uint64_t)__builtin_clzll(ink);
                }
                n_valid += (uint64_t)__popcll(trim_valid(c[j], qv[j], tq));
            }
        }
        const uint64_t lead = first - l2, seq_len = first == e2 ? 0u : last + 1u - first;
        if (lane == 0u) {
            geo[r] = pos + first;
            geo[R + r] = pos + (e4 - l4 < lead ? e4 : l4 + lead);
            geo[2u * R + r] = pos + e2;
            geo[3u * R + r] = pos + e4;
            geo[4u * R + r] = seq_len;
            geo[8u * R + r] = lead;
            cnt[r] = n_valid;
        }
    }
}

// cnt[0 .. R): counts -> base + their exclusive prefix sums, in place; *total = base + all of them
__global__ __launch_bounds__(TRIM_SCAN_T) void k_trim_scan(unsigned long long *__restrict__ cnt, uint64_t R, unsigned long long base,
                                                           unsigned long long *__restrict__ total) {
    __shared__ unsigned long long wsum[TRIM_SCAN_T / 64];
    unsigned long long run = base;
    for (uint64_t b0 = 0; b0 < R; b0 += (uint64_t)TRIM_SCAN_T * TRIM_SCAN_PER) {
        const uint64_t b = b0 + (uint64_t)threadIdx.x * TRIM_SCAN_PER;
        unsigned long long v[TRIM_SCAN_PER], mine = 0;
#pragma unroll
        for (int j = 0; j < TRIM_SCAN_PER; j++) { v[j] = b + j < R ? cnt[b + j] : 0ull; mine += v[j]; }
        unsigned long long sum;
        unsigned long long pre = run + wg_excl_sum<TRIM_SCAN_T / 64, true>(mine, wsum, sum);
#pragma unroll
        for (int j = 0; j < TRIM_SCAN_PER; j++) { if (b + j < R) cnt[b + j] = pre; pre += v[j]; }
        run += sum;
    }
    if (threadIdx.x == 0) *total = run;
}

// Per record r: geo fields 5 trim_start, 6 trim_end (half-open positions of the longest run of covered positions, the
// smallest start among equals; 0, 0 without a covered base) and 7 covered (the covered bases of all its runs).  first[r]:
// the stream's valid bases before the record, which is the ordinal of its first cover bit.
__global__ __launch_bounds__(WG) void k_trim_runs(const uint8_t *__restrict__ text, uint64_t R, uint64_t pos, uint32_t tq,
                                                  const unsigned long long *__restrict__ first, const uint32_t *__restrict__ bits,
                                                  unsigned long long n_words, unsigned long long *__restrict__ geo) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform: the record's offsets are scalar loads
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_WAVES + wave; r < R; r += (uint64_t)gridDim.x * TRIM_WAVES) {
        const uint64_t p2 = geo[r] - pos, p4 = geo[R + r] - pos, e4 = geo[3u * R + r] - pos, n = geo[4u * R + r];
        unsigned long long g = first[r];
        uint64_t best_s = 0, best_l = 0, cur_s = 0, cur_l = 0, covered = 0;
        for (uint64_t q0 = 0; q0 < n; q0 += TRIM_ROUND) {
            uint32_t c[TRIM_STEPS], qv[TRIM_STEPS];
            trim_load(text, p2 + q0, p2 + n, lane, 32u, c);
            trim_load_qual(text, p2 + q0, p2 + n, p4 + q0, e4, lane, tq, qv);
#pragma unroll
            for (int j = 0; j < TRIM_STEPS; j++) {
                const uint64_t q = q0 + 64u * (uint32_t)j;       // the position of the step's first byte
                const unsigned long long V = trim_valid(c[j], qv[j], tq);
                const unsigned long long C = V ? cover_select(V, g, bits, n_words, false) : 0ull;
                g += (unsigned long long)__popcll(V);
                covered += (uint64_t)__popcll(C);
                if (!(C & 1ull)) cur_l = 0;                      // the run open at the step's start ends there
                unsigned long long rest = C;
                while (rest) {                                   // run by run, lowest first
                    const uint32_t at = (uint32_t)__builtin_ctzll(rest);
                    const unsigned long long above = ~(rest >> at);
                    const uint32_t len = above ? (uint32_t)__builtin_ctzll(above) : 64u;
                    if (at == 0u && cur_l) cur_l += len;
                    else { cur_s = q + at; cur_l = len; }
                    if (cur_l > best_l) { best_l = cur_l; best_s = cur_s; }
                    if (at + len >= 64u) break;                  // open at the step's end: the next step goes on with it
                    cur_l = 0;
                    rest &= ~(((1ull << len) - 1ull) << at);
                }
            }
        }
        if (lane == 0u) {
            geo[5u * R + r] = best_s;
            geo[6u * R + r] = best_s + best_l;
            geo[7u * R + r] = covered;
        }
    }
}

static uint32_t trim_workgroups(uint64_t R) {
    const uint64_t want = (R + TRIM_WAVES - 1u) / TRIM_WAVES;
    return (uint32_t)(want < TRIM_MAX_WGS ? want : TRIM_MAX_WGS);
}

void launch_trim_geometry(const uint8_t *text, const unsigned long long *starts, uint64_t R, uint64_t pos, uint32_t tq, unsigned long long base,
                          unsigned long long *cnt, unsigned long long *total, unsigned long long *geo, hipStream_t s) {
    hipLaunchKernelGGL(k_trim_count, dim3(trim_workgroups(R)), dim3(WG), 0, s, text, starts, R, pos, tq, geo, cnt);
    hipLaunchKernelGGL(k_trim_scan, dim3(1), dim3(TRIM_SCAN_T), 0, s, cnt, R, base, total);
}

int launch_trim(const uint8_t *text, const unsigned long long *starts, uint64_t R, uint64_t pos, uint32_t tq, const uint32_t *bits,
                uint64_t n_words, unsigned long long base, unsigned long long *cnt, unsigned long long *total, unsigned long long *geo,
                hipStream_t s) {
    if (!R) return 0;
    launch_trim_geometry(text, starts, R, pos, tq, base, cnt, total, geo, s);
    hipLaunchKernelGGL(k_trim_runs, dim3(trim_workgroups(R)), dim3(WG), 0, s, text, R, pos, tq, (const unsigned long long *)cnt, bits,
                       (unsigned long long)n_words, geo);
    return hipGetLastError() != hipSuccess;
}

}  // namespace pk
