// kmer_trim.h -- what the per-record walkers over feeds of whole FASTQ records share (kmer_trim.hip, kmer_correct.hip): one
// wavefront per record, 64-byte steps with the loads of TRIM_STEPS steps in flight, every load guarded by the end of the
// range it belongs to, and the valid bases of a step as a ballot.
#pragma once
#include "kmer_pieces.h"

namespace pk {

constexpr int TRIM_WAVES = WG / 64;              // records per workgroup and round
constexpr uint32_t TRIM_MAX_WGS = 8192;
constexpr int TRIM_STEPS = 4;                    // 64-byte steps whose loads are in flight together: the walks wait for memory, not for arithmetic
constexpr uint32_t TRIM_ROUND = 64u * TRIM_STEPS;

// TRIM_STEPS steps of text[q ..) below `end`, one byte per lane and step; a byte the range does not have reads as `fill`
__device__ __forceinline__ void trim_load(const uint8_t *__restrict__ text, uint64_t q, uint64_t end, uint32_t lane, uint32_t fill,
                                          uint32_t (&c)[TRIM_STEPS]) {
#pragma unroll
    for (int j = 0; j < TRIM_STEPS; j++) {
        const uint64_t i = q + 64u * (uint32_t)j + lane;
        c[j] = i < end ? (uint32_t)text[i] : fill;
    }
}

// the first line terminator of text[from, end), or end.  The whole wave calls it; the answer is uniform.
__device__ __forceinline__ uint64_t trim_line_end(const uint8_t *__restrict__ text, uint64_t from, uint64_t end, uint32_t lane) {
    for (uint64_t q = from; q < end; q += TRIM_ROUND) {
        uint32_t c[TRIM_STEPS];
        trim_load(text, q, end, lane, 0u, c);
#pragma unroll
        for (int j = 0; j < TRIM_STEPS; j++) {
            const unsigned long long m = __ballot(is_term(c[j]));
            if (m) return q + 64u * (uint32_t)j + (uint64_t)__builtin_ctzll(m);
        }
    }
    return end;
}

// where the line behind the terminator at `at` begins: \n, \r\n and a lone \r end a line (at == end: no terminator, no line)
__device__ __forceinline__ uint64_t trim_next_line(const uint8_t *__restrict__ text, uint64_t at, uint64_t end) {
    if (at >= end) return end;
    return at + ((text[at] == 13u && at + 1u < end && text[at + 1u] == 10u) ? 2u : 1u);
}

// The bytes of line 4 at the offsets of the TRIM_STEPS steps of line 2 at i2 (line 2 ends at e2; i4: the offset of line 4 that
// goes with i2, line 4 ends at e4).  Without a threshold nothing is loaded; a byte that line 4 does not have passes none.
__device__ __forceinline__ void trim_load_qual(const uint8_t *__restrict__ text, uint64_t i2, uint64_t e2, uint64_t i4, uint64_t e4, uint32_t lane,
                                               uint32_t tq, uint32_t (&qv)[TRIM_STEPS]) {
#pragma unroll
    for (int j = 0; j < TRIM_STEPS; j++) {
        const uint64_t d = 64u * (uint32_t)j + lane;
        qv[j] = (tq && i2 + d < e2 && i4 + d < e4) ? (uint32_t)text[i4 + d] : 0u;
    }
}
// the valid bases of one step: bit = lane.  c: the byte of line 2 (a blank where the line has none), qv: that of line 4.
__device__ __forceinline__ unsigned long long trim_valid(uint32_t c, uint32_t qv, uint32_t tq) {
    return __ballot(base_code(c) < 4u && (!tq || qv >= tq));
}

}  // namespace pk
