// wg_scan.h -- exclusive prefix scans over one workgroup of NW 64-wide waves: a __shfl_up ladder inside each wave, the
// wave totals through NW words of LDS (sh), and every thread folds the totals of the waves before its own.
//
// SH_BUSY is the one thing the callers differ in.  true: sh may still be read by an earlier call -- the scan sits in a
// loop, or follows another scan on the same words, with no barrier in between -- so a barrier goes in front of the store
// of the wave totals.  false: the caller knows that every reader of sh has passed a barrier since (or that there was
// none), and the scan costs one barrier.  Either way there is none behind the last read of sh.
// (k_query_count and k_query_lookup pass true on free words: their scans have always had the barrier, and it stays so that
// their code stays as it was.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pk {

// Sums (T: uint32_t or unsigned long long).  Returns the sum of v over the threads before this one; total: over all.
template <int NW, bool SH_BUSY, typename T>
__device__ __forceinline__ T wg_excl_sum(T v, T *sh, T &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (SH_BUSY) __syncthreads();
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    T pre = 0;
    total = 0;
    for (int i = 0; i < NW; i++) { if (i < w) pre += sh[i]; total += sh[i]; }
    return pre + inc - v;
}

// Any associative operator, commutative or not: compose(a, b) = a first, then b; shfl_up(v, d) = v of the lane d below.
// Returns seed . (the threads before this one), total = seed . (all of them); seed must be the same in every thread.
template <int NW, bool SH_BUSY, typename S, class Compose, class Shfl>
__device__ __forceinline__ S wg_excl_scan(const S &mine, const S &seed, S *sh, S &total, Compose compose, Shfl shfl_up) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    S inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        S o = shfl_up(inc, d);
        if (lane >= d) inc = compose(o, inc);
    }
    if (SH_BUSY) __syncthreads();
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    S pre = seed, tot = seed;
    for (int j = 0; j < NW; j++) { if (j == w) pre = tot; tot = compose(tot, sh[j]); }
    total = tot;
    S up = shfl_up(inc, 1);
    return lane == 0 ? pre : compose(pre, up);
}

}  // namespace pk
