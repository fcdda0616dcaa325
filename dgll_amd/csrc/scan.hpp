// scan.hpp -- the one-workgroup exclusive scan of the samplers (subgraph.hip; neighbor.hip and edge_pred.hip still carry copies of
// their own).  A launch of ONE workgroup of kBlock threads: thread t owns the contiguous chunk [t * ceil(n / kBlock), ...) of the n
// items, sums it, thread 0 turns the kBlock chunk sums into chunk offsets (serial: 256 adds), and every thread walks its chunk
// again with its offset.  Integer sums in a fixed order: the same bits every run.  n items cost each thread 2 * ceil(n / kBlock)
// reads, strided by the chunk, which is what bounds it: use it for row pointers and bitmap words, not for entries.
#pragma once
#include "common.hpp"

namespace dgll {

// get(i) -> the int64 value of item i; put(i, below, x) receives item i, the sum of the items before it and its own value.
// Returns the total to every thread.  Every thread of the workgroup must call it (two barriers inside).
template <typename Get, typename Put>
__device__ __forceinline__ int64_t workgroup_scan(int64_t n, Get get, Put put) {
    __shared__ int64_t part[kBlock + 1];
    const int t = threadIdx.x;
    const int64_t chunk = (n + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += get(i);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int j = 0; j < kBlock; ++j) { const int64_t x = part[j]; part[j] = run; run += x; }
        part[kBlock] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) { const int64_t x = get(i); put(i, run, x); run += x; }
    return part[kBlock];
}

// counts[1 .. n] hold one count per row: in place to row pointers (counts[0] = 0, counts[i + 1] = rows 0 .. i); the total to *total
__device__ __forceinline__ void scan_counts_to_rowptr(int64_t* __restrict__ counts, int64_t n, int64_t* __restrict__ total) {
    const int64_t sum = workgroup_scan(n, [&](int64_t i) { return counts[i + 1]; },
                                       [&](int64_t i, int64_t below, int64_t x) { counts[i + 1] = below + x; });
    if (threadIdx.x == 0) { counts[0] = 0; *total = sum; }
}

// prefix[w] = set bits in the words before w; their total to *total
__device__ __forceinline__ void scan_bitmap_words(const uint32_t* __restrict__ bitmap, int64_t n_words, int32_t* __restrict__ prefix,
                                                  int64_t* __restrict__ total) {
    const int64_t sum = workgroup_scan(n_words, [&](int64_t w) { return (int64_t)__popc(bitmap[w]); },
                                       [&](int64_t w, int64_t below, int64_t) { prefix[w] = (int32_t)below; });
    if (threadIdx.x == 0) *total = sum;
}

}  // namespace dgll
