// Sorted column chunks: the one LDS bitonic sort and the one binary search of the slide analytics.
//   cs_sort            in-place bitonic sort of npow2 keys in LDS (mapstats, gtalign through cs_sort_chunks; evalstats directly)
//   cs_sort_chunks     colsort.hip: every column of a strided table cut into chunks of CS_CHUNK rows, each sorted by one workgroup
//   cs_first_ge / _gt  lower and upper bound in a sorted range staged in LDS (the percentile's ranks, the distinct-value count)
//   cs_blocks          the grid cap of the grid-stride kernels
#pragma once
#include "sq_common.h"

constexpr int CS_CHUNK = 4096;            // keys of one sorted chunk: 16 KiB (f32) / 32 KiB (f64) of LDS
constexpr int CS_SORT_THREADS = 512;
constexpr int CS_MAX_BLOCKS = 1 << 20;    // grid-stride beyond

static_assert((CS_CHUNK & (CS_CHUNK - 1)) == 0 && CS_CHUNK * sizeof(double) <= 32768, "a chunk's keys fit the static LDS limit");

// key[0 .. npow2) ascending; npow2 a power of two, the keys ordered (no NaN), written and synchronised by the caller.  All
// THREADS threads of the workgroup call it; a thread takes one compare-exchange per pair index, and it returns behind a barrier.
template <typename T, int THREADS>
__device__ __forceinline__ void cs_sort(T* key, int npow2) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= npow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;      // i has bit j clear; i, l < npow2
                const T a = key[i], b = key[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { key[i] = b; key[l] = a; }
            }
            __syncthreads();
        }
}

// first key >= x of the sorted key[0 .. len)
template <typename T>
__device__ __forceinline__ int cs_first_ge(const T* key, int len, T x) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// first key > x of the sorted key[lo .. len), lo at or before it (cs_first_ge's answer for the same x)
template <typename T>
__device__ __forceinline__ int cs_first_gt(const T* key, int lo, int len, T x) {
    int hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

static inline unsigned cs_blocks(size_t items, int threads) {
    const size_t b = (items + (size_t)threads - 1) / (size_t)threads;
    return (unsigned)(b < (size_t)CS_MAX_BLOCKS ? b : (size_t)CS_MAX_BLOCKS);
}

static inline int cs_chunks(int n) { return (n + CS_CHUNK - 1) / CS_CHUNK; }

// Column c (cols ? cols[c] : c) of values [n, ld] (f32, or f64 when values_f64), chunk k: its min(CS_CHUNK, n - k CS_CHUNK) keys
// ascending at sorted[c * npad + k * CS_CHUNK], npad = cs_chunks(n) * CS_CHUNK.  A NaN is stored as +inf and sets nan_flag[c]
// (cleared here first).  valid, when not null, gets the chunk's count of numbers at [c * cs_chunks(n) + k]: its first
// len - #NaN keys (a real +inf is among them; which +inf is which does not matter to a count).
int cs_sort_chunks(const void* values, int values_f64, int n, int ld, const int32_t* cols, int C, void* sorted, int32_t* valid,
                   int32_t* nan_flag, hipStream_t st);
