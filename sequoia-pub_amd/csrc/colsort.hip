// The chunk sort of colsort.h: the first pass of the percentile of score (mapstats.hip) and of the distinct-value count
// (gtalign.hip).  Keys only, no index payload; keys keep the input's type and are compared as IEEE numbers, so -0.0 ties with
// 0.0 as it does in numpy.  A NaN is stored as +inf, as the pad keys of a short chunk are: the sort network only ever sees
// ordered keys, and pads sort behind or beside every real key.
#include "colsort.h"

namespace {

// grid (C, chunks): neighbouring blocks read neighbouring columns of the same rows (the table is row-major)
template <typename T>
__global__ __launch_bounds__(CS_SORT_THREADS) void cs_sort_chunks_kernel(const T* __restrict__ values, int n, int ld,
                                                                         const int32_t* __restrict__ cols, T* __restrict__ sorted, int npad,
                                                                         int32_t* __restrict__ valid, int32_t* __restrict__ nan_flag) {
    __shared__ T key[CS_CHUNK];
    __shared__ int n_nan;
    const int c = blockIdx.x, r0 = blockIdx.y * CS_CHUNK, tid = threadIdx.x;
    const int len = min(CS_CHUNK, n - r0);
    int npow2 = 1;
    while (npow2 < len) npow2 <<= 1;
    const size_t col = (size_t)(cols ? cols[c] : c);
    if (tid == 0) n_nan = 0;
    __syncthreads();                                          // stays: folded into the barrier behind the loads, one-chunk counts ran 2.5 % slower
    int mine = 0;
    for (int i = tid; i < npow2; i += CS_SORT_THREADS) {
        T v = (T)INFINITY;
        if (i < len) {
            v = values[(size_t)(r0 + i) * (size_t)ld + col];
            if (v != v) { ++mine; v = (T)INFINITY; }
        }
        key[i] = v;
    }
    if (mine) {
        atomicAdd(&n_nan, mine);                              // an integer counter in LDS
        nan_flag[c] = 1;                                      // every writer stores the same value
    }
    __syncthreads();
    cs_sort<T, CS_SORT_THREADS>(key, npow2);
    T* const dst = sorted + (size_t)c * (size_t)npad + (size_t)r0;
    for (int i = tid; i < len; i += CS_SORT_THREADS) dst[i] = key[i];
    if (valid && tid == 0) valid[(size_t)c * (size_t)gridDim.y + blockIdx.y] = len - n_nan;
}

template <typename T>
void cs_launch(const void* values, int n, int ld, const int32_t* cols, int C, void* sorted, int32_t* valid, int32_t* nan_flag, hipStream_t st) {
    const int chunks = cs_chunks(n);
    hipLaunchKernelGGL(cs_sort_chunks_kernel<T>, dim3((unsigned)C, (unsigned)chunks), dim3(CS_SORT_THREADS), 0, st, (const T*)values, n, ld, cols,
                       (T*)sorted, chunks * CS_CHUNK, valid, nan_flag);
}

}  // namespace

int cs_sort_chunks(const void* values, int values_f64, int n, int ld, const int32_t* cols, int C, void* sorted, int32_t* valid,
                   int32_t* nan_flag, hipStream_t st) {
    SQ_HIP_CHECK(hipMemsetAsync(nan_flag, 0, (size_t)C * sizeof(int32_t), st));
    if (values_f64) cs_launch<double>(values, n, ld, cols, C, sorted, valid, nan_flag, st);
    else cs_launch<float>(values, n, ld, cols, C, sorted, valid, nan_flag, st);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
