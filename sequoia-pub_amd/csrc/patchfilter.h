// The arithmetic of get_mask_image (pre_processing/patch_gen_hdf5.py:25-38) shared by the per-tile patch filter
// (patchfilter.hip) and the whole-slide mask (slidemask.hip): saturation, numpy's histogram edges and bins, the integer and
// the float Otsu threshold, and the staging of misaligned uint8 pixels through LDS.  Every quantity is a chain of single
// IEEE double operations in numpy's order (include/sequoia_hip.h, "Patch filter"); nothing may be contracted into a fused
// multiply-add, so every function repeats `#pragma clang fp contract(off)` and the including files set it for themselves.
#pragma once
#include "sq_common.h"

constexpr int PF_CHUNK_PX = 4096;                                  // pixels staged at a time
constexpr int PF_STAGE_BYTES = 3 * PF_CHUNK_PX + 32;               // + skew (<= 15) + the tail of the last 16-byte line

// skimage rgb2hsv's saturation of one pixel: c = fl(u8 * (1 / 255.0)), delta = max - min, s = delta / max, 0 where delta == 0
__device__ __forceinline__ double pf_saturation(int r, int g, int b) {
#pragma clang fp contract(off)
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    if (mx == mn) return 0.0;                  // u8 -> c is strictly increasing: delta == 0 exactly when the bytes are equal
    const double k = 1.0 / 255.0;
    const double v = (double)mx * k, lo = (double)mn * k;
    return (v - lo) / v;
}

// np.linspace(s_min, s_max, 257)[i]
__device__ __forceinline__ double pf_edge(int i, double s_min, double s_max, double step) {
#pragma clang fp contract(off)
    const double e = (double)i * step;
    return i >= 256 ? s_max : e + s_min;
}

// np.histogram(s, 256, (s_min, s_max)): the bin with edge[i] <= s < edge[i + 1], the last one closed
__device__ __forceinline__ int pf_bin(double s, double s_min, double s_max, double step, double inv_step) {
#pragma clang fp contract(off)
    int i = (int)((s - s_min) * inv_step);
    i = min(max(i, 0), 255);
    while (i > 0 && s < pf_edge(i, s_min, s_max, step)) --i;
    while (i < 255 && s >= pf_edge(i + 1, s_min, s_max, step)) ++i;
    return i;
}

// skimage threshold_otsu of a uint8 channel from its 256 counts: bins lo..hi, centres the integers, first maximum.
// counts and counts * centre sum to integers below 2^53, so the backward sums are total - forward, exactly.
static __device__ int pf_otsu_u8(const uint32_t* cnt, int total) {
#pragma clang fp contract(off)
    int lo = 0, hi = 255;
    while (lo < 255 && cnt[lo] == 0) ++lo;
    while (hi > lo && cnt[hi] == 0) --hi;
    if (lo == hi) return lo;
    unsigned long long all_cs = 0;
    for (int i = lo; i <= hi; ++i) all_cs += (unsigned long long)cnt[i] * i;
    unsigned long long w1 = 0, cs1 = 0;
    double best = -1.0;
    int arg = lo;
    for (int i = lo; i < hi; ++i) {
        w1 += cnt[i];
        cs1 += (unsigned long long)cnt[i] * i;
        const double dw1 = (double)w1, dw2 = (double)((unsigned long long)total - w1);
        const double m1 = (double)cs1 / dw1, m2 = (double)(all_cs - cs1) / dw2;
        const double d = m1 - m2;
        const double var = (dw1 * dw2) * (d * d);
        if (var > best) best = var, arg = i;
    }
    return arg;
}

// threshold_otsu of the saturation from its 256 counts (one lane): centres (edge[i] + edge[i + 1]) / 2, cumulative sums of
// counts * centre in np.cumsum's order
static __device__ double pf_otsu_s(const uint32_t* cnt, int total, double s_min, double s_max, double* cs2) {
#pragma clang fp contract(off)
    const double step = (s_max - s_min) / 256.0;
    double acc = 0.0;
    for (int i = 255; i >= 0; --i) {
        const double c = (pf_edge(i, s_min, s_max, step) + pf_edge(i + 1, s_min, s_max, step)) / 2.0;
        const double t = (double)cnt[i] * c;
        acc = i == 255 ? t : acc + t;
        cs2[i] = acc;
    }
    unsigned long long w1 = 0;
    double best = -1.0;
    int arg = 0;
    acc = 0.0;
    for (int i = 0; i < 255; ++i) {
        const double c = (pf_edge(i, s_min, s_max, step) + pf_edge(i + 1, s_min, s_max, step)) / 2.0;
        const double t = (double)cnt[i] * c;
        acc = i == 0 ? t : acc + t;
        w1 += cnt[i];
        const double dw1 = (double)w1, dw2 = (double)((unsigned long long)total - w1);
        const double d = acc / dw1 - cs2[i + 1] / dw2;
        const double var = (dw1 * dw2) * (d * d);
        if (var > best) best = var, arg = i;
    }
    return (pf_edge(arg, s_min, s_max, step) + pf_edge(arg + 1, s_min, s_max, step)) / 2.0;
}

// pixel_bytes = 4 (RGBA, the fourth byte ignored): f(i, r, g, b) for the npx pixels at p0, which is 4-byte aligned, so a pixel
// is one dword and a wave's load 256 contiguous bytes: nothing to stage and no skew.  Thread t takes pixels t, t + THREADS,
// ...; four loads are issued before the first is used.  No barrier.
template <int THREADS, typename F>
__device__ __forceinline__ void pf_pixels4(const uint8_t* p0, int npx, F&& f) {
    const uint32_t* __restrict__ px = (const uint32_t*)p0;
    int i = threadIdx.x;
    for (; i + 3 * THREADS < npx; i += 4 * THREADS) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = px[i + u * THREADS];
#pragma unroll
        for (int u = 0; u < 4; ++u) f(i + u * THREADS, (int)(v[u] & 255u), (int)((v[u] >> 8) & 255u), (int)((v[u] >> 16) & 255u));
    }
    for (; i < npx; i += THREADS) {
        const uint32_t v = px[i];
        f(i, (int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u));
    }
}

// Stages the npx <= PF_CHUNK_PX 3-byte pixels at p0 (any alignment) in LDS with 16-byte loads aligned down; returns the skew: pixel
// i's bytes are stage[skew + 3 i ..].  [src, send) is the whole buffer: only the 16-byte lines at its two ends are read by
// the byte.  Every thread of the workgroup calls it; it ends with a barrier and begins with one (the previous chunk has
// been read).
template <int THREADS>
__device__ __forceinline__ int pf_stage(const uint8_t* src, const uint8_t* send, const uint8_t* p0, int npx, uint8_t* stage) {
    const uint8_t* const lo = (const uint8_t*)((uintptr_t)p0 & ~(uintptr_t)15);
    const int skew = (int)(p0 - lo);
    const int lines = (skew + npx * 3 + 15) >> 4;              // <= (15 + 12288 + 15) / 16 = 769 lines: 12304 <= PF_STAGE_BYTES
    __syncthreads();                                           // the previous chunk has been read
    for (int c = threadIdx.x; c < lines; c += THREADS) {
        const uint8_t* p = lo + (size_t)c * 16;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (p >= src && p + 16 <= send) {
            v = *(const u32x4*)p;
        } else {                                               // the 16-byte lines at either end of the whole buffer
            for (int b = 0; b < 16; ++b)
                if (p + b >= src && p + b < send) v[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
        }
        *(u32x4*)(stage + c * 16) = v;
    }
    __syncthreads();
    return skew;
}
