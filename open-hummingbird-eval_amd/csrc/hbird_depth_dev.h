// What the two depth units share (hbird_depth.hip, hbird_depth_grid.hip): the validity test, K6's source index and bands on the cell grid,
// and the row pass of the summation rule.  One definition each, so that a grid call's slabs cannot drift from the single call's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

// every value here is specified step by step in fp32: no contraction, whichever unit includes this (both switch it off for themselves too)
#pragma clang fp contract(off)

__device__ __forceinline__ bool depth_valid(float v, float lo, float hi) { return __builtin_isfinite(v) && v >= lo && v <= hi; }

static inline const char* depth_bounds_error(float lo, float hi) {
    return (std::isfinite(lo) && std::isfinite(hi) && lo > 0.0f && lo <= hi) ? nullptr : "the bounds must be finite with 0 < min_depth <= max_depth";
}

// K6's source index and bands (hbird_post.hip), on the cell grid of side G = S r.
__host__ __device__ __forceinline__ int depth_src0(float scale, int dst, int G) {
    const float f = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    const int i = (int)floorf(f);
    return i < G - 1 ? i : G - 1;
}
// first output index whose upper source index is >= j (the source index is monotone: bands are contiguous)
__host__ __device__ __forceinline__ int depth_band_begin(float scale, int j, int G, int n) {
    if (j <= 0) return 0;
    if (j > G - 1) return n;
    int g = (int)(((float)j + 0.5f) / scale - 0.5f);
    g = g < 0 ? 0 : (g > n ? n : g);
    while (g > 0 && depth_src0(scale, g - 1, G) >= j) --g;
    while (g < n && depth_src0(scale, g, G) < j) ++g;
    return g;
}

#define DEPTH_ROWS 16      // output rows of a band per workgroup

// depth_row_sums_kernel (hbird_depth.hip) over `slabs` images' partials part[slabs][h][nb][HB_DEPTH_NSUMS] -> sums[slabs][HB_DEPTH_NSUMS]
int hb_launch_depth_row_sums(const double* part, int64_t slabs, int h, int nb, double* sums, hipStream_t s);
