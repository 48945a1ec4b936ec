// Depth estimation by retrieval (include/hbird_hip_depth.h): depth maps -> patch label rows for the bank (depth_targets), aggregated rows ->
// depth map + deterministic per-image error sums (depth_upsample_metrics, depth_row_sums).  Plain VALU, memory-bound; no MFMA.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include "hbird_depth_dev.h"
#include <algorithm>
#include <cmath>

// Every value below is specified step by step (the cell sums, K6's interpolation, the float64 terms), so contraction into FMAs is switched
// off for this file, as in hbird_post.hip.
#pragma clang fp contract(off)

// One wave per patch, four patches per workgroup.  The wave's lanes walk the patch's pixels row by row (runs of ps neighbouring floats) into
// LDS and vote on "any pixel valid"; then lane = cell adds its s x s pixels from LDS in row-major order -- the stated chain, whatever r is.
__global__ __launch_bounds__(256) void depth_targets_kernel(const float* __restrict__ y, int64_t n_patches, int H, int W, int ps, int r,
                                                            float lo, float hi, float* __restrict__ rows, int* __restrict__ nonempty) {
    extern __shared__ __attribute__((aligned(16))) float dt_sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * 4 + wv;
    if (p >= n_patches) return;                             // wave-uniform; no workgroup barrier below
    const int P = ps * ps, Sw = W / ps, Sh = H / ps;
    float* px = dt_sm + wv * P;
    const int64_t b = p / ((int64_t)Sh * Sw);
    const int pi = (int)((p / Sw) % Sh), pj = (int)(p % Sw);
    const float* base = y + (b * H + (int64_t)pi * ps) * W + (int64_t)pj * ps;
    bool any = false;
    for (int e = lane; e < P; e += 64) {
        const int u = e / ps, v = e - u * ps;
        const float d = base[(int64_t)u * W + v];
        px[e] = d;
        any = any || depth_valid(d, lo, hi);
    }
    const bool some = __ballot(any) != 0ull;
    if (lane == 0) nonempty[p] = some ? 1 : 0;
    __builtin_amdgcn_s_waitcnt(0xc07f);                     // lgkmcnt(0): the wave's own LDS writes are visible to all its lanes
    const int s = ps / r, cells = r * r;
    const float area = (float)(s * s);
    float* o = rows + p * (int64_t)(2 * cells);
    for (int c = lane; c < cells; c += 64) {
        const int cy = c / r, cx = c - cy * r;
        const float* cp = px + (cy * s) * ps + cx * s;
        float sum = 0.0f;
        int cnt = 0;
        for (int u = 0; u < s; ++u)
            for (int v = 0; v < s; ++v) {
                const float d = cp[u * ps + v];
                if (depth_valid(d, lo, hi)) { sum = sum + d; ++cnt; }
            }
        o[c] = sum / area;
        o[cells + c] = (float)cnt / area;
    }
}

extern "C" int hb_patch_depth_targets(const float* y, int64_t B, int H, int W, int ps, int r, float min_depth, float max_depth, float* rows_out,
                                      int* nonempty_out, void* stream) {
    const std::string who = "hb_patch_depth_targets: ";
    if (B < 0) return hb_fail(who + "B is negative");
    if (H <= 0 || W <= 0) return hb_fail(who + "H and W must be positive");
    if (ps <= 0 || ps > HB_DEPTH_MAX_PS) return hb_fail(who + "the patch size must be in [1, " + std::to_string(HB_DEPTH_MAX_PS) + "]");
    if (H % ps || W % ps) return hb_fail(who + "H and W must be multiples of the patch size");
    if (r <= 0 || ps % r) return hb_fail(who + "target_grid must be positive and divide the patch size");
    if (const char* why = depth_bounds_error(min_depth, max_depth)) return hb_fail(who + why);
    if (B == 0) return 0;
    if (!y || !rows_out || !nonempty_out) return hb_fail(who + "NULL pointer");
    const int64_t np = B * (H / ps) * (W / ps);
    if ((np + 3) / 4 > 0x7FFFFFFFLL) return hb_fail(who + "too many patches per call");
    depth_targets_kernel<<<dim3((unsigned)((np + 3) / 4)), dim3(256), (size_t)4 * ps * ps * sizeof(float), (hipStream_t)stream>>>(
        y, np, H, W, ps, r, min_depth, max_depth, rows_out, nonempty_out);
    HB_HIP(hipGetLastError());
    return 0;
}

// ---- prediction and sums ---------------------------------------------------------------------------------------------------------------
// (K6's source index and bands on the cell grid, and DEPTH_ROWS: hbird_depth_dev.h)
// One workgroup = (image, band j, chunk of <= DEPTH_ROWS rows of the band, one column chunk of the summation rule).  It stages the columns
// it needs of the source cell rows j and j + 1 of both grids in LDS ([4][ncols]); one lane per output column forms top / bot of N and Dn once
// and walks the chunk's rows.  A row's 11 float64 terms meet by the rule of the header: butterfly inside the wave, the waves in order; the
// chunk's partial goes to part[b][row][chunk][.] and depth_row_sums_kernel adds chunks and rows in order.
__global__ __launch_bounds__(256) void depth_upsample_metrics_kernel(const float* __restrict__ agg, int S, int r, int h, int w, float sy, float sx,
                                                                     int chunks, int ncols_max, const float* __restrict__ gt, float lo, float hi,
                                                                     double* __restrict__ part, float* __restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) float du_sm[];
    __shared__ double wave_part[4][HB_DEPTH_NSUMS];
    const int G = S * r, cells = r * r, C2 = 2 * cells;
    const int j = blockIdx.y / chunks, rc = blockIdx.y % chunks;
    const int64_t b = blockIdx.z;
    const int r0 = depth_band_begin(sy, j, G, h) + rc * DEPTH_ROWS;
    const int r1 = min(depth_band_begin(sy, j + 1, G, h), r0 + DEPTH_ROWS);
    if (r0 >= r1) return;                                   // block-uniform
    const int bw = blockDim.x, nw = bw >> 6, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xs = blockIdx.x * bw, xe = min(w, xs + bw) - 1;
    const int cx_lo = depth_src0(sx, xs, G), cx_hi = min(depth_src0(sx, xe, G) + 1, G - 1);
    const int ncols = min(cx_hi - cx_lo + 1, ncols_max);    // (== cx_hi - cx_lo + 1: the host sized ncols_max with the same arithmetic)
    const int j1 = min(j + 1, G - 1);
    // stage [N row j][N row j1][D row j][D row j1], ncols_max floats apart
    const float* base = agg + b * (int64_t)S * S * C2;
    for (int e = threadIdx.x; e < 2 * ncols; e += bw) {
        const int row = e >= ncols, col = e - row * ncols;
        const int gy = row ? j1 : j, gx = cx_lo + col;
        const float* cell = base + ((int64_t)(gy / r) * S + gx / r) * C2 + (gy % r) * r + gx % r;
        du_sm[row * ncols_max + col] = cell[0];
        du_sm[(2 + row) * ncols_max + col] = cell[cells];
    }
    __syncthreads();
    const bool live = xs + (int)threadIdx.x < w;
    const int x = min(xs + (int)threadIdx.x, w - 1);        // lanes past the right border repeat the last column (no store, zero terms)
    const float fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.0f);
    const int x0 = min((int)floorf(fx), G - 1), x1 = min(x0 + 1, G - 1);
    const float lx1 = fx - (float)x0, lx0 = 1.0f - lx1;
    const int a0 = min(max(x0 - cx_lo, 0), ncols_max - 1), a1 = min(max(x1 - cx_lo, 0), ncols_max - 1);   // (in range by construction; clamped all the same)
    const float topN = lx0 * du_sm[a0] + lx1 * du_sm[a1];
    const float botN = lx0 * du_sm[ncols_max + a0] + lx1 * du_sm[ncols_max + a1];
    const float topD = lx0 * du_sm[2 * ncols_max + a0] + lx1 * du_sm[2 * ncols_max + a1];
    const float botD = lx0 * du_sm[3 * ncols_max + a0] + lx1 * du_sm[3 * ncols_max + a1];
    for (int yy = r0; yy < r1; ++yy) {                      // block-uniform trip count
        const float fy = fmaxf(sy * ((float)yy + 0.5f) - 0.5f, 0.0f);
        const float ly1 = fy - (float)j, ly0 = 1.0f - ly1;   // j = min(floor(fy), G - 1) for every row of the band
        const float N = ly0 * topN + ly1 * botN;
        const float Dn = ly0 * topD + ly1 * botD;
        const bool has = Dn > 0.0f;
        const float pv = has ? fminf(fmaxf(N / Dn, lo), hi) : __builtin_nanf("");
        const int64_t at = (b * h + yy) * (int64_t)w + x;
        if (pred && live) pred[at] = pv;
        double t[HB_DEPTH_NSUMS];
#pragma unroll
        for (int i = 0; i < HB_DEPTH_NSUMS; ++i) t[i] = 0.0;
        const float gv = live ? gt[at] : 0.0f;
        if (live && depth_valid(gv, lo, hi)) {
            if (!has) t[HB_DEPTH_SUM_NOPRED] = 1.0;
            else {
                const double p = (double)pv, g = (double)gv, d = p - g, d2 = d * d;
                const double dl = log(p) - log(g);
                const double ratio = fmax(p / g, g / p);
                t[HB_DEPTH_SUM_N] = 1.0;
                t[HB_DEPTH_SUM_SQ] = d2;
                t[HB_DEPTH_SUM_ABS_REL] = fabs(d) / g;
                t[HB_DEPTH_SUM_SQ_REL] = d2 / g;
                t[HB_DEPTH_SUM_LOG_SQ] = dl * dl;
                t[HB_DEPTH_SUM_LOG] = dl;
                t[HB_DEPTH_SUM_LOG10] = fabs(log10(p) - log10(g));
                t[HB_DEPTH_SUM_D1] = ratio < 1.25 ? 1.0 : 0.0;
                t[HB_DEPTH_SUM_D2] = ratio < 1.5625 ? 1.0 : 0.0;
                t[HB_DEPTH_SUM_D3] = ratio < 1.953125 ? 1.0 : 0.0;
            }
        }
#pragma unroll
        for (int i = 0; i < HB_DEPTH_NSUMS; ++i) {
            double v = t[i];
            for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
            if (lane == 0) wave_part[wv][i] = v;
        }
        __syncthreads();
        if (threadIdx.x < HB_DEPTH_NSUMS) {
            double v = wave_part[0][threadIdx.x];
            for (int k = 1; k < nw; ++k) v = v + wave_part[k][threadIdx.x];
            part[(((b * h + yy) * (int64_t)gridDim.x) + blockIdx.x) * HB_DEPTH_NSUMS + threadIdx.x] = v;
        }
        __syncthreads();
    }
}

#define DEPTH_TILE 2048    // partials per LDS tile of the row pass (16 KiB)
// One workgroup per image: the partials of part[b] ([h][nb][11], i.e. rows ascending, chunks ascending) come through LDS in tiles of whole
// (row, chunk) entries; thread i < 11 adds its term: the row's chunks from 0.0 in order, then acc = acc + row.
__global__ __launch_bounds__(256) void depth_row_sums_kernel(const double* __restrict__ part, int h, int nb, double* __restrict__ sums) {
    __shared__ double tile[DEPTH_TILE];
    const int64_t b = blockIdx.x;
    const double* pb = part + b * (int64_t)h * nb * HB_DEPTH_NSUMS;
    const int64_t entries = (int64_t)h * nb;
    const int per_tile = DEPTH_TILE / HB_DEPTH_NSUMS;
    double acc = 0.0, row = 0.0;
    int chunk = 0;                                          // position of the next entry within its row
    for (int64_t e0 = 0; e0 < entries; e0 += per_tile) {
        const int n = (int)min((int64_t)per_tile, entries - e0);
        if (e0) __syncthreads();
        for (int e = threadIdx.x; e < n * HB_DEPTH_NSUMS; e += 256) tile[e] = pb[e0 * HB_DEPTH_NSUMS + e];
        __syncthreads();
        if (threadIdx.x < HB_DEPTH_NSUMS)
            for (int e = 0; e < n; ++e) {
                row = row + tile[e * HB_DEPTH_NSUMS + threadIdx.x];
                if (++chunk == nb) { acc = acc + row; row = 0.0; chunk = 0; }
            }
    }
    if (threadIdx.x < HB_DEPTH_NSUMS) sums[b * HB_DEPTH_NSUMS + threadIdx.x] = acc;
}

// the row pass for another unit's partials (hbird_depth_grid.hip: one slab per configuration and image)
int hb_launch_depth_row_sums(const double* part, int64_t slabs, int h, int nb, double* sums, hipStream_t s) {
    if (slabs < 1 || slabs > 0x7FFFFFFFLL) return hb_fail("hb_launch_depth_row_sums: bad slab count");
    depth_row_sums_kernel<<<dim3((unsigned)slabs), dim3(256), 0, s>>>(part, h, nb, sums);
    HB_HIP(hipGetLastError());
    return 0;
}

extern "C" int hb_depth_upsample_metrics(const float* agg, int64_t B, int S, int r, int h, int w, const float* gt, float min_depth, float max_depth,
                                         double* sums_out, float* pred_out_opt, void* stream) {
    const std::string who = "hb_depth_upsample_metrics: ";
    if (B < 0) return hb_fail(who + "B is negative");
    if (S <= 0 || r <= 0 || h <= 0 || w <= 0) return hb_fail(who + "S, target_grid, h and w must be positive");
    if ((long long)S * r > HB_DEPTH_MAX_GRID) return hb_fail(who + "the cell grid's side S * target_grid exceeds " + std::to_string(HB_DEPTH_MAX_GRID));
    if (const char* why = depth_bounds_error(min_depth, max_depth)) return hb_fail(who + why);
    if (B == 0) return 0;
    if (!agg || !gt || !sums_out) return hb_fail(who + "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int G = S * r;
    const float sy = (float)G / (float)h, sx = (float)G / (float)w;
    // the column chunks of the summation rule: whole groups of 64 columns, dealt evenly to chunks of at most four
    const int w64 = (w + 63) / 64, nb = (w64 + 3) / 4, bw = (w64 + nb - 1) / nb * 64;
    // tallest band, widest column window (the kernel's own fp32 arithmetic: contraction is off on both sides)
    int maxband = 1, run = 0, prev = -1;
    for (int yy = 0; yy < h; ++yy) {
        const int y0 = depth_src0(sy, yy, G);
        run = y0 == prev ? run + 1 : 1;
        prev = y0;
        maxband = std::max(maxband, run);
    }
    int ncols_max = 1;
    for (int bx = 0; bx < nb; ++bx) {
        const int xs = bx * bw, xe = std::min(w, xs + bw) - 1;
        ncols_max = std::max(ncols_max, std::min(depth_src0(sx, xe, G) + 1, G - 1) - depth_src0(sx, xs, G) + 1);
    }
    const int chunks = (maxband + DEPTH_ROWS - 1) / DEPTH_ROWS;
    if ((long long)G * chunks > 65535 || B > 65535) return hb_fail(who + "grid too large");
    hb_dev<double> part;                                    // [B][h][nb][HB_DEPTH_NSUMS]; every entry is written by exactly one workgroup
    const size_t part_bytes = (size_t)B * h * nb * HB_DEPTH_NSUMS * sizeof(double);
    if (part.ensure(part_bytes, HB_GROW_EXACT)) return -1;
    HB_HIP(hipMemsetAsync(part, 0, part_bytes, s));
    depth_upsample_metrics_kernel<<<dim3((unsigned)nb, (unsigned)(G * chunks), (unsigned)B), dim3(bw), (size_t)4 * ncols_max * sizeof(float), s>>>(
        agg, S, r, h, w, sy, sx, chunks, ncols_max, gt, min_depth, max_depth, part, pred_out_opt);
    HB_HIP(hipGetLastError());
    depth_row_sums_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(part, h, nb, sums_out);
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(s));                        // the partials are a local of this call
    return 0;
}
