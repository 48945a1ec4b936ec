// Depth grids (include/hbird_hip_depth_grid.h, DESIGN.md section 4 "Depth grids"): the aggregated rows of up to 16 (k, beta) configurations ->
// every configuration's depth map and deterministic per-image error sums out of one launch (depth_grid_metrics_kernel, then the row pass of
// hbird_depth.hip over n_cfg x B slabs), and the resampling reduction of the paired bootstrap over float64 per-image sums
// (bootstrap_weighted_sums_kernel).  Plain VALU; no MFMA, no atomic.
#include "../../include/hbird_hip.h"
#include "../../include/hbird_hip_bootstrap.h"
#include "../../include/hbird_hip_depth_grid.h"
#include "hbird_internal.h"
#include "hbird_depth_dev.h"
#include <algorithm>
#include <cmath>

// Slab c of the grid entry has the bits of hb_depth_upsample_metrics (hbird_depth.hip) and the weighted sums are a stated chain of rounded
// products and adds: contraction into FMAs is switched off for this file, as there.
#pragma clang fp contract(off)

static_assert(HB_DEPTH_GRID_MAX_CONFIGS == HB_GRID_MAX_CONFIGS, "a depth grid call takes what one aggregation launch writes");

#define DG_LDS_BYTES 65536         // a workgroup's whole LDS: the staged source rows and the wave partials of one group of configurations

// depth_upsample_metrics_kernel's workgroup -- (image, band j, chunk of <= DEPTH_ROWS rows of the band, one column chunk of the summation
// rule) -- for EVERY configuration.  LDS: [wave_part: cpg x waves x 11 float64][stage: cpg x [N row j][N row j1][D row j][D row j1], ncols_max
// floats apart], cpg = the configurations whose staged rows fit together (all of them unless the column window is very wide; then the groups
// are re-staged one after the other).  The band, the lane's x taps and weights are formed once.  Per output row the lane reads its
// ground-truth pixel, tests it and takes its two float64 logarithms once, then walks the group's configurations: top / bot of N and Dn from
// the stage (the single kernel's operations in its order -- it forms them once per band, which gives the same floats), the prediction, the 11
// float64 terms, which meet by the rule of hbird_hip_depth.h: butterfly inside the wave, then the waves in order behind ONE pair of barriers
// per row for the whole group.  The chunk's partial goes to part[c][b][row][chunk][.]; the row pass adds chunks and rows in order.
__global__ __launch_bounds__(256) void depth_grid_metrics_kernel(const float* __restrict__ agg, int n_cfg, int cpg, int64_t B, int S, int r, int h, int w,
                                                                 float sy, float sx, int chunks, int ncols_max, const float* __restrict__ gt,
                                                                 float lo, float hi, double* __restrict__ part, float* __restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) double dg_sm[];
    const int G = S * r, cells = r * r, C2 = 2 * cells;
    const int j = blockIdx.y / chunks, rc = blockIdx.y % chunks;
    const int64_t b = blockIdx.z;
    const int r0 = depth_band_begin(sy, j, G, h) + rc * DEPTH_ROWS;
    const int r1 = min(depth_band_begin(sy, j + 1, G, h), r0 + DEPTH_ROWS);
    if (r0 >= r1) return;                                   // block-uniform
    const int bw = blockDim.x, nw = bw >> 6, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* wave_part = dg_sm;                                                         // [cpg][nw][HB_DEPTH_NSUMS]
    float* stage = reinterpret_cast<float*>(wave_part + cpg * nw * HB_DEPTH_NSUMS);    // [cpg][4][ncols_max]
    const int xs = blockIdx.x * bw, xe = min(w, xs + bw) - 1;
    const int cx_lo = depth_src0(sx, xs, G), cx_hi = min(depth_src0(sx, xe, G) + 1, G - 1);
    const int ncols = min(cx_hi - cx_lo + 1, ncols_max);    // (== cx_hi - cx_lo + 1: the host sized ncols_max with the same arithmetic)
    const int j1 = min(j + 1, G - 1);
    const bool live = xs + (int)threadIdx.x < w;
    const int x = min(xs + (int)threadIdx.x, w - 1);        // lanes past the right border repeat the last column (no store, zero terms)
    const float fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.0f);
    const int x0 = min((int)floorf(fx), G - 1), x1 = min(x0 + 1, G - 1);
    const float lx1 = fx - (float)x0, lx0 = 1.0f - lx1;
    const int a0 = min(max(x0 - cx_lo, 0), ncols_max - 1), a1 = min(max(x1 - cx_lo, 0), ncols_max - 1);   // (in range by construction; clamped all the same)
    const int64_t img = (int64_t)S * S * C2, hw = (int64_t)h * w;      // floats of one image's aggregated rows / of one map
    for (int c0 = 0; c0 < n_cfg; c0 += cpg) {               // block-uniform; one trip unless the stage is re-used
        const int nc = min(cpg, n_cfg - c0);
        for (int e = threadIdx.x; e < nc * 2 * ncols; e += bw) {        // (the previous group's last row ended in a barrier)
            const int cc = e / (2 * ncols), rem = e - cc * 2 * ncols;
            const int row = rem >= ncols, col = rem - row * ncols;
            const int gy = row ? j1 : j, gx = cx_lo + col;
            const float* cell = agg + ((int64_t)(c0 + cc) * B + b) * img + ((int64_t)(gy / r) * S + gx / r) * C2 + (gy % r) * r + gx % r;
            float* st = stage + cc * 4 * ncols_max;
            st[row * ncols_max + col] = cell[0];
            st[(2 + row) * ncols_max + col] = cell[cells];
        }
        __syncthreads();
        for (int yy = r0; yy < r1; ++yy) {                  // block-uniform trip count
            const float fy = fmaxf(sy * ((float)yy + 0.5f) - 0.5f, 0.0f);
            const float ly1 = fy - (float)j, ly0 = 1.0f - ly1;   // j = min(floor(fy), G - 1) for every row of the band
            const int64_t at = (int64_t)yy * w + x;
            const float gv = live ? gt[b * hw + at] : 0.0f;
            const bool scored = live && depth_valid(gv, lo, hi);
            const double g = scored ? (double)gv : 1.0, lg = log(g), lg10 = log10(g);      // once for the group's configurations
            for (int cc = 0; cc < nc; ++cc) {
                const float* st = stage + cc * 4 * ncols_max;
                const float topN = lx0 * st[a0] + lx1 * st[a1];
                const float botN = lx0 * st[ncols_max + a0] + lx1 * st[ncols_max + a1];
                const float topD = lx0 * st[2 * ncols_max + a0] + lx1 * st[2 * ncols_max + a1];
                const float botD = lx0 * st[3 * ncols_max + a0] + lx1 * st[3 * ncols_max + a1];
                const float N = ly0 * topN + ly1 * botN;
                const float Dn = ly0 * topD + ly1 * botD;
                const bool has = Dn > 0.0f;
                const float pv = has ? fminf(fmaxf(N / Dn, lo), hi) : __builtin_nanf("");
                if (pred && live) pred[((int64_t)(c0 + cc) * B + b) * hw + at] = pv;
                double t[HB_DEPTH_NSUMS];
#pragma unroll
                for (int i = 0; i < HB_DEPTH_NSUMS; ++i) t[i] = 0.0;
                if (scored) {
                    if (!has) t[HB_DEPTH_SUM_NOPRED] = 1.0;
                    else {
                        const double p = (double)pv, d = p - g, d2 = d * d;
                        const double dl = log(p) - lg;
                        const double ratio = fmax(p / g, g / p);
                        t[HB_DEPTH_SUM_N] = 1.0;
                        t[HB_DEPTH_SUM_SQ] = d2;
                        t[HB_DEPTH_SUM_ABS_REL] = fabs(d) / g;
                        t[HB_DEPTH_SUM_SQ_REL] = d2 / g;
                        t[HB_DEPTH_SUM_LOG_SQ] = dl * dl;
                        t[HB_DEPTH_SUM_LOG] = dl;
                        t[HB_DEPTH_SUM_LOG10] = fabs(log10(p) - lg10);
                        t[HB_DEPTH_SUM_D1] = ratio < 1.25 ? 1.0 : 0.0;
                        t[HB_DEPTH_SUM_D2] = ratio < 1.5625 ? 1.0 : 0.0;
                        t[HB_DEPTH_SUM_D3] = ratio < 1.953125 ? 1.0 : 0.0;
                    }
                }
#pragma unroll
                for (int i = 0; i < HB_DEPTH_NSUMS; ++i) {
                    double v = t[i];
                    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
                    if (lane == 0) wave_part[(cc * nw + wv) * HB_DEPTH_NSUMS + i] = v;
                }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < nc * HB_DEPTH_NSUMS; e += bw) {
                const int cc = e / HB_DEPTH_NSUMS, i = e - cc * HB_DEPTH_NSUMS;
                double v = wave_part[(cc * nw) * HB_DEPTH_NSUMS + i];
                for (int k = 1; k < nw; ++k) v = v + wave_part[(cc * nw + k) * HB_DEPTH_NSUMS + i];
                part[(((((int64_t)(c0 + cc) * B + b) * h + yy) * (int64_t)gridDim.x) + blockIdx.x) * HB_DEPTH_NSUMS + i] = v;
            }
            __syncthreads();                                // ... which also lets the next group overwrite the stage
        }
    }
}

extern "C" int hb_depth_upsample_metrics_grid(const float* agg, int n_cfg, int64_t B, int S, int r, int h, int w, const float* gt, float min_depth,
                                              float max_depth, double* sums_out, float* pred_out_opt, void* stream) {
    hb_range range("hbird:depth_upsample_metrics_grid");
    const std::string who = "hb_depth_upsample_metrics_grid: ";
    if (n_cfg < 1 || n_cfg > HB_DEPTH_GRID_MAX_CONFIGS)
        return hb_fail(who + "n_cfg must be in [1, " + std::to_string(HB_DEPTH_GRID_MAX_CONFIGS) + "], got " + std::to_string(n_cfg));
    if (B < 0) return hb_fail(who + "B is negative");
    if (S <= 0 || r <= 0 || h <= 0 || w <= 0) return hb_fail(who + "S, target_grid, h and w must be positive");
    if ((long long)S * r > HB_DEPTH_MAX_GRID) return hb_fail(who + "the cell grid's side S * target_grid exceeds " + std::to_string(HB_DEPTH_MAX_GRID));
    if (const char* why = depth_bounds_error(min_depth, max_depth)) return hb_fail(who + why);
    if (B == 0) return 0;
    if (!agg || !gt || !sums_out) return hb_fail(who + "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int G = S * r;
    const float sy = (float)G / (float)h, sx = (float)G / (float)w;
    // hb_depth_upsample_metrics' geometry: the column chunks of the summation rule, the tallest band, the widest column window
    const int w64 = (w + 63) / 64, nb = (w64 + 3) / 4, bw = (w64 + nb - 1) / nb * 64;
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
    // one configuration's LDS: its wave partials and its four staged rows; as many configurations per group as fit
    const size_t per_cfg = (size_t)(bw / 64) * HB_DEPTH_NSUMS * sizeof(double) + (size_t)4 * ncols_max * sizeof(float);
    const int cpg = (int)std::min<size_t>((size_t)n_cfg, DG_LDS_BYTES / per_cfg);
    if (cpg < 1) return hb_fail(who + "grid too large: one configuration's staged rows (" + std::to_string(ncols_max) + " columns) do not fit the LDS");
    hb_dev<double> part;                                    // [n_cfg][B][h][nb][HB_DEPTH_NSUMS]; every entry is written by exactly one workgroup
    const size_t part_bytes = (size_t)n_cfg * B * h * nb * HB_DEPTH_NSUMS * sizeof(double);
    if (part.ensure(part_bytes, HB_GROW_EXACT)) return -1;
    HB_HIP(hipMemsetAsync(part, 0, part_bytes, s));
    depth_grid_metrics_kernel<<<dim3((unsigned)nb, (unsigned)(G * chunks), (unsigned)B), dim3(bw), (size_t)cpg * per_cfg, s>>>(
        agg, n_cfg, cpg, B, S, r, h, w, sy, sx, chunks, ncols_max, gt, min_depth, max_depth, part, pred_out_opt);
    HB_HIP(hipGetLastError());
    if (hb_launch_depth_row_sums(part, (int64_t)n_cfg * B, h, nb, sums_out, s)) return -1;
    HB_HIP(hipStreamSynchronize(s));                        // the partials are a local of this call
    return 0;
}

// ---- the resampling reduction: out[r][col] = the chain over i ascending of acc + (double)W[r][i] * table[i][col] ---------------------------
// bootstrap_counts_kernel's shape (hbird_bootstrap.hip) in float64: a workgroup owns 256 columns x WS_TR replicates, one thread per column
// with the tile's accumulators in registers (2 x WS_TR VGPRs), walking the images IN ORDER with one coalesced table load each; the tile's
// multiplicities are staged WS_IC images at a time into LDS, transposed to [image][replicate], so that an image's WS_TR values are one
// 128-byte line read at a wave-uniform address.  A thread's chain is the definition itself, so no geometry enters the bits.
// Ragged edges: columns past `cols` load and store nothing, replicates past R carry multiplicity 0 and are not stored.
#define WS_TR 32
#define WS_IC 64
__global__ __launch_bounds__(256) void bootstrap_weighted_sums_kernel(const double* __restrict__ table, int64_t n_img, int64_t cols,
                                                                      const int32_t* __restrict__ W, int64_t R, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int wt[WS_IC][WS_TR];
    const int64_t r0 = (int64_t)blockIdx.x * WS_TR;
    const int64_t col = (int64_t)blockIdx.y * 256 + threadIdx.x;
    const bool live = col < cols;
    double acc[WS_TR];
#pragma unroll
    for (int t = 0; t < WS_TR; ++t) acc[t] = 0.0;
    for (int64_t i0 = 0; i0 < n_img; i0 += WS_IC) {
        const int ni = (int)std::min<int64_t>(WS_IC, n_img - i0);
        __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int e = threadIdx.x; e < WS_TR * WS_IC; e += 256) {
            const int rr = e / WS_IC, ii = e % WS_IC;       // consecutive lanes: consecutive images of one replicate (coalesced)
            wt[ii][rr] = (r0 + rr < R && ii < ni) ? W[(r0 + rr) * n_img + i0 + ii] : 0;
        }
        __syncthreads();
        if (live) {
            const double* tp = table + i0 * cols + col;
            for (int ii = 0; ii < ni; ++ii) {
                const double tv = tp[(int64_t)ii * cols];
#pragma unroll
                for (int t = 0; t < WS_TR; ++t) acc[t] = acc[t] + (double)wt[ii][t] * tv;
            }
        }
    }
    if (live) {
#pragma unroll
        for (int t = 0; t < WS_TR; ++t)
            if (r0 + t < R) out[(r0 + t) * cols + col] = acc[t];
    }
}

extern "C" int hb_bootstrap_weighted_sums(const double* table, int64_t n_img, int64_t cols, const int32_t* W, int64_t R, double* out, void* stream) {
    hb_range range("hbird:bootstrap_weighted_sums");
    const std::string who = "hb_bootstrap_weighted_sums: ";
    if (n_img < 1 || n_img > HB_BOOTSTRAP_MAX_IMAGES)
        return hb_fail(who + std::to_string(n_img) + " images; between 1 and " + std::to_string(HB_BOOTSTRAP_MAX_IMAGES));
    if (cols < 1) return hb_fail(who + "cols must be positive");
    if (R < 0 || R > HB_BOOTSTRAP_MAX_REPLICATES) return hb_fail(who + "R must lie in [0, 2^20]");
    if (R == 0) return 0;
    if (!table || !W || !out) return hb_fail(who + "table / W / out is NULL");
    const int64_t col_blocks = (cols + 255) / 256, r_tiles = (R + WS_TR - 1) / WS_TR;
    if (col_blocks > 65535) return hb_fail(who + "grid too large");
    bootstrap_weighted_sums_kernel<<<dim3((unsigned)r_tiles, (unsigned)col_blocks), dim3(256), 0, (hipStream_t)stream>>>(table, n_img, cols, W, R, out);
    HB_HIP(hipGetLastError());
    return 0;
}
