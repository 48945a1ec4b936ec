// The linear probe (include/hbird_hip_linprobe.h): logits, softmax cross-entropy and its gradient over the resident bank, one evaluation per
// call; the optimiser runs on the host (hbird_mi/linear_probe.py).  gfx950 only.  Definitions -- the bit-defined logits, the fp32 objective,
// the segment rule of the gradient -- are the header's; here are the kernels.
//
// linprobe_forward_kernel: a workgroup of 512 threads takes 256 rows, a wave one 32-row tile with all Cp = 32 * CT classes in CT x 16 accumulator
// registers started at the bias.  The bank's 1 KiB block (rt, g) is the A operand of four successive v_mfma_f32_32x32x2_f32 (lane h * 32 + i
// holds k = 8 g + {h, 2 + h, 4 + h, 6 + h} of row i); Wb, re-tiled once per call into the same fragment layout with classes as "rows"
// (linprobe_retile_kernel), is the B operand, staged through LDS eight column groups at a time for the eight waves.  The result has the class
// on the lane (lane & 31) and the rows in the registers: row max and sums are ds_swizzle butterflies over the 32 lanes of a half-wave.
// linprobe_stage_rows_kernel copies a chunk's rows to row-major [1, x] (skipped and padding rows as zeros) and linprobe_backward_kernel
// contracts residuals and staged rows over the ROW index with the same MFMA: one wave = (segment) x (a 32-column tile of [1, x]) x (two class
// tiles), one fmaf chain over the segment's ascending rows per output, partials to HBM; linprobe_reduce_kernel adds them in float64 in segment order.
// Beyond eight class tiles (the image-level probe, hbird_linprobe_class.hip) linprobe_backward_wide_kernel takes four class tiles x two
// column tiles per wave: the same chains, fewer loads per MFMA.  The kernels that take any class-tile count are reached by both units
// through the host launchers of hbird_linprobe_dev.h.  No floating-point atomic appears in this unit.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include "hbird_k5_dev.h"
#include "hbird_linprobe_dev.h"
#include <algorithm>

#define LP_BWD_CTW 2                 // class tiles of a backward wave
#define LP_BWD_STAGE 16              // row pairs of one stage of its loads (two stages in flight)
#define LP_BWD_WIDE_CTW 4            // the wide form beyond eight class tiles (cp > 256): class tiles x column tiles of a wave,
#define LP_BWD_WIDE_DTW 2            //   eight accumulators fed by six loads per row pair
#define LP_BWD_WIDE_STAGE 8

struct lp_fwd_args {
    const float* tiles; int g8; int64_t ntotal;
    int64_t row0;                    // first row of the launch, a multiple of 256
    const float* wt; const float* bias; int C;
    const void* labels; int u16, P, ls;      // the label table (rows by bank row), nullptr: logits only
    float* logits;                   // [ntotal][C] or nullptr
    float* resid;                    // [rows of the launch, padded to 256][32 CT] or nullptr
    float* resid_out;                // [ntotal][C] or nullptr
    float* rowloss;                  // [ntotal padded to 256] or nullptr
    unsigned char* skip;             // [ntotal padded to 256] or nullptr: 1 for a skipped or padding row
};

// Wb [C][D + 1] -> wt [CT][g8][256] in the bank's fragment layout with classes as rows (zeros beyond C and D), bias [32 CT]
__global__ __launch_bounds__(256) void linprobe_retile_kernel(const float* __restrict__ Wb, int C, int d, int g8, int ct, float* __restrict__ wt,
                                                              float* __restrict__ bias) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)ct * g8 * HB_BLK;
    if (e < ct * 32) bias[e] = e < C ? Wb[e * (int64_t)(d + 1)] : 0.0f;
    if (e >= total) return;
    const int within = (int)(e & (HB_BLK - 1));
    const int64_t blk = e >> 8;
    const int g = (int)(blk % g8), t = (int)(blk / g8);
    const int comp = within & 3, l = within >> 2, h = l >> 5, i = l & 31;
    const int k = 8 * g + 2 * comp + h, c = t * 32 + i;
    wt[e] = (c < C && k < d) ? Wb[c * (int64_t)(d + 1) + 1 + k] : 0.0f;
}

template <int X> __device__ __forceinline__ float lp_swz(float v) {      // lane ^ X inside each group of 32 lanes
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (X << 10) | 0x1f));
}
__device__ __forceinline__ float lp_half_max(float v) {
    v = fmaxf(v, lp_swz<16>(v)); v = fmaxf(v, lp_swz<8>(v)); v = fmaxf(v, lp_swz<4>(v)); v = fmaxf(v, lp_swz<2>(v));
    return fmaxf(v, lp_swz<1>(v));
}
__device__ __forceinline__ float lp_half_sum(float v) {
    v += lp_swz<16>(v); v += lp_swz<8>(v); v += lp_swz<4>(v); v += lp_swz<2>(v);
    return v + lp_swz<1>(v);
}

template <int CT>
__global__ __launch_bounds__(LP_THREADS) void linprobe_forward_kernel(const lp_fwd_args a) {
    extern __shared__ float4 s_w[];      // [CT][LP_GC][64]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
    const int64_t rbase = a.row0 + (int64_t)blockIdx.x * LP_ROWS + wave * 32;      // (below the index's capacity, a multiple of 256)
    const int64_t rt = rbase >> 5;
    const bool live = rbase < a.ntotal;
    const float4* __restrict__ tiles4 = reinterpret_cast<const float4*>(a.tiles);
    const float4* __restrict__ wt4 = reinterpret_cast<const float4*>(a.wt);
    lp_f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const float b = a.bias[t * 32 + i];
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = b;
    }
    int bad = 0;
    for (int g0 = 0; g0 < a.g8; g0 += LP_GC) {
        const int ng = min(LP_GC, a.g8 - g0);
        __syncthreads();                 // the previous groups have been consumed
        for (int e = tid; e < CT * ng * 64; e += LP_THREADS) {
            const int t = e / (ng * 64), rem = e - t * ng * 64;
            s_w[t * LP_GC * 64 + rem] = wt4[((int64_t)t * a.g8 + g0) * 64 + rem];
        }
        float4 av[LP_GC];
#pragma unroll
        for (int gg = 0; gg < LP_GC; ++gg)
            av[gg] = (live && gg < ng) ? tiles4[(rt * (int64_t)a.g8 + g0 + gg) * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
#pragma unroll
        for (int gg = 0; gg < LP_GC; ++gg) {
            if (gg >= ng) break;
            const float4 x = av[gg];
            bad |= (int)!(fabsf(x.x) < INFINITY && fabsf(x.y) < INFINITY && fabsf(x.z) < INFINITY && fabsf(x.w) < INFINITY);
            float4 w[CT];
#pragma unroll
            for (int t = 0; t < CT; ++t) w[t] = s_w[(t * LP_GC + gg) * 64 + lane];
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, w[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, w[t].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, w[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, w[t].w, acc[t], 0, 0, 0);
        }
    }
    // ---- epilogue: lane = class (t * 32 + i), register v = row (v & 3) + 8 (v >> 2) + 4 h of the wave's tile
    const unsigned long long bm = __ballot(bad);
    const int64_t nvalid = a.ntotal - rbase;
    const unsigned beyond = nvalid >= 32 ? 0u : nvalid <= 0 ? 0xFFFFFFFFu : ~((1u << (int)nvalid) - 1u);
    const unsigned masked = (unsigned)bm | (unsigned)(bm >> 32) | beyond;
    if (a.skip && h == 0) a.skip[rbase + i] = (unsigned char)((masked >> i) & 1u);
    const int C = a.C, cp = CT * 32;
    const float Pf = (float)a.P, Pr = 1.0f / Pf;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int ri = (v & 3) + 8 * (v >> 2) + 4 * h;
        const int64_t r = rbase + ri;
        const bool off = (masked >> ri) & 1u, inside = r < a.ntotal;
        float z[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) z[t] = acc[t][v];
        if (a.logits && inside) {
#pragma unroll
            for (int t = 0; t < CT; ++t)
                if (t * 32 + i < C) a.logits[r * (int64_t)C + t * 32 + i] = off ? 0.0f : z[t];
        }
        if (!a.labels) continue;
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < CT; ++t) m = fmaxf(m, t * 32 + i < C ? z[t] : -INFINITY);
        m = lp_half_max(m);
        float se = 0.0f;
#pragma unroll
        for (int t = 0; t < CT; ++t) se += t * 32 + i < C ? expf(z[t] - m) : 0.0f;
        se = lp_half_sum(se);
        const float lse = m + logf(se);
        float y[CT], ys = 0.0f, yz = 0.0f;
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const int c = t * 32 + i;
            y[t] = 0.0f;
            if (c < C && !off) y[t] = a.u16 ? k5_label_at<true>(a.labels, r, a.ls, c, a.P, Pf, Pr) : k5_label_at<false>(a.labels, r, a.ls, c, a.P, Pf, Pr);
            ys += y[t];
            yz = fmaf(y[t], off ? 0.0f : z[t], yz);
        }
        ys = lp_half_sum(ys);
        yz = lp_half_sum(yz);
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const int c = t * 32 + i;
            const float res = (c < C && !off) ? fmaf(ys, expf(z[t] - lse), -y[t]) : 0.0f;
            if (a.resid) a.resid[(r - a.row0) * (int64_t)cp + c] = res;
            if (a.resid_out && inside && c < C) a.resid_out[r * (int64_t)C + c] = res;
        }
        if (a.rowloss && i == 0) a.rowloss[r] = off ? 0.0f : ys * lse - yz;
    }
}

// rows row0 + 32 blockIdx.x .. + 31 as row-major [1, x, 0 ..] of stride xs (the chunk's local row index); a skipped or padding row: zeros
__global__ __launch_bounds__(256) void linprobe_stage_rows_kernel(const float* __restrict__ tiles, int g8, int d, int64_t row0,
                                                                  const unsigned char* __restrict__ skip, float* __restrict__ out, int xs) {
    __shared__ float s[32][65];
    __shared__ unsigned char s_skip[32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
    const int64_t rt = (row0 >> 5) + blockIdx.x, rl0 = (int64_t)blockIdx.x * 32;
    if (tid < 32) s_skip[tid] = skip[rt * 32 + tid];
    __syncthreads();
    const int extra = xs - d;            // column 0 and the padding columns d + 1 .. xs - 1
    for (int e = tid; e < 32 * extra; e += 256) {
        const int row = e / extra, j = e - row * extra;
        out[(rl0 + row) * (int64_t)xs + (j == 0 ? 0 : d + j)] = (j == 0 && !s_skip[row]) ? 1.0f : 0.0f;
    }
    for (int g0 = 0; g0 < g8; g0 += 8) {
        for (int gg = wave; gg < 8; gg += 4) {
            const int g = g0 + gg;
            if (g < g8) {
                const float4 v = *reinterpret_cast<const float4*>(tiles + (rt * (int64_t)g8 + g) * HB_BLK + lane * 4);
                s[i][gg * 8 + h] = v.x; s[i][gg * 8 + 2 + h] = v.y; s[i][gg * 8 + 4 + h] = v.z; s[i][gg * 8 + 6 + h] = v.w;
            }
        }
        __syncthreads();
        for (int e = tid; e < 32 * 64; e += 256) {
            const int row = e >> 6, col = e & 63, k = g0 * 8 + col;
            if (k < d) out[(rl0 + row) * (int64_t)xs + 1 + k] = s_skip[row] ? 0.0f : s[row][col];
        }
        __syncthreads();
    }
}

// partial[seg][c][j] = the fmaf chain over the segment's ascending rows of resid[r][c] * X[r][j], started at 0: the MFMA's k index is the row.
// One wave per (32-column tile of [1, x], segment, group of CTW class tiles): the chains of a segment are sequential by definition, so the
// parallelism is segments x tiles, and small workgroups spread it over the SIMDs.  Both operands come straight from the row-major chunk
// buffers (lane h * 32 + i: row r + h, column / class i -- 128-byte pieces); the loads of the next LP_BWD_STAGE row pairs are in flight while
// the MFMAs of the current ones issue.
template <int CTW>
__global__ __launch_bounds__(64) void linprobe_backward_kernel(const float* __restrict__ resid, int cp, const float* __restrict__ X, int xs,
                                                               int64_t seg_rows, int64_t rows_pad, float* __restrict__ partial) {
    const int lane = threadIdx.x, h = lane >> 5, i = lane & 31;
    const int dt = blockIdx.x, t0 = blockIdx.z * CTW, nt = min(CTW, cp / 32 - t0);
    const int64_t seg = blockIdx.y, r0 = seg * seg_rows, r1 = std::min<int64_t>(rows_pad, r0 + seg_rows);      // (both multiples of 256)
    lp_f32x16 acc[CTW];
#pragma unroll
    for (int t = 0; t < CTW; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.0f;
    const float* xp = X + dt * 32 + i;
    const float* rp = resid + t0 * 32 + i;
    float ra[2][LP_BWD_STAGE][CTW], xb[2][LP_BWD_STAGE];
    auto load = [&](int b, int64_t r) {
#pragma unroll
        for (int u = 0; u < LP_BWD_STAGE; ++u) {
            const int64_t row = r + 2 * u + h;
            xb[b][u] = xp[row * (int64_t)xs];
#pragma unroll
            for (int t = 0; t < CTW; ++t) ra[b][u][t] = t < nt ? rp[row * (int64_t)cp + t * 32] : 0.0f;
        }
    };
    auto compute = [&](int b) {
#pragma unroll
        for (int u = 0; u < LP_BWD_STAGE; ++u)
#pragma unroll
            for (int t = 0; t < CTW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[b][u][t], xb[b][u], acc[t], 0, 0, 0);
    };
    load(0, r0);
    for (int64_t r = r0; r < r1; r += 4 * LP_BWD_STAGE) {      // (256 rows are a whole number of double stages)
        load(1, r + 2 * LP_BWD_STAGE);
        compute(0);
        if (r + 4 * LP_BWD_STAGE < r1) load(0, r + 4 * LP_BWD_STAGE);
        compute(1);
    }
#pragma unroll
    for (int t = 0; t < CTW; ++t) {
        if (t >= nt) break;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int c = (t0 + t) * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
            partial[(seg * cp + c) * (int64_t)xs + dt * 32 + i] = acc[t][v];
        }
    }
}

// The same chains with a wave tile of CTW class tiles x DTW column tiles: every output is still its own fmaf chain over the segment's ascending
// rows, so the bits are those of linprobe_backward_kernel; CTW + DTW loads feed CTW * DTW MFMAs per row pair.
template <int CTW, int DTW>
__global__ __launch_bounds__(64) void linprobe_backward_wide_kernel(const float* __restrict__ resid, int cp, const float* __restrict__ X, int xs,
                                                                    int64_t seg_rows, int64_t rows_pad, float* __restrict__ partial) {
    const int lane = threadIdx.x, h = lane >> 5, i = lane & 31;
    const int d0 = blockIdx.x * DTW, nd = min(DTW, xs / 32 - d0), t0 = blockIdx.z * CTW, nt = min(CTW, cp / 32 - t0);
    const int64_t seg = blockIdx.y, r0 = seg * seg_rows, r1 = std::min<int64_t>(rows_pad, r0 + seg_rows);      // (both multiples of 256)
    lp_f32x16 acc[CTW][DTW];
#pragma unroll
    for (int t = 0; t < CTW; ++t)
#pragma unroll
        for (int u = 0; u < DTW; ++u)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][u][v] = 0.0f;
    const float* xp = X + d0 * 32 + i;
    const float* rp = resid + t0 * 32 + i;
    float ra[2][LP_BWD_WIDE_STAGE][CTW], xb[2][LP_BWD_WIDE_STAGE][DTW];
    auto load = [&](int b, int64_t r) {
#pragma unroll
        for (int p = 0; p < LP_BWD_WIDE_STAGE; ++p) {
            const int64_t row = r + 2 * p + h;
#pragma unroll
            for (int u = 0; u < DTW; ++u) xb[b][p][u] = u < nd ? xp[row * (int64_t)xs + u * 32] : 0.0f;
#pragma unroll
            for (int t = 0; t < CTW; ++t) ra[b][p][t] = t < nt ? rp[row * (int64_t)cp + t * 32] : 0.0f;
        }
    };
    auto compute = [&](int b) {
#pragma unroll
        for (int p = 0; p < LP_BWD_WIDE_STAGE; ++p)
#pragma unroll
            for (int t = 0; t < CTW; ++t)
#pragma unroll
                for (int u = 0; u < DTW; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[b][p][t], xb[b][p][u], acc[t][u], 0, 0, 0);
    };
    load(0, r0);
    for (int64_t r = r0; r < r1; r += 4 * LP_BWD_WIDE_STAGE) {      // (256 rows are a whole number of double stages)
        load(1, r + 2 * LP_BWD_WIDE_STAGE);
        compute(0);
        if (r + 4 * LP_BWD_WIDE_STAGE < r1) load(0, r + 4 * LP_BWD_WIDE_STAGE);
        compute(1);
    }
#pragma unroll
    for (int t = 0; t < CTW; ++t) {
        if (t >= nt) break;
#pragma unroll
        for (int u = 0; u < DTW; ++u) {
            if (u >= nd) break;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int c = (t0 + t) * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                partial[(seg * cp + c) * (int64_t)xs + (d0 + u) * 32 + i] = acc[t][u][v];
            }
        }
    }
}

// acc[c][j] += the chunk's segment partials in float64, ascending segments
__global__ __launch_bounds__(256) void linprobe_reduce_kernel(const float* __restrict__ partial, int nseg, int cp, int xs, int C, int d1,
                                                              double* __restrict__ acc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)C * d1) return;
    const int c = (int)(e / d1), j = (int)(e - (int64_t)c * d1);
    double a = acc[e];
    for (int sgm = 0; sgm < nseg; ++sgm) a += (double)partial[((int64_t)sgm * cp + c) * xs + j];
    acc[e] = a;
}

// grad = acc / n + l2 * Wb, in place
__global__ __launch_bounds__(256) void linprobe_finish_kernel(double* __restrict__ grad, const float* __restrict__ Wb, int64_t total, double n, double l2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) grad[e] = grad[e] / n + l2 * (double)Wb[e];
}

// the float64 trees of the header: 256 blocks x 256 threads over the rows, then one block over the 256 partials
__device__ __forceinline__ double lp_block_tree(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const double t = s[0];
    __syncthreads();
    return t;
}
__global__ __launch_bounds__(256) void linprobe_loss_partial_kernel(const float* __restrict__ rowloss, const unsigned char* __restrict__ skip, int64_t n,
                                                                    double* __restrict__ partial) {
    __shared__ double s[256];
    double acc = 0.0, used = 0.0;        // (counts below 2^53 are exact in a double)
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)LP_TREE_BLOCKS * 256)
        if (!skip[r]) { acc += (double)rowloss[r]; used += 1.0; }
    const double t = lp_block_tree(acc, s), u = lp_block_tree(used, s);
    if (threadIdx.x == 0) { partial[blockIdx.x] = t; partial[LP_TREE_BLOCKS + blockIdx.x] = u; }
}
// out = {sum of the row losses, rows used, sum of Wb^2}
__global__ __launch_bounds__(256) void linprobe_loss_final_kernel(const double* __restrict__ partial, const float* __restrict__ Wb, int64_t total,
                                                                  double* __restrict__ out) {
    __shared__ double s[256];
    const double t = lp_block_tree(partial[threadIdx.x], s), u = lp_block_tree(partial[LP_TREE_BLOCKS + threadIdx.x], s);
    double q = 0.0;
    for (int64_t e = threadIdx.x; e < total; e += 256) q += (double)Wb[e] * (double)Wb[e];
    q = lp_block_tree(q, s);
    if (threadIdx.x == 0) { out[0] = t; out[1] = u; out[2] = q; }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
namespace {
int lp_check_c(const char* who, int C) {
    if (C < 1 || C > HB_LINPROBE_MAX_C) return hb_fail(std::string(who) + ": C must be in [1, " + std::to_string(HB_LINPROBE_MAX_C) + "], got " + std::to_string(C));
    return 0;
}

int lp_forward(const lp_fwd_args& a, int ct, int64_t rows_pad, hipStream_t s) {
    const int lds = ct * LP_GC * 1024;
    const dim3 grid((unsigned)(rows_pad / LP_ROWS)), block(LP_THREADS);
#define LP_FWD(N)                                                                                  \
    case N:                                                                                        \
        if (hb_ensure_dyn_lds((const void*)linprobe_forward_kernel<N>, lds)) return -1;            \
        linprobe_forward_kernel<N><<<grid, block, lds, s>>>(a);                                    \
        break;
    switch (ct) {
        LP_FWD(1) LP_FWD(2) LP_FWD(3) LP_FWD(4) LP_FWD(5) LP_FWD(6) LP_FWD(7) LP_FWD(8)
        default: return hb_fail("linprobe: class tiles out of range");
    }
#undef LP_FWD
    HB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int hb_lp_backward(int ct, const float* resid, const float* X, int xs, int64_t seg_rows, int64_t rows_pad, int nseg, float* partial, hipStream_t s) {
    if (ct > 8)      // (measured against linprobe_backward_kernel<2> at C = 1000: profiles/r36/README.md)
        linprobe_backward_wide_kernel<LP_BWD_WIDE_CTW, LP_BWD_WIDE_DTW><<<dim3((unsigned)((xs / 32 + LP_BWD_WIDE_DTW - 1) / LP_BWD_WIDE_DTW), (unsigned)nseg,
                                                                              (unsigned)((ct + LP_BWD_WIDE_CTW - 1) / LP_BWD_WIDE_CTW)), dim3(64), 0, s>>>(
            resid, ct * 32, X, xs, seg_rows, rows_pad, partial);
    else if (ct == 1)
        linprobe_backward_kernel<1><<<dim3((unsigned)(xs / 32), (unsigned)nseg, 1), dim3(64), 0, s>>>(resid, 32, X, xs, seg_rows, rows_pad, partial);
    else
        linprobe_backward_kernel<LP_BWD_CTW><<<dim3((unsigned)(xs / 32), (unsigned)nseg, (unsigned)((ct + LP_BWD_CTW - 1) / LP_BWD_CTW)), dim3(64), 0, s>>>(
            resid, ct * 32, X, xs, seg_rows, rows_pad, partial);
    HB_HIP(hipGetLastError());
    return 0;
}

int lp_params::make(const hb_index* ix, const float* Wb, int C, hipStream_t s) {
    ct = (C + 31) / 32;
    const int64_t total = (int64_t)ct * ix->g8 * HB_BLK;
    if (wt.ensure((size_t)total * 4, HB_GROW_EXACT) || bias.ensure((size_t)ct * 32 * 4, HB_GROW_EXACT)) return -1;
    linprobe_retile_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(Wb, C, ix->d, ix->g8, ct, wt, bias);
    HB_HIP(hipGetLastError());
    return 0;
}

int hb_lp_stage_rows(const hb_index* ix, int64_t row0, int64_t rows_pad, const unsigned char* skip, float* X, int xs, hipStream_t s) {
    linprobe_stage_rows_kernel<<<dim3((unsigned)(rows_pad / 32)), dim3(256), 0, s>>>(ix->tiles, ix->g8, ix->d, row0, skip, X, xs);
    if (hipGetLastError() != hipSuccess) return hb_fail("linprobe: linprobe_stage_rows_kernel did not launch");
    return 0;
}
int hb_lp_reduce(const float* partial, int nseg, int cp, int xs, int C, int d1, double* grad, hipStream_t s) {
    linprobe_reduce_kernel<<<dim3((unsigned)(((int64_t)C * d1 + 255) / 256)), dim3(256), 0, s>>>(partial, nseg, cp, xs, C, d1, grad);
    if (hipGetLastError() != hipSuccess) return hb_fail("linprobe: linprobe_reduce_kernel did not launch");
    return 0;
}
int hb_lp_loss_tree(const float* rowloss, const unsigned char* skip, int64_t n, double* tree, const float* Wb, int64_t total, double* scal, hipStream_t s) {
    linprobe_loss_partial_kernel<<<dim3(LP_TREE_BLOCKS), dim3(256), 0, s>>>(rowloss, skip, n, tree);
    linprobe_loss_final_kernel<<<dim3(1), dim3(256), 0, s>>>(tree, Wb, total, scal);
    if (hipGetLastError() != hipSuccess) return hb_fail("linprobe: the loss kernels did not launch");
    return 0;
}
int hb_lp_finish(double* grad, const float* Wb, int64_t total, double n, double l2, hipStream_t s) {
    linprobe_finish_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(grad, Wb, total, n, l2);
    HB_HIP(hipGetLastError());
    return 0;
}

extern "C" int hb_linprobe_partition(int64_t ntotal, int64_t* seg_rows, int* nseg) {
    if (!seg_rows || !nseg) return hb_fail("hb_linprobe_partition: NULL pointer");
    if (ntotal < 1) return hb_fail("hb_linprobe_partition: ntotal must be positive");
    const int64_t t = (ntotal + 255) / 256;
    *seg_rows = 256 * std::max<int64_t>(1, (t + HB_LINPROBE_MAX_SEGS - 1) / HB_LINPROBE_MAX_SEGS);
    *nseg = (int)((ntotal + *seg_rows - 1) / *seg_rows);
    return 0;
}

static int64_t g_linprobe_workspace = 0;      // 0 = HB_LINPROBE_WORKSPACE (tests: a small one makes the chunk loop run on small banks)
extern "C" int hb_linprobe_set_workspace(int64_t bytes) {
    if (bytes < 0) return hb_fail("hb_linprobe_set_workspace: bytes must be 0 (HB_LINPROBE_WORKSPACE) or positive, got " + std::to_string(bytes));
    g_linprobe_workspace = bytes;
    return 0;
}
int64_t hb_lp_workspace() { return g_linprobe_workspace > 0 ? g_linprobe_workspace : (int64_t)HB_LINPROBE_WORKSPACE; }

extern "C" int hb_linprobe_logits(hb_index_t* ix, const float* Wb, int C, float* out) {
    if (!ix) return hb_fail("hb_linprobe_logits: NULL index handle");
    if (!Wb || !out) return hb_fail("hb_linprobe_logits: NULL pointer");
    if (lp_check_c("hb_linprobe_logits", C)) return -1;
    if (ix->ntotal < 1) return hb_fail("hb_linprobe_logits: the index is empty");
    hb_range range("hbird:linprobe_logits");
    HB_HIP(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    lp_params par;
    if (par.make(ix, Wb, C, s)) return -1;
    lp_fwd_args a{};
    a.tiles = ix->tiles; a.g8 = ix->g8; a.ntotal = ix->ntotal; a.row0 = 0;
    a.wt = par.wt; a.bias = par.bias; a.C = C; a.P = 1; a.logits = out;
    const int rc = lp_forward(a, par.ct, (ix->ntotal + LP_ROWS - 1) / LP_ROWS * LP_ROWS, s);
    HB_HIP(hipStreamSynchronize(s));      // (the re-tiled parameters go with the call)
    return rc;
}

extern "C" int hb_linprobe_loss_grad(hb_index_t* bank, const float* Wb, int C, double l2, double* loss_host, double* grad, int64_t* used_host,
                                     float* resid_opt) {
    if (!bank) return hb_fail("hb_linprobe_loss_grad: NULL index handle");
    if (!Wb || !loss_host || !grad || !used_host) return hb_fail("hb_linprobe_loss_grad: NULL pointer");
    if (lp_check_c("hb_linprobe_loss_grad", C)) return -1;
    if (bank->ntotal < 1) return hb_fail("hb_linprobe_loss_grad: the bank is empty");
    const int64_t n = bank->ntotal;
    hb_k5_table t;
    if (bank->lab.view(0, n, bank->bnorm, nullptr, 0, &t) != HB_LABELS_OK || t.id_base > 0 || t.id_base + t.nlabels < n)
        return hb_fail("hb_linprobe_loss_grad: the bank has no label row for every one of its " + std::to_string(n) + " rows");
    if (bank->lab.classes() != C)
        return hb_fail("hb_linprobe_loss_grad: C = " + std::to_string(C) + " differs from the label table's " + std::to_string(bank->lab.classes()) + " classes");
    hb_range range("hbird:linprobe_loss_grad");
    HB_HIP(hipSetDevice(bank->device));
    if (hb_labels_checked(bank)) return -1;
    hipStream_t s = bank->stream;
    const int d = bank->d, d1 = d + 1, xs = (d1 + 31) / 32 * 32;
    int64_t seg_rows = 0; int nseg = 0;
    if (hb_linprobe_partition(n, &seg_rows, &nseg)) return -1;
    lp_params par;
    if (par.make(bank, Wb, C, s)) return -1;
    const int cp = par.ct * 32;
    // the bank in row chunks of whole segments: residuals [rows][cp], staged rows [rows][xs], segment partials [segments][cp][xs]
    const int64_t seg_bytes = seg_rows * (int64_t)(cp + xs) * 4;
    const int64_t workspace = hb_lp_workspace();
    const int chunk_segs = (int)std::min<int64_t>(nseg, std::max<int64_t>(1, workspace / seg_bytes));
    const int64_t chunk_rows = (int64_t)chunk_segs * seg_rows, npad = (n + LP_ROWS - 1) / LP_ROWS * LP_ROWS;
    const int64_t chunk_pad = std::min(chunk_rows, npad);
    hb_dev<float> resid, X, partial, rowloss; hb_dev<unsigned char> skip; hb_dev<double> tree, scal;
    if (resid.ensure((size_t)chunk_pad * cp * 4, HB_GROW_EXACT) || X.ensure((size_t)chunk_pad * xs * 4, HB_GROW_EXACT)
        || partial.ensure((size_t)chunk_segs * cp * xs * 4, HB_GROW_EXACT) || rowloss.ensure((size_t)npad * 4, HB_GROW_EXACT)
        || skip.ensure((size_t)npad, HB_GROW_EXACT) || tree.ensure(2 * LP_TREE_BLOCKS * 8, HB_GROW_EXACT) || scal.ensure(3 * 8, HB_GROW_EXACT)) return -1;
    const int64_t total = (int64_t)C * d1;
    HB_HIP(hipMemsetAsync(grad, 0, (size_t)total * 8, s));
    lp_fwd_args a{};
    a.tiles = bank->tiles; a.g8 = bank->g8; a.ntotal = n;
    a.wt = par.wt; a.bias = par.bias; a.C = C;
    a.labels = static_cast<const char*>(t.labels) - t.id_base * (int64_t)t.ls * (t.u16 ? 2 : 4);
    a.u16 = t.u16 ? 1 : 0; a.P = t.u16 ? t.P : 1; a.ls = t.ls;
    a.resid = resid; a.resid_out = resid_opt; a.rowloss = rowloss; a.skip = skip;
    int rc = 0;
    for (int seg0 = 0; seg0 < nseg && !rc; seg0 += chunk_segs) {
        const int segs = std::min(chunk_segs, nseg - seg0);
        a.row0 = (int64_t)seg0 * seg_rows;
        const int64_t rows = std::min(n, a.row0 + (int64_t)segs * seg_rows) - a.row0, rows_pad = (rows + LP_ROWS - 1) / LP_ROWS * LP_ROWS;
        if (lp_forward(a, par.ct, rows_pad, s)) { rc = -1; break; }
        if (hb_lp_stage_rows(bank, a.row0, rows_pad, skip, X, xs, s) || hb_lp_backward(par.ct, resid, X, xs, seg_rows, rows_pad, segs, partial, s)
            || hb_lp_reduce(partial, segs, cp, xs, C, d1, grad, s)) { rc = -1; break; }
    }
    double h[3] = {0.0, 0.0, 0.0};
    if (!rc) {
        if (hb_lp_loss_tree(rowloss, skip, n, tree, Wb, total, scal, s)) rc = -1;
        else if (hipMemcpyAsync(h, scal, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess) rc = hb_fail("hb_linprobe_loss_grad: the loss did not come back");
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = hb_fail("hb_linprobe_loss_grad: the stream failed");
    if (rc) return rc;
    *used_host = (int64_t)h[1];
    if (h[1] < 1.0) return hb_fail("hb_linprobe_loss_grad: every row of the bank holds a non-finite component");
    *loss_host = h[0] / h[1] + 0.5 * l2 * h[2];
    if (hb_lp_finish(grad, Wb, total, h[1], l2, s)) return -1;
    HB_HIP(hipStreamSynchronize(s));      // (the workspace goes with the call)
    return 0;
}
