// The MEAN-CENTRED form of the fp16 candidate copy (hb_index_set_fp16_centre; DESIGN.md 4, "the centred screen").
//
// For any fixed vector mu and any scalar t
//
//     q.b  =  (q - t mu).(b - mu)  +  t mu.(b - mu)  +  q.mu
//             `- fp16 MFMA pass -'    `- per ROW: g -'   `- per QUERY: c_q
//
// so the candidate kernel (knn_f16v2_kernel, used as it is) can run on fp16 images of the CENTRED operands: the per-row term enters
// through its row-init pointer (init16 = fmaf(t, g, binit)), the per-query term shifts all of one query's scores alike and is added
// back by the re-rank wherever it compares a pass score with an exact one.  fp16 rounding then acts on q - t mu and b - mu only, and the
// certificate's bound scales with ||q - t mu|| max ||b - mu|| instead of ||q|| max ||b||: on banks whose rows share a large component
// (ViT features with massive activations) that is where the first certificate starts to pass.  Correctness never depends on mu being
// the mean, nor on t: any finite values give the identity above.
//
// Kernels of this unit (plain HIP C++, all HBM-bound or tiny):
//   centre_row_valid_kernel   bank tiles -> one bit per row: every component finite and the row init is not -inf
//   centre_colsum_kernel      column sums of the valid rows over a FIXED partition of the row tiles (float64 partials, fixed order)
//   centre_mean_kernel        partials -> mu[dp16] (0 on the padding dimensions), mu.mu (k-ascending chain), ||mu||
//   centre_bank_kernel        fp32 tiles -> fp16 tiles of fl32(b - mu); g[row]; running max ||b - mu||; overflow flag of the centred values
//   centre_query_dot_kernel   fp32 query tiles -> c_q = q.mu per query (k-ascending chain) and per-block float64 partial sums of them
//   centre_t_kernel           t = sum c_q / (nq mu.mu), partials added in a fixed order (0 when mu.mu = 0)
//   centre_query_kernel       fp32 query tiles -> fp16 tiles of fl32(q - t mu); ||q - t mu||
//   centre_init16_kernel      init16[row] = fmaf(t, g[row], binit[row])   (-inf stays -inf)
#include "hbird_internal.h"
#include "hbird_f16_centre.h"
#include <algorithm>
#include <cmath>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define HC_PARTS 128        // row-tile partitions of the column sums

// fp32 fragment block (rt, gg): 64 float4; float4 p holds row i = p & 31, k = 8 gg + 2 c + (p >> 5) for its components c = 0..3.

__global__ __launch_bounds__(256) void centre_row_valid_kernel(const float* __restrict__ t32, int g8, const float* __restrict__ binit,
                                                               int64_t n_row_tiles, unsigned* __restrict__ valid) {
    const int lane = threadIdx.x & 63;
    const int64_t rt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per row tile
    if (rt >= n_row_tiles) return;
    bool bad = false;
    const f32x4* base = reinterpret_cast<const f32x4*>(t32 + rt * g8 * HB_BLK) + lane;
    for (int gg = 0; gg < g8; ++gg) {
        const f32x4 v = base[(int64_t)gg * 64];
        bad = bad || !(fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY && fabsf(v[3]) < INFINITY);
    }
    if (lane < 32) bad = bad || !(binit[rt * 32 + lane] > -INFINITY);      // (-inf: a padding row; NaN fails too)
    const unsigned long long m = __ballot(bad);
    if (lane == 0) valid[rt] = ~((unsigned)m | (unsigned)(m >> 32));
}

// grid (HC_PARTS, g8); partition p owns the row tiles [p * per, (p + 1) * per); wave w of the block takes every fourth of them in
// ascending order, lanes of one parity are folded by a fixed shuffle tree, the four waves in order 0..3.
__global__ __launch_bounds__(256) void centre_colsum_kernel(const float* __restrict__ t32, int g8, const unsigned* __restrict__ valid,
                                                            int64_t n_row_tiles, int64_t per, double* __restrict__ part,
                                                            long long* __restrict__ part_rows) {
    __shared__ double s_sum[4][8];
    __shared__ long long s_cnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int gg = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < n_row_tiles ? r0 + per : n_row_tiles;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long long cnt = 0;
    for (int64_t rt = r0 + w; rt < r1; rt += 4) {
        const unsigned m = valid[rt];
        cnt += __popc(m);
        if ((m >> (lane & 31)) & 1u) {
            const f32x4 v = reinterpret_cast<const f32x4*>(t32 + (rt * g8 + gg) * HB_BLK)[lane];
            a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
        }
    }
    for (int o = 16; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
    }
    if ((lane & 31) == 0) {       // lane 0: even k (0, 2, 4, 6), lane 32: odd k (1, 3, 5, 7)
        const int odd = lane >> 5;
        s_sum[w][0 + odd] = a0; s_sum[w][2 + odd] = a1; s_sum[w][4 + odd] = a2; s_sum[w][6 + odd] = a3;
    }
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x < 8)
        part[((int64_t)blockIdx.x * g8 + gg) * 8 + threadIdx.x] = ((s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x]) + s_sum[2][threadIdx.x]) + s_sum[3][threadIdx.x];
    if (threadIdx.x == 0 && gg == 0) part_rows[blockIdx.x] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
}

// one block; sc: {cmax, ||mu||, mu.mu, t}
__global__ __launch_bounds__(256) void centre_mean_kernel(const double* __restrict__ part, const long long* __restrict__ part_rows, int g8,
                                                          int n_mu, float* __restrict__ mu, float* __restrict__ sc) {
    long long rows = 0;
    for (int p = 0; p < HC_PARTS; ++p) rows += part_rows[p];
    for (int k = threadIdx.x; k < n_mu; k += 256) {
        double s = 0.0;
        if (k < g8 * 8 && rows > 0) {
            for (int p = 0; p < HC_PARTS; ++p) s += part[(int64_t)p * g8 * 8 + k];
            s /= (double)rows;
        }
        mu[k] = (float)s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m2 = 0.0;
        for (int k = 0; k < n_mu; ++k) m2 = fma((double)mu[k], (double)mu[k], m2);
        sc[0] = 0.0f; sc[1] = __double2float_ru(sqrt(m2)); sc[2] = (float)m2; sc[3] = 0.0f;
    }
}

// One thread per row: the row's fp32 pieces in k order -> fl32(b - mu) -> fp16 pieces; g = mu.(b - mu) as one k-ascending fmaf chain on
// the fp32 differences; ||b - mu|| (float64 sum, rounded up).  A wave covers two row tiles: per step it reads 2 x 2 x 512 contiguous bytes
// and writes 2 x 512.  Rows at and beyond n_rows (the last tile's padding) are converted like any other (their init stays -inf) but do
// not count for cmax or the overflow flag.
__global__ __launch_bounds__(256) void centre_bank_kernel(const float* __restrict__ t32, int g8, const float* __restrict__ mu,
                                                          _Float16* __restrict__ t16, int g16, int64_t rt0, int64_t n_row_tiles,
                                                          int64_t n_rows, float* __restrict__ g_out, float* __restrict__ sc,
                                                          int* __restrict__ overflow) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(gid & 31);
    const int64_t rt = rt0 + (gid >> 5);
    float cn = 0.0f;
    if (rt < rt0 + n_row_tiles) {
        const f32x4* src = reinterpret_cast<const f32x4*>(t32 + rt * g8 * HB_BLK) + i;
        f16x8* dst = reinterpret_cast<f16x8*>(t16) + rt * g16 * 64 + i;
        const int64_t row = rt * 32 + i;
        float g = 0.0f;
        double n2 = 0.0;
        bool ovf = false;
        for (int gg = 0; gg < 2 * g16; ++gg) {
            f16x8 out;
            if (gg < g8) {
                const f32x4 e = src[(int64_t)gg * 64], o = src[(int64_t)gg * 64 + 32];
                const f32x4 me = *reinterpret_cast<const f32x4*>(mu + 8 * gg), mo = *reinterpret_cast<const f32x4*>(mu + 8 * gg + 4);
                // mu is stored in k order: k = 8 gg + 0..7 = {me[0..3], mo[0..3]}; e[c] is k = 8 gg + 2 c, o[c] is k = 8 gg + 2 c + 1
                const float m[8] = {me[0], me[1], me[2], me[3], mo[0], mo[1], mo[2], mo[3]};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d0 = e[c] - m[2 * c], d1 = o[c] - m[2 * c + 1];
                    g = fmaf(m[2 * c], d0, g); g = fmaf(m[2 * c + 1], d1, g);
                    n2 = fma((double)d0, (double)d0, n2); n2 = fma((double)d1, (double)d1, n2);
                    ovf = ovf || (fabsf(d0) > 65504.0f && fabsf(d0) < INFINITY) || (fabsf(d1) > 65504.0f && fabsf(d1) < INFINITY);
                    out[2 * c] = (_Float16)d0; out[2 * c + 1] = (_Float16)d1;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) out[j] = (_Float16)0.0f;
            }
            dst[((int64_t)(gg >> 1) * 2 + (gg & 1)) * 32] = out;
        }
        g_out[row] = g;
        if (row < n_rows) {
            cn = __double2float_ru(sqrt(n2));
            if (ovf) *overflow = 1;
        }
    }
    float m = cn == cn ? cn : 0.0f;                       // (a NaN row counts for nothing, an infinite one makes cmax infinite: no certificate passes)
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(reinterpret_cast<int*>(sc), __float_as_int(m));   // positive floats order like ints
}

// c_q = q.mu, one thread per query row of the fp32 query tiles (coalesced 16-byte pieces, centre_bank_kernel's walk), k ascending; the block's
// 64 values are folded by a fixed shuffle tree into one float64 partial
__global__ __launch_bounds__(64) void centre_query_dot_kernel(const float* __restrict__ t32, int g8, int64_t nq, const float* __restrict__ mu,
                                                              float* __restrict__ cq, double* __restrict__ part) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    float c = 0.0f;
    if (r < nq) {
        const f32x4* src = reinterpret_cast<const f32x4*>(t32 + (r >> 5) * g8 * HB_BLK) + (int)(r & 31);
        for (int gg = 0; gg < g8; ++gg) {
            const f32x4 e = src[(int64_t)gg * 64], o = src[(int64_t)gg * 64 + 32];
            const f32x4 me = *reinterpret_cast<const f32x4*>(mu + 8 * gg), mo = *reinterpret_cast<const f32x4*>(mu + 8 * gg + 4);
            c = fmaf(e[0], me[0], c); c = fmaf(o[0], me[1], c); c = fmaf(e[1], me[2], c); c = fmaf(o[1], me[3], c);
            c = fmaf(e[2], mo[0], c); c = fmaf(o[2], mo[1], c); c = fmaf(e[3], mo[2], c); c = fmaf(o[3], mo[3], c);
        }
        cq[r] = c;
    }
    if (part) {
        double s = r < nq && fabsf(c) < INFINITY ? (double)c : 0.0;      // (a non-finite query has no say in t)
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// one block: thread j adds the partials j, j + 256, ... in ascending order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void centre_t_kernel(const double* __restrict__ part, int n_part, int64_t nq, float* __restrict__ sc) {
    __shared__ double s_w[4];
    double s = 0.0;
    for (int p = threadIdx.x; p < n_part; p += 256) s += part[p];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
        const float m2 = sc[2];
        const float t = m2 > 0.0f ? (float)(tot / ((double)nq * (double)m2)) : 0.0f;
        sc[3] = fabsf(t) < INFINITY ? t : 0.0f;
    }
}

// One thread per query row of the fp32 query tiles (centre_bank_kernel's walk): fp16 tiles of fl32(q - t mu), one fmaf per component, and
// ||q - t mu|| (float64 sum, rounded up).  The padding queries of the last tile stay zero vectors.
__global__ __launch_bounds__(256) void centre_query_kernel(const float* __restrict__ t32, int g8, const float* __restrict__ mu,
                                                           const float* __restrict__ sc, _Float16* __restrict__ t16, int g16,
                                                           int64_t n_row_tiles, int64_t nq, float* __restrict__ qcn) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(gid & 31);
    const int64_t rt = gid >> 5;
    if (rt >= n_row_tiles) return;
    const float nt = -sc[3];
    const int64_t row = rt * 32 + i;
    const f32x4* src = reinterpret_cast<const f32x4*>(t32 + rt * g8 * HB_BLK) + i;
    f16x8* dst = reinterpret_cast<f16x8*>(t16) + rt * g16 * 64 + i;
    double n2 = 0.0;
    for (int gg = 0; gg < 2 * g16; ++gg) {
        f16x8 out;
        if (gg < g8 && row < nq) {
            const f32x4 e = src[(int64_t)gg * 64], o = src[(int64_t)gg * 64 + 32];
            const f32x4 me = *reinterpret_cast<const f32x4*>(mu + 8 * gg), mo = *reinterpret_cast<const f32x4*>(mu + 8 * gg + 4);
            const float m[8] = {me[0], me[1], me[2], me[3], mo[0], mo[1], mo[2], mo[3]};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float d0 = fmaf(nt, m[2 * c], e[c]), d1 = fmaf(nt, m[2 * c + 1], o[c]);
                // The fp16 image is taken of the ROUNDED fp32 value, the one the norm below is summed from.  Left to itself the compiler merges
                // the fmaf and the conversion of the first and last component of every 8-group into v_fma_mixlo/hi_f16, which rounds the exact
                // q - t mu to fp16 ONCE: one element in 2^13 then differs in its last bit from the image of fl32(q - t mu)
                // (tests/test_f16_centre_readout_gpu.py caught it).  The empty asm hides where d0 / d1 came from.
                asm volatile("" : "+v"(d0), "+v"(d1));
                n2 = fma((double)d0, (double)d0, n2); n2 = fma((double)d1, (double)d1, n2);
                out[2 * c] = (_Float16)d0; out[2 * c + 1] = (_Float16)d1;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) out[j] = (_Float16)0.0f;
        }
        dst[((int64_t)(gg >> 1) * 2 + (gg & 1)) * 32] = out;
    }
    if (row < nq) qcn[row] = __double2float_ru(sqrt(n2));
}

__global__ __launch_bounds__(256) void centre_init16_kernel(const float* __restrict__ binit, const float* __restrict__ g,
                                                            const float* __restrict__ sc, int64_t n, float* __restrict__ init16) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const float b = binit[r];
    init16[r] = b == -INFINITY ? b : fmaf(sc[3], g[r], b);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// mu from the rows present now.  -> c.active (0: a non-finite or all-zero mean: the plain copy serves this bank)
static int centre_derive_mean(hb_index* ix, hipStream_t s) {
    hb_centre_state& c = ix->copy16.centre;
    const int64_t nrt = (ix->ntotal + 31) / 32;
    const int64_t per = (nrt + HC_PARTS - 1) / HC_PARTS;
    const size_t b_valid = al256((size_t)nrt * 4), b_part = (size_t)HC_PARTS * ix->g8 * 8 * 8;
    hb_devbuf tmp;
    if (tmp.ensure(b_valid + b_part + HC_PARTS * 8, HB_GROW_EXACT)) return -1;
    unsigned* valid = tmp.as<unsigned>(); double* part = tmp.as<double>(b_valid); long long* part_rows = tmp.as<long long>(b_valid + b_part);
    centre_row_valid_kernel<<<dim3((unsigned)((nrt + 3) / 4)), dim3(256), 0, s>>>(ix->tiles, ix->g8, ix->binit, nrt, valid);
    centre_colsum_kernel<<<dim3(HC_PARTS, (unsigned)ix->g8), dim3(256), 0, s>>>(ix->tiles, ix->g8, valid, nrt, per, part, part_rows);
    centre_mean_kernel<<<dim3(1), dim3(256), 0, s>>>(part, part_rows, ix->g8, std::max(ix->dp16, ix->g8 * 8), c.mu, c.sc);
    HB_HIP(hipGetLastError());
    float h[4] = {0, 0, 0, 0};
    HB_HIP(hipMemcpyAsync(h, c.sc, 16, hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));      // (the kernels are done with tmp)
    c.active = std::isfinite(h[1]) && h[2] > 0.0f ? 1 : 0;
    return 0;
}

// Bring the centred copy up to date (the caller has made the copy's tiles for ix->cap_rows and zeroed them, and marks the rows converted).
// *centred_out = 0: this bank has no usable mean, the caller converts with hb_launch_tiles_to_f16 as without centring.
int hb_centre_convert(hb_index* ix, hipStream_t s, int* centred_out) {
    hb_fp16_copy& copy = ix->copy16;
    hb_centre_state& c = copy.centre;
    *centred_out = 0;
    if (!copy.has_centre_arrays()) {      // (the row arrays go with the tiles: a new copy has none)
        if (copy.make_centre_arrays((size_t)std::max(ix->dp16, ix->g8 * 8))) return -1;
        HB_HIP(hipMemsetAsync(c.g, 0, (size_t)copy.m.cap * 4, s));
        HB_HIP(hipMemsetD32Async((hipDeviceptr_t)c.init16, 0xFF800000u, (size_t)copy.m.cap, s));
    }
    if (copy.m.rows == 0 && centre_derive_mean(ix, s)) return -1;      // a new copy (first use, hb_index_reset, a capacity change): mu anew
    if (!c.active) return 0;
    int64_t rt0 = 0, n_rt = 0;
    copy.m.pending(ix->ntotal, &rt0, &n_rt);
    const int64_t threads = n_rt * 32;
    if (threads > 0) {
        centre_bank_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(ix->tiles, ix->g8, c.mu, copy.tiles.as<_Float16>(), ix->dp16 / 16, rt0, n_rt,
                                                                                         ix->ntotal, c.g, c.sc, copy.flag);
        HB_HIP(hipGetLastError());
    }
    *centred_out = 1;
    return 0;
}

static int centre_qaux(hb_index* ix, int64_t nq, float** cq, float** qcn, double** part) {
    hb_centre_state& c = ix->copy16.centre;
    const size_t b_f = al256((size_t)nq * 4), need = 2 * b_f + (size_t)((nq + 63) / 64) * 8;
    if (c.qaux.ensure(need, HB_GROW_QUARTER)) return -1;
    *cq = c.qaux.as<float>(); *qcn = c.qaux.as<float>(b_f); *part = c.qaux.as<double>(2 * b_f);
    return 0;
}

// The query side of one pass.  first = a caller's search: t is derived from its queries and init16 from t; a nested second pass over the
// uncertified queries (first = 0) keeps both and only converts its gathered queries.
int hb_centre_queries(hb_index* ix, int64_t nq, int first, _Float16* q16, hb_centre_view* view, hipStream_t s) {
    hb_centre_state& c = ix->copy16.centre;
    float *cq = nullptr, *qcn = nullptr;
    double* part = nullptr;
    if (centre_qaux(ix, nq, &cq, &qcn, &part)) return -1;
    const int n_part = (int)((nq + 63) / 64);
    centre_query_dot_kernel<<<dim3((unsigned)n_part), dim3(64), 0, s>>>(ix->q_tiles, ix->g8, nq, c.mu, cq, first ? part : nullptr);
    if (first) {
        centre_t_kernel<<<dim3(1), dim3(256), 0, s>>>(part, n_part, nq, c.sc);
        const int64_t n = (ix->ntotal + HB_BT - 1) / HB_BT * HB_BT;
        centre_init16_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(ix->binit, c.g, c.sc, n, c.init16);
    }
    const int64_t nqp = (nq + HB_QT - 1) / HB_QT * HB_QT;
    centre_query_kernel<<<dim3((unsigned)((nqp + 255) / 256)), dim3(256), 0, s>>>(ix->q_tiles, ix->g8, c.mu, c.sc, q16, ix->dp16 / 16, nqp / 32, nq, qcn);
    HB_HIP(hipGetLastError());
    view->cq = cq; view->qcn = qcn; view->sc = c.sc;      // (whose queries and which level: the pass says so in its report, hb_index_last_centre reads it there)
    return 0;
}

// What the conversion left (include/hbird_hip_centre.h): host bookkeeping and copies, no launch.
int hb_centre_readout(hb_index* ix, float* mu, float* scalars, float* g, float* init16, uint16_t* bank16, float* cq, float* qcn, uint16_t* q16,
                      int64_t info[8]) {
    const hb_fp16_copy& copy = ix->copy16;
    const hb_centre_state& c = copy.centre;
    for (int i = 0; i < 8; ++i) info[i] = 0;
    info[4] = -1;
    const int64_t rows = copy.centred_rows(), n_g = (rows + 31) / 32 * 32, n_init = (rows + HB_BT - 1) / HB_BT * HB_BT;      // (n_g <= n_init)
    if (!ix->fp16_centre || rows <= 0 || !copy.tiles || !copy.has_centre_arrays() || copy.m.cap < n_init)
        return hb_fail("hb_index_last_centre: no active centred copy (centring off, no screened search yet, a bank without a usable mean, or a reset since)");
    const int n_mu = std::max(ix->dp16, ix->g8 * 8);
    // the query side: the last search of a caller ran centred and the bank has not changed since (the report's question)
    const hb_search_report& r = ix->last;
    const bool q_ok = r.centred_queries_readable() && c.qaux.bytes >= 2 * al256((size_t)r.q16_n * 4) &&
                      ix->q16.bytes >= (size_t)((r.q16_n + HB_QT - 1) / HB_QT * HB_QT) * ix->dp16 * 2;
    const int64_t n = q_ok ? r.q16_n : 0, n_qpad = (n + HB_QT - 1) / HB_QT * HB_QT;
    info[0] = rows; info[1] = ix->dp16; info[2] = n_mu; info[3] = n; info[4] = q_ok ? r.q16_level : -1; info[5] = n_g; info[6] = n_init; info[7] = n_qpad;
    HB_HIP(hipSetDevice(ix->device));
    HB_HIP(hipStreamSynchronize(ix->stream));
    if ((cq || qcn || q16) && !q_ok)
        return hb_fail("hb_index_last_centre: the last search of a caller did not run centred (or the bank has changed since: reset, add, capacity)");
    if (mu) HB_HIP(hipMemcpy(mu, c.mu, (size_t)n_mu * 4, hipMemcpyDeviceToHost));
    if (scalars) HB_HIP(hipMemcpy(scalars, c.sc, 16, hipMemcpyDeviceToHost));
    if (g) HB_HIP(hipMemcpy(g, c.g, (size_t)n_g * 4, hipMemcpyDeviceToHost));
    if (init16) HB_HIP(hipMemcpy(init16, c.init16, (size_t)n_init * 4, hipMemcpyDeviceToHost));
    if (bank16) HB_HIP(hipMemcpy(bank16, copy.tiles, (size_t)n_g * ix->dp16 * 2, hipMemcpyDeviceToHost));
    const size_t b_f = al256((size_t)n * 4);      // (centre_qaux's carve-up)
    if (cq && n) HB_HIP(hipMemcpy(cq, c.qaux.as<float>(), (size_t)n * 4, hipMemcpyDeviceToHost));
    if (qcn && n) HB_HIP(hipMemcpy(qcn, c.qaux.as<float>(b_f), (size_t)n * 4, hipMemcpyDeviceToHost));
    if (q16 && n) HB_HIP(hipMemcpy(q16, ix->q16, (size_t)n_qpad * ix->dp16 * 2, hipMemcpyDeviceToHost));
    return 0;
}
