// K5 of SURVEY.md 2.3: soft-label aggregation over the k neighbours of every query patch
// (reference hbird_eval.py:575-609 `_cross_attention` after the CPU index_select of 632-633).  The arithmetic -- every step of it, with
// its derivation -- is k5_body's (hbird_k5_dev.h); the two kernels here differ only in where a query's k weights and rows live.
#include "hbird_internal.h"
#include "hbird_k5_dev.h"

#define AGG_MAX_K 256

// k <= 256: four waves per workgroup, a static 12 B x 256 per wave (the fp32 weight and the row as a 64-bit index)
template <bool U16>
__global__ __launch_bounds__(256) void aggregate_kernel(const void* __restrict__ labels_v, int ls, int wide, int P, int64_t nlabels, int C,
                                                        const float* __restrict__ bnorm, int64_t norm_base, int64_t nnorm,
                                                        const float* __restrict__ qnorm,
                                                        const int64_t* __restrict__ idx,
                                                        const float* __restrict__ dist, int64_t nq, int k,
                                                        int64_t id_base, int metric, const float* __restrict__ qn2,
                                                        float beta, float* __restrict__ out) {
    __shared__ float s_w[4][AGG_MAX_K];
    __shared__ int64_t s_row[4][AGG_MAX_K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wv;
    if (q >= nq) return;   // whole wave exits together (no block-level barrier below)
    k5_body<U16, int64_t>(labels_v, ls, wide, P, nlabels, C, bnorm, norm_base, nnorm, qnorm, idx, dist, k, id_base, metric, qn2, beta, out,
                          q, lane, s_w[wv], s_row[wv]);
}

// 1 <= k <= 2048 (the hb_bigk_* family, DESIGN.md section 4, "k beyond 256"): the same body, so that for k <= 256 the output bits are
// aggregate_kernel's.  Here a workgroup IS one wave and holds k x 8 B of dynamic LDS -- the fp32 weight and the row as a 32-bit index
// (the launcher refuses tables of 2^31 rows): 16 KiB at k = 2048, under the 64 KiB that needs no attribute, and ten such waves still fit
// the CU's 160 KiB where four-wave workgroups of 64 KiB would leave it with eight.  No wave waits for another, so nothing is lost by
// splitting the workgroup; at k <= 256 the 2 KiB per wave leave the wave slots, not LDS, as the limit, as before.
template <bool U16>
__global__ __launch_bounds__(64) void aggregate_bigk_kernel(const void* __restrict__ labels_v, int ls, int wide, int P, int64_t nlabels, int C,
                                                            const float* __restrict__ bnorm, int64_t norm_base, int64_t nnorm,
                                                            const float* __restrict__ qnorm,
                                                            const int64_t* __restrict__ idx,
                                                            const float* __restrict__ dist, int64_t nq, int k,
                                                            int64_t id_base, int metric, const float* __restrict__ qn2,
                                                            float beta, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char bigk_smem[];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    if (q >= nq) return;
    k5_body<U16, int>(labels_v, ls, wide, P, nlabels, C, bnorm, norm_base, nnorm, qnorm, idx, dist, k, id_base, metric, qn2, beta, out,
                      q, lane, reinterpret_cast<float*>(bigk_smem), reinterpret_cast<int*>(bigk_smem) + k);
}

// The table an aggregation reads: the index's own rows (fp32 or counts), a borrowed table covering a global id range, or (norms_all)
// the label-sharded form with everybody's norms and this index's own label rows.  `who` names the entry in the error message.
int hb_k5_table_choose(const hb_index* ix, int64_t id_base, const float* norms_all, int64_t n_all, const char* who, hb_k5_table* t) {
    if (ix->lab.view(id_base, ix->ntotal, ix->bnorm, norms_all, n_all, t) == HB_LABELS_ROWS_MISSING)
        return hb_fail(std::string(who) + ": label rows missing (hb_index_add_labels)");
    // K5's wide gather: rows of whole 16-byte granules at a 16-byte aligned base, the three-instruction quotient's range, at most 64
    // lanes per row, and more classes than the (neighbour group, class) form takes
    t->wide = t->u16 && (t->ls & 7) == 0 && (reinterpret_cast<uintptr_t>(t->labels) & 15) == 0 && t->P > 0 && t->P <= K5_LUT && ix->lab.classes() > 32 && ix->lab.classes() <= 512 ? 1 : 0;
    return 0;
}

int hb_launch_aggregate(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq,
                        int k, int64_t id_base, float beta, float* out, hipStream_t s, const float* norms_all, int64_t n_all) {
    if (nq == 0) return 0;
    if (k > AGG_MAX_K) return hb_fail("hb_index_search_aggregate: k must be <= 256");
    hb_k5_table t;
    if (hb_k5_table_choose(ix, id_base, norms_all, n_all, norms_all ? "hb_index_aggregate_partial" : "hb_index_search_aggregate", &t)) return -1;
    const dim3 grid((unsigned)((nq + 3) / 4)), block(256);
    (t.u16 ? aggregate_kernel<true> : aggregate_kernel<false>)<<<grid, block, 0, s>>>(t.labels, t.ls, t.wide, t.P, t.nlabels, ix->lab.classes(), t.bnorm, t.norm_base, t.nnorm, qnorm, idx, dist, nq, k, t.id_base, ix->metric, ix->q_aux, beta, out);
    HB_HIP(hipGetLastError());
    return 0;
}

int hb_launch_aggregate_bigk(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq,
                             int k, int64_t id_base, float beta, float* out, hipStream_t s, const float* norms_all, int64_t n_all) {
    if (nq == 0) return 0;
    if (k < 1 || k > HB_MAX_K) return hb_fail("hb_bigk_aggregate: k must be in [1, " + std::to_string(HB_MAX_K) + "]");
    if (nq > 0x7FFFFFFFLL) return hb_fail("hb_bigk_aggregate: more than 2^31 - 1 queries in one call");
    hb_k5_table t;
    if (hb_k5_table_choose(ix, id_base, norms_all, n_all, norms_all ? "hb_bigk_aggregate_partial" : "hb_bigk_search_aggregate", &t)) return -1;
    if (t.nlabels > 0x7FFFFFFFLL) return hb_fail("hb_bigk_aggregate: label tables of more than 2^31 - 1 rows are not supported");
    const dim3 grid((unsigned)nq), block(64);
    (t.u16 ? aggregate_bigk_kernel<true> : aggregate_bigk_kernel<false>)<<<grid, block, (size_t)k * 8, s>>>(t.labels, t.ls, t.wide, t.P, t.nlabels, ix->lab.classes(), t.bnorm, t.norm_base, t.nnorm, qnorm, idx, dist, nq, k, t.id_base, ix->metric, ix->q_aux, beta, out);
    HB_HIP(hipGetLastError());
    return 0;
}

// fp32 label values -> uint16 counts: j = round(v P); the stored j is exact iff (float)j / (float)P == v (every value K2 produces);
// anything else raises the sticky flag (read once after the table grew: hb_labels_checked).  Dense [rows, c] in, rows of dst_stride out.
__global__ __launch_bounds__(256) void labels_to_counts_kernel(const float* __restrict__ src, int64_t n, int c, int dst_stride, int P,
                                                               unsigned short* __restrict__ dst, int* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = src[i], Pf = (float)P;
    const float r = rintf(v * Pf);
    const bool ok = r >= 0.0f && r <= Pf && r / Pf == v;
    dst[(i / c) * dst_stride + (i % c)] = ok ? (unsigned short)r : 0;
    if (!ok) *flag = 1;
}

int hb_launch_labels_to_counts(const float* src, int64_t rows, int c, int dst_stride, int P, uint16_t* dst, int* flag, hipStream_t s) {
    const int64_t n = rows * c;
    if (n == 0) return 0;
    labels_to_counts_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(src, n, c, dst_stride, P, dst, flag);
    HB_HIP(hipGetLastError());
    return 0;
}

// out[i, :] = counts[ids[i], :] / P as fp32 (label_memory.index_select on a table stored as counts); ids outside the table give zeros
__global__ __launch_bounds__(256) void gather_label_counts_kernel(const unsigned short* __restrict__ src, int64_t src_rows, int c, int src_stride, int P,
                                                                  const int64_t* __restrict__ ids, int64_t n, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * c) return;
    const int64_t i = t / c, r = ids ? ids[i] : i;      // (ids == nullptr: the rows in order -- hb_index_labels_to_fp32)
    out[t] = (r >= 0 && r < src_rows) ? (float)src[r * src_stride + (t % c)] / (float)P : 0.0f;
}

int hb_launch_gather_label_counts(const uint16_t* src, int64_t src_rows, int c, int src_stride, int P, const int64_t* ids, int64_t n, float* out, hipStream_t s) {
    if (n == 0) return 0;
    gather_label_counts_kernel<<<dim3((unsigned)((n * c + 255) / 256)), dim3(256), 0, s>>>(src, src_rows, c, src_stride, P, ids, n, out);
    HB_HIP(hipGetLastError());
    return 0;
}
