// The excluding form of the fp16 screen's exact re-rank (include/hbird_hip_exclude_screen.h; DESIGN.md 4 "Excluding searches on the screen").
//
// The screen's certificate is a statement about the rows OUTSIDE a query's k' candidates: their exact score is at most the k'-th pass score + E.
// It says nothing about which of the candidates are allowed.  So the query's own row group is dropped among the candidates, and when the exact
// k-th best of the remaining ones lies strictly above that same bound, the answer is the excluding search's answer, bit for bit -- at the cost
// of a plain search at k instead of one at k + (largest group).  The candidate kernel, the merge, the pools and the plan are untouched; the
// rank, the certificate and the output are hb_rerank_tail's, unchanged: an excluded candidate enters LDS as "none" at its position, missing
// entries rank last, and the threshold and the list's last entry are read from the unmasked list in global memory.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include "hbird_rerank_dev.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One wave per query, four queries per workgroup.  Candidate c (row = cand[qi][c]) is excluded when row >= 0, qgroups[qi] >= 0,
// row < n_group_rows and groups[row] == qgroups[qi].  A row at or beyond ntotal (a caller's own list: hb_index_exclude_rerank) is never
// dereferenced and counts as "none".
// Skip rule: p_k = the list position of the k-th allowed candidate (ballot + prefix count over chunks of 64 entries).  The k allowed candidates
// up to p_k have pass scores >= cand_score[p_k], hence exact scores >= cand_score[p_k] - E; a candidate behind p_k whose pass score is below
// cut = cand_score[p_k] - 2E is exactly below all k of them and is not scored.  No such candidate, or a non-finite E: nothing is skipped.
// Scoring: rerank_kernel's per-lane chain over the fp32 fragment tiles (acc = row init; fmaf(q_k, b_k, acc), k ascending): the fp32 search's bits.
template <bool CENTRED>
__global__ __launch_bounds__(256) void excl_screen_rerank_kernel(const float* __restrict__ tiles, int g8, const float* __restrict__ binit, int d,
                                                                 const float* __restrict__ q, const float* __restrict__ qn2,
                                                                 const int64_t* __restrict__ cand, const float* __restrict__ cand_score,
                                                                 const float* __restrict__ qnorm, const float* __restrict__ bmax,
                                                                 unsigned char* __restrict__ certified, int kc, int64_t nq, int k, int64_t id_base,
                                                                 int metric, int out_metric, int64_t ntotal, int64_t* __restrict__ out_idx,
                                                                 float* __restrict__ out_dist, hb_rerank_seeds sd, hb_centre_view cv,
                                                                 const int32_t* __restrict__ groups, int64_t n_group_rows,
                                                                 const int32_t* __restrict__ qgroups) {
    __shared__ float s_sc[4][256];
    __shared__ int64_t s_id[4][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wv;
    if (qi >= nq) return;   // wave-uniform: the ballots below see whole waves
    const float* qr = q + qi * (int64_t)d;
    const int64_t* li = cand + qi * (int64_t)kc;
    const float* ls = cand_score + qi * (int64_t)kc;
    const hb_rerank_query qc = hb_rerank_query_of<CENTRED>(qi, qnorm, bmax, d, metric, cv, cand, cand_score, kc, k);   // (E and c_q; the cut is this kernel's own)
    const int32_t qg = qgroups[qi];
    // pass 1: which of this lane's candidates are allowed (bit i: candidate lane + 64 i), and p_k
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned allowed_bits = 0;
    int before = 0, pk = -1;
    for (int c0 = 0, i = 0; c0 < kc; c0 += 64, ++i) {
        const int c = c0 + lane;
        const int64_t row = c < kc ? li[c] : -1;
        bool allowed = row >= 0 && row < ntotal;
        if (allowed && qg >= 0 && row < n_group_rows) allowed = groups[row] != qg;
        if (allowed) allowed_bits |= 1u << i;
        const unsigned long long m = __ballot(allowed);
        const unsigned long long hit = __ballot(allowed && before + __popcll(m & lt) == k - 1);
        if (hit && pk < 0) pk = c0 + __ffsll((long long)hit) - 1;
        before += __popcll(m);
    }
    const float cut = (pk >= 0 && fabsf(qc.E) < INFINITY) ? ls[pk] - 2.0f * qc.E : -INFINITY;      // (false for a NaN bound as well)
    // pass 2: the exact scores
    for (int c = lane, i = 0; c < kc; c += 64, ++i) {
        const bool allowed = (allowed_bits >> i) & 1u;
        const int64_t row = allowed ? li[c] : -1;
        float acc = -INFINITY;
        if (allowed && !(c > pk && ls[c] < cut)) {
            acc = binit[row];
            const float* base = tiles + ((row >> 5) * (int64_t)g8) * HB_BLK + (int)(row & 31) * 4;
            for (int g = 0; g < g8; ++g) {
                const f32x4 e = *reinterpret_cast<const f32x4*>(base + (int64_t)g * HB_BLK);         // k = 8g + 0,2,4,6
                const f32x4 o = *reinterpret_cast<const f32x4*>(base + (int64_t)g * HB_BLK + 128);   // k = 8g + 1,3,5,7
                const int k0 = 8 * g;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k0 + 2 * j < d) acc = fmaf(qr[k0 + 2 * j], e[j], acc);
                    if (k0 + 2 * j + 1 < d) acc = fmaf(qr[k0 + 2 * j + 1], o[j], acc);
                }
            }
        }
        s_sc[wv][c] = acc;
        s_id[wv][c] = row;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to its lanes
    hb_rerank_tail<CENTRED>(s_sc[wv], s_id[wv], lane, qi, qc.E, qc.cq, cand, cand_score, qnorm, qn2, certified, kc, k, id_base, out_metric, ntotal, out_idx, out_dist, sd, cv);
}

// the excluding re-rank of one pass' candidates, from the fragment tiles.  a.cv.cq != nullptr: a centred pass
int hb_launch_excl_screen_rerank(const hb_rerank_args& a, const float* tiles, int g8, const int32_t* groups, int64_t n_group_rows, const int32_t* qgroups,
                                 hipStream_t s) {
    if (a.nq == 0) return 0;
    if (a.kc > 256 || a.k > a.kc || a.k < 1) return hb_fail("excluding re-rank: 1 <= k <= candidates <= 256");
    auto fn = a.cv.cq != nullptr ? excl_screen_rerank_kernel<true> : excl_screen_rerank_kernel<false>;
    fn<<<dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s>>>(tiles, g8, a.binit, a.d, a.q, a.qn2, a.cand, a.cand_score, a.qnorm, a.bmax, a.certified, a.kc, a.nq, a.k,
                                                            a.id_base, a.metric, a.out_metric, a.ntotal, a.out_idx, a.out_dist, a.sd, a.cv, groups, n_group_rows, qgroups);
    HB_HIP(hipGetLastError());
    return 0;
}

// out[i] = src[ids[i]]: the groups of the queries a nested pass searches again
__global__ __launch_bounds__(256) void excl_gather_groups_kernel(const int32_t* __restrict__ src, int64_t n_src, const int64_t* __restrict__ ids, int64_t n,
                                                                 int32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t i = ids[t];
    out[t] = i >= 0 && i < n_src ? src[i] : -1;
}
int hb_launch_gather_groups(const int32_t* src, int64_t n_src, const int64_t* ids, int64_t n, int32_t* out, hipStream_t s) {
    if (n == 0) return 0;
    excl_gather_groups_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(src, n_src, ids, n, out);
    HB_HIP(hipGetLastError());
    return 0;
}

extern "C" int hb_index_set_exclude_screen(hb_index_t* ix, int on) {
    if (!ix) return hb_fail("hb_index_set_exclude_screen: NULL index handle");
    if (on < 0 || on > 1) return hb_fail("hb_index_set_exclude_screen: on must be 0 or 1");
    ix->excl_screen = on;
    return 0;
}

extern "C" int hb_index_last_exclusion_screen(const hb_index_t* ix, int64_t out[8]) {
    if (!ix) return hb_fail("hb_index_last_exclusion_screen: NULL index handle");
    if (!out) return hb_fail("hb_index_last_exclusion_screen: out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = ix->last_excl_screen[i];
    return 0;
}

// (hb_index_last_exclusion_seeds: hbird_readout.hip)

extern "C" int hb_index_exclude_rerank(hb_index_t* ix, const float* q, int64_t nq, const int64_t* cand_rows, const float* pass_scores, int kc,
                                       const int32_t* qgroups, int k, int64_t id_base, int64_t* out_idx, float* out_dist,
                                       unsigned char* out_certified, float* out_kth, float* out_floor) {
    if (!ix) return hb_fail("hb_index_exclude_rerank: NULL index handle");
    if (nq < 0) return hb_fail("hb_index_exclude_rerank: negative query count");
    if (k < 1) return hb_fail("hb_index_exclude_rerank: k must be at least 1");
    if (kc < k || kc > 256 || kc % 8 != 0) return hb_fail("hb_index_exclude_rerank: kc must be a multiple of 8 in [k, 256]");
    if (ix->row_groups_n == 0) return hb_fail("hb_index_exclude_rerank: the index has no row-group table (hb_index_set_row_groups)");
    if (ix->row_groups_n != ix->ntotal)
        return hb_fail("hb_index_exclude_rerank: the row-group table covers " + std::to_string(ix->row_groups_n) + " rows, the bank holds " +
                       std::to_string(ix->ntotal) + " (set the table again)");
    if (!q || !cand_rows || !pass_scores || !qgroups || !out_idx || !out_dist || !out_certified) return hb_fail("hb_index_exclude_rerank: NULL pointer");
    if (nq == 0) return 0;
    HB_HIP(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    if (!ix->bmax) return hb_fail("hb_index_exclude_rerank: the bank is empty");
    // chain ||q||^2 and fp32 norms of these queries, in a workspace of their own (q_aux belongs to the searches); the tail writes the k-th
    // score and the floor together: where the caller takes only one, the other lands behind them
    if (ix->excl1.ensure(al256((size_t)nq * 12), HB_GROW_EXACT)) return -1;
    float* aux = ix->excl1.as<float>();
    if (hb_launch_query_aux(q, nq, ix->d, aux, aux + nq, s)) return -1;
    if (out_kth && !out_floor) out_floor = aux + 2 * nq;
    if (out_floor && !out_kth) out_kth = aux + 2 * nq;
    const int out_metric = ix->score_output ? 0 : ix->metric;
    const hb_rerank_args ra{ix->binit, ix->d, q, aux, cand_rows, pass_scores, aux + nq, ix->bmax, out_certified, kc, nq, k, id_base, ix->metric, out_metric,
                            ix->ntotal, out_idx, out_dist, hb_rerank_seeds{nullptr, out_kth, out_floor}, hb_centre_view{nullptr, nullptr, nullptr}};
    if (hb_launch_excl_screen_rerank(ra, ix->tiles, ix->g8, ix->row_groups, ix->row_groups_n, qgroups, s)) return -1;
    HB_HIP(hipStreamSynchronize(s));
    return 0;
}
