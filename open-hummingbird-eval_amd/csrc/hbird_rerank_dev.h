// The exact re-rank of the fp16 screen, everything that is not "score one candidate row": the argument block of a launch (rerank_kernel
// scores from the fragment tiles, rerank_rows_kernel from the row-major copy: hbird_knn_f16.hip), the per-query constants, which candidates
// need an exact score at all, and the tail -- rank, CERTIFICATE, output -- over the wave's scores in LDS.
// The device pieces take plain parameters, as the kernels do: with the argument block passed through them rerank_rows_kernel<false> needs
// two more VGPRs than the spill guard's baseline (tests/test_kernel_resources_cpu.py) -- the block is the launcher's interface only.
#pragma once
#include "hbird_internal.h"
#include "hbird_certificate.h"

// What the re-rank leaves for an ESCALATION of the queries whose certificate fails (hb_launch_knn), and what it takes from the pass before:
//   seed_in  [query] (second pass only): the fp16-score floor this pass ran under -- every row with an fp16 score >= it was offered to the
//            pools, so a candidate list that is NOT full holds every such row: the rows outside score below the floor in fp16, hence below
//            floor + E exactly, and the answer is exact when its k-th best exceeds that: plain  kth > seed + E ;  centred, in the pass'
//            units as the floor was formed:  kth - c_q > seed + E' ;
//   kth_out  [query]: the exact k-th best score among this pass's candidates -- a lower bound of the true k-th best: the floor of an fp32
//            search of this query (ties pass: floor_from_key);
//   floor_out[query]: kth - 1.001 E, a hair lower: every row that can still enter the top k has an exact score >= kth, hence an fp16 score
//            above this -- the floor of a second, wider fp16 pass (0.001 E is twenty times the rounding of these few operations).
// CENTRED (hbird_f16_centre.hip): the pass ran on q - t mu and b - mu and its scores lack the query's constant c_q = q.mu -- every comparison of
// an exact score with a pass score adds it to the latter; floor_out seeds the second PASS and is written in the pass' units (kth - c_q - 1.001 E'),
// kth_out seeds the fp32 kernel and stays exact.
struct hb_rerank_seeds { const float* seed_in; float* kth_out; float* floor_out; };

// One re-rank launch, whichever form the bank's rows are read in: what both kernels take after their row source, in their order.
// cand / cand_score [nq][kc]: the pass' candidates, sorted by pass score (-1: none); qnorm [nq], bmax[0]: the norms of the bound;
// cv.cq == nullptr: the plain pass.
struct hb_rerank_args {
    const float* binit; int d; const float* q; const float* qn2;
    const int64_t* cand; const float* cand_score; const float* qnorm; const float* bmax;
    unsigned char* certified; int kc; int64_t nq; int k; int64_t id_base; int metric, out_metric; int64_t ntotal;
    int64_t* out_idx; float* out_dist;
    hb_rerank_seeds sd; hb_centre_view cv;
};

template <bool CENTRED>
__device__ __forceinline__ bool hb_rerank_finish(const hb_rerank_seeds& sd, int64_t qi, bool ok, bool list_not_full, bool have_kth, float s, float E, float cq) {
    // (centred: compared in the pass' units, as floor_out was formed -- s - cq is rounded at ITS size, seed + cq at the size of c_q, whose ulp
    // exceeds the 0.001 E' between floor and rule wherever |c_q| 2^-24 > 0.001 E': a complete first answer then passed or failed by rounding)
    if (sd.seed_in && list_not_full && have_kth && !ok) ok = CENTRED ? s - cq > sd.seed_in[qi] + E : s > sd.seed_in[qi] + E;
    if (sd.kth_out) {
        const bool fin = have_kth && E < INFINITY && fabsf(s) < INFINITY && (!CENTRED || fabsf(cq) < INFINITY);      // (false for NaN as well)
        float f = CENTRED ? s - cq - 1.001f * E : s - 1.001f * E;
        f = f - fabsf(f) * 2.4e-7f - 1e-37f;
        sd.kth_out[qi] = fin ? s : -INFINITY;
        sd.floor_out[qi] = fin ? f : -INFINITY;
    }
    return ok;
}

// the centred bound of query qi from what hb_centre_queries left: sc = {cmax, ||mu||, mu.mu, t}
__device__ __forceinline__ float hb_centred_E(const hb_centre_view& cv, int64_t qi, float qn, float bmax, int d, int metric) {
    return hb_certificate_bound_centred(cv.qcn[qi], cv.sc[0], cv.sc[1], fabsf(cv.sc[3]), qn, bmax, d, metric);
}

// Per query: the bound E (hbird_certificate.h) -- the certificate below, and which candidates need an exact score at all: the list comes
// sorted by fp16 score, its first k have exact scores >= (k-th fp16 score) - E, so a candidate whose fp16 score is more than 2E below the
// k-th's (the cut) is exactly below k of them and cannot be in the answer.  Its row is not read (in the tiles a row is 2 x D/8 sixteen-byte
// pieces 512 B apart: the re-rank is bound by the sectors it touches; 50,176 x 384, 12,544 queries: 0.96 ms of a 2.4 ms search).
// A non-finite E (query norm) skips nothing, and fails the certificate.  cq: the centred pass' c_q (0 for the plain pass).
struct hb_rerank_query { float E, cq, cut; };
template <bool CENTRED>
__device__ __forceinline__ hb_rerank_query hb_rerank_query_of(int64_t qi, const float* qnorm, const float* bmax, int d, int metric, const hb_centre_view& cv,
                                                              const int64_t* cand, const float* cand_score, int kc, int k) {
    hb_rerank_query c;
    c.E = CENTRED ? hb_centred_E(cv, qi, qnorm[qi], bmax[0], d, metric) : hb_certificate_bound(qnorm[qi], bmax[0], d, metric);
    c.cq = CENTRED ? cv.cq[qi] : 0.0f;
    c.cut = (k <= kc && cand[qi * (int64_t)kc + (k - 1)] >= 0) ? cand_score[qi * (int64_t)kc + (k - 1)] - 2.0f * c.E : -INFINITY;
    return c;
}
// does candidate c of a query's list (bank row `row`, negative: none; pass_score: the query's kc scores) need an exact score
__device__ __forceinline__ bool hb_rerank_needs_score(int64_t row, int c, int k, const float* pass_score, float cut) { return row >= 0 && !(c >= k && pass_score[c] < cut); }

// The tail of one wave = one query: s_sc[c] / s_id[c], c < kc, hold candidate c's exact score (-inf: skipped or none) and bank row, visible
// to every lane.  ID: the row as the kernel keeps it in LDS -- 4 bytes with HB_ID_NONE for "none" (bank rows are below 2^32 everywhere in this
// library), or the list's own 8 bytes (negative: none).  Lane j ranks candidates j, j + 64, ... by (score desc, id asc, position asc), missing entries last; the lane that holds
// rank k - 1 decides the certificate; ranks below k are written.
template <bool CENTRED, typename ID>
__device__ __forceinline__ void hb_rerank_tail(const float* s_sc, const ID* s_id, int lane, int64_t qi, float E, float cq, const int64_t* cand, const float* cand_score,
                                               const float* qnorm, const float* qn2, unsigned char* certified, int kc, int k, int64_t id_base, int out_metric,
                                               int64_t ntotal, int64_t* out_idx, float* out_dist, const hb_rerank_seeds& sd, const hb_centre_view& cv) {
    for (int c = lane; c < kc; c += 64) {
        const float s = s_sc[c];
        const int64_t id = sizeof(ID) == 4 && s_id[c] == (ID)HB_ID_NONE ? -1 : (int64_t)s_id[c];
        int rank = 0;
        for (int j = 0; j < kc; ++j) {
            const float sj = s_sc[j];
            const int64_t ij = sizeof(ID) == 4 && s_id[j] == (ID)HB_ID_NONE ? -1 : (int64_t)s_id[j];
            bool better;
            if (ij < 0 || id < 0) better = (ij >= 0 && id < 0) || (ij < 0 && id < 0 && j < c);
            else better = (sj > s) || (sj == s && (ij < id || (ij == id && j < c)));
            rank += better;
        }
        if (rank == k - 1) {
            // Certificate: every row outside the candidate list has an fp16 score <= the kc-th candidate's, hence an
            // exact score <= that + E.  If the exact k-th best is strictly above that bound, no outside row can enter the
            // top k: the answer IS the fp32 answer.
            // The argument needs finite fp16 operands: a query with |q_i| > 65504 becomes inf in fp16 and its scores inf / NaN
            // (||q|| <= 65504 rules that out; a NaN / inf norm fails the test too), and a candidate list that is not full
            // although the bank has kc rows has lost rows to NaN / -inf fp16 scores that nothing bounds.
            const int64_t last = cand[qi * (int64_t)kc + kc - 1];
            const bool finite_q = CENTRED ? (cv.qcn[qi] <= 65504.0f && qnorm[qi] < INFINITY && fabsf(cq) < INFINITY) : qnorm[qi] <= 65504.0f;   // (centred: the operands of the pass are q - t mu)
            bool ok = last < 0 && ntotal < kc && finite_q;   // fewer than kc rows exist: every row was a candidate
            if (last >= 0 && id >= 0 && finite_q) ok = CENTRED ? s > cand_score[qi * (int64_t)kc + kc - 1] + cq + E : s > cand_score[qi * (int64_t)kc + kc - 1] + E;
            ok = hb_rerank_finish<CENTRED>(sd, qi, ok, last < 0, id >= 0 && finite_q, s, E, cq);
            certified[qi] = ok ? 1 : 0;
        }
        if (rank < k) {
            const int64_t o = qi * (int64_t)k + rank;
            if (id < 0) { out_idx[o] = -1; out_dist[o] = out_metric == 1 ? INFINITY : -INFINITY; }
            else {
                out_idx[o] = id + id_base;
                if (out_metric == 1) { const float d2 = fmaf(-2.0f, s, qn2[qi]); out_dist[o] = d2 > 0.0f ? d2 : 0.0f; }
                else out_dist[o] = s;
            }
        }
    }
}
