// Neighbour lists beyond 256 (up to HB_MAX_K = 2048) behind the search: K5 without the bound on k, and a merge of per-shard lists
// without the parts * k bound.  The entries of hbird_aggregate.hip / hbird_knn.hip keep serving k <= 256 exactly as they did (their
// limits are part of their contract); these are the hb_bigk_* family beside them ("k beyond 256").
#include "hbird_internal.h"
#include <algorithm>

#define BIGK_LUT 2048   // uint16 counts: the three-instruction quotient holds for P <= 2048 (hbird_aggregate.hip: AGG_LUT)

// K5 for 1 <= k <= 2048: aggregate_kernel's contract and arithmetic order (hbird_aggregate.hip has the derivation of every step), so
// that for k <= 256 the output bits are aggregate_kernel's:
//   logit_j = (ip_j / (max(|q|, 1e-12) max(|b_j|, 1e-12))) / beta for every neighbour inside the norm table, mx = max_j logit_j,
//   e_j = expf(logit_j - mx), den = lane sums over j = l, l + 64, ... ascending, then the xor butterfly 32 .. 1,
//   w_j = e_j * (den > 0 ? 1 / den : 0), weight 0 for a neighbour whose label row is not here,
//   out_c = one fmaf(w_j, label_j[c], acc) chain over j ascending (C <= 32: per neighbour group g over j = g mod G, groups added in order).
// What differs is where a query's k weights and rows live.  aggregate_kernel keeps them in a static 12 B x 256 per wave, four waves to
// a workgroup.  Here a workgroup IS one wave and holds k x 8 B of dynamic LDS -- the fp32 weight and the row as a 32-bit index (the
// launcher refuses tables of 2^31 rows): 16 KiB at k = 2048, under the 64 KiB that needs no attribute, and ten such waves still fit the
// CU's 160 KiB where four-wave workgroups of 64 KiB would leave it with eight.  No wave waits for another, so nothing is lost by
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
    const float* labels = reinterpret_cast<const float*>(labels_v);
    const unsigned short* counts = reinterpret_cast<const unsigned short*>(labels_v);
    const float Pf = (float)P, Pr = 1.0f / Pf;
    if (q >= nq) return;
    float* wgt = reinterpret_cast<float*>(bigk_smem);          // [k]
    int* rows = reinterpret_cast<int*>(bigk_smem) + k;         // [k]
    // logits of the k neighbours (lane-strided), running maximum
    float mx = -INFINITY;
    for (int j = lane; j < k; j += 64) {
        float logit = -INFINITY;
        int row = -1;
        const int64_t gid = idx[q * (int64_t)k + j];
        const int64_t r = gid - id_base, rn = gid - norm_base;
        if (gid >= 0 && rn >= 0 && rn < nnorm) {
            if (r >= 0 && r < nlabels) row = (int)r;
            const float bn = fmaxf(bnorm[rn], 1e-12f);
            const float qn = fmaxf(qnorm[q], 1e-12f);
            float ip = dist[q * (int64_t)k + j];
            if (metric == 1) ip = 0.5f * (qn2[q] + bnorm[rn] * bnorm[rn] - ip);   // squared L2 -> inner product
            logit = (ip / (qn * bn)) / beta;
        }
        wgt[j] = logit;
        rows[j] = row;
        mx = fmaxf(mx, logit);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float den = 0.0f;
    for (int j = lane; j < k; j += 64) {
        const float e = wgt[j] > -INFINITY ? expf(wgt[j] - mx) : 0.0f;   // every neighbour with a norm takes part (owned or not)
        wgt[j] = e;
        den += e;
    }
    for (int o = 32; o > 0; o >>= 1) den += __shfl_xor(den, o);
    const float inv = den > 0.0f ? 1.0f / den : 0.0f;
    // the weights as they enter the sum, and row 0 with weight 0 for a neighbour whose label row is not here (branch-free gather below)
    for (int j = lane; j < k; j += 64) {
        const bool own = rows[j] >= 0;
        wgt[j] = own ? wgt[j] * inv : 0.0f;
        if (!own) rows[j] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to all its lanes
    auto label_at = [&](int64_t rj, int c) -> float {
        if (U16) {
            const float jf = (float)counts[rj * (int64_t)ls + c];
            if (P > BIGK_LUT) return jf / Pf;
            const float q1 = jf * Pr;
            return fmaf(fmaf(-q1, Pf, jf), Pr, q1);
        }
        return labels[rj * (int64_t)ls + c];
    };
    constexpr int UB = 8;                  // label rows in flight per lane
    if (C <= 32) {
        // lane = (neighbour group g, class c): group g sums the neighbours j = g, g + G, ... ascending, the G partial sums are added in group order
        const int G = 64 / C, g = lane / C, c = lane - g * C;
        const bool act = g < G;
        float accv = 0.0f;
        for (int j0 = 0; j0 < k; j0 += G * UB) {
            float lv[UB], wj[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + u * G + g;
                const bool in = act && j < k;
                wj[u] = in ? wgt[j] : 0.0f;
                lv[u] = in ? label_at(rows[j], c) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) accv = fmaf(wj[u], lv[u], accv);
        }
        float total = accv;
        for (int gg = 1; gg < G; ++gg) total += __shfl(accv, gg * C + c);
        if (g == 0) out[q * (int64_t)C + c] = total;
        return;
    }
    if (U16 && wide) {
        // count rows of 16-byte granules: lane l gathers the eight counts 8 l .. 8 l + 7 of a row with one 16-byte load
        const int nl = (C + 7) >> 3;
        float a8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a8[i] = 0.0f;
        if (lane < nl) {
            for (int j0 = 0; j0 < k; j0 += UB) {
                uint4 raw[UB];
                float wj[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int j = j0 + u;
                    wj[u] = j < k ? wgt[j] : 0.0f;
                    raw[u] = *reinterpret_cast<const uint4*>(counts + (int64_t)(j < k ? rows[j] : 0) * (int64_t)ls + 8 * lane);
                }
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const unsigned wds[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float jf = (float)((wds[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu);
                        const float q1 = jf * Pr;
                        a8[i] = fmaf(wj[u], fmaf(fmaf(-q1, Pf, jf), Pr, q1), a8[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (8 * lane + i < C) out[q * (int64_t)C + 8 * lane + i] = a8[i];
        }
        return;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const int cc = c < C ? c : C - 1;   // lanes past the last class repeat it (no store)
        float accv = 0.0f;
        for (int j0 = 0; j0 < k; j0 += UB) {
            float lv[UB], wj[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + u;
                wj[u] = j < k ? wgt[j] : 0.0f;
                lv[u] = j < k ? label_at(rows[j], cc) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) accv = fmaf(wj[u], lv[u], accv);
        }
        if (c < C) out[q * (int64_t)C + c] = accv;
    }
}

// The table an aggregation reads, chosen as hb_launch_aggregate chooses it: the index's own rows, a borrowed table, or (norms_all) the
// label-sharded form with everybody's norms and this index's label rows.
int hb_launch_aggregate_bigk(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq,
                             int k, int64_t id_base, float beta, float* out, hipStream_t s, const float* norms_all, int64_t n_all) {
    if (nq == 0) return 0;
    if (k < 1 || k > HB_MAX_K) return hb_fail("hb_bigk_aggregate: k must be in [1, " + std::to_string(HB_MAX_K) + "]");
    if (nq > 0x7FFFFFFFLL) return hb_fail("hb_bigk_aggregate: more than 2^31 - 1 queries in one call");
    bool u16 = ix->label_P > 0;
    const void* labels = u16 ? (const void*)ix->labels16 : (const void*)ix->labels;
    const float* bnorm = ix->bnorm;
    int64_t nlab = ix->nlabels, norm_base = id_base, nnorm = ix->nlabels;
    int P = ix->label_P, ls = ix->lab_stride();
    if (norms_all) {   // label-sharded: this index's own label rows, everybody's norms
        if (!labels || ix->nlabels < ix->ntotal) return hb_fail("hb_bigk_aggregate_partial: label rows missing (hb_index_add_labels)");
        nlab = ix->ntotal; bnorm = norms_all; norm_base = 0; nnorm = n_all;
    } else if (ix->ext_labels || ix->ext_labels16) {
        ls = ix->c;                                  // borrowed tables are dense [n, C]
        u16 = ix->ext_labels16 != nullptr;
        labels = u16 ? (const void*)ix->ext_labels16 : (const void*)ix->ext_labels; P = ix->ext_P;
        bnorm = ix->ext_bnorm; nlab = ix->ext_n; id_base = ix->ext_base;
        norm_base = id_base; nnorm = nlab;
    } else if (!labels || ix->nlabels < ix->ntotal) return hb_fail("hb_bigk_search_aggregate: label rows missing (hb_index_add_labels)");
    if (nlab > 0x7FFFFFFFLL) return hb_fail("hb_bigk_aggregate: label tables of more than 2^31 - 1 rows are not supported");
    if (!u16) P = 0;
    // the 16-byte gather's conditions (hb_launch_aggregate: wide_ok)
    const int wide = u16 && (ls & 7) == 0 && (reinterpret_cast<uintptr_t>(labels) & 15) == 0 && P > 0 && P <= BIGK_LUT && ix->c > 32 && ix->c <= 512 ? 1 : 0;
    const dim3 grid((unsigned)nq), block(64);
    const size_t lds = (size_t)k * 8;
    if (u16) aggregate_bigk_kernel<true><<<grid, block, lds, s>>>(labels, ls, wide, P, nlab, ix->c, bnorm, norm_base, nnorm, qnorm, idx, dist, nq, k, id_base, ix->metric, ix->q_aux, beta, out);
    else aggregate_bigk_kernel<false><<<grid, block, lds, s>>>(labels, ls, 0, 0, nlab, ix->c, bnorm, norm_base, nnorm, qnorm, idx, dist, nq, k, id_base, ix->metric, ix->q_aux, beta, out);
    HB_HIP(hipGetLastError());
    return 0;
}

// ---- merge of per-shard lists [parts][nq][k] without staging the union ---------------------------------------------------------
// PRECONDITION (stated at hb_bigk_merge_topk in the header): every list is sorted best-first by (score descending, id ascending) with
// its missing entries (id < 0) only at its tail -- what a search with score output leaves.  Then the union's order under
// merge_parts_kernel's key (present before missing, better score, lower id, lower part, lower position) gives the element at position
// i of part p the rank
//     i + sum over p' != p of #{x in part p' : x before it},
// where "before" lets a tie on (score, id) go to the lower part.  Along a sorted list that predicate is true on a prefix, so each count
// is one binary search: O(parts log k) per element, nothing staged, no bound on parts * k.  The ranks are a permutation of
// 0 .. parts k - 1, so every output slot below k is written exactly once, by the element that owns it.  A list that breaks the
// precondition yields wrong ranks, never a write outside the output: a slot is written only when rank < k.
__global__ __launch_bounds__(256) void merge_sorted_parts_kernel(const float* __restrict__ dist_parts, const int64_t* __restrict__ idx_parts,
                                                                 int parts, int64_t nq, int k, int metric, int64_t dist_stride,
                                                                 int64_t idx_stride, int64_t* __restrict__ out_idx, float* __restrict__ out_dist) {
    const int64_t q = blockIdx.x;
    const int n = parts * k;
    const size_t qoff = (size_t)q * k;
    for (int c = blockIdx.y * 256 + threadIdx.x; c < n; c += gridDim.y * 256) {
        const int p = c / k, i = c - p * k;
        const float d = dist_parts[(size_t)p * dist_stride + qoff + i];
        const int64_t id = idx_parts[(size_t)p * idx_stride + qoff + i];
        const float s = metric == 1 ? -d : d;
        int rank = i;
        for (int pp = 0; pp < parts && rank < k; ++pp) {
            if (pp == p) continue;
            const bool tie = pp < p;      // an equal (score, id) pair, and a missing entry among missing ones, of a lower part comes first
            const float* ds = dist_parts + (size_t)pp * dist_stride + qoff;
            const int64_t* is = idx_parts + (size_t)pp * idx_stride + qoff;
            int lo = 0, hi = k;           // first position of part pp that is NOT before this element
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int64_t ij = is[mid];
                const float dj = ds[mid];
                const float sj = metric == 1 ? -dj : dj;
                bool before;
                if (ij < 0) before = id < 0 && tie;
                else if (id < 0) before = true;
                else before = (sj > s) || (sj == s && (ij < id || (ij == id && tie)));
                if (before) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            const int64_t o = q * (int64_t)k + rank;
            out_idx[o] = id < 0 ? -1 : id;
            out_dist[o] = id < 0 ? (metric == 1 ? INFINITY : -INFINITY) : d;
        }
    }
}

int hb_launch_merge_sorted_parts(const float* dist_parts, const int64_t* idx_parts, int parts, int64_t nq, int k, int metric,
                                 int64_t dist_stride, int64_t idx_stride, int64_t* out_idx, float* out_dist, hipStream_t s) {
    if (nq == 0) return 0;
    if (nq > 0x7FFFFFFFLL) return hb_fail("hb_bigk_merge_topk: more than 2^31 - 1 queries in one call");
    // one workgroup row per query; few queries with long lists spread a query's parts * k elements over several workgroups
    const int64_t per_q = ((int64_t)parts * k + 255) / 256;
    const int64_t ny = std::max<int64_t>(1, std::min<int64_t>(per_q, 2048 / nq));
    merge_sorted_parts_kernel<<<dim3((unsigned)nq, (unsigned)ny), dim3(256), 0, s>>>(dist_parts, idx_parts, parts, nq, k, metric, dist_stride,
                                                                                      idx_stride, out_idx, out_dist);
    HB_HIP(hipGetLastError());
    return 0;
}
