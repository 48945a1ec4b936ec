// Neighbour lists beyond 256 (up to HB_MAX_K = 2048) behind the search: the merge of per-shard lists without the parts * k bound
// (hb_bigk_merge_topk; DESIGN.md section 4, "k beyond 256").  The family's K5, aggregate_bigk_kernel, lives beside aggregate_kernel in
// hbird_aggregate.hip: they are one body.
#include "hbird_internal.h"
#include <algorithm>

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
