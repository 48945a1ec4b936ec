// Device code shared by the three K5 kernels: aggregate_kernel and aggregate_bigk_kernel (hbird_aggregate.hip), which are two LDS
// placements of ONE body (k5_body), and aggregate_grid_kernel (hbird_grid.hip), which keeps its own softmax per configuration and its
// multi-accumulator gathers but resolves neighbours and decodes counts with the functions below.  Bit-identity between the three is the
// contract (tests/test_bigk_aggregate_gpu.py, tests/test_grid_aggregate_gpu.py): the float operations below are written once, in the
// order every kernel applies them.
//
//   q^ = q / max(||q||, 1e-12), k^_j = b_j / max(||b_j||, 1e-12)           (F.normalize, reference hbird_eval.py:594-595)
//   attn = softmax_j( (q^ . k^_j) / beta ),  label_hat = sum_j attn_j * label_j   (603-608)
//
// The kNN kernel already produced ip_j = q . b_j for the k neighbours, so q^.k^_j = ip_j / (||q|| ||b_j||)
// and only the k label rows (k*C*4 bytes per query) are gathered -- the k x D neighbour features
// the reference gathers on the CPU are never touched.  HBM-bound gather: one wave per query.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Label rows come as fp32 values or (U16) as uint16 counts j of values j / P -- what K2 produces: (float)j / (float)P -- at half the
// gather traffic and half the table in HBM (6.2 -> 3.1 GB at cfg-3, per rank when the table is replicated).  The very same fp32 value
// comes back from three instructions instead of a division: r = RN(1 / P) once, q' = RN(j r), e = fma(-q', P, j) (exact), q = fma(e, r, q')
// -- correctly rounded for every 0 <= j <= P <= 2048 (checked exhaustively: tests/test_ops_gpu.py::test_count_quotients_are_exact); larger
// denominators divide in place.  (Until round 5 a table of the P + 1 quotients in LDS: 64 lanes looking up random entries conflict three-
// to four-way, and the kernel ran slower on counts than on fp32 rows although it moved half the bytes.)
#define K5_LUT 2048

// Pf = (float)P, Pr = 1.0f / Pf; P <= K5_LUT
__device__ __forceinline__ float k5_quotient(float jf, float Pf, float Pr) {
    const float q1 = jf * Pr;
    return fmaf(fmaf(-q1, Pf, jf), Pr, q1);
}

// element c of label row rj of a table of row stride ls: the fp32 value, or the value of the count stored there
template <bool U16>
__device__ __forceinline__ float k5_label_at(const void* __restrict__ labels_v, int64_t rj, int ls, int c, int P, float Pf, float Pr) {
    if (U16) {
        const float jf = (float)reinterpret_cast<const unsigned short*>(labels_v)[rj * (int64_t)ls + c];
        if (P > K5_LUT) return jf / Pf;
        return k5_quotient(jf, Pf, Pr);
    }
    return reinterpret_cast<const float*>(labels_v)[rj * (int64_t)ls + c];
}

// the eight counts of one 16-byte granule as label values (the wide gathers: P <= K5_LUT is among their launch conditions)
__device__ __forceinline__ void k5_unpack8(const uint4& raw, float Pf, float Pr, float (&lv)[8]) {
    const unsigned wds[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) lv[i] = k5_quotient((float)((wds[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu), Pf, Pr);
}

// One list position.  Two id ranges: the NORM table covers global ids [norm_base, norm_base + nnorm) and decides which neighbours take
// part in the softmax; the LABEL table covers [id_base, id_base + nlabels) and decides whose label rows are summed here.  They coincide
// for an ordinary index.  Label-sharded aggregation (hb_index_aggregate_partial): the norms of ALL rows are replicated (4 B per row), the
// label rows stay with their owners; every rank computes the same weights and the partial sum over the neighbours it owns, the
// all-reduce of the partial sums is label_hat ("distributed softmax + all-reduce").
// -> the cosine ip / (max(|q|, 1e-12) max(|b|, 1e-12)) (L2 lists: ip = 0.5 (qn2 + bn^2 - dist)), -inf outside the norm table; row = the
// label row, -1 where it is not in the label table.  ip_j, qnorm_q, qn2_q point at this position's / this query's entries and are read
// only for a neighbour inside the norm table.
__device__ __forceinline__ float k5_neighbour(int64_t gid, const float* __restrict__ ip_j, int64_t id_base, int64_t nlabels,
                                              const float* __restrict__ bnorm, int64_t norm_base, int64_t nnorm,
                                              const float* __restrict__ qnorm_q, int metric, const float* __restrict__ qn2_q, int64_t& row) {
    float cs = -INFINITY;
    row = -1;
    const int64_t r = gid - id_base, rn = gid - norm_base;
    if (gid >= 0 && rn >= 0 && rn < nnorm) {
        if (r >= 0 && r < nlabels) row = r;
        const float bn = fmaxf(bnorm[rn], 1e-12f);
        const float qn = fmaxf(*qnorm_q, 1e-12f);
        float ip = *ip_j;
        if (metric == 1) ip = 0.5f * (*qn2_q + bnorm[rn] * bnorm[rn] - ip);   // squared L2 -> inner product
        cs = ip / (qn * bn);
    }
    return cs;
}

// K5 for one (k, beta): the aggregation of query q by one wave (lane 0 .. 63) whose k weights and k label rows live in wgt / rows, LDS
// of the caller's placing (RowT: the width it stores a row index in).
//   logit_j = cosine_j / beta for every neighbour inside the norm table, mx = max_j logit_j,
//   e_j = expf(logit_j - mx), den = lane sums over j = l, l + 64, ... ascending, then the xor butterfly 32 .. 1,
//   w_j = e_j * (den > 0 ? 1 / den : 0), weight 0 for a neighbour whose label row is not here,
//   out_c = one fmaf(w_j, label_j[c], acc) chain over j ascending (C <= 32: per neighbour group g over j = g mod G, groups added in order).
template <bool U16, typename RowT>
__device__ __forceinline__ void k5_body(const void* __restrict__ labels_v, int ls, int wide, int P, int64_t nlabels, int C,
                                        const float* __restrict__ bnorm, int64_t norm_base, int64_t nnorm,
                                        const float* __restrict__ qnorm, const int64_t* __restrict__ idx,
                                        const float* __restrict__ dist, int k, int64_t id_base, int metric,
                                        const float* __restrict__ qn2, float beta, float* __restrict__ out,
                                        int64_t q, int lane, float* wgt, RowT* rows) {
    const unsigned short* counts = reinterpret_cast<const unsigned short*>(labels_v);
    const float Pf = (float)P, Pr = 1.0f / Pf;
    // logits of the k neighbours (lane-strided), running maximum
    float mx = -INFINITY;
    for (int j = lane; j < k; j += 64) {
        int64_t row;
        const float cs = k5_neighbour(idx[q * (int64_t)k + j], dist + q * (int64_t)k + j, id_base, nlabels, bnorm, norm_base, nnorm,
                                      qnorm + q, metric, qn2 + q, row);
        const float logit = cs / beta;      // (a position outside the norm table: -inf / beta = -inf)
        wgt[j] = logit;
        rows[j] = (RowT)row;
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
    // the weights as they enter the sum (attn_j = e_j / den), and row 0 with weight 0 for a neighbour whose label row is not here: the
    // gather below is then branch-free, so that a batch of loads is in flight before the first is used (the kernel is bound by the
    // gather's latency: 90 dependent-looking two-byte loads per lane at C = 151, k = 30 until round 5)
    for (int j = lane; j < k; j += 64) {
        const bool own = rows[j] >= 0;
        wgt[j] = own ? wgt[j] * inv : 0.0f;
        if (!own) rows[j] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to all its lanes
    constexpr int UB = 8;                  // label rows in flight per lane
    if (C <= 32) {
        // few classes (VOC 21, Cityscapes 19, COCO-Stuff 15 ...): G = 64 / C neighbours at a time, lane = (neighbour group g, class c);
        // group g sums the neighbours j = g, g + G, ... in ascending order, the G partial sums are added in group order
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
                lv[u] = in ? k5_label_at<U16>(labels_v, rows[j], ls, c, P, Pf, Pr) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) accv = fmaf(wj[u], lv[u], accv);
        }
        float total = accv;                 // lanes of group 0: + group 1 + group 2 ...
        for (int gg = 1; gg < G; ++gg) total += __shfl(accv, gg * C + c);
        if (g == 0) out[q * (int64_t)C + c] = total;
        return;
    }
    if (U16 && wide) {
        // count rows of 16-byte granules (the index's own table, padded; hb_k5_table_choose checks stride, alignment, P and C): lane l
        // gathers the eight counts 8 l .. 8 l + 7 of a row with ONE 16-byte load -- ceil(C / 8) lanes cover a row (19 of 64 at C = 151),
        // k loads per lane instead of 3 k two-byte ones: the kernel is bound by the number of gather instructions in flight, not by lanes
        // or bytes.  Every class still sums its neighbours in ascending order with the same fmaf chain, so the bits equal the narrow
        // path's (and the fp32 table's).
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
                    raw[u] = *reinterpret_cast<const uint4*>(counts + (int64_t)(j < k ? rows[j] : (RowT)0) * (int64_t)ls + 8 * lane);
                }
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    float lv[8];
                    k5_unpack8(raw[u], Pf, Pr, lv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) a8[i] = fmaf(wj[u], lv[i], a8[i]);
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
                lv[u] = j < k ? k5_label_at<U16>(labels_v, rows[j], ls, cc, P, Pf, Pr) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) accv = fmaf(wj[u], lv[u], accv);
        }
        if (c < C) out[q * (int64_t)C + c] = accv;
    }
}
