// K5 over a grid of (k, beta) configurations from ONE neighbour list per query ("Evaluation grids").
//
// The engine's lists are the exact top-k under one total order (score descending, id ascending) with deterministic score bits, so the
// best k of a query are the first k entries of its best k_max: one search at the largest k serves every smaller k, and beta only
// enters after the search.  aggregate_grid_kernel is aggregate_kernel (hbird_aggregate.hip; k5_body of hbird_k5_dev.h, which also holds
// the neighbour resolution and the count decode used here) applied to the first k POSITIONS of the
// list for every configuration (k, beta) of the grid -- whatever those positions hold: -1 entries, ids outside the norm table, repeated
// ids -- and agrees with it bit for bit.  That fixes the arithmetic order, configuration by configuration:
//   c_j = ip_j / (max(|q|, 1e-12) max(|b_j|, 1e-12)) once per neighbour (L2: ip = 0.5 (qn2 + bn^2 - dist)), logit = c_j / beta,
//   mx = max over the prefix, e_j = expf(logit - mx), lane l sums e_j over j = l, l + 64, ... ascending, the xor butterfly 32 .. 1
//   completes den, w_j = e_j * (den > 0 ? 1 / den : 0) and 0 where the label row is not in the table, out_c = one fmaf(w_j, label_j[c], acc)
//   chain over j ascending (C <= 32: per neighbour group g over j = g mod G, the group sums added in group order).
// What the grid shares is everything that does not depend on the configuration: the list is read once, the cosines and rows are worked
// out once, and the gather loop loads every label row ONCE (and converts its counts once) and feeds the accumulators of all
// configurations -- G configurations cost one launch and one gather, not G.  A position beyond a configuration's k is predicated out
// of its accumulator (not multiplied by a zero weight: an fp32 table may hold a non-finite value).
//
// Shape: aggregate_bigk_kernel's (hbird_aggregate.hip) -- a workgroup IS one wave with dynamic LDS: kmax cosines and 32-bit rows plus NC
// weights per position, 4 (2 + NC) kmax bytes = 18 KiB at 256 x 16.  The weights of one position are contiguous (w[j][cfg]): the gather
// loop fetches them with 16-byte LDS reads at an address all lanes (wide / generic body) or all lanes of a neighbour group share.
// The configurations are a template parameter (4 / 8 / 12 / 16 accumulator sets, a smaller grid padded with weights of zero) so that
// the accumulators are registers: 8 x 16 = 128 VGPRs in the wide body, no scratch (profiles/r12/README.md has the resource report).
#include "hbird_internal.h"
#include "../../include/hbird_hip.h"
#include "hbird_k5_dev.h"
#include <cmath>

template <bool U16, int NC>
__global__ __launch_bounds__(64) void aggregate_grid_kernel(const void* __restrict__ labels_v, int ls, int wide, int P, int64_t nlabels, int C,
                                                            const float* __restrict__ bnorm, int64_t norm_base, int64_t nnorm,
                                                            const float* __restrict__ qnorm,
                                                            const int64_t* __restrict__ idx,
                                                            const float* __restrict__ dist, int64_t nq, int k_list,
                                                            int64_t id_base, int metric, const float* __restrict__ qn2,
                                                            hb_grid_spec gs, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char grid_smem[];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const unsigned short* counts = reinterpret_cast<const unsigned short*>(labels_v);
    const float Pf = (float)P, Pr = 1.0f / Pf;
    if (q >= nq) return;
    const int nk = gs.nk, nb = gs.nb, ncfg = nk * nb;
    const int kmax = gs.ks[nk - 1];                                  // <= k_list: positions beyond it belong to no configuration
    float* wgt = reinterpret_cast<float*>(grid_smem);                // [kmax][NC]: the weights of position j, configuration by configuration
    float* cosv = wgt + (size_t)kmax * NC;                           // [kmax] cosines; later (an int's bits) the first configuration position j belongs to
    int* rows = reinterpret_cast<int*>(cosv + kmax);                 // [kmax]
    // the cosine and the label row of every position, once (lane-strided: lane l owns the positions l, l + 64, ... in every phase below)
    for (int j = lane; j < kmax; j += 64) {
        int64_t row;
        cosv[j] = k5_neighbour(idx[q * (int64_t)k_list + j], dist + q * (int64_t)k_list + j, id_base, nlabels, bnorm, norm_base, nnorm,
                               qnorm + q, metric, qn2 + q, row);
        rows[j] = (int)row;
    }
    // the softmax of every configuration over its prefix: aggregate_kernel's three passes, lane sums and butterflies
    for (int ik = 0; ik < nk; ++ik) {
        const int k = gs.ks[ik];
        for (int ib = 0; ib < nb; ++ib) {
            const float beta = gs.betas[ib];
            const int cfg = ik * nb + ib;
            float mx = -INFINITY;
            for (int j = lane; j < k; j += 64) mx = fmaxf(mx, cosv[j] / beta);      // (a position outside the norm table: -inf / beta = -inf)
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float den = 0.0f;
            for (int j = lane; j < k; j += 64) {
                const float logit = cosv[j] / beta;
                const float e = logit > -INFINITY ? expf(logit - mx) : 0.0f;       // every neighbour with a norm takes part (owned or not)
                wgt[j * NC + cfg] = e;
                den += e;
            }
            for (int o = 32; o > 0; o >>= 1) den += __shfl_xor(den, o);
            const float inv = den > 0.0f ? 1.0f / den : 0.0f;
            for (int j = lane; j < k; j += 64) wgt[j * NC + cfg] = rows[j] >= 0 ? wgt[j * NC + cfg] * inv : 0.0f;
        }
    }
    // row 0 for a neighbour whose label row is not here (weight 0 above: the gather is branch-free, as aggregate_kernel's), the first
    // configuration each position belongs to -- position j is inside the prefixes of the configurations cfg >= first(j), the ks being
    // ascending --, and zero weights for the accumulator sets beyond the grid
    for (int j = lane; j < kmax; j += 64) {
        if (rows[j] < 0) rows[j] = 0;
        int f = 0;
        for (int ik = 0; ik < nk; ++ik) f += gs.ks[ik] <= j ? nb : 0;
        cosv[j] = __int_as_float(f);
        for (int cfg = ncfg; cfg < NC; ++cfg) wgt[j * NC + cfg] = 0.0f;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to all its lanes
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // ... and the compiler keeps the gather's LDS reads behind them (no instruction)
    auto label_at = [&](int64_t rj, int c) -> float { return k5_label_at<U16>(labels_v, rj, ls, c, P, Pf, Pr); };
    const size_t slab = (size_t)nq * C;   // out[cfg][nq][C]
    constexpr int UB = 8;                 // label rows in flight per lane
    if (C <= 32) {
        // lane = (neighbour group g, class c): group g sums the neighbours j = g, g + G, ... ascending, the G partial sums are added in group order
        const int G = 64 / C, g = lane / C, c = lane - g * C;
        const bool act = g < G;
        float acc[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) acc[n] = 0.0f;
        for (int j0 = 0; j0 < kmax; j0 += G * UB) {
            float lv[UB];
            int jj[UB], fj[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + u * G + g;
                const bool in = act && j < kmax;
                jj[u] = in ? j : 0;
                fj[u] = in ? __float_as_int(cosv[j]) : NC;
                lv[u] = in ? label_at(rows[j], c) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const float4* w4 = reinterpret_cast<const float4*>(wgt + jj[u] * NC);
#pragma unroll
                for (int n4 = 0; n4 < NC / 4; ++n4) {
                    const float4 w = w4[n4];
                    const float ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int n = n4 * 4 + i;
                        acc[n] = n >= fj[u] ? fmaf(ws[i], lv[u], acc[n]) : acc[n];
                    }
                }
            }
        }
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            float total = acc[n];
            for (int gg = 1; gg < G; ++gg) total += __shfl(acc[n], gg * C + c);
            if (g == 0 && n < ncfg) out[n * slab + q * (int64_t)C + c] = total;
        }
        return;
    }
    if (U16 && wide) {
        // count rows of 16-byte granules: lane l gathers the eight counts 8 l .. 8 l + 7 of a row with one 16-byte load
        const int nl = (C + 7) >> 3;
        float a8[NC][8];
#pragma unroll
        for (int n = 0; n < NC; ++n)
#pragma unroll
            for (int i = 0; i < 8; ++i) a8[n][i] = 0.0f;
        if (lane < nl) {
            for (int j0 = 0; j0 < kmax; j0 += UB) {
                uint4 raw[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int j = j0 + u;
                    raw[u] = *reinterpret_cast<const uint4*>(counts + (int64_t)(j < kmax ? rows[j] : 0) * (int64_t)ls + 8 * lane);
                }
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int j = j0 + u;
                    const int fj = j < kmax ? __float_as_int(cosv[j]) : NC;
                    float lv[8];
                    k5_unpack8(raw[u], Pf, Pr, lv);
                    const float4* w4 = reinterpret_cast<const float4*>(wgt + (j < kmax ? j : 0) * NC);
#pragma unroll
                    for (int n4 = 0; n4 < NC / 4; ++n4) {
                        const float4 w = w4[n4];
                        const float ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int n = n4 * 4 + t;
                            if (n >= fj) {
#pragma unroll
                                for (int i = 0; i < 8; ++i) a8[n][i] = fmaf(ws[t], lv[i], a8[n][i]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < NC; ++n)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (n < ncfg && 8 * lane + i < C) out[n * slab + q * (int64_t)C + 8 * lane + i] = a8[n][i];
        }
        return;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const int cc = c < C ? c : C - 1;   // lanes past the last class repeat it (no store)
        float acc[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) acc[n] = 0.0f;
        for (int j0 = 0; j0 < kmax; j0 += UB) {
            float lv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + u;
                lv[u] = j < kmax ? label_at(rows[j], cc) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + u;
                const int fj = j < kmax ? __float_as_int(cosv[j]) : NC;
                const float4* w4 = reinterpret_cast<const float4*>(wgt + (j < kmax ? j : 0) * NC);
#pragma unroll
                for (int n4 = 0; n4 < NC / 4; ++n4) {
                    const float4 w = w4[n4];
                    const float ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int n = n4 * 4 + i;
                        acc[n] = n >= fj ? fmaf(ws[i], lv[u], acc[n]) : acc[n];
                    }
                }
            }
        }
#pragma unroll
        for (int n = 0; n < NC; ++n)
            if (c < C && n < ncfg) out[n * slab + q * (int64_t)C + c] = acc[n];
    }
}

// The grid of a call, checked before anything is launched: ks strictly ascending in [1, min(k_list, 256)], betas finite and positive,
// at most HB_GRID_MAX_CONFIGS configurations.  k_list < 0: the list is the search's own (hb_index_search_aggregate_grid), k_list = ks[nk - 1].
int hb_grid_check(const char* who, const int* ks, int nk, const float* betas, int nb, int k_list, hb_grid_spec* gs) {
    const std::string w(who);
    if (!ks || !betas) return hb_fail(w + ": ks / betas is NULL");
    if (nk < 1 || nb < 1) return hb_fail(w + ": the grid needs at least one k and one beta");
    if ((int64_t)nk * nb > HB_GRID_MAX_CONFIGS)
        return hb_fail(w + ": " + std::to_string((int64_t)nk * nb) + " configurations, at most " + std::to_string(HB_GRID_MAX_CONFIGS) + " per call (nk * nb)");
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1) return hb_fail(w + ": every k must be positive");
        if (i && ks[i] <= ks[i - 1]) return hb_fail(w + ": ks must be strictly ascending (no repeats)");
    }
    if (ks[nk - 1] > HB_MAX_K_AGGREGATE)
        return hb_fail(w + ": the largest k must be <= " + std::to_string(HB_MAX_K_AGGREGATE) + " (beyond it: hb_bigk_aggregate on prefixes of the list)");
    if (k_list >= 0 && (k_list < 1 || k_list > HB_MAX_K_AGGREGATE)) return hb_fail(w + ": k_list must be in [1, " + std::to_string(HB_MAX_K_AGGREGATE) + "]");
    if (k_list >= 0 && ks[nk - 1] > k_list) return hb_fail(w + ": the largest k exceeds k_list, the length of the given lists");
    for (int i = 0; i < nb; ++i)
        if (!(betas[i] > 0.f) || !std::isfinite(betas[i])) return hb_fail(w + ": every beta must be finite and positive");
    if (gs) {
        *gs = hb_grid_spec{};
        gs->nk = nk; gs->nb = nb;
        for (int i = 0; i < nk; ++i) gs->ks[i] = ks[i];
        for (int i = 0; i < nb; ++i) gs->betas[i] = betas[i];
    }
    return 0;
}

template <int NC, typename... A>
static void launch_grid_nc(bool u16, dim3 grid, int kmax, hipStream_t s, A... a) {
    (u16 ? aggregate_grid_kernel<true, NC> : aggregate_grid_kernel<false, NC>)<<<grid, dim3(64), (size_t)kmax * 4 * (2 + NC), s>>>(a...);
}

template <typename... A>
static void launch_grid(int ncfg, A... a) {
    if (ncfg <= 4) launch_grid_nc<4>(a...);
    else if (ncfg <= 8) launch_grid_nc<8>(a...);
    else if (ncfg <= 12) launch_grid_nc<12>(a...);
    else launch_grid_nc<16>(a...);
}

// The index's own rows (fp32 or counts) or a borrowed table (hb_k5_table_choose); the grid has no label-sharded form.
int hb_launch_aggregate_grid(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq, int k_list,
                             int64_t id_base, const hb_grid_spec& gs, float* out, hipStream_t s) {
    if (nq == 0) return 0;
    if (nq > 0x7FFFFFFFLL) return hb_fail("hb_index_aggregate_grid: more than 2^31 - 1 queries in one call");
    hb_k5_table t;
    if (hb_k5_table_choose(ix, id_base, nullptr, 0, "hb_index_aggregate_grid", &t)) return -1;
    if (t.nlabels > 0x7FFFFFFFLL) return hb_fail("hb_index_aggregate_grid: label tables of more than 2^31 - 1 rows are not supported");
    const dim3 grid((unsigned)nq);
    const int ncfg = gs.nk * gs.nb, kmax = gs.ks[gs.nk - 1];
    launch_grid(ncfg, t.u16, grid, kmax, s, t.labels, t.ls, t.wide, t.P, t.nlabels, ix->lab.classes(), t.bnorm, t.norm_base, t.nnorm, qnorm, idx, dist, nq, k_list, t.id_base,
                ix->metric, (const float*)ix->q_aux, gs, out);
    HB_HIP(hipGetLastError());
    return 0;
}
