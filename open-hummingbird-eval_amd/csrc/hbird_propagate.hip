// Video label propagation (include/hbird_hip_propagate.h, DESIGN.md section 4 "Video label propagation"): the windowed retrieval of one target
// frame against up to 32 context frames of a pool, and the softmax-weighted sum of the neighbours' label rows, in one launch.
//
// propagate_kernel.  A workgroup (8 waves, 4 where d and k leave no room for 8 waves' lists) owns a PG_TH x PG_TW rectangle of 32 query
// cells, clipped at the grid's edges (padded queries take zero tokens and never list anything).  LDS: [the 32 queries' tokens, one row of qstride floats each][per wave: 32 lists of k scores][... of
// k ids].  For every context position the key set is the rectangle grown by the position's radius and clipped (the whole frame for an
// unrestricted one), walked in tiles of 32 keys; the tiles of all positions are dealt to the waves round robin.  One score tile is one
// v_mfma_f32_32x32x2_f32 chain over d, dd ascending: A = the keys (lane l reads row l % 32 of the tile from HBM, 8 consecutive floats per
// four MFMA steps, and feeds dd = 2 s + l / 32), B = the queries (the staged rows are permuted inside every group of 8 floats so that the
// four values a lane feeds are one ds_read_b128).  Lane (n, h) ends with the scores of query n against keys 8 j + 4 h + i; the upper half
// hands its 16 scores to the lower one, and lane n alone pushes into the wave's list of query n (so no two lanes ever write one list).
// The window test, the NaN test and the padding tests mask a score before the push.  The lists are ordered by (score descending, id
// ascending), a total order over distinct ids: what a list holds does not depend on which wave saw a candidate or in which order.
// After one barrier 32 threads merge the waves' lists, write the optional outputs and form the weights by the definition's sequential
// chains; after another, all threads run the label chains.  No atomic, no floating-point reassociation: two calls return the same bits.
#include "../../include/hbird_hip.h"
#include "../../include/hbird_hip_propagate.h"
#include "hbird_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>

// the aggregation is a stated sequence of rounded operations (the fmaf chains are written as fmaf)
#pragma clang fp contract(off)

#define PG_MAX_WAVES 8     // 8 waves where their lists fit beside the staged queries, else 4
#define PG_TH 4
#define PG_TW 8
#define PG_LDS_BYTES (160 * 1024)

static_assert(PG_TH * PG_TW == 32, "one MFMA tile of queries");
static_assert(32 * HB_PROPAGATE_MAX_D * 4 + 4 * 32 * HB_PROPAGATE_MAX_K * 8 <= PG_LDS_BYTES, "the staged queries and the lists fit the LDS");

struct pg_ctx { int slots[HB_PROPAGATE_MAX_CTX]; int radii[HB_PROPAGATE_MAX_CTX]; };
typedef float pg_acc_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool pg_better(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// sorted insertion into a list of k (score, id) pairs that one lane owns; the list's padding is (-inf, INT_MAX)
__device__ __forceinline__ void pg_push(float* S, int* I, int k, float s, int id) {
    if (!(s > -INFINITY)) return;                           // NaN and -inf never enter
    if (!pg_better(s, id, S[k - 1], I[k - 1])) return;
    int j = k - 1;
    while (j > 0 && pg_better(s, id, S[j - 1], I[j - 1])) { S[j] = S[j - 1]; I[j] = I[j - 1]; --j; }
    S[j] = s; I[j] = id;
}

__global__ __launch_bounds__(64 * PG_MAX_WAVES) void propagate_kernel(const float* __restrict__ q, const float* __restrict__ feat_pool,
                                                               const float* __restrict__ label_pool, pg_ctx ctx, int n_ctx, int gh, int gw, int d,
                                                               int c, int k, float temperature, int qstride, int qregion, float* __restrict__ out_labels,
                                                               int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    extern __shared__ __attribute__((aligned(16))) float pg_sm[];
    float* qs = pg_sm;                                      // [32][qstride]; after the search: the final lists and weights
    const int nthreads = blockDim.x, nw = nthreads >> 6;    // 4 or 8 waves
    float* ls = pg_sm + qregion;                            // [nw][32][k]
    int* li = reinterpret_cast<int*>(ls + nw * 32 * k);
    const int N = gh * gw;
    const int tiles_x = (gw + PG_TW - 1) / PG_TW;
    const int ty0 = ((int)blockIdx.x / tiles_x) * PG_TH, tx0 = ((int)blockIdx.x % tiles_x) * PG_TW;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 31, h = lane >> 5;
    const int d4 = d >> 2, g8 = d >> 3;

    // ---- stage the queries: inside a full group of 8 floats position 4 (dd & 1) + (dd >> 1) holds dd; a last group of 4 stays in order
    for (int e = tid; e < 32 * d4; e += nthreads) {
        const int t = e / d4, g4 = e - t * d4;
        const int y = ty0 + t / PG_TW, x = tx0 + t % PG_TW;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (y < gh && x < gw) v = *reinterpret_cast<const float4*>(q + ((int64_t)y * gw + x) * d + 4 * g4);
        float* row = qs + t * qstride;
        if (g4 < 2 * g8) {
            float* p = row + 8 * (g4 >> 1) + ((g4 & 1) ? 2 : 0);
            p[0] = v.x; p[4] = v.y; p[1] = v.z; p[5] = v.w;
        } else {
            *reinterpret_cast<float4*>(row + 4 * g4) = v;
        }
    }
    for (int e = tid; e < nw * 32 * k; e += nthreads) { ls[e] = -INFINITY; li[e] = INT_MAX; }
    __syncthreads();

    const int qy = ty0 + n / PG_TW, qx = tx0 + n % PG_TW;
    const bool qvalid = qy < gh && qx < gw;
    float* myS = ls + (wv * 32 + n) * k;
    int* myI = li + (wv * 32 + n) * k;
    const float* qrow = qs + n * qstride;

    int item = 0;
    for (int f = 0; f < n_ctx; ++f) {
        const int r = ctx.radii[f];                         // (clamped to the grid's larger side by the host: no overflow below)
        const int ya = r < 0 ? 0 : max(ty0 - r, 0), yb = r < 0 ? gh - 1 : min(min(ty0 + PG_TH - 1, gh - 1) + r, gh - 1);
        const int xa = r < 0 ? 0 : max(tx0 - r, 0), xb = r < 0 ? gw - 1 : min(min(tx0 + PG_TW - 1, gw - 1) + r, gw - 1);
        const int KW = xb - xa + 1, cnt = (yb - ya + 1) * KW, nt = (cnt + 31) >> 5;
        const float* fbase = feat_pool + (int64_t)ctx.slots[f] * N * d;
        for (int t = 0; t < nt; ++t, ++item) {
            if ((item & (nw - 1)) != wv) continue;    // wave-uniform
            const int kidx = t * 32 + n, kc = min(kidx, cnt - 1);       // lanes past the key set repeat its last key, masked below
            const int ky = ya + kc / KW, kx = xa + kc % KW;
            const float4* kp = reinterpret_cast<const float4*>(fbase + ((int64_t)ky * gw + kx) * d);
            pg_acc_t acc;
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
            for (int g = 0; g < g8; ++g) {
                const float4 k0 = kp[2 * g], k1 = kp[2 * g + 1];
                const float4 qv = *reinterpret_cast<const float4*>(qrow + 8 * g + 4 * h);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? k0.y : k0.x, qv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? k0.w : k0.z, qv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? k1.y : k1.x, qv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? k1.w : k1.z, qv.w, acc, 0, 0, 0);
            }
            if (d & 4) {
                const float4 k0 = kp[2 * g8];
                const float* qt = qrow + 8 * g8;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? k0.y : k0.x, qt[h], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? k0.w : k0.z, qt[2 + h], acc, 0, 0, 0);
            }
            // acc[4 j + i] of lane (n, h): query n against key 8 j + 4 h + i of the tile
            const int kyv = kidx < cnt ? ky : -1;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m0 = 8 * (v >> 2) + (v & 3), m1 = m0 + 4;
                const float s0 = acc[v], s1 = __shfl_xor(s0, 32);       // (for h == 0: the upper half's score of key m1)
                const int y0 = __shfl(kyv, m0), x0 = __shfl(kx, m0), y1 = __shfl(kyv, m1), x1 = __shfl(kx, m1);
                if (h == 0 && qvalid) {
                    if (y0 >= 0 && (r < 0 || (abs(y0 - qy) <= r && abs(x0 - qx) <= r))) pg_push(myS, myI, k, s0, f * N + y0 * gw + x0);
                    if (y1 >= 0 && (r < 0 || (abs(y1 - qy) <= r && abs(x1 - qx) <= r))) pg_push(myS, myI, k, s1, f * N + y1 * gw + x1);
                }
            }
        }
    }
    __syncthreads();                                        // every wave's lists are complete; the staged queries are no longer read

    // ---- merge, optional outputs, weights: one thread per query
    float* fs = qs;                                         // [32][k] scores
    int* fi = reinterpret_cast<int*>(qs + 32 * k);          // [32][k] ids (-1 past the list's end)
    float* fw = qs + 64 * k;                                // [32][k] weights
    if (tid < 32) {
        const int t = tid;
        const int y = ty0 + t / PG_TW, x = tx0 + t % PG_TW;
        const bool live = y < gh && x < gw;
        const int64_t cell = (int64_t)y * gw + x;
        int p[PG_MAX_WAVES], got = 0;
#pragma unroll
        for (int w = 0; w < PG_MAX_WAVES; ++w) p[w] = 0;
        for (; got < k; ++got) {
            float bs = 0.0f; int bi = INT_MAX, bw = -1;
#pragma unroll
            for (int w = 0; w < PG_MAX_WAVES; ++w) {
                if (w < nw && p[w] < k) {
                    const float s = ls[(w * 32 + t) * k + p[w]];
                    const int i = li[(w * 32 + t) * k + p[w]];
                    if (i != INT_MAX && (bw < 0 || pg_better(s, i, bs, bi))) { bs = s; bi = i; bw = w; }
                }
            }
            if (bw < 0) break;
#pragma unroll
            for (int w = 0; w < PG_MAX_WAVES; ++w) p[w] += bw == w;
            fs[t * k + got] = bs; fi[t * k + got] = bi;
        }
        for (int j = got; j < k; ++j) { fs[t * k + j] = -INFINITY; fi[t * k + j] = -1; }
        if (live && out_idx) {
            for (int j = 0; j < k; ++j) { out_idx[cell * k + j] = fi[t * k + j]; out_score[cell * k + j] = fs[t * k + j]; }
        }
        if (got > 0) {
            const float mx = fs[t * k] / temperature;
            float den = 0.0f;
            for (int j = 0; j < got; ++j) {
                const float e = expf(fs[t * k + j] / temperature - mx);
                fw[t * k + j] = e;
                den = den + e;
            }
            for (int j = 0; j < got; ++j) fw[t * k + j] = fw[t * k + j] / den;
        }
    }
    __syncthreads();

    // ---- the label chains: out[i][ch] = fmaf(w_j, label[id_j][ch], acc) over j ascending
    for (int e = tid; e < 32 * c; e += nthreads) {
        const int t = e / c, ch = e - t * c;
        const int y = ty0 + t / PG_TW, x = tx0 + t % PG_TW;
        if (y >= gh || x >= gw) continue;
        float acc = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int id = fi[t * k + j];
            if (id < 0) break;
            const int f = id / N, cell = id - f * N;
            acc = fmaf(fw[t * k + j], label_pool[((int64_t)ctx.slots[f] * N + cell) * c + ch], acc);
        }
        out_labels[((int64_t)y * gw + x) * c + ch] = acc;
    }
}

extern "C" int hb_propagate_labels(const float* q, const float* feat_pool, const float* label_pool, int pool_slots, const int* slots, const int* radii,
                                   int n_ctx, int gh, int gw, int d, int c, int k, float temperature, float* out_labels, int64_t* out_idx_opt,
                                   float* out_score_opt, void* hip_stream) {
    hb_range range("hbird:propagate_labels");
    const std::string who = "hb_propagate_labels: ";
    if (!q || !feat_pool || !label_pool || !slots || !radii || !out_labels) return hb_fail(who + "NULL pointer");
    if ((out_idx_opt == nullptr) != (out_score_opt == nullptr)) return hb_fail(who + "out_idx_opt and out_score_opt: both or neither (one is a NULL pointer)");
    if (pool_slots <= 0 || n_ctx <= 0 || gh <= 0 || gw <= 0 || d <= 0 || c <= 0 || k <= 0)
        return hb_fail(who + "pool_slots, n_ctx, gh, gw, d, c and k must be positive");
    if (k > HB_PROPAGATE_MAX_K) return hb_fail(who + "k exceeds the limit " + std::to_string(HB_PROPAGATE_MAX_K));
    if (n_ctx > HB_PROPAGATE_MAX_CTX) return hb_fail(who + "n_ctx exceeds the limit " + std::to_string(HB_PROPAGATE_MAX_CTX));
    if (c > HB_PROPAGATE_MAX_C) return hb_fail(who + "c exceeds the limit " + std::to_string(HB_PROPAGATE_MAX_C));
    if (d > HB_PROPAGATE_MAX_D) return hb_fail(who + "d exceeds the limit " + std::to_string(HB_PROPAGATE_MAX_D));
    if (d % 4 != 0) return hb_fail(who + "d must be a multiple of 4, got " + std::to_string(d));
    if ((long long)n_ctx * gh * gw >= (1LL << 31)) return hb_fail(who + "n_ctx * gh * gw exceeds the limit 2^31 - 1");
    if (!(temperature > 0.0f) || !std::isfinite(temperature)) return hb_fail(who + "temperature must be positive and finite");
    if (((uintptr_t)q | (uintptr_t)feat_pool) & 15) return hb_fail(who + "q and feat_pool must be 16-byte aligned");
    pg_ctx ctx;
    const int rmax = std::max(gh, gw);
    for (int f = 0; f < HB_PROPAGATE_MAX_CTX; ++f) { ctx.slots[f] = 0; ctx.radii[f] = 0; }
    for (int f = 0; f < n_ctx; ++f) {
        if (slots[f] < 0 || slots[f] >= pool_slots)
            return hb_fail(who + "slot " + std::to_string(slots[f]) + " at context position " + std::to_string(f) + " is outside [0, " + std::to_string(pool_slots) + ")");
        ctx.slots[f] = slots[f];
        ctx.radii[f] = radii[f] < 0 ? -1 : std::min(radii[f], rmax);    // (a window wider than the grid is the whole grid)
    }
    const long long blocks = (long long)((gh + PG_TH - 1) / PG_TH) * ((gw + PG_TW - 1) / PG_TW);
    if (blocks > 0x7FFFFFFFLL) return hb_fail(who + "grid exceeds the limit of 2^31 - 1 workgroups");
    // the query rows are padded by 4 floats (rows 4 banks apart) wherever that still fits
    // and 8 waves (two per SIMD: one hides the other's loads) wherever their lists still fit
    int qstride = d + 4, waves = PG_MAX_WAVES;
    if (32 * qstride * 4 + waves * 32 * k * 8 > PG_LDS_BYTES) waves = 4;
    if (32 * qstride * 4 + waves * 32 * k * 8 > PG_LDS_BYTES) qstride = d;
    const int lists = waves * 32 * k * 8;
    const int qregion = std::max(32 * qstride, 96 * k);     // floats; the merged lists and weights reuse the region
    const int lds = qregion * 4 + lists;
    if (lds > PG_LDS_BYTES) return hb_fail(who + "d exceeds the limit of the LDS staging");
    if (hb_ensure_dyn_lds((const void*)propagate_kernel, PG_LDS_BYTES)) return -1;
    propagate_kernel<<<dim3((unsigned)blocks), dim3(64 * waves), (size_t)lds, (hipStream_t)hip_stream>>>(
        q, feat_pool, label_pool, ctx, n_ctx, gh, gw, d, c, k, temperature, qstride, qregion, out_labels, out_idx_opt, out_score_opt);
    HB_HIP(hipGetLastError());
    return 0;
}
