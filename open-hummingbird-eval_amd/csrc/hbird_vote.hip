// The weighted vote of the image-level k-NN classifier and the counts behind its accuracies (include/hbird_hip_vote.h, DESIGN.md section 4
// "k-NN classification").  Plain VALU / integer code; no MFMA, no floating-point atomic.
//
// knn_vote_kernel (hb_knn_vote): a workgroup owns one query's list (thread t holds positions t, t + 256, ...: SLOTS of them).  The list's
// classes and scores are staged in LDS.  A LEADER SCAN gathers the votes: the first position of a class (its leader) walks the list once,
// adding the e of every position of its class in ascending j -- the stated chain -- and notes the sum every time the walk passes one of the
// ks: the chain of a smaller k is a prefix of the chain of a larger k.  Nothing is sized by the class count.  Leaders are numbered in list
// order, so the classes present in the first k positions are the first s_nl[ik] leaders; each of them counts the leaders that beat it
// (vote descending, ties to the lower class) and, where fewer than topn do, writes its class into that slot.  Every output word has one
// writer.
//
// vote_check_kernel + vote_counts_kernel (hb_vote_counts): one thread per (configuration, query) finds the slot of the query's label among
// the predictions; hits meet in LDS integers, then one integer atomicAdd per slot and workgroup.
#include "../../include/hbird_hip_vote.h"
#include "hbird_internal.h"
#include <cmath>

// the logit, its shift and the chain are stated sequences of rounded fp32 operations
#pragma clang fp contract(off)

#define VT_THREADS 256

struct vote_grid {
    int ks[HB_VOTE_MAX_CONFIGS];
    float temps[HB_VOTE_MAX_CONFIGS];
    int nk, nt;
};

template <int SLOTS>
__global__ __launch_bounds__(VT_THREADS) void knn_vote_kernel(const int64_t* __restrict__ idx, const float* __restrict__ score, int64_t nq, int k_list,
                                                              int64_t id_base, const int32_t* __restrict__ labels, int64_t n_rows, vote_grid g, int topn,
                                                              int32_t* __restrict__ pred, float* __restrict__ votes) {
    constexpr int CAP = SLOTS * VT_THREADS;                 // k_list <= CAP
    __shared__ int s_cls[CAP];                              // the class of a position that takes part, -1 otherwise
    __shared__ float s_sc[CAP], s_e[CAP];
    __shared__ int s_lead[CAP];                             // 1: the first position of its class
    __shared__ int s_lcls[CAP];                             // leaders in list order: their classes ...
    __shared__ float s_vote[CAP];                           // ... and their votes in the configuration at hand
    __shared__ int s_ks[HB_VOTE_MAX_CONFIGS], s_nl[HB_VOTE_MAX_CONFIGS];
    __shared__ float s_temp[HB_VOTE_MAX_CONFIGS];
    __shared__ int s_first;
    const int tid = threadIdx.x, nk = g.nk, nt = g.nt;
    if (tid < HB_VOTE_MAX_CONFIGS) { s_ks[tid] = g.ks[tid]; s_temp[tid] = g.temps[tid]; }
    for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        __syncthreads();
        if (tid == 0) s_first = k_list;
#pragma unroll
        for (int p = 0; p < SLOTS; ++p) {
            const int j = p * VT_THREADS + tid;
            if (j < k_list) {
                const int64_t id = idx[q * k_list + j];
                int c = -1;
                if (id >= 0) {
                    const int64_t row = id - id_base;
                    if (row >= 0 && row < n_rows) c = max(labels[row], -1);
                }
                s_cls[j] = c;
                s_sc[j] = score[q * k_list + j];
            }
        }
        __syncthreads();
        int cls[SLOTS], li[SLOTS];
        bool lead[SLOTS];
#pragma unroll
        for (int p = 0; p < SLOTS; ++p) {
            const int j = p * VT_THREADS + tid;
            cls[p] = j < k_list ? s_cls[j] : -1;
            bool ld = cls[p] >= 0;
            for (int i = 0; i < j && ld; ++i)
                if (s_cls[i] == cls[p]) ld = false;
            lead[p] = ld;
            if (j < k_list) s_lead[j] = ld ? 1 : 0;
            if (ld) atomicMin(&s_first, j);                 // the first position that takes part leads its class
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < SLOTS; ++p) {
            li[p] = 0;
            if (lead[p]) {
                const int j = p * VT_THREADS + tid;
                int n = 0;
                for (int i = 0; i < j; ++i) n += s_lead[i];
                li[p] = n;
                s_lcls[n] = cls[p];
            }
        }
        if (tid < nk) {
            int n = 0;
            for (int i = 0; i < s_ks[tid]; ++i) n += s_lead[i];
            s_nl[tid] = n;
        }
        __syncthreads();
        const int first = s_first;
        for (int it = 0; it < nt; ++it) {
            const float T = s_temp[it];
            const float mx = first < k_list ? s_sc[first] / T : 0.0f;
#pragma unroll
            for (int p = 0; p < SLOTS; ++p) {
                const int j = p * VT_THREADS + tid;
                if (j < k_list) s_e[j] = cls[p] >= 0 ? expf(s_sc[j] / T - mx) : 0.0f;
            }
            __syncthreads();
            float acc[SLOTS];
#pragma unroll
            for (int p = 0; p < SLOTS; ++p) acc[p] = 0.0f;
            int at = 0;
            for (int ik = 0; ik < nk; ++ik) {
                const int kk = s_ks[ik], nl = s_nl[ik];
#pragma unroll
                for (int p = 0; p < SLOTS; ++p) {
                    if (!lead[p]) continue;
                    float a = acc[p];
                    for (int i = at; i < kk; ++i)
                        if (s_cls[i] == cls[p]) a = a + s_e[i];
                    acc[p] = a;
                    if (p * VT_THREADS + tid < kk) s_vote[li[p]] = a;
                }
                at = kk;
                __syncthreads();
                const int64_t base = ((int64_t)(ik * nt + it) * nq + q) * topn;
#pragma unroll
                for (int p = 0; p < SLOTS; ++p) {
                    if (!lead[p] || p * VT_THREADS + tid >= kk) continue;
                    const float v = acc[p];
                    int beat = 0;
                    for (int m = 0; m < nl; ++m) {
                        const float vm = s_vote[m];
                        beat += (vm > v || (vm == v && s_lcls[m] < cls[p])) ? 1 : 0;
                    }
                    if (beat < topn) {
                        pred[base + beat] = cls[p];
                        if (votes) votes[base + beat] = v;
                    }
                }
                if (tid < topn && tid >= nl) {              // fewer classes than slots: the tail
                    pred[base + tid] = -1;
                    if (votes) votes[base + tid] = 0.0f;
                }
                __syncthreads();
            }
        }
    }
}

extern "C" int hb_knn_vote(const int64_t* idx, const float* score, int64_t nq, int k_list, int64_t id_base, const int32_t* labels, int64_t n_rows, int C,
                           const int* ks, int nk, const float* temps, int nt, int topn, int32_t* pred, float* votes_opt, void* hip_stream) {
    hb_range range("hbird:knn_vote");
    const std::string who = "hb_knn_vote: ";
    if (!idx || !score || !labels || !pred || !ks || !temps) return hb_fail(who + "NULL pointer");
    if (nq < 0 || n_rows < 0) return hb_fail(who + "nq and n_rows must not be negative");
    if (k_list < 1 || k_list > HB_VOTE_MAX_K) return hb_fail(who + "k_list outside [1, " + std::to_string(HB_VOTE_MAX_K) + "]: limit");
    if (nk < 1 || nt < 1 || (long long)nk * nt > HB_VOTE_MAX_CONFIGS)
        return hb_fail(who + "nk and nt must be positive and nk * nt within the limit of " + std::to_string(HB_VOTE_MAX_CONFIGS) + " configurations");
    if (topn < 1 || topn > HB_VOTE_MAX_TOP) return hb_fail(who + "topn outside [1, " + std::to_string(HB_VOTE_MAX_TOP) + "]");
    if (C < 1) return hb_fail(who + "C must be positive (classes)");
    vote_grid g = {};
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1 || (i > 0 && ks[i] <= ks[i - 1])) return hb_fail(who + "ks must be strictly ascending and start at 1 or above");
        g.ks[i] = ks[i];
    }
    if (ks[nk - 1] > k_list) return hb_fail(who + "ks: the largest k " + std::to_string(ks[nk - 1]) + " exceeds k_list " + std::to_string(k_list));
    for (int i = 0; i < nt; ++i) {
        if (!(temps[i] > 0.0f) || !std::isfinite(temps[i])) return hb_fail(who + "temperature must be positive and finite");
        g.temps[i] = temps[i];
    }
    g.nk = nk; g.nt = nt;
    if (nq == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)std::min<int64_t>(nq, 1 << 20)), block(VT_THREADS);
    if (k_list <= VT_THREADS)
        knn_vote_kernel<1><<<grid, block, 0, s>>>(idx, score, nq, k_list, id_base, labels, n_rows, g, topn, pred, votes_opt);
    else if (k_list <= 2 * VT_THREADS)
        knn_vote_kernel<2><<<grid, block, 0, s>>>(idx, score, nq, k_list, id_base, labels, n_rows, g, topn, pred, votes_opt);
    else
        knn_vote_kernel<HB_VOTE_MAX_K / VT_THREADS><<<grid, block, 0, s>>>(idx, score, nq, k_list, id_base, labels, n_rows, g, topn, pred, votes_opt);
    HB_HIP(hipGetLastError());
    return 0;
}

// ---- the counts ----------------------------------------------------------------------------------------------------------------------------
// *flag |= 1 for a query label outside [-1, C)
__global__ __launch_bounds__(256) void vote_check_kernel(const int32_t* __restrict__ qlabels, int64_t nq, int C, int32_t* __restrict__ flag) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const int32_t lab = qlabels[q];
    if (lab < -1 || lab >= C) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void vote_counts_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ qlabels, int64_t nq, int topn, int C,
                                                          unsigned long long* __restrict__ counts, unsigned long long* __restrict__ class_io,
                                                          unsigned long long* __restrict__ n_io) {
    __shared__ unsigned hit[HB_VOTE_MAX_TOP + 1];           // hit[t]: labels found at slot t; hit[HB_VOTE_MAX_TOP]: labelled queries
    const int tid = threadIdx.x, cfg = blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * 256 + tid;
    if (tid <= HB_VOTE_MAX_TOP) hit[tid] = 0;
    __syncthreads();
    if (q < nq) {
        const int32_t lab = qlabels[q];
        if (lab >= 0) {
            const int32_t* row = pred + ((int64_t)cfg * nq + q) * topn;
            atomicAdd(&hit[HB_VOTE_MAX_TOP], 1u);
            for (int t = 0; t < topn; ++t)
                if (row[t] == lab) { atomicAdd(&hit[t], 1u); break; }
            if (class_io) {
                unsigned long long* cell = class_io + ((int64_t)cfg * C + lab) * 2;
                atomicAdd(cell, 1ull);
                if (row[0] == lab) atomicAdd(cell + 1, 1ull);
            }
        }
    }
    __syncthreads();
    if (tid < topn) {
        unsigned n = 0;
        for (int t = 0; t <= tid; ++t) n += hit[t];         // the label is among pred[0 .. tid]
        if (n) atomicAdd(counts + (int64_t)cfg * topn + tid, (unsigned long long)n);
    }
    if (tid == HB_VOTE_MAX_TOP && cfg == 0 && hit[HB_VOTE_MAX_TOP]) atomicAdd(n_io, (unsigned long long)hit[HB_VOTE_MAX_TOP]);
}

extern "C" int hb_vote_counts(const int32_t* pred, const int32_t* qlabels, int64_t nq, int n_cfg, int topn, int C, int64_t* counts_io,
                              int64_t* class_io_opt, int64_t* n_io, void* hip_stream) {
    hb_range range("hbird:vote_counts");
    const std::string who = "hb_vote_counts: ";
    if (!pred || !qlabels || !counts_io || !n_io) return hb_fail(who + "NULL pointer");
    if (nq < 0) return hb_fail(who + "nq must not be negative");
    if (n_cfg < 1 || n_cfg > HB_VOTE_MAX_CONFIGS) return hb_fail(who + "n_cfg outside the limit [1, " + std::to_string(HB_VOTE_MAX_CONFIGS) + "] configurations");
    if (topn < 1 || topn > HB_VOTE_MAX_TOP) return hb_fail(who + "topn outside [1, " + std::to_string(HB_VOTE_MAX_TOP) + "]");
    if (C < 1) return hb_fail(who + "C must be positive (classes)");
    if (nq == 0) return 0;
    const int64_t blocks = (nq + 255) / 256;
    if (blocks > 0x7FFFFFFFLL) return hb_fail(who + "launch grid exceeds the limit (nq / 256 workgroups)");
    hipStream_t s = (hipStream_t)hip_stream;
    hb_dev<int32_t> flag;                                   // a local of this call
    if (flag.ensure(256, HB_GROW_EXACT)) return -1;
    HB_HIP(hipMemsetAsync(flag, 0, 4, s));
    vote_check_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(qlabels, nq, C, flag);
    HB_HIP(hipGetLastError());
    int32_t bad = 0;
    HB_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));
    if (bad) return hb_fail(who + "a query label lies outside [-1, " + std::to_string(C) + ")");
    vote_counts_kernel<<<dim3((unsigned)blocks, (unsigned)n_cfg), dim3(256), 0, s>>>(pred, qlabels, nq, topn, C,
                                                                                    reinterpret_cast<unsigned long long*>(counts_io),
                                                                                    reinterpret_cast<unsigned long long*>(class_io_opt),
                                                                                    reinterpret_cast<unsigned long long*>(n_io));
    HB_HIP(hipGetLastError());
    return 0;
}
