// Searches that exclude one group of bank rows per query (include/hbird_hip_exclude.h): leave-one-image-out evaluation of a bank on its own
// training images, where a query must not retrieve the patches of the image it came from.
//
// The kNN kernels are not touched.  A search returns the exact top-k under one total order (score descending, id ascending) with score bits
// that do not depend on k, so the best k rows outside a group of at most gmax rows are the first k non-excluded entries of the best k + gmax
// rows, bit for bit.  An excluding search is therefore hb_index_search at kf = a rung (hbird_calibrate.cpp: hb_exclude_plan) into a workspace
// list, followed by the filter below; where rung 0 is shorter than k + gmax, the queries it leaves incomplete are compacted in ascending order,
// searched again at k + gmax and scattered back.
//
// The kernels move a few KiB per query and are bound by the latency of two dependent loads (id, then its group): one wave per query, 64
// entries per step, no LDS.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>

// One wave per query.  The list is walked in chunks of 64 entries; a lane keeps its entry when id >= 0 and its row is outside the table
// (kept, never dereferenced) or belongs to another group than the query's.  Ballot + prefix popcount + the running count of the chunks before
// make the compaction stable: the list's order survives.  The first k survivors are written verbatim, the tail is -1 / pad.
// complete = the list held k survivors, or a negative id (the bank had no more rows to give: a longer list would add nothing).
__global__ __launch_bounds__(256) void exclude_filter_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist, int64_t nq, int k_list,
                                                             int64_t id_base, const int32_t* __restrict__ groups, int64_t n_rows,
                                                             const int32_t* __restrict__ qgroups, int k, float pad,
                                                             int64_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                             int32_t* __restrict__ complete, int32_t* __restrict__ incomplete) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                       // (whole waves leave: the ballots below see full waves)
    const int32_t qg = qgroups[qi];
    const int64_t* li = idx + qi * (int64_t)k_list;
    const float* ld = dist + qi * (int64_t)k_list;
    int64_t* oi = out_idx + qi * (int64_t)k;
    float* od = out_dist + qi * (int64_t)k;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int kept = 0;
    bool exhausted = false;
    for (int c0 = 0; c0 < k_list && kept < k; c0 += 64) {
        const int p = c0 + lane;
        const bool in_list = p < k_list;
        const int64_t id = in_list ? li[p] : -1;
        const float v = in_list ? ld[p] : 0.0f;
        bool keep = in_list && id >= 0;
        if (keep && qg >= 0) {
            const int64_t row = id - id_base;
            if (row >= 0 && row < n_rows) keep = groups[row] != qg;
        }
        const unsigned long long gone = __ballot(in_list && id < 0);
        exhausted = exhausted || gone != 0ull;
        const unsigned long long m = __ballot(keep);
        const int dst = kept + __popcll(m & lt);
        if (keep && dst < k) { oi[dst] = id; od[dst] = v; }
        kept += __popcll(m);
    }
    for (int j = (kept < k ? kept : k) + lane; j < k; j += 64) { oi[j] = -1; od[j] = pad; }
    if (lane == 0) {
        const bool done = kept >= k || exhausted;
        if (complete) complete[qi] = done ? 1 : 0;
        if (incomplete && !done) atomicAdd(incomplete, 1);
    }
}

// The sizes of the groups of a row-group table (counts[n_groups], zeroed by the caller) and its validation: bit 0 of *flag for a value outside
// [-1, n_groups).  A wave adds every distinct value once (rows of one group are mostly neighbours: one or two atomics per wave).
__global__ __launch_bounds__(256) void exclude_group_sizes_kernel(const int32_t* __restrict__ groups, int64_t n, int32_t n_groups,
                                                                  int32_t* __restrict__ counts, int32_t* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t g = t < n ? groups[t] : -1;
    if (g < -1 || g >= n_groups) atomicOr(flag, 1);
    unsigned long long todo = __ballot(g >= 0 && g < n_groups);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t g0 = __shfl(g, leader);
        const unsigned long long same = __ballot(g == g0) & todo;
        if (lane == leader) atomicAdd(&counts[g0], (int32_t)__popcll(same));
        todo &= ~same;
    }
}

// bit 0 of *flag: a query group outside [-1, n_groups)
__global__ __launch_bounds__(256) void exclude_check_qgroups_kernel(const int32_t* __restrict__ qgroups, int64_t nq, int32_t n_groups,
                                                                    int32_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq) return;
    const int32_t g = qgroups[t];
    if (g < -1 || g >= n_groups) atomicOr(flag, 1);
}

// The incomplete queries in ascending order: rows[j] = the j-th query with complete == 0, qg_out[j] = its group.  ONE workgroup walks the flags
// 256 at a time (ballot per wave, the four wave totals through LDS, a running base): the order is the queries' own, whatever the hardware does.
__global__ __launch_bounds__(256) void exclude_compact_kernel(const int32_t* __restrict__ complete, const int32_t* __restrict__ qgroups, int64_t nq,
                                                              int64_t* __restrict__ rows, int32_t* __restrict__ qg_out) {
    __shared__ int wave_sum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t base = 0;
    for (int64_t c0 = 0; c0 < nq; c0 += 256) {
        const int64_t i = c0 + threadIdx.x;
        const bool inc = i < nq && complete[i] == 0;
        const unsigned long long m = __ballot(inc);
        if (lane == 0) wave_sum[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int c = wave_sum[w]; total += c; if (w < wv) before += c; }
        if (inc) {
            const int64_t p = base + before + __popcll(m & ((1ull << lane) - 1ull));
            rows[p] = i;
            qg_out[p] = qgroups[i];
        }
        base += total;
        __syncthreads();
    }
}

int hb_launch_exclude_filter(const int64_t* idx, const float* dist, int64_t nq, int k_list, int64_t id_base, const int32_t* groups, int64_t n_rows,
                             const int32_t* qgroups, int k, float pad, int64_t* out_idx, float* out_dist, int32_t* complete_opt, int32_t* incomplete_opt,
                             hipStream_t s) {
    if (nq == 0) return 0;
    exclude_filter_kernel<<<dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s>>>(idx, dist, nq, k_list, id_base, groups, n_rows, qgroups, k, pad, out_idx,
                                                                              out_dist, complete_opt, incomplete_opt);
    HB_HIP(hipGetLastError());
    return 0;
}

extern "C" int hb_exclude_filter(const int64_t* idx, const float* dist, int64_t nq, int k_list, int64_t id_base, const int32_t* groups,
                                 int64_t n_rows, const int32_t* qgroups, int k, float pad, int64_t* out_idx, float* out_dist,
                                 int32_t* out_complete, void* hip_stream) {
    if (nq < 0) return hb_fail("hb_exclude_filter: negative query count");
    if (n_rows < 0) return hb_fail("hb_exclude_filter: negative row count");
    if (k_list < 1 || k_list > HB_MAX_K) return hb_fail("hb_exclude_filter: k_list must be in [1, " + std::to_string(HB_MAX_K) + "]");
    if (k < 1 || k > HB_MAX_K) return hb_fail("hb_exclude_filter: k must be in [1, " + std::to_string(HB_MAX_K) + "]");
    if (nq == 0) return 0;
    if (!idx || !dist || !qgroups || !out_idx || !out_dist || (n_rows > 0 && !groups)) return hb_fail("hb_exclude_filter: NULL pointer");
    return hb_launch_exclude_filter(idx, dist, nq, k_list, id_base, groups, n_rows, qgroups, k, pad, out_idx, out_dist, out_complete, nullptr,
                                    (hipStream_t)hip_stream);
}

extern "C" int hb_index_set_row_groups(hb_index_t* ix, const int32_t* groups, int64_t n, int32_t n_groups, int on_device) {
    if (!ix) return hb_fail("hb_index_set_row_groups: NULL index handle");
    if (n < 0) return hb_fail("hb_index_set_row_groups: negative row count");
    if (!groups || n == 0) { ix->row_groups_n = 0; ix->n_groups = 0; ix->gmax = 0; return 0; }
    if (n_groups < 0) return hb_fail("hb_index_set_row_groups: negative group count");
    HB_HIP(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    // the new table is built beside the old one: a failing call (a value outside the range) leaves the index as it was
    hb_dev<int32_t> tab;
    if (tab.ensure((size_t)n * 4, HB_GROW_EXACT)) return -1;
    const size_t cb = ((size_t)n_groups + 1) * 4;       // counts[n_groups], flag
    if (ix->excl.ensure(al256(cb), HB_GROW_EXACT)) return -1;
    int32_t* counts = ix->excl.as<int32_t>();
    hipError_t e = hipMemcpyAsync(tab, groups, (size_t)n * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, cb, s);
    if (e != hipSuccess) return hb_fail(std::string("hb_index_set_row_groups: ") + hipGetErrorString(e));
    exclude_group_sizes_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(tab, n, n_groups, counts, counts + n_groups);
    e = hipGetLastError();
    std::vector<int32_t> host((size_t)n_groups + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), counts, cb, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hb_fail(std::string("hb_index_set_row_groups: ") + hipGetErrorString(e));
    if (host[n_groups]) return hb_fail("hb_index_set_row_groups: a row's group lies outside [-1, " + std::to_string(n_groups) + ")");
    ix->row_groups = std::move(tab); ix->row_groups_cap = n; ix->row_groups_n = n; ix->n_groups = n_groups;
    ix->gmax = n_groups ? *std::max_element(host.begin(), host.begin() + n_groups) : 0;
    return 0;
}

extern "C" int hb_index_last_exclusion(const hb_index_t* ix, int64_t out[4]) {
    if (!ix) return hb_fail("hb_index_last_exclusion: NULL index handle");
    if (!out) return hb_fail("hb_index_last_exclusion: out is NULL");
    for (int i = 0; i < 4; ++i) out[i] = ix->last_excl[i];
    return 0;
}

// The rung route on device pointers: rung 0 at rungs[0] into the workspace's lists, the filter, and rung 1 on the queries it left incomplete.
// ws: exclude_rungs_bytes(nq, rungs[0]) bytes -- [flags: incomplete count | 256 B] [complete, nq] [rung 0's lists]; rung 1 sizes ix->excl1 once
// its queries are counted.  Writes last_excl.  det == nullptr: the rungs ARE the search, and each commits its report like any search of a caller;
// else (the leftover of a search the screen served) they run detached: their reports and adaptive policy go to *det, which nobody commits.
static int rung_search(hb_index* ix, const float* qd, int64_t nq, int kf, int64_t id_base, int64_t* idx, float* dist, hb_detached* det) {
    hb_range range("hbird:search");
    return hb_search_device(ix, qd, nq, kf, id_base, idx, dist, det);
}
static size_t exclude_rungs_bytes(int64_t nq, int kf0) { return 256 + al256((size_t)nq * 4) + al256((size_t)nq * kf0 * 8) + al256((size_t)nq * kf0 * 4); }
static int exclude_rungs(hb_index* ix, const float* qd, int64_t nq, int k, int64_t id_base, const int32_t* qgd, int64_t* d_oi, float* d_od,
                         const int* rungs, int n_rungs, char* ws, hipStream_t s, hb_detached* det) {
    const int kf0 = rungs[0];
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    int32_t* complete = reinterpret_cast<int32_t*>(ws + 256);
    int64_t* l_idx = reinterpret_cast<int64_t*>(ws + 256 + al256((size_t)nq * 4));
    float* l_dist = reinterpret_cast<float*>(ws + 256 + al256((size_t)nq * 4) + al256((size_t)nq * kf0 * 8));
    HB_HIP(hipMemsetAsync(flags, 0, 8, s));
    // the missing-neighbour value of the search these lists come from
    const float pad = (ix->metric == HB_METRIC_L2 && !ix->score_output) ? INFINITY : -INFINITY;
    ix->last_excl[0] = 1; ix->last_excl[1] = 0; ix->last_excl[2] = kf0; ix->last_excl[3] = ix->gmax;
    // rung 0: hb_index_search's own path (k > 256: its ceiling passes) into the workspace lists, then the filter
    if (rung_search(ix, qd, nq, kf0, id_base, l_idx, l_dist, det)) return -1;
    if (hb_launch_exclude_filter(l_idx, l_dist, nq, kf0, id_base, ix->row_groups, ix->row_groups_n, qgd, k, pad, d_oi, d_od,
                                 n_rungs > 1 ? complete : nullptr, n_rungs > 1 ? flags : nullptr, s)) return -1;
    if (n_rungs > 1) {
        int32_t n1 = 0;
        HB_HIP(hipMemcpyAsync(&n1, flags, 4, hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
        if (n1 > 0) {
            // rung 1 on the incomplete queries only: [rows, n1] [their groups] [their query rows] [lists at need] [filtered lists]
            const int kf1 = rungs[1];
            const size_t c_rows = al256((size_t)n1 * 8), c_qg = al256((size_t)n1 * 4), c_q = al256((size_t)n1 * ix->d * 4);
            const size_t c_li = al256((size_t)n1 * kf1 * 8), c_ld = al256((size_t)n1 * kf1 * 4);
            const size_t c_fi = al256((size_t)n1 * k * 8), c_fd = al256((size_t)n1 * k * 4);
            if (ix->excl1.ensure(c_rows + c_qg + c_q + c_li + c_ld + c_fi + c_fd, HB_GROW_EXACT)) return -1;
            char* c = ix->excl1;
            int64_t* rows = reinterpret_cast<int64_t*>(c); c += c_rows;
            int32_t* qg1 = reinterpret_cast<int32_t*>(c); c += c_qg;
            float* q1 = reinterpret_cast<float*>(c); c += c_q;
            int64_t* l1_idx = reinterpret_cast<int64_t*>(c); c += c_li;
            float* l1_dist = reinterpret_cast<float*>(c); c += c_ld;
            int64_t* f_idx = reinterpret_cast<int64_t*>(c); c += c_fi;
            float* f_dist = reinterpret_cast<float*>(c);
            exclude_compact_kernel<<<dim3(1), dim3(256), 0, s>>>(complete, qgd, nq, rows, qg1);
            HB_HIP(hipGetLastError());
            if (hb_launch_gather_rows(qd, nq, ix->d, rows, n1, q1, s)) return -1;
            if (rung_search(ix, q1, n1, kf1, id_base, l1_idx, l1_dist, det)) return -1;
            if (hb_launch_exclude_filter(l1_idx, l1_dist, n1, kf1, id_base, ix->row_groups, ix->row_groups_n, qg1, k, pad, f_idx, f_dist, nullptr,
                                         nullptr, s)) return -1;
            if (hb_launch_scatter_rows(rows, n1, k, f_idx, f_dist, d_oi, d_od, s)) return -1;
            ix->last_excl[0] = 2; ix->last_excl[1] = n1; ix->last_excl[2] = kf1;
        }
    }
    return 0;
}

// The queries `left` (ascending) that the screen could not certify, through the rungs: compacted, gathered, searched, scattered into the outputs.
static int exclude_rungs_on(hb_index* ix, const std::vector<int64_t>& left, const float* qd, int64_t nq, int k, int64_t id_base, const int32_t* qgd,
                            int64_t* d_oi, float* d_od, const int* rungs, int n_rungs, hipStream_t s, hb_detached* det) {
    const int64_t n = (int64_t)left.size();
    // [rows, n] [complete, nq] [their groups] [their query rows] [their lists] [the rungs' workspace]
    const size_t o_comp = al256((size_t)n * 8), o_qg = o_comp + al256((size_t)nq * 4), o_q = o_qg + al256((size_t)n * 4),
                 o_oi = o_q + al256((size_t)n * ix->d * 4), o_od = o_oi + al256((size_t)n * k * 8), o_ws = o_od + al256((size_t)n * k * 4);
    if (ix->excl_sub.ensure(o_ws + exclude_rungs_bytes(n, rungs[0]), HB_GROW_EXACT)) return -1;
    int64_t* rows = ix->excl_sub.as<int64_t>();
    int32_t* complete = ix->excl_sub.as<int32_t>(o_comp);
    int32_t* qg = ix->excl_sub.as<int32_t>(o_qg);
    float* q1 = ix->excl_sub.as<float>(o_q);
    int64_t* oi = ix->excl_sub.as<int64_t>(o_oi);
    float* od = ix->excl_sub.as<float>(o_od);
    std::vector<int32_t> done((size_t)nq, 1);
    for (int64_t i : left) done[(size_t)i] = 0;
    HB_HIP(hipMemcpyAsync(complete, done.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
    exclude_compact_kernel<<<dim3(1), dim3(256), 0, s>>>(complete, qgd, nq, rows, qg);
    HB_HIP(hipGetLastError());
    if (hb_launch_gather_rows(qd, nq, ix->d, rows, n, q1, s)) return -1;
    HB_HIP(hipStreamSynchronize(s));      // (`done` goes out of use)
    if (exclude_rungs(ix, q1, n, k, id_base, qg, oi, od, rungs, n_rungs, ix->excl_sub.as<char>(o_ws), s, det)) return -1;
    return hb_launch_scatter_rows(rows, n, k, oi, od, d_oi, d_od, s);
}

extern "C" int hb_index_search_excluding(hb_index_t* ix, const float* q, int64_t nq, int k, int64_t id_base, const int32_t* qgroups,
                                         int64_t* out_idx, float* out_dist, int io_on_device) {
    if (!ix) return hb_fail("hb_index_search_excluding: NULL index handle");
    if (nq < 0) return hb_fail("hb_index_search_excluding: negative query count");
    if (k < 1 || k > HB_MAX_K) return hb_fail("hb_index_search_excluding: k must be in [1, " + std::to_string(HB_MAX_K) + "]");
    if (ix->row_groups_n == 0) return hb_fail("hb_index_search_excluding: the index has no row-group table (hb_index_set_row_groups)");
    if (ix->row_groups_n != ix->ntotal)
        return hb_fail("hb_index_search_excluding: the row-group table covers " + std::to_string(ix->row_groups_n) + " rows, the bank holds " +
                       std::to_string(ix->ntotal) + " (rows were added or removed since hb_index_set_row_groups: set the table again)");
    int rungs[2] = {0, 0};
    const int n_rungs = hb_exclude_plan_replay(k, ix->gmax, rungs, 2);      // (need > HB_MAX_K: its message names k, gmax, the limit and the remedy)
    if (n_rungs < 0) return -1;
    if (nq == 0) return 0;
    if (!q || !qgroups || !out_idx || !out_dist) return hb_fail("hb_index_search_excluding: NULL pointer");
    if (!io_on_device)
        for (int64_t i = 0; i < nq; ++i)
            if (qgroups[i] < -1 || qgroups[i] >= ix->n_groups)
                return hb_fail("hb_index_search_excluding: query " + std::to_string(i) + " names group " + std::to_string(qgroups[i]) + ", outside [-1, " +
                               std::to_string(ix->n_groups) + ")");
    hb_range range("hbird:search_excluding");
    HB_HIP(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    // Does the certified fp16 screen get the search (hb_index_set_exclude_screen; include/hbird_hip_exclude_screen.h)?  What can be told here;
    // whether the index's own choice for (nq, k) is the candidate pass is the search's decision (hb_launch_knn_excluding).
    int why_not = HB_EXCL_SCREEN_SERVED;
    if (!ix->excl_screen) why_not = HB_EXCL_SCREEN_OFF;
    else if (k > 128) why_not = HB_EXCL_SCREEN_K;
    else if ((int64_t)k + ix->gmax <= 128) why_not = HB_EXCL_SCREEN_NEED;
    else if (ix->fp16 == 0) why_not = HB_EXCL_SCREEN_PATH;
    else if (ix->ntotal == 0) why_not = HB_EXCL_SCREEN_EMPTY;
    const bool try_screen = why_not == HB_EXCL_SCREEN_SERVED;
    // workspace: [bad-group flag | 256 B] [queries, qgroups, idx, dist (host path)] [the rungs' workspace (where the screen is not tried)]
    const size_t b_flag = 256;
    const size_t b_q = io_on_device ? 0 : al256((size_t)nq * ix->d * 4), b_qg = io_on_device ? 0 : al256((size_t)nq * 4);
    const size_t b_oi = io_on_device ? 0 : al256((size_t)nq * k * 8), b_od = io_on_device ? 0 : al256((size_t)nq * k * 4);
    const size_t b_head = b_flag + b_q + b_qg + b_oi + b_od, b_rungs = exclude_rungs_bytes(nq, rungs[0]);
    if (ix->excl.ensure(b_head + (try_screen ? 0 : b_rungs), HB_GROW_EXACT)) return -1;
    const float* qd = q; const int32_t* qgd = qgroups; int64_t* d_oi = out_idx; float* d_od = out_dist;
    auto carve = [&]() {      // (again after the buffer has moved)
        if (io_on_device) return;
        char* cur = ix->excl.as<char>(b_flag);
        qd = reinterpret_cast<const float*>(cur); cur += b_q;
        qgd = reinterpret_cast<const int32_t*>(cur); cur += b_qg;
        d_oi = reinterpret_cast<int64_t*>(cur); cur += b_oi;
        d_od = reinterpret_cast<float*>(cur);
    };
    carve();
    if (!io_on_device) {
        HB_HIP(hipMemcpyAsync(const_cast<float*>(qd), q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice, s));
        HB_HIP(hipMemcpyAsync(const_cast<int32_t*>(qgd), qgroups, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    }
    if (io_on_device) {      // device query groups: one small launch and a flag read, before anything is searched or written
        int32_t* flags = ix->excl.as<int32_t>();
        HB_HIP(hipMemsetAsync(flags, 0, 8, s));
        exclude_check_qgroups_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s>>>(qgd, nq, ix->n_groups, flags + 1);
        HB_HIP(hipGetLastError());
        int32_t bad = 0;
        HB_HIP(hipMemcpyAsync(&bad, flags + 1, 4, hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
        if (bad) return hb_fail("hb_index_search_excluding: a query names a group outside [-1, " + std::to_string(ix->n_groups) + ")");
    }
    hb_search_report rep;
    if (try_screen) {
        if (hb_launch_knn_excluding(ix, qd, nq, k, id_base, qgd, d_oi, d_od, &rep)) return -1;
        if (!rep.took_candidate_pass()) why_not = HB_EXCL_SCREEN_PATH;
    }
    int64_t* o = ix->last_excl_screen;
    for (int i = 0; i < 8; ++i) o[i] = 0;
    o[1] = why_not;
    if (!rep.took_candidate_pass()) {
        if (try_screen) {      // the screen declined: the rungs' workspace after all, behind the staged inputs
            if (ix->excl.ensure_keep(b_head + b_rungs, HB_GROW_EXACT, b_head, s)) return -1;
            carve();
        }
        if (exclude_rungs(ix, qd, nq, k, id_base, qgd, d_oi, d_od, rungs, n_rungs, ix->excl.as<char>(b_head), s, nullptr)) return -1;
    } else {
        // What describes THIS search is the report of its passes.  The rungs of the leftover are searches of their own and run detached: their
        // reports, and what they would teach the adaptive fp16 policy (an excluding search's failures say nothing about plain searches), go to a
        // scratch pair that is never committed.  They search at kf > 128, the fp32 kernel, which writes none of `cand`, `fb`, `fb1`, `q16`; should
        // one of them take the candidate pass after all, the buffers are its own and the read-outs refuse.
        ix->last_excl[0] = 0; ix->last_excl[1] = 0; ix->last_excl[2] = 0; ix->last_excl[3] = ix->gmax;
        hb_detached scratch{hb_search_report(), ix->f16_adapt};
        const int rc = rep.n_left() > 0 ? exclude_rungs_on(ix, rep.left, qd, nq, k, id_base, qgd, d_oi, d_od, rungs, n_rungs, s, &scratch) : 0;
        if (scratch.rep.took_candidate_pass()) rep.buffers_reused();
        if (ix->commit(std::move(rep), rc)) return -1;
        const hb_search_report& r = ix->last;
        o[0] = 1; o[2] = r.kc; o[3] = r.certified0(); o[4] = r.sent1(); o[5] = r.certified1(); o[6] = r.n_left(); o[7] = r.lists_centred;
    }
    if (!io_on_device) {
        HB_HIP(hipMemcpyAsync(out_idx, d_oi, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
        HB_HIP(hipMemcpyAsync(out_dist, d_od, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

