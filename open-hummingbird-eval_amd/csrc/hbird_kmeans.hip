// k-means over the resident bank (include/hbird_hip_kmeans.h): Lloyd's iteration whose assignment step IS the exact k = 1 search on an L2 index
// of the centroids, and whose update step sums the bank's fragment tiles in exact integers.  gfx950 only.
//
// The update, Q(x) = llrint(x * 2^30) summed in int64: integer adds commute, so the sums -- and the centroids, one double division and one
// fp32 rounding later -- do not depend on the order in which workgroups, waves or atomics arrive, nor on how the rows were chunked or split
// over calls.  No floating-point atomic appears anywhere in this unit.
//
// kmeans_accumulate_kernel, the one kernel that reads the bank: workgroup = (segment of row tiles) x (one 8-column block group g).  A wave
// takes one 1 KiB fragment block (32 rows x 8 k) per 16-byte load per lane -- lane l = h * 32 + i holds k = 8 g + {h, 2 + h,
// 4 + h, 6 + h} of row i -- and adds its four Q values into a [K][8] int64 table in LDS (64 K bytes: 128 KiB at K = 2048) with 64-bit LDS
// atomics; the table leaves with one 64-bit global atomic per non-zero cell.  The number of segments is a function of the row count alone.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include <algorithm>

#define KM_THREADS 512
#define KM_WAVES (KM_THREADS / 64)
#define KM_UNROLL 4                  // fragment blocks in flight per wave
#define KM_SEG_TILES 16              // row tiles per segment at the least ...
#define KM_MAX_SEGS 128              // ... and segments at the most: segments = min(ceil(row tiles / 16), 128)
#define KM_FLAG_RANGE 1              // a component outside [-2, 2] (or not finite) in an assigned row
#define KM_FLAG_ID 2                 // an assignment >= K
#define KM_INERTIA_BLOCKS 256

__device__ __forceinline__ long long km_quantise(float x) { return __double2ll_rn((double)x * 1073741824.0); }

__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_kernel(const float* __restrict__ tiles, int g8, int d, const int32_t* __restrict__ assign,
                                                                       int64_t row0, int64_t n, int K, int64_t rt_begin, int64_t rt_end,
                                                                       int64_t seg_tiles, unsigned long long* __restrict__ sums, int* __restrict__ flag) {
    extern __shared__ unsigned long long s_tab[];      // [K][8]
    const int tid = threadIdx.x, g = blockIdx.x;
    const int cells = K * 8;
    for (int c = tid; c < cells; c += KM_THREADS) s_tab[c] = 0ull;
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
    const int64_t t0 = rt_begin + (int64_t)blockIdx.y * seg_tiles, t1 = std::min<int64_t>(rt_end, t0 + seg_tiles);
    int bad = 0;
    for (int64_t rt = t0 + wave; rt < t1; rt += KM_WAVES * KM_UNROLL) {
        float4 v[KM_UNROLL];
        int a[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            const int64_t t = rt + (int64_t)u * KM_WAVES;
            a[u] = -1;
            v[u] = float4{0.f, 0.f, 0.f, 0.f};
            if (t < t1) {
                const int64_t r = t * HB_RT + i;
                if (r >= row0 && r < row0 + n) a[u] = assign[r - row0];
                v[u] = *reinterpret_cast<const float4*>(tiles + (t * (int64_t)g8 + g) * HB_BLK + lane * 4);
            }
        }
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            if (a[u] < 0) continue;
            if (a[u] >= K) { bad |= KM_FLAG_ID; continue; }
            const float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = 2 * j + h;
                if (8 * g + kk >= d) continue;                              // (the padding columns of the last group hold zeros)
                if (!(fabsf(x[j]) <= 2.0f)) { bad |= KM_FLAG_RANGE; continue; }
                const long long q = km_quantise(x[j]);
                if (q != 0) atomicAdd(&s_tab[a[u] * 8 + kk], (unsigned long long)q);
            }
        }
    }
    if (bad) atomicOr(flag, bad);
    __syncthreads();
    for (int c = tid; c < cells; c += KM_THREADS) {
        const unsigned long long s = s_tab[c];
        const int k = 8 * g + (c & 7);
        if (s != 0ull && k < d) atomicAdd(&sums[(int64_t)(c >> 3) * d + k], s);
    }
}

// counts[c] += #{i : assign[i] == c}; a block-private table in LDS, one global atomic per non-zero cell
__global__ __launch_bounds__(256) void kmeans_counts_kernel(const int32_t* __restrict__ assign, int64_t n, int K, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long s_cnt[HB_KMEANS_MAX_K];
    for (int c = threadIdx.x; c < K; c += 256) s_cnt[c] = 0ull;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int a = assign[r];
        if (a >= 0 && a < K) atomicAdd(&s_cnt[a], 1ull);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < K; c += 256)
        if (s_cnt[c]) atomicAdd(&counts[c], s_cnt[c]);
}

// out[c][j] = (float)((double)S / ((double)n * 2^30)), or prev[c][j] for an empty cluster (out may be prev); *n_empty += empty clusters
__global__ __launch_bounds__(256) void kmeans_centroids_kernel(const long long* __restrict__ sums, const long long* __restrict__ counts, int K, int d,
                                                               const float* prev, float* out, unsigned long long* __restrict__ n_empty) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)K * d) return;
    const int c = (int)(e / d), j = (int)(e - (int64_t)c * d);
    const long long cnt = counts[c];
    if (cnt <= 0) {
        out[e] = prev[e];
        if (j == 0) atomicAdd(n_empty, 1ull);
        return;
    }
    out[e] = (float)((double)sums[e] / ((double)cnt * 1073741824.0));
}

__device__ __forceinline__ unsigned long long km_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// out[0] += #{r : a[r] != prev[r]}, out[1] += #{r : a[r] < 0}; prev[r] = a[r].  (prev starts as all -1: the first iteration's `changed` is the
// number of assigned rows.)
__global__ __launch_bounds__(256) void kmeans_changed_kernel(const int32_t* __restrict__ a, int32_t* __restrict__ prev, int64_t n,
                                                             unsigned long long* __restrict__ out) {
    unsigned long long ch = 0, un = 0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int x = a[r];
        ch += x != prev[r];
        un += x < 0;
        prev[r] = x;
    }
    ch = km_wave_sum(ch); un = km_wave_sum(un);
    if ((threadIdx.x & 63) == 0) {
        if (ch) atomicAdd(&out[0], ch);
        if (un) atomicAdd(&out[1], un);
    }
}

// inertia = sum of dist[r] over a[r] >= 0 in float64, by a tree that depends on n alone: thread t of block b adds its rows
// (b * 256 + t) + j * 65536 in ascending j, the block's 256 sums meet pairwise in LDS, and one block does the same with the 256 partials
__device__ __forceinline__ double km_block_tree(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    return s[0];
}
__global__ __launch_bounds__(256) void kmeans_inertia_partial_kernel(const int32_t* __restrict__ a, const float* __restrict__ dist, int64_t n,
                                                                     double* __restrict__ partial) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)KM_INERTIA_BLOCKS * 256)
        if (a[r] >= 0) acc += (double)dist[r];
    const double t = km_block_tree(acc, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void kmeans_inertia_final_kernel(const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double s[256];
    const double t = km_block_tree(partial[threadIdx.x], s);
    if (threadIdx.x == 0) *out = t;
}

// the bank's rows row0 .. row0 + m - 1 as row-major queries: one workgroup per row tile, 64 columns at a time through LDS (16-byte loads of
// whole fragment blocks in, 256-byte row pieces out)
__global__ __launch_bounds__(256) void kmeans_stage_rows_kernel(const float* __restrict__ tiles, int g8, int d, int64_t row0, int64_t m, float* __restrict__ out) {
    __shared__ float s[32][65];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
    const int64_t rt = (row0 >> 5) + blockIdx.x;
    for (int g0 = 0; g0 < g8; g0 += 8) {
        for (int gg = wave; gg < 8; gg += 4) {
            const int g = g0 + gg;
            if (g < g8) {
                const float4 v = *reinterpret_cast<const float4*>(tiles + (rt * (int64_t)g8 + g) * HB_BLK + lane * 4);
                s[i][gg * 8 + h] = v.x; s[i][gg * 8 + 2 + h] = v.y; s[i][gg * 8 + 4 + h] = v.z; s[i][gg * 8 + 6 + h] = v.w;
            }
        }
        __syncthreads();
        for (int e = tid; e < 32 * 64; e += 256) {
            const int row = e >> 6, col = e & 63, k = g0 * 8 + col;
            const int64_t r = rt * 32 + row;
            if (k < d && r >= row0 && r < row0 + m) out[(r - row0) * (int64_t)d + k] = s[row][col];
        }
        __syncthreads();
    }
}

// the k = 1 lists of a chunk -> assign (int32, -1: no neighbour) and, unless NULL, the distances
__global__ __launch_bounds__(256) void kmeans_ids_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist, int64_t m, int32_t* __restrict__ assign,
                                                         float* __restrict__ dist_out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const int64_t id = idx[r];
    assign[r] = id < 0 ? -1 : (int32_t)id;
    if (dist_out) dist_out[r] = dist[r];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
namespace {
int km_blocks(int64_t n, int per_block, int cap) { return (int)std::max<int64_t>(1, std::min<int64_t>(cap, (n + per_block - 1) / per_block)); }

struct km_stage {      // the workspace of an assignment: one chunk's rows, lists and distances
    hb_dev<float> rows; hb_dev<int64_t> idx; hb_dev<float> dist;
    int64_t chunk = 0;
    int ensure(const hb_index* bank, int64_t n, int64_t chunk_rows) {
        chunk = std::max<int64_t>(1, chunk_rows > 0 ? std::min(chunk_rows, n) : std::min<int64_t>(n, HB_KMEANS_CHUNK_ROWS));
        return rows.ensure((size_t)chunk * bank->d * 4, HB_GROW_EXACT) || idx.ensure((size_t)chunk * 8, HB_GROW_EXACT) || dist.ensure((size_t)chunk * 4, HB_GROW_EXACT);
    }
};

int km_check_range(const char* who, const hb_index* bank, int64_t row0, int64_t n) {
    if (row0 < 0 || n < 0 || row0 + n > bank->ntotal)
        return hb_fail(std::string(who) + ": rows " + std::to_string(row0) + " .. " + std::to_string(row0 + n) + " lie outside the bank's " + std::to_string(bank->ntotal) + " rows");
    return 0;
}
int km_check_k(const char* who, int K) {
    if (K < 1 || K > HB_KMEANS_MAX_K) return hb_fail(std::string(who) + ": K must be in [1, " + std::to_string(HB_KMEANS_MAX_K) + "], got " + std::to_string(K));
    return 0;
}

// the searches run on the bank's stream: the centroid index takes it for the call
struct km_stream_loan {
    hb_index* cent; hipStream_t keep;
    km_stream_loan(hb_index* c, hipStream_t s) : cent(c), keep(c->stream) { c->stream = s; }
    ~km_stream_loan() { cent->stream = keep; }
};

int km_assign(hb_index* bank, hb_index* cent, km_stage& st, int64_t row0, int64_t n, int32_t* assign, float* dist_opt) {
    hipStream_t s = bank->stream;
    km_stream_loan loan(cent, s);
    for (int64_t r = 0; r < n; r += st.chunk) {
        const int64_t m = std::min(st.chunk, n - r), first = row0 + r;
        const unsigned row_tiles = (unsigned)(((first + m + 31) >> 5) - (first >> 5));
        kmeans_stage_rows_kernel<<<dim3(row_tiles), dim3(256), 0, s>>>(bank->tiles, bank->g8, bank->d, first, m, st.rows);
        HB_HIP(hipGetLastError());
        if (hb_index_search(cent, st.rows, m, 1, 0, st.idx, st.dist, 1)) return -1;
        kmeans_ids_kernel<<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s>>>(st.idx, st.dist, m, assign + r, dist_opt ? dist_opt + r : nullptr);
        HB_HIP(hipGetLastError());
    }
    return 0;
}

// sums / counts += the rows' contributions; flag_dev: a zeroed int the kernel raises KM_FLAG_* in (read by the caller)
int km_accumulate(const hb_index* bank, const int32_t* assign, int64_t row0, int64_t n, int K, int64_t* sums, int64_t* counts, int* flag_dev) {
    if (n == 0) return 0;
    hipStream_t s = bank->stream;
    const int64_t rt_begin = row0 >> 5, rt_end = (row0 + n + 31) >> 5, nt = rt_end - rt_begin;
    const int64_t segs = std::max<int64_t>(1, std::min<int64_t>(KM_MAX_SEGS, (nt + KM_SEG_TILES - 1) / KM_SEG_TILES));
    const int64_t seg_tiles = (nt + segs - 1) / segs;
    const int lds = K * 8 * 8;
    if (hb_ensure_dyn_lds((const void*)kmeans_accumulate_kernel, lds)) return -1;
    kmeans_accumulate_kernel<<<dim3((unsigned)bank->g8, (unsigned)segs), dim3(KM_THREADS), lds, s>>>(
        bank->tiles, bank->g8, bank->d, assign, row0, n, K, rt_begin, rt_end, seg_tiles, reinterpret_cast<unsigned long long*>(sums), flag_dev);
    HB_HIP(hipGetLastError());
    kmeans_counts_kernel<<<dim3(km_blocks(n, 4096, 1024)), dim3(256), 0, s>>>(assign, n, K, reinterpret_cast<unsigned long long*>(counts));
    HB_HIP(hipGetLastError());
    return 0;
}
int km_flag_status(const char* who, int flag) {
    if (flag & KM_FLAG_ID) return hb_fail(std::string(who) + ": an assignment is not below K");
    if (flag & KM_FLAG_RANGE) return hb_fail(std::string(who) + ": an assigned row holds a component outside [-2, 2] (k-means is for normalised banks)");
    return 0;
}

int km_centroids(const int64_t* sums, const int64_t* counts, int K, int d, const float* prev, float* out, unsigned long long* n_empty_dev, hipStream_t s) {
    const int64_t e = (int64_t)K * d;
    kmeans_centroids_kernel<<<dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s>>>(reinterpret_cast<const long long*>(sums), reinterpret_cast<const long long*>(counts),
                                                                                     K, d, prev, out, n_empty_dev);
    HB_HIP(hipGetLastError());
    return 0;
}

int km_check_cent(const char* who, const hb_index* bank, const hb_index* cent) {
    if (cent == bank) return hb_fail(std::string(who) + ": the centroid index is the bank");
    if (cent->metric != HB_METRIC_L2) return hb_fail(std::string(who) + ": the centroid index must be an HB_METRIC_L2 index");
    if (cent->d != bank->d) return hb_fail(std::string(who) + ": the centroid index holds rows of width " + std::to_string(cent->d) + ", the bank " + std::to_string(bank->d));
    if (cent->device != bank->device) return hb_fail(std::string(who) + ": the centroid index lives on another device than the bank");
    if (cent->ntotal < 1) return hb_fail(std::string(who) + ": the centroid index is empty");
    return 0;
}
}  // namespace

extern "C" int hb_kmeans_assign(hb_index_t* bank, hb_index_t* cent, int64_t row0, int64_t n, int64_t chunk_rows, int32_t* assign, float* dist_opt) {
    if (!bank || !cent) return hb_fail("hb_kmeans_assign: NULL index handle");
    if (km_check_range("hb_kmeans_assign", bank, row0, n)) return -1;
    if (chunk_rows < 0) return hb_fail("hb_kmeans_assign: negative chunk_rows");
    if (km_check_cent("hb_kmeans_assign", bank, cent)) return -1;
    if (n == 0) return 0;
    if (!assign) return hb_fail("hb_kmeans_assign: assign is NULL");
    hb_range range("hbird:kmeans_assign");
    HB_HIP(hipSetDevice(bank->device));
    km_stage st;
    if (st.ensure(bank, n, chunk_rows)) return -1;
    const int rc = km_assign(bank, cent, st, row0, n, assign, dist_opt);
    HB_HIP(hipStreamSynchronize(bank->stream));      // (the staging buffers go with the call)
    return rc;
}

extern "C" int hb_kmeans_accumulate(hb_index_t* bank, const int32_t* assign, int64_t row0, int64_t n, int K, int64_t* sums, int64_t* counts) {
    if (!bank) return hb_fail("hb_kmeans_accumulate: NULL index handle");
    if (km_check_k("hb_kmeans_accumulate", K) || km_check_range("hb_kmeans_accumulate", bank, row0, n)) return -1;
    if (n == 0) return 0;
    if (!assign || !sums || !counts) return hb_fail("hb_kmeans_accumulate: NULL pointer");
    hb_range range("hbird:kmeans_accumulate");
    HB_HIP(hipSetDevice(bank->device));
    hb_dev<int> flag;
    if (flag.ensure(4, HB_GROW_EXACT)) return -1;
    HB_HIP(hipMemsetAsync(flag, 0, 4, bank->stream));
    if (km_accumulate(bank, assign, row0, n, K, sums, counts, flag)) return -1;
    int f = 0;
    HB_HIP(hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, bank->stream));
    HB_HIP(hipStreamSynchronize(bank->stream));
    return km_flag_status("hb_kmeans_accumulate", f);
}

extern "C" int hb_kmeans_centroids(const int64_t* sums, const int64_t* counts, int K, int d, const float* prev, float* out, int64_t* n_empty_host,
                                   void* stream) {
    if (km_check_k("hb_kmeans_centroids", K)) return -1;
    if (d < 1) return hb_fail("hb_kmeans_centroids: d must be positive");
    if (!sums || !counts || !prev || !out) return hb_fail("hb_kmeans_centroids: NULL pointer");
    hipPointerAttribute_t at;
    HB_HIP(hipPointerGetAttributes(&at, sums));
    HB_HIP(hipSetDevice(at.device));
    hipStream_t s = (hipStream_t)stream;
    hb_dev<unsigned long long> ne;
    if (ne.ensure(8, HB_GROW_EXACT)) return -1;
    HB_HIP(hipMemsetAsync(ne, 0, 8, s));
    if (km_centroids(sums, counts, K, d, prev, out, ne, s)) return -1;
    unsigned long long h = 0;
    HB_HIP(hipMemcpyAsync(&h, ne, 8, hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));
    if (n_empty_host) *n_empty_host = (int64_t)h;
    return 0;
}

namespace {
struct km_index_owner {      // fit's own centroid index
    hb_index_t* ix = nullptr;
    ~km_index_owner() { if (ix) hb_index_free(ix); }
};
// what one iteration reads back: {changed, unassigned, empty}, the inertia, the accumulate kernel's flag
struct km_scalars { unsigned long long changed, unassigned, empty; double inertia; int flag; int pad; };
}  // namespace

extern "C" int hb_kmeans_fit(hb_index_t* bank, int K, const float* init, int max_iter, int64_t chunk_rows, float* centroids, int64_t* counts,
                             int32_t* assign_opt, double* history, int* iters, int* converged) {
    if (!bank) return hb_fail("hb_kmeans_fit: NULL index handle");
    if (km_check_k("hb_kmeans_fit", K)) return -1;
    if (K > bank->ntotal) return hb_fail("hb_kmeans_fit: K = " + std::to_string(K) + " exceeds the bank's " + std::to_string(bank->ntotal) + " rows");
    if (max_iter < 1) return hb_fail("hb_kmeans_fit: max_iter must be positive");
    if (chunk_rows < 0) return hb_fail("hb_kmeans_fit: negative chunk_rows");
    if (!init || !centroids || !counts || !history || !iters || !converged) return hb_fail("hb_kmeans_fit: NULL pointer");
    hb_range range("hbird:kmeans_fit");
    HB_HIP(hipSetDevice(bank->device));
    hipStream_t s = bank->stream;
    const int64_t n = bank->ntotal;
    const int d = bank->d;
    *iters = 0; *converged = 0;

    km_index_owner cent;
    if (hb_index_create(d, HB_METRIC_L2, bank->device, &cent.ix) || hb_index_set_fp16(cent.ix, 0)) return -1;
    km_stage st;
    hb_dev<int32_t> a_own, prev; hb_dev<float> dist; hb_dev<int64_t> sums; hb_dev<double> partial; hb_dev<km_scalars> sc;
    if (st.ensure(bank, n, chunk_rows) || (!assign_opt && a_own.ensure((size_t)n * 4, HB_GROW_EXACT)) || prev.ensure((size_t)n * 4, HB_GROW_EXACT)
        || dist.ensure((size_t)n * 4, HB_GROW_EXACT) || sums.ensure((size_t)K * d * 8, HB_GROW_EXACT) || partial.ensure(KM_INERTIA_BLOCKS * 8, HB_GROW_EXACT)
        || sc.ensure(sizeof(km_scalars), HB_GROW_EXACT)) return -1;
    int32_t* a = assign_opt ? assign_opt : (int32_t*)a_own;
    km_scalars* scd = sc;
    if (centroids != init) HB_HIP(hipMemcpyAsync(centroids, init, (size_t)K * d * 4, hipMemcpyDeviceToDevice, s));
    HB_HIP(hipMemsetAsync(counts, 0, (size_t)K * 8, s));
    HB_HIP(hipMemsetAsync(prev, 0xFF, (size_t)n * 4, s));      // every row starts unassigned (-1)
    unsigned long long last_empty = (unsigned long long)K;      // (no update yet: no cluster has a row)
    int rc = 0;
    for (int it = 1; it <= max_iter && !rc; ++it) {
        {   // the centroid index of this iteration; its stream is the bank's while rows are added
            km_stream_loan loan(cent.ix, s);
            if (hb_index_reset(cent.ix) || hb_index_add(cent.ix, centroids, K, 1, 0)) { rc = -1; break; }
        }
        if (km_assign(bank, cent.ix, st, 0, n, a, dist)) { rc = -1; break; }
        HB_HIP(hipMemsetAsync(scd, 0, sizeof(km_scalars), s));
        kmeans_changed_kernel<<<dim3(km_blocks(n, 4096, 1024)), dim3(256), 0, s>>>(a, prev, n, &scd->changed);
        HB_HIP(hipGetLastError());
        kmeans_inertia_partial_kernel<<<dim3(KM_INERTIA_BLOCKS), dim3(256), 0, s>>>(a, dist, n, partial);
        HB_HIP(hipGetLastError());
        kmeans_inertia_final_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, &scd->inertia);
        HB_HIP(hipGetLastError());
        km_scalars h;
        HB_HIP(hipMemcpyAsync(&h, scd, sizeof(h), hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
        double* row = history + (size_t)(it - 1) * 4;
        row[0] = (double)h.changed; row[2] = (double)h.unassigned; row[3] = h.inertia;
        *iters = it;
        if (h.changed == 0) {      // the assignment is the previous iteration's: so are its update, counts and empty clusters
            row[1] = (double)last_empty;
            *converged = 1;
            break;
        }
        HB_HIP(hipMemsetAsync(sums, 0, (size_t)K * d * 8, s));
        HB_HIP(hipMemsetAsync(counts, 0, (size_t)K * 8, s));
        if (km_accumulate(bank, a, 0, n, K, sums, counts, &scd->flag)) { rc = -1; break; }
        if (km_centroids(sums, counts, K, d, centroids, centroids, &scd->empty, s)) { rc = -1; break; }
        HB_HIP(hipMemcpyAsync(&h, scd, sizeof(h), hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
        if (km_flag_status("hb_kmeans_fit", h.flag)) { rc = -1; break; }
        last_empty = h.empty;
        row[1] = (double)last_empty;
    }
    (void)hipStreamSynchronize(s);      // (the workspace and the centroid index go with the call)
    return rc;
}
