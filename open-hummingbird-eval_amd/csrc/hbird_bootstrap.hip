// Paired bootstrap over images for mIoU grids (include/hbird_hip_bootstrap.h, DESIGN.md section 4 "Bootstrap intervals"): per-image class
// counts, the counter-based resampler, the resampling reduction cnt = W x stats in 64-bit integers, and the mIoU epilogue.
//
// Every grid point of an evaluation sees the same images in the same order and mIoU is a function of per-class pixel counts that add over
// images, so a bootstrap replicate of ALL configurations at once is one row of multiplicities W[r][.] applied to the image-major table
// stats[n_img][n_cfg * 3 G]: R * n_img * cols 32 x 32 -> 64-bit multiply-adds (1.4e11 for 10,000 replicates of an ADE20K-shaped grid).
// Integer sums have no order: every kernel here is exact, and the float64 epilogue sums its G terms sequentially.
#include "../../include/hbird_hip_bootstrap.h"
#include "hbird_internal.h"
#include <algorithm>

// the epilogue's steps are specified one by one in float64 (the numpy restatement evaluates them so): no contraction
#pragma clang fp contract(off)

// ---- per-image class counts ---------------------------------------------------------------------------------------------------------------
// grid (blocks per image, B): a workgroup counts its share of image b's pixels into an LDS histogram of 3 G counters [G][3] = (tp, fp, fn)
// and adds it once to the image's (zeroed) block; where 3 G counters do not fit the LDS budget the counts go to the block directly, as in
// confusion_kernel.  A wave's 64 neighbouring pixels mostly share one or two (gt, pred) pairs (piecewise-constant maps): up to two groups
// are counted by their leaders, the rest lane by lane.
#define BS_COUNT_LDS_BYTES (48 * 1024)
__global__ __launch_bounds__(256) void image_class_zero_kernel(int32_t* __restrict__ out, int64_t row_stride, int bins) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < bins) out[(int64_t)blockIdx.y * row_stride + e] = 0;
}

__global__ __launch_bounds__(256) void image_class_counts_kernel(const int64_t* __restrict__ gt, const int64_t* __restrict__ pred, int64_t hw,
                                                                 int G, int64_t ignore, int has_ignore, int use_lds,
                                                                 int32_t* __restrict__ out, int64_t row_stride) {
    extern __shared__ __attribute__((aligned(16))) int bs_hist[];
    const int bins = 3 * G;
    int* dst = out + (int64_t)blockIdx.y * row_stride;
    if (use_lds) {
        for (int e = threadIdx.x; e < bins; e += 256) bs_hist[e] = 0;
        __syncthreads();
    }
    int* tab = use_lds ? bs_hist : dst;
    const int64_t* g_img = gt + (int64_t)blockIdx.y * hw;
    const int64_t* p_img = pred + (int64_t)blockIdx.y * hw;
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); i0 < hw; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + lane;
        bool valid = i < hw;
        const int64_t g64 = valid ? g_img[i] : -1, p64 = valid ? p_img[i] : -1;
        valid = valid && !(has_ignore && g64 == ignore) && g64 >= 0 && g64 < G && p64 >= 0 && p64 < G;
        const int g = valid ? (int)g64 : -1, p = valid ? (int)p64 : -1;
        unsigned long long todo = __ballot(valid);
#pragma unroll 1
        for (int round = 0; round < 2 && todo; ++round) {
            const int leader = __builtin_ctzll(todo);
            const int gl = __builtin_amdgcn_readlane(g, leader), pl = __builtin_amdgcn_readlane(p, leader);
            const unsigned long long same = __ballot(g == gl && p == pl) & todo;
            if (lane == leader) {
                const int n = __popcll(same);
                if (gl == pl) atomicAdd(&tab[3 * gl], n);
                else { atomicAdd(&tab[3 * pl + 1], n); atomicAdd(&tab[3 * gl + 2], n); }
            }
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) {
            if (g == p) atomicAdd(&tab[3 * g], 1);
            else { atomicAdd(&tab[3 * p + 1], 1); atomicAdd(&tab[3 * g + 2], 1); }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int e = threadIdx.x; e < bins; e += 256)
            if (bs_hist[e]) atomicAdd(&dst[e], bs_hist[e]);
    }
}

extern "C" int hb_image_class_counts(const int64_t* gt, const int64_t* pred, int64_t B, int h, int w, int G, int64_t ignore, int has_ignore,
                                     int32_t* out, int64_t row_stride, void* stream) {
    hb_range range("hbird:image_class_counts");
    if (B == 0) return 0;
    if (!gt || !pred || !out) return hb_fail("hb_image_class_counts: gt / pred / out is NULL");
    if (B < 0 || B > 65535 || h < 1 || w < 1) return hb_fail("hb_image_class_counts: bad shape (1 <= B <= 65535, h, w >= 1)");
    if ((long long)h * w >= 0x80000000LL) return hb_fail("hb_image_class_counts: h * w must be below 2^31 (int32 counts)");
    if (G < 1 || G > 0x7FFFFFFF / 3) return hb_fail("hb_image_class_counts: bad class count");
    if (row_stride < 3LL * G) return hb_fail("hb_image_class_counts: row_stride is smaller than an image's 3 G counts");
    const hipStream_t s = (hipStream_t)stream;
    const int bins = 3 * G;
    const int64_t hw = (int64_t)h * w;
    const int use_lds = (size_t)bins * 4 <= BS_COUNT_LDS_BYTES;
    const unsigned per_image = (unsigned)std::min<int64_t>(std::max<int64_t>((hw + 4095) / 4096, 1), 64);
    image_class_zero_kernel<<<dim3((unsigned)((bins + 255) / 256), (unsigned)B), dim3(256), 0, s>>>(out, row_stride, bins);
    HB_HIP(hipGetLastError());
    image_class_counts_kernel<<<dim3(per_image, (unsigned)B), dim3(256), use_lds ? (size_t)bins * 4 : 0, s>>>(gt, pred, hw, G, ignore, has_ignore,
                                                                                                          use_lds, out, row_stride);
    HB_HIP(hipGetLastError());
    return 0;
}

// ---- the resampler --------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t bs_splitmix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one workgroup per replicate: its n_img draws counted into an LDS histogram of n_img counters (<= 128 KiB), written out as row blockIdx.x
__global__ __launch_bounds__(256) void bootstrap_multiplicities_kernel(int n_img, uint64_t base, int64_t r0, int32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int bs_mult[];
    for (int e = threadIdx.x; e < n_img; e += 256) bs_mult[e] = 0;
    __syncthreads();
    const uint64_t row = base + ((uint64_t)(r0 + blockIdx.x) << 32);
    for (int j = threadIdx.x; j < n_img; j += 256) {
        const uint64_t i = __umul64hi(bs_splitmix(row + (uint64_t)j), (uint64_t)n_img);      // < n_img
        atomicAdd(&bs_mult[(int)i], 1);
    }
    __syncthreads();
    int32_t* dst = out + (int64_t)blockIdx.x * n_img;
    for (int e = threadIdx.x; e < n_img; e += 256) dst[e] = bs_mult[e];
}

static int bs_launch_multiplicities(int n_img, uint64_t seed, int64_t r0, int64_t R, int32_t* out, hipStream_t s) {
    if (n_img < 1) return hb_fail("hb_bootstrap_multiplicities: n_img must be positive");
    if (n_img > HB_BOOTSTRAP_MAX_IMAGES)
        return hb_fail("hb_bootstrap_multiplicities: " + std::to_string(n_img) + " images; at most " + std::to_string(HB_BOOTSTRAP_MAX_IMAGES) +
                       " (a replicate's multiplicities are one LDS histogram)");
    if (r0 < 0 || R < 0 || r0 + R > HB_BOOTSTRAP_MAX_REPLICATES) return hb_fail("hb_bootstrap_multiplicities: replicates must lie in [0, 2^20)");
    if (R == 0) return 0;
    if (!out) return hb_fail("hb_bootstrap_multiplicities: out is NULL");
    if (hb_ensure_dyn_lds((const void*)bootstrap_multiplicities_kernel, HB_BOOTSTRAP_MAX_IMAGES * 4)) return -1;
    bootstrap_multiplicities_kernel<<<dim3((unsigned)R), dim3(256), (size_t)n_img * 4, s>>>(n_img, bs_splitmix(seed), r0, out);
    HB_HIP(hipGetLastError());
    return 0;
}

extern "C" int hb_bootstrap_multiplicities(int n_img, uint64_t seed, int64_t r0, int64_t R, int32_t* out, void* stream) {
    hb_range range("hbird:bootstrap_multiplicities");
    return bs_launch_multiplicities(n_img, seed, r0, R, out, (hipStream_t)stream);
}

// ---- the reduction: cnt[r][col] = sum_i W[r][i] * stats[i][col] ----------------------------------------------------------------------------
// A workgroup owns 256 columns x BS_TR replicates: one thread per column with the tile's int64 accumulators in registers (2 x BS_TR VGPRs),
// walking the images with one coalesced stats load each.  The tile's multiplicities are staged BS_IC images at a time into LDS, transposed
// to [image][replicate], so that an image's BS_TR values are one 128-byte line read at a wave-uniform address (broadcast, ds_read_b128).
// The replicate tile is the FAST grid index: the workgroups in flight together cover many replicate tiles of a few column blocks and read the
// same stats lines out of L2 (the table -- 57.6 MB for an ADE20K grid -- is walked once per replicate tile).
// Ragged edges: columns past `cols` load and store nothing, replicates past R carry multiplicity 0 and are not stored.
#define BS_TR 32
#define BS_IC 64
__global__ __launch_bounds__(256) void bootstrap_counts_kernel(const int32_t* __restrict__ stats, int64_t n_img, int64_t cols,
                                                               const int32_t* __restrict__ W, int64_t R, long long* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int wt[BS_IC][BS_TR];
    const int64_t r0 = (int64_t)blockIdx.x * BS_TR;
    const int64_t col = (int64_t)blockIdx.y * 256 + threadIdx.x;
    const bool live = col < cols;
    long long acc[BS_TR];
#pragma unroll
    for (int t = 0; t < BS_TR; ++t) acc[t] = 0;
    for (int64_t i0 = 0; i0 < n_img; i0 += BS_IC) {
        const int ni = (int)std::min<int64_t>(BS_IC, n_img - i0);
        __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int e = threadIdx.x; e < BS_TR * BS_IC; e += 256) {
            const int rr = e / BS_IC, ii = e % BS_IC;       // consecutive lanes: consecutive images of one replicate (coalesced)
            wt[ii][rr] = (r0 + rr < R && ii < ni) ? W[(r0 + rr) * n_img + i0 + ii] : 0;
        }
        __syncthreads();
        if (live) {
            const int32_t* sp = stats + i0 * cols + col;
            for (int ii = 0; ii < ni; ++ii) {
                const long long sv = sp[(int64_t)ii * cols];
#pragma unroll
                for (int t = 0; t < BS_TR; ++t) acc[t] += sv * (long long)wt[ii][t];
            }
        }
    }
    if (live) {
#pragma unroll
        for (int t = 0; t < BS_TR; ++t)
            if (r0 + t < R) out[(r0 + t) * cols + col] = acc[t];
    }
}

static int bs_launch_counts(const int32_t* stats, int64_t n_img, int64_t cols, const int32_t* W, int64_t R, long long* out, hipStream_t s) {
    if (n_img < 1 || cols < 1 || R < 0) return hb_fail("hb_bootstrap_counts: bad shape (n_img, cols >= 1, R >= 0)");
    if (R == 0) return 0;
    if (!stats || !W || !out) return hb_fail("hb_bootstrap_counts: stats / W / out is NULL");
    const int64_t col_blocks = (cols + 255) / 256, r_tiles = (R + BS_TR - 1) / BS_TR;
    if (col_blocks > 65535 || r_tiles > 0x7FFFFFFFLL) return hb_fail("hb_bootstrap_counts: grid too large");
    bootstrap_counts_kernel<<<dim3((unsigned)r_tiles, (unsigned)col_blocks), dim3(256), 0, s>>>(stats, n_img, cols, W, R, out);
    HB_HIP(hipGetLastError());
    return 0;
}

extern "C" int hb_bootstrap_counts(const int32_t* stats, int64_t n_img, int64_t cols, const int32_t* W, int64_t R, int64_t* out, void* stream) {
    hb_range range("hbird:bootstrap_counts");
    return bs_launch_counts(stats, n_img, cols, W, R, reinterpret_cast<long long*>(out), (hipStream_t)stream);
}

// ---- the epilogue: m[r][c] = (sum_g tp / max(tp + fp + fn, 1e-8)) / G, float64, g ascending ------------------------------------------------
// one wave per (replicate, configuration): the lanes read 64 classes' counts (contiguous) and form their terms, lane 0 adds them in order
__global__ __launch_bounds__(64) void bootstrap_miou_kernel(const long long* __restrict__ cnt, int n_cfg, int G, double* __restrict__ out) {
    __shared__ double term[64];
    const int64_t e = blockIdx.x;                           // r * n_cfg + c: the counts of (r, c) start at e * 3 G
    const long long* p = cnt + e * 3 * (int64_t)G;
    double sum = 0.0;
    for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + (int)threadIdx.x;
        __syncthreads();
        if (g < G) {
            const double tp = (double)p[3 * g], fp = (double)p[3 * g + 1], fn = (double)p[3 * g + 2];
            term[threadIdx.x] = tp / fmax(tp + fp + fn, 1e-8);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = std::min(64, G - g0);
            for (int t = 0; t < n; ++t) sum = sum + term[t];
        }
    }
    if (threadIdx.x == 0) out[e] = sum / (double)G;
}

__global__ __launch_bounds__(256) void bootstrap_fill_kernel(int32_t* __restrict__ p, int n, int32_t v) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) p[e] = v;
}

static int bs_launch_miou(const long long* cnt, int64_t R, int n_cfg, int G, double* out, hipStream_t s) {
    if (R == 0) return 0;
    bootstrap_miou_kernel<<<dim3((unsigned)(R * n_cfg)), dim3(64), 0, s>>>(cnt, n_cfg, G, out);
    HB_HIP(hipGetLastError());
    return 0;
}

// ---- the composite --------------------------------------------------------------------------------------------------------------------------
#define BS_WORKSPACE_BYTES (256ull << 20)
extern "C" int hb_bootstrap_miou(const int32_t* stats, int n_img, int n_cfg, int G, uint64_t seed, int64_t R, double* out_point,
                                 double* out_samples, int64_t chunk_replicates, void* stream) {
    hb_range range("hbird:bootstrap_miou");
    if (!stats || !out_point) return hb_fail("hb_bootstrap_miou: stats / out_point is NULL");
    if (n_img < 1 || n_img > HB_BOOTSTRAP_MAX_IMAGES)
        return hb_fail("hb_bootstrap_miou: " + std::to_string(n_img) + " images; between 1 and " + std::to_string(HB_BOOTSTRAP_MAX_IMAGES));
    if (n_cfg < 1 || G < 1 || (long long)n_cfg * 3 * G > 0x7FFFFFFFLL) return hb_fail("hb_bootstrap_miou: bad n_cfg / G");
    if (R < 0 || R > HB_BOOTSTRAP_MAX_REPLICATES) return hb_fail("hb_bootstrap_miou: R must lie in [0, 2^20]");
    if (R > 0 && !out_samples) return hb_fail("hb_bootstrap_miou: out_samples is NULL");
    if (chunk_replicates < 0) return hb_fail("hb_bootstrap_miou: chunk_replicates must not be negative");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t cols = (int64_t)n_cfg * 3 * G;
    const size_t w_row = al256((size_t)n_img * 4), c_row = al256((size_t)cols * 8);
    if (w_row + c_row > BS_WORKSPACE_BYTES) return hb_fail("hb_bootstrap_miou: one replicate's workspace exceeds 256 MiB");
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(R, 1), (int64_t)(BS_WORKSPACE_BYTES / ((size_t)n_img * 4 + (size_t)cols * 8))));
    if (chunk_replicates > 0) chunk = std::min(chunk, chunk_replicates);
    hb_devbuf wbuf, cbuf;                                   // W [chunk][n_img] int32, counts [chunk][cols] int64: within 256 MiB together
    if (wbuf.ensure((size_t)chunk * n_img * 4, HB_GROW_EXACT) || cbuf.ensure((size_t)chunk * cols * 8, HB_GROW_EXACT)) return -1;
    int32_t* W = wbuf.as<int32_t>();
    long long* cnt = cbuf.as<long long>();
    // the point row: W == 1
    bootstrap_fill_kernel<<<dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, s>>>(W, n_img, 1);
    HB_HIP(hipGetLastError());
    if (bs_launch_counts(stats, n_img, cols, W, 1, cnt, s) || bs_launch_miou(cnt, 1, n_cfg, G, out_point, s)) return -1;
    for (int64_t r0 = 0; r0 < R; r0 += chunk) {
        const int64_t rc = std::min(chunk, R - r0);
        if (bs_launch_multiplicities(n_img, seed, r0, rc, W, s) || bs_launch_counts(stats, n_img, cols, W, rc, cnt, s) ||
            bs_launch_miou(cnt, rc, n_cfg, G, out_samples + r0 * n_cfg, s))
            return -1;
    }
    HB_HIP(hipStreamSynchronize(s));                         // the workspace goes with this frame
    return 0;
}
