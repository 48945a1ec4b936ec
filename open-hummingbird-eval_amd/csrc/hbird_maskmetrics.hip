// The label map of a rectangular frame and the counts behind J and F (include/hbird_hip_propagate.h, DESIGN.md section 4 "Video label
// propagation").  Plain VALU / integer code; no MFMA, no floating-point atomic.
//
// mask_extrema_kernel + mask_argmax_kernel (hb_mask_upsample_argmax): one thread per output pixel walks the channels with K6's four taps
// (hbird_post.hip) on a gh x gw grid.  With channel_norm the first launch brings every (image, channel)'s minimum and maximum of the
// upsampled values together -- wave butterfly, then integer atomicMin / atomicMax on the order-preserving unsigned image of the float, exact
// in any order -- and the second launch recomputes the same floats (the same uncontracted operations), normalises and takes the argmax.
//
// jf_counts_kernel (hb_mask_jf_counts): a workgroup owns a 32 x 32 pixel tile of one (image, object).  It stages both boundary maps of the
// tile grown by bound_px (a halo tile in LDS, zero outside the image), then every pixel counts its six terms: a boundary pixel looks for a
// boundary pixel of the other map inside the disk.  Counts meet in LDS integers, then one integer atomicAdd per count and workgroup.
#include "../../include/hbird_hip.h"
#include "../../include/hbird_hip_propagate.h"
#include "hbird_internal.h"
#include <algorithm>
#include <cmath>

// the upsampled value and the normalisation are stated sequences of rounded fp32 operations
#pragma clang fp contract(off)

// ---- upsample + channel norm + argmax ----------------------------------------------------------------------------------------------------
struct mk_taps { int i00, i01, i10, i11; float ly0, ly1, lx0, lx1; };

__device__ __forceinline__ void mk_axis(float scale, int dst, int G, int* i0, int* i1, float* l0, float* l1) {
    const float f = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    *i0 = min((int)floorf(f), G - 1);
    *i1 = min(*i0 + 1, G - 1);
    *l1 = f - (float)*i0;
    *l0 = 1.0f - *l1;
}

__device__ __forceinline__ mk_taps mk_pixel(float sy, float sx, int y, int x, int gh, int gw, int c) {
    int y0, y1, x0, x1;
    mk_taps t;
    mk_axis(sy, y, gh, &y0, &y1, &t.ly0, &t.ly1);
    mk_axis(sx, x, gw, &x0, &x1, &t.lx0, &t.lx1);
    t.i00 = (y0 * gw + x0) * c; t.i01 = (y0 * gw + x1) * c; t.i10 = (y1 * gw + x0) * c; t.i11 = (y1 * gw + x1) * c;
    return t;
}

__device__ __forceinline__ float mk_value(const float* __restrict__ img, const mk_taps& t, int ch) {
    const float top = t.lx0 * img[t.i00 + ch] + t.lx1 * img[t.i01 + ch];
    const float bot = t.lx0 * img[t.i10 + ch] + t.lx1 * img[t.i11 + ch];
    return t.ly0 * top + t.ly1 * bot;
}

// float <-> unsigned, order-preserving (negative floats below positive ones)
__device__ __forceinline__ unsigned mk_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mk_unkey(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key); }

// ext [B][c][2] unsigned keys: {min, max}, initialised to {0xFFFFFFFF, 0}
__global__ __launch_bounds__(256) void mask_extrema_kernel(const float* __restrict__ labels, int gh, int gw, int c, int h, int w, float sy, float sx,
                                                           unsigned* __restrict__ ext) {
    const int64_t b = blockIdx.y;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x, hw = (int64_t)h * w;
    const bool live = pix < hw;
    const int64_t pc = live ? pix : hw - 1;                 // lanes past the image repeat its last pixel: extrema are idempotent
    const mk_taps t = mk_pixel(sy, sx, (int)(pc / w), (int)(pc % w), gh, gw, c);
    const float* img = labels + b * (int64_t)gh * gw * c;
    for (int ch = 0; ch < c; ++ch) {
        const unsigned key = mk_key(mk_value(img, t, ch));
        unsigned lo = key, hi = key;
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
            hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
        }
        if ((threadIdx.x & 63) == 0) {
            // the extrema only ever move outwards: a wave whose own do not beat what it reads (however stale) has nothing to add, and
            // thousands of waves stop queueing on one address
            unsigned* e = ext + (b * c + ch) * 2;
            if (lo < __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(e, lo);
            if (hi > __hip_atomic_load(e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(e + 1, hi);
        }
    }
}

__global__ __launch_bounds__(256) void mask_argmax_kernel(const float* __restrict__ labels, int gh, int gw, int c, int h, int w, float sy, float sx,
                                                          const unsigned* __restrict__ ext, int64_t* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x, hw = (int64_t)h * w;
    if (pix >= hw) return;
    const mk_taps t = mk_pixel(sy, sx, (int)(pix / w), (int)(pix % w), gh, gw, c);
    const float* img = labels + b * (int64_t)gh * gw * c;
    float best = 0.0f;
    int arg = 0;
    for (int ch = 0; ch < c; ++ch) {
        float v = mk_value(img, t, ch);
        if (ext) {
            const float mn = mk_unkey(ext[(b * c + ch) * 2]), mx = mk_unkey(ext[(b * c + ch) * 2 + 1]);
            if (mx > 0.0f && mx > mn) v = (v - mn) / (mx - mn);
        }
        if (ch == 0 || v > best) { best = v; arg = ch; }   // first maximum wins
    }
    out[b * hw + pix] = arg;
}

__global__ void mask_extrema_init_kernel(unsigned* ext, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ext[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
}

extern "C" int hb_mask_upsample_argmax(const float* labels, int64_t B, int gh, int gw, int c, int h, int w, int channel_norm, int64_t* out,
                                       void* hip_stream) {
    hb_range range("hbird:mask_upsample_argmax");
    const std::string who = "hb_mask_upsample_argmax: ";
    if (!labels || !out) return hb_fail(who + "NULL pointer");
    if (B <= 0 || gh <= 0 || gw <= 0 || c <= 0 || h <= 0 || w <= 0) return hb_fail(who + "B, gh, gw, c, h and w must be positive");
    if (c > HB_PROPAGATE_MAX_C) return hb_fail(who + "c exceeds the limit " + std::to_string(HB_PROPAGATE_MAX_C));
    if ((long long)gh * gw * c >= (1LL << 31)) return hb_fail(who + "gh * gw * c exceeds the limit 2^31 - 1");
    const long long pblocks = ((long long)h * w + 255) / 256;
    if (pblocks > 0x7FFFFFFFLL || B > 65535) return hb_fail(who + "launch grid exceeds the limit (h * w / 256 workgroups, B <= 65535)");
    hipStream_t s = (hipStream_t)hip_stream;
    const float sy = (float)gh / (float)h, sx = (float)gw / (float)w;
    const dim3 grid((unsigned)pblocks, (unsigned)B);
    if (!channel_norm) {
        mask_argmax_kernel<<<grid, dim3(256), 0, s>>>(labels, gh, gw, c, h, w, sy, sx, nullptr, out);
        HB_HIP(hipGetLastError());
        return 0;
    }
    hb_dev<unsigned> ext;                                   // [B][c][2], a local of this call
    const int64_t n_ext = B * c * 2;
    if (ext.ensure((size_t)n_ext * sizeof(unsigned), HB_GROW_EXACT)) return -1;
    mask_extrema_init_kernel<<<dim3((unsigned)((n_ext + 255) / 256)), dim3(256), 0, s>>>(ext, n_ext);
    HB_HIP(hipGetLastError());
    mask_extrema_kernel<<<grid, dim3(256), 0, s>>>(labels, gh, gw, c, h, w, sy, sx, ext);
    HB_HIP(hipGetLastError());
    mask_argmax_kernel<<<grid, dim3(256), 0, s>>>(labels, gh, gw, c, h, w, sy, sx, ext, out);
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(s));                        // the extrema are a local of this call
    return 0;
}

// ---- J and F counts ------------------------------------------------------------------------------------------------------------------------
#define JF_TILE 32
#define JF_EXT (JF_TILE + 2 * HB_JF_MAX_BOUND)

__device__ __forceinline__ int jf_is(const int64_t* __restrict__ m, int h, int w, int y, int x, int64_t o) { return m[(int64_t)y * w + x] == o; }

// the toolkit's seg2bmap at equal size, at a pixel inside the image
__device__ __forceinline__ int jf_bmap(const int64_t* __restrict__ m, int h, int w, int y, int x, int64_t o) {
    const int M = jf_is(m, h, w, y, x, o);
    const bool lastrow = y == h - 1, lastcol = x == w - 1;
    if (lastrow && lastcol) return 0;
    if (lastrow) return M ^ jf_is(m, h, w, y, x + 1, o);
    if (lastcol) return M ^ jf_is(m, h, w, y + 1, x, o);
    return (M ^ jf_is(m, h, w, y, x + 1, o)) | (M ^ jf_is(m, h, w, y + 1, x, o)) | (M ^ jf_is(m, h, w, y + 1, x + 1, o));
}

__device__ __forceinline__ int jf_near(const unsigned char* map, int ext, int cy, int cx, int R) {
    for (int dy = -R; dy <= R; ++dy) {
        const int span = (int)floorf(sqrtf((float)(R * R - dy * dy)));          // exact for R <= 32: corrected below all the same
        int sp = span;
        while ((sp + 1) * (sp + 1) + dy * dy <= R * R) ++sp;
        while (sp > 0 && sp * sp + dy * dy > R * R) --sp;
        const unsigned char* row = map + (cy + dy) * ext + cx;
        for (int dx = -sp; dx <= sp; ++dx)
            if (row[dx]) return 1;
    }
    return 0;
}

__global__ __launch_bounds__(256) void jf_counts_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int h, int w, int n_objects,
                                                        int R, unsigned long long* __restrict__ counts) {
    __shared__ unsigned char bp[JF_EXT * JF_EXT], bg[JF_EXT * JF_EXT];
    __shared__ unsigned cnt[HB_JF_NCOUNTS];
    const int tiles_x = (w + JF_TILE - 1) / JF_TILE;
    const int ty0 = ((int)blockIdx.x / tiles_x) * JF_TILE, tx0 = ((int)blockIdx.x % tiles_x) * JF_TILE;
    const int64_t o = (int64_t)blockIdx.y + 1, b = blockIdx.z;
    const int64_t* P = pred + b * (int64_t)h * w;
    const int64_t* G = gt + b * (int64_t)h * w;
    const int ext = JF_TILE + 2 * R;
    if (threadIdx.x < HB_JF_NCOUNTS) cnt[threadIdx.x] = 0;
    for (int e = threadIdx.x; e < ext * ext; e += 256) {
        const int y = ty0 - R + e / ext, x = tx0 - R + e % ext;
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        bp[e] = in ? (unsigned char)jf_bmap(P, h, w, y, x, o) : 0;
        bg[e] = in ? (unsigned char)jf_bmap(G, h, w, y, x, o) : 0;
    }
    __syncthreads();
    unsigned mine[HB_JF_NCOUNTS] = {0, 0, 0, 0, 0, 0};
    for (int e = threadIdx.x; e < JF_TILE * JF_TILE; e += 256) {
        const int ly = e / JF_TILE, lx = e % JF_TILE, y = ty0 + ly, x = tx0 + lx;
        if (y >= h || x >= w) continue;
        const int p = jf_is(P, h, w, y, x, o), g = jf_is(G, h, w, y, x, o);
        mine[HB_JF_INTER] += p & g;
        mine[HB_JF_UNION] += p | g;
        const int at = (ly + R) * ext + lx + R;
        if (bp[at]) { mine[HB_JF_NFG] += 1; mine[HB_JF_FG_MATCH] += jf_near(bg, ext, ly + R, lx + R, R); }
        if (bg[at]) { mine[HB_JF_NGT] += 1; mine[HB_JF_GT_MATCH] += jf_near(bp, ext, ly + R, lx + R, R); }
    }
#pragma unroll
    for (int i = 0; i < HB_JF_NCOUNTS; ++i)
        if (mine[i]) atomicAdd(&cnt[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < HB_JF_NCOUNTS && cnt[threadIdx.x])
        atomicAdd(counts + (b * n_objects + (o - 1)) * HB_JF_NCOUNTS + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

extern "C" int hb_mask_jf_counts(const int64_t* pred, const int64_t* gt, int64_t B, int h, int w, int n_objects, int bound_px, int64_t* counts_out,
                                 void* hip_stream) {
    hb_range range("hbird:mask_jf_counts");
    const std::string who = "hb_mask_jf_counts: ";
    if (!pred || !gt || !counts_out) return hb_fail(who + "NULL pointer");
    if (B <= 0 || h <= 0 || w <= 0 || n_objects <= 0) return hb_fail(who + "B, h, w and n_objects must be positive");
    if (bound_px < 0 || bound_px > HB_JF_MAX_BOUND) return hb_fail(who + "bound_px outside [0, " + std::to_string(HB_JF_MAX_BOUND) + "]: limit");
    const long long tiles = (long long)((h + JF_TILE - 1) / JF_TILE) * ((w + JF_TILE - 1) / JF_TILE);
    if (tiles > 0x7FFFFFFFLL || n_objects > 65535 || B > 65535) return hb_fail(who + "launch grid exceeds the limit (n_objects, B <= 65535)");
    hipStream_t s = (hipStream_t)hip_stream;
    HB_HIP(hipMemsetAsync(counts_out, 0, (size_t)B * n_objects * HB_JF_NCOUNTS * sizeof(int64_t), s));
    jf_counts_kernel<<<dim3((unsigned)tiles, (unsigned)n_objects, (unsigned)B), dim3(256), 0, s>>>(pred, gt, h, w, n_objects, bound_px,
                                                                                                  reinterpret_cast<unsigned long long*>(counts_out));
    HB_HIP(hipGetLastError());
    return 0;
}
