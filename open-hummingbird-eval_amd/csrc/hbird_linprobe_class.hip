// The image-level linear probe (include/hbird_hip_linprobe_class.h): logits, softmax cross-entropy on one class id per row and its gradient
// over the resident bank for class counts beyond one register tile, and the top-n of a logit table.  gfx950 only.  The definitions are the
// header's; here are the forward and the top-n kernels.  The backward side -- staged rows, the contraction over the rows, the float64 segment
// adds, the loss tree -- is hbird_linprobe.hip's, reached through hbird_linprobe_dev.h.
//
// linprobe_class_forward_kernel: a workgroup of 512 threads keeps 256 rows, a wave one 32-row tile, as linprobe_forward_kernel does, and sweeps
// the classes in groups of at most LPC_SWEEP = 8 class tiles (8 x 16 accumulator registers started at the bias, Wb's fragments staged through
// LDS eight column groups at a time).  The result of a sweep has the class on the lane (lane & 31) and the rows in the registers.
//   pass 1 (every sweep)  raw logits go to the chunk's [rows][cp] buffer; each lane carries the running max of its classes per row
//   pass 2                the row max meets over the half-wave; each lane re-reads its logits and adds expf(z - m) in ascending class order
//   pass 3                the buffer turns from z into R in place; the lane that holds class y writes the row loss
// A lane re-reads only the words it wrote itself (row (v & 3) + 8 (v >> 2) + 4 h of its wave's tile, classes = i mod 32), so no visibility
// between lanes or waves is needed.  An online (rescaling) softmax would save pass 2's read and change the defined bits.
// logits_topn_kernel: one wave per query; a lane keeps the best eight of its classes (c = lane mod 64) in registers, then eight rounds of a
// wave-wide butterfly pick the winners.  No atomic on a float or a double appears in this unit.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include "hbird_linprobe_dev.h"
#include <algorithm>

#define LPC_SWEEP 8                  // class tiles of one sweep: the register budget of linprobe_forward_kernel<8>
#define LPC_TOP 8                    // = HB_VOTE_MAX_TOP of include/hbird_hip_vote.h

struct lpc_fwd_args {
    const float* tiles; int g8; int64_t ntotal;
    int64_t row0;                    // first row of the launch, a multiple of 256
    const float* wt; const float* bias; int C, ct;
    const int32_t* labels;           // [ntotal] class ids, nullptr: logits only
    float* logits;                   // [ntotal][C] (logits only) or nullptr
    float* z;                        // [rows of the launch, padded to 256][32 ct]: raw logits, then residuals
    float* resid_out;                // [ntotal][C] or nullptr
    float* rowloss;                  // [ntotal padded to 256]
    unsigned char* skip;             // [ntotal padded to 256]: 1 for a skipped or padding row
};

// the butterflies of hbird_linprobe.hip (lp_half_max, lp_half_sum), restated: lane ^ X inside each group of 32 lanes, X = 16, 8, 4, 2, 1
template <int X> __device__ __forceinline__ float lpc_swz(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (X << 10) | 0x1f));
}
__device__ __forceinline__ float lpc_half_max(float v) {
    v = fmaxf(v, lpc_swz<16>(v)); v = fmaxf(v, lpc_swz<8>(v)); v = fmaxf(v, lpc_swz<4>(v)); v = fmaxf(v, lpc_swz<2>(v));
    return fmaxf(v, lpc_swz<1>(v));
}
__device__ __forceinline__ float lpc_half_sum(float v) {
    v += lpc_swz<16>(v); v += lpc_swz<8>(v); v += lpc_swz<4>(v); v += lpc_swz<2>(v);
    return v + lpc_swz<1>(v);
}

// One sweep: the class tiles t0 .. t0 + CT - 1 of the wave's 32 rows, linprobe_forward_kernel's stage loop.  -> the mask of the tile's rows
// that are skipped for a non-finite component or lie beyond ntotal (the same value every sweep).
template <int CT, bool LOGITS>
__device__ __forceinline__ unsigned lpc_sweep(const lpc_fwd_args& a, float4* s_w, float* s_m, int t0, int64_t rbase) {
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, i = lane & 31;
    const int64_t rt = rbase >> 5;
    const bool live = rbase < a.ntotal;
    const float4* __restrict__ tiles4 = reinterpret_cast<const float4*>(a.tiles);
    const float4* __restrict__ wt4 = reinterpret_cast<const float4*>(a.wt) + (int64_t)t0 * a.g8 * 64;
    lp_f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const float b = a.bias[(t0 + t) * 32 + i];
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = b;
    }
    int bad = 0;
    for (int g0 = 0; g0 < a.g8; g0 += LP_GC) {
        const int ng = min(LP_GC, a.g8 - g0);
        __syncthreads();                 // the previous groups have been consumed
        for (int e = tid; e < CT * ng * 64; e += LP_THREADS) {
            const int t = e / (ng * 64), rem = e - t * ng * 64;
            s_w[t * LP_GC * 64 + rem] = wt4[((int64_t)t * a.g8 + g0) * 64 + rem];
        }
        float4 av[LP_GC];
#pragma unroll
        for (int gg = 0; gg < LP_GC; ++gg)
            av[gg] = (live && gg < ng) ? tiles4[(rt * (int64_t)a.g8 + g0 + gg) * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
#pragma unroll
        for (int gg = 0; gg < LP_GC; ++gg) {
            if (gg >= ng) break;
            const float4 x = av[gg];
            bad |= (int)!(fabsf(x.x) < INFINITY && fabsf(x.y) < INFINITY && fabsf(x.z) < INFINITY && fabsf(x.w) < INFINITY);
            float4 w[CT];
#pragma unroll
            for (int t = 0; t < CT; ++t) w[t] = s_w[(t * LP_GC + gg) * 64 + lane];
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, w[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, w[t].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, w[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, w[t].w, acc[t], 0, 0, 0);
        }
    }
    // lane = class ((t0 + t) * 32 + i), register v = row (v & 3) + 8 (v >> 2) + 4 h of the wave's tile
    const unsigned long long bm = __ballot(bad);
    const int64_t nvalid = a.ntotal - rbase;
    const unsigned beyond = nvalid >= 32 ? 0u : nvalid <= 0 ? 0xFFFFFFFFu : ~((1u << (int)nvalid) - 1u);
    const unsigned masked = (unsigned)bm | (unsigned)(bm >> 32) | beyond;
    const int C = a.C, cp = a.ct * 32;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int ri = (v & 3) + 8 * (v >> 2) + 4 * h;
        const int64_t r = rbase + ri;
        if (LOGITS) {
            if (!((beyond >> ri) & 1u)) {      // r < ntotal
                const bool off = (masked >> ri) & 1u;
                float* lr = a.logits + rbase * (int64_t)C;      // (uniform over the wave; a row tile's offsets fit 32 bits: 32 rows x C <= 16384)
                const int o = ri * C + t0 * 32 + i, left = C - t0 * 32 - i;      // `left` classes from this lane's first one on
#pragma unroll
                for (int t = 0; t < CT; ++t)
                    if (t * 32 < left) lr[o + t * 32] = off ? 0.0f : acc[t][v];
            }
        } else {
            float* zr = a.z + (r - a.row0) * (int64_t)cp + t0 * 32 + i;
            float mv = t0 ? s_m[v * LP_THREADS] : -INFINITY;      // (the running max waits in LDS while the next sweep's accumulators are live)
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                zr[t * 32] = acc[t][v];
                mv = fmaxf(mv, (t0 + t) * 32 + i < C ? acc[t][v] : -INFINITY);
            }
            s_m[v * LP_THREADS] = mv;
        }
    }
    return masked;
}

// LOGITS: the form of hb_linprobe_class_logits, the sweeps alone with the logits written to [ntotal][C] (one epilogue per instantiation:
// with both in one kernel the compiler spills the accumulators)
template <bool LOGITS>
__global__ __launch_bounds__(LP_THREADS) void linprobe_class_forward_kernel(const lpc_fwd_args a) {
    extern __shared__ float4 s_w[];      // [min(ct, LPC_SWEEP)][LP_GC][64], then the lanes' running row maxima [16][LP_THREADS]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
    const int64_t rbase = a.row0 + (int64_t)blockIdx.x * LP_ROWS + wave * 32;      // (below the index's capacity, a multiple of 256)
    float* s_m = reinterpret_cast<float*>(s_w + min(a.ct, LPC_SWEEP) * LP_GC * 64) + tid;      // (a lane reads its own words only)
    unsigned masked = 0;
    for (int t0 = 0; t0 < a.ct; t0 += LPC_SWEEP) {      // (the branch is uniform over the workgroup: every sweep has its barriers)
        switch (min(LPC_SWEEP, a.ct - t0)) {
            case 8: masked = lpc_sweep<8, LOGITS>(a, s_w, s_m, t0, rbase); break;
            case 7: masked = lpc_sweep<7, LOGITS>(a, s_w, s_m, t0, rbase); break;
            case 6: masked = lpc_sweep<6, LOGITS>(a, s_w, s_m, t0, rbase); break;
            case 5: masked = lpc_sweep<5, LOGITS>(a, s_w, s_m, t0, rbase); break;
            case 4: masked = lpc_sweep<4, LOGITS>(a, s_w, s_m, t0, rbase); break;
            case 3: masked = lpc_sweep<3, LOGITS>(a, s_w, s_m, t0, rbase); break;
            case 2: masked = lpc_sweep<2, LOGITS>(a, s_w, s_m, t0, rbase); break;
            default: masked = lpc_sweep<1, LOGITS>(a, s_w, s_m, t0, rbase); break;
        }
    }
    if (LOGITS) return;
    // a row without a label (-1) is skipped like a non-finite one
    const int64_t rl = rbase + i;
    const int lab_i = rl < a.ntotal ? a.labels[rl] : -1;
    masked |= (unsigned)__ballot(h == 0 && lab_i < 0);
    if (h == 0) a.skip[rl] = (unsigned char)((masked >> i) & 1u);
    const int C = a.C, ct = a.ct, cp = ct * 32;
    float* zb = a.z + (rbase - a.row0) * (int64_t)cp + i;
    int y[16];
    float m[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int ri = (v & 3) + 8 * (v >> 2) + 4 * h;
        y[v] = __shfl(lab_i, ri);        // (lane ri of the first half-wave holds row ri's label)
        m[v] = lpc_half_max(s_m[v * LP_THREADS]);
    }
    // ---- pass 2: se = the lane sums of expf(z - m) over ascending classes, met in the butterfly; lse = m + logf(se)
    float lse[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) lse[v] = 0.0f;
    for (int t = 0; t < ct; ++t) {
        const bool in = t * 32 + i < C;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int ri = (v & 3) + 8 * (v >> 2) + 4 * h;
            const float zz = zb[ri * (int64_t)cp + t * 32];
            lse[v] += in ? expf(zz - m[v]) : 0.0f;
        }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) lse[v] = m[v] + logf(lpc_half_sum(lse[v]));
    // ---- pass 3: R = expf(z - lse) - [c == y] in place of z; the lane of class y keeps z[y] for the row loss
    float zy[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) zy[v] = 0.0f;
    for (int t = 0; t < ct; ++t) {
        const int c = t * 32 + i;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int ri = (v & 3) + 8 * (v >> 2) + 4 * h;
            const int64_t r = rbase + ri;
            const bool off = (masked >> ri) & 1u;
            float* zp = zb + ri * (int64_t)cp + t * 32;
            const float zz = *zp, p = expf(zz - lse[v]);
            const bool hit = c == y[v];
            const float res = (c < C && !off) ? (hit ? p - 1.0f : p) : 0.0f;
            if (hit) zy[v] = zz;
            *zp = res;
            if (a.resid_out && r < a.ntotal && c < C) a.resid_out[r * (int64_t)C + c] = res;
        }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int ri = (v & 3) + 8 * (v >> 2) + 4 * h;
        const bool off = (masked >> ri) & 1u;
        if (off ? i == 0 : i == (y[v] & 31)) a.rowloss[rbase + ri] = off ? 0.0f : lse[v] - zy[v];      // one writer per row
    }
}

// *flag |= 1 for a label outside [-1, C)
__global__ __launch_bounds__(256) void linprobe_class_check_kernel(const int32_t* __restrict__ labels, int64_t n, int C, int32_t* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t lab = labels[r];
    if (lab < -1 || lab >= C) atomicOr(flag, 1);
}

// ---- top-n of a logit table ---------------------------------------------------------------------------------------------------------------------
struct lpc_cand { float v; int c; };      // c < 0: empty
// a ranks before b: a number before nothing, the larger logit, then the lower class id
__device__ __forceinline__ bool lpc_before(const lpc_cand& a, const lpc_cand& b) {
    return a.c >= 0 && (b.c < 0 || a.v > b.v || (a.v == b.v && a.c < b.c));
}

__global__ __launch_bounds__(256) void logits_topn_kernel(const float* __restrict__ logits, int64_t nq, int C, int topn, int32_t* __restrict__ pred) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += waves) {
        lpc_cand best[LPC_TOP];
#pragma unroll
        for (int j = 0; j < LPC_TOP; ++j) best[j] = lpc_cand{0.0f, -1};
        const float* row = logits + q * (int64_t)C;
        for (int c = lane; c < C; c += 64) {
            const float z = row[c];
            lpc_cand x{z, z == z ? c : -1};      // a NaN logit is no candidate
#pragma unroll
            for (int j = 0; j < LPC_TOP; ++j)
                if (lpc_before(x, best[j])) { const lpc_cand o = best[j]; best[j] = x; x = o; }
        }
        for (int slot = 0; slot < topn; ++slot) {
            lpc_cand w = best[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const lpc_cand other{__shfl_xor(w.v, o), __shfl_xor(w.c, o)};
                if (lpc_before(other, w)) w = other;
            }
            if (w.c >= 0 && w.c == best[0].c) {      // the winner's lane moves on to its next candidate
#pragma unroll
                for (int j = 0; j + 1 < LPC_TOP; ++j) best[j] = best[j + 1];
                best[LPC_TOP - 1] = lpc_cand{0.0f, -1};
            }
            if (lane == 0) pred[q * topn + slot] = w.c >= 0 ? w.c : -1;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
namespace {
int lpc_check_c(const char* who, int C) {
    if (C < 1 || C > HB_LINPROBE_CLASS_MAX_C)
        return hb_fail(std::string(who) + ": C must be in [1, " + std::to_string(HB_LINPROBE_CLASS_MAX_C) + "], got " + std::to_string(C));
    return 0;
}

int lpc_forward(const lpc_fwd_args& a, int64_t rows_pad, hipStream_t s) {
    const int lds = std::min(a.ct, LPC_SWEEP) * LP_GC * 1024 + (a.logits ? 0 : 16 * LP_THREADS * 4);
    const int most = LPC_SWEEP * LP_GC * 1024 + 16 * LP_THREADS * 4;      // (the attribute is set once per kernel: the largest launch there is)
    const dim3 grid((unsigned)(rows_pad / LP_ROWS)), block(LP_THREADS);
    if (a.logits) {
        if (hb_ensure_dyn_lds((const void*)linprobe_class_forward_kernel<true>, most)) return -1;
        linprobe_class_forward_kernel<true><<<grid, block, lds, s>>>(a);
    } else {
        if (hb_ensure_dyn_lds((const void*)linprobe_class_forward_kernel<false>, most)) return -1;
        linprobe_class_forward_kernel<false><<<grid, block, lds, s>>>(a);
    }
    HB_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int hb_linprobe_class_logits(hb_index_t* ix, const float* Wb, int C, float* out) {
    if (!ix) return hb_fail("hb_linprobe_class_logits: NULL index handle");
    if (!Wb || !out) return hb_fail("hb_linprobe_class_logits: NULL pointer");
    if (lpc_check_c("hb_linprobe_class_logits", C)) return -1;
    if (ix->ntotal < 1) return hb_fail("hb_linprobe_class_logits: the index is empty");
    hb_range range("hbird:linprobe_class_logits");
    HB_HIP(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    lp_params par;
    if (par.make(ix, Wb, C, s)) return -1;
    lpc_fwd_args a{};
    a.tiles = ix->tiles; a.g8 = ix->g8; a.ntotal = ix->ntotal; a.row0 = 0;
    a.wt = par.wt; a.bias = par.bias; a.C = C; a.ct = par.ct; a.logits = out;
    const int rc = lpc_forward(a, (ix->ntotal + LP_ROWS - 1) / LP_ROWS * LP_ROWS, s);
    HB_HIP(hipStreamSynchronize(s));      // (the re-tiled parameters go with the call)
    return rc;
}

extern "C" int hb_linprobe_class_loss_grad(hb_index_t* bank, const int32_t* labels, const float* Wb, int C, double l2, double* loss_host, double* grad,
                                           int64_t* used_host, float* resid_opt) {
    if (!bank) return hb_fail("hb_linprobe_class_loss_grad: NULL index handle");
    if (!labels || !Wb || !loss_host || !grad || !used_host) return hb_fail("hb_linprobe_class_loss_grad: NULL pointer");
    if (lpc_check_c("hb_linprobe_class_loss_grad", C)) return -1;
    if (bank->ntotal < 1) return hb_fail("hb_linprobe_class_loss_grad: the bank is empty");
    const int64_t n = bank->ntotal;
    hb_range range("hbird:linprobe_class_loss_grad");
    HB_HIP(hipSetDevice(bank->device));
    hipStream_t s = bank->stream;
    {   // the labels first: one small flag launch and a read of the flag, before any output is written
        hb_dev<int32_t> flag;
        if (flag.ensure(256, HB_GROW_EXACT)) return -1;
        HB_HIP(hipMemsetAsync(flag, 0, 4, s));
        linprobe_class_check_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(labels, n, C, flag);
        HB_HIP(hipGetLastError());
        int32_t bad = 0;
        HB_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
        if (bad) return hb_fail("hb_linprobe_class_loss_grad: a label lies outside [-1, " + std::to_string(C) + ")");
    }
    const int d = bank->d, d1 = d + 1, xs = (d1 + 31) / 32 * 32;
    int64_t seg_rows = 0; int nseg = 0;
    if (hb_linprobe_partition(n, &seg_rows, &nseg)) return -1;
    lp_params par;
    if (par.make(bank, Wb, C, s)) return -1;
    const int cp = par.ct * 32;
    // the bank in row chunks of whole segments: logits / residuals [rows][cp], staged rows [rows][xs], segment partials [segments][cp][xs]
    const int64_t seg_bytes = seg_rows * (int64_t)(cp + xs) * 4;
    const int chunk_segs = (int)std::min<int64_t>(nseg, std::max<int64_t>(1, hb_lp_workspace() / seg_bytes));
    const int64_t chunk_rows = (int64_t)chunk_segs * seg_rows, npad = (n + LP_ROWS - 1) / LP_ROWS * LP_ROWS;
    const int64_t chunk_pad = std::min(chunk_rows, npad);
    hb_dev<float> resid, X, partial, rowloss; hb_dev<unsigned char> skip; hb_dev<double> tree, scal;
    if (resid.ensure((size_t)chunk_pad * cp * 4, HB_GROW_EXACT) || X.ensure((size_t)chunk_pad * xs * 4, HB_GROW_EXACT)
        || partial.ensure((size_t)chunk_segs * cp * xs * 4, HB_GROW_EXACT) || rowloss.ensure((size_t)npad * 4, HB_GROW_EXACT)
        || skip.ensure((size_t)npad, HB_GROW_EXACT) || tree.ensure(2 * LP_TREE_BLOCKS * 8, HB_GROW_EXACT) || scal.ensure(3 * 8, HB_GROW_EXACT)) return -1;
    const int64_t total = (int64_t)C * d1;
    HB_HIP(hipMemsetAsync(grad, 0, (size_t)total * 8, s));
    lpc_fwd_args a{};
    a.tiles = bank->tiles; a.g8 = bank->g8; a.ntotal = n;
    a.wt = par.wt; a.bias = par.bias; a.C = C; a.ct = par.ct;
    a.labels = labels; a.z = resid; a.resid_out = resid_opt; a.rowloss = rowloss; a.skip = skip;
    int rc = 0;
    for (int seg0 = 0; seg0 < nseg && !rc; seg0 += chunk_segs) {
        const int segs = std::min(chunk_segs, nseg - seg0);
        a.row0 = (int64_t)seg0 * seg_rows;
        const int64_t rows = std::min(n, a.row0 + (int64_t)segs * seg_rows) - a.row0, rows_pad = (rows + LP_ROWS - 1) / LP_ROWS * LP_ROWS;
        if (lpc_forward(a, rows_pad, s) || hb_lp_stage_rows(bank, a.row0, rows_pad, skip, X, xs, s)
            || hb_lp_backward(par.ct, resid, X, xs, seg_rows, rows_pad, segs, partial, s) || hb_lp_reduce(partial, segs, cp, xs, C, d1, grad, s)) rc = -1;
    }
    double h[3] = {0.0, 0.0, 0.0};
    if (!rc) {
        if (hb_lp_loss_tree(rowloss, skip, n, tree, Wb, total, scal, s)) rc = -1;
        else if (hipMemcpyAsync(h, scal, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess) rc = hb_fail("hb_linprobe_class_loss_grad: the loss did not come back");
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = hb_fail("hb_linprobe_class_loss_grad: the stream failed");
    if (rc) return rc;
    *used_host = (int64_t)h[1];
    if (h[1] < 1.0) return hb_fail("hb_linprobe_class_loss_grad: every row of the bank is skipped (a non-finite component or label -1)");
    *loss_host = h[0] / h[1] + 0.5 * l2 * h[2];
    if (hb_lp_finish(grad, Wb, total, h[1], l2, s)) return -1;
    HB_HIP(hipStreamSynchronize(s));      // (the workspace goes with the call)
    return 0;
}

extern "C" int hb_logits_topn(const float* logits, int64_t nq, int C, int topn, int32_t* pred, void* hip_stream) {
    hb_range range("hbird:logits_topn");
    if (!logits || !pred) return hb_fail("hb_logits_topn: NULL pointer");
    if (nq < 0) return hb_fail("hb_logits_topn: nq must not be negative");
    if (lpc_check_c("hb_logits_topn", C)) return -1;
    if (topn < 1 || topn > LPC_TOP) return hb_fail("hb_logits_topn: topn outside [1, " + std::to_string(LPC_TOP) + "]");
    if (nq == 0) return 0;
    logits_topn_kernel<<<dim3((unsigned)std::min<int64_t>((nq + 3) / 4, 1 << 20)), dim3(256), 0, (hipStream_t)hip_stream>>>(logits, nq, C, topn, pred);
    HB_HIP(hipGetLastError());
    return 0;
}
