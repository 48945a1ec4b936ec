// Sub-bank views: an index made of selected rows of another index, on the device (hb_index_add_from, hb_index_select_rows).
//
// Why views nest in the banks this engine builds.  The bounded build keeps, per (epoch, image), the K = max(1, memory_size //
// (dataset_size * augmentation_epoch)) patches with the smallest noisy scores (reference hbird_eval.py:146-147), in ascending score order
// with ties to the lower patch index (hbird_eval.py:497-511: the noise torch.rand(total_nz) is drawn per batch and does not depend on K,
// the K smallest of one fixed score vector are a prefix of the K' >= K smallest).  So the bank of memory_size m is, row for row and bit for
// bit, the first K_m rows of every block of K_M rows of the bank of M >= m; and in the unbounded build an image subset is the rows of those
// images.  A view is therefore a row gather -- no ViT pass, no sampling.
//
// The gather is fragment tiles -> fragment tiles (layout: hbird_layout.hip).  One row's share of block (rt, g) is two 16-byte pieces at
// float offset ((rt * G8) + g) * 256 + (h * 32 + i) * 4, h = 0, 1; a destination block's 64 pieces are one contiguous 1 KiB.  A wave owns
// whole destination blocks: lane l = h * 32 + i loads the piece of ids[...] in the source tiles and stores piece l, 16 bytes each way, so
// the writes are fully coalesced, and for runs of consecutive source rows (prefixes of per-image blocks: the expected input) adjacent lanes
// read adjacent pieces too.  Fully random ids use one 16-byte piece of every line they touch.  The per-row constants --
// the accumulator init (L2: -0.5 |b|^2) and the norm -- are copied verbatim, nothing is recomputed; label rows are copied in their stored
// form (uint16 counts as 16-byte pieces, fp32 rows as floats).  HBM-bound: every byte of the view is read once and written once.
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include <algorithm>

// bit 0: an id outside [0, rows); bit 1: an id without a label row (>= lab_rows).  Sticky; read back once per call.
__global__ __launch_bounds__(256) void select_check_ids_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t rows, int64_t lab_rows,
                                                               int* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t id = ids[t];
    const int f = (id < 0 || id >= rows) ? 1 : (id >= lab_rows ? 2 : 0);
    if (f) atomicOr(flag, f);
}

// One workgroup per destination row tile (32 rows), four waves; wave w copies the k8 groups g = w, w + 4, ... (four 16-byte loads in
// flight per lane).  Destination rows are row0 + j, j in [0, n): lanes whose row lies outside that range store nothing, so the rows before
// row0 keep their values and the rows of the last tile beyond the new ntotal keep what hb_index_reserve / hb_index_reset left (zero tiles,
// binit = -inf, bnorm = 0).  An id outside the source (the caller has checked: select_check_ids_kernel) is skipped, never read.
__global__ __launch_bounds__(256) void tiles_select_rows_kernel(const float* __restrict__ src, int64_t src_rows, int g8,
                                                                const int64_t* __restrict__ ids, int64_t n, int64_t row0,
                                                                float* __restrict__ dst, const float* __restrict__ src_binit,
                                                                const float* __restrict__ src_bnorm, float* __restrict__ dst_binit,
                                                                float* __restrict__ dst_bnorm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int64_t rt = (row0 >> 5) + blockIdx.x;
    const int64_t j = rt * 32 + i - row0;
    if (j < 0 || j >= n) return;
    const int64_t sid = ids[j];
    if (sid < 0 || sid >= src_rows) return;
    const float4* sp = reinterpret_cast<const float4*>(src + ((sid >> 5) * (int64_t)g8) * HB_BLK + (h * 32 + (int)(sid & 31)) * 4);
    float4* dp = reinterpret_cast<float4*>(dst + (rt * (int64_t)g8) * HB_BLK + lane * 4);
    constexpr int B4 = HB_BLK / 4;      // float4 per block
    int g = w;
    for (; g + 12 < g8; g += 16) {      // four loads in flight, then four stores
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = sp[(int64_t)(g + 4 * u) * B4];
#pragma unroll
        for (int u = 0; u < 4; ++u) dp[(int64_t)(g + 4 * u) * B4] = v[u];
    }
    for (; g < g8; g += 4) dp[(int64_t)g * B4] = sp[(int64_t)g * B4];
    if (w == 0 && h == 0) {
        dst_binit[row0 + j] = src_binit[sid];
        dst_bnorm[row0 + j] = src_bnorm[sid];
    }
}

// Label rows in their stored form: T = uint4 (16-byte pieces: uint16 count rows, fp32 rows of a multiple of four classes) or float.
// One thread per destination piece: the writes are dense.
template <typename T>
__global__ __launch_bounds__(256) void select_label_rows_kernel(const T* __restrict__ src, int64_t src_rows, int per_row,
                                                                const int64_t* __restrict__ ids, int64_t n, T* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * per_row) return;
    const int64_t r = t / per_row;
    const int p = (int)(t - r * per_row);
    const int64_t sid = ids[r];
    if (sid < 0 || sid >= src_rows) return;
    dst[t] = src[sid * per_row + p];
}

extern "C" int hb_index_add_from(hb_index_t* dst, const hb_index_t* src, const int64_t* ids, int64_t n, int ids_on_device) {
    if (!dst || !src) return hb_fail("hb_index_add_from: NULL index handle");
    if (n < 0) return hb_fail("hb_index_add_from: negative row count");
    if (src == dst) return hb_fail("hb_index_add_from: src and dst are the same index");
    if (src->d != dst->d) return hb_fail("hb_index_add_from: the indexes differ in d (" + std::to_string(src->d) + " vs " + std::to_string(dst->d) + ")");
    if (src->metric != dst->metric) return hb_fail("hb_index_add_from: the indexes differ in metric");
    if (src->device != dst->device) return hb_fail("hb_index_add_from: the indexes live on different devices");
    const bool labs = src->lab.own_rows();
    if (labs) {
        if (dst->lab.rows() != dst->ntotal) return hb_fail("hb_index_add_from: the destination's label rows do not cover its rows (nlabels != ntotal)");
        if (dst->ntotal > 0 && (dst->lab.classes() != src->lab.classes() || dst->lab.denominator() != src->lab.denominator()))
            return hb_fail("hb_index_add_from: the destination holds label rows of another class count or label denominator");
    }
    if (n == 0) return 0;
    if (!ids) return hb_fail("hb_index_add_from: ids is NULL");
    hb_range range("hbird:index_add_from");
    HB_HIP(hipSetDevice(dst->device));
    hipStream_t s = dst->stream;
    // the source may still be appending on its own stream
    if (src->stream != s) {
        hipEvent_t ev = nullptr;
        HB_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, src->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);
        (void)hipEventDestroy(ev);
        if (e != hipSuccess) return hb_fail(std::string("hb_index_add_from: ") + hipGetErrorString(e));
    }
    // staging in dst->tmp: [flag, 256 B] [ids (host path)]
    if (dst->tmp.ensure(256 + (ids_on_device ? 0 : (size_t)n * 8), HB_GROW_EXACT)) return -1;
    int* flag = dst->tmp.as<int>();
    const int64_t* d_ids = ids;
    if (!ids_on_device) {
        HB_HIP(hipMemcpyAsync(dst->tmp + 256, ids, (size_t)n * 8, hipMemcpyHostToDevice, s));
        d_ids = dst->tmp.as<const int64_t>(256);
    }
    HB_HIP(hipMemsetAsync(flag, 0, 4, s));
    select_check_ids_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(d_ids, n, src->ntotal, labs ? src->lab.rows() : src->ntotal, flag);
    HB_HIP(hipGetLastError());
    int bad = 0;
    HB_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));
    if (bad & 1) return hb_fail("hb_index_add_from: an id lies outside [0, " + std::to_string(src->ntotal) + ") (the source's rows)");
    if (bad & 2) return hb_fail("hb_index_add_from: an id lies beyond the source's " + std::to_string(src->lab.rows()) + " label rows");
    // nothing of the destination has changed so far; from here on the call only fails where hb_index_add would
    if (dst->ntotal + n > dst->cap_rows) {
        const int64_t want = std::max<int64_t>(dst->ntotal + n, dst->cap_rows + dst->cap_rows / 2);
        if (hb_index_reserve(dst, want)) return -1;
    }
    if (labs) {
        // an empty destination adopts the source's class count and label denominator (a failing allocation leaves them as they were)
        hb_label_form old = dst->lab.form();
        if (dst->ntotal == 0) {
            if (dst->lab.adopt_drops(src->lab.classes(), src->lab.denominator())) HB_HIP(hipStreamSynchronize(s));
            old = dst->lab.adopt(src->lab.classes(), src->lab.denominator());
        }
        if (hb_labels_ensure(dst, src->lab.classes(), n)) { dst->lab.restore(old); return -1; }
    }
    const int64_t row0 = dst->ntotal;
    const int64_t n_rt = ((row0 + n - 1) >> 5) - (row0 >> 5) + 1;
    tiles_select_rows_kernel<<<dim3((unsigned)n_rt), dim3(256), 0, s>>>(src->tiles, src->ntotal, src->g8, d_ids, n, row0, dst->tiles, src->binit,
                                                                         src->bnorm, dst->binit, dst->bnorm);
    HB_HIP(hipGetLastError());
    if (labs) {
        const size_t row_bytes = dst->lab.row_bytes();
        if (row_bytes % 16 == 0) {
            const int per = (int)(row_bytes / 16);
            select_label_rows_kernel<uint4><<<dim3((unsigned)((n * per + 255) / 256)), dim3(256), 0, s>>>(src->lab.own_base<const uint4>(), src->lab.rows(), per, d_ids, n,
                                                                                                         dst->lab.own_tail<uint4>());
        } else {
            const int per = dst->lab.classes();
            select_label_rows_kernel<float><<<dim3((unsigned)((n * per + 255) / 256)), dim3(256), 0, s>>>(src->lab.own_base<const float>(), src->lab.rows(), per, d_ids, n,
                                                                                                         dst->lab.own_tail<float>());
        }
        HB_HIP(hipGetLastError());
    }
    // max bank-row norm over the new rows, as hb_index_add: the fp16 screen's certificate is bounded by it
    if (hb_launch_bnorm_max(dst->bnorm + row0, n, dst->bmax, s)) return -1;
    dst->ntotal += n;
    if (labs) dst->lab.appended(n, false);      // (no conversion happened: nothing new to check)
    return dst->bank_changed(HB_BANK_APPENDED);      // (the lazy copies follow at the next screened search, as after hb_index_add)
}

extern "C" int hb_index_select_rows(const hb_index_t* src, const int64_t* ids, int64_t n, int ids_on_device, hb_index_t** out) {
    if (!out) return hb_fail("hb_index_select_rows: out is NULL");
    *out = nullptr;
    if (!src) return hb_fail("hb_index_select_rows: NULL index handle");
    if (n < 0) return hb_fail("hb_index_select_rows: negative row count");
    if (n > 0 && !ids) return hb_fail("hb_index_select_rows: ids is NULL");
    hb_index_t* v = nullptr;
    if (hb_index_create(src->d, src->metric, src->device, &v)) return -1;
    v->stream = src->stream;      // (the view's work is queued where the source's is; hb_index_set_stream moves it)
    if (src->lab.own_rows()) v->lab.adopt(src->lab.classes(), src->lab.denominator());
    if (hb_index_reserve(v, n) || hb_index_add_from(v, src, ids, n, ids_on_device)) {
        const std::string msg = hb_last_error();
        hb_index_free(v);
        return hb_fail(msg);
    }
    *out = v;
    return 0;
}
