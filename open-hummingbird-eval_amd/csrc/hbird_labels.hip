// The label entries of libhbird_hip.so: the HIP side of hb_label_store (hbird_labels.h), which decides; here the synchronisations before a
// drop, the flag's memset and read-back, the staging of host pointers, and the conversion / gather launches (kernels: hbird_aggregate.hip,
// hbird_bank.hip).
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"

extern "C" int64_t hb_index_nlabels(const hb_index_t* ix) {      // (no status channel: a NULL handle reads as -1 rows, as hb_index_ntotal)
    if (!ix) { hb_set_error("hb_index_nlabels: NULL index handle"); return -1; }
    return ix->lab.rows();
}

extern "C" int hb_index_set_label_denominator(hb_index_t* ix, int P) {
    if (!ix) return hb_fail("hb_index_set_label_denominator: NULL index handle");
    if (P < 0 || P > 65535) return hb_fail("hb_index_set_label_denominator: the denominator must be in [0, 65535]");
    if (ix->lab.rows() > 0 && P != ix->lab.denominator()) return hb_fail("hb_index_set_label_denominator: the index already holds label rows");
    if (ix->lab.set_denominator_drops(P)) {
        HB_HIP(hipSetDevice(ix->device));
        HB_HIP(hipStreamSynchronize(ix->stream));
    }
    ix->lab.set_denominator(P);
    return 0;
}
extern "C" int hb_index_label_denominator(const hb_index_t* ix, int* P) {
    if (!ix || !P) return hb_fail("hb_index_label_denominator: NULL pointer");
    *P = ix->lab.denominator();
    return 0;
}
extern "C" int hb_index_labels_to_fp32(hb_index_t* ix) {
    if (!ix) return hb_fail("hb_index_labels_to_fp32: NULL index handle");
    hb_label_store& lab = ix->lab;
    if (!lab.counts()) return 0;
    HB_HIP(hipSetDevice(ix->device));
    if (hb_labels_checked(ix)) return -1;
    hb_dev<float> nl;
    const int64_t cap = lab.fp32_capacity();
    if (lab.rows() > 0) {
        if (nl.ensure((size_t)cap * lab.classes() * 4, HB_GROW_EXACT)) return -1;
        // one pass: count j of the value j / P -> (float)j / (float)P, the fp32 value K2 produced (hbird_eval.py:319-320)
        if (hb_launch_gather_label_counts(lab.own_base<const uint16_t>(), lab.rows(), lab.classes(), lab.stride(), lab.denominator(), nullptr, lab.rows(), nl, ix->stream)) return -1;
    }
    HB_HIP(hipStreamSynchronize(ix->stream));
    lab.replace_with_fp32(std::move(nl), cap);
    return 0;
}

// one read-back (a stream synchronisation) after the label table grew: was every stored value a multiple of 1 / P?
int hb_labels_checked(hb_index* ix) {
    if (!ix->lab.unchecked()) return 0;
    int bad = 0;
    HB_HIP(hipMemcpyAsync(&bad, ix->lab.flag, 4, hipMemcpyDeviceToHost, ix->stream));
    HB_HIP(hipStreamSynchronize(ix->stream));
    if (bad) return hb_fail("label rows are not multiples of 1 / " + std::to_string(ix->lab.denominator()) +
                            " (hb_index_set_label_denominator): store them as fp32 (denominator 0) instead");
    ix->lab.checked();
    return 0;
}

int hb_labels_ensure(hb_index* ix, int c, int64_t n) {
    if (ix->lab.ensure_drops(c)) HB_HIP(hipStreamSynchronize(ix->stream));
    return ix->lab.ensure(c, n, ix->cap_rows, ix->stream) ? -1 : 0;
}

extern "C" int hb_index_add_labels(hb_index_t* ix, const float* labels, int64_t n, int c, int on_device) {
    if (!ix) return hb_fail("hb_index_add_labels: NULL index handle");
    if (n < 0 || c <= 0) return hb_fail("hb_index_add_labels: bad shape");
    if (n == 0) return 0;
    HB_HIP(hipSetDevice(ix->device));
    hb_label_store& lab = ix->lab;
    if (lab.classes() != 0 && lab.classes() != c && lab.rows() > 0) return hb_fail("hb_index_add_labels: class count changed");
    if (hb_labels_ensure(ix, c, n)) return -1;
    if (lab.counts()) {
        // values j / P (what K2 produces, hbird_eval.py:319-320) stored as the uint16 count j: half the table, the same fp32 value back
        if (!lab.flag) { if (lab.flag.ensure(4, HB_GROW_EXACT)) return -1; HB_HIP(hipMemsetAsync(lab.flag, 0, 4, ix->stream)); }
        const float* src = labels;
        if (!on_device) {
            if (ix->tmp.ensure((size_t)n * c * 4, HB_GROW_EXACT)) return -1;
            HB_HIP(hipMemcpyAsync(ix->tmp, labels, (size_t)n * c * 4, hipMemcpyHostToDevice, ix->stream));
            src = ix->tmp.as<const float>();
        }
        if (hb_launch_labels_to_counts(src, n, c, lab.stride(), lab.denominator(), lab.own_tail<uint16_t>(), lab.flag, ix->stream)) return -1;
    } else {
        HB_HIP(hipMemcpyAsync(lab.own_tail<float>(), labels, (size_t)n * c * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ix->stream));
    }
    if (!on_device) HB_HIP(hipStreamSynchronize(ix->stream));
    lab.appended(n, true);
    return 0;
}

extern "C" int hb_index_gather_labels(hb_index_t* ix, const int64_t* ids, int64_t n, int64_t id_base, float* out, int io_on_device) {
    if (!ix) return hb_fail("hb_index_gather_labels: NULL index handle");
    if (n < 0) return hb_fail("hb_index_gather_labels: n is negative");
    if (n == 0) return 0;
    if (!ids || !out) return hb_fail("hb_index_gather_labels: ids / out is NULL");
    HB_HIP(hipSetDevice(ix->device));
    const hb_label_store& lab = ix->lab;
    const int width = lab.classes();
    if (!lab.allocated()) return hb_fail("hb_index_gather_labels: no labels stored");
    if (hb_labels_checked(ix)) return -1;
    const int64_t* d_ids = ids;
    float* d_out = out;
    if (!io_on_device) {
        const size_t b_ids = al256((size_t)n * 8);
        if (ix->tmp.ensure(b_ids + (size_t)n * width * 4, HB_GROW_EXACT)) return -1;
        HB_HIP(hipMemcpyAsync(ix->tmp, ids, (size_t)n * 8, hipMemcpyHostToDevice, ix->stream));
        d_ids = ix->tmp.as<const int64_t>();
        d_out = ix->tmp.as<float>(b_ids);
    }
    // ids are global, rows local
    if (id_base != 0) return hb_fail("hb_index_gather_labels: id_base != 0 is not supported yet");
    if (lab.counts() ? hb_launch_gather_label_counts(lab.own_base<const uint16_t>(), lab.rows(), width, lab.stride(), lab.denominator(), d_ids, n, d_out, ix->stream)
                     : hb_launch_gather_rows(lab.own_base<const float>(), lab.rows(), width, d_ids, n, d_out, ix->stream)) return -1;
    if (!io_on_device) {
        HB_HIP(hipMemcpyAsync(out, d_out, (size_t)n * width * 4, hipMemcpyDeviceToHost, ix->stream));
        HB_HIP(hipStreamSynchronize(ix->stream));
    }
    return 0;
}

extern "C" int hb_index_set_label_table(hb_index_t* ix, const float* labels, const float* bnorm, int64_t n, int c, int64_t id_base) {
    if (!ix) return hb_fail("hb_index_set_label_table: NULL index handle");
    if (labels && (!bnorm || n <= 0 || c <= 0)) return hb_fail("hb_index_set_label_table: bad arguments");
    if (labels) ix->lab.borrow_f32(labels, bnorm, n, c, id_base);
    else ix->lab.unborrow();
    return 0;
}

extern "C" int hb_index_set_label_count_table(hb_index_t* ix, const uint16_t* counts, const float* bnorm, int64_t n, int c, int P, int64_t id_base) {
    if (!ix) return hb_fail("hb_index_set_label_count_table: NULL index handle");
    if (counts && (!bnorm || n <= 0 || c <= 0 || P <= 0 || P > 65535)) return hb_fail("hb_index_set_label_count_table: bad arguments");
    if (counts) ix->lab.borrow_counts(counts, bnorm, n, c, P, id_base);
    else ix->lab.unborrow();
    return 0;
}

extern "C" int hb_index_copy_label_counts(hb_index_t* ix, uint16_t* out, int on_device) {
    if (!ix) return hb_fail("hb_index_copy_label_counts: NULL index handle");
    const hb_label_store& lab = ix->lab;
    if (!lab.counts()) return hb_fail("hb_index_copy_label_counts: the labels are stored as fp32 (hb_index_set_label_denominator)");
    if (lab.rows() == 0) return 0;
    HB_HIP(hipSetDevice(ix->device));
    if (hb_labels_checked(ix)) return -1;
    // (the stored rows are padded to 16 bytes; the caller gets dense [rows, C] rows)
    HB_HIP(hipMemcpy2DAsync(out, (size_t)lab.classes() * 2, lab.own_base<const uint16_t>(), lab.row_bytes(), (size_t)lab.classes() * 2, (size_t)lab.rows(),
                            on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ix->stream));
    if (!on_device) HB_HIP(hipStreamSynchronize(ix->stream));
    return 0;
}
