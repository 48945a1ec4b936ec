// The read-outs of what the fp16 screen's passes left behind (include/hbird_hip_screen.h, include/hbird_hip_exclude_screen.h): host bookkeeping
// and copies, no launch.  Whether a buffer still holds what its read-out hands out is the question of the last search's report (hbird_report.h),
// asked here and nowhere re-derived; where the levels' values lie in `fb` / `fb1` is hb_level_layout, which the searches carve by as well.
// Level 0 leaves its lists and pass scores in `cand`, its certificates, k-th scores and floors in `fb`; a second pass its gathered seeds (and, of an
// excluding search, query groups) further back in `fb`, its lists in `cand` and its own level workspace in `fb1`; the fp32 search of what is left
// takes `state` and the tail of `fb1` only.  An excluding search the screen served leaves the same (its k-th scores over the allowed candidates),
// and the leftover's rungs run detached from the report (hb_index_search_excluding), so all of it answers behind them too.
// (hb_index_last_centre reads the centre's own arrays: hbird_f16_centre.hip, with its query-side condition from the same report.)
#include "../../include/hbird_hip.h"
#include "hbird_internal.h"
#include <algorithm>

namespace {
// The shape the read-outs share once the report has let them through: the device set and the stream synchronised, each capacity held against the
// count it stands for, the copies to the host pointers that were given.
struct readout {
    hb_index* ix;
    const char* who;
    int sync() const {
        HB_HIP(hipSetDevice(ix->device));
        HB_HIP(hipStreamSynchronize(ix->stream));
        return 0;
    }
    int room(int64_t capacity, int64_t n, const char* what, const char* had) const {
        if (capacity >= n) return 0;
        return hb_fail(std::string(who) + ": room for " + std::to_string(capacity) + " " + what + ", " + had + " " + std::to_string(n));
    }
    template <class T> int copy(T* dst, const void* src, size_t n) const {
        if (dst && n) HB_HIP(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
        return 0;
    }
};
}

// The merged lists and pass scores of level 0 in `cand`, the first certificates at the start of `fb`.
extern "C" int hb_index_last_screen(hb_index_t* ix, int64_t* cand_rows, float* pass_scores, unsigned char* certified, int64_t capacity_queries, int64_t info[4]) {
    if (!ix) return hb_fail("hb_index_last_screen: NULL index handle");
    if (!info) return hb_fail("hb_index_last_screen: info is NULL");
    info[0] = info[1] = info[2] = info[3] = 0;
    const readout ro{ix, "hb_index_last_screen"};
    const hb_search_report& r = ix->last;
    const hb_lists_answer lists = r.lists();
    if (lists == HB_LISTS_OVERWRITTEN)
        return hb_fail("hb_index_last_screen: the second fp16 pass of the last search has overwritten the first pass's candidates (hb_index_set_fp16_escalation(ix, 1) keeps them)");
    if (lists != HB_LISTS_READABLE || !ix->cand || !ix->fb)      // (never, or the bank has changed: one message)
        return hb_fail("hb_index_last_screen: the last search did not take the fp16 candidate pass (or the bank has changed since: reset, add, capacity)");
    info[0] = r.nq; info[1] = r.kc; info[2] = r.lists_centred; info[3] = r.klw;
    if (ro.sync()) return -1;
    if (!cand_rows && !pass_scores && !certified) return 0;
    if (ro.room(capacity_queries, r.nq, "queries", "the last search had")) return -1;
    const size_t n = (size_t)r.nq * r.kc;
    if (ro.copy(cand_rows, ix->cand, n) || ro.copy(pass_scores, ix->cand + n * 8, n) || ro.copy(certified, ix->fb, (size_t)r.nq)) return -1;
    return 0;
}

// What the chain behind the first candidate pass left: level 0's seeds, and of a second pass its size, its queries, their seeds and its own output.
extern "C" int hb_index_last_screen_seeds(hb_index_t* ix, float* kth0, float* floor0, unsigned char* certified0, int64_t* queries1, float* seed1, int64_t* cand_rows1,
                                          float* pass_scores1, unsigned char* certified1, float* kth1, int64_t capacity_queries, int64_t capacity_queries1, int64_t info[8]) {
    if (!ix) return hb_fail("hb_index_last_screen_seeds: NULL index handle");
    if (!info) return hb_fail("hb_index_last_screen_seeds: info is NULL");
    for (int i = 0; i < 8; ++i) info[i] = 0;
    const readout ro{ix, "hb_index_last_screen_seeds"};
    const hb_search_report& r = ix->last;
    if (!r.seeds_readable() || !ix->fb)
        return hb_fail("hb_index_last_screen_seeds: the last search did not take the fp16 candidate pass (or the bank has changed since: reset, add, capacity)");
    const hb_level_layout l0(r.nq);
    const int64_t n1 = r.n1_read();
    const hb_level_layout l1(n1);
    if (ix->fb.bytes < l0.o_rows) return hb_fail("hb_index_last_screen_seeds: the level-0 workspace is smaller than its record says");
    if (n1 > 0 && ((int64_t)r.bad.size() != n1 || r.kc1 <= 0 || !ix->cand || !ix->fb1 || ix->cand.bytes < (size_t)n1 * r.kc1 * 12 || ix->fb1.bytes < l1.o_rows ||
                   r.o_seed1 < l0.o_rows || ix->fb.bytes < r.o_seed1 + (size_t)n1 * 4))
        return hb_fail("hb_index_last_screen_seeds: the second pass' buffers are smaller than its record says");
    info[0] = r.nq; info[1] = r.kc; info[2] = n1; info[3] = n1 ? r.kc1 : 0; info[4] = n1 ? r.klw1 : 0; info[5] = r.lists_centred; info[6] = r.fallbacks;
    info[7] = r.klw;
    if (ro.sync()) return -1;
    const bool want0 = kth0 || floor0 || certified0, want1 = queries1 || seed1 || cand_rows1 || pass_scores1 || certified1 || kth1;
    if (want0 && ro.room(capacity_queries, r.nq, "queries", "the last search had")) return -1;
    if (want1 && ro.room(capacity_queries1, n1, "queries of the second pass", "it had")) return -1;
    if (ro.copy(kth0, ix->fb + l0.o_kth, (size_t)r.nq) || ro.copy(floor0, ix->fb + l0.o_flo, (size_t)r.nq) || ro.copy(certified0, ix->fb, (size_t)r.nq)) return -1;
    if (n1 == 0) return 0;
    const size_t n = (size_t)n1 * r.kc1;
    if (queries1) std::copy(r.bad.begin(), r.bad.end(), queries1);
    if (ro.copy(seed1, ix->fb + r.o_seed1, (size_t)n1) || ro.copy(cand_rows1, ix->cand, n) || ro.copy(pass_scores1, ix->cand + n * 8, n) ||
        ro.copy(certified1, ix->fb1, (size_t)n1) || ro.copy(kth1, ix->fb1 + l1.o_kth, (size_t)n1)) return -1;
    return 0;
}

// What an excluding search the screen served handed on besides its seeds: the second pass' query groups as gathered into `fb`, and the queries
// left to the rungs.
extern "C" int hb_index_last_exclusion_seeds(hb_index_t* ix, int32_t* groups1, int64_t* left, int64_t capacity_queries1, int64_t capacity_left, int64_t info[2]) {
    if (!ix) return hb_fail("hb_index_last_exclusion_seeds: NULL index handle");
    if (!info) return hb_fail("hb_index_last_exclusion_seeds: info is NULL");
    info[0] = info[1] = 0;
    const readout ro{ix, "hb_index_last_exclusion_seeds"};
    const hb_search_report& r = ix->last;
    if (!r.exclusion_seeds_readable() || !ix->fb)
        return hb_fail("hb_index_last_exclusion_seeds: the last search was not an excluding one served by the fp16 screen (or the bank has changed since: reset, add, capacity)");
    const int64_t n1 = r.n1_read(), n_left = r.n_left();
    if (n1 > 0 && ((int64_t)r.bad.size() != n1 || r.o_qg1 == 0 || ix->fb.bytes < r.o_qg1 + (size_t)n1 * 4))
        return hb_fail("hb_index_last_exclusion_seeds: the second pass' groups lie outside the workspace its record names");
    info[0] = n1; info[1] = n_left;
    if (ro.sync()) return -1;
    if (groups1 && ro.room(capacity_queries1, n1, "queries of the second pass", "it had")) return -1;
    if (left && ro.room(capacity_left, n_left, "queries of the rungs", "they had")) return -1;
    if (ro.copy(groups1, ix->fb + r.o_qg1, (size_t)n1)) return -1;
    if (left) std::copy(r.left.begin(), r.left.end(), left);
    return 0;
}

// The plain fp16 copy, its overflow flag and the query tiles of the last plain pass.
extern "C" int hb_index_last_fp16_copy(hb_index_t* ix, uint16_t* bank16, uint16_t* q16, int64_t info[8]) {
    if (!ix) return hb_fail("hb_index_last_fp16_copy: NULL index handle");
    if (!info) return hb_fail("hb_index_last_fp16_copy: info is NULL");
    for (int i = 0; i < 8; ++i) info[i] = 0;
    info[6] = -1;
    const readout ro{ix, "hb_index_last_fp16_copy"};
    const hb_fp16_copy& copy = ix->copy16;
    if (!copy.tiles || !copy.flag || !copy.m.has(ix->cap_rows))
        return hb_fail("hb_index_last_fp16_copy: no fp16 copy for this bank (no screened search yet, a capacity change since, or an automatic index that dropped it)");
    if (copy.centre.active)
        return hb_fail("hb_index_last_fp16_copy: the fp16 copy is centred (hb_index_last_centre reads that form)");
    const int64_t rows = copy.m.rows, n_g = (rows + 31) / 32 * 32;
    if (n_g > copy.m.cap) return hb_fail("hb_index_last_fp16_copy: the copy holds more rows than it was allocated for");
    const hb_search_report& r = ix->last;
    const bool q_ok = r.plain_queries_readable() && ix->q16 && ix->q16.bytes >= (size_t)((r.q16_n + HB_QT - 1) / HB_QT * HB_QT) * ix->dp16 * 2;
    const int64_t n = q_ok ? r.q16_n : 0, n_qpad = (n + HB_QT - 1) / HB_QT * HB_QT;
    if (ro.sync()) return -1;
    int flag = 0;
    HB_HIP(hipMemcpy(&flag, copy.flag, 4, hipMemcpyDeviceToHost));
    info[0] = rows; info[1] = ix->dp16; info[2] = n_g; info[3] = flag; info[4] = copy.overflow; info[5] = n; info[6] = q_ok ? r.q16_level : -1; info[7] = n_qpad;
    if (q16 && !q_ok)
        return hb_fail("hb_index_last_fp16_copy: the last search of a caller did not run the plain fp16 candidate pass (or the bank has changed since: reset, add, capacity)");
    if (ro.copy(bank16, copy.tiles, (size_t)n_g * ix->dp16) || ro.copy(q16, ix->q16, (size_t)n_qpad * ix->dp16)) return -1;
    return 0;
}
