// What a finished search of a caller says about itself: which path served it, what the levels of the fp16 screen certified and handed on, and
// which of the buffers they wrote (`cand`, `fb`, `fb1`, `q16`) still hold what the read-outs hand out.  Plain C++, no HIP, in the style of
// hbird_mirror.h -- data, questions, transitions: tests/report_check.cpp drives the type on the host.
// A search writes the report it is handed (knn_call::rep, hbird_knn.hip), never the index's; the caller-level entry commits it when the search
// is over (hb_index::commit), so a nested or detached search leaves no trace in the index.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>
#include "hbird_devbuf.h"

// hb_search_report::state: what the level-0 lists in `cand` are worth
#define HB_SCREEN_NONE 0           // no level-0 fp16 candidate pass in this search (or a later search reused its buffers)
#define HB_SCREEN_VALID 1
#define HB_SCREEN_OVERWRITTEN 2    // a second fp16 pass has reused `cand`
#define HB_SCREEN_BANK_CHANGED 3   // a pass ran, and the bank has changed since (reset, add, capacity)

// the lists' question (hb_index_last_screen)
enum hb_lists_answer { HB_LISTS_READABLE, HB_LISTS_NEVER, HB_LISTS_OVERWRITTEN, HB_LISTS_BANK_CHANGED };

// workspace of one level of the screen: [certificates nq + 64][exact k-th scores nq][floors for a second pass nq], then from o_rows on what the
// re-search of its failures gathers -- a caller's pass keeps it in fb, the second fp16 pass in fb1
struct hb_level_layout {
    size_t o_kth, o_flo, o_rows;
    explicit hb_level_layout(int64_t nq) : o_kth(al256((size_t)nq + 64)), o_flo(o_kth + al256((size_t)nq * 4)), o_rows(o_flo + al256((size_t)nq * 4)) {}
};

struct hb_search_report {
    int path = 0, reason = 0;          // HB_PATH_*, HB_WHY_* (hb_last_search_path); of a search with k > 256 its last pass'
    int centred = 0;                   // the candidate pass ran on the centred copy (cleared by a change of the copy's form)
    int64_t fallbacks = 0;             // queries that the fp32 kernel (an excluding search: the rungs) had to answer ...
    int64_t escalated = 0;             // ... and queries whose first certificate failed and that a NESTED search took (0 where an excluding
                                       // search hands its level-0 failures straight to the rungs)
    // the screen: level 0's lists and pass scores in `cand`, its certificates, k-th scores and floors in `fb` (hb_level_layout)
    int state = HB_SCREEN_NONE;
    int64_t nq = 0; int kc = 0, klw = 0, lists_centred = 0;
    int excluding = 0;                 // the search dropped row groups (hb_index_search_excluding): the k-th scores are those of the ALLOWED candidates
    int64_t failed0 = 0;               // level-0 queries whose certificate failed
    // the second fp16 pass: its lists in `cand`, its level workspace in `fb1`
    int64_t n1 = 0; int kc1 = 0, klw1 = 0;
    int64_t failed1 = 0;
    size_t o_seed1 = 0;                // byte offset in `fb` of its gathered seeds [n1]
    size_t o_qg1 = 0;                  // ... and (excluding) of its gathered query groups [n1]
    std::vector<int64_t> bad;          // the level-0 queries sent to it, ascending
    std::vector<int64_t> left;         // (excluding) the level-0 queries handed to the rungs, ascending
    // the last candidate pass that wrote `q16` (a centred one: also the centre's per-query values): its queries, level (-1: none), form
    int64_t q16_n = 0; int q16_level = -1, q16_centred = 0;
    int passes = 0;                    // level-0 candidate passes written into this report since it was made (begin() keeps the count)

    // ---- transitions ----
    // a search of a caller begins, plain or excluding (every pass of a search with k > 256 is one: the last one wins)
    void begin(bool excl) { const int p = passes; *this = hb_search_report(); passes = p; excluding = excl ? 1 : 0; }
    // the path is chosen; fell_back: queries the fp32 kernel answers without a pass having looked at them (adaptive skip, overflow)
    void path_chosen(int path_, int reason_, bool centred_, int64_t fell_back) { path = path_; reason = reason_; centred = centred_ ? 1 : 0; fallbacks = fell_back; escalated = 0; }
    // level 0 finished: `cand` and the certificates are complete
    void level0_finished(int64_t nq_, int kc_, int klw_, bool centred_, int64_t failed) {
        state = HB_SCREEN_VALID; nq = nq_; kc = kc_; klw = klw_; lists_centred = centred_ ? 1 : 0; failed0 = failed;
        fallbacks = 0; escalated = 0; ++passes;
        q16_n = nq_; q16_level = 0; q16_centred = lists_centred;
    }
    // level 0's failures go to a second fp16 pass: from here on the lists in `cand` are no longer level 0's
    void sent_to_second_pass(const std::vector<int64_t>& queries, size_t o_seed, size_t o_qg) {
        state = HB_SCREEN_OVERWRITTEN; bad = queries; o_seed1 = o_seed; o_qg1 = o_qg; escalated = (int64_t)queries.size();
    }
    void level1_finished(int64_t n, int kc_, int klw_, bool centred_, int64_t failed) {
        n1 = n; kc1 = kc_; klw1 = klw_; failed1 = failed;
        q16_n = n; q16_level = 1; q16_centred = centred_ ? 1 : 0;
    }
    // n queries of `level` went on to the fp32 kernel (from level 0: escalation off, k' already 256, fewer than 4,096 rows)
    void reached_fp32(int64_t n, int level) { fallbacks = n; if (level == 0) escalated = n; }
    // (excluding) what the last level could not certify is the rungs' (caller's query numbers, ascending)
    void left_to_rungs(std::vector<int64_t> queries) { left = std::move(queries); fallbacks = (int64_t)left.size(); }
    // a later search reused `cand` / `fb` / `fb1` / `q16` (a leftover's rung that took the candidate pass itself): the counts stay, the buffers are gone
    void buffers_reused() { state = HB_SCREEN_NONE; }
    // the bank changed (rows appended, emptied, a new capacity): whatever the buffers hold spoke of the bank as it was
    void bank_changed() { if (state != HB_SCREEN_NONE) state = HB_SCREEN_BANK_CHANGED; }
    // the fp16 copy changed its form (hb_index_set_fp16_centre): the query side went with the copy; `cand` and `fb` are untouched
    void form_changed() { centred = 0; q16_n = 0; q16_level = -1; q16_centred = 0; }

    // ---- questions ----
    bool took_candidate_pass() const { return passes > 0; }
    bool second_pass_ran() const { return state == HB_SCREEN_OVERWRITTEN; }
    hb_lists_answer lists() const {
        return state == HB_SCREEN_VALID ? HB_LISTS_READABLE : state == HB_SCREEN_OVERWRITTEN ? HB_LISTS_OVERWRITTEN
             : state == HB_SCREEN_BANK_CHANGED ? HB_LISTS_BANK_CHANGED : HB_LISTS_NEVER;
    }
    bool seeds_readable() const { return state == HB_SCREEN_VALID || state == HB_SCREEN_OVERWRITTEN; }
    bool exclusion_seeds_readable() const { return seeds_readable() && excluding; }
    // the query side of the last pass (q16_n queries of level q16_level), for the plain form and for the centred one
    bool plain_queries_readable() const { return seeds_readable() && q16_level >= 0 && !centred && !q16_centred; }
    bool centred_queries_readable() const { return seeds_readable() && q16_level >= 0 && centred && q16_centred; }
    // ---- derived counts (hb_index_last_exclusion_screen, hb_index_last_screen_seeds) ----
    int64_t certified0() const { return nq - failed0; }
    int64_t sent1() const { return (int64_t)bad.size(); }
    int64_t certified1() const { return n1 - failed1; }
    int64_t n_left() const { return (int64_t)left.size(); }
    int64_t n1_read() const { return second_pass_ran() ? n1 : 0; }      // queries of the second pass as the read-outs state them
};
