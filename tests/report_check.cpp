// The report of a search (csrc/hbird_report.h: hb_search_report, hb_level_layout) alone, on the host.  The type is taken through the transitions
// in the order the searches make them (csrc/hbird_knn.hip, csrc/hbird_exclude.hip) -- an fp32 search, screened searches with and without a second
// pass and an fp32 tail, escalation off, served excluding searches, reused buffers, the bank's three events, a change of the copy's form, a
// failed search, no search at all, the passes of a search with k > 256 -- and after EVERY step every question and every derived count is held
// against what the step must leave.  Built with ASan + UBSan (make -C csrc report_check), run by tests/test_report_cpu.py; exits non-zero on any
// mismatch.
#include "hbird_report.h"
#include <cstdio>
#include <utility>

static int g_bad = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

// the path and reason codes of include/hbird_hip.h that the scenarios use (the report only stores them)
enum { FP32 = 0, CHAIN = 1, WIDE = 2 };
enum { WHY_FP32 = 0, WHY_FP16 = 1, WHY_K = 3, WHY_CEILING = 4, WHY_OVERFLOW = 10, WHY_ADAPTIVE = 11 };

// everything a read-out can ask of a report
struct want {
    int path, reason, centred;
    int64_t fallbacks, escalated;
    hb_lists_answer lists;
    bool seeds, excl_seeds, plain_q, centred_q;
    int64_t certified0, sent1, certified1, n_left, n1_read;
    int64_t q16_n; int q16_level;
};
static void holds(const hb_search_report& r, const want& w, int line) {
    const bool ok = r.path == w.path && r.reason == w.reason && r.centred == w.centred && r.fallbacks == w.fallbacks && r.escalated == w.escalated &&
                    r.lists() == w.lists && r.seeds_readable() == w.seeds && r.exclusion_seeds_readable() == w.excl_seeds &&
                    r.plain_queries_readable() == w.plain_q && r.centred_queries_readable() == w.centred_q && r.certified0() == w.certified0 &&
                    r.sent1() == w.sent1 && r.certified1() == w.certified1 && r.n_left() == w.n_left && r.n1_read() == w.n1_read &&
                    r.q16_n == w.q16_n && r.q16_level == w.q16_level && r.second_pass_ran() == (w.lists == HB_LISTS_OVERWRITTEN);
    if (!ok) {
        std::fprintf(stderr, "%s:%d: report {path %d reason %d centred %d fallbacks %lld escalated %lld lists %d seeds %d excl %d plain_q %d centred_q %d "
                             "certified0 %lld sent1 %lld certified1 %lld n_left %lld n1 %lld q16 %lld/%d}\n", __FILE__, line, r.path, r.reason, r.centred,
                     (long long)r.fallbacks, (long long)r.escalated, (int)r.lists(), (int)r.seeds_readable(), (int)r.exclusion_seeds_readable(),
                     (int)r.plain_queries_readable(), (int)r.centred_queries_readable(), (long long)r.certified0(), (long long)r.sent1(),
                     (long long)r.certified1(), (long long)r.n_left(), (long long)r.n1_read(), (long long)r.q16_n, r.q16_level);
        ++g_bad;
    }
}
#define HOLDS(r, ...) holds(r, want{__VA_ARGS__}, __LINE__)

static const want EMPTY{0, 0, 0, 0, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1};
static std::vector<int64_t> iota_from(int64_t first, int64_t n, int64_t step = 1) {
    std::vector<int64_t> v;
    for (int64_t i = 0; i < n; ++i) v.push_back(first + i * step);
    return v;
}

// nq = 0 never reaches the launcher: no transition at all; a failed search commits the same empty report
static void no_search_and_failed_search() {
    hb_search_report r;
    holds(r, EMPTY, __LINE__);
    CHECK(!r.took_candidate_pass() && r.state == HB_SCREEN_NONE && r.bad.empty() && r.left.empty() && r.excluding == 0);
    // a search that failed half way: what the entry commits is a report of its own making, not the one the search had reached
    hb_search_report half;
    half.begin(false); half.path_chosen(CHAIN, WHY_FP16, false, 0); half.level0_finished(700, 64, 128, false, 90);
    half.sent_to_second_pass(iota_from(3, 90), 4096, 0);
    hb_search_report last = half;      // (an earlier search's report in the index)
    const int rc = -1;
    last = rc ? hb_search_report() : std::move(half);      // hb_index::commit
    holds(last, EMPTY, __LINE__);
    CHECK(!last.took_candidate_pass() && last.bad.empty());
    r.bank_changed(); r.form_changed();      // events on an empty report leave it empty
    holds(r, EMPTY, __LINE__);
}

static void fp32_searches() {
    hb_search_report r;
    r.begin(false);
    holds(r, EMPTY, __LINE__);
    r.path_chosen(FP32, WHY_FP32, false, 0);
    HOLDS(r, FP32, WHY_FP32, 0, 0, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    // the adaptive skip and an overflowed copy: every query counts as a fallback though no pass ran
    r.begin(false); r.path_chosen(FP32, WHY_ADAPTIVE, false, 700);
    HOLDS(r, FP32, WHY_ADAPTIVE, 0, 700, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    r.begin(false); r.path_chosen(FP32, WHY_OVERFLOW, false, 700);
    HOLDS(r, FP32, WHY_OVERFLOW, 0, 700, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    r.bank_changed();      // nothing to invalidate: still "never"
    HOLDS(r, FP32, WHY_OVERFLOW, 0, 700, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    CHECK(!r.took_candidate_pass());
}

static void screened_all_certified() {
    hb_search_report r;
    r.begin(false); r.path_chosen(CHAIN, WHY_FP16, false, 0);
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    r.level0_finished(700, 64, 128, false, 0);
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 0, HB_LISTS_READABLE, true, false, true, false, 700, 0, 0, 0, 0, 700, 0);
    CHECK(r.took_candidate_pass() && r.nq == 700 && r.kc == 64 && r.klw == 128 && r.lists_centred == 0 && r.excluding == 0);
    // the same centred: the other query side answers
    hb_search_report c;
    c.begin(false); c.path_chosen(WIDE, WHY_FP16, true, 0); c.level0_finished(700, 256, 256, true, 0);
    HOLDS(c, WIDE, WHY_FP16, 1, 0, 0, HB_LISTS_READABLE, true, false, false, true, 700, 0, 0, 0, 0, 700, 0);
    CHECK(c.lists_centred == 1 && c.q16_centred == 1);
}

static void second_pass_nothing_left() {
    hb_search_report r;
    const std::vector<int64_t> bad = iota_from(5, 90, 7);
    r.begin(false); r.path_chosen(CHAIN, WHY_FP16, false, 0); r.level0_finished(700, 64, 128, false, 90);
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 0, HB_LISTS_READABLE, true, false, true, false, 610, 0, 0, 0, 0, 700, 0);
    r.sent_to_second_pass(bad, 8192, 0);      // here `cand` stops being level 0's
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 90, HB_LISTS_OVERWRITTEN, true, false, true, false, 610, 90, 0, 0, 0, 700, 0);
    CHECK(r.bad == bad && r.o_seed1 == 8192 && r.o_qg1 == 0);
    r.level1_finished(90, 256, 256, false, 0);
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 90, HB_LISTS_OVERWRITTEN, true, false, true, false, 610, 90, 90, 0, 90, 90, 1);
    CHECK(r.n1 == 90 && r.kc1 == 256 && r.klw1 == 256 && r.passes == 1);
}

static void second_pass_then_fp32() {
    hb_search_report r;
    r.begin(false); r.path_chosen(CHAIN, WHY_FP16, true, 0); r.level0_finished(700, 64, 128, true, 100);
    r.sent_to_second_pass(iota_from(0, 100), 8192, 0);
    r.level1_finished(100, 256, 256, true, 40);
    HOLDS(r, CHAIN, WHY_FP16, 1, 0, 100, HB_LISTS_OVERWRITTEN, true, false, false, true, 600, 100, 60, 0, 100, 100, 1);
    r.reached_fp32(40, 1);
    HOLDS(r, CHAIN, WHY_FP16, 1, 40, 100, HB_LISTS_OVERWRITTEN, true, false, false, true, 600, 100, 60, 0, 100, 100, 1);
}

// escalation off (or k' already 256, or fewer than 4,096 rows): level 0's failures go straight to the fp32 kernel, `cand` stays level 0's
static void escalation_off() {
    hb_search_report r;
    r.begin(false); r.path_chosen(CHAIN, WHY_FP16, false, 0); r.level0_finished(700, 64, 128, false, 100);
    r.reached_fp32(100, 0);
    HOLDS(r, CHAIN, WHY_FP16, 0, 100, 100, HB_LISTS_READABLE, true, false, true, false, 600, 0, 0, 0, 0, 700, 0);
}

static void excluding_served() {
    // level 0, second pass, leftovers; the second pass' queries are numbered 0 .. n1 - 1, `left` holds the caller's numbers
    hb_search_report r;
    const std::vector<int64_t> bad = iota_from(2, 50, 4), left = {2, 10, 198};
    r.begin(true);
    CHECK(r.excluding == 1);
    r.path_chosen(CHAIN, WHY_FP16, false, 0); r.level0_finished(240, 64, 128, false, 50);
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 0, HB_LISTS_READABLE, true, true, true, false, 190, 0, 0, 0, 0, 240, 0);
    r.sent_to_second_pass(bad, 8192, 12288);
    r.level1_finished(50, 256, 256, false, 3);
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 50, HB_LISTS_OVERWRITTEN, true, true, true, false, 190, 50, 47, 0, 50, 50, 1);
    r.left_to_rungs(left);
    HOLDS(r, CHAIN, WHY_FP16, 0, 3, 50, HB_LISTS_OVERWRITTEN, true, true, true, false, 190, 50, 47, 3, 50, 50, 1);
    CHECK(r.left == left && r.o_qg1 == 12288);
    // the rungs run detached: a scratch report of their own, which took no candidate pass, and this one is not touched
    hb_search_report rung;
    rung.begin(false); rung.path_chosen(FP32, WHY_K, false, 0);
    rung.begin(false); rung.path_chosen(FP32, WHY_K, false, 0);
    CHECK(!rung.took_candidate_pass());
    HOLDS(r, CHAIN, WHY_FP16, 0, 3, 50, HB_LISTS_OVERWRITTEN, true, true, true, false, 190, 50, 47, 3, 50, 50, 1);
    // ... the hand-over straight to the rungs (escalation off): nothing nested ran, escalated stays 0, the lists stay level 0's
    hb_search_report s;
    s.begin(true); s.path_chosen(CHAIN, WHY_FP16, true, 0); s.level0_finished(240, 64, 128, true, 50);
    s.left_to_rungs(bad);
    HOLDS(s, CHAIN, WHY_FP16, 1, 50, 0, HB_LISTS_READABLE, true, true, false, true, 190, 0, 0, 50, 0, 240, 0);
    // ... and a rung that took the candidate pass itself: the counts stay for hb_index_last_exclusion_screen, every read-out refuses
    rung.begin(false); rung.path_chosen(CHAIN, WHY_FP16, false, 0); rung.level0_finished(3, 256, 256, false, 0);
    rung.begin(false); rung.path_chosen(FP32, WHY_K, false, 0);      // (a later rung: the count of passes survives its begin)
    CHECK(rung.took_candidate_pass());
    r.buffers_reused();
    HOLDS(r, CHAIN, WHY_FP16, 0, 3, 50, HB_LISTS_NEVER, false, false, false, false, 190, 50, 47, 3, 0, 50, 1);
}

static void bank_events_and_form() {
    // appended, emptied, moved: one transition, from each of the two readable states
    for (int event = 0; event < 3; ++event)
        for (int second = 0; second < 2; ++second) {
            hb_search_report r;
            r.begin(second != 0); r.path_chosen(CHAIN, WHY_FP16, false, 0); r.level0_finished(700, 64, 128, false, second ? 9 : 0);
            if (second) { r.sent_to_second_pass(iota_from(0, 9), 8192, 12288); r.level1_finished(9, 256, 256, false, 0); }
            r.bank_changed();
            HOLDS(r, CHAIN, WHY_FP16, 0, 0, second ? 9 : 0, HB_LISTS_BANK_CHANGED, false, false, false, false, second ? 691 : 700, second ? 9 : 0,
                  second ? 9 : 0, 0, 0, second ? 9 : 700, second ? 1 : 0);
            r.bank_changed();      // (twice is the same)
            CHECK(r.lists() == HB_LISTS_BANK_CHANGED && r.state == HB_SCREEN_BANK_CHANGED);
        }
    // the copy's form changes: the query side goes with the copy, lists and seeds lie in buffers the change does not touch
    hb_search_report r;
    r.begin(false); r.path_chosen(CHAIN, WHY_FP16, true, 0); r.level0_finished(700, 64, 128, true, 0);
    r.form_changed();
    HOLDS(r, CHAIN, WHY_FP16, 0, 0, 0, HB_LISTS_READABLE, true, false, false, false, 700, 0, 0, 0, 0, 0, -1);
    CHECK(r.lists_centred == 1);      // (what hb_index_last_screen's info says of the lists it still hands out)
    hb_search_report p;
    p.begin(false); p.path_chosen(CHAIN, WHY_FP16, false, 0); p.level0_finished(700, 64, 128, false, 0);
    p.form_changed();
    HOLDS(p, CHAIN, WHY_FP16, 0, 0, 0, HB_LISTS_READABLE, true, false, false, false, 700, 0, 0, 0, 0, 0, -1);
}

// k > 256: every pass begins anew on the same report, the last one wins; a first pass that took the candidate pass is still counted
static void bigk_passes() {
    hb_search_report r;
    r.begin(false); r.path_chosen(FP32, WHY_K, false, 0);
    r.begin(false); r.path_chosen(FP32, WHY_CEILING, false, 0);
    r.begin(false); r.path_chosen(FP32, WHY_CEILING, false, 0);
    HOLDS(r, FP32, WHY_CEILING, 0, 0, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    CHECK(!r.took_candidate_pass());
    hb_search_report s;
    s.begin(false); s.path_chosen(CHAIN, WHY_FP16, false, 0); s.level0_finished(700, 256, 256, false, 4); s.reached_fp32(4, 0);
    s.begin(false); s.path_chosen(FP32, WHY_CEILING, false, 0);
    HOLDS(s, FP32, WHY_CEILING, 0, 0, 0, HB_LISTS_NEVER, false, false, false, false, 0, 0, 0, 0, 0, 0, -1);
    CHECK(s.took_candidate_pass() && s.passes == 1);
}

// the level workspace against the literal formulas the searches used to carry (knn_level_buf)
static void level_layout() {
    const int64_t nqs[6] = {0, 1, 63, 64, 65, 700};
    for (int64_t nq : nqs) {
        const size_t o_kth = ((size_t)nq + 64 + 255) / 256 * 256, o_flo = o_kth + ((size_t)nq * 4 + 255) / 256 * 256, o_rows = o_flo + ((size_t)nq * 4 + 255) / 256 * 256;
        const hb_level_layout l(nq);
        CHECK(l.o_kth == o_kth && l.o_flo == o_flo && l.o_rows == o_rows);
        CHECK(l.o_kth >= (size_t)nq + 64 && l.o_kth % 256 == 0 && l.o_flo - l.o_kth >= (size_t)nq * 4 && l.o_rows - l.o_flo >= (size_t)nq * 4);
    }
    CHECK(hb_level_layout(0).o_rows == 256 && hb_level_layout(700).o_kth == 768 && hb_level_layout(700).o_flo == 768 + 2816 && hb_level_layout(700).o_rows == 768 + 2 * 2816);
}

int main() {
    no_search_and_failed_search();
    fp32_searches();
    screened_all_certified();
    second_pass_nothing_left();
    second_pass_then_fp32();
    escalation_off();
    excluding_served();
    bank_events_and_form();
    bigk_passes();
    level_layout();
    if (g_bad) { std::fprintf(stderr, "report_check: %d mismatches\n", g_bad); return 1; }
    std::puts("report_check: ok");
    return 0;
}
