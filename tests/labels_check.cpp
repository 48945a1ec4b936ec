// hb_label_store (csrc/hbird_labels.h) alone, on the host: the three device functions over malloc / free / memcpy with a switch that makes the
// n-th allocation fail, and the store taken through the orders the label entries make (hbird_labels.hip, hbird_select.hip, hb_index_reset),
// every question held after every step.  Built with ASan + UBSan (make -C csrc labels_check), run by tests/test_labels_cpu.py; exits non-zero
// on any mismatch.
#include "hbird_labels.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

static long long g_count = 0, g_bytes = 0;
static int g_fail_in = 0;      // > 0: that many allocations from now, one fails
static int g_copies = 0;
static std::string g_err;
static int g_bad = 0;

const char* hb_dev_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (g_fail_in > 0 && --g_fail_in == 0) return "out of memory (asked for by the test)";
    *p = std::malloc(bytes ? bytes : 1);
    if (!*p) return "malloc failed";
    ++g_count; g_bytes += (long long)bytes;
    return nullptr;
}
void hb_dev_free(void* p, size_t bytes) {
    std::free(p);
    --g_count; g_bytes -= (long long)bytes;
}
const char* hb_dev_copy_sync(void* dst, const void* src, size_t bytes, void*) {
    if (bytes) std::memcpy(dst, src, bytes);
    ++g_copies;
    return nullptr;
}
int hb_fail(const std::string& msg) { g_err = msg; return -1; }

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

// after every scenario nothing is live
static void scenario_end(const char* name) {
    if (g_count != 0 || g_bytes != 0) { std::fprintf(stderr, "%s: %lld allocations / %lld bytes still live\n", name, g_count, g_bytes); ++g_bad; }
    g_count = 0; g_bytes = 0; g_fail_in = 0; g_err.clear();
}

// every question of a store in one line: what the scenario says it must be
struct expect {
    int c, P; int64_t rows, cap, unchecked;
    bool buf32, buf16;
};
static bool is(const hb_label_store& s, const expect& e, int line) {
    const int stride = e.P ? (e.c + 7) / 8 * 8 : e.c;
    const bool alloc = e.buf32 || e.buf16;
    const void* base = e.P ? (const void*)s.rows16.p : (const void*)s.rows32.p;
    const bool ok = s.classes() == e.c && s.denominator() == e.P && s.counts() == (e.P > 0) && s.stride() == stride &&
                    s.row_bytes() == (size_t)stride * (e.P ? 2 : 4) && s.rows() == e.rows && s.capacity() == e.cap && s.unchecked() == e.unchecked &&
                    (bool)s.rows32 == e.buf32 && (bool)s.rows16 == e.buf16 && s.allocated() == alloc && s.own_rows() == (e.rows > 0 && alloc) &&
                    s.own_base<const void>() == base && (const char*)s.own_tail<const void>() == (const char*)base + (size_t)e.rows * stride * (e.P ? 2 : 4) &&
                    (e.cap > 0) == alloc && e.rows <= e.cap &&
                    (!e.buf32 || s.rows32.bytes == (size_t)e.cap * stride * 4) && (!e.buf16 || s.rows16.bytes == (size_t)e.cap * stride * 2);
    if (!ok) { std::fprintf(stderr, "%s:%d: the store is not what the step leaves\n", __FILE__, line); ++g_bad; }
    return ok;
}
#define IS(s, ...) is(s, expect{__VA_ARGS__}, __LINE__)

// what hb_index_add_labels does to the store (the conversion's device flag is made by the first count rows); rows are filled with `fill`
static int add_labels(hb_label_store& s, int c, int64_t n, int64_t bank_cap, unsigned char fill) {
    if (s.ensure(c, n, bank_cap, nullptr)) return -1;
    if (s.counts() && !s.flag && s.flag.ensure(4, HB_GROW_EXACT)) return -1;
    std::memset(s.own_tail<void>(), fill, (size_t)n * s.row_bytes());
    s.appended(n, true);
    return 0;
}

static void stride_table() {
    const int cs[7] = {1, 7, 8, 21, 151, 152, 512};
    const int counts_stride[7] = {8, 8, 8, 24, 152, 152, 512};
    for (int i = 0; i < 7; ++i) {
        hb_label_store s;
        CHECK(s.ensure(cs[i], 0, 0, nullptr) == HB_LABELS_OK);      // (no room asked for: only the class count)
        CHECK(s.stride() == cs[i] && s.row_bytes() == (size_t)cs[i] * 4 && !s.counts());
        CHECK(s.set_denominator(196) == HB_LABELS_OK);
        CHECK(s.stride() == counts_stride[i] && s.row_bytes() == (size_t)counts_stride[i] * 2 && s.counts() && s.row_bytes() % 16 == 0);
        IS(s, cs[i], 196, 0, 0, 0, false, false);
    }
    scenario_end("stride_table");
}

static void growth() {
    for (int P : {0, 196}) {
        hb_label_store s;
        CHECK(s.set_denominator(P) == HB_LABELS_OK);
        const bool u = P > 0;
        // the first rows: the capacity follows the bank's where that is larger
        CHECK(add_labels(s, 21, 10, 64, 0x11) == 0);
        IS(s, 21, P, 10, 64, u ? 10 : 0, !u, u);
        unsigned char* const p0 = s.own_base<unsigned char>();
        for (size_t i = 0; i < 10 * s.row_bytes(); ++i) p0[i] = (unsigned char)(i * 13 + 5);
        g_copies = 0;
        CHECK(add_labels(s, 21, 54, 64, 0x22) == 0 && s.own_base<unsigned char>() == p0 && g_copies == 0);      // within the capacity: no growth
        IS(s, 21, P, 64, 64, u ? 64 : 0, !u, u);
        // x 1.5 where neither the request nor the bank asks for more; the rows move with the buffer
        CHECK(s.ensure(21, 1, 64, nullptr) == HB_LABELS_OK && g_copies == 1);
        IS(s, 21, P, 64, 96, u ? 64 : 0, !u, u);
        bool same = true;
        for (size_t i = 0; i < 10 * s.row_bytes(); ++i) same = same && s.own_base<unsigned char>()[i] == (unsigned char)(i * 13 + 5);
        for (size_t i = 10 * s.row_bytes(); i < 64 * s.row_bytes(); ++i) same = same && s.own_base<unsigned char>()[i] == 0x22;
        CHECK(same);
        // the request itself where it is the largest, then the bank's capacity again
        CHECK(s.ensure(21, 200, 64, nullptr) == HB_LABELS_OK);
        IS(s, 21, P, 64, 264, u ? 64 : 0, !u, u);
        CHECK(s.ensure(21, 201, 1024, nullptr) == HB_LABELS_OK);
        IS(s, 21, P, 64, 1024, u ? 64 : 0, !u, u);
        // a failing growth leaves the store as it was, contents included
        unsigned char* const p1 = s.own_base<unsigned char>();
        g_fail_in = 1;
        CHECK(s.ensure(21, 5000, 1024, nullptr) == HB_LABELS_FAILED && !g_err.empty() && s.own_base<unsigned char>() == p1 && p1[0] == 5);
        IS(s, 21, P, 64, 1024, u ? 64 : 0, !u, u);
        // ... and so does a failing first allocation, but for the class count (what restore() is for)
        hb_label_store e;
        CHECK(e.set_denominator(P) == HB_LABELS_OK);
        g_fail_in = 1;
        CHECK(e.ensure(21, 10, 64, nullptr) == HB_LABELS_FAILED);
        IS(e, 21, P, 0, 0, 0, false, false);
        CHECK(e.ensure(21, 10, 64, nullptr) == HB_LABELS_OK);
        IS(e, 21, P, 0, 64, 0, !u, u);
    }
    scenario_end("growth");
}

// hb_index_reset keeps allocations; rows of the other form may follow it
static void reset_then_form_change() {
    {
        hb_label_store s;      // fp32 -> counts
        CHECK(add_labels(s, 21, 100, 128, 1) == 0);
        IS(s, 21, 0, 100, 128, 0, true, false);
        CHECK(s.emptied() == nullptr);      // (no flag yet: nothing for the caller to clear)
        IS(s, 21, 0, 0, 128, 0, true, false);
        CHECK(s.set_denominator_drops(196) && !s.set_denominator_drops(0));
        CHECK(s.set_denominator(196) == HB_LABELS_OK);
        IS(s, 21, 196, 0, 0, 0, false, false);
        CHECK(g_count == 0);
        CHECK(add_labels(s, 21, 300, 0, 2) == 0);      // more rows than the old capacity: they land in a buffer of their own form
        IS(s, 21, 196, 300, 300, 300, false, true);
        CHECK(g_count == 2);      // the rows and the flag
    }
    {
        hb_label_store s;      // counts -> fp32
        CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 21, 100, 128, 1) == 0);
        IS(s, 21, 196, 100, 128, 100, false, true);
        s.checked();
        IS(s, 21, 196, 100, 128, 0, false, true);
        CHECK(s.emptied() == (int*)s.flag.p && s.flag);      // the flag stays allocated, and the caller is told to clear it
        IS(s, 21, 196, 0, 128, 0, false, true);
        CHECK(!s.set_denominator_drops(98));
        CHECK(s.set_denominator(98) == HB_LABELS_OK);      // another denominator, the same form: the buffer stays
        IS(s, 21, 98, 0, 128, 0, false, true);
        CHECK(s.set_denominator_drops(0) && s.set_denominator(0) == HB_LABELS_OK);
        IS(s, 21, 0, 0, 0, 0, false, false);
        CHECK(add_labels(s, 21, 300, 0, 2) == 0);
        IS(s, 21, 0, 300, 300, 0, true, false);
    }
    scenario_end("reset_then_form_change");
}

// ... and rows of another width: the capacity counts rows of the OLD width
static void reset_then_wider_rows() {
    for (int P : {0, 196}) {
        hb_label_store s;
        const bool u = P > 0;
        CHECK(s.set_denominator(P) == HB_LABELS_OK && add_labels(s, 21, 100, 128, 1) == 0);
        s.checked(); s.emptied();
        IS(s, 21, P, 0, 128, 0, !u, u);
        CHECK(!s.ensure_drops(21) && s.ensure_drops(151));
        CHECK(add_labels(s, 151, 100, 0, 3) == 0);      // 100 <= 128 rows would "fit"; the buffer of 21-class rows goes all the same
        IS(s, 151, P, 100, 100, u ? 100 : 0, !u, u);
        CHECK(s.own_tail<unsigned char>()[-1] == 3);      // (ASan: the last byte of the 100th row is inside the buffer)
        s.drop();      // drop() alone: the buffers and the capacity, nothing else
        CHECK(!s.allocated() && !s.rows32 && !s.rows16 && s.capacity() == 0 && s.rows() == 100 && s.classes() == 151 && s.denominator() == P);
    }
    scenario_end("reset_then_wider_rows");
}

static void denominator_refusal() {
    hb_label_store s;
    CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 8, 4, 0, 1) == 0);
    CHECK(s.set_denominator(0) == HB_LABELS_HOLD_ROWS && s.set_denominator(98) == HB_LABELS_HOLD_ROWS);
    IS(s, 8, 196, 4, 4, 4, false, true);
    CHECK(s.set_denominator(196) == HB_LABELS_OK);      // the same one: accepted
    IS(s, 8, 196, 4, 4, 4, false, true);
    hb_label_store f;
    CHECK(add_labels(f, 8, 4, 0, 1) == 0);
    CHECK(f.set_denominator(196) == HB_LABELS_HOLD_ROWS && f.set_denominator(0) == HB_LABELS_OK);
    IS(f, 8, 0, 4, 4, 0, true, false);
    s.drop(); s.flag.drop(); f.drop();
    scenario_end("denominator_refusal");
}

static void appended_and_checked() {
    {
        hb_label_store s;
        CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 8, 10, 0, 1) == 0);
        IS(s, 8, 196, 10, 10, 10, false, true);
        CHECK(add_labels(s, 8, 5, 0, 1) == 0);      // converted rows never count as checked
        IS(s, 8, 196, 15, 15, 15, false, true);
        s.checked();
        IS(s, 8, 196, 15, 15, 0, false, true);
        // copied rows (hb_index_add_from): a table that was caught up still is ...
        CHECK(s.ensure(8, 5, 0, nullptr) == HB_LABELS_OK);
        s.appended(5, false);
        IS(s, 8, 196, 20, 22, 0, false, true);
        // ... one that was behind stays behind by what it was
        CHECK(add_labels(s, 8, 1, 0, 1) == 0);
        IS(s, 8, 196, 21, 22, 1, false, true);
        s.appended(1, false);
        IS(s, 8, 196, 22, 22, 2, false, true);
        s.checked();
        IS(s, 8, 196, 22, 22, 0, false, true);
    }
    {
        hb_label_store s;      // copied count rows on a store that never converted: no flag, nothing to read back
        CHECK(s.set_denominator(196) == HB_LABELS_OK && s.ensure(8, 4, 0, nullptr) == HB_LABELS_OK);
        s.appended(4, false);
        IS(s, 8, 196, 4, 4, 0, false, true);
        CHECK(!s.flag);
    }
    scenario_end("appended_and_checked");
}

static void to_fp32() {
    {
        hb_label_store s;      // with rows: the new buffer has the old capacity
        CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 21, 10, 64, 1) == 0);
        s.checked();
        CHECK(s.fp32_capacity() == 64);
        hb_dev<float> nl;
        CHECK(nl.ensure((size_t)64 * 21 * 4, HB_GROW_EXACT) == 0);
        void* const p = nl.p;
        s.replace_with_fp32(std::move(nl), 64);
        IS(s, 21, 0, 10, 64, 0, true, false);
        CHECK(s.rows32.p == p && !nl && s.flag);
        CHECK(add_labels(s, 21, 54, 64, 2) == 0 && s.rows32.p == p);
        IS(s, 21, 0, 64, 64, 0, true, false);
    }
    {
        hb_label_store s;      // without rows (after a reset): no buffer, no capacity
        CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 21, 10, 64, 1) == 0);
        s.emptied();
        CHECK(s.fp32_capacity() == 64);
        s.replace_with_fp32(hb_dev<float>(), 64);
        IS(s, 21, 0, 0, 0, 0, false, false);
        CHECK(add_labels(s, 21, 100, 0, 2) == 0);
        IS(s, 21, 0, 100, 100, 0, true, false);
    }
    {
        hb_label_store s;      // more rows than capacity cannot be; fp32_capacity still never answers less than the rows
        CHECK(s.set_denominator(7) == HB_LABELS_OK && add_labels(s, 3, 5, 0, 1) == 0 && s.fp32_capacity() == 5);
    }
    scenario_end("to_fp32");
}

// hb_index_add_from into an empty destination: adopt, ensure, and on a failing ensure restore
static void adopt_and_restore() {
    {
        hb_label_store s;      // a new store (hb_index_select_rows): nothing to drop
        CHECK(!s.adopt_drops(151, 196));
        const hb_label_form old = s.adopt(151, 196);
        CHECK(old.c == 0 && old.P == 0);
        IS(s, 151, 196, 0, 0, 0, false, false);
        g_fail_in = 1;
        CHECK(s.ensure(151, 300, 300, nullptr) == HB_LABELS_FAILED);
        s.restore(old);
        IS(s, 0, 0, 0, 0, 0, false, false);      // without buffers: the form it had
    }
    {
        hb_label_store s;      // emptied fp32 rows of 21 classes take count rows of 151: both drops, one question
        CHECK(add_labels(s, 21, 100, 128, 1) == 0);
        s.emptied();
        CHECK(s.adopt_drops(151, 196) && s.adopt_drops(21, 196) && s.adopt_drops(151, 0) && !s.adopt_drops(21, 0));
        const hb_label_form old = s.adopt(151, 196);
        CHECK(old.c == 21 && old.P == 0);
        IS(s, 151, 196, 0, 0, 0, false, false);
        g_fail_in = 1;
        CHECK(s.ensure(151, 300, 300, nullptr) == HB_LABELS_FAILED);
        s.restore(old);
        IS(s, 21, 0, 0, 0, 0, false, false);      // the old buffer is gone, the old form is back
        const hb_label_form again = s.adopt(151, 196);
        CHECK(again.c == 21 && again.P == 0 && s.ensure(151, 300, 300, nullptr) == HB_LABELS_OK);
        s.appended(300, false);
        IS(s, 151, 196, 300, 300, 0, false, true);
    }
    {
        hb_label_store s;      // the same form and width, another denominator: the buffer stays, so a failing growth restores nothing
        CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 21, 100, 128, 1) == 0);
        s.checked(); s.emptied();
        CHECK(!s.adopt_drops(21, 98));
        const hb_label_form old = s.adopt(21, 98);
        CHECK(old.c == 21 && old.P == 196);
        g_fail_in = 1;
        CHECK(s.ensure(21, 500, 0, nullptr) == HB_LABELS_FAILED);
        s.restore(old);
        IS(s, 21, 98, 0, 128, 0, false, true);
    }
    scenario_end("adopt_and_restore");
}

static void truth_table() {
    static float t32[4]; static uint16_t t16[4]; static float nrm[4];
    const int64_t ntotal = 10;
    for (int own = 0; own < 3; ++own) {          // none, short, covering
        for (int bor = 0; bor < 3; ++bor) {      // none, fp32, counts
            hb_label_store s;
            if (own) CHECK(add_labels(s, 4, own == 1 ? 6 : 10, 0, 1) == 0);
            if (bor == 1) s.borrow_f32(t32, nrm, 1, 4, 0);
            if (bor == 2) s.borrow_counts(t16, nrm, 1, 4, 9, 0);
            CHECK(s.borrowed() == (bor != 0));
            CHECK(s.own_rows() == (own != 0));
            CHECK(s.covers(ntotal) == (own == 2));
            CHECK(s.missing(ntotal) == (bor == 0 && own != 2));
            CHECK(s.covers(0) == (own != 0) && s.missing(0) == (bor == 0 && own == 0));      // an empty bank: a buffer covers it, no buffer does not
            s.unborrow();
            CHECK(!s.borrowed() && s.missing(ntotal) == (own != 2) && s.classes() == (own || bor ? 4 : 0));
        }
    }
    {
        hb_label_store s;      // an emptied store keeps its buffer and covers an empty bank only
        CHECK(add_labels(s, 4, 10, 0, 1) == 0);
        s.emptied();
        CHECK(s.allocated() && !s.own_rows() && s.covers(0) && !s.covers(1) && s.missing(1) && !s.missing(0));
    }
    scenario_end("truth_table");
}

static bool same_table(const hb_k5_table& t, const void* labels, bool u16, int P, int ls, int64_t nlabels, const float* bnorm, int64_t norm_base, int64_t nnorm,
                       int64_t id_base) {
    return t.labels == labels && t.u16 == u16 && t.P == P && t.ls == ls && t.nlabels == nlabels && t.bnorm == bnorm && t.norm_base == norm_base && t.nnorm == nnorm &&
           t.id_base == id_base && t.wide == 0;
}

static void views() {
    static float bnorm[1], norms_all[1], ext_norm[1], ext32[1]; static uint16_t ext16[1];
    hb_k5_table t;
    {
        hb_label_store s;      // own fp32 rows
        std::memset(&t, 0xEE, sizeof t);
        CHECK(s.view(0, 0, bnorm, nullptr, 0, &t) == HB_LABELS_ROWS_MISSING);      // nothing at all, not even for an empty bank
        CHECK(add_labels(s, 151, 300, 0, 1) == 0);
        CHECK(s.view(1000, 300, bnorm, nullptr, 0, &t) == HB_LABELS_OK);
        CHECK(same_table(t, s.rows32.p, false, 0, 151, 300, bnorm, 1000, 300, 1000));
        CHECK(s.view(1000, 301, bnorm, nullptr, 0, &t) == HB_LABELS_ROWS_MISSING);
        CHECK(add_labels(s, 151, 20, 0, 1) == 0);      // more label rows than bank rows: the table is as long as the labels
        CHECK(s.view(0, 300, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, s.rows32.p, false, 0, 151, 320, bnorm, 0, 320, 0));
        // label-sharded: everybody's norms from 0 on, the own rows of the bank's rows
        CHECK(s.view(600, 300, bnorm, norms_all, 900, &t) == HB_LABELS_OK && same_table(t, s.rows32.p, false, 0, 151, 300, norms_all, 0, 900, 600));
        CHECK(s.view(600, 321, bnorm, norms_all, 900, &t) == HB_LABELS_ROWS_MISSING);
        // borrowed fp32 (P = 0), dense, covering its own id range; the own rows are not asked
        s.borrow_f32(ext32, ext_norm, 900, 151, 5000);
        CHECK(s.view(600, 1000000, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, ext32, false, 0, 151, 900, ext_norm, 5000, 900, 5000));
        // borrowed counts: the dense stride 151, not the padded 152
        s.borrow_counts(ext16, ext_norm, 900, 151, 196, 5000);
        CHECK(s.view(600, 1000000, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, ext16, true, 196, 151, 900, ext_norm, 5000, 900, 5000));
        // the label-sharded form reads the own rows whatever is borrowed
        CHECK(s.view(600, 300, bnorm, norms_all, 900, &t) == HB_LABELS_OK && same_table(t, s.rows32.p, false, 0, 151, 300, norms_all, 0, 900, 600));
        s.unborrow();
        CHECK(s.view(7, 320, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, s.rows32.p, false, 0, 151, 320, bnorm, 7, 320, 7));
    }
    {
        hb_label_store s;      // own counts: the padded stride
        CHECK(s.set_denominator(196) == HB_LABELS_OK && add_labels(s, 151, 300, 0, 1) == 0);
        CHECK(s.view(64, 300, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, s.rows16.p, true, 196, 152, 300, bnorm, 64, 300, 64));
        CHECK(s.view(64, 300, bnorm, norms_all, 900, &t) == HB_LABELS_OK && same_table(t, s.rows16.p, true, 196, 152, 300, norms_all, 0, 900, 64));
        // a borrowed fp32 table on an index of counts: P = 0 goes to the kernel
        s.borrow_f32(ext32, ext_norm, 900, 151, 0);
        CHECK(s.view(64, 300, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, ext32, false, 0, 151, 900, ext_norm, 0, 900, 0));
    }
    {
        hb_label_store s;      // a borrowed table alone, and the class count it sets
        s.borrow_counts(ext16, ext_norm, 50, 21, 64, 100);
        CHECK(s.classes() == 21 && s.view(0, 10, bnorm, nullptr, 0, &t) == HB_LABELS_OK && same_table(t, ext16, true, 64, 21, 50, ext_norm, 100, 50, 100));
        CHECK(s.view(0, 10, bnorm, norms_all, 30, &t) == HB_LABELS_ROWS_MISSING);
        s.unborrow();
        CHECK(s.classes() == 21 && s.view(0, 10, bnorm, nullptr, 0, &t) == HB_LABELS_ROWS_MISSING);
    }
    scenario_end("views");
}

// the order of a whole life, failing allocations at every ensure: the store is as it was each time, and the next attempt succeeds
static void failing_allocations() {
    for (int P : {0, 196}) {
        hb_label_store s;
        const bool u = P > 0;
        CHECK(s.set_denominator(P) == HB_LABELS_OK);
        int64_t rows = 0, cap = 0;
        const int64_t steps[4] = {10, 30, 100, 1000};
        for (int64_t n : steps) {
            g_fail_in = 1;
            CHECK(s.ensure(21, n, 0, nullptr) == HB_LABELS_FAILED);
            IS(s, 21, P, rows, cap, 0, cap > 0 && !u, cap > 0 && u);
            CHECK(s.ensure(21, n, 0, nullptr) == HB_LABELS_OK);
            cap = rows + n > cap + cap / 2 ? rows + n : cap + cap / 2;
            s.appended(n, false);
            rows += n;
            IS(s, 21, P, rows, cap, 0, !u, u);
        }
        CHECK(rows == 1140 && cap == 1140);
    }
    scenario_end("failing_allocations");
}

int main() {
    stride_table();
    growth();
    reset_then_form_change();
    reset_then_wider_rows();
    denominator_refusal();
    appended_and_checked();
    to_fp32();
    adopt_and_restore();
    truth_table();
    views();
    failing_allocations();
    if (g_bad) { std::fprintf(stderr, "labels_check: %d mismatches\n", g_bad); return 1; }
    std::puts("labels_check: ok");
    return 0;
}
