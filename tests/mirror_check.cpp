// The bookkeeping of the bank's lazy copies (csrc/hbird_mirror.h: hb_bank_mirror, hb_fp16_copy, hb_row_copy) alone, on the host: the device
// functions of hbird_devbuf.h over malloc / free with a switch that makes the n-th allocation fail.  The two members are taken through the life
// of a bank -- made, rows converted, appended to, moved to a new capacity, emptied, declined, dropped -- as the searches and
// hb_index::bank_changed take them, and their state is checked after every step.  Built with ASan + UBSan (make -C csrc mirror_check), run by
// tests/test_mirror_cpu.py; exits non-zero on any mismatch.
#include "hbird_mirror.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static long long g_count = 0, g_bytes = 0;
static int g_fail_in = 0;      // > 0: that many allocations from now, one fails
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
    return nullptr;
}
int hb_fail(const std::string& msg) { g_err = msg; return -1; }

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

static void scenario_end(const char* name) {
    if (g_count != 0 || g_bytes != 0) { std::fprintf(stderr, "%s: %lld allocations / %lld bytes still live\n", name, g_count, g_bytes); ++g_bad; }
    g_count = 0; g_bytes = 0; g_fail_in = 0; g_err.clear();
}

static bool pending_is(const hb_bank_mirror& m, int64_t ntotal, int64_t rt0, int64_t n_rt) {
    int64_t a = -1, b = -1;
    m.pending(ntotal, &a, &b);
    return a == rt0 && b == n_rt;
}
static bool mirror_is(const hb_bank_mirror& m, int64_t cap, int64_t rows, int64_t declined) { return m.cap == cap && m.rows == rows && m.declined_cap == declined; }

const size_t ROW16 = 128 * 2;      // bytes of an fp16 row of 128 padded dimensions
const int RS = 64;                 // floats of a row of the row copy

// what a search does to both copies for a bank of (cap, ntotal): the shape of knn_fp16_copy_upkeep / knn_row_copy_upkeep (hbird_knn.hip)
static void search_like(hb_fp16_copy& f, hb_row_copy& r, int64_t cap, int64_t ntotal) {
    if (!f.m.has(cap)) CHECK(f.make(cap, ROW16, false) == 0);
    if (f.m.behind(ntotal)) f.m.converted(ntotal);
    if (r.rows && !r.has(cap, RS)) r.drop();
    if (!r.rows && !r.m.declined_at(cap)) CHECK(r.make(cap, RS));
    if (r.rows && r.m.behind(ntotal)) r.m.converted(ntotal);
}

static void life_of_a_bank() {
    {
        hb_fp16_copy f;
        hb_row_copy r;
        // fresh
        CHECK(mirror_is(f.m, 0, 0, -1) && mirror_is(r.m, 0, 0, -1) && !f.tiles && !r.rows && r.bytes() == 0 && f.overflow == 0);
        CHECK(!f.m.has(256) && !f.m.has(0) && !r.has(256, RS) && !f.m.declined_at(256) && f.centred_rows() == 0 && !f.has_centre_arrays());
        // allocated at capacity 256
        CHECK(f.make(256, ROW16, false) == 0 && r.make(256, RS));
        CHECK(mirror_is(f.m, 256, 0, -1) && mirror_is(r.m, 256, 0, -1) && f.tiles.bytes == 256 * ROW16 && r.rows.bytes == 256 * RS * 4 && r.rs == RS);
        CHECK(f.m.has(256) && !f.m.has(512) && r.has(256, RS) && !r.has(256, RS + 32) && r.bytes() == 256 * RS * 4 && g_count == 2);
        // 100 rows: tiles 0..3 are pending, then converted
        CHECK(f.m.behind(100) && pending_is(f.m, 100, 0, 4) && pending_is(r.m, 100, 0, 4));
        search_like(f, r, 256, 100);
        CHECK(mirror_is(f.m, 256, 100, -1) && mirror_is(r.m, 256, 100, -1) && !f.m.behind(100) && !r.m.behind(100) && g_count == 2);
        // appended to 130: the partly filled tile 3 again, and tile 4
        CHECK(f.m.behind(130) && pending_is(f.m, 130, 3, 2) && pending_is(r.m, 130, 3, 2));
        search_like(f, r, 256, 130);
        CHECK(mirror_is(f.m, 256, 130, -1) && mirror_is(r.m, 256, 130, -1));
        // appended to 256: tiles 4..7
        CHECK(pending_is(f.m, 256, 4, 4));
        search_like(f, r, 256, 256);
        CHECK(mirror_is(f.m, 256, 256, -1) && !f.m.behind(256) && pending_is(f.m, 256, 8, 0));
        // moved to capacity 512 (hb_index_reserve): the copies stay as they are until a search needs them, and are no copy for 512
        void* const t0 = f.tiles.p;
        CHECK(!f.m.has(512) && !r.has(512, RS) && f.tiles.p == t0 && mirror_is(f.m, 256, 256, -1));
        search_like(f, r, 512, 256);      // ... which makes them anew, from tile 0 on
        CHECK(f.m.has(512) && r.has(512, RS) && f.tiles.bytes == 512 * ROW16 && r.bytes() == 512 * RS * 4 && g_count == 2);
        CHECK(mirror_is(f.m, 512, 256, -1) && mirror_is(r.m, 512, 256, -1));
        {
            hb_fp16_copy again;
            CHECK(again.make(512, ROW16, false) == 0 && pending_is(again.m, 256, 0, 8) && again.m.rows == 0);
        }
        // emptied (hb_index_reset): no rows, the overflow image cleared, allocations and declined marks kept
        f.overflow = 1; f.m.declined(512);
        f.emptied(); r.m.emptied();
        CHECK(mirror_is(f.m, 512, 0, 512) && mirror_is(r.m, 512, 0, -1) && f.overflow == 0 && f.m.has(512) && f.tiles.bytes == 512 * ROW16 && r.rows && g_count == 2);
        CHECK(pending_is(f.m, 40, 0, 2));
        // declined at 512, then asked again
        f.m.ask_again(); r.m.declined(512);
        CHECK(mirror_is(f.m, 512, 0, -1) && r.m.declined_at(512) && !r.m.declined_at(256) && !f.m.declined_at(512));
        r.m.ask_again();
        CHECK(!r.m.declined_at(512) && mirror_is(r.m, 512, 0, -1));
        // dropped
        search_like(f, r, 512, 40);
        f.drop(); r.drop();
        CHECK(mirror_is(f.m, 0, 0, -1) && mirror_is(r.m, 0, 0, -1) && !f.tiles && !r.rows && r.bytes() == 0 && !f.m.has(512) && g_count == 0 && g_bytes == 0);
        f.drop(); r.drop();      // twice is harmless
        CHECK(g_count == 0);
    }
    scenario_end("life_of_a_bank");
}

// the centred form: its row arrays are sized like the tiles and go with them
static void centre_arrays() {
    {
        hb_fp16_copy f;
        CHECK(f.make(256, ROW16, false) == 0);
        CHECK(f.make_centre_arrays(128) == 0 && f.has_centre_arrays() && g_count == 5);
        CHECK(f.centre.mu.bytes == 128 * 4 && f.centre.g.bytes == 256 * 4 && f.centre.init16.bytes == 256 * 4 && f.centre.sc.bytes == 16);
        f.m.converted(100);
        CHECK(f.centred_rows() == 0);      // (no usable mean: the rows were converted plainly)
        f.centre.active = 1;
        CHECK(f.centred_rows() == 100);
        f.emptied();
        CHECK(f.centred_rows() == 0 && f.has_centre_arrays() && g_count == 5);      // mu is derived anew at rows == 0
        f.m.converted(60);
        // a drop of the tiles takes the row arrays along: converted rows without row arrays cannot be written down
        f.drop();
        CHECK(!f.has_centre_arrays() && !f.centre.g && !f.centre.init16 && f.centred_rows() == 0 && f.m.rows == 0 && g_count == 2);
        // a capacity change: new tiles, then new arrays for the new capacity
        CHECK(f.make(512, ROW16, false) == 0 && !f.has_centre_arrays());
        CHECK(f.make_centre_arrays(128) == 0 && f.centre.g.bytes == 512 * 4 && f.centre.active == 0 && g_count == 5);
        // a change of the form: everything goes
        f.centre.active = 1; f.overflow = 1; f.m.declined(512); f.m.converted(300);
        f.drop_form();
        CHECK(mirror_is(f.m, 0, 0, -1) && f.overflow == 0 && f.centre.active == 0 && !f.centre.mu && g_count == 0);
    }
    scenario_end("centre_arrays");
}

// every one of the four allocations of the centre arrays made to fail: the member as before the call, nothing leaked
static void centre_allocation_fails() {
    {
        hb_fp16_copy f;
        CHECK(f.make(256, ROW16, false) == 0);
        f.m.converted(77);
        for (int round = 0; round < 2; ++round) {      // without arrays, then with the arrays of an earlier call
            const long long count0 = g_count, bytes0 = g_bytes;
            void* const mu0 = f.centre.mu.p; void* const g0 = f.centre.g.p; void* const i0 = f.centre.init16.p; void* const sc0 = f.centre.sc.p;
            const int active0 = f.centre.active;
            for (int nth = 1; nth <= 4; ++nth) {
                g_fail_in = nth; g_err.clear();
                CHECK(f.make_centre_arrays(128) == -1 && !g_err.empty());
                CHECK(g_count == count0 && g_bytes == bytes0);
                CHECK(f.centre.mu.p == mu0 && f.centre.g.p == g0 && f.centre.init16.p == i0 && f.centre.sc.p == sc0 && f.centre.active == active0);
                CHECK(mirror_is(f.m, 256, 77, -1) && f.tiles.bytes == 256 * ROW16);
            }
            CHECK(f.make_centre_arrays(128) == 0 && f.has_centre_arrays() && g_count == 5);
            f.centre.active = 1;
        }
    }
    scenario_end("centre_allocation_fails");
}

// allocations of the copies themselves that fail
static void copy_allocation_fails() {
    {
        hb_row_copy r;
        g_fail_in = 1;
        CHECK(!r.make(256, RS) && !r.rows && mirror_is(r.m, 0, 0, 256) && r.m.declined_at(256) && r.bytes() == 0 && g_err.empty() && g_count == 0);
        CHECK(r.make(256, RS) && mirror_is(r.m, 256, 0, -1) && g_count == 1);      // (set again / a new capacity: asked again, made, the mark cleared)
        hb_fp16_copy f;
        // the automatic state: quiet, and declined at the capacity
        g_fail_in = 1;
        CHECK(f.make(256, ROW16, true) == -1 && !f.tiles && mirror_is(f.m, 0, 0, 256) && g_err.empty());
        // states 1 / 2: the caller's error, nothing marked
        f.m.ask_again();
        g_fail_in = 1;
        CHECK(f.make(256, ROW16, false) == -1 && !f.tiles && mirror_is(f.m, 0, 0, -1) && g_err.find("out of memory") != std::string::npos);
        CHECK(f.make(256, ROW16, true) == 0 && mirror_is(f.m, 256, 0, -1) && g_count == 2);
        // a copy that is made again lets the old one go first
        f.m.converted(200);
        g_fail_in = 1;
        CHECK(f.make(512, ROW16, true) == -1 && !f.tiles && mirror_is(f.m, 0, 0, 512) && g_count == 1);
    }
    scenario_end("copy_allocation_fails");
}

int main() {
    life_of_a_bank();
    centre_arrays();
    centre_allocation_fails();
    copy_allocation_fails();
    if (g_bad) { std::fprintf(stderr, "mirror_check: %d mismatches\n", g_bad); return 1; }
    std::puts("mirror_check: ok");
    return 0;
}
