// hb_devbuf (csrc/hbird_devbuf.h) alone, on the host: the three device functions over malloc / free / memcpy with a switch that makes the n-th
// allocation fail.  Built with ASan + UBSan (make -C csrc devbuf_check), run by tests/test_devbuf_cpu.py; exits non-zero on any mismatch.
#include "hbird_devbuf.h"
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

static void policies() {
    {
        hb_devbuf b;
        CHECK(!b && b.p == nullptr && b.bytes == 0);
        CHECK(b.ensure(1000, HB_GROW_EXACT) == 0 && b.bytes == 1000 && b.p && g_count == 1 && g_bytes == 1000);
        void* const p0 = b.p;
        CHECK(b.ensure(1000, HB_GROW_EXACT) == 0 && b.p == p0 && b.bytes == 1000);      // large enough: a no-op
        CHECK(b.ensure(10, HB_GROW_QUARTER) == 0 && b.p == p0 && b.bytes == 1000 && g_count == 1);
        CHECK(b.ensure(1001, HB_GROW_EXACT) == 0 && b.bytes == 1001 && g_count == 1 && g_bytes == 1001);      // free, then allocate
        CHECK(b.ensure(2002, HB_GROW_QUARTER) == 0 && b.bytes == 2002 + 2002 / 4 && g_count == 1 && g_bytes == 2502);
        CHECK(b.ensure(2502, HB_GROW_QUARTER) == 0 && b.bytes == 2502);      // within the quarter: a no-op
        CHECK(b.try_ensure(3000, HB_GROW_EXACT) == nullptr && b.bytes == 3000);
    }
    scenario_end("policies");
}

static void typed_access() {
    {
        hb_dev<float> f;
        CHECK(f.ensure(64, HB_GROW_EXACT) == 0);
        float* fp = f;
        CHECK(fp == f.p && f.as<char>(8) == static_cast<char*>(f.p) + 8 && f.as<float>(8) == fp + 2);
        std::memset(f.p, 0, 64);
    }
    scenario_end("typed_access");
}

static void keeps_prefix() {
    {
        hb_devbuf b;
        CHECK(b.ensure(256, HB_GROW_QUARTER) == 0 && b.bytes == 320);
        for (int i = 0; i < 320; ++i) b.as<unsigned char>()[i] = (unsigned char)(i * 7 + 1);
        void* const p0 = b.p;
        g_copies = 0;
        CHECK(b.ensure_keep(300, HB_GROW_QUARTER, 100, nullptr) == 0 && b.p == p0 && g_copies == 0);      // large enough: a no-op
        CHECK(b.ensure_keep(4000, HB_GROW_QUARTER, 100, nullptr) == 0 && b.bytes == 5000 && g_copies == 1 && g_count == 1 && g_bytes == 5000);
        bool same = true;
        for (int i = 0; i < 100; ++i) same = same && b.as<unsigned char>()[i] == (unsigned char)(i * 7 + 1);
        CHECK(same);
        CHECK(b.ensure_keep(6000, HB_GROW_EXACT, 0, nullptr) == 0 && b.bytes == 6000 && g_copies == 2);      // nothing to keep: still waits for the stream
        // a growth that fails leaves the buffer as it was
        std::memset(b.p, 0x5A, 6000);
        void* const p1 = b.p;
        g_fail_in = 1;
        CHECK(b.ensure_keep(7000, HB_GROW_EXACT, 6000, nullptr) == -1 && b.p == p1 && b.bytes == 6000 && !g_err.empty() && g_count == 1);
        CHECK(b.as<unsigned char>()[5999] == 0x5A);
        hb_devbuf empty;
        CHECK(empty.ensure_keep(16, HB_GROW_EXACT, 0, nullptr) == 0 && empty.bytes == 16);      // from nothing
    }
    scenario_end("keeps_prefix");
}

static void failed_ensure() {
    {
        hb_devbuf b;
        CHECK(b.ensure(100, HB_GROW_EXACT) == 0);
        g_fail_in = 1; g_err.clear();
        CHECK(b.ensure(200, HB_GROW_EXACT) == -1 && b.p == nullptr && b.bytes == 0 && !b);
        CHECK(g_err.find("200") != std::string::npos && g_err.find("out of memory") != std::string::npos);
        CHECK(g_count == 0 && g_bytes == 0);
        // the quiet form: the same state, the reason returned, no error text
        CHECK(b.ensure(100, HB_GROW_EXACT) == 0);
        g_fail_in = 1; g_err.clear();
        const char* why = b.try_ensure(200, HB_GROW_QUARTER);
        CHECK(why != nullptr && b.p == nullptr && b.bytes == 0 && g_err.empty() && g_count == 0);
        CHECK(b.ensure(50, HB_GROW_EXACT) == 0 && b.bytes == 50);      // and usable again
    }
    scenario_end("failed_ensure");
}

static void moves_and_drops() {
    {
        hb_devbuf a;
        CHECK(a.ensure(128, HB_GROW_EXACT) == 0);
        void* const pa = a.p;
        hb_devbuf b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == pa && b.bytes == 128 && g_count == 1);      // a moved-from buffer is empty
        hb_devbuf c;
        CHECK(c.ensure(64, HB_GROW_EXACT) == 0 && g_count == 2);
        c = std::move(b);      // the target's own allocation goes
        CHECK(b.p == nullptr && b.bytes == 0 && c.p == pa && c.bytes == 128 && g_count == 1 && g_bytes == 128);
        hb_devbuf& self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.bytes == 128 && g_count == 1);
        hb_dev<float> t;
        CHECK(t.ensure(32, HB_GROW_EXACT) == 0);
        hb_dev<float> u;
        u = std::move(t);      // the typed form moves the same way
        CHECK(!t && u.bytes == 32 && g_count == 2);
        c.drop();
        CHECK(c.p == nullptr && c.bytes == 0 && g_count == 1);
        c.drop();      // twice is harmless
        CHECK(c.p == nullptr && c.bytes == 0 && g_count == 1);
        a.drop();
    }
    scenario_end("moves_and_drops");
}

// hb_index_reserve's shape: three locals, moved into their owner only once all are there
struct owner { hb_dev<float> tiles, binit, bnorm; long long cap = 0; };
static int reserve_like(owner& o, long long cap) {
    hb_dev<float> tiles, binit, bnorm;
    if (tiles.ensure((size_t)cap * 64, HB_GROW_EXACT) || binit.ensure((size_t)cap * 4, HB_GROW_EXACT) || bnorm.ensure((size_t)cap * 4, HB_GROW_EXACT)) return -1;
    o.tiles = std::move(tiles); o.binit = std::move(binit); o.bnorm = std::move(bnorm); o.cap = cap;
    return 0;
}
static void three_allocations() {
    {
        owner o;
        CHECK(reserve_like(o, 256) == 0 && g_count == 3 && g_bytes == 256 * 72);
        const long long count0 = g_count, bytes0 = g_bytes;
        void* const t0 = o.tiles.p;
        for (int nth = 1; nth <= 3; ++nth) {
            g_fail_in = nth;
            CHECK(reserve_like(o, 512) == -1);
            CHECK(g_count == count0 && g_bytes == bytes0 && o.tiles.p == t0 && o.cap == 256);      // nothing leaked, the owner as it was
        }
        CHECK(reserve_like(o, 512) == 0 && g_count == 3 && g_bytes == 512 * 72 && o.cap == 512);
    }
    scenario_end("three_allocations");
}

int main() {
    CHECK(al256(0) == 0 && al256(1) == 256 && al256(256) == 256 && al256(257) == 512);
    policies();
    typed_access();
    keeps_prefix();
    failed_ensure();
    moves_and_drops();
    three_allocations();
    if (g_bad) { std::fprintf(stderr, "devbuf_check: %d mismatches\n", g_bad); return 1; }
    std::puts("devbuf_check: ok");
    return 0;
}
