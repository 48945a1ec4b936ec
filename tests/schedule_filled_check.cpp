// The work-list planner (csrc/hbird_schedule.cpp) with the FILLED clustered dealing, alone on the host under ASan + UBSan: every shape of
// tests/test_schedule_filled_cpu.py is built with both sharing forms, with and without XCD shares, phased and not, filled and -- through the
// slot limit -- refused, and each list is walked the way the kernels and the launcher walk it: every segment's tiles inside the bank, every
// (query tile, bank tile) pair once, slots and their per-tile tables inside their arrays, phase bounds inside the blocks' segments.  Built by
// `make -C csrc schedule_filled_check`, run by tests/test_schedule_filled_asan_cpu.py; exits non-zero on any mismatch or sanitizer report.
#include "hbird_schedule.h"
#include <cstdio>
#include <vector>

static int g_bad = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { if (++g_bad < 20) std::fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_what); } \
    } while (0)
static char g_what[160];

static void walk(const hb_schedule& sc, int nqt, int nbt) {
    CHECK(sc.nqt == nqt && sc.nbt == nbt && (int)sc.wg_off.size() == sc.G + 1 && sc.wg_off[sc.G] == (int)sc.segs.size());
    std::vector<unsigned char> seen((size_t)nqt * nbt, 0);
    std::vector<int> slot_q((size_t)sc.n_slots, -1), slot_blk((size_t)sc.n_slots, -1), slot_last((size_t)sc.n_slots, -1);
    long long pairs = 0;
    for (int b = 0; b < sc.G; ++b) {
        CHECK(sc.wg_off[b] <= sc.wg_off[b + 1]);
        int clock = 0;
        for (int i = sc.wg_off[b]; i < sc.wg_off[b + 1]; ++i) {
            const hb_seg& g = sc.segs[(size_t)i];
            CHECK(g.q_tile >= 0 && g.q_tile < nqt && g.n_tiles > 0 && g.stride >= 1 && g.b_tile0 >= 0);
            CHECK(g.slot >= 0 && g.slot < sc.n_slots && g.tile0 >= clock && g.ord >= 0 && g.ord < g.nsl && g.nsl <= sc.max_slots_per_qt);
            clock = g.tile0 + g.n_tiles;
            if (g.slot < 0 || g.slot >= sc.n_slots || g.q_tile < 0 || g.q_tile >= nqt) continue;
            if (g.first) { CHECK(slot_q[g.slot] < 0); slot_q[g.slot] = g.q_tile; slot_blk[g.slot] = b; }
            CHECK(slot_q[g.slot] == g.q_tile && slot_blk[g.slot] == b && g.b_tile0 > slot_last[g.slot]);
            for (int j = 0; j < g.n_tiles; ++j) {
                const long long t = (long long)g.b_tile0 + (long long)g.stride * j;
                CHECK(t < nbt);
                if (t >= nbt) break;
                CHECK(!seen[(size_t)g.q_tile * nbt + t]);
                seen[(size_t)g.q_tile * nbt + t] = 1;
                slot_last[g.slot] = (int)t;
                ++pairs;
            }
        }
    }
    CHECK(pairs == (long long)nqt * nbt);
    CHECK((int)sc.qt_off.size() == nqt + 1 && sc.qt_off[nqt] == (int)sc.qt_slots.size() && (int)sc.qt_slots.size() == sc.n_slots);
    for (int q = 0; q < nqt; ++q)
        for (int i = sc.qt_off[q]; i < sc.qt_off[q + 1]; ++i) CHECK(sc.qt_slots[i] >= 0 && sc.qt_slots[i] < sc.n_slots && slot_q[sc.qt_slots[i]] == q);
    CHECK(sc.phase_bounds.size() == sc.phase_clock.size() * (size_t)sc.G);
    for (size_t p = 0; p < sc.phase_clock.size(); ++p)
        for (int b = 0; b < sc.G; ++b) {
            const int at = sc.phase_bounds[p * sc.G + b];
            CHECK(at >= sc.wg_off[b] && at <= sc.wg_off[b + 1] && (p == 0 || at >= sc.phase_bounds[(p - 1) * sc.G + b]));
        }
    if (sc.cq * sc.cb > 1) {
        CHECK((int)sc.wg_member.size() == sc.G && sc.member_ticks - sc.idle_member_ticks == (long long)nqt * nbt);
        for (int b = 0; b < sc.G; ++b) CHECK(sc.wg_member[b] >= 0 && sc.wg_member[b] / HB_CLUSTER_LINE < sc.n_clusters && sc.wg_member[b] % HB_CLUSTER_LINE < sc.cq * sc.cb);
    }
}

int main() {
    struct shape { int nqt, nbt, G, panel, cq, cb; };
    std::vector<shape> shapes = {{86, 39063, 256, 0, 8, 1}, {49, 8102, 256, 0, 4, 1}, {49, 8102, 256, 0, 4, 2}, {86, 4883, 256, 0, 8, 1}, {7, 1001, 64, 0, 2, 2},
                                 {5, 333, 32, 7, 2, 2}, {3, 4, 256, 0, 2, 2}, {7, 79, 64, 0, 8, 1}, {2, 79, 64, 0, 4, 2}, {11, 79, 64, 0, 4, 2}, {27, 300, 48, 0, 3, 2}};
    for (int r = 1; r < 8; ++r) shapes.push_back({24 + r, 300, 64, 0, 8, 1});
    const double shares[8] = {1.02, 0.98, 1.01, 0.99, 1.0, 1.0, 1.03, 0.97};
    int lists = 0, filled = 0, refused = 0;
    for (const shape& s : shapes)
        for (int form = 0; form < 16; ++form) {
            const bool share = form & 1, weighted = form & 2, phased = form & 4, limited = form & 8;
            if ((long long)s.nqt * s.nbt > 1000000 && form != 1 && form != 4 && form != 7 && form != 13) continue;      // (the headline's lists: four forms)
            std::snprintf(g_what, sizeof g_what, "%d x %d tiles, G %d, panel %d, %d x %d, form %d", s.nqt, s.nbt, s.G, s.panel, s.cq, s.cb, form);
            const int panel = s.panel > 0 ? s.panel : hb_default_panel(s.nqt, (int)std::min<long long>(s.G, (long long)s.nqt * s.nbt), (size_t)HB_BT * 768 * 4, s.cq, s.cb);
            hb_schedule sc;
            hb_build_schedule(s.nqt, s.nbt, s.G, panel, sc, s.cq, s.cb, phased, share, weighted ? shares : nullptr, true, 0);
            walk(sc, s.nqt, s.nbt);
            ++lists; filled += sc.filled;
            if (limited && sc.filled) {
                const int most = sc.max_slots_per_qt;
                hb_schedule lim;
                hb_build_schedule(s.nqt, s.nbt, s.G, panel, lim, s.cq, s.cb, phased, share, weighted ? shares : nullptr, true, most - 1);
                CHECK(!lim.filled && lim.fill_refused && lim.fill_asked && lim.fill_slot_limit == most - 1);
                walk(lim, s.nqt, s.nbt);
                ++lists; refused += lim.fill_refused;
            }
        }
    std::printf("schedule_filled_check: %s (%d lists, %d filled, %d refused)\n", g_bad ? "FAILED" : "ok", lists, filled, refused);
    return g_bad ? 1 : 0;
}
