// The calibration decisions of the kNN launcher as plain host code (see hbird_calibrate.h): compiled by hipcc into libhbird_hip.so and,
// host-only under sanitizers, into lib/build/libhbird_plan_asan.so beside the planner.
#include "hbird_calibrate.h"
#include "hbird_certificate.h"
#include <algorithm>
#include <cmath>
#include <vector>

bool hb_stamps_summarise(const unsigned* st, int G, hb_stamp_summary& o) {
    if (G < 8 || G % 8 != 0) return false;
    std::vector<double> dur[8], every, ghz;
    const unsigned s0 = st[0];
    long long first = 0, last = 0;
    for (int b = 0; b < G; ++b) {
        const unsigned* sb = st + 8 * (size_t)b;
        const unsigned t0 = sb[0], t1 = sb[4], xcc = sb[1];
        if (t0 == 0u && t1 == 0u) return false;
        if (xcc > 7u || sb[5] != xcc) return false;
        if (b < 8) o.xcc[b] = (int)xcc;
        else if ((int)xcc != o.xcc[b & 7]) return false;
        const unsigned d = t1 - t0;                       // (mod 2^32: a launch is far shorter than 43 s)
        if (d == 0u || d > 0x7FFFFFFFu) return false;
        dur[b & 7].push_back((double)d); every.push_back((double)d);
        const long long rs = (long long)(int)(t0 - s0), re = rs + (long long)d;
        if (b == 0) { first = rs; last = re; }
        first = std::min(first, rs); last = std::max(last, re);
        const unsigned long long c0 = ((unsigned long long)sb[3] << 32) | sb[2], c1 = ((unsigned long long)sb[7] << 32) | sb[6];
        if (c1 > c0 && d >= 100u) ghz.push_back((double)(c1 - c0) / (double)d * 0.1);       // cycles per 10 ns tick -> GHz
    }
    for (int x = 0, seen = 0; x < 8; ++x) { if (seen & (1 << o.xcc[x])) return false; seen |= 1 << o.xcc[x]; }
    std::nth_element(every.begin(), every.begin() + every.size() / 2, every.end());
    const double m_all = every[every.size() / 2];
    o.all = 0.0;
    for (int x = 0; x < 8; ++x) {
        if (dur[x].empty()) return false;
        std::nth_element(dur[x].begin(), dur[x].begin() + dur[x].size() / 2, dur[x].end());
        o.med[x] = dur[x][dur[x].size() / 2];
        if (!(o.med[x] > 0.5 * m_all && o.med[x] < 1.5 * m_all)) return false;
        o.all += o.med[x] / 8.0;
    }
    o.span_ticks = (double)(last - first);
    o.ghz_med = o.ghz_min = o.ghz_max = 0.0;
    if (!ghz.empty()) {
        std::sort(ghz.begin(), ghz.end());
        o.ghz_med = ghz[ghz.size() / 2]; o.ghz_min = ghz.front(); o.ghz_max = ghz.back();
    }
    return true;
}

int hb_xcd_step(hb_xcd_state& c, int fam, const hb_stamp_set& s) {
    int flags = 0;
    hb_stamp_summary sm;
    if (!hb_stamps_summarise(s.stamps, s.G, sm)) { ++c.rejected; return HB_CAL_REJECTED; }
    ++c.samples;
    // Everything below is in terms of the PHYSICAL XCDs: group g of this launch ran on XCD sm.xcc[g] with the share stamp_w[g].  A launch
    // whose groups sat on other XCDs than the work list assumed (c.perm) moves the map (and the list is rebuilt for it); a map that keeps
    // moving makes shares meaningless: after three moves this index keeps equal shares.
    double run_w[8], med[8];
    for (int g = 0; g < 8; ++g) { run_w[sm.xcc[g]] = s.run_shares[g]; med[sm.xcc[g]] = sm.med[g]; }
    if (!std::equal(sm.xcc, sm.xcc + 8, c.perm)) {
        std::copy(sm.xcc, sm.xcc + 8, c.perm);
        flags |= HB_CAL_REBUILD;
        if (++c.perm_moves >= 3) { for (int x = 0; x < 8; ++x) c.w[x] = 1.0; c.locked = 2; }
    }
    // The fp32 kernel's automatic L2-sharing clusters (2 x 4 for the biggest searches) cut the L2-miss traffic by 60 % and cost cycles (the
    // soft sync, more slots, shorter segments).  Whether that pays is a property of the BOX: round 5's driver box -- held at 2.31 GHz by its
    // power budget -- ran 2.5 % FASTER with them (2314 vs 2374 ms), every box of rounds 5 and 6 that held 2.38-2.39 GHz ran 0.2-0.7 % slower at
    // the same clock.  So it is measured: launches with calibrated shares are timed with clusters (two), then without (two), by their
    // spans; the faster form stays for this index and is remembered for the device.  Five searches in all, then nothing changes any more.
    const std::array<int, 3> shape_now{{s.key[0], s.key[1], s.key[4]}};      // (query tiles, bank tiles, k: spans of one shape only)
    if (fam == 0 && s.auto_cluster && c.cl_state < 2 && c.rounds >= 1 && (c.cl_n_on + c.cl_n_off == 0 || shape_now == c.cl_shape)) {
        const bool clustered = s.key[5] != 17;      // (cluster shape q * 16 + b; 1 x 1 = 17)
        c.cl_shape = shape_now;
        if (c.cl_state == 0 && clustered) {
            c.cl_span_on = c.cl_n_on ? std::min(c.cl_span_on, sm.span_ticks) : sm.span_ticks;
            if (++c.cl_n_on >= 2) { c.cl_state = 1; flags |= HB_CAL_REBUILD; }
        } else if (c.cl_state == 1 && !clustered) {
            c.cl_span_off = c.cl_n_off ? std::min(c.cl_span_off, sm.span_ticks) : sm.span_ticks;
            if (++c.cl_n_off >= 2) {
                c.cl_state = 2; c.cl_choice = c.cl_span_on < c.cl_span_off ? 1 : 0;
                flags |= HB_CAL_REBUILD;
                flags |= HB_CAL_REMEMBER_CLUSTERS;
            }
        }
    }
    if (c.locked == 2) return flags;
    // The GUARD: shares are kept only while they measure faster.  Launches of one shape (the key) are compared by their span (first start to
    // last end, the minimum over a share set's launches: clock dips only ever lengthen one); a share set that has had two launches and is still
    // 0.15 % slower than the best set seen (fp16 family: three launches, 0.8 %) goes, the best set comes back, and this index stops calibrating that family (round 5's driver box
    // ran 1.6 % slower than the builder's boxes with shares spread +- 2.8 %, and its record could not say whether the shares were the reason).
    if (c.key != s.key) { c.key = s.key; c.best_span = 0.0; c.cur_n = 0; c.locked = 0; }
    if (c.cur_n > 0 && std::equal(run_w, run_w + 8, c.cur_w)) { c.cur_span = std::min(c.cur_span, sm.span_ticks); ++c.cur_n; }
    else {
        if (c.cur_n > 0 && (c.best_span == 0.0 || c.cur_span < c.best_span)) { c.best_span = c.cur_span; std::copy(c.cur_w, c.cur_w + 8, c.best_w); }
        std::copy(run_w, run_w + 8, c.cur_w); c.cur_span = sm.span_ticks; c.cur_n = 1;
    }
    // (the fp16 candidate kernel's launches scatter by +- 0.5 % from search to search and its stamps cover the last phase only: three launches and
    // 0.8 % there -- with the fp32 rule one box of round 6 went back to equal shares on a 0.4 % difference and kept them: 284 ms where shares give 275)
    const int guard_n = fam ? 3 : 2;
    const double guard_tol = fam ? 1.008 : 1.0015;
    if (c.best_span > 0.0 && c.cur_n >= guard_n && c.cur_span > c.best_span * guard_tol && !std::equal(c.cur_w, c.cur_w + 8, c.best_w)) {
        for (int x = 0; x < 8; ++x) c.w[x] = c.best_w[x];
        flags |= HB_CAL_REBUILD;
        c.locked = 1; ++c.reverts; ++c.rounds;
        flags |= HB_CAL_REMEMBER_SHARES;
        return flags;
    }
    if (c.locked) return flags;
    // (a duration that is off by e in a launch holding the part f of the work is mended by e x f of the whole share)
    double w[8], mean = 0.0, change = 0.0;
    for (int x = 0; x < 8; ++x) { w[x] = run_w[x] * (1.0 + s.frac * (sm.all / med[x] - 1.0)); mean += w[x] / 8.0; }
    for (int x = 0; x < 8; ++x) {
        w[x] = std::min(1.25, std::max(0.8, w[x] / mean));
        if (fam && c.rounds >= 2) w[x] = 0.5 * (w[x] + c.w[x]);      // the fp16 kernel's durations scatter by +- 0.5 % from search to search: damped ...
        change = std::max(change, std::fabs(w[x] / c.w[x] - 1.0));
    }
    // ... and a new work list (10 M x 768: 8 ms of host time) only for a change that is worth it
    const double worth = fam ? (c.rounds < 2 ? 0.003 : c.rounds < 4 ? 0.006 : 0.012) : (c.rounds < 2 ? 0.0015 : c.rounds < 6 ? 0.003 : 0.006);   // (fp16: 0.5 % / 0.8 % kept the shares moving: slower; fp32, round 6: 0.3 % for ever re-planned four times in twenty steps)
    if (change > worth) {
        for (int x = 0; x < 8; ++x) c.w[x] = w[x];
        flags |= HB_CAL_REBUILD;                            // rebuilt with the new shares by the caller
        flags |= HB_CAL_REMEMBER_SHARES;
    }
    ++c.rounds;
    return flags;
}

int hb_f16_choose(hb_f16_adapt& a) {
    const bool probe = (a.searches++ & 15) == 15;
    if (!probe && a.r12 > 0.5) return HB_F16_FP32;
    if (!probe && a.r1 > 0.5) return HB_F16_WIDE_FIRST;
    return HB_F16_CHAIN;
}
void hb_f16_observe(hb_f16_adapt& a, int how, int64_t nq, int64_t first_failed, int64_t reached_fp32) {
    if (nq <= 0 || how == HB_F16_FP32) return;                 // (the fp32 kernel right away: nothing was observed)
    if (how == HB_F16_CHAIN) a.r1 = 0.5 * a.r1 + 0.5 * (double)first_failed / (double)nq;      // (a wide-first search does not run the first pass)
    a.r12 = first_failed == 0 ? 0.5 * a.r12 : 0.5 * a.r12 + 0.5 * (double)reached_fp32 / (double)nq;
}

bool hb_screen_choose(const hb_screen_in& in, int* why) {
    int w = HB_WHY_EXPLICIT_FP32;
    bool screen = false;
    const double kc_rel = std::min(256, std::max(64, (2 * in.k + 7) / 8 * 8)) / 64.0;
    const bool worth = in.rows >= 4096 && (double)in.rows * (double)in.nq * (double)in.d >= 1.5e10 * kc_rel * kc_rel;
    if (in.setting == 0) w = HB_WHY_EXPLICIT_FP32;
    else if (in.k > 128) w = HB_WHY_K;
    else if (in.ceiling) w = HB_WHY_CEILING;       // (only the fp32 pool kernel knows ceilings)
    else if (in.setting == 1) { screen = true; w = HB_WHY_EXPLICIT_FP16; }
    else if (!worth) w = HB_WHY_WORK;
    else if (in.setting == 2) { screen = true; w = HB_WHY_EXPLICIT_FP16; }
    else if (in.pinned) w = HB_WHY_PINNED;
    else if (in.env_off) w = HB_WHY_ENV;
    else if (in.stages_per_wg < 30000) w = HB_WHY_SMALL;
    else if (in.overflow) w = HB_WHY_OVERFLOW;
    else if (in.have_copy) { screen = true; w = HB_WHY_AUTO; }
    else if (in.declined) w = HB_WHY_MEMORY;
    // the optional re-rank copy's rule (hbird_knn.hip): all copies within 55 % of the device, and free memory above the need plus the larger of
    // 1/16 of the device and 2 GiB -- the search's workspace comes after the copy, and a device shared with a model or another rank is not
    // filled to the brim by a copy that only buys speed
    else if (in.mem_known && !(in.bank_b + in.copy_b <= in.total_b / 100 * 55 &&
                               in.free_b > in.copy_b + std::max<uint64_t>(in.total_b / 16, (uint64_t)2 << 30))) w = HB_WHY_MEMORY;
    else { screen = true; w = HB_WHY_AUTO; }
    if (why) *why = w;
    return screen;
}

// Automatic (round 6, by measurement: profiles/r06/final/fp16_residency.json): what the copy saves is a few ms of re-rank per search (about 4 ms
// for 21,904 queries x 64 candidates), whatever the bank's size, and what it costs is the bank once more.  At 300,000 x 768 that is 17 % of a
// search for 0.9 GB; at 10 M x 768 1.5 % for 30.7 GB (30.7 GB of tiles + 15.4 GB of fp16 tiles + 30.7 GB of rows, of 288), at 20 M x 1024 and
// 27.7 M x 768 0.4 % for 83-85 GB.  So only banks of up to 4e9 values (16 GB of fp32: 5.2 M x 768) get it -- a use_fp16 index of a bigger bank
// holds 1.5 x the bank (fp32 tiles for the exact re-rank and the fp32 searches, fp16 tiles for the candidate pass), not 2.5 x -- and, as before,
// only where the three copies stay within 55 % of the device with room to spare: the search's own workspace is allocated after the copy, and a
// device shared with a model or another rank must not be filled to the brim by an optional copy.
bool hb_rerank_copy_choose(int setting, uint64_t bank_b, uint64_t need_b, uint64_t free_b, uint64_t total_b) {
    if (setting != 0) return setting == 1;
    return bank_b <= (uint64_t)16e9 && bank_b + bank_b / 2 + need_b <= total_b / 100 * 55 && free_b > need_b + std::max<uint64_t>(total_b / 16, (uint64_t)2 << 30);
}

// ---- the shape plan of one search (hbird_calibrate.h) -----------------------------------------------------------------------------------
long long hb_stages_per_wg(long long nqt, long long nbt, int workgroups, int stages_per_tile) {
    return nqt * nbt / std::max(1, workgroups) * stages_per_tile;
}
long long hb_stages_per_busy_wg(long long nqt, long long nbt, int workgroups, int stages_per_tile) {
    const long long pairs = nqt * nbt;
    return pairs / std::max<long long>(1, std::min<long long>(workgroups, pairs)) * stages_per_tile;
}

void hb_knn_plan_shape(const hb_knn_plan_in& in, hb_knn_plan& p) {
    const int k = in.k;
    const bool f16 = in.f16, ceil = in.ceil;
    // fp16 mode: the fused kernel collects kc >= 2k candidates, the fp32 chain arithmetic re-ranks them
    // k' = 2k, at least 64 (rounded up to 8, not to 64 as until round 4: the candidate kernel's time is linear in k' -- 300,000 x 768, 21,904
    // queries: k' = 64 / 128 / 192 / 256 -> 12.95 / 15.85 / 20.7 / 25.0 ms -- so k = 33 paid for 128 candidates where it needs 66)
    p.kc = f16 ? (in.esc == 1 || in.wide_first ? 256 : std::min(256, std::max(64, (2 * k + 7) / 8 * 8))) : k;     // (the second pass: the widest list the re-rank takes)
    // Small searches (few stages per workgroup) on the kernel with register-resident query fragments run on POOLS even for k <= 32:
    // phased, with the bisection cold start and the scan epilogue (hbird_knn_bd.hip <WIDE, COLD>) a pool takes a tile's survivors in one
    // drain, a sorted LDS list one wave-cooperative insertion each.  Same box, kernel ms, lists / pools, k = 30: 50,176 x 384 x 12,544
    // queries 4.61 / 4.13 (k = 32: 4.50 / 3.84), x 21,904 queries 7.04 / 6.52, 50,176 x 768 12.47 / 12.16, 200 k x 384 14.76 / 13.89,
    // 300 k x 768 40.6 / 39.9, 2,074,072 x 384 140.5 / 137.4, 600 k x 1024 105.8 / 105.3, 1.25 M x 768 286.0 / 286.7, 2.5 M x 768
    // 573.5 / 571.5, 20 k x 384 x 784 queries 0.59 / 0.26, 100 k x 384 x 196 queries 0.61 / 0.26; k = 5 at 50,176 x 384 3.61 / 3.68 and
    // k = 1 at 200 k x 384 13.47 / 13.54 (few insertions anyway) -> from k = 8.  (Round 2 measured pools at 8.1 vs 5.0 ms for the first
    // of these: unphased, radix cold start, LDS walk.)  Variant 6 keeps the lists (A/B, tests).
    p.small_limit = in.small_limit > 0 ? in.small_limit : 400000;   // stages per workgroup (hb_index_set_search_options)
    p.G = hb_knn_workgroups(in.force_G, in.num_cu);
    const long long nqt = (in.nq + HB_QT - 1) / HB_QT, nbt = (in.ntotal + HB_BT - 1) / HB_BT;
    const bool small_shape = hb_stages_per_busy_wg(nqt, nbt, p.G, in.g8) < std::min<long long>(p.small_limit, 120000);   // no gain beyond (1.25 M x 768: 157 k stages)
    p.bd_shape = in.g8 % 4 == 0 && in.variant != 4;
    p.small_pools = !f16 && !ceil && k >= 8 && k <= HB_KL && small_shape && p.bd_shape && (in.variant == 0 || in.variant == 3) && in.force_cq <= 1;
    p.wide = f16 || k > HB_KL || p.small_pools || ceil;
    // pools (k > HB_KL): capacity >= 2 kc so that a compaction is paid for by >= kc cheap appends
    // (smaller / larger pools measure the same on the fp16 candidate kernel: kc + 64, kc + 192)
    p.klw = p.wide ? std::min(HB_POOL_MAX, (std::max(2 * p.kc, p.kc + 128) + 63) / 64 * 64) : HB_KL;
    // (tile counts as int from here on, as the work list holds them: the same values for every bank and query set of up to (2^31 - 1) x 256 rows)
    p.nqt = (int)nqt; p.nbt = (int)nbt;
    // per-XCD work shares (hb_xcd_calibrate, hbird_knn.hip; read BEFORE the cluster shape is chosen: the calibration also decides whether the fp32 clusters stay): calibrated for fp32 searches from 30,000 stages per workgroup (30-60 ms of kernel; from 150,000 until late in
    // round 5: cfg-2's 2 M x 384 bank went without, 135.3 -> 134.7 ms with; phased searches gain in their last phase only);
    // shares given by the caller (mode 2) apply to searches of any size, both kernel families (tests/fuzz_small.py FUZZ_XCD=1)
    p.fam = f16 ? 1 : 0;
    p.balance = p.G % 8 == 0 && (in.xcd_balance == 2 || (in.xcd_balance == 0 && hb_stages_per_wg(p.nqt, p.nbt, p.G, in.g8) >= 30000));
    p.calibrated = p.balance && in.xcd_balance == 0;
}

void hb_knn_plan_clusters(const hb_knn_plan_in& in, hb_knn_plan& p) {
    const bool f16 = in.f16;
    const int nqt = p.nqt, nbt = p.nbt, G = p.G;
    // L2-sharing clusters (hb_index_set_cluster; automatic shapes below): q x b workgroups of one XCD walk the same bank /
    // query tiles within `lag` stages of each other, so one L2 fill serves several.  Neither kernel is bound by the fabric
    // (the fp32 one by the matrix pipe, the fp16 candidate kernel by its LDS-DMA copies and the power the chip grants it:
    // profiles/LABBOOK.md, profiles/r02), so what they buy is traffic, and time only for the fp16 kernel (-8 %).  The 4-wave variant
    // does not know strided segments.
    int cq = 1, cb = 1;
    p.auto_cluster = false;      // fp32: the cluster shape of this search is the automatic choice (kept only where it measures faster)
    if (in.ceil) { cq = 1; cb = 1; }
    else if (in.force_cq > 0 && in.force_cb > 0) { cq = in.force_cq; cb = in.force_cb; }
    // fp16 candidate kernel: from 70 k stages per workgroup up (round 4: with the lean stage loop and the XCD-level query sharing the
    // clusters pay much earlier than the 400 k of round 3).  Same box, kernel ms (phased), none vs automatic: 10 M x 768 321 / 284,
    // 2.5 M x 768 (157 k stages) 83.0 / 77.5, 5 M x 384 (157 k) 85.3 / 80.3, 1.25 M x 768 (79 k) 43.7 / 41.8, 5 M x 768 x 12,544 queries
    // (179 k; 49 query tiles: 4 x 2) 94.0 / 88.2 -- but 2,074,072 x 384 (37 k) 21.3 / 22.8: more slots, shorter segments
    // (profiles/r04/f16_cluster_threshold.txt)
    else if (f16 && in.variant == 0 && in.force_cq == 0) {
        if (hb_stages_per_wg(nqt, nbt, G, in.dp16 / 16) >= 70000) hb_default_cluster(nqt, nbt, G, false, &cq, &cb);
    }
    // fp32: only beside the kernel with register-resident query fragments (its sync is free of spills), and only for the
    // biggest searches: 2 x 4 clusters cut the fabric reads by 60 % (10 M x 768: 4.79 -> 1.93 TB per search, L2 hit rate
    // 10 % -> 63 %) but the kernel is bound by the matrix pipe, so all they can do for the time is cost little -- measured
    // (same box, kernel ms, none vs 2 x 4): 10 M x 768 2280 vs 2298 (+0.8 %), 5 M x 1024 1528 vs 1531 (+0.2 %), but
    // 1.25 M x 768 289.3 vs 293.9 (+1.6 %), 2 M x 384 142.3 vs 146.4 (+2.9 %): more slots, shorter segments.  Automatic from
    // one million stages per workgroup up (8 M rows at D = 768); hb_index_set_cluster(ix, 1, 1, 0) turns them off, (ix, 2, 4, -1) forces them.
    // Round 6: ... and only where they MEASURE faster on this box (hb_xcd_calibrate: two calibrated launches with, two without, the faster
    // form stays); without the calibration's stamps (equal or given shares) they stay on.
    else if (!f16 && !p.wide && in.variant == 0 && in.force_cq == 0 && in.g8 % 4 == 0 && hb_stages_per_wg(nqt, nbt, G, in.g8) >= 1000000) {
        p.auto_cluster = true;
        const bool measured = in.xcd_balance == 0 && G % 8 == 0;
        // (a decision, once made, holds whatever the share mode; before it: on while measuring with, off while measuring without)
        if (in.cl_state == 2 ? in.cl_choice != 0 : (!measured || in.cl_state == 0)) hb_default_cluster(nqt, nbt, G, true, &cq, &cb);
    }
    if ((long long)nqt * nbt < G || cq * cb > HB_CLUSTER_MAX || G % (8 * cq * cb) != 0) { cq = 1; cb = 1; }
    p.cq = cq; p.cb = cb;
    const size_t tile_bytes = (size_t)HB_BT * in.dp * 4;
    p.panel = in.force_panel > 0 ? in.force_panel : hb_default_panel(nqt, std::min<long long>(G, (long long)nqt * nbt), tile_bytes, cq, cb);
    // phased searches (pools only: "Phased searches" above hb_launch_knn); hb_index_set_search_options(ix, 0, ...) turns them off (A/B, tests)
    // (a nested search of uncertified queries starts from seeded floors: phases would only add boundaries -- and with one query tile over 256
    // workgroups the floors between them go through the merge kernels: 70 ms for two queries)
    p.phased = p.wide && in.phases_on && in.esc == 0;
    // XCD-level sharing of the query tiles (hb_build_clustered): automatic for the fp16 candidate kernel -- same box, 10 M x 768, 8 x 1
    // clusters: 302.7 -> 291.5 ms and 0.97 -> 0.52 TB of L2-miss traffic per search (L2 hit rate 0.60 -> 0.78); the fp32 kernel's 2 x 4
    // clusters lose 1.6 % with it (2298 -> 2334 ms: 1600 slots instead of 592, and its 768 KiB query tiles do not stay in L2 beside
    // sixteen bank streams anyway: 1.95 -> 1.62 TB) -> off there (profiles/r04/xs_*.txt)
    p.xs = cq * cb > 1 && (in.xcd_share >= 2 || (in.xcd_share == 0 && f16));
    // The filled dealing (hb_build_clustered): the leftover tiles of a ragged last query group as rows of other shapes, so that no member idles
    // for a whole row -- the fp16 candidate kernel's lists only (automatic wherever its clusters are on and a tile is left over; mode 3 asks
    // for it by name, modes 1 and 2 keep the lists of old).  The launcher adds the slot limit (hb_fill_slot_limit).
    p.filled = f16 && cq * cb > 1 && nqt > cq && nqt % cq != 0 && (in.xcd_share == 3 || in.xcd_share == 0);
    // soft-sync lag in stages: the members stay inside the L2's reach (4 MiB per XCD: tens of fp32 k8 stages); 0 disables
    // the sync (the members then share only while they happen to run together: 36 % instead of 53 % L2 hits)
    p.lag = cq * cb > 1 ? (in.sync_lag >= 0 ? in.sync_lag : 16) : 0;
}

int hb_fill_slot_limit(int klw, int kc, bool phased) {
    const long long lds = 48 * 1024 / 8;                                           // entries of a merge block's LDS
    const long long w = std::max(1, klw), k = std::max(1, kc);
    long long lim = lds / w >= 2 ? std::max<long long>(lds / w, (lds / w) * (lds / k)) : 2 * (lds / k);   // one level, or groups of lds / w slots x lds / k groups
    if (phased) lim = std::min<long long>(lim, 144 * 1024 / 16 / w);               // one wave's share of the floor kernel's LDS, in pool entries
    return (int)std::max<long long>(1, std::min<long long>(lim, 1 << 20));
}

void hb_knn_plan_kernel(const hb_knn_plan_in& in, int sched_G, hb_knn_plan& p) {
    const bool clustered = p.cq * p.cb > 1;
    // Few stages per workgroup: a slot sees few rows, so its cold start (the first tile inserts all 256 rows of every
    // query) and its insertions (k ln(rows / k) per query) are a visible share of the search -> the instantiations with the
    // cold start, the scan epilogue (register queue + immediate inserts) and the per-tile exchange of
    // threshold floors (hbird_knn_dev.h: small_floor_*).  Same box, kernel ms, LDS-staged small / B-direct plain / B-direct small:
    // 50,176 x 384: 4.86 / 6.76 / 4.62 (round 1: 6.3; 0.49 -> 0.665 of the fp32 MFMA peak); 200 k x 384: 15.9 / 17.7 / 15.1;
    // 300 k x 768: 74.7 / 72.8 / 70.7; 2 M x 384: 149.3 / 143.1 / 142.3; 1.25 M x 768: 305.9 / 291.2 / 289.8; 2.5 M x 768 (315 k
    // stages per workgroup): 612.7 / 579.1 / 579.6 -> small below 400 k stages.  The big searches keep the plain
    // instantiations: at 10 M x 768 the extra code costs 0.3 % (same-box A/B).
    // lists: cold_fn / <false, false, COLD>; pools: <WIDE, false, COLD> -- for k > 32 only below 50 k stages (k = 90: 50,176 x 384 4.78 -> 4.45 ms,
    // k = 64 at 300 k x 768 41.9 -> 40.3, but 2,074,072 x 384 (74 k stages) 142.0 -> 142.7)
    const long long stages_per_wg = hb_stages_per_wg(p.nqt, p.nbt, sched_G, in.g8);
    p.small = !in.f16 && !clustered && stages_per_wg < (in.k > HB_KL ? std::min<long long>(p.small_limit, 50000) : p.small_limit);
    // The query fragments straight into registers (hbird_knn_bd.hip): -3.8 % kernel time at 10 M x 768 (0.895 -> 0.93 of the
    // fp32 MFMA peak), same bits.  Default for the big LDS-list searches whose stage count per tile is a multiple of four
    // (D = 384, 768, 1024, ...); variant 3 forces it wherever it applies (tests), variant 4 keeps the LDS-staged kernel.
    if (in.f16) p.kernel = HB_KERNEL_F16;
    else if (in.ceil) p.kernel = HB_KERNEL_CEIL;
    else if (p.bd_shape && (in.variant == 0 || in.variant == 3 || in.variant == 6)) p.kernel = HB_KERNEL_BD + (p.wide ? 4 : 0) + (clustered ? 2 : 0) + (p.small ? 1 : 0);
    else if (clustered) p.kernel = p.wide ? HB_KERNEL_POOLS_CL : HB_KERNEL_LISTS_CL;
    else if (p.small && !p.wide) p.kernel = HB_KERNEL_LISTS_COLD;
    else p.kernel = p.wide ? HB_KERNEL_POOLS : HB_KERNEL_LISTS;
}

// ---- test hooks (no GPU): a calibration state fed with synthetic stamp sets -----------------------------------------------------------
struct hb_calibration { hb_xcd_state st; int fam; };
extern "C" void* hb_calibration_new(int fp16_kernel) { hb_calibration* h = new hb_calibration(); h->fam = fp16_kernel ? 1 : 0; return h; }
extern "C" void hb_calibration_free(void* h) { delete static_cast<hb_calibration*>(h); }
// the GROUP shares the next launch would run with (the physical shares through the group -> XCD map, divided by their mean), and the state
extern "C" int hb_calibration_state(const void* hv, double shares8[8], int64_t out[12]) {
    if (!hv || !shares8 || !out) return -1;
    const hb_xcd_state& c = static_cast<const hb_calibration*>(hv)->st;
    double mean = 0.0;
    for (int x = 0; x < 8; ++x) mean += c.w[x] / 8.0;
    for (int g = 0; g < 8; ++g) shares8[g] = c.w[c.perm[g]] / mean;
    out[0] = c.rounds; out[1] = c.locked; out[2] = c.reverts; out[3] = c.samples; out[4] = c.rejected; out[5] = c.perm_moves;
    out[6] = c.cl_state; out[7] = c.cl_choice; out[8] = c.cur_n; out[9] = c.perm[0]; out[10] = c.cl_n_on; out[11] = c.cl_n_off;
    return 0;
}
// one launch's stamps [G][2][4] (wg_stamp layout), the group shares it ran with, its shape key [6], whether its cluster shape was automatic
extern "C" int hb_calibration_feed(void* hv, const uint32_t* stamps, int G, const double run_shares8[8], const int key6[6], int auto_cluster, double frac) {
    if (!hv || !stamps || !run_shares8 || !key6) return -1;
    hb_calibration* h = static_cast<hb_calibration*>(hv);
    hb_stamp_set s;
    s.stamps = stamps; s.G = G; s.frac = frac; s.auto_cluster = auto_cluster;
    for (int x = 0; x < 8; ++x) s.run_shares[x] = run_shares8[x];
    for (int x = 0; x < 6; ++x) s.key[x] = key6[x];
    return hb_xcd_step(h->st, h->fam, s);
}
// the adaptive use of use_fp16 (mode 2): a fresh state walked through a stream of searches -- per search how it would run (out_how[i]) given
// what the searches before it saw: failing shares of the first certificate f1[i] and of the second pass f2[i] (of those that entered it)
extern "C" int hb_f16_adapt_replay(int n, const double* f1, const double* f2, int64_t nq, int* out_how) {
    if (n < 0 || !f1 || !f2 || !out_how || nq <= 0) return -1;
    hb_f16_adapt a;
    for (int i = 0; i < n; ++i) {
        const int how = hb_f16_choose(a);
        out_how[i] = how;
        const int64_t failed1 = (int64_t)std::llround(f1[i] * (double)nq);
        // chain: the second pass takes the first's failures, its own failures reach fp32; wide-first: the k' = 256 pass runs on all queries and
        // fails where BOTH would have (f1 x f2 of them)
        const int64_t first_failed = how == HB_F16_WIDE_FIRST ? (int64_t)std::llround(f1[i] * f2[i] * (double)nq) : failed1;
        const int64_t fp32 = how == HB_F16_WIDE_FIRST ? first_failed : (int64_t)std::llround(f2[i] * (double)failed1);
        hb_f16_observe(a, how, nq, first_failed, fp32);
    }
    return 0;
}
// the automatic state's decision for one imagined search (include/hbird_hip.h)
extern "C" int hb_exact_screen_replay(int setting, int pinned, int env_off, int k, int ceiling, int64_t rows, int64_t nq, int d, int64_t stages_per_wg,
                                      int overflow, int have_copy, int declined, uint64_t free_bytes, uint64_t total_bytes, uint64_t bank_bytes,
                                      uint64_t copy_bytes, int* why) {
    if (!why || setting < 0 || setting > HB_FP16_AUTO || k < 1 || rows < 0 || nq < 0 || d < 1) return -1;
    hb_screen_in in;
    in.setting = setting; in.pinned = pinned != 0; in.env_off = env_off != 0; in.k = k; in.ceiling = ceiling != 0; in.rows = rows; in.nq = nq; in.d = d;
    in.stages_per_wg = stages_per_wg; in.overflow = overflow != 0; in.have_copy = have_copy != 0; in.declined = declined != 0;
    in.mem_known = true; in.free_b = free_bytes; in.total_b = total_bytes; in.bank_b = bank_bytes; in.copy_b = copy_bytes;
    return hb_screen_choose(in, why) ? 1 : 0;
}
// the re-rank copy's admission for one imagined index (include/hbird_hip.h)
extern "C" int hb_rerank_copy_replay(int setting, uint64_t bank_bytes, uint64_t need_bytes, uint64_t free_bytes, uint64_t total_bytes) {
    if (setting < 0 || setting > 2 || bank_bytes == 0 || need_bytes == 0 || total_bytes == 0 || free_bytes > total_bytes) return -1;
    return hb_rerank_copy_choose(setting, bank_bytes, need_bytes, free_bytes, total_bytes) ? 1 : 0;
}
// the launcher's shape plan for one imagined search (include/hbird_hip.h: the slots)
extern "C" int hb_knn_plan_replay(const int64_t* in, int n_in, int64_t* out, int n_out) {
    if (!in || !out || n_in < 23 || n_out < 19) return -1;
    if (in[4] < 1 || in[5] < 0 || in[6] < 0 || in[7] < 1 || in[8] < 1 || in[9] < 16 || in[10] < 1 || (n_in > 23 && in[23] < 0)) return -1;
    hb_knn_plan_in pin;
    pin.f16 = in[0] != 0; pin.wide_first = in[1] != 0; pin.esc = (int)in[2]; pin.ceil = in[3] != 0;
    pin.k = (int)in[4]; pin.nq = in[5]; pin.ntotal = in[6]; pin.g8 = (int)in[7]; pin.dp = (int)in[8]; pin.dp16 = (int)in[9]; pin.num_cu = (int)in[10];
    pin.force_G = (int)in[11]; pin.force_panel = (int)in[12]; pin.force_cq = (int)in[13]; pin.force_cb = (int)in[14]; pin.variant = (int)in[15];
    pin.small_limit = in[16]; pin.phases_on = (int)in[17]; pin.xcd_balance = (int)in[18]; pin.xcd_share = (int)in[19]; pin.sync_lag = (int)in[20];
    pin.cl_state = (int)in[21]; pin.cl_choice = (int)in[22];
    hb_knn_plan p;
    hb_knn_plan_shape(pin, p);
    hb_knn_plan_clusters(pin, p);
    // the workgroups of a work list built for this search (hb_build_schedule: at most one per pair), or the caller's (a cached list)
    const long long pairs = (long long)p.nqt * p.nbt;
    const int sched_G = n_in > 23 && in[23] > 0 ? (int)in[23] : pairs < p.G ? (int)std::max<long long>(1, pairs) : p.G;
    hb_knn_plan_kernel(pin, sched_G, p);
    out[0] = p.kc; out[1] = p.wide; out[2] = p.klw; out[3] = p.small_pools; out[4] = p.nqt; out[5] = p.nbt; out[6] = p.G; out[7] = p.fam; out[8] = p.balance;
    out[9] = p.cq; out[10] = p.cb; out[11] = p.auto_cluster; out[12] = p.panel; out[13] = p.phased; out[14] = p.xs; out[15] = p.lag; out[16] = p.kernel;
    out[17] = sched_G; out[18] = p.small;
    if (n_out > 19) out[19] = p.filled;
    return 0;
}
// the fp16 screen's bounds as the re-rank kernels compile them (hbird_certificate.h), in float (include/hbird_hip.h: the slots)
extern "C" int hb_certificate_bound_replay(const double* in, int n_in, double* out, int n_out) {
    if (!in || !out || n_in < 8 || n_out < 2 || !(in[0] >= 1.0 && in[0] <= 1048576.0)) return -1;
    const int d = (int)in[0], metric = in[1] != 0.0 ? 1 : 0;
    const float qn = (float)in[2], bmax = (float)in[3], qc = (float)in[4], cmax = (float)in[5], mun = (float)in[6], at = fabsf((float)in[7]);
    out[0] = (double)hb_certificate_bound(qn, bmax, d, metric);
    out[1] = (double)hb_certificate_bound_centred(qc, cmax, mun, at, qn, bmax, d, metric);
    return 0;
}
// the rungs of an excluding search (hbird_calibrate.h)
int hb_exclude_plan(int k, int64_t gmax, int rungs[2]) {
    if (k < 1 || k > HB_MAX_K || gmax < 0) return -1;
    const int64_t need = (int64_t)k + gmax;
    if (need > HB_MAX_K) return -2;
    const int64_t r0 = 256 * (((int64_t)k + std::min<int64_t>(k, gmax) + 255) / 256);
    if (r0 >= need) { rungs[0] = (int)need; return 1; }
    rungs[0] = (int)r0; rungs[1] = (int)need;
    return 2;
}
extern "C" int hb_exclude_plan_replay(int k, int64_t gmax, int* rungs, int max_rungs) {
    int r[2] = {0, 0};
    const int n = hb_exclude_plan(k, gmax, r);
    if (n == -1) return hb_fail("hb_exclude_plan_replay: k must be in [1, " + std::to_string(HB_MAX_K) + "] and gmax >= 0");
    if (n == -2) {
        hb_fail("excluding search: k = " + std::to_string(k) + " plus the largest row group (gmax = " + std::to_string(gmax) + " rows) exceeds the limit of " +
                       std::to_string(HB_MAX_K) + " neighbours per search: use a smaller memory_size or fewer epochs per group");
        return -2;
    }
    if (!rungs || max_rungs < n) return hb_fail("hb_exclude_plan_replay: rungs is NULL or holds fewer than " + std::to_string(n) + " entries");
    for (int i = 0; i < n; ++i) rungs[i] = r[i];
    return n;
}
