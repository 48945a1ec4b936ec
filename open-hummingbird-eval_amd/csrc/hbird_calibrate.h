// The decisions the kNN launcher takes from its workgroups' own time stamps (host side, plain C++: no HIP types) -- per-XCD work shares with
// their guard, and whether the fp32 L2-sharing clusters stay.  Shared by hbird_knn.hip (which feeds it the stamps of real launches) and by the
// host-only test hooks hb_calibration_* (tests/test_calibrate_cpu.py; also built under sanitizers with the planner: make plan_asan).
#pragma once
#include <array>
#include <stdint.h>
#include "../../include/hbird_hip.h"
#include "hbird_schedule.h"

#define HB_POOL_MAX 512  // largest candidate pool per (slot, query) in global memory (k > HB_KL)
#define HB_KL 32         // per-query list capacity kept in LDS (k <= HB_KL on the fused path)

// What one launch's stamps say (wg_stamp, hbird_knn_dev.h: per block, at its start and at its end, {100 MHz real-time counter (low word),
// XCC id, shader-cycle counter lo, hi}).
struct hb_stamp_summary {
    double med[8];            // median duration (ticks) of the blocks equal to g mod 8
    int xcc[8];               // the XCD that group ran on
    double all;               // mean of the eight medians
    double span_ticks;        // first start to last end
    double ghz_med, ghz_min, ghz_max;     // shader cycles per tick x 100 MHz, over the workgroups
};
// -> false when the sample cannot be trusted (the region is zeroed before a stamping launch: a block that never stamped reads 0 / 0; blocks
// equal mod 8 that did NOT share an XCD, or two such groups on one XCD, say the dispatch order is not what the share groups assume; a
// duration far from the others' is a wrap or a preempted block).  WHICH XCD a group ran on is an output: HIP promises no placement, block 0
// usually lands on XCD 0 but need not (MI355X_MICROARCH.md, "Workgroup dispatch"), and the shares belong to the physical XCDs.
bool hb_stamps_summarise(const unsigned* st, int G, hb_stamp_summary& o);

// The calibration state of one kernel family of one index (hb_index::xcd_cal adds the HIP side: pinned stamps, event, what is pending).
struct hb_xcd_state {
    double w[8] = {1, 1, 1, 1, 1, 1, 1, 1};          // shares in use, per PHYSICAL XCD
    int rounds = 0;
    int samples = 0, rejected = 0;                   // stamp sets read / thrown away (hb_stamps_summarise)
    // the guard: shares stay only while launches of the same shape measure faster with them
    std::array<int, 6> key{{0, 0, 0, 0, 0, 0}};      // shape of the launches being compared: query tiles, bank tiles, workgroups, phases, k, cluster shape
    double cur_w[8] = {1, 1, 1, 1, 1, 1, 1, 1}, best_w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    double cur_span = 0.0, best_span = 0.0;          // shortest launch (100 MHz ticks, first start to last end) with the current / the best share set
    int cur_n = 0, locked = 0, reverts = 0;          // locked: 1 = by the guard, 2 = the group -> XCD map kept moving (equal shares)
    int perm[8] = {0, 1, 2, 3, 4, 5, 6, 7};          // XCD that group g (blocks equal to g mod 8) was last seen on
    int perm_moves = 0;
    // fp32 family only: the automatic L2-sharing clusters of the biggest searches are kept only where they measure faster
    int cl_state = 0;                                // 0 = measuring with clusters, 1 = measuring without, 2 = decided
    int cl_choice = 1;                               // decided: 1 = clusters, 0 = none
    int cl_n_on = 0, cl_n_off = 0;
    std::array<int, 3> cl_shape{{0, 0, 0}};          // (query tiles, bank tiles, k) of the launches being compared
    double cl_span_on = 0.0, cl_span_off = 0.0;      // shortest qualifying launch with / without clusters (ticks)
};
// One stamp set of a launch that ran with the GROUP shares `run_shares` (group g = blocks equal to g mod 8).
struct hb_stamp_set {
    const unsigned* stamps; int G;
    double run_shares[8];
    std::array<int, 6> key;
    double frac;              // the stamped launch's part of the search's work (a phased search stamps its last launch)
    int auto_cluster;         // the cluster shape of that search was the automatic choice
};
enum { HB_CAL_REBUILD = 1, HB_CAL_REMEMBER_SHARES = 2, HB_CAL_REMEMBER_CLUSTERS = 4, HB_CAL_REJECTED = 8 };
// Feed one stamp set to the state: -> flags (HB_CAL_*): the work list must be rebuilt / the shares (the cluster decision) are worth
// remembering for the device / the set was thrown away.  fam: 0 = the fp32 kernels, 1 = the fp16 candidate kernel.
int hb_xcd_step(hb_xcd_state& c, int fam, const hb_stamp_set& s);

// ---- use_fp16, adaptive use (mode 2: what the plugin's use_fp16=True selects) ---------------------------------------------------------
// On a bank whose neighbours sit closer together than fp16 can tell apart most certificates fail, and passes that certify nothing are pure
// overhead.  The index keeps moving averages of the share of queries that failed the first certificate (r1) and of the share that reached
// the fp32 kernel (r12): r12 > 1/2 -> the fp32 kernel right away; r1 > 1/2 -> the first pass is skipped, ONE pass with k' = 256 serves all
// queries; every 16th search walks the whole chain again, so that a bank (or a query stream) that changes is noticed.
struct hb_f16_adapt { double r1 = 0.0, r12 = 0.0; int searches = 0; };
enum { HB_F16_CHAIN = 0, HB_F16_WIDE_FIRST = 1, HB_F16_FP32 = 2 };
int hb_f16_choose(hb_f16_adapt& a);                                                   // how the next search runs (counts it)
// what that search saw: `first_failed` of `nq` queries failed the first certificate it ran, `reached_fp32` went to the fp32 kernel
void hb_f16_observe(hb_f16_adapt& a, int how, int64_t nq, int64_t first_failed, int64_t reached_fp32);

// ---- the automatic state of the fp16 setting (HB_FP16_AUTO, what a new index starts in: include/hbird_hip.h) --------------------------------
// Whether a search takes the certified fp16 screen.  States 1 / 2 keep their rules (k, ceiling, state 2's work bound); the automatic state adds:
// a big search (>= 30,000 stages per workgroup), an index the caller has not pinned to the fp32 kernel, no HBIRD_EXACT_SCREEN=0, no overflow,
// and room for the fp16 copy.  Memory is asked about last and only in the automatic state without a copy: the launcher calls once with
// mem_known = false (no hipMemGetInfo for searches that stay on the fp32 kernel anyway) and, on "screen", again with the device's figures.
struct hb_screen_in {
    int setting = 0;              // 0 / 1 / 2 / HB_FP16_AUTO
    bool pinned = false;          // hb_index_set_variant / _tuning / _cluster / _cluster_sharing / _xcd_weights / _search_options was used
    bool env_off = false;         // HBIRD_EXACT_SCREEN=0 at hb_index_create
    int k = 0;
    bool ceiling = false;         // a later pass of a search with k > 256
    int64_t rows = 0, nq = 0;
    int d = 0;
    long long stages_per_wg = 0;
    bool overflow = false;        // the bank holds a finite value beyond the fp16 range
    bool have_copy = false;       // the fp16 tiles exist for the bank's current capacity
    bool declined = false;        // ... or were found not to fit at this capacity
    bool mem_known = false;
    uint64_t free_b = 0, total_b = 0, bank_b = 0, copy_b = 0;
};
bool hb_screen_choose(const hb_screen_in& in, int* why);     // -> the screen (true) or the fp32 kernel; *why = HB_WHY_*

// ---- the re-rank's row copy (hb_index_set_rerank_copy): whether an index gets the bank once more as fp32 rows -------------------------------
// setting 1: always, 2: never, 0: by the bank's and the device's sizes (the rule and its measurements: hbird_calibrate.cpp).  The launcher
// (hbird_knn.hip) asks the device and remembers a refusal for the capacity.
bool hb_rerank_copy_choose(int setting, uint64_t bank_b, uint64_t need_b, uint64_t free_b, uint64_t total_b);

// ---- the shape plan of one search (hb_launch_knn, hbird_knn.hip) ------------------------------------------------------------------------
// Everything the launcher derives from the search's sizes and the index's override fields before it touches the device: which kernel runs,
// on pools or lists, with which clusters, phased or not.  Plain values in, plain values out (CPU tests: hb_knn_plan_replay, tests/
// test_knn_plan_cpu.py).  Three steps, because two facts of the launcher sit between them:
//   hb_knn_plan_shape     what needs only the sizes: kc, pools or lists, the grid, whether the shares are calibrated (balance);
//   -- the launcher runs hb_xcd_calibrate where `balance` says so: it may flip cl_state / cl_choice, which the caller then copies into `in` --
//   hb_knn_plan_clusters  the cluster shape from the state the calibration left, and what hangs on it: panel, phased, xs, lag;
//   -- the launcher builds (or finds cached) the work list: a list has fewer workgroups than G when there are fewer pairs, and a cached list
//      of the nested searches may date from another hb_index_set_tuning --
//   hb_knn_plan_kernel    `small` and the kernel, from the work list's own workgroup count.
struct hb_knn_plan_in {
    bool f16 = false;             // the final decision of the screen (hb_screen_choose, the adaptive use, the copy's upkeep)
    bool wide_first = false;      // adaptive use: one pass with k' = 256 serves all queries
    int esc = 0;                  // 0: a caller's search; 1: the second fp16 pass over its uncertified queries; 2: the fp32 search of what is left
    bool ceil = false;            // a later pass of a search with k > 256
    int k = 0;
    int64_t nq = 0, ntotal = 0;
    int g8 = 0, dp = 0, dp16 = 0, num_cu = 0;
    int force_G = 0, force_panel = 0, force_cq = 0, force_cb = 0, variant = 0;
    long long small_limit = 0;    // hb_index_set_search_options (0 = the built-in 400,000)
    int phases_on = 1, xcd_balance = 0, xcd_share = 0, sync_lag = -1;
    int cl_state = 0, cl_choice = 1;      // the fp32 family's measured decision about its automatic clusters (hb_xcd_state)
};
// The kernel of the search.  The register-resident forms (hbird_knn_bd.hip) are HB_KERNEL_BD + 4 wide + 2 clustered + 1 small.
enum hb_knn_kernel {
    HB_KERNEL_F16 = 0,            // the fp16 candidate kernel (hbird_knn_f16.hip)
    HB_KERNEL_LISTS = 1, HB_KERNEL_LISTS_COLD = 2, HB_KERNEL_POOLS = 3, HB_KERNEL_LISTS_CL = 4, HB_KERNEL_POOLS_CL = 5, HB_KERNEL_CEIL = 6,      // LDS-staged (hbird_knn.hip)
    HB_KERNEL_BD = 8
};
struct hb_knn_plan {
    // hb_knn_plan_shape
    int kc = 0; bool wide = false; int klw = 0; bool small_pools = false;
    int nqt = 0, nbt = 0, G = 0, fam = 0; bool balance = false;
    bool calibrated = false;      // ... and the shares are the calibration's own: the search stamps its workgroups and (a caller's) feeds hb_xcd_step
    long long small_limit = 0; bool bd_shape = false;      // (kept for hb_knn_plan_kernel)
    // hb_knn_plan_clusters
    int cq = 1, cb = 1; bool auto_cluster = false; int panel = 0;
    bool phased = false, xs = false; int lag = 0;
    bool filled = false;          // the ragged last query group's tiles as rows of other shapes (hb_build_clustered)
    // hb_knn_plan_kernel
    bool small = false; int kernel = HB_KERNEL_LISTS;
};
// "Stages per workgroup", the size by which every threshold of the launcher is stated.  Two formulas, and they differ only when there are
// fewer pairs than workgroups:
// ... all `workgroups` in the divisor (idle ones included: 0 stages when pairs < workgroups).  Used by the screen's automatic state
// (hb_screen_in::stages_per_wg), `balance`, both cluster bounds (the fp16 one with dp16 / 16 stages per tile) and, with the work list's own
// workgroup count, `small`.
long long hb_stages_per_wg(long long nqt, long long nbt, int workgroups, int stages_per_tile);
// ... only the workgroups that get a pair in the divisor (one tile's stages when pairs < workgroups).  Used by small_shape (lists or small pools).
long long hb_stages_per_busy_wg(long long nqt, long long nbt, int workgroups, int stages_per_tile);
inline int hb_knn_workgroups(int force_G, int num_cu) { return force_G > 0 ? force_G : num_cu; }
void hb_knn_plan_shape(const hb_knn_plan_in& in, hb_knn_plan& p);
void hb_knn_plan_clusters(const hb_knn_plan_in& in, hb_knn_plan& p);
void hb_knn_plan_kernel(const hb_knn_plan_in& in, int sched_G, hb_knn_plan& p);
// Most slots per query tile a filled list may have for a pool search of width klw that delivers kc entries: what pool_floor_kernel gathers
// in its 144 KiB of LDS between two phases (beyond it the floors go through the merge, ten times the cost: knn_seed_floors), and what
// launch_merge reaches in two levels of 48 KiB.
int hb_fill_slot_limit(int klw, int kc, bool phased);

// ---- the rungs of an excluding search (hb_index_search_excluding, hbird_exclude.hip) -----------------------------------------------------
// The best k rows outside a group of at most gmax rows are the first k non-excluded entries of the best need = k + gmax rows.  Few queries
// lose a whole group from the top of their list: rung 0 fetches r0 = 256 * ceil((k + min(k, gmax)) / 256) entries -- room for as many excluded
// entries as kept ones, rounded up to whole pool passes of 256, which cost the same -- and only the queries it leaves incomplete are searched
// at need.  r0 >= need: ONE rung at need, complete by construction.
// -> the rung count (1 or 2), rungs[0 .. count) ascending; -1: k outside [1, HB_MAX_K] or gmax < 0; -2: need > HB_MAX_K.
int hb_exclude_plan(int k, int64_t gmax, int rungs[2]);
