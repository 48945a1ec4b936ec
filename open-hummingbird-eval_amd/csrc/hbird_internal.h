// Internal declarations shared by the HIP translation units of libhbird_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <array>
#include <string>
#include <vector>
#include "hbird_schedule.h"
#include "hbird_calibrate.h"
#include "hbird_f16_centre.h"
#include "hbird_devbuf.h"
#include "hbird_mirror.h"
#include "hbird_report.h"
#include "hbird_labels.h"

// ---- tile geometry of the kNN kernel (see DESIGN.md "Data layout in HBM") -------------------
#define HB_RT 32         // rows per fragment tile (MFMA 32x32x2)
// (HB_POOL_MAX and HB_KL, the pool and list capacities: hbird_calibrate.h, beside the plan that chooses between them)
#define HB_THREADS 512
#define HB_WAVES 8
#define HB_BLK 256       // floats per fragment block (32 rows x 8 k) = 1 KiB

#define HB_ID_NONE 0xFFFFFFFFu

// hb_index::bank_changed: what happened to the bank
enum hb_bank_event {
    HB_BANK_APPENDED,      // rows were added within the capacity: the copies catch up at the next search
    HB_BANK_EMPTIED,       // hb_index_reset: no rows, the same capacity
    HB_BANK_MOVED          // hb_index_reserve: a new capacity (the next search that needs a copy releases the old one and makes it anew)
};

// Optional ROCTx range around a host-side phase (shows up under `rocprofv3 --marker-trace`).  The marker library
// (librocprofiler-sdk-roctx.so, else libroctx64.so) is looked up at run time; without it the ranges are no-ops.
struct hb_range {
    explicit hb_range(const char* name);
    ~hb_range();
    hb_range(const hb_range&) = delete;
    hb_range& operator=(const hb_range&) = delete;
};

struct hb_index {
    int d = 0, dp = 0, g8 = 0, metric = 0, device = 0;
    hipStream_t stream = nullptr;
    int64_t ntotal = 0, cap_rows = 0;      // cap_rows is a multiple of HB_BT
    hb_dev<float> tiles;                   // fragment-tiled bank  [cap_rows/32][g8][256]
    hb_dev<float> binit;                   // per-row accumulator init [cap_rows]
    hb_dev<float> bnorm;                   // per-row L2 norm (fp32)  [cap_rows]
    hb_label_store lab;                    // the label table: own rows (fp32 or counts), their counters, the borrowed table (hbird_labels.h)
    int num_cu = 256;
    // search workspace (grown on demand, reused)
    hb_dev<float> q_tiles;
    hb_dev<float> q_aux;                                 // qn2 (chain) and qnorm (fp32), 2*nq floats
    hb_dev<char> state;
    hb_dev<char> sched_dev;
    hb_dev<char> tmp;                                    // staging for host<->device convenience paths
    hb_schedule sched;                                   // cached for (nqt, nbt)
    int force_G = 0, force_panel = 0;                    // test/tuning overrides
    int force_cq = 0, force_cb = 0;                      // cluster shape override (0 = automatic)
    int sync_lag = -1;                                   // soft-sync lag in stages (-1 = automatic, 0 = no sync)
    int xcd_share = 0;                                   // clustered work lists: 0 = automatic, 1 = off, 2 = on, 3 = on and filled (hb_index_set_cluster_sharing)
    // work shares per XCD group (blocks equal mod 8): hb_index_set_xcd_weights / calibrated from the workgroups' own time stamps.
    // Two families with shares of their own: [0] the fp32 kernels, [1] the fp16 candidate kernel (power-limited: its XCDs differ by other amounts)
    struct xcd_cal : hb_xcd_state {                      // (the decisions' state: hbird_calibrate.h; here the HIP side)
        unsigned* stamp_host = nullptr;                  // pinned copy of the last calibrating launch's per-block stamps ...
        hipEvent_t stamp_ev = nullptr;                   // ... complete when this event is
        int stamp_pending = 0;                           // blocks of that launch (0: nothing to read)
        double stamp_w[8] = {1, 1, 1, 1, 1, 1, 1, 1};    // the GROUP shares that launch ran with
        double stamp_frac = 1.0;                         // ... and its part of the search's work (phased searches stamp their LAST launch)
        std::array<int, 6> stamp_key{{0, 0, 0, 0, 0, 0}};   // ... its shape
        int stamp_auto_cluster = 0;                      // ... and whether its cluster shape was the automatic choice
    } xcal[2];
    int64_t sched_builds = 0;                            // work lists built for this index (a re-plan costs host time: 8 ms at 10 M x 768)
    int xcd_balance = 0;                                 // 0 = automatic (big fp32 searches calibrate the shares from their own workgroups' durations), 1 = equal shares, 2 = as set
    const int* cl_stats_dev = nullptr;                   // {checks, spins, timeouts} of the last clustered launch (in `state`)
    // fp16 candidate mode (use_fp16): fp16 copies of the bank / query fragment tiles, candidate buffers
    int fp16 = HB_FP16_AUTO, dp16 = 0;                    // 0 = the fp32 kernel, 1 = always, 2 = where it pays, HB_FP16_AUTO = the certified screen for big exact searches (hb_screen_choose)
    int fp32_pinned = 0;                                 // sticky: the caller steered the fp32 kernel (variant, tuning, clusters, shares, search options): the automatic state stays on it
    int screen_env_off = 0;                              // HBIRD_EXACT_SCREEN=0 when the index was created
    hb_dev<unsigned> stamp_keep;                          // the candidate launch's stamps, kept aside while nested searches reuse `state`
    // the lazy copies of the bank (hbird_mirror.h), brought up to date by the first search that needs them and told of the bank by bank_changed
    hb_fp16_copy copy16;                                 // the fp16 tiles of the candidate pass, with their mean-centred form (hbird_f16_centre.hip)
    hb_row_copy row_copy;                                // the bank as fp32 rows for the exact re-rank, where memory allows
    int rerank_copy = 0;                                 // 0 = automatic, 1 = always, 2 = never (hb_index_set_rerank_copy)
    int fp16_centre = 0;                                 // the setting: 0 = the plain fp16 copy (default), 1 = centred (hb_index_set_fp16_centre)
    hb_dev<void> q16;
    hb_dev<char> cand;
    hb_dev<float> bmax;                                  // device scalar: max bank-row norm
    hb_dev<char> mtmp;                                   // first-level lists of a two-level merge
    hb_dev<char> fb;                                     // workspace of the uncertified queries (a caller's search) ...
    hb_dev<char> fb1;                                    // ... and of their second fp16 pass
    int fp16_escalation = 0;                             // 0 = on (automatic), 1 = off: uncertified queries go straight to the fp32 kernel (round 5)
    // What the last search of a caller said about itself, and what of `cand`, `fb`, `fb1` and `q16` the read-outs may still hand out
    // (hbird_report.h).  Searches write the report they are handed; it gets here by commit() alone, from the caller-level entries
    // (hb_launch_knn, hb_index_search_excluding), and is told of the bank by bank_changed and of the copy's form by hb_index_set_fp16_centre.
    hb_search_report last;
    int commit(hb_search_report&& r, int rc) { last = rc ? hb_search_report() : std::move(r); return rc; }      // (a failed search: the empty report, every read-out refuses)
    hb_f16_adapt f16_adapt;                              // adaptive use of use_fp16 in mode 2 (hbird_calibrate.h): moving averages of the failing shares
    hb_dev<char> bigk;                                   // workspace of a search with k > 256 (hb_launch_knn_bigk): one pass's lists and the ceilings
    hb_schedule sched_esc; hb_dev<char> sched_esc_dev;   // the nested searches' work list (the caller's stays cached)
    int score_output = 0;                                // 1: searches return ordering scores instead of distances
    int variant = 0;                                     // kernel selection for A/B runs and tests (hb_index_set_variant)
    int phases_on = 1;                                   // pool searches are launched in phases (hb_index_set_search_options)
    const unsigned* wg_stamp_dev = nullptr; int wg_stamp_blocks = 0;   // per-block stamps of the last timed kNN launch (hb_index_wg_stamps, hb_index_kernel_clock)
    long long small_limit = 0;                           // stages per workgroup below which a search counts as small (0 = default)
    double last_knn_ms = 0.0;                            // HIP-event time of the last knn kernel launch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int time_kernels = 0;
    // searches that exclude one row group per query (hb_index_set_row_groups / hb_index_search_excluding, hbird_exclude.hip)
    hb_dev<int32_t> row_groups; int64_t row_groups_n = 0, row_groups_cap = 0;   // device copy of groups[n]; n == 0: no table
    int n_groups = 0; int64_t gmax = 0;                  // ... its group count and the largest group's rows
    hb_dev<char> excl;                                   // workspace of an excluding search: staging, rung 0's lists, flags ...
    hb_dev<char> excl1;                                  // ... and of its rung 1 (sized once the incomplete queries are counted)
    int64_t last_excl[4] = {0, 0, 0, 0};                 // {rungs run, queries sent to rung 1, kf of the last rung run, gmax}
    // ... on the certified fp16 screen (hb_index_set_exclude_screen, hbird_exclude_screen.hip): the re-rank drops the query's group among the candidates
    int excl_screen = 0;                                 // the setting: 0 = the rungs serve every excluding search (default), 1 = the screen where it applies
    int64_t last_excl_screen[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hb_index_last_exclusion_screen's slots
    hb_dev<char> excl_sub;                               // the queries the screen left to the rungs: their rows, groups, query rows and lists
    // The one place that tells the report and the lazy copies: hb_index_add, hb_index_add_from, hb_index_reset and
    // hb_index_reserve each call it once (hbird_capi.hip)
    int bank_changed(hb_bank_event what);
};

void hb_set_error(const std::string& msg);
int hb_fail(const std::string& msg);
#define HB_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t _e = (call);                                                              \
        if (_e != hipSuccess)                                                                \
            return hb_fail(std::string(#call) + ": " + hipGetErrorString(_e));               \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) acts on the CURRENT device only: remembers the (kernel, device)
// pairs already configured (thread-safe), so an index on a second GPU of the same process gets its own call.
int hb_ensure_dyn_lds(const void* kernel, int bytes);

// kernels/launchers (each returns 0 or a negative status after hb_set_error)
int hb_launch_rows_to_tiles(const float* src, int64_t n_rows, int d, int dp, int64_t row0, float* tiles,
                            float* binit, float* bnorm, int metric, int normalize, int is_bank, hipStream_t s);
int hb_launch_scores_to_l2(const float* qn2, int64_t nq, int k, float* dist_inout, hipStream_t s);
int hb_launch_query_aux(const float* q, int64_t nq, int d, float* qn2, float* qnorm, hipStream_t s);
int hb_launch_tiles_to_rows(const float* tiles, int g8, int d, const int64_t* ids, int64_t n, int64_t id_base, int64_t ntotal,
                            float* out, hipStream_t s);
// One search on device pointers, under the hbird:query_tiles / hbird:knn ranges: the queries prepared, the launch (hbird_knn.hip).
// detached == nullptr: a caller's search, which commits its report to the index.  Else the search writes the report and the adaptive fp16
// policy it is handed and leaves the index's alone (the leftover's rungs of an excluding search the screen served).
struct hb_detached { hb_search_report rep; hb_f16_adapt adapt; };
int hb_search_device(hb_index* ix, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist, hb_detached* detached);
int hb_launch_tiles_to_f16(const float* t32, int g8, _Float16* t16, int g16, int64_t n_row_tiles, int64_t rt0, int* overflow,
                           hipStream_t s);
int hb_launch_tiles_to_row_copy(const float* t32, int g8, float* rows, int rs, int64_t n_row_tiles, int64_t rt0, hipStream_t s);
// the exact re-rank of a pass' candidates (hbird_rerank_dev.h: the argument block); rows != nullptr: from the row-major copy [row][rs], else from the tiles
struct hb_rerank_args;
int hb_launch_rerank(const hb_rerank_args& a, const float* tiles, int g8, const float* rows, int rs, hipStream_t s);
int hb_launch_bnorm_max(const float* bnorm, int64_t n, float* bmax, hipStream_t s);
int hb_launch_scatter_rows(const int64_t* rows, int64_t n, int k, const int64_t* src_idx, const float* src_dist,
                           int64_t* out_idx, float* out_dist, hipStream_t s);
struct knn16_args;
int hb_knn_f16_launch(const knn16_args& args, int grid, hipStream_t s);
// label storage: fp32 values, or uint16 counts of values j / P (exactly the fp32 value: K2 computes (float)j / (float)P)
int hb_launch_labels_to_counts(const float* src, int64_t rows, int c, int dst_stride, int P, uint16_t* dst, int* flag, hipStream_t s);
int hb_launch_gather_label_counts(const uint16_t* src, int64_t src_rows, int c, int src_stride, int P, const int64_t* ids, int64_t n, float* out, hipStream_t s);
// (hbird_labels.hip) room for n more label rows of c classes, after the synchronisation a drop needs; the one read-back after the table grew
int hb_labels_ensure(hb_index* ix, int c, int64_t n);
int hb_labels_checked(hb_index* ix);   // 0, or fails when a stored label was not a multiple of 1 / P
// K5 (hbird_aggregate.hip, hbird_grid.hip; device code in hbird_k5_dev.h).  The table one launch reads (hb_k5_table, hbird_labels.h): the
// store's view, and whether the 16-byte gather of count rows applies.  norms_all: the label-sharded form.
int hb_k5_table_choose(const hb_index* ix, int64_t id_base, const float* norms_all, int64_t n_all, const char* who, hb_k5_table* t);
int hb_launch_aggregate(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq,
                        int k, int64_t id_base, float beta, float* out, hipStream_t s, const float* norms_all = nullptr, int64_t n_all = 0);
int hb_launch_merge_parts(const float* dist_parts, const int64_t* idx_parts, int parts, int64_t nq, int k, int metric,
                          int64_t dist_stride, int64_t idx_stride, int64_t* out_idx, float* out_dist, hipStream_t s);
// k beyond 256: K5 for 1 <= k <= HB_MAX_K with hb_launch_aggregate's tables and bits (hbird_aggregate.hip), and the merge of SORTED per-shard lists (hbird_bigk.hip)
int hb_launch_aggregate_bigk(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq,
                             int k, int64_t id_base, float beta, float* out, hipStream_t s, const float* norms_all = nullptr, int64_t n_all = 0);
int hb_launch_merge_sorted_parts(const float* dist_parts, const int64_t* idx_parts, int parts, int64_t nq, int k, int metric,
                                 int64_t dist_stride, int64_t idx_stride, int64_t* out_idx, float* out_dist, hipStream_t s);
// a grid of (k, beta) configurations over one list per query (hbird_grid.hip): cfg = ik * nb + ib; hb_grid_check validates a caller's
// arrays (k_list < 0: the list is a search's own, at ks[nk - 1]) and fills the spec the kernel takes by value
struct hb_grid_spec { int ks[16]; float betas[16]; int nk, nb; };
int hb_grid_check(const char* who, const int* ks, int nk, const float* betas, int nb, int k_list, hb_grid_spec* gs);
int hb_launch_aggregate_grid(const hb_index* ix, const float* qnorm, const int64_t* idx, const float* dist, int64_t nq, int k_list,
                             int64_t id_base, const hb_grid_spec& gs, float* out, hipStream_t s);
// the filter of an excluding search (hbird_exclude.hip); incomplete_opt: a device counter the launch adds its incomplete queries to
int hb_launch_exclude_filter(const int64_t* idx, const float* dist, int64_t nq, int k_list, int64_t id_base, const int32_t* groups, int64_t n_rows,
                             const int32_t* qgroups, int k, float pad, int64_t* out_idx, float* out_dist, int32_t* complete_opt, int32_t* incomplete_opt,
                             hipStream_t s);
// the excluding form of the screen's re-rank, from the fragment tiles, and the gather of the re-searched queries' groups (hbird_exclude_screen.hip)
int hb_launch_excl_screen_rerank(const hb_rerank_args& a, const float* tiles, int g8, const int32_t* groups, int64_t n_group_rows, const int32_t* qgroups,
                                 hipStream_t s);
int hb_launch_gather_groups(const int32_t* src, int64_t n_src, const int64_t* ids, int64_t n, int32_t* out, hipStream_t s);
// One excluding search at k on the screen (hbird_knn.hip): the candidate pass of a plain search at k, the excluding re-rank, the second pass for
// what fails.  What both levels leave uncertified comes back in `left` (ascending query numbers) for the rungs; their output rows hold no result.
// Writes *rep and commits nothing: hb_index_search_excluding does, once the rungs are through.  !rep->took_candidate_pass(): the index's own
// choice for (nq, k) is not the candidate pass -- nothing was searched or written.  A failure commits the empty report.
int hb_launch_knn_excluding(hb_index* ix, const float* q_dev, int64_t nq, int k, int64_t id_base, const int32_t* qgroups, int64_t* out_idx, float* out_dist,
                            hb_search_report* rep);
int hb_launch_patch_label_hist(const int64_t* y, int64_t B, int H, int W, int ps, int C, int map255, float* out,
                               hipStream_t s);
int hb_launch_normalize_rows(const float* x, int64_t n, int d, float* out, hipStream_t s);
int hb_launch_gather_rows(const float* src, int64_t src_rows, int width, const int64_t* ids, int64_t n, float* out,
                          hipStream_t s);
int hb_launch_upsample_argmax(const float* label_hat, int64_t B, int S, int C, int h, int w, int64_t* out,
                              hipStream_t s);
int hb_launch_upsample_argmax_confusion(const float* label_hat, int64_t B, int S, int C, int h, int w, int64_t* out, const int64_t* gt,
                                        int num_gt, int num_pred, int64_t ignore, int has_ignore, unsigned long long* conf, hipStream_t s);
int hb_launch_upsample_accumulate(const float* label_hat, int64_t B, int S, int C, int win_h, int win_w, float* acc, int H,
                                  int W, int y0, int x0, hipStream_t s);
int hb_launch_argmax_channels(const float* acc, int64_t n, int C, int64_t* out, hipStream_t s);
int hb_launch_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int num_gt, int num_pred, int64_t ignore,
                        int has_ignore, unsigned long long* conf, hipStream_t s);
