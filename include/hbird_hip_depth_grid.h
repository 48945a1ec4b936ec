/* Part of the C ABI of libhbird_hip.so: depth grids (csrc/hbird_depth_grid.hip) -- the depth metrics of a whole grid of (k, beta)
 * configurations out of one call, and the resampling reduction of a paired bootstrap over float64 per-image sums.
 * Stands on its own (no hb_index_t): hbird_hip.h does not include it, hbird_mi/_lib.py binds it as SIGNATURES_DEPTH_GRID.
 * Every pointer is a device pointer, every call enqueues on `stream` (NULL: the default stream) and returns 0, or -1 with hb_last_error set
 * before anything is launched.  HB_DEPTH_NSUMS (11), the slots HB_DEPTH_SUM_*, HB_DEPTH_MAX_GRID and the words "valid", "prediction" and
 * "THE SUMMATION RULE" are those of hbird_hip_depth.h; HB_BOOTSTRAP_MAX_IMAGES and HB_BOOTSTRAP_MAX_REPLICATES those of hbird_hip_bootstrap.h.
 *
 * hb_depth_upsample_metrics_grid.  agg [n_cfg][B][S * S][2 r^2] fp32 is the layout hb_index_search_aggregate_grid writes on a depth bank
 *   (every configuration a contiguous [B * S * S, 2 r^2] slab), gt [B][h][w] fp32, sums_out [n_cfg][B][HB_DEPTH_NSUMS] float64, pred_out_opt
 *   [n_cfg][B][h][w] fp32 or NULL, 1 <= n_cfg <= HB_DEPTH_GRID_MAX_CONFIGS.
 *   DEFINITION: slab c of sums_out and of pred_out_opt has the bits of hb_depth_upsample_metrics(agg + c * B * S * S * 2 r^2, B, S, r, h, w,
 *   gt, min_depth, max_depth, sums_out + c * B * HB_DEPTH_NSUMS, pred_out_opt + c * B * h * w): the same prediction arithmetic (the ratio of
 *   the two bilinearly upsampled grids, fp32, step by step, no contraction, clamped), the same float64 terms, THE SUMMATION RULE of
 *   hbird_hip_depth.h (a function of (h, w) alone: never of n_cfg, of B or of the launch geometry) and the same quiet NaN 0x7FC00000 in the
 *   map where Dn <= 0.
 *   What does not depend on the configuration is done once per call: one launch of the metric kernel and one of the row pass, one workspace
 *   (the per-row partials, [n_cfg][B][h][NB][HB_DEPTH_NSUMS] float64, a local of the call: hb_debug_live_allocations afterwards equals its
 *   value before) and one stream synchronisation before the call returns.
 *   Refused: n_cfg outside [1, HB_DEPTH_GRID_MAX_CONFIGS]; everything hb_depth_upsample_metrics refuses, with that entry's words (B < 0, a
 *   non-positive S, r, h or w, S r > HB_DEPTH_MAX_GRID, bounds that are not 0 < min_depth <= max_depth < inf, a NULL agg, gt or sums_out);
 *   a launch grid that would not fit (S r x the row chunks of the tallest band, or B, beyond 65535; one configuration's staged rows and
 *   wave partials beyond 64 KiB of LDS: a column chunk's window of more than some 4,070 cells, i.e. S r near its limit under a more than
 *   16-fold horizontal downsampling).  B == 0 is an empty call: 0.
 *
 * hb_bootstrap_weighted_sums.  table [n_img][cols] float64, image-major; W [R][n_img] int32 -- rows of hb_bootstrap_multiplicities, so that
 *   the replicates pair with those of hb_bootstrap_miou for the same (seed, n_img); out [R][cols] float64.
 *   DEFINITION: out[r][col] is the chain acc = 0.0; for i = 0 .. n_img - 1 ascending: acc = acc + (double)W[r][i] * table[i][col] -- the
 *   product is rounded to float64 first and then added (no contraction), there is no floating-point atomic: the result is a function of the
 *   inputs alone, not of the launch geometry and not of how a caller cuts R into passes.  Non-finite table values propagate as IEEE
 *   arithmetic says (0 * inf is NaN).
 *   1 <= n_img <= HB_BOOTSTRAP_MAX_IMAGES, 0 <= R <= HB_BOOTSTRAP_MAX_REPLICATES, cols >= 1; R == 0 is an empty call: 0. */
#ifndef HBIRD_HIP_DEPTH_GRID_H
#define HBIRD_HIP_DEPTH_GRID_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define HB_DEPTH_GRID_MAX_CONFIGS 16          /* the value of HB_GRID_MAX_CONFIGS: one aggregation launch's configurations */
int hb_depth_upsample_metrics_grid(const float* agg, int n_cfg, int64_t B, int S, int r, int h, int w, const float* gt, float min_depth,
                                   float max_depth, double* sums_out, float* pred_out_opt, void* stream);
int hb_bootstrap_weighted_sums(const double* table, int64_t n_img, int64_t cols, const int32_t* W, int64_t R, double* out, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* HBIRD_HIP_DEPTH_GRID_H */
