/* Part of the C ABI of libhbird_hip.so: depth estimation by retrieval (csrc/hbird_depth.hip) -- the bank's label rows hold a patch's local
 * depth values instead of class frequencies, the aggregated rows become a depth map and per-image error sums.
 * Included by hbird_hip.h (inside its extern "C" block, after hbird_hip_linprobe.h); not meant to be included on its own.
 *
 * Valid depth.  A value v (fp32, metres) is valid iff it is finite and min_depth <= v <= max_depth (defaults HB_DEPTH_MIN_DEFAULT, HB_DEPTH_MAX_DEFAULT).
 *   Both entries want finite bounds with 0 < min_depth <= max_depth (the metrics take logarithms of clamped predictions).
 *
 * Target rows (hb_patch_depth_targets).  y [B, H, W] fp32, H and W multiples of ps; target_grid r divides ps, the cell side is s = ps / r.
 *   The row of patch (b, py, px) has HB_DEPTH_CHANNELS(r) = 2 r^2 channels, cell-major (cy, cx):
 *     num[cell] = the fp32 sum of the cell's valid values, added in row-major pixel order starting from 0.0f with plain adds (no contraction,
 *                 an invalid pixel adds nothing), then divided by (float)(s * s);
 *     den[cell] = (float)valid_count / (float)(s * s).
 *   Channels [0, r^2) hold num (HB_DEPTH_NUM_CHANNEL), channels [r^2, 2 r^2) hold den (HB_DEPTH_DEN_CHANNEL).
 *   rows_out [B, H / ps, W / ps, 2 r^2] fp32; nonempty_out [B, H / ps, W / ps] int32 = 1 iff any pixel of the patch is valid (the form
 *   hb_patch_select takes).  ps <= HB_DEPTH_MAX_PS.  The rows go into an index as fp32 label rows (hb_index_set_label_denominator(ix, 0)).
 *
 * Prediction (hb_depth_upsample_metrics).  agg [B, S * S, 2 r^2] is what hb_index_search_aggregate returns on such a bank.  The cell grids
 *   Ngrid and Dgrid are [S r, S r] with gy = py * r + cy, gx = px * r + cx.  Both are upsampled to (h, w) with the bilinear arithmetic of
 *   hb_upsample_argmax (csrc/hbird_post.hip), step by step in fp32 and without contraction: scale = (float)(S r) / (float)h,
 *   f = max(scale * ((float)dst + 0.5f) - 0.5f, 0), i0 = min((int)floor(f), S r - 1), i1 = min(i0 + 1, S r - 1), l1 = f - (float)i0, l0 = 1 - l1
 *   (ATen's area_pixel_compute_source_index, align_corners = False), value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11).
 *   That gives N and Dn: a ratio of bilinears, not a bilinear of ratios.  Where Dn > 0:
 *   pred = fminf(fmaxf(N / Dn, min_depth), max_depth) (IEEE fp32 division).  Elsewhere the pixel has NO prediction; pred_out_opt
 *   [B, h, w] fp32 (or NULL) holds the quiet NaN 0x7FC00000 there.  S r <= HB_DEPTH_MAX_GRID.
 *
 * Sums.  gt [B, h, w] fp32.  For every image, over the pixels whose ground truth g is valid: HB_DEPTH_SUM_NOPRED counts those with Dn <= 0; over
 *   the rest, with p = pred and g promoted to float64 (plain float64 operations, no contraction, log and log10 the device's):
 *     HB_DEPTH_SUM_N        the pixel count n           HB_DEPTH_SUM_SQ       sum (p - g)^2           HB_DEPTH_SUM_ABS_REL  sum |p - g| / g
 *     HB_DEPTH_SUM_SQ_REL   sum (p - g)^2 / g           HB_DEPTH_SUM_LOG_SQ   sum (ln p - ln g)^2     HB_DEPTH_SUM_LOG      sum (ln p - ln g)
 *     HB_DEPTH_SUM_LOG10    sum |log10 p - log10 g|     HB_DEPTH_SUM_D1 / _D2 / _D3   the counts of max(p / g, g / p) < 1.25, 1.25^2, 1.25^3
 *   sums_out [B][HB_DEPTH_NSUMS] float64 (the counts are exact integers in float64).
 *   THE SUMMATION RULE, a function of (h, w) alone -- never of the CU count, the launch geometry or B.  With W64 = ceil(w / 64),
 *   NB = ceil(W64 / 4) and CW = 64 * ceil(W64 / NB), an output row is cut into NB column chunks of CW columns (the last one shorter), a
 *   chunk into groups of 64 neighbouring columns.  A group's 64 terms (0.0 past column w - 1 and for a pixel that does not take part) meet in
 *   the xor butterfly: t[l] += t[l ^ 32], then ^ 16, 8, 4, 2, 1.  A chunk's groups are added in ascending order starting from the first, the
 *   row's chunks are added in ascending order starting from 0.0, and the image's rows are added in ascending order starting from 0.0:
 *   acc = acc + row.  No floating-point atomic: two calls return the same bits, and an image's sums do not depend on the images beside it.
 *
 * y, rows_out, nonempty_out, agg, gt, sums_out, pred_out_opt are DEVICE pointers; work is enqueued on hip_stream.  hb_depth_upsample_metrics
 * synchronises the stream before it returns: its workspace (the per-row partials, [B, h, NB, HB_DEPTH_NSUMS] float64) is a local of the
 * call, and hb_debug_live_allocations afterwards equals its value before.
 * Both entries return 0, or -1 with hb_last_error set -- before anything is launched for a NULL pointer, r not dividing ps, H or W not a
 * multiple of ps, a non-positive size (B == 0 is an empty call: 0), bounds that are not 0 < min_depth <= max_depth < inf, ps or S r beyond
 * their limits. */
#ifndef HBIRD_HIP_DEPTH_H
#define HBIRD_HIP_DEPTH_H
#define HB_DEPTH_MIN_DEFAULT 1e-3f
#define HB_DEPTH_MAX_DEFAULT 10.0f
#define HB_DEPTH_MAX_PS 64                    /* pixels per patch side: four staged patches of a workgroup within 64 KiB of LDS */
#define HB_DEPTH_MAX_GRID 4096                /* cells per grid side (S r): two staged rows of both grids within 64 KiB of LDS */
#define HB_DEPTH_CHANNELS(r) (2 * (r) * (r))
#define HB_DEPTH_NUM_CHANNEL(r, cy, cx) ((cy) * (r) + (cx))
#define HB_DEPTH_DEN_CHANNEL(r, cy, cx) ((r) * (r) + (cy) * (r) + (cx))
#define HB_DEPTH_SUM_N 0
#define HB_DEPTH_SUM_NOPRED 1
#define HB_DEPTH_SUM_SQ 2
#define HB_DEPTH_SUM_ABS_REL 3
#define HB_DEPTH_SUM_SQ_REL 4
#define HB_DEPTH_SUM_LOG_SQ 5
#define HB_DEPTH_SUM_LOG 6
#define HB_DEPTH_SUM_LOG10 7
#define HB_DEPTH_SUM_D1 8
#define HB_DEPTH_SUM_D2 9
#define HB_DEPTH_SUM_D3 10
#define HB_DEPTH_NSUMS 11
int hb_patch_depth_targets(const float* y, int64_t B, int H, int W, int ps, int r, float min_depth, float max_depth, float* rows_out,
                           int* nonempty_out, void* hip_stream);
int hb_depth_upsample_metrics(const float* agg, int64_t B, int S, int r, int h, int w, const float* gt, float min_depth, float max_depth,
                              double* sums_out, float* pred_out_opt, void* hip_stream);
#endif /* HBIRD_HIP_DEPTH_H */
