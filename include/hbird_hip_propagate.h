/* Part of the C ABI of libhbird_hip.so: video label propagation (csrc/hbird_propagate.hip, csrc/hbird_maskmetrics.hip) -- windowed retrieval
 * over a pool of context frames, the label map of a rectangular frame, and the integer counts behind the region (J) and boundary (F) measures
 * of semi-supervised video object segmentation.
 * Stands on its own (no hb_index_t): hbird_hip.h does not include it, hbird_mi/_lib.py binds it as SIGNATURES_PROPAGATE.
 * All pointers are device pointers except where noted, work is enqueued on `hip_stream` (NULL: the default stream).  Each entry returns 0, or
 * -1 with hb_last_error set before anything is launched: for a NULL pointer, a non-positive size, a limit exceeded, d % 4 != 0, a
 * temperature that is <= 0 or not finite, a slot outside [0, pool_slots), a pointer that is not 16-byte aligned (q, feat_pool).
 *
 * THE DEFINITIONS BELOW ARE THIS ENGINE'S OWN.  They follow DINO's eval_video_segmentation.py and the DAVIS-2017 toolkit as restated from
 * memory; no J&F figure of this engine has been held to a published one.
 *
 * hb_propagate_labels.  N = gh * gw, cells row-major (cell = y * gw + x).  q [N, d] fp32 holds the target frame's tokens,
 *   feat_pool [pool_slots, N, d] and label_pool [pool_slots, N, c] are fp32.  Rows are expected L2-normalised by the caller
 *   (hb_normalize_rows); the entry does not normalise.  slots and radii are HOST int[n_ctx]: they are read before the call returns and passed
 *   by value into the launch.  Context position f reads pool slot slots[f]; radii[f] < 0 means unrestricted.
 *   Candidates of query cell (y, x): for f = 0 .. n_ctx - 1, every cell (y', x') with radii[f] < 0, or with |y' - y| <= radii[f] and
 *   |x' - x| <= radii[f] (a square window clipped to the grid, as DINO's restrict_neighborhood).  Candidate id = f * N + cell'.
 *   Score: the project's chain, acc = fmaf(q[dd], b[dd], acc) for dd ascending from 0.0f -- what v_mfma_f32_32x32x2_f32 computes.
 *   A NaN score is never a neighbour (nor is a score of -inf: the list's padding value).
 *   List: the up-to-k best candidates, in descending score, ties by ascending id; positions past the candidate count hold idx -1 and
 *   score -inf.  out_idx_opt [N, k] int64, out_score_opt [N, k] fp32: both or neither.
 *   Aggregation over the list, j ascending: logit_j = s_j / temperature (IEEE fp32 division); mx = logit_0; e_j = expf(logit_j - mx);
 *   den = ((0.0f + e_0) + e_1) + ...; w_j = e_j / den; out_labels[i][ch] is one fmaf(w_j, label[id_j][ch], acc) chain from 0.0f, where
 *   label[f * N + cell'] is row cell' of pool slot slots[f].  An empty list gives a row of zeros.  out_labels [N, c] fp32.
 *   Limits: k <= HB_PROPAGATE_MAX_K, n_ctx <= HB_PROPAGATE_MAX_CTX, c <= HB_PROPAGATE_MAX_C, d <= HB_PROPAGATE_MAX_D (a workgroup stages its 32
 *   queries' tokens in LDS: 128 KiB at d = 1024, beside 32 KiB of lists), n_ctx * N < 2^31.
 *   No floating-point atomic: two calls return the same bits.
 *
 * hb_mask_upsample_argmax.  labels [B, gh * gw, c] fp32 -> out [B, h, w] int64.  Per axis the source-index arithmetic of hbird_hip_depth.h
 *   (scale = (float)G / (float)n, f = max(scale * ((float)dst + 0.5f) - 0.5f, 0), i0 = min((int)floor(f), G - 1), i1 = min(i0 + 1, G - 1),
 *   l1 = f - (float)i0, l0 = 1 - l1: align_corners = False), gh in the role of G for rows, gw for columns, and K6's four-tap order
 *   ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11), in fp32 without contraction.
 *   With channel_norm != 0 (DINO's norm_mask), for every (b, channel) take mn and mx of the upsampled values over all h * w pixels; where
 *   mx > 0 and mx > mn the value becomes (v - mn) / (mx - mn) (fp32 subtractions, IEEE division), otherwise the channel is unchanged.
 *   Argmax: first maximum wins (lowest channel), as in K6.  c <= HB_PROPAGATE_MAX_C.  The channel-norm form keeps the extrema in a workspace
 *   local to the call and synchronises the stream before it returns.
 *
 * hb_mask_jf_counts.  pred, gt [B, h, w] int64 -> counts_out [B, n_objects, HB_JF_NCOUNTS] int64.  For object o = 1 .. n_objects, with
 *   P = (pred == o) and G = (gt == o): HB_JF_INTER = |P & G|, HB_JF_UNION = |P | G|.
 *   Boundary map bmap(M), the toolkit's seg2bmap at equal size: b = (M ^ E) | (M ^ S) | (M ^ SE), with E[y][x] = M[y][x + 1],
 *   S[y][x] = M[y + 1][x], SE[y][x] = M[y + 1][x + 1]; in the last row b = M ^ E; in the last column b = M ^ S; the bottom-right pixel is 0.
 *   HB_JF_NFG = |bmap(P)|, HB_JF_NGT = |bmap(G)|, HB_JF_FG_MATCH = |bmap(P) & dil(bmap(G))|, HB_JF_GT_MATCH = |bmap(G) & dil(bmap(P))|;
 *   dil is dilation by the disk dy^2 + dx^2 <= bound_px^2.  0 <= bound_px <= HB_JF_MAX_BOUND.  The counts are added with integer atomics:
 *   they are the same every call.
 *   The host computes, in float64: bound_px = ceil(0.008 * hypot(h, w)); J = inter / union, and 1 where the union is 0; precision
 *   = FG_MATCH / NFG and recall = GT_MATCH / NGT with the toolkit's empty cases (NFG = 0 and NGT > 0: precision 1, recall 0; NFG > 0 and
 *   NGT = 0: precision 0, recall 1; both 0: precision 1, recall 1); F = 2 p r / (p + r), and 0 where p + r = 0. */
#ifndef HBIRD_HIP_PROPAGATE_H
#define HBIRD_HIP_PROPAGATE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define HB_PROPAGATE_MAX_K 32
#define HB_PROPAGATE_MAX_CTX 32
#define HB_PROPAGATE_MAX_C 64
#define HB_PROPAGATE_MAX_D 1024
#define HB_JF_MAX_BOUND 32
#define HB_JF_INTER 0
#define HB_JF_UNION 1
#define HB_JF_NFG 2
#define HB_JF_NGT 3
#define HB_JF_FG_MATCH 4
#define HB_JF_GT_MATCH 5
#define HB_JF_NCOUNTS 6
int hb_propagate_labels(const float* q, const float* feat_pool, const float* label_pool, int pool_slots, const int* slots, const int* radii,
                        int n_ctx, int gh, int gw, int d, int c, int k, float temperature, float* out_labels, int64_t* out_idx_opt,
                        float* out_score_opt, void* hip_stream);
int hb_mask_upsample_argmax(const float* labels, int64_t B, int gh, int gw, int c, int h, int w, int channel_norm, int64_t* out,
                            void* hip_stream);
int hb_mask_jf_counts(const int64_t* pred, const int64_t* gt, int64_t B, int h, int w, int n_objects, int bound_px, int64_t* counts_out,
                      void* hip_stream);
#ifdef __cplusplus
}
#endif
#endif /* HBIRD_HIP_PROPAGATE_H */
