/* Part of the C ABI of libhbird_hip.so: the image-level linear probe, a softmax head fitted on one class id per bank row, for 1000 classes
 * and more (csrc/hbird_linprobe_class.hip).  Included by hbird_hip.h (inside its extern "C" block, after hbird_hip_depth.h); not meant to be
 * included on its own.  Everything that hbird_hip_linprobe.h defines holds here unless stated otherwise; the two differ in the targets (a
 * class id per row here, a label row there) and in the class count (nothing here is sized statically by C).
 *
 * THE DEFINITION IS THIS ENGINE'S OWN: a softmax head with an L2 penalty on L2-normalised features, fitted by full-batch L-BFGS
 * (hbird_mi/linear_probe.py).  It is not DINO's SGD recipe with batch norm.  No dataset is on our machines, and no accuracy of this engine
 * has been held to a published one.
 *
 * x[r] is a stored bank row; Wb [C][D + 1] fp32, Wb[c][0] the bias b[c], Wb[c][1 + k] = w[c][k]; 1 <= C <= HB_LINPROBE_CLASS_MAX_C.  The
 * constant states the largest C accepted and sizes nothing: the forward keeps a workgroup's 256 rows and sweeps the classes in groups of at
 * most eight 32-class tiles.
 *
 * Logits.  Exactly hbird_hip_linprobe.h's: z[r][c] = the k-ascending fp32 fmaf chain over k = 0 .. D - 1 of x[r][k] * w[c][k], started at
 *   b[c], as v_mfma_f32_32x32x2_f32 computes it.  A row with a non-finite component is SKIPPED: its logits are all zeros.
 * Labels.  labels [ntotal] int32 (DEVICE): labels[r] lies in [0, C), or is -1.  A row with label -1 is SKIPPED like a non-finite row: its
 *   residuals are zero, it adds no loss and it is not counted in n.  A label outside [-1, C) is refused through one small flag launch and a
 *   read of the flag before anything else runs (as hb_vote_counts does), with the outputs untouched.
 * Objective, fp32.  y = labels[r].  m = max_c z[c].  Lane i (the classes c = i mod 32) adds expf(z[c] - m) over its classes in ascending c,
 *   starting at 0; the 32 lane sums meet in the ds_swizzle butterfly of lp_half_sum, in the order 16, 8, 4, 2, 1: se.  lse = m + logf(se).
 *   The row loss l = lse - z[y]; the residual R[c] = expf(z[c] - lse) - [c == y], one rounding.  This is hbird_hip_linprobe.h's arithmetic
 *   with s = 1 and a one-hot label row, for any number of class tiles: the bits do not depend on how many classes the forward sweeps at a
 *   time, and for C <= HB_LINPROBE_MAX_C they equal those of hb_linprobe_loss_grad on the one-hot label table.
 *   L = (1 / n) sum_r l[r] + (l2 / 2) sum Wb^2 (the bias is regularised too); sum_r l[r] is a float64 sum by a tree that depends on the row
 *   count alone: thread t of block b (256 x 256) adds its rows (b * 256 + t) + j * 65536 in ascending j, the block's 256 sums meet pairwise,
 *   one block does the same with the 256 partials.  sum Wb^2 is a float64 sum by one such block.
 * Gradient, deterministic.  G[c][0] = (1 / n) sum_r R[r][c] + l2 b[c], G[c][1 + k] = (1 / n) sum_r R[r][c] x[r][k] + l2 w[c][k].
 *   THE SEGMENT RULE: with t = ceil(ntotal / 256), seg_rows = 256 * max(1, ceil(t / HB_LINPROBE_MAX_SEGS)) and nseg = ceil(ntotal / seg_rows):
 *   segment j holds the rows [j * seg_rows, min(ntotal, (j + 1) * seg_rows)) -- a function of ntotal alone, never of the CU count, the
 *   workgroup order or the workspace chunk.  Inside a segment the sum over rows is an fp32 fmaf chain over ascending rows started at 0
 *   (a skipped row adds an exact zero); the segment partials are added in float64 in ascending segment order, the division by n and the l2 term
 *   are float64.  No floating-point atomic: two evaluations return the same bits.  hb_linprobe_partition is the rule.
 *
 * hb_linprobe_class_logits(ix, Wb, C, out): z of every row of ANY index into out [ntotal][C].
 * hb_linprobe_class_loss_grad(bank, labels, Wb, C, l2, loss_host, grad, used_host, resid_opt): *loss_host = L (HOST), grad [C][D + 1] float64
 *   = G, *used_host = n (HOST; skipped = ntotal - n), resid_opt [ntotal][C] fp32 = R or NULL.  The bank needs no label table.  It is read in
 *   row chunks of whole segments of seg_rows * (cp + xs) * 4 bytes (cp = 32 ceil(C / 32), xs = 32 ceil((D + 1) / 32)) with a workspace of at
 *   most about HB_LINPROBE_WORKSPACE bytes; hb_linprobe_set_workspace is the shared test seam, a chunk is at least one segment, and no output
 *   depends on it.  Every buffer is a local of the call: hb_debug_live_allocations afterwards equals its value before.  Fails when every row
 *   is skipped.
 * hb_logits_topn(logits, nq, C, topn, pred, hip_stream): logits [nq][C] fp32 -> pred [nq][topn] int32.  Classes rank by logit descending,
 *   ties to the LOWER class id; a NaN logit ranks below every number and is never written.  The first topn <= HB_VOTE_MAX_TOP (8) classes
 *   are written; the tail holds -1, both when C < topn and when fewer than topn logits are numbers.  nq == 0 is an empty call and returns
 *   0.  Work is enqueued on hip_stream (NULL: the default stream) and not waited for; no index is involved.
 *
 * labels, Wb, out, grad, resid_opt, logits, pred are DEVICE pointers; the two index entries enqueue on the index's stream and synchronise it.
 * Every entry returns 0, or -1 with hb_last_error set -- before anything is launched, with outputs untouched and hb_debug_live_allocations
 * unchanged, for a NULL handle or pointer, C outside [1, HB_LINPROBE_CLASS_MAX_C], an empty index, topn outside [1, 8], nq < 0. */
#ifndef HBIRD_HIP_LINPROBE_CLASS_H
#define HBIRD_HIP_LINPROBE_CLASS_H
#define HB_LINPROBE_CLASS_MAX_C 16384         /* the largest C accepted; nothing is sized by it */
int hb_linprobe_class_logits(hb_index_t* ix, const float* Wb, int C, float* out);
int hb_linprobe_class_loss_grad(hb_index_t* bank, const int32_t* labels, const float* Wb, int C, double l2, double* loss_host, double* grad,
                                int64_t* used_host, float* resid_opt);
int hb_logits_topn(const float* logits, int64_t nq, int C, int topn, int32_t* pred, void* hip_stream);
#endif /* HBIRD_HIP_LINPROBE_CLASS_H */
