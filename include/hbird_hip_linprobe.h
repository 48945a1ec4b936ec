/* Part of the C ABI of libhbird_hip.so: the linear probe, a softmax segmentation head fitted on the resident bank (csrc/hbird_linprobe.hip).
 * Included by hbird_hip.h (inside its extern "C" block, after hbird_hip_kmeans.h); not meant to be included on its own.
 *
 * x[r] is a stored bank row (what hb_index_reconstruct returns), y[r][c] its label row as the fp32 value K5 reads (a count j of denominator
 * P: k5_quotient's value, so counts and fp32 tables give the same bits).  Parameters: Wb [C][D + 1] fp32, Wb[c][0] the bias b[c],
 * Wb[c][1 + k] = w[c][k]; 1 <= C <= HB_LINPROBE_MAX_C.
 *
 * Logits, bit-defined.  z[r][c] = the k-ascending fp32 fmaf chain over k = 0 .. D - 1 of x[r][k] * w[c][k], started at b[c] (what
 *   v_mfma_f32_32x32x2_f32 computes with C-in = b[c]; padding dimensions add exact zeros).  A row with a non-finite component is SKIPPED: its
 *   logits are all zeros and it takes no part in the objective.
 * Objective.  s = sum_c y[c], m = max_c z[c], lse = m + log sum_c exp(z[c] - m), p[c] = exp(z[c] - lse); the row loss l = s * lse - sum_c y[c] z[c],
 *   the residual R[c] = fma(s, p[c], -y[c]); all in fp32, exp and log the device's.  n = the rows not skipped.
 *   L = (1 / n) sum_r l[r] + (l2 / 2) sum Wb^2 (the bias is regularised too); sum_r l[r] is a float64 sum by a tree that depends on the row
 *   count alone: thread t of block b (256 x 256) adds its rows (b * 256 + t) + j * 65536 in ascending j, the block's 256 sums meet pairwise,
 *   one block does the same with the 256 partials.  sum Wb^2 is a float64 sum by one such block.
 * Gradient, deterministic.  G[c][0] = (1 / n) sum_r R[r][c] + l2 b[c], G[c][1 + k] = (1 / n) sum_r R[r][c] x[r][k] + l2 w[c][k].
 *   THE SEGMENT RULE: with t = ceil(ntotal / 256), seg_rows = 256 * max(1, ceil(t / HB_LINPROBE_MAX_SEGS)) and nseg = ceil(ntotal / seg_rows):
 *   segment j holds the rows [j * seg_rows, min(ntotal, (j + 1) * seg_rows)) -- a function of ntotal alone, never of the CU count, the
 *   workgroup order or the workspace chunk.  Inside a segment the sum over rows is an fp32 fmaf chain over ascending rows started at 0
 *   (a skipped row adds an exact zero); the segment partials are added in float64 in ascending segment order, the division by n and the l2 term
 *   are float64.  No floating-point atomic: two evaluations return the same bits.
 *
 * hb_linprobe_partition(ntotal, seg_rows, nseg): the segment rule, host only.
 * hb_linprobe_logits(ix, Wb, C, out): z of every row of ANY index (no labels needed) into out [ntotal][C].
 * hb_linprobe_loss_grad(bank, Wb, C, l2, loss_host, grad, used_host, resid_opt): *loss_host = L (HOST), grad [C][D + 1] float64 = G,
 *   *used_host = n (HOST; skipped = ntotal - n), resid_opt [ntotal][C] fp32 = R or NULL.  The bank is read in row chunks of whole segments with
 *   a workspace of at most about HB_LINPROBE_WORKSPACE bytes; every buffer is a local of the call: hb_debug_live_allocations afterwards equals
 *   its value before.  Fails when every row is skipped.
 * hb_linprobe_set_workspace(bytes): a test seam, process-wide like hb_set_layout_form: the workspace of later hb_linprobe_loss_grad calls;
 *   0 restores HB_LINPROBE_WORKSPACE, a negative value is refused.  A chunk is at least one segment whatever the value, and no result depends
 *   on it (the segment rule above).
 *
 * Wb, out, grad, resid_opt are DEVICE pointers on the index's device; work is enqueued on the index's stream, which the entries synchronise.
 * Every entry returns 0, or -1 with hb_last_error set -- before anything is launched for a NULL handle or pointer, C outside
 * [1, HB_LINPROBE_MAX_C] or (loss_grad) different from the label table's class count, a bank without label rows for every row, an empty index. */
#ifndef HBIRD_HIP_LINPROBE_H
#define HBIRD_HIP_LINPROBE_H
#define HB_LINPROBE_MAX_C 256                 /* classes: eight 32-class accumulator tiles per wave */
#define HB_LINPROBE_MAX_SEGS 512              /* gradient segments at the most */
#define HB_LINPROBE_WORKSPACE 1073741824      /* bytes of residual and row staging per chunk, about */
int hb_linprobe_partition(int64_t ntotal, int64_t* seg_rows, int* nseg);
int hb_linprobe_logits(hb_index_t* ix, const float* Wb, int C, float* out);
int hb_linprobe_loss_grad(hb_index_t* bank, const float* Wb, int C, double l2, double* loss_host, double* grad, int64_t* used_host,
                          float* resid_opt);
int hb_linprobe_set_workspace(int64_t bytes);
#endif /* HBIRD_HIP_LINPROBE_H */
