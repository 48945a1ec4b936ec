/* Part of the C ABI of libhbird_hip.so: sub-bank views (csrc/hbird_select.hip).
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t is declared); not meant to be included on its own.
 *
 * An index out of selected rows of another index of the same d, metric and device, gathered on the
 * device tile to tile.  The bounded build keeps per (epoch, image) the K = max(1, memory_size // (dataset_size * augmentation_epoch)) patches
 * with the smallest noisy scores (hbird_eval.py:146-147) in ascending order, ties to the lower patch index, and the noise does not depend on K
 * (hbird_eval.py:497-511): the bank of a smaller memory_size is the first K' rows of every block of K rows of a bigger one, bit for bit, and an
 * image subset of an unbounded bank is those images' rows.  So a memory-size or data-efficiency sweep needs ONE bank build.
 * hb_index_add_from appends rows ids[0..n) of src, in that order (duplicates allowed), to dst: tiles, accumulator-init values and norms are
 * copied verbatim (nothing is recomputed: also NaN rows and the L2 constants come over as they are), the max row norm is updated as by
 * hb_index_add, capacity grows as hb_index_add grows it.  When src holds label rows they come along in their stored form (then every id must be
 * < src's nlabels and dst's nlabels == ntotal; an empty dst adopts src's class count and label denominator, a non-empty one must have the
 * same); borrowed tables (hb_index_set_label_table) are not followed.  Every id must lie in [0, src ntotal): checked on the device BEFORE
 * anything is written, so a failing call leaves dst exactly as it was (one stream synchronisation per call).  src == dst is refused.  The work
 * is queued on dst's stream behind what src's stream holds at the call; src must not be freed, reset or grown until that work is done.
 * hb_index_select_rows = hb_index_create on src's device + hb_index_reserve for n rows + hb_index_add_from: a NEW index (automatic fp16 state, own
 * calibration and workspace; it starts on src's stream) that takes only the class count and the label denominator from src. */
#ifndef HBIRD_HIP_SELECT_H
#define HBIRD_HIP_SELECT_H
int hb_index_add_from(hb_index_t* dst, const hb_index_t* src, const int64_t* ids, int64_t n, int ids_on_device);
int hb_index_select_rows(const hb_index_t* src, const int64_t* ids, int64_t n, int ids_on_device, hb_index_t** out);
#endif /* HBIRD_HIP_SELECT_H */
