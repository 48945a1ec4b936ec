/* Part of the C ABI of libhbird_hip.so: searches that exclude one group of bank rows per query (csrc/hbird_exclude.hip).
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t is declared); not meant to be included on its own.
 *
 * A bank may carry a ROW-GROUP TABLE groups[ntotal] (int32): a value in [0, n_groups) names the row's group, -1 puts the row in no group.  A
 * call passes qgroups[nq], -1 = "exclude nothing".  hb_index_search_excluding returns, for query i, the exact top-k of the rows with
 * groups[row] != qgroups[i] (rows of group -1 are never excluded): order and tie rule of hb_index_search, ORIGINAL ids (id_base + row), and
 * distances (ordering scores under hb_index_set_score_output) with the bits of hb_index_search on an index that holds only the allowed rows in
 * ascending order; fewer than k allowed rows leave -1 and the search's own missing-neighbour value (-inf / +inf) in the tail.  Leave-one-image-out
 * evaluation of a bank on its own training images is one such search per batch (a group = a dataset image).
 * How: a search returns the exact top-k under one total order (score descending, id ascending) and its score bits do not depend on k, so the best k
 * rows outside a group are the first k non-excluded entries of the best k + gmax rows, gmax = the largest group's size -- bit for bit.  The kNN
 * kernels are hb_index_search's, called at kf = a RUNG; a filter kernel drops the excluded entries of the fetched lists.  need = k + gmax must not
 * exceed HB_MAX_K.  Rungs (hb_exclude_plan_replay): r0 = 256 * ceil((k + min(k, gmax)) / 256); r0 >= need: one rung at need, complete by
 * construction (no flag is read); else [r0, need]: the queries whose rung-0 list holds fewer than k allowed entries and no -1 (the bank is not
 * exhausted) are compacted in ascending order, searched again at need and scattered back -- one stream synchronisation for their count.
 * hb_index_set_row_groups: keeps a device copy of groups[n] and computes gmax (a device histogram, one copy to the host, which synchronises the
 *   stream); NULL or n = 0 clears the table; hb_index_reset clears it too.  n must equal ntotal when a search runs.
 * hb_index_search_excluding: q, qgroups, out_idx, out_dist host or device memory (io_on_device).  A NULL handle or pointer, no table, a table that
 *   does not cover the bank (rows added since), a query group outside [-1, n_groups) and need > HB_MAX_K fail with hb_last_error set before any
 *   search is launched and with nothing written to the outputs (device qgroups are checked by one small launch and a flag read).
 *   hb_last_search_path and the fp16 counters describe the last rung's search.
 * hb_exclude_filter: the filter kernel alone on given lists idx / dist [nq, k_list] (device pointers; rows best-first, as a search leaves them):
 *   entry j of query i survives when idx >= 0 and its row (idx - id_base) lies outside [0, n_rows) -- kept, never dereferenced -- or has
 *   groups[row] != qgroups[i] or qgroups[i] == -1.  The first k survivors go to out_idx / out_dist [nq, k] verbatim and in order, the tail is
 *   -1 / pad.  out_complete[i] (may be NULL) = 1 when the list held at least k survivors or a negative id.  The outputs must not overlap the lists.
 * hb_index_last_exclusion: out = {rungs run, queries sent to rung 1, kf of the last rung run, gmax} of the last excluding search.
 * hb_exclude_plan_replay: the rung rule without a GPU: rungs[0 .. return value) for (k, gmax); negative: bad arguments, or need > HB_MAX_K
 *   (hb_last_error names k, gmax, the limit and the remedy). */
#ifndef HBIRD_HIP_EXCLUDE_H
#define HBIRD_HIP_EXCLUDE_H
int hb_index_set_row_groups(hb_index_t* ix, const int32_t* groups, int64_t n, int32_t n_groups, int on_device);
int hb_index_search_excluding(hb_index_t* ix, const float* q, int64_t nq, int k, int64_t id_base, const int32_t* qgroups,
                              int64_t* out_idx, float* out_dist, int io_on_device);
int hb_exclude_filter(const int64_t* idx, const float* dist, int64_t nq, int k_list, int64_t id_base, const int32_t* groups,
                      int64_t n_rows, const int32_t* qgroups, int k, float pad, int64_t* out_idx, float* out_dist,
                      int32_t* out_complete, void* hip_stream);
int hb_index_last_exclusion(const hb_index_t* ix, int64_t out[4]);
int hb_exclude_plan_replay(int k, int64_t gmax, int* rungs, int max_rungs);
#endif /* HBIRD_HIP_EXCLUDE_H */
