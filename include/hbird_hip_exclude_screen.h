/* Part of the C ABI of libhbird_hip.so: excluding searches (hbird_hip_exclude.h) served by the certified fp16 screen (csrc/hbird_exclude_screen.hip).
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t is declared); not meant to be included on its own.
 *
 * The rungs of hb_index_search_excluding search at kf = k + gmax: beyond 128 that is the fp32 kernel, beyond 256 several passes of it.  The
 * screen's certificate, however, is a statement about the rows OUTSIDE a query's k' candidates (exact score <= the k'-th pass score + E) and
 * says nothing about which candidates are allowed: with the query's group dropped among the candidates, an exact k-th best of the remaining
 * ones strictly above that bound makes the list the excluding search's answer, bit for bit.  With the route on, an excluding search costs a
 * plain search at k; queries that fail take the screen's second pass (k' = 256, seeded floors) with their groups, and what fails again is
 * handed to the rungs -- on those queries only.  Results are those of the route off in ids and distance bits.
 *
 * hb_index_set_exclude_screen(ix, on): 0 (default) leaves every excluding search on the rungs; 1 lets the screen serve it when k <= 128,
 *   k + gmax > 128 (below that the single rung is on the screen already and complete by construction), the index's own choice for a plain
 *   search of these queries at k is the candidate pass (hb_index_set_fp16 1, 2 or the automatic state; the adaptive policy's "fp32 right away"
 *   counts as no), nq > 0 and ntotal > 0.  Otherwise the rungs serve the search exactly as with the route off.
 * hb_index_last_exclusion_screen(ix, out): of the last excluding search
 *     out[0] served by the route (0 / 1)            out[4] queries sent to the second pass
 *     out[1] reason when not served (HB_EXCL_SCREEN_*)  out[5] queries certified at the second pass
 *     out[2] kc of level 0                          out[6] queries sent to the rungs
 *     out[3] queries certified at level 0           out[7] centred (0 / 1)
 *   On a served search hb_index_last_exclusion's rungs / rung-1 queries / kf describe the leftover's rung run (0 / 0 / 0: nothing was left over);
 *   hb_last_search_path describes the level-0 pass.  A served search does not feed the adaptive fp16 policy.
 * hb_index_exclude_rerank: the excluding re-rank kernel alone, in its plain (not centred) form, on the caller's lists -- cand_rows and
 *   pass_scores [nq][kc] as hb_index_last_screen hands them out (best pass score first, -1 / -inf: no entry) --, with the index's tiles,
 *   norms, largest row norm and group table.  Candidate c of query i is excluded when row >= 0, qgroups[i] >= 0 and groups[row] == qgroups[i];
 *   a row at or beyond ntotal counts as no entry.  out_idx / out_dist [nq][k]: the best k allowed candidates by exact score (ids + id_base,
 *   distances as hb_index_search gives them), -1 and the missing value in the tail; out_certified[nq]: 1 where the k-th allowed exact score
 *   lies strictly above pass_scores[i][kc - 1] + E (or the list ends in -1 and the bank holds fewer than kc rows); out_kth / out_floor [nq]
 *   (each may be NULL): the k-th allowed exact score and that score - 1.001 E, -inf where fewer than k candidates are allowed.  All pointers
 *   are DEVICE pointers.  Runs on the index's stream and synchronises it.  Refuses, before any launch and with hb_last_error set: a NULL handle
 *   or pointer, a missing table or one that does not cover the bank, kc outside [k, 256] or not a multiple of 8, k < 1.
 * hb_index_last_exclusion_seeds(ix, groups1, left, capacity_queries1, capacity_left, info): what a served excluding search handed on besides the
 *   values of hb_index_last_screen_seeds (hbird_hip_screen.h, which states their meaning for an excluding search) -- a group gathered for the wrong
 *   query, or a failing query that never reaches the rungs, shows in no certificate:
 *     info        {n1: queries of the second pass, 0 when none ran; n_left: queries handed to the rungs}
 *     groups1[n1] the second pass' query groups as gathered on the device, in the order of hb_index_last_screen_seeds' queries1 (not recomputed)
 *     left[n_left] the level-0 query numbers handed to the rungs, ascending: what failed the second pass, or level 0 where none ran
 *   HOST pointers, each may be NULL; a first call with both NULL returns the sizes.  Synchronises the index's stream; launches nothing.
 *   Fails (hb_last_error says which) on a NULL handle or a NULL info; when the last search of a caller was not an excluding one that the screen
 *   served, when hb_index_reset, hb_index_add or a capacity change came after it, or when one of the leftover's rungs took the candidate pass
 *   itself; when a capacity is smaller than the count it stands for. */
#ifndef HBIRD_HIP_EXCLUDE_SCREEN_H
#define HBIRD_HIP_EXCLUDE_SCREEN_H
#define HB_EXCL_SCREEN_SERVED 0      /* reason codes of hb_index_last_exclusion_screen's out[1] */
#define HB_EXCL_SCREEN_OFF 1         /* the route is switched off */
#define HB_EXCL_SCREEN_K 2           /* k > 128 */
#define HB_EXCL_SCREEN_NEED 3        /* k + gmax <= 128: the single rung is on the screen already */
#define HB_EXCL_SCREEN_PATH 4        /* the index's own choice for (nq, k) is the fp32 kernel */
#define HB_EXCL_SCREEN_EMPTY 5       /* no queries, or an empty bank */
int hb_index_set_exclude_screen(hb_index_t* ix, int on);
int hb_index_last_exclusion_screen(const hb_index_t* ix, int64_t out[8]);
int hb_index_exclude_rerank(hb_index_t* ix, const float* q, int64_t nq, const int64_t* cand_rows, const float* pass_scores, int kc,
                            const int32_t* qgroups, int k, int64_t id_base, int64_t* out_idx, float* out_dist,
                            unsigned char* out_certified, float* out_kth, float* out_floor);
int hb_index_last_exclusion_seeds(hb_index_t* ix, int32_t* groups1, int64_t* left, int64_t capacity_queries1, int64_t capacity_left, int64_t info[2]);
#endif /* HBIRD_HIP_EXCLUDE_SCREEN_H */
