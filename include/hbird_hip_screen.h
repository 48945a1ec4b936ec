/* Part of the C ABI of libhbird_hip.so: a read-out of what the certified fp16 screen's candidate pass left behind, for tests of that pass.
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t is declared); not meant to be included on its own.
 *
 * A screened search (hb_index_set_fp16) answers with the fp32 search's bits whatever its candidate kernel delivers: a query whose certificate
 * fails is searched again.  So a candidate kernel that loses rows or mis-scores them shows in no result, only in time.  The certificate itself
 * rests on two statements about the pass: every candidate's pass score lies within E of its exact score, and no row outside a
 * query's k' candidates has a pass score above the k'-th candidate's.  This entry hands out the pass' own output so that both can be checked.
 *
 * hb_index_last_screen(ix, cand_rows, pass_scores, certified, capacity_queries, info): of the LEVEL-0 candidate pass of the last search of a
 *   caller (not of the second pass over uncertified queries), after the merge of the partial pools:
 *     cand_rows[nq][kc]    bank rows (without id_base), best pass score first, ties by lower row; -1: no entry (fewer than kc rows scored)
 *     pass_scores[nq][kc]  the candidate kernel's own scores, in the pass' units: q16.b16 + row init (L2: -|b|^2 / 2); the centred form
 *                          (hb_index_set_fp16_centre) lacks the query's constant c_q = q.mu; -inf where cand_rows is -1
 *     certified[nq]        1: the first certificate held; 0: the query was searched again
 *     info                 {nq, kc, centred (0 / 1), klw: the pools' capacity per query and slot}
 *   All four are HOST pointers; cand_rows, pass_scores and certified may each be NULL (all three NULL: info only).  capacity_queries: the
 *   queries the arrays have room for.  Synchronises the index's stream; launches nothing.
 *   Fails (hb_last_error says which) on a NULL handle; when the last search did not take the fp16 candidate pass, or hb_index_reset,
 *   hb_index_add or a capacity change came after it; when that search ran its second fp16 pass, which reuses the buffers
 *   (hb_index_set_fp16_escalation(ix, 1) keeps them); when capacity_queries is smaller than the search's query count.
 *
 * hb_index_last_screen_seeds(ix, kth0, floor0, certified0, queries1, seed1, cand_rows1, pass_scores1, certified1, kth1, capacity_queries,
 *   capacity_queries1, info): what the chain BEHIND the first pass left, of the last search of a caller that took the candidate pass -- the
 *   seeds level 0 handed on, and, where a second fp16 pass ran (escalation on, k' < 256, at least 4,096 rows), that pass' own output.  A floor
 *   that is too high loses rows the second pass would have needed, its list does not fill up and the not-full rule certifies an incomplete
 *   answer -- which no result shows unless the fp32 search disagrees; so the values themselves are handed out.
 *     info  {nq; kc0: k' of level 0; n1: queries of the second pass, 0 when none ran; kc1: its k' (256); klw1: its pools' capacity per query
 *            and slot; centred (0 / 1); n2: queries that reached the fp32 kernel; klw0}
 *   Level 0, valid whether or not a second pass followed:
 *     kth0[nq]             the exact k-th best score among the first pass' candidates (the metric's ordering score: q.b + row init, fp32
 *                          chain) -- the floor of an fp32 search of that query; -inf: no seed (fewer than k candidates, a non-finite norm or bound)
 *     floor0[nq]           kth0 - 1.001 E and a hair, in the pass' units (centred: kth0 - c_q - 1.001 E') -- the floor of the second pass; -inf
 *                          where kth0 is
 *     certified0[nq]       the first certificates, as hb_index_last_screen hands them out
 *   Level 1, n1 > 0 only (the queries of that pass are numbered 0 .. n1 - 1 in the order of queries1):
 *     queries1[n1]         the level-0 query numbers sent to the second pass, ascending
 *     seed1[n1]            what that pass was seeded with, as gathered on the device (not recomputed from floor0)
 *     cand_rows1[n1][kc1], pass_scores1[n1][kc1]   its merged lists, in the units and with the conventions of hb_index_last_screen
 *     certified1[n1]       its certificates (0: the query went on to the fp32 kernel, seeded with kth1)
 *     kth1[n1]             as kth0, over the second pass' candidates
 *   All pointers are HOST pointers and each of the nine arrays may be NULL; a first call with all of them NULL returns the sizes in info.
 *   capacity_queries: the queries kth0 / floor0 / certified0 have room for; capacity_queries1: the same for the level-1 arrays (not looked at
 *   when none of them is asked for).  Synchronises the index's stream; launches nothing.
 *   Fails (hb_last_error says which) on a NULL handle or a NULL info; when the last search did not take the fp16 candidate pass, or
 *   hb_index_reset, hb_index_add or a capacity change came after it; when a capacity is smaller than the count it stands for.
 *   After an EXCLUDING search that the screen served (hb_index_search_excluding with hb_index_set_exclude_screen, hbird_hip_exclude_screen.h) both
 *   read-outs answer as well, the leftover's rungs notwithstanding (they refuse if one of those rungs took the candidate pass itself), and mean:
 *     kth0 / kth1          the k-th best exact score among the ALLOWED candidates of the list (-inf also where fewer than k are allowed);
 *                          floor0 and the second pass' seed rule are formed from it
 *     the lists            unmasked: cand_rows / cand_rows1 hold excluded rows too, and the certificates' threshold is the list's last entry,
 *                          allowed or not; a full list with fewer than k allowed candidates is never certified
 *     n2                   the queries handed to the rungs (hb_index_last_exclusion_seeds names them)
 *   With the record the QUERY side of hb_index_last_fp16_copy (q16, n, level) and of hb_index_last_centre (hbird_hip_centre.h: cq, qcn, q16)
 *   answers behind those rungs too, where it used to refuse once a rung had run: the rungs' fp32 searches write neither the fp16 query tiles
 *   nor the centred pass' per-query values, so both still describe the search's last fp16 pass.
 *
 * hb_index_last_fp16_copy(ix, bank16, q16, info): the PLAIN (uncentred) fp16 copy the pass reads -- one round-to-nearest-even conversion per
 *   component is what the bound's h = 2^-11 assumes, and the overflow flag decides between "certificate valid" and "scores inf / NaN".
 *     info  {rows: rows converted so far; dp16: halves per row of an fp16 tile (D rounded up to 128); n_g = 32 ceil(rows / 32); flag: the device
 *            overflow flag (sticky: some finite |x| > 65504 was converted since the last hb_index_reset); flag_host: its host image, which the
 *            searches decide by; n: queries of the last plain candidate pass, 0 when the query side is not valid; level: 0 = that pass was the
 *            caller's, 1 = the second pass over its uncertified queries (which overwrites the query tiles), -1: not valid;
 *            n_qpad = 256 ceil(n / 256)}
 *     bank16[n_g * dp16]   the raw fp16 tiles of the converted row tiles, as uint16, in the layout stated for hb_index_last_centre
 *                          (hbird_hip_centre.h); rows [rows, n_g) and the components [D, dp16) are zero
 *     q16[n_qpad * dp16]   the raw query tiles of that pass, same layout (the padding queries are zero vectors)
 *   HOST pointers, each may be NULL.  Synchronises the index's stream; launches nothing.
 *   Fails on a NULL handle or a NULL info; while there is no fp16 copy for the bank's capacity (no screened search yet, a capacity change
 *   since, an automatic index that dropped it) or the copy is centred; and, when q16 is asked for, when the last search of a caller did not run
 *   the plain candidate pass or hb_index_add, hb_index_reset or a capacity change came after it. */
#ifndef HBIRD_HIP_SCREEN_H
#define HBIRD_HIP_SCREEN_H
int hb_index_last_screen(hb_index_t* ix, int64_t* cand_rows, float* pass_scores, unsigned char* certified, int64_t capacity_queries, int64_t info[4]);
int hb_index_last_screen_seeds(hb_index_t* ix, float* kth0, float* floor0, unsigned char* certified0, int64_t* queries1, float* seed1, int64_t* cand_rows1, float* pass_scores1, unsigned char* certified1, float* kth1, int64_t capacity_queries, int64_t capacity_queries1, int64_t info[8]);
int hb_index_last_fp16_copy(hb_index_t* ix, uint16_t* bank16, uint16_t* q16, int64_t info[8]);
#endif /* HBIRD_HIP_SCREEN_H */
