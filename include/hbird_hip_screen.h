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
 *   (hb_index_set_fp16_escalation(ix, 1) keeps them); when capacity_queries is smaller than the search's query count. */
#ifndef HBIRD_HIP_SCREEN_H
#define HBIRD_HIP_SCREEN_H
int hb_index_last_screen(hb_index_t* ix, int64_t* cand_rows, float* pass_scores, unsigned char* certified, int64_t capacity_queries, int64_t info[4]);
#endif /* HBIRD_HIP_SCREEN_H */
