/* Part of the C ABI of libhbird_hip.so: image-level k-NN classification (csrc/hbird_vote.hip) -- the weighted vote of DINO / iBOT / DINOv2's
 * k-NN classifier over the neighbour lists a search left, for a whole (k, T) grid out of one list per query, and the integer counts behind
 * top-1 / top-n / mean-per-class accuracy.
 * Stands on its own (no hb_index_t): hbird_hip.h does not include it, hbird_mi/_lib.py binds it as SIGNATURES_VOTE.
 * All pointers are device pointers except where noted (ks, temps: HOST arrays, read before the call returns and passed by value into the
 * launch), work is enqueued on `hip_stream` (NULL: the default stream).  Each entry returns 0, or -1 with hb_last_error set before anything is
 * launched: for a NULL idx, score, labels, pred, ks or temps (hb_knn_vote), a NULL pred, qlabels, counts_io or n_io (hb_vote_counts), ks that are not
 * strictly ascending or start below 1, ks[nk - 1] > k_list, k_list > 2048, nk * nt > HB_VOTE_MAX_CONFIGS, a temperature that is <= 0 or not
 * finite, topn outside [1, HB_VOTE_MAX_TOP], C < 1, n_rows < 0, nq < 0.  nq == 0 is an empty call and returns 0.
 *
 * THE DEFINITIONS BELOW ARE THIS ENGINE'S OWN.  They follow the weighted k-NN classifier of DINO's eval_knn.py as restated from memory, with
 * none of its code at hand; no accuracy of this engine has been held to a published one.
 *
 * hb_knn_vote.  idx [nq][k_list] int64 and score [nq][k_list] fp32 are neighbour lists, best first, as hb_index_search leaves them on an
 *   inner-product index: a larger score is better, positions past the neighbours hold idx -1 and score -inf.  labels [n_rows] int32 holds one
 *   class per bank row, a value in [0, C), or -1 for an unlabelled row.  ks[nk] and temps[nt] span the grid; configuration cfg = ik * nt + it.
 *   Configuration (k, T) looks at the first k POSITIONS of the list, as hb_index_aggregate_grid does: k counts list positions, not labelled
 *   rows, so that every configuration is the vote over the list cut to k columns.  Position j TAKES PART when
 *     idx_j >= 0 and row = idx_j - id_base lies in [0, n_rows), and labels[row] >= 0.
 *   For a position that takes part: logit_j = score_j / T (IEEE fp32 division); mx = the logit of the first position that takes part;
 *   e_j = expf(logit_j - mx).  vote[c] is the chain ((0.0f + e_a) + e_b) + ... over the positions of class c that take part, in ascending j.
 *   DINO's exp(sim / T) is this up to a factor common to all classes of a query.
 *   Ranking covers the classes with at least one position that takes part: vote descending, ties to the LOWER class id.  The first topn go to
 *   pred [n_cfg][nq][topn] int32, their votes to votes_opt [n_cfg][nq][topn] fp32 (or NULL); the tail holds -1 / 0.0f; a query with nothing
 *   taking part gets all -1.
 *   Consequences: no floating-point atomic -- two calls give the same bits.  For one T the chain of a smaller k is a prefix of the chain of a
 *   larger k: one sweep over the list serves every k, and each configuration has the bits of a call of its own on the list cut to k columns.
 *   HB_VOTE_MAX_CLASSES: there is NO LIMIT on C beyond int32.  The votes are gathered by a leader scan over the <= 2048 list positions (the
 *   first position of a class collects that class), not in per-class bins, so nothing is sized by C; the macro states the largest C accepted.
 *   C is not otherwise read: a label >= C takes part under its own value.
 *
 * hb_vote_counts.  pred [n_cfg][nq][topn] int32 as hb_knn_vote wrote it, qlabels [nq] int32, -1 = the query is counted nowhere.
 *   ACCUMULATES (the caller zeroes the tables once and calls once per batch):
 *     counts_io [n_cfg][topn] int64: slot t += 1 when the query's label is among pred[cfg][q][0 .. t];
 *     class_io_opt [n_cfg][C][2] int64 or NULL: [c][0] += 1 per labelled query of class c, [c][1] += 1 when its pred[cfg][q][0] == c;
 *     n_io [1] int64 += the number of labelled queries.
 *   Integer atomics: the counts are the same every call.  A query label >= C (or < -1) is refused: one small flag launch and a read of the
 *   flag before anything is counted -- the entry synchronises the stream for it. */
#ifndef HBIRD_HIP_VOTE_H
#define HBIRD_HIP_VOTE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define HB_VOTE_MAX_CONFIGS 16
#define HB_VOTE_MAX_TOP 8
#define HB_VOTE_MAX_K 2048
#define HB_VOTE_MAX_CLASSES 2147483647
int hb_knn_vote(const int64_t* idx, const float* score, int64_t nq, int k_list, int64_t id_base, const int32_t* labels, int64_t n_rows, int C,
                const int* ks, int nk, const float* temps, int nt, int topn, int32_t* pred, float* votes_opt, void* hip_stream);
int hb_vote_counts(const int32_t* pred, const int32_t* qlabels, int64_t nq, int n_cfg, int topn, int C, int64_t* counts_io,
                   int64_t* class_io_opt, int64_t* n_io, void* hip_stream);
#ifdef __cplusplus
}
#endif
#endif /* HBIRD_HIP_VOTE_H */
