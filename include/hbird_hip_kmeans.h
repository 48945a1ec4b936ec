/* Part of the C ABI of libhbird_hip.so: k-means over the resident bank (csrc/hbird_kmeans.hip), the clustering of the overclustering protocol.
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t is declared); not meant to be included on its own.
 *
 * Lloyd's iteration on the bank's stored rows x[r] (what hb_index_reconstruct returns: normalised rows for a bank added with normalize = 1).
 *
 * Assignment.  a[r] is the id that hb_index_search(cent, x[r], k = 1) returns on an HB_METRIC_L2 index `cent` of the K centroids (added with
 *   normalize = 0, hb_index_set_fp16(cent, 0)): the nearest centroid under the engine's bit-defined scores, the lower id on ties, -1 for a row
 *   with a non-finite component; d[r] is the distance that search returns.  The rows reach `cent` as ordinary queries, in chunks copied from
 *   the bank's tiles to a row-major staging buffer; the result does not depend on the chunking.
 * Update, in exact integers.  Q(x) = llrint(x * 2^30), round-half-even of the exact double product.  S[c][j] = sum over the rows with
 *   a[r] == c of Q(x[r][j]) in int64, n[c] their count.  The new centroid is (float)((double)S[c][j] / ((double)n[c] * 2^30)): within 2^-31
 *   of the true mean before its one fp32 rounding.  A cluster with n[c] == 0 keeps its previous centroid and counts as empty.  Integer sums
 *   do not depend on order, chunking or partition: the same bits every run.  A row with a[r] >= 0 and a component outside [-2, 2] (or an
 *   a[r] >= K) fails the call: k-means here is for normalised banks, and 2^31 rows then keep |S| within 2^62.
 *
 * hb_kmeans_assign(bank, cent, row0, n, chunk_rows, assign, dist_opt): a[r], d[r] for the bank's rows row0 .. row0 + n - 1 into assign[0 .. n) and,
 *   unless NULL, dist_opt[0 .. n).  chunk_rows: rows per staging chunk, 0 = automatic (at most 131,072).  `cent` must be an L2 index of the
 *   bank's width on the bank's device; it is searched on the bank's stream.
 * hb_kmeans_accumulate(bank, assign, row0, n, K, sums, counts): sums[c][j] += Q(x[row0 + i][j]), counts[c] += 1 for every i in [0, n) with
 *   c = assign[i] >= 0.  sums [K][d] and counts [K] are ADDED to: calls over split row ranges equal one call.  Synchronises the bank's stream
 *   and fails (after the adds of the rows in range were made) when a row was out of range.
 * hb_kmeans_centroids(sums, counts, K, d, prev, out, n_empty_host, stream): out[c][j] from sums and counts as above, prev[c][j] where
 *   counts[c] == 0 (out may be prev); *n_empty_host (a HOST pointer, may be NULL): the clusters with counts[c] == 0.  Runs on `stream` of the
 *   device that holds `sums` and synchronises it.
 * hb_kmeans_fit(bank, K, init, max_iter, chunk_rows, centroids, counts, assign_opt, history, iters, converged): for it = 1 .. max_iter: assign
 *   with the current centroids (init at it = 1); changed = the rows whose assignment differs from the previous iteration's (at it = 1: the rows
 *   with a >= 0); changed == 0: stop, converged; otherwise update.  On return, converged or not, `centroids` are the update of the returned
 *   assignment (assign_opt[ntotal], may be NULL) and `counts` its n[c].  history[it - 1] (a HOST array [max_iter][4], the rest untouched) =
 *   {changed, empty clusters, unassigned rows, inertia}: exact integers as doubles, and the float64 sum of d[r] over the assigned rows by a
 *   fixed tree (reported only).  *iters: the iterations run; *converged: 0 / 1.  The call creates and frees its own centroid index and
 *   workspace: hb_debug_live_allocations afterwards equals its value before.
 *
 * assign, dist_opt, sums, counts, prev, out, init, centroids, assign_opt are DEVICE pointers on the bank's device; work is enqueued on the
 * bank's stream.  Every entry returns 0, or -1 with hb_last_error set -- before anything is launched for a NULL handle or pointer, K outside
 * [1, HB_KMEANS_MAX_K], K > ntotal (fit), a row range outside the bank, max_iter < 1, or a centroid index of another width, metric or device. */
#ifndef HBIRD_HIP_KMEANS_H
#define HBIRD_HIP_KMEANS_H
#define HB_KMEANS_MAX_K 2048          /* clusters: the [K][8] int64 table of one column group is 128 KiB of LDS at 2048 */
#define HB_KMEANS_CHUNK_ROWS 131072   /* the staging chunk of an assignment, at most, when chunk_rows = 0 */
int hb_kmeans_assign(hb_index_t* bank, hb_index_t* cent, int64_t row0, int64_t n, int64_t chunk_rows, int32_t* assign, float* dist_opt);
int hb_kmeans_accumulate(hb_index_t* bank, const int32_t* assign, int64_t row0, int64_t n, int K, int64_t* sums, int64_t* counts);
int hb_kmeans_centroids(const int64_t* sums, const int64_t* counts, int K, int d, const float* prev, float* out, int64_t* n_empty_host,
                        void* stream);
int hb_kmeans_fit(hb_index_t* bank, int K, const float* init, int max_iter, int64_t chunk_rows, float* centroids, int64_t* counts,
                  int32_t* assign_opt, double* history, int* iters, int* converged);
#endif /* HBIRD_HIP_KMEANS_H */
