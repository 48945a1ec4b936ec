/* Part of the C ABI of libhbird_hip.so: evaluation grids (csrc/hbird_grid.hip).
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t is declared); not meant to be included on its own.
 *
 * The label aggregation of a whole grid of (k, beta) configurations out of ONE neighbour list per query.  A search returns the exact top-k
 * under one total order (score descending, id ascending) with deterministic score bits, so the best k of a query are the first k entries of
 * its best k_max, bit for bit: one search at the largest k serves every smaller k, and beta only enters after the search.
 * ks[nk] (host array) strictly ascending with 1 <= ks[0] and ks[nk - 1] <= k_list <= HB_MAX_K_AGGREGATE; betas[nb] (host array) finite and
 * > 0; nk * nb <= HB_GRID_MAX_CONFIGS.  out[cfg][nq][c] with cfg = ik * nb + ib: every configuration's label_hat is a contiguous [nq, c] slab.
 * Configuration (k, beta) is hb_index_aggregate applied to the first k POSITIONS of the list (row stride k_list), whatever they hold -- -1
 * entries, ids outside the norm table, repeated ids -- and has its bits; the label tables are chosen as hb_index_aggregate chooses them.
 * One launch gathers every label row once for all configurations.
 * hb_index_aggregate_grid: q, idx, dist, out are device pointers (io_on_device must be 1), as for hb_index_aggregate.
 * hb_index_search_aggregate_grid: ONE search at ks[nk - 1] -- exactly what hb_index_search_aggregate launches for that k (automatic fp16
 * state, hb_last_search_path and the counters behave as for that call) -- followed by the grid launch; out_idx_opt / out_dist_opt
 * [nq, ks[nk - 1]] may be NULL.
 * A bad grid (unordered or repeated ks, ks[nk - 1] > 256 or > k_list, more than HB_GRID_MAX_CONFIGS configurations, a beta that is not
 * finite and positive) and missing label rows fail with hb_last_error set before anything is launched. */
#ifndef HBIRD_HIP_GRID_H
#define HBIRD_HIP_GRID_H
#define HB_GRID_MAX_CONFIGS 16
int hb_index_aggregate_grid(hb_index_t* ix, const float* q, int64_t nq, const int64_t* idx, const float* dist, int k_list,
                            int64_t id_base, const int* ks, int nk, const float* betas, int nb, float* out, int io_on_device);
int hb_index_search_aggregate_grid(hb_index_t* ix, const float* q, int64_t nq, int64_t id_base, const int* ks, int nk,
                                   const float* betas, int nb, float* out, int64_t* out_idx_opt, float* out_dist_opt,
                                   int io_on_device);
#endif /* HBIRD_HIP_GRID_H */
