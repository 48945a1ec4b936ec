"""ctypes binding of lib/libhbird_hip.so (C ABI: include/hbird_hip.h).

This is the only way the Python side reaches the HIP kernels.  There is no CPU fallback: if the
shared library is missing, or no GPU is visible when an index is created, the call fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("HBIRD_HIP_LIB") or os.path.join(_PKG_ROOT, "lib", "libhbird_hip.so")   # override: A/B builds
CSRC_DIR = os.path.join(_PKG_ROOT, "csrc")

_lib = None

# name -> (restype, argtypes); mirrors include/hbird_hip.h one to one
SIGNATURES = {
    "hb_last_error": (c_char_p, []),
    "hb_device_count": (c_int, [POINTER(c_int)]),
    "hb_index_create": (c_int, [c_int, c_int, c_int, POINTER(c_void_p)]),
    "hb_index_free": (c_int, [c_void_p]),
    "hb_index_set_stream": (c_int, [c_void_p, c_void_p]),
    "hb_index_reserve": (c_int, [c_void_p, c_int64]),
    "hb_index_add": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int]),
    "hb_index_add_labels": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int]),
    "hb_index_ntotal": (c_int64, [c_void_p]),
    "hb_index_nlabels": (c_int64, [c_void_p]),
    "hb_index_reset": (c_int, [c_void_p]),
    "hb_index_search": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_int]),
    "hb_index_search_aggregate": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_float, c_void_p, c_void_p,
                                          c_void_p, c_int]),
    "hb_index_aggregate": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, c_float,
                                   c_void_p, c_int]),
    "hb_index_aggregate_partial": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, c_float, c_void_p, c_int64,
                                           c_void_p]),
    "hb_index_reconstruct": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int]),
    "hb_index_gather_labels": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int]),
    "hb_index_set_label_table": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64]),
    "hb_index_copy_norms": (c_int, [c_void_p, c_void_p, c_int]),
    "hb_index_set_score_output": (c_int, [c_void_p, c_int]),
    "hb_index_distances_from_scores": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "hb_merge_topk": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hb_packed_list_bytes": (c_int64, [c_int64, c_int]),
    "hb_merge_topk_packed": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    # k beyond 256 (K5: csrc/hbird_aggregate.hip, merges: csrc/hbird_bigk.hip): the argument lists of their hb_index_* / hb_merge_* counterparts
    "hb_bigk_search_aggregate": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_float, c_void_p, c_void_p,
                                         c_void_p, c_int]),
    "hb_bigk_aggregate": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, c_float,
                                  c_void_p, c_int]),
    "hb_bigk_aggregate_partial": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, c_float, c_void_p, c_int64,
                                          c_void_p]),
    "hb_bigk_merge_topk": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hb_bigk_merge_topk_packed": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hb_multi_create": (c_int, [c_int, c_int, POINTER(c_int), c_int, c_int, POINTER(c_void_p)]),
    "hb_multi_free": (c_int, [c_void_p]),
    "hb_multi_reserve": (c_int, [c_void_p, c_int64]),
    "hb_multi_add": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
    "hb_multi_ntotal": (c_int64, [c_void_p]),
    "hb_multi_shard_rows": (c_int, [c_void_p, POINTER(c_int64), c_int]),
    "hb_multi_set_fp16": (c_int, [c_void_p, c_int]),
    "hb_multi_search": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "hb_normalize_rows": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "hb_patch_label_hist": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hb_patch_scores": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hb_patch_select": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p,
                                c_void_p]),
    "hb_gather_rows": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "hb_upsample_argmax": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hb_upsample_argmax_confusion": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int64, c_int,
                                             c_void_p, c_void_p, c_void_p]),
    "hb_upsample_accumulate": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "hb_argmax_channels": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "hb_confusion_update": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "hb_index_set_timing": (c_int, [c_void_p, c_int]),
    "hb_index_last_knn_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "hb_index_set_tuning": (c_int, [c_void_p, c_int, c_int]),
    "hb_index_set_fp16": (c_int, [c_void_p, c_int]),
    "hb_index_last_fp16_fallbacks": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_last_search_path": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "hb_index_set_fp16_escalation": (c_int, [c_void_p, c_int]),
    "hb_index_last_fp16_escalated": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_schedule_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, POINTER(c_int64)]),
    "hb_schedule_plan_phased": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, POINTER(c_int64),
                                        c_void_p, c_int, POINTER(c_int), c_void_p]),
    "hb_schedule_plan_shared": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, POINTER(c_int64)]),
    "hb_schedule_plan_filled": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int64,
                                        POINTER(c_int64), c_void_p, c_int, POINTER(c_int), c_void_p]),
    "hb_last_schedule_fill": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_index_set_cluster": (c_int, [c_void_p, c_int, c_int, c_int]),
    "hb_index_set_cluster_sharing": (c_int, [c_void_p, c_int]),
    "hb_index_set_label_denominator": (c_int, [c_void_p, c_int]),
    "hb_index_labels_to_fp32": (c_int, [c_void_p]),
    "hb_index_label_denominator": (c_int, [c_void_p, POINTER(c_int)]),
    "hb_index_copy_label_counts": (c_int, [c_void_p, c_void_p, c_int]),
    "hb_index_set_label_count_table": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64]),
    "hb_index_cluster_stats": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_index_set_variant": (c_int, [c_void_p, c_int]),
    "hb_index_set_search_options": (c_int, [c_void_p, c_int, c_int64]),
    "hb_index_wg_stamps": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_int)]),
    "hb_index_set_xcd_weights": (c_int, [c_void_p, c_int, POINTER(c_double)]),
    "hb_index_xcd_weights": (c_int, [c_void_p, c_int, POINTER(c_double), POINTER(c_int)]),
    "hb_schedule_plan_weighted": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_double), c_void_p, c_int64, POINTER(c_int64)]),
    "hb_index_kernel_clock": (c_int, [c_void_p, POINTER(c_double)]),
    "hb_index_xcd_stats": (c_int, [c_void_p, c_int, POINTER(c_double)]),
    "hb_debug_live_allocations": (c_int, [POINTER(c_int64), POINTER(c_int64)]),
    "hb_calibration_new": (c_void_p, [c_int]),
    "hb_calibration_free": (None, [c_void_p]),
    "hb_calibration_state": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    "hb_calibration_feed": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_double), POINTER(c_int), c_int, c_double]),
    "hb_f16_adapt_replay": (c_int, [c_int, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int)]),
    "hb_exact_screen_replay": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int, c_int64, c_int, c_int, c_int,
                                       c_uint64, c_uint64, c_uint64, c_uint64, POINTER(c_int)]),
    "hb_rerank_copy_replay": (c_int, [c_int, c_uint64, c_uint64, c_uint64, c_uint64]),
    "hb_knn_plan_replay": (c_int, [POINTER(c_int64), c_int, POINTER(c_int64), c_int]),
    "hb_certificate_bound_replay": (c_int, [POINTER(c_double), c_int, POINTER(c_double), c_int]),
    "hb_set_layout_form": (c_int, [c_int]),
    "hb_index_set_rerank_copy": (c_int, [c_void_p, c_int]),
    "hb_index_rerank_copy_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_index_schedule_info": (c_int, [c_void_p, POINTER(c_int64)]),
}

# ... and include/hbird_hip_centre.h (the mean-centred form of the fp16 copy), which hbird_hip.h includes
SIGNATURES_CENTRE = {
    "hb_index_set_fp16_centre": (c_int, [c_void_p, c_int]),
    "hb_index_fp16_centre_info": (c_int, [c_void_p, POINTER(c_double)]),
    "hb_multi_set_fp16_centre": (c_int, [c_void_p, c_int]),
    "hb_index_last_centre": (c_int, [c_void_p] + [c_void_p] * 8 + [POINTER(c_int64)]),
}

# ... and include/hbird_hip_select.h (sub-bank views, csrc/hbird_select.hip: rows of one index gathered into another on the device)
SIGNATURES_SELECT = {
    "hb_index_add_from": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int]),
    "hb_index_select_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_void_p)]),
}

# ... and include/hbird_hip_grid.h (evaluation grids, csrc/hbird_grid.hip: every (k, beta) of a grid aggregated from one neighbour list per query)
GRID_MAX_CONFIGS = 16      # HB_GRID_MAX_CONFIGS
SIGNATURES_GRID = {
    "hb_index_aggregate_grid": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, POINTER(c_int), c_int,
                                        POINTER(c_float), c_int, c_void_p, c_int]),
    "hb_index_search_aggregate_grid": (c_int, [c_void_p, c_void_p, c_int64, c_int64, POINTER(c_int), c_int, POINTER(c_float), c_int,
                                               c_void_p, c_void_p, c_void_p, c_int]),
}

# ... and include/hbird_hip_exclude.h (searches that exclude one row group per query, csrc/hbird_exclude.hip: leave-one-image-out evaluation)
SIGNATURES_EXCLUDE = {
    "hb_index_set_row_groups": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int]),
    "hb_index_search_excluding": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int]),
    "hb_exclude_filter": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "hb_index_last_exclusion": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_exclude_plan_replay": (c_int, [c_int, c_int64, POINTER(c_int), c_int]),
}

# ... and include/hbird_hip_screen.h (the read-out of the fp16 screen's last candidate pass: lists, pass scores, first certificates)
SIGNATURES_SCREEN = {
    "hb_index_last_screen": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int64)]),
    # ... the seeds level 0 handed on and the second pass' output; the plain fp16 copy with its overflow flag
    "hb_index_last_screen_seeds": (c_int, [c_void_p] + [c_void_p] * 9 + [c_int64, c_int64, POINTER(c_int64)]),
    "hb_index_last_fp16_copy": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
}

# ... and include/hbird_hip_exclude_screen.h (excluding searches served by the fp16 screen, csrc/hbird_exclude_screen.hip)
EXCL_SCREEN_REASONS = {0: "served", 1: "off", 2: "k", 3: "need", 4: "path", 5: "empty"}      # HB_EXCL_SCREEN_*
SIGNATURES_EXCLUDE_SCREEN = {
    "hb_index_set_exclude_screen": (c_int, [c_void_p, c_int]),
    "hb_index_last_exclusion_screen": (c_int, [c_void_p, POINTER(c_int64)]),
    "hb_index_exclude_rerank": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "hb_index_last_exclusion_seeds": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, POINTER(c_int64)]),
}

# ... and include/hbird_hip_bootstrap.h (paired bootstrap over images for mIoU grids, csrc/hbird_bootstrap.hip); a header of its own, not
# included by hbird_hip.h
BOOTSTRAP_MAX_IMAGES = 32768          # HB_BOOTSTRAP_MAX_IMAGES
BOOTSTRAP_MAX_REPLICATES = 1 << 20    # HB_BOOTSTRAP_MAX_REPLICATES
SIGNATURES_BOOTSTRAP = {
    "hb_image_class_counts": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "hb_bootstrap_multiplicities": (c_int, [c_int, c_uint64, c_int64, c_int64, c_void_p, c_void_p]),
    "hb_bootstrap_counts": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "hb_bootstrap_miou": (c_int, [c_void_p, c_int, c_int, c_int, c_uint64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
}

# ... and include/hbird_hip_kmeans.h (k-means over the resident bank, csrc/hbird_kmeans.hip: the clustering of the overclustering protocol), which
# hbird_hip.h includes
KMEANS_MAX_K = 2048              # HB_KMEANS_MAX_K
KMEANS_CHUNK_ROWS = 131072       # HB_KMEANS_CHUNK_ROWS
SIGNATURES_KMEANS = {
    "hb_kmeans_assign": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "hb_kmeans_accumulate": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "hb_kmeans_centroids": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, POINTER(c_int64), c_void_p]),
    "hb_kmeans_fit": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_double), POINTER(c_int),
                              POINTER(c_int)]),
}

# ... and include/hbird_hip_linprobe.h (the linear probe, csrc/hbird_linprobe.hip: a softmax segmentation head's logits, loss and gradient over
# the resident bank), which hbird_hip.h includes
LINPROBE_MAX_C = 256             # HB_LINPROBE_MAX_C
LINPROBE_MAX_SEGS = 512          # HB_LINPROBE_MAX_SEGS
SIGNATURES_LINPROBE = {
    "hb_linprobe_partition": (c_int, [c_int64, POINTER(c_int64), POINTER(c_int)]),
    "hb_linprobe_logits": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "hb_linprobe_loss_grad": (c_int, [c_void_p, c_void_p, c_int, c_double, POINTER(c_double), c_void_p, POINTER(c_int64), c_void_p]),
    "hb_linprobe_set_workspace": (c_int, [c_int64]),
}

# ... and include/hbird_hip_depth.h (depth estimation by retrieval, csrc/hbird_depth.hip: depth maps to patch label rows, aggregated rows to a
# depth map and per-image error sums), which hbird_hip.h includes
DEPTH_NSUMS = 11                 # HB_DEPTH_NSUMS
DEPTH_SUMS = ("n", "n_nopred", "sq", "abs_rel", "sq_rel", "log_sq", "log", "log10", "d1", "d2", "d3")      # HB_DEPTH_SUM_*: the slots in order
DEPTH_MAX_PS = 64                # HB_DEPTH_MAX_PS
DEPTH_MAX_GRID = 4096            # HB_DEPTH_MAX_GRID
SIGNATURES_DEPTH = {
    "hb_patch_depth_targets": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "hb_depth_upsample_metrics": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p]),
}

# ... and include/hbird_hip_depth_grid.h (depth grids, csrc/hbird_depth_grid.hip: the depth metrics of a whole (k, beta) grid out of one call, the
# resampling reduction of the paired bootstrap over float64 per-image sums); a header of its own, not included by hbird_hip.h
DEPTH_GRID_MAX_CONFIGS = 16      # HB_DEPTH_GRID_MAX_CONFIGS
SIGNATURES_DEPTH_GRID = {
    "hb_depth_upsample_metrics_grid": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p,
                                               c_void_p]),
    "hb_bootstrap_weighted_sums": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
}

# ... and include/hbird_hip_propagate.h (video label propagation, csrc/hbird_propagate.hip and csrc/hbird_maskmetrics.hip: windowed retrieval over a
# pool of context frames, the label map of a rectangular frame, the counts behind J and F); a header of its own, not included by hbird_hip.h
PROPAGATE_MAX_K = 32             # HB_PROPAGATE_MAX_K
PROPAGATE_MAX_CTX = 32           # HB_PROPAGATE_MAX_CTX
PROPAGATE_MAX_C = 64             # HB_PROPAGATE_MAX_C
PROPAGATE_MAX_D = 1024           # HB_PROPAGATE_MAX_D
JF_MAX_BOUND = 32                # HB_JF_MAX_BOUND
JF_COUNTS = ("inter", "union", "nfg", "ngt", "fg_match", "gt_match")      # HB_JF_*: the slots in order
SIGNATURES_PROPAGATE = {
    "hb_propagate_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hb_mask_upsample_argmax": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hb_mask_jf_counts": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}

# ... and include/hbird_hip_vote.h (image-level k-NN classification, csrc/hbird_vote.hip: the weighted vote of a (k, T) grid over one neighbour list
# per query, the counts behind top-1 / top-n / mean-per-class accuracy); a header of its own, not included by hbird_hip.h
VOTE_MAX_CONFIGS = 16            # HB_VOTE_MAX_CONFIGS
VOTE_MAX_TOP = 8                 # HB_VOTE_MAX_TOP
VOTE_MAX_K = 2048                # HB_VOTE_MAX_K
VOTE_MAX_CLASSES = 2147483647    # HB_VOTE_MAX_CLASSES: no limit beyond int32 (a leader scan, no per-class bins)
SIGNATURES_VOTE = {
    "hb_knn_vote": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_int, POINTER(c_int), c_int, POINTER(c_float), c_int,
                            c_int, c_void_p, c_void_p, c_void_p]),
    "hb_vote_counts": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# ... and include/hbird_hip_linprobe_class.h (the image-level linear probe, csrc/hbird_linprobe_class.hip: a softmax head's logits, loss and gradient
# on one class id per bank row for 1000 classes and more, the top-n of a logit table), which hbird_hip.h includes
LINPROBE_CLASS_MAX_C = 16384     # HB_LINPROBE_CLASS_MAX_C: the largest C accepted; nothing is sized by it
SIGNATURES_LINPROBE_CLASS = {
    "hb_linprobe_class_logits": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "hb_linprobe_class_loss_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, POINTER(c_double), c_void_p, POINTER(c_int64), c_void_p]),
    "hb_logits_topn": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
}


class HbirdHipError(RuntimeError):
    pass


class HbirdClassRangeError(HbirdHipError, ValueError):
    """A mask holds a class id outside [0, num_classes): F.one_hot of the reference raises for it (hbird_eval.py:319)."""


def lib() -> ctypes.CDLL:
    """Load libhbird_hip.so (built by __graft_entry__.build() / `make -C csrc`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HbirdHipError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                f"g.build()' or make -C {CSRC_DIR}). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        # HBIRD_PLAN_ONLY=1 (tests/test_sanitizers_cpu.py): LIB_PATH names the host-only sanitizer build of the work-list planner,
        # which exports the hb_schedule_plan* / hb_calibration_* entry points and hb_last_error only
        plan_only = os.environ.get("HBIRD_PLAN_ONLY") == "1"
        for name, (res, args) in list(SIGNATURES.items()) + list(SIGNATURES_CENTRE.items()) + list(SIGNATURES_SELECT.items()) + list(SIGNATURES_GRID.items()) + list(SIGNATURES_EXCLUDE.items()) + list(SIGNATURES_SCREEN.items()) + list(SIGNATURES_EXCLUDE_SCREEN.items()) + list(SIGNATURES_BOOTSTRAP.items()) + list(SIGNATURES_KMEANS.items()) + list(SIGNATURES_LINPROBE.items()) + list(SIGNATURES_DEPTH.items()) + list(SIGNATURES_DEPTH_GRID.items()) + list(SIGNATURES_PROPAGATE.items()) + list(SIGNATURES_VOTE.items()) + list(SIGNATURES_LINPROBE_CLASS.items()):
            if plan_only and not (name.startswith("hb_schedule_plan") or name.startswith("hb_calibration_") or name in ("hb_f16_adapt_replay", "hb_exact_screen_replay", "hb_rerank_copy_replay", "hb_knn_plan_replay", "hb_certificate_bound_replay", "hb_exclude_plan_replay") or name == "hb_last_error"):
                continue
            fn = getattr(L, name)  # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    msg = lib().hb_last_error()
    return msg.decode() if msg else ""


def check(rc: int, exc=HbirdHipError):
    if rc != 0:
        raise exc(last_error() or f"libhbird_hip call failed with status {rc}")


def device_count() -> int:
    n = c_int(0)
    lib().hb_device_count(ctypes.byref(n))
    return int(n.value)
